"""The RNN resampler's kernels under hostile LDS leftovers (-m gpu, MI355X).

k_rnn_recur keeps the hidden states of both time parities (and, resident, the weight fragments) in
LDS and reads the "previous" state at t = 0 before any step has written it; k_rnn_assign reduces
through LDS.  With PF_TEST_HOOKS=1 and PF_TEST_LDS_POISON=1 every launch of the two is preceded by
k_lds_poison, which fills the LDS of every CU with a NaN pattern (tests/test_gpu_lds_poison.py checks
the mechanism): a kernel that reads a word it did not write turns its output into NaN.  The runs must
be finite and bitwise the clean runs, and the hook must have fired once per LDS-using launch.
"""

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from tests import dpf_rnn_restatement as R
from tests import test_gpu_dpf_rnn as TR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c,stream", [
    (R.case(17, 2, 5, 2, "gru", seed=21), False),   # a tile and one row; padded units 5..15; two layers
    (R.case(33, 1, 24, 1, "lstm", seed=22), True),  # three tiles, two waves, weights streamed
    (R.case(16, 1, 128, 1, "gru", seed=23, res=False), False),  # 512 lanes zeroing the state; streams on its own
    (R.case(17, 1, 8, 4, "gru", seed=24), False),   # four layers resident: eight state blocks
], ids=["N17-H5-L2-gru", "N33-H24-L1-lstm-streamed", "N16-H128-L1-gru", "N17-H8-L4-gru"])
def test_rnn_resampler_poisoned(c, stream, monkeypatch):
    X, lw, W = R.case_inputs(c)
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    monkeypatch.delenv("PF_TEST_RNN_STREAM", raising=False)
    if stream:  # the variant is fixed when the handle is made, in the clean run as well
        monkeypatch.setenv("PF_TEST_HOOKS", "1")
        monkeypatch.setenv("PF_TEST_RNN_STREAM", "1")
    lib = NV.load()
    c0 = lib.pf_test_lds_poison_count()
    clean = TR.device(c, X, lw, W)
    assert lib.pf_test_lds_poison_count() == c0
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_LDS_POISON", "1")
    got = TR.device(c, X, lw, W)
    assert lib.pf_test_lds_poison_count() == c0 + 2, "one poison per LDS-using launch: the recurrence and the assignment"
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    assert all(np.all(np.isfinite(a)) for a in got)
    assert all(np.array_equal(a, b) for a, b in zip(got, clean))
    ref = R.resample(X[0], lw[0], W, c["cell"], c["T"], c["uw"], c["up"])
    TR.compare(R.case_id(c) + " poisoned", got[0][0], got[1][0], got[2][0], ref)
