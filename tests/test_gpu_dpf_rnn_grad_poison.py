"""The RNN resampler's backward pass under hostile LDS leftovers (-m gpu, MI355X).

pf_rnn_backward launches four kernels that stage through LDS: the recording recurrence and the
assignment of the forward pass, k_rnn_bwd_assign (its row reduction) and k_rnn_bwd_recur, which copies
the history of every step into LDS, writes the slot deltas there and, resident, keeps both sets of
weight fragments there.  With PF_TEST_HOOKS=1 and PF_TEST_LDS_POISON=1 each of the four is preceded by
k_lds_poison, which fills the LDS of every CU with a NaN pattern (tests/test_gpu_lds_poison.py checks
the mechanism): a kernel that reads a word it did not write turns its output into NaN.  The runs must
be finite and bitwise the clean runs, and the hook must have fired exactly four times.
"""

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from tests import dpf_rnn_grad_restatement as G
from tests import dpf_rnn_restatement as R
from tests import test_gpu_dpf_rnn_grad as TG

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c,stream", [
    (R.case(17, 2, 5, 2, "gru", seed=21), False),   # a tile and one row; padded units 5..15; two layers
    (R.case(33, 1, 24, 1, "lstm", seed=22), True),  # three tiles, two waves, weights streamed
    (R.case(16, 1, 128, 1, "gru", seed=23, res=False), False),  # 512 lanes; streams on its own
    (R.case(17, 1, 8, 4, "gru", seed=24), False),   # four layers resident
], ids=["N17-H5-L2-gru", "N33-H24-L1-lstm-streamed", "N16-H128-L1-gru", "N17-H8-L4-gru"])
def test_rnn_backward_poisoned(c, stream, monkeypatch):
    X, lw, W, gXo, gA, ref = G.solved(c)
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    monkeypatch.delenv("PF_TEST_RNN_STREAM", raising=False)
    if stream:  # the variant is fixed when the handle is made, in the clean run as well
        monkeypatch.setenv("PF_TEST_HOOKS", "1")
        monkeypatch.setenv("PF_TEST_RNN_STREAM", "1")
    lib = NV.load()
    c0 = lib.pf_test_lds_poison_count()
    clean = TG.device(c, X, lw, W, gXo, gA)
    assert lib.pf_test_lds_poison_count() == c0
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_LDS_POISON", "1")
    got = TG.device(c, X, lw, W, gXo, gA)
    assert lib.pf_test_lds_poison_count() == c0 + 4, "one poison per LDS-staging launch of pf_rnn_backward"
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    assert all(np.all(np.isfinite(a)) for a in got)
    assert TG.same_bits(got, clean)
    TG.compare(R.case_id(c) + " poisoned", got, [ref[2], ref[3]] + list(ref[4]), c["L"])
