"""The soft resampler's kernels under hostile LDS leftovers (-m gpu, MI355X).

k_soft_pass and k_soft_entropy stage tiles of 64 sources through LDS, the last one partial.  With
PF_TEST_HOOKS=1 and PF_TEST_LDS_POISON=1 every launch of the two is preceded by k_lds_poison, which
fills the LDS of every CU with a NaN pattern (tests/test_gpu_lds_poison.py checks the mechanism): a
kernel that reads a word it did not write turns its output into NaN.  The runs must be finite and
bitwise the clean runs, and the hook must have fired.
"""

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from tests import dpf_soft_restatement as R
from tests import test_gpu_dpf_soft as TS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,d,splits", [
    (300, 17, "1"),   # unsplit: tiles 64 x 4 + 44, a last component chunk of one of 16
    (130, 3, None),   # splits of 32 and a last one of 2 sources; 3 of 4 components staged
    (300, 40, "2"),   # splits of 160 and 140: tiles 64 + 64 + 32 / 12, then a merge
])
def test_soft_resampler_poisoned(N, d, splits, monkeypatch):
    X, lw = R.make_case(N, d, seed=1)
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    monkeypatch.delenv("PF_TEST_SOFT_SPLITS", raising=False)
    if splits is not None:  # the split is fixed when the handle is made, in the clean run as well
        monkeypatch.setenv("PF_TEST_HOOKS", "1")
        monkeypatch.setenv("PF_TEST_SOFT_SPLITS", splits)
    lib = NV.load()
    c0 = lib.pf_test_lds_poison_count()
    ref, Href = TS.device(X, lw, 0.1, 0.2, 3, 1)
    assert lib.pf_test_lds_poison_count() == c0
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_LDS_POISON", "1")
    got, Hgot = TS.device(X, lw, 0.1, 0.2, 3, 1)
    assert lib.pf_test_lds_poison_count() == c0 + 2, "one poison per LDS-staging launch: the pass and the entropy pass"
    got_x, none = TS.device(X, lw, 0.1, 0.2, 3, 1, want_entropy=False)
    assert lib.pf_test_lds_poison_count() == c0 + 3 and none is None
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(Hgot))
    assert np.array_equal(got, ref) and np.array_equal(Hgot, Href) and np.array_equal(got_x, ref)
