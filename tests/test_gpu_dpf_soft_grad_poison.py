"""The soft resampler's backward pass under hostile LDS leftovers (-m gpu, MI355X).

k_soft_bwd_pass stages tiles of 64 rows (gX'_i, r_i, M_i, 1 / L_i) through LDS, the last one partial;
it is the only launch of the backward pass that uses LDS.  With PF_TEST_HOOKS=1 and
PF_TEST_LDS_POISON=1 it is preceded by k_lds_poison, which fills the LDS of every CU with a NaN
pattern (tests/test_gpu_lds_poison.py checks the mechanism): a kernel that reads a word it did not
write turns its output into NaN.  At (N, d, B) = (130, 17, 2) - splits of 32 rows and a last one of
2, two component chunks with 1 of 16 components staged in the second - the run must be finite and
bitwise the clean run.  The hook fires once with the forward pass's saved results, and twice without
them: the call then runs the forward's k_soft_pass first.
"""

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from tests import dpf_soft_restatement as R
from tests import test_gpu_dpf_soft_grad as TG

pytestmark = pytest.mark.gpu


def test_soft_backward_poisoned(monkeypatch):
    N, d, B = 130, 17, 2
    cases = [R.make_case(N, d, seed=1 + b) for b in range(B)]
    X, lw = np.stack([x for x, _ in cases]), np.stack([w for _, w in cases])
    g = np.random.default_rng([N, d, B]).standard_normal((B, N, d))
    args = (X, lw, g, 0.1, 0.2, 3, 1)
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    monkeypatch.delenv("PF_TEST_SOFT_SPLITS", raising=False)
    lib = NV.load()
    c0 = lib.pf_test_lds_poison_count()
    saved = TG.fresh(TG.forward, X, lw, 0.1, 0.2, 3, 1)
    ref = TG.fresh(TG.backward, *args, saved=saved)
    assert lib.pf_test_lds_poison_count() == c0
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_LDS_POISON", "1")
    got = TG.fresh(TG.backward, *args, saved=saved)
    assert lib.pf_test_lds_poison_count() == c0 + 1, "one poison per LDS-staging launch: the backward's pass"
    null = TG.fresh(TG.backward, *args)
    assert lib.pf_test_lds_poison_count() == c0 + 3, "the forward's pass and the backward's"
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    for out in (got, null):
        assert np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[1]))
        assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])
    assert np.max(np.abs(ref[1])) > 0.0
