"""The OT resampler's backward pass under hostile LDS leftovers (-m gpu, MI355X).

With PF_TEST_HOOKS=1 and PF_TEST_LDS_POISON=1 every launch that stages through LDS is preceded by
k_lds_poison, which fills the LDS of every CU with a NaN pattern (tests/test_gpu_lds_poison.py checks
the mechanism): a kernel that reads a word it did not write turns its output into NaN.  At
(N, d, B) = (130, 17, 2) - five source splits of 32 and a last one of 2, two component chunks with
1 of 16 components staged in the second - and K = 5 iterations (tol = 0: none stops early) the run
must be finite and bitwise the clean run, with the saved history and without.

The LDS-staging launches of one pf_ot_backward with a history of K iterations are 5 + K: k_ot_prepare
and k_ot_cost (the cost matrix again), k_ot_bwd_q, K times k_ot_bwd_cols<true> (the f passes), the
cost's backward (one poison in front of its row and column launches) and k_ot_bwd_weights: 10 here.
Without a history the replay adds K launches of k_ot_tau_cols, 15, and sinkhorn_ot_resample_vjp
first runs a forward pass, 2 + 2 K + 1 = 13 (prepare, cost, tau_cols and check per iteration, project):
28 in all.
"""

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_ot as OT
from tests import dpf_ot_restatement as R

pytestmark = pytest.mark.gpu


def test_ot_backward_poisoned(monkeypatch):
    N, d, B, K = 130, 17, 2, 5
    cases = [R.make_case(N, d, seed=1 + b) for b in range(B)]
    X, w = np.stack([x for x, _ in cases]), np.stack([v for _, v in cases])
    g = np.random.default_rng([N, d, B]).standard_normal((B, N, d))
    args = (X, w, g, 2.0, K, 1e-12, 0.0)
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    monkeypatch.delenv("PF_TEST_OT_SPLITS", raising=False)
    lib = NV.load()
    c0 = lib.pf_test_lds_poison_count()
    saved = OT.sinkhorn_ot_resample(X, w, 2.0, K, 1e-12, 0.0, return_saved=True)[2]
    assert [int(k) for k in saved.iterations] == [K, K]
    ref = OT.sinkhorn_ot_resample_vjp(*args, saved=saved)
    assert lib.pf_test_lds_poison_count() == c0
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_LDS_POISON", "1")
    got = OT.sinkhorn_ot_resample_vjp(*args, saved=saved)
    assert lib.pf_test_lds_poison_count() == c0 + 10, "5 + K LDS-staging launches with a history"
    null = OT.sinkhorn_ot_resample_vjp(*args)
    assert lib.pf_test_lds_poison_count() == c0 + 10 + 28, "the forward's 13 and 5 + 2 K of the backward"
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    for out in (got, null):
        assert np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[1]))
        assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])
    assert np.max(np.abs(ref[0])) > 0.0 and np.max(np.abs(ref[1])) > 0.0
