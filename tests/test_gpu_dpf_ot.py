"""Sinkhorn OT resampler and DPF_OT on the device vs the NumPy restatement (-m gpu, MI355X).

TensorFlow is not available, so there is no fixture of reference outputs: the device is compared
with tests/dpf_ot_restatement.py, the reference's formulas in fp64, which tests/test_dpf_ot_host.py
checks against the literal per-row loop.  The cases are the smallest at which tiles (64 columns, 4
rows per workgroup, 16 cost rows), tails, the three component chunks of d = 40, the source split
and the stopping rule can go wrong.

Bounds (fp64 engine, the 1e-9 x scale bound of the other fp64 flow filters): particles within
1e-9 max(1, max|X_ref|), f and g within 1e-9 max(1, max|f|, max|g|), iteration counts equal.  The
device sums in another order, multiplies by 1 / eps where NumPy divides, and uses the device
library's exp and log; the iteration is a contraction, so this stays at rounding level.  The
conditions that make "equal" well defined (no convergence check within 1e-3 tol of tol, no plan
entry within 1e-12 of the sparsity threshold) are asserted on the CPU in tests/test_dpf_ot_host.py.
"""

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_ot as OT
from tests import dpf_ot_restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert NV.device_count() > 0, "no HIP device visible: -m gpu tests must run on an MI355X"


def device(X, w, eps, n_iters, **kw):
    """(X_out, iterations, history, f, g, plan_stats) of one pf_ot_resample call, batch axis first."""
    X = np.ascontiguousarray(X, dtype=float)
    w = np.ascontiguousarray(w, dtype=float)
    batched = X.ndim == 3
    Xb, wb = (X, w) if batched else (X[None], w[None])
    h = OT._Handle(Xb.shape[1], Xb.shape[2], Xb.shape[0])
    try:
        out, its, hist, f, g, stats = h.resample(Xb, wb, eps, n_iters, kw.get("min_val", 1e-12), kw.get("tol", 1e-6),
                                                 True)
    finally:
        h.close()
    return out, its, hist, f, g, stats


def compare(tag, X, w, eps, n_iters, ref):
    out, its, hist, f, g, stats = device(X, w, eps, n_iters)
    assert np.all(np.isfinite(out))
    sx = max(1.0, float(np.max(np.abs(ref["particles"]))))
    sf = max(1.0, float(np.max(np.abs(ref["f"]))), float(np.max(np.abs(ref["g"]))))
    ex = float(np.max(np.abs(out[0] - ref["particles"])))
    ef = max(float(np.max(np.abs(f[0] - ref["f"]))), float(np.max(np.abs(g[0] - ref["g"]))))
    print(f"OT {tag}: iterations {int(its[0])} (restatement {ref['iterations']}), particle error {ex:.3e} "
          f"(scale {sx:.3g}), dual error {ef:.3e} (scale {sf:.3g})")
    assert int(its[0]) == ref["iterations"]
    assert ex <= TOL * sx
    assert ef <= TOL * sf
    return out, its, hist, f, g, stats


@pytest.mark.parametrize("case", R.FULL)
def test_full_length_runs(case):
    N, d, eps, n_iters, seed = case
    X, w, ref = R.solved(N, d, eps, n_iters, 1.0, 1.0, seed)
    compare(f"full N={N} d={d}", X, w, eps, n_iters, ref)


@pytest.mark.parametrize("n_iters", [0, 1])
def test_zero_and_one_iteration(n_iters):
    X, w, ref = R.solved(65, 1, 0.1, n_iters)
    out, its, hist, f, g, stats = compare(f"N=65 d=1 n_iters={n_iters}", X, w, 0.1, n_iters, ref)
    if n_iters == 0:
        assert not f.any() and not g.any()


@pytest.mark.parametrize("case", R.EARLY)
def test_early_stop(case):
    N, d, eps, scale, conc, seed, stop = case
    X, w, ref = R.solved(N, d, eps, R.EARLY_ITERS, scale, conc, seed)
    assert ref["iterations"] == stop
    out, its, hist, f, g, stats = compare(f"early N={N} d={d}", X, w, eps, R.EARLY_ITERS, ref)
    assert not hist[0, stop:].any()  # nothing ran after the stopping iteration


@pytest.mark.parametrize("kind", R.WEIGHT_KINDS)
def test_weights(kind):
    X, w, ref = R.solved_weights(kind)
    compare(f"weights {kind}", X, w, 0.1, 50, ref)


@pytest.mark.parametrize("case", R.DIAG)
def test_diagnostics(case):
    N, d, eps, n_iters, scale, conc, seed = case
    X, w, ref = R.solved(*case)
    new, nw, dg = OT.sinkhorn_ot_resample(X, w, epsilon=eps, n_iters=n_iters, return_diagnostics=True)
    rd = ref["diagnostics"]
    assert set(dg) == set(rd)
    assert new.dtype == np.float64 and np.array_equal(nw, np.full(N, 1.0 / N))
    assert dg["sinkhorn_iterations"] == rd["sinkhorn_iterations"] and dg["converged"] == rd["converged"]
    assert dg["epsilon"] == eps
    print(f"OT diagnostics N={N} d={d}: ot_distance {dg['ot_distance']:.15g} vs {rd['ot_distance']:.15g}")
    assert dg["ot_distance"] == pytest.approx(rd["ot_distance"], rel=1e-9)
    for k, v in rd["dual_variables"].items():
        assert dg["dual_variables"][k] == pytest.approx(v, rel=1e-9)
    assert dg["transport_plan_sparsity"] == rd["transport_plan_sparsity"]  # the same count over N^2
    assert [e["iteration"] for e in dg["convergence_history"]] == [e["iteration"] for e in rd["convergence_history"]]
    for a, b in zip(dg["convergence_history"], rd["convergence_history"]):
        assert abs(a["f_change"] - b["f_change"]) <= 1e-9 and abs(a["g_change"] - b["g_change"]) <= 1e-9


def test_batch_is_bitwise_the_problems_alone_and_independent_of_the_polling_chunk(monkeypatch):
    c = R.BATCH
    cases = [R.solved(c["N"], c["d"], c["eps"], R.EARLY_ITERS, c["scale"], c["conc"], seed) for seed, _ in c["seeds"]]
    X = np.stack([x for x, _, _ in cases])
    w = np.stack([v for _, v, _ in cases])
    out, its, hist, f, g, stats = device(X, w, c["eps"], R.EARLY_ITERS)
    assert [int(i) for i in its] == [stop for _, stop in c["seeds"]]
    for b, (xb, wb, ref) in enumerate(cases):
        assert np.max(np.abs(out[b] - ref["particles"])) <= TOL * max(1.0, float(np.max(np.abs(ref["particles"]))))
        alone = device(xb, wb, c["eps"], R.EARLY_ITERS)
        for got, one in zip((out, its, hist, f, g, stats), alone):
            assert np.array_equal(got[b], one[0])
    again = device(X, w, c["eps"], R.EARLY_ITERS)
    for got, rep in zip((out, its, hist, f, g, stats), again):
        assert np.array_equal(got, rep)
    for chunk in ("1", "7", "500"):
        monkeypatch.setenv("PF_OT_POLL", chunk)
        polled = device(X, w, c["eps"], R.EARLY_ITERS)
        for got, rep in zip((out, its, hist, f, g, stats), polled):
            assert np.array_equal(got, rep), f"PF_OT_POLL={chunk}"
    # the public call, batched: a list of dicts, each problem's own iteration count
    new, nw, dgs = OT.sinkhorn_ot_resample(X, w, epsilon=c["eps"], n_iters=R.EARLY_ITERS, return_diagnostics=True)
    assert new.shape == X.shape and nw.shape == w.shape and np.array_equal(new, out)
    assert [dg["sinkhorn_iterations"] for dg in dgs] == [stop for _, stop in c["seeds"]]
    assert all(dg["converged"] for dg in dgs)


def test_source_split_and_the_unsplit_order(monkeypatch):
    N, d, eps, n_iters, scale, conc, seed = R.SPLIT
    X, w, ref = R.solved(*R.SPLIT)
    split = compare(f"split N={N}", X, w, eps, n_iters, ref)
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_OT_SPLITS", "1")
    one = compare(f"unsplit N={N}", X, w, eps, n_iters, ref)
    sx = max(1.0, float(np.max(np.abs(ref["particles"]))))
    assert np.max(np.abs(split[0] - one[0])) <= TOL * sx
    assert not np.array_equal(split[0], one[0])  # the hook took effect: another summation order


def _sv_filter(resampler_rng_seed=11):
    """The 1-D SV model of the nonlinear notebook, in NumPy: x' = mu + phi (x - mu) + sigma n,
    y ~ N(0, beta^2 exp(x))."""
    mu, phi, sigma, beta = 0.0, 0.95, 0.25, 0.6
    noise = np.random.default_rng(resampler_rng_seed)

    def transition_fn(p, t):
        return mu + phi * (p - mu) + sigma * noise.standard_normal(p.shape)

    def obs_loglik_fn(p, y, t):
        x = p[:, 0]
        return -0.5 * np.log(2.0 * np.pi * beta ** 2) - 0.5 * x - 0.5 * y * y * np.exp(-x) / beta ** 2
    return transition_fn, obs_loglik_fn


def test_run_filter_on_the_sv_model():
    N, T = 100, 10
    y = 0.6 * np.exp(0.5 * 0.3 * np.random.default_rng(21).standard_normal(T)) * np.random.default_rng(
        22).standard_normal(T)
    runs = {}
    for which in ("device", "restatement"):
        tf_, lf_ = _sv_filter()
        flt = OT.DPF_OT(N, 1, tf_, lf_, epsilon=0.1, sinkhorn_iters=50, rng=np.random.default_rng(5))
        if which == "restatement":
            flt._resample = R.resample_fn
        try:
            runs[which] = flt.run_filter(y, np.zeros(1), 0.5 * np.eye(1), return_diagnostics=True,
                                         ground_truth=np.zeros((T + 1, 1)))
        finally:
            flt.close()
    (pd, wd, dd), (pr, wr, dr) = runs["device"], runs["restatement"]
    assert len(pd) == T and len(wd) == T
    worst = 0.0
    for t in range(T):
        assert pd[t].shape == (N, 1) and pd[t].dtype == np.float64
        err = float(np.max(np.abs(pd[t] - pr[t]))) / max(1.0, float(np.max(np.abs(pr[t]))))
        worst = max(worst, err)
        assert err <= TOL, f"step {t}"
        assert np.array_equal(wd[t], wr[t]) and np.array_equal(wd[t], np.full(N, 1.0 / N))
    print(f"DPF_OT SV run: worst per-step particle error {worst:.3e} (relative to max(1, max|x|))")
    assert set(dd) == set(dr)
    assert dd["sinkhorn_iterations_mean"] == dr["sinkhorn_iterations_mean"]
    assert dd["converged_rate"] == dr["converged_rate"]
    assert dd["ot_distance_mean"] == pytest.approx(dr["ot_distance_mean"], rel=1e-9)
    assert dd["mean_rmse"] == pytest.approx(dr["mean_rmse"], rel=1e-9)
    # a single step with diagnostics returns the reference's keys
    tf_, lf_ = _sv_filter()
    flt = OT.DPF_OT(N, 1, tf_, lf_, rng=np.random.default_rng(5))
    try:
        p0, w0 = flt.init_particles(np.zeros(1), np.eye(1))
        _, _, sd = flt.step(p0, w0, y[0], t=0, return_diagnostics=True)
    finally:
        flt.close()
    assert set(sd) == {"ess_before", "ess_after", "entropy_before", "entropy_after", "diversity_before",
                       "diversity_after", "max_weight_before", "step_time", "sinkhorn_iterations", "converged",
                       "ot_distance", "transport_plan_sparsity", "dual_variables", "convergence_history", "epsilon"}
