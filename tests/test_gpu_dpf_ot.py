"""Sinkhorn OT resampler and DPF_OT on the device vs the NumPy restatement (-m gpu, MI355X).

TensorFlow is not available, so there is no fixture of reference outputs: the device is compared
with tests/dpf_ot_restatement.py, the reference's formulas in fp64, which tests/test_dpf_ot_host.py
checks against the literal per-row loop.  The cases are the smallest at which tiles (64 columns, 4
rows per workgroup, 16 cost rows), tails, the LDS stages of 64 components of the cost kernel
(d = 64, 65, 130), the component chunks of 16 of the projection (d = 40: three), the source split
and the stopping rule can go wrong.

The source split.  pf_ot_create splits the source range of k_ot_tau_cols and k_ot_project from
N = 33 on: S0 = min(ceil(N / 32), 8192 / ceil(N / 64), 64), chunk = ceil(N / S0) rounded up to 32,
S = ceil(N / chunk).  N = 65 has S = 3, N = 130 S = 5, N = 300 S = 10, all with chunk = 32; the chunk
is at most 64 up to N = 4096, so by itself no case here runs the LDS tile loops of the two kernels
(128 and 64 sources) more than once inside a split.  The hooked runs do (PF_TEST_HOOKS=1):
PF_TEST_OT_SPLITS=1 at N = 2500 is chunk = 2528, S = 1 (20 and 40 tiles, nothing merged), against
chunk = 64, S = 40 unhooked; =2 and =3 at N = 300 are chunk = 160, S = 2 and chunk = 128, S = 3:
several tiles per split and a merge, which is what the library does unhooked from N = 4097 on
(N = 10000: S = 45, chunk = 224).

Beyond parity: a batch of problems with component chunks and splits is bitwise the problems alone;
the call without diagnostics (null plan_stats, f, g, history, iterations) returns the same bits; a
handle that has solved other problems returns the bits of a fresh one; numerical edges (the floor
inside Tau binding, cancellation in C, duplicates, a plan almost wholly at min_val); and
permuting the particles permutes the result, which needs no reference.

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


def _batched(X, w):
    X = np.ascontiguousarray(X, dtype=float)
    w = np.ascontiguousarray(w, dtype=float)
    return (X, w) if X.ndim == 3 else (X[None], w[None])


def call(h, X, w, eps, n_iters, want_diag=True, **kw):
    """One pf_ot_resample call on the handle h, batch axis first."""
    Xb, wb = _batched(X, w)
    return h.resample(Xb, wb, eps, n_iters, kw.get("min_val", 1e-12), kw.get("tol", 1e-6), want_diag)


def device(X, w, eps, n_iters, want_diag=True, **kw):
    """(X_out, iterations, history, f, g, plan_stats) of one pf_ot_resample call on a fresh handle,
    batch axis first; without want_diag the last four are None (null pointers in the call)."""
    Xb, wb = _batched(X, w)
    h = OT._Handle(Xb.shape[1], Xb.shape[2], Xb.shape[0])
    try:
        return call(h, Xb, wb, eps, n_iters, want_diag, **kw)
    finally:
        h.close()


def compare(tag, X, w, eps, n_iters, ref):
    return compare_result(tag, device(X, w, eps, n_iters), ref)


def compare_result(tag, res, ref, b=0):
    """Problem b of a device result against its restatement; returns the result."""
    out, its, hist, f, g, stats = (v[b:b + 1] for v in res)
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
    compare_diagnostics(X, w, eps, n_iters, ref)


def compare_diagnostics(X, w, eps, n_iters, ref):
    N, d = X.shape
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


def _same_within_the_bound(a, b):
    sx = max(1.0, float(np.max(np.abs(a[0]))))
    sf = max(1.0, float(np.max(np.abs(a[3]))), float(np.max(np.abs(a[4]))))
    assert np.array_equal(a[1], b[1])
    assert np.max(np.abs(a[0] - b[0])) <= TOL * sx
    assert max(np.max(np.abs(a[3] - b[3])), np.max(np.abs(a[4] - b[4]))) <= TOL * sf


def test_source_split_with_several_tiles_per_split(monkeypatch):
    """k_ot_tau_cols stages its sources through LDS in tiles of TT = 128 and k_ot_project in tiles of
    PT = 64, inside each split of the source range.  pf_ot_create takes S0 = min(ceil(N / 32),
    8192 / ceil(N / 64), 64), or PF_TEST_OT_SPLITS when that is smaller, then chunk = ceil(N / S0)
    rounded up to a multiple of 32 and S = ceil(N / chunk).  At N = 300:

    =====================  =====  ==  ==============  ====================  ==========================
    PF_TEST_OT_SPLITS      chunk  S   sources         tiles of 128          tiles of 64
    =====================  =====  ==  ==============  ====================  ==========================
    2                      160    2   160, 140        128 + 32, 128 + 12    64 + 64 + 32, 64 + 64 + 12
    3                      128    3   128, 128, 44    128, 128, 44          64 + 64, 64 + 64, 44
    unset                  32     10  9 x 32, 12      one each              one each
    =====================  =====  ==  ==============  ====================  ==========================

    so the first two runs merge splits whose tile loops ran more than once, with a partial and with an
    exactly full last tile; that is what the library does by itself from N = 4097 on (chunk > 64).
    A change of the split rule or of TT / PT invalidates this table."""
    N, d, eps, n_iters, seed = R.TILES[0]
    X, w, ref = R.solved(N, d, eps, n_iters, 1.0, 1.0, seed)
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    runs = {}
    for splits in ("2", "3", None):
        if splits is None:
            monkeypatch.delenv("PF_TEST_OT_SPLITS", raising=False)
        else:
            monkeypatch.setenv("PF_TEST_OT_SPLITS", splits)
        runs[splits] = compare(f"N={N} d={d} PF_TEST_OT_SPLITS={splits}", X, w, eps, n_iters, ref)
    for a, b in (("2", "3"), ("2", None), ("3", None)):
        _same_within_the_bound(runs[a], runs[b])
        assert not np.array_equal(runs[a][0], runs[b][0])  # the hook took effect: another summation order
    # three component chunks on top of the multi-tile splits
    N, d, eps, n_iters, seed = R.TILES[1]
    X, w, ref = R.solved(N, d, eps, n_iters, 1.0, 1.0, seed)
    plain = compare(f"N={N} d={d} PF_TEST_OT_SPLITS=None", X, w, eps, n_iters, ref)
    monkeypatch.setenv("PF_TEST_OT_SPLITS", "2")
    two = compare(f"N={N} d={d} PF_TEST_OT_SPLITS=2", X, w, eps, n_iters, ref)
    _same_within_the_bound(two, plain)
    assert not np.array_equal(two[0], plain[0])


def test_batch_with_component_chunks_and_source_splits():
    """part is [B][S][d][Npad]: B = 3, S = 5 (N = 130, Npad 192) and three component chunks (d = 40),
    so that a wrong stride in the problem or in the chunk moves one problem's partials into
    another's."""
    c = R.CHUNK_BATCH
    cases = [R.solved_chunk_batch(b) for b in range(3)]
    X = np.stack([x for x, _, _ in cases])
    w = np.stack([v for _, v, _ in cases])
    res = device(X, w, c["eps"], c["n_iters"])
    for b, (xb, wb, ref) in enumerate(cases):
        compare_result(f"chunk batch problem {b}", res, ref, b)
        alone = device(xb, wb, c["eps"], c["n_iters"])
        for got, one in zip(res, alone):
            assert np.array_equal(got[b], one[0])
    for got, rep in zip(res, device(X, w, c["eps"], c["n_iters"])):
        assert np.array_equal(got, rep)


@pytest.mark.parametrize("case", R.NODIAG)
def test_call_without_diagnostics(case):
    """The public default: null plan_stats (k_ot_project without its statistics, no k_ot_stats), null
    f, g and history; and through the C ABI a null iterations as well, which the header allows."""
    N, d, eps, n_iters, scale, conc, seed = case
    X, w, ref = R.solved(*case)
    full = compare(f"with diagnostics N={N} d={d}", X, w, eps, n_iters, ref)
    out, its, hist, f, g, stats = device(X, w, eps, n_iters, want_diag=False)
    assert hist is None and f is None and g is None and stats is None
    assert np.array_equal(out, full[0]) and np.array_equal(its, full[1])
    new, nw = OT.sinkhorn_ot_resample(X, w, epsilon=eps, n_iters=n_iters)
    assert new.shape == (N, d) and np.array_equal(new, full[0][0]) and np.array_equal(nw, np.full(N, 1.0 / N))
    Xb, wb = _batched(X, w)
    bare = np.full_like(Xb, np.nan)
    h = OT._Handle(N, d, 1)
    try:
        NV.check(NV.load().pf_ot_resample(h.h, NV.dptr(Xb), NV.dptr(wb), eps, n_iters, 1e-12, 1e-6, NV.dptr(bare),
                                          None, None, None, None, None), "pf_ot_resample")
    finally:
        h.close()
    assert np.array_equal(bare, full[0])


def test_batched_call_without_diagnostics():
    c = R.BATCH
    cases = [R.solved(c["N"], c["d"], c["eps"], R.EARLY_ITERS, c["scale"], c["conc"], seed) for seed, _ in c["seeds"]]
    X = np.stack([x for x, _, _ in cases])
    w = np.stack([v for _, v, _ in cases])
    full = device(X, w, c["eps"], R.EARLY_ITERS)
    out, its, *rest = device(X, w, c["eps"], R.EARLY_ITERS, want_diag=False)
    assert rest == [None] * 4 and np.array_equal(out, full[0]) and np.array_equal(its, full[1])
    assert [int(i) for i in its] == [stop for _, stop in c["seeds"]]
    new, nw = OT.sinkhorn_ot_resample(X, w, epsilon=c["eps"], n_iters=R.EARLY_ITERS)
    assert np.array_equal(new, full[0]) and np.array_equal(nw, np.full(w.shape, 1.0 / c["N"]))


@pytest.mark.parametrize("batch", [False, True])
def test_one_handle_many_calls(batch):
    """Every call on a used handle equals the same call on a fresh one, bit for bit: nothing of an
    earlier call (done flags, iteration counts, f, g, a history of another length) is left over."""
    B = 3 if batch else 1
    early = [stop for _, stop in R.BATCH["seeds"]][:B]
    expect = {"early stop": early, "full length": [50] * B, "no iteration": [0] * B, "one iteration": [1] * B,
              "early stop, other seed": (early[1:] + early[:1]) if batch else [R.BATCH["seeds"][1][1]],
              "eps 0.5": [50] * B}
    h = OT._Handle(R.BATCH["N"], R.BATCH["d"], B)
    try:
        for tag, X, w, eps, n_iters in R.handle_sequence(batch):
            used = call(h, X, w, eps, n_iters)
            fresh = device(X, w, eps, n_iters)
            print(f"OT one handle, B={B}, {tag}: iterations {[int(i) for i in used[1]]}")
            assert [int(i) for i in used[1]] == expect[tag]
            for name, got, ref in zip(("particles", "iterations", "history", "f", "g", "plan_stats"), used, fresh):
                assert np.array_equal(got, ref), f"{tag}: {name}"
            assert np.all(np.isfinite(used[0]))
            if n_iters == 0:
                assert not used[3].any() and not used[4].any()
    finally:
        h.close()


@pytest.mark.parametrize("name", R.EDGES)
def test_numerical_edges(name):
    """The floor inside Tau binding, a cloud far from the origin (cancellation in C, the clamp at 0 on
    its diagonal), duplicate particles, and an eps so sharp that almost the whole plan is at min_val."""
    X, w, eps, n_iters, ref = R.solved_edge(name)
    compare(f"edge {name}", X, w, eps, n_iters, ref)
    if name == "sharp":
        compare_diagnostics(X, w, eps, n_iters, ref)


def _permuted(N):
    return np.random.default_rng(R.PERMUTATION_SEED).permutation(N)


def _check_permuted(tag, plain, moved, perm):
    """The device against itself: relabelling the particles relabels the outputs."""
    out, its, _, f, g, _ = plain
    sx = max(1.0, float(np.max(np.abs(out))))
    sf = max(1.0, float(np.max(np.abs(f))), float(np.max(np.abs(g))))
    ex = float(np.max(np.abs(moved[0] - out[:, perm])))
    ef = max(float(np.max(np.abs(moved[3] - f[:, perm]))), float(np.max(np.abs(moved[4] - g[:, perm]))))
    print(f"OT permuted {tag}: particle difference {ex:.3e} (scale {sx:.3g}), dual difference {ef:.3e} (scale {sf:.3g})")
    assert np.array_equal(moved[1], its)
    assert ex <= TOL * sx and ef <= TOL * sf
    assert not np.array_equal(moved[0], out)  # the permutation did move the particles


@pytest.mark.parametrize("case", R.PERMUTED)
def test_permuting_the_particles_permutes_the_result(case):
    N, d, eps, n_iters, seed = case
    X, w = R.make_case(N, d, seed=seed)
    perm = _permuted(N)
    _check_permuted(f"N={N} d={d}", device(X, w, eps, n_iters), device(X[perm], w[perm], eps, n_iters), perm)


def test_permuting_the_particles_of_a_batch_permutes_the_result():
    c = R.CHUNK_BATCH
    cases = [R.solved_chunk_batch(b) for b in range(3)]
    X = np.stack([x for x, _, _ in cases])
    w = np.stack([v for _, v, _ in cases])
    perm = _permuted(c["N"])
    _check_permuted("chunk batch", device(X, w, c["eps"], c["n_iters"]),
                    device(X[:, perm], w[:, perm], c["eps"], c["n_iters"]), perm)


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
