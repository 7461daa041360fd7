"""CPU checks of the Sinkhorn OT resampler's host side (no GPU).

* the vectorised restatement (tests/dpf_ot_restatement.py), which the GPU tests compare the device
  with, equals the literal per-row transcription of the reference's loop;
* properties of the resampler that hold for the formulas themselves;
* the conditions tests/test_gpu_dpf_ot.py relies on: the stopping iterations of its cases, the
  distance of every convergence check from the tolerance, and the distance of every plan entry
  from the sparsity threshold; for the numerical edges also that the floor inside Tau binds with no
  sum near it, and that the cloud far from the origin is conditioned a decade inside the bound;
* pf_ot_create's argument checks, which answer before a device is touched, and the Python
  validation, which answers before the library is loaded;
* DPF_OT's weight update, with a host resampler injected;
* the split of the source range (csrc/pf_dpf_plan.h), which is part of the summation order.
"""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_ot as OT
from tests import dpf_ot_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-6  # the stopping tolerance of every case


@pytest.mark.parametrize("N,d,eps,n_iters,seed", [(1, 2, 0.1, 50, 0), (2, 1, 0.1, 50, 224), (7, 3, 0.1, 50, 1),
                                                  (24, 2, 0.5, 80, 2), (17, 5, 2.0, 30, 3)])
def test_vectorised_restatement_equals_the_per_row_loop(N, d, eps, n_iters, seed):
    X, w = R.make_case(N, d, seed=seed)
    v = R.sinkhorn_resample(X, w, eps, n_iters)
    l = R.loop_resample(X, w, eps, n_iters)
    assert v["iterations"] == l["iterations"]
    for key in ("particles", "f", "g", "P"):
        err = float(np.max(np.abs(v[key] - l[key])))
        print(f"restatement vs loop N={N} d={d} {key}: {err:.3e}")
        assert err <= 1e-13
    hv, hl = v["diagnostics"]["convergence_history"], l["diagnostics"]["convergence_history"]
    assert [e["iteration"] for e in hv] == [e["iteration"] for e in hl]
    for a, b in zip(hv, hl):
        assert abs(a["f_change"] - b["f_change"]) <= 1e-13 and abs(a["g_change"] - b["g_change"]) <= 1e-13


def test_tau_epsilon_and_distances_are_the_reference_expressions():
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((6, 3)), rng.standard_normal((4, 3))
    D = OT.pairwise_squared_distances(x, y)
    direct = np.sum((x[:, None, :] - y[None, :, :]) ** 2, axis=-1)
    assert D.shape == (6, 4) and np.all(D >= 0.0)
    np.testing.assert_allclose(D, direct, rtol=0, atol=1e-13)
    assert np.all(np.diag(OT.pairwise_squared_distances(x, x)) <= 1e-14)
    a = rng.random(6)
    f, c = rng.standard_normal(6), rng.random(6)
    direct = -0.3 * np.log(np.sum(a * np.exp((f - c) / 0.3)))
    assert abs(OT.tau_epsilon(a, f, c, 0.3) - direct) <= 1e-14
    # the floor inside the logarithm
    assert OT.tau_epsilon(np.zeros(3), np.zeros(3), np.zeros(3), 0.5, 1e-12) == -0.5 * np.log(1e-12)


def test_new_weights_are_exactly_uniform_and_n1_returns_the_particle():
    X, w = R.make_case(9, 2, seed=4)
    r = R.sinkhorn_resample(X, w)
    assert np.array_equal(r["weights"], np.full(9, 1.0 / 9.0))
    X1 = np.array([[0.7, -1.3]])
    r1 = R.sinkhorn_resample(X1, np.array([1.0]))
    np.testing.assert_allclose(r1["particles"], X1, rtol=0, atol=1e-11)
    assert np.array_equal(r1["weights"], [1.0])


@pytest.mark.parametrize("case", R.EARLY)
def test_early_stop_cases_stop_where_stated_with_a_margin_and_balance_the_plan(case):
    N, d, eps, scale, conc, seed, stop = case
    X, w, r = R.solved(N, d, eps, R.EARLY_ITERS, scale, conc, seed)
    assert r["iterations"] == stop
    hist = r["diagnostics"]["convergence_history"]
    assert [e["iteration"] for e in hist] == list(range(1, stop))
    margin = min(min(abs(e["f_change"] - TOL), abs(e["g_change"] - TOL)) for e in hist)
    print(f"early stop N={N}: stops at {stop}, smallest |change - tol| = {margin / TOL:.3g} tol")
    assert margin >= 1e-3 * TOL
    # a stopped problem is close to the fixed point: column sums 1/N, weighted mean preserved
    b = 1.0 / N
    assert np.max(np.abs(r["P"].sum(axis=0) - b)) <= 1e-4 * b
    mean_in = np.sum(r["a"][:, None] * X, axis=0)
    mean_out = np.mean(r["particles"], axis=0)
    assert np.max(np.abs(mean_out - mean_in)) <= 1e-4 * max(1.0, float(np.max(np.abs(X))))


@pytest.mark.parametrize("case", R.FULL)
def test_full_length_cases_stop_where_stated(case):
    N, d, eps, n_iters, seed = case
    X, w, r = R.solved(N, d, eps, n_iters, 1.0, 1.0, seed)
    stop = R.FULL_STOPS.get((N, d), n_iters)
    assert r["iterations"] == stop
    hist = r["diagnostics"]["convergence_history"]
    if hist and N > 1:  # N = 1: both changes are zero to rounding, far below tol
        margin = min(min(abs(e["f_change"] - TOL), abs(e["g_change"] - TOL)) for e in hist)
        assert margin >= 1e-3 * TOL
    assert np.all(np.isfinite(r["particles"]))


@pytest.mark.parametrize("case", R.DIAG)
def test_no_plan_entry_of_the_diagnostics_cases_is_at_the_sparsity_threshold(case):
    X, w, r = R.solved(*case)
    gap = float(np.min(np.abs(r["P"] - 1e-6)))
    print(f"sparsity margin N={case[0]} d={case[1]}: {gap:.3e}")
    assert gap >= 1e-12


# ------------------------------------------------------------------ C ABI, no device
def _create(n, d, b, dev=0):
    h = C.c_void_p()
    st = NV.load().pf_ot_create(C.byref(NV.OtOpts(n, d, b, dev)), C.byref(h))
    return st, h


def test_create_rejects_bad_arguments_before_touching_a_device():
    lib = NV.load()
    for n, d, b in ((0, 2, 1), (-5, 2, 1), (10, 0, 1), (10, 1025, 1), (10, 2, 0), (10, 2, -1)):
        st, h = _create(n, d, b)
        assert st == NV.PF_E_ARG and not h.value, (n, d, b)
        assert lib.pf_last_error()
    h = C.c_void_p()
    assert lib.pf_ot_create(None, C.byref(h)) == NV.PF_E_ARG
    assert lib.pf_ot_create(C.byref(NV.OtOpts(10, 2, 1, 0)), None) == NV.PF_E_ARG
    with pytest.raises(ValueError):
        NV.check(NV.PF_E_ARG)
    # null handles
    assert lib.pf_ot_resample(None, None, None, 0.1, 1, 1e-12, 1e-6, None, None, None, None, None, None) == NV.PF_E_ARG
    assert lib.pf_ot_synchronize(None) == NV.PF_E_ARG
    assert not lib.pf_ot_stream(None)
    lib.pf_ot_destroy(None)


@pytest.mark.parametrize("particles,weights,kw", [
    (np.zeros(4), np.ones(4), {}),                      # rank
    (np.zeros((2, 3, 4, 5)), np.ones((2, 3)), {}),      # rank
    (np.zeros((4, 2)), np.ones((4, 1)), {}),            # weights rank
    (np.zeros((4, 2)), np.ones(5), {}),                 # N mismatch
    (np.zeros((3, 4, 2)), np.ones((2, 4)), {}),         # batch mismatch
    (np.zeros((0, 2)), np.ones(0), {}),                 # N < 1
    (np.zeros((4, 0)), np.ones(4), {}),                 # d < 1
    (np.array([[0.0], [np.nan]]), np.ones(2), {}),      # non-finite particles
    (np.zeros((2, 1)), np.array([1.0, np.inf]), {}),    # non-finite weights
    (np.zeros((2, 1)), np.ones(2), {"epsilon": 0.0}),
    (np.zeros((2, 1)), np.ones(2), {"epsilon": -1.0}),
    (np.zeros((2, 1)), np.ones(2), {"n_iters": -1}),
])
def test_python_validation_raises_before_the_library_is_loaded(monkeypatch, particles, weights, kw):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(NV, "load", no_load)
    with pytest.raises(ValueError):
        OT.sinkhorn_ot_resample(particles, weights, **kw)


# ------------------------------------------------------------------ DPF_OT on the host
def _sv_model(rng):
    def transition_fn(p, t):
        return 0.95 * p + 0.2 * rng.standard_normal(p.shape)

    def obs_loglik_fn(p, y, t):
        return -0.5 * p[:, 0] - 0.5 * y * y * np.exp(-p[:, 0])
    return transition_fn, obs_loglik_fn


def test_step_does_the_reference_weight_update_and_hands_it_to_the_resampler():
    N = 12
    rng = np.random.default_rng(3)
    tf_, lf_ = _sv_model(np.random.default_rng(8))
    flt = OT.DPF_OT(N, 1, tf_, lf_, epsilon=0.3, sinkhorn_iters=7, rng=rng)
    seen = {}

    def stub(particles, weights, epsilon=0.1, n_iters=50, return_diagnostics=False):
        seen.update(particles=particles.copy(), weights=weights.copy(), epsilon=epsilon, n_iters=n_iters)
        return particles + 1.0, np.full(len(weights), 1.0 / len(weights))
    flt._resample = stub
    particles, weights = flt.init_particles(np.zeros(1), np.eye(1))
    assert particles.shape == (N, 1) and np.array_equal(weights, np.full(N, 1.0 / N))
    w_in = np.random.default_rng(1).random(N)
    out, w_out = flt.step(particles, w_in, 0.4, t=0)
    pred = 0.95 * particles + 0.2 * np.random.default_rng(8).standard_normal(particles.shape)
    un = np.maximum(w_in * np.exp(lf_(pred, 0.4, 0)), 0.0)
    assert np.array_equal(seen["particles"], pred)
    assert np.array_equal(seen["weights"], un / (np.sum(un) + 1e-12))
    assert seen["epsilon"] == 0.3 and seen["n_iters"] == 7
    assert np.array_equal(out, pred + 1.0) and np.array_equal(w_out, np.full(N, 1.0 / N))
    flt.close()


def test_run_filter_with_the_restatement_as_resampler_and_its_diagnostics():
    N, T = 20, 4
    tf_, lf_ = _sv_model(np.random.default_rng(8))
    flt = OT.DPF_OT(N, 1, tf_, lf_, epsilon=0.5, sinkhorn_iters=30, rng=np.random.default_rng(2))
    flt._resample = R.resample_fn
    y = np.random.default_rng(4).standard_normal(T)
    truth = np.zeros((T + 1, 1))
    ps, ws, diag = flt.run_filter(y, np.zeros(1), np.eye(1), return_diagnostics=True, ground_truth=truth)
    assert len(ps) == T and len(ws) == T and ps[0].shape == (N, 1)
    for key in ("ess_before_mean", "ess_after_mean", "entropy_before_mean", "sinkhorn_iterations_mean",
                "sinkhorn_iterations_max", "converged_rate", "ot_distance_mean", "transport_plan_sparsity_mean",
                "epsilon_mean", "step_time_mean", "total_time", "mean_step_time", "rmse_sequence", "mean_rmse",
                "final_rmse", "max_weight_before_mean"):
        assert key in diag, key
    assert "convergence_history" not in diag
    assert set(diag["dual_variables"]) == {k + s for k in ("f_mean", "f_std", "g_mean", "g_std")
                                           for s in ("_mean", "_std")}
    assert set(diag["diversity_before"]) == {"mean_pairwise_dist_mean", "mean_pairwise_dist_std",
                                             "particle_spread_mean", "particle_spread_std"}
    assert abs(diag["ess_after_mean"] - N) <= 1e-9 and diag["rmse_sequence"].shape == (T,)
    flt.close()


def test_static_diagnostics_match_their_formulas():
    rng = np.random.default_rng(6)
    w = rng.random(30)
    wn = w / (w.sum() + 1e-12)
    assert OT.DPF_OT.compute_ess(w) == pytest.approx(1.0 / np.sum(wn ** 2), rel=1e-15)
    assert OT.DPF_OT.compute_ess(np.stack([w, w])).shape == (2,)
    assert OT.DPF_OT.compute_weight_entropy(w) == pytest.approx(-np.sum(wn * np.log(wn + 1e-10)), rel=1e-15)
    P = rng.standard_normal((30, 3))
    full = np.linalg.norm(P[:, None, :] - P[None, :, :], axis=-1)
    dv = OT.DPF_OT.compute_particle_diversity(P, block=7)  # blocks with a tail
    assert dv["mean_pairwise_dist"] == pytest.approx(full.sum() / (30 * 29), rel=1e-13)
    assert dv["particle_spread"] == pytest.approx(np.trace(np.cov(P.T, bias=True)), rel=1e-13)
    dvb = OT.DPF_OT.compute_particle_diversity(np.stack([P, 2 * P]))
    assert dvb["mean_pairwise_dist"].shape == (2,) and dvb["mean_pairwise_dist"][1] == pytest.approx(
        2 * dv["mean_pairwise_dist"], rel=1e-13)


def _margin(hist):
    return min(min(abs(e["f_change"] - TOL), abs(e["g_change"] - TOL)) for e in hist)


@pytest.mark.parametrize("kind", R.WEIGHT_KINDS)
def test_weight_cases_are_normalised_as_the_reference_does(kind):
    X, w, r = R.solved_weights(kind)
    a = np.maximum(w, 1e-12)
    a = a / (a.sum() + 1e-12)
    assert np.array_equal(r["a"], a) and np.all(r["a"] > 0.0)
    assert _margin(r["diagnostics"]["convergence_history"]) >= 1e-3 * TOL
    assert np.all(np.isfinite(r["particles"]))


def _well_posed(tag, X, w, eps, n_iters, r, sparsity=False):
    """The conditions every GPU case rests on: no convergence check within 1e-3 tol of tol, the
    restatement within 1e-10 of the scales of the per-row loop (a tenth of the GPU bound) and, where
    the diagnostics are compared, no plan entry within 1e-12 of the sparsity threshold."""
    hist = r["diagnostics"]["convergence_history"]
    if hist:
        m = _margin(hist)
        print(f"{tag}: stops at {r['iterations']}, smallest |change - tol| = {m / TOL:.3g} tol")
        assert m >= 1e-3 * TOL
    l = R.loop_resample(X, w, eps, n_iters)
    assert l["iterations"] == r["iterations"]
    sx = max(1.0, float(np.max(np.abs(l["particles"]))))
    sf = max(1.0, float(np.max(np.abs(l["f"]))), float(np.max(np.abs(l["g"]))))
    ex = float(np.max(np.abs(r["particles"] - l["particles"])))
    ef = max(float(np.max(np.abs(r["f"] - l["f"]))), float(np.max(np.abs(r["g"] - l["g"]))))
    print(f"{tag}: restatement vs loop, particles {ex:.3e} (scale {sx:.3g}), duals {ef:.3e} (scale {sf:.3g})")
    assert ex <= 1e-10 * sx and ef <= 1e-10 * sf
    assert np.all(np.isfinite(r["particles"]))
    if sparsity:
        gap = float(np.min(np.abs(r["P"] - 1e-6)))
        print(f"{tag}: sparsity margin {gap:.3e}")
        assert gap >= 1e-12


@pytest.mark.parametrize("case", R.STAGES + R.TILES[:1])  # TILES[1] is FULL's and DIAG's (300, 40)
def test_stage_and_tile_cases_are_well_posed(case):
    N, d, eps, n_iters, seed = case
    X, w, r = R.solved(N, d, eps, n_iters, 1.0, 1.0, seed)
    assert r["iterations"] == n_iters
    _well_posed(f"N={N} d={d}", X, w, eps, n_iters, r)


def test_the_tile_and_no_diagnostics_cases_are_cases_checked_elsewhere():
    full = {(N, d, eps, n, seed) for N, d, eps, n, seed in R.FULL}
    assert R.TILES[1] in full and all(c in full for c in R.PERMUTED)
    known = set(R.DIAG) | {(N, d, eps, R.EARLY_ITERS, sc, co, seed) for N, d, eps, sc, co, seed, _ in R.EARLY}
    assert all(c in known for c in R.NODIAG)


@pytest.mark.parametrize("b", range(3))
def test_chunk_batch_problems_are_well_posed(b):
    c = R.CHUNK_BATCH
    X, w, r = R.solved_chunk_batch(b)
    assert r["iterations"] == c["n_iters"] and (np.count_nonzero(w == 0.0) > 40) == (b == c["zeros"])
    _well_posed(f"chunk batch problem {b}", X, w, c["eps"], c["n_iters"], r)


@pytest.mark.parametrize("batch", [False, True])
def test_the_calls_on_one_handle_stop_where_the_sequence_needs_them_to(batch):
    stops = []
    for tag, X, w, eps, n_iters in R.handle_sequence(batch):
        for xb, wb in (zip(X, w) if batch else [(X, w)]):
            r = R.sinkhorn_resample(xb, wb, eps, n_iters)
            hist = r["diagnostics"]["convergence_history"]
            assert not hist or _margin(hist) >= 1e-3 * TOL
            stops.append(r["iterations"])
    per = 3 if batch else 1
    early = {s for _, s in R.BATCH["seeds"]}
    assert stops[:per] == [s for _, s in R.BATCH["seeds"]][:per]  # stops early, before a full-length call
    assert stops[per:4 * per] == [50] * per + [0] * per + [1] * per
    assert set(stops[4 * per:5 * per]) <= early and stops[4 * per:5 * per] != stops[:per]
    assert stops[5 * per:] == [50] * per


@pytest.mark.parametrize("name", R.EDGES)
def test_edge_cases_are_well_posed(name):
    X, w, eps, n_iters, r = R.solved_edge(name)
    _well_posed(name, X, w, eps, n_iters, r, sparsity=True)


@pytest.mark.parametrize("name", ["floor eps=0.1", "floor eps=0.05", "sharp"])
def test_the_floor_inside_tau_binds_and_no_sum_is_near_it(name):
    """In every iteration at least one column sum of the g pass is below min_val, and none in any
    iteration is within 10 % of min_val on either side, so the floor decision cannot flip on
    rounding.  The sharp case has the same particles; almost its whole plan sits at min_val."""
    X, w, eps, n_iters = R.edge_case(name)
    sums = []
    r = R.sinkhorn_resample(X, w, eps, n_iters, col_sums=sums)
    S = np.array(sums)
    assert S.shape == (n_iters, 130)
    below = np.sum(S < 1e-12, axis=1)
    near = float(np.min(np.abs(S / 1e-12 - 1.0)))
    at_floor = float(np.mean(r["P"] == 1e-12))
    print(f"{name}: min a {r['a'].min():.3e}, columns below min_val per iteration {below.min()}..{below.max()} "
          f"({below.sum()} in all), nearest relative distance to the floor {near:.3g}, "
          f"{100 * at_floor:.1f} % of the plan at min_val")
    assert np.all(below >= 1) and near >= 0.1
    if name == "sharp":
        assert at_floor >= 0.95


def test_far_cloud_is_conditioned_a_decade_inside_the_bound():
    """The expansion |x_i|^2 - 2 x_i.x_j + |x_j|^2 cancels 30^2 d against distances of order 1.  With C
    from exact differences instead the restatement moves by at most 1e-10 of the scales, so the
    device's other rounding of C (fma) cannot use up the 1e-9 bound; the clamp acts on the diagonal."""
    X, w, eps, n_iters, r = R.solved_edge("far")
    Ce = R.exact_cost(X)
    e = R.sinkhorn_resample(X, w, eps, n_iters, cost=Ce)
    diag = np.diag(r["C"])
    sx = max(1.0, float(np.max(np.abs(r["particles"]))))
    ex = float(np.max(np.abs(r["particles"] - e["particles"])))
    ef = max(float(np.max(np.abs(r["f"] - e["f"]))), float(np.max(np.abs(r["g"] - e["g"]))))
    print(f"far: C error {np.max(np.abs(r['C'] - Ce)):.3e}, diagonal of C in [{diag.min():.3e}, {diag.max():.3e}], "
          f"exact-C shift: particles {ex / sx:.3e} of the scale {sx:.3g}, duals {ef:.3e}")
    assert e["iterations"] == r["iterations"]
    assert ex <= 1e-10 * sx and ef <= 1e-10
    assert diag.min() == 0.0 and diag.max() > 0.0  # the clamp acts, and the cancellation is there
    assert np.max(np.abs(r["C"] - Ce)) > 1e-13


def test_duplicate_cases_hold_duplicates():
    X, *_ = R.edge_case("ten points")
    assert X.shape == (130, 3) and len(np.unique(X, axis=0)) == 10
    X, *_ = R.edge_case("one point")
    assert X.shape == (70, 3) and len(np.unique(X, axis=0)) == 1


def test_batch_problems_stop_at_different_iterations_with_a_margin():
    c = R.BATCH
    stops = []
    for seed, stop in c["seeds"]:
        X, w, r = R.solved(c["N"], c["d"], c["eps"], R.EARLY_ITERS, c["scale"], c["conc"], seed)
        assert r["iterations"] == stop
        assert _margin(r["diagnostics"]["convergence_history"]) >= 1e-3 * TOL
        stops.append(stop)
    assert len(set(stops)) == 3


# ------------------------------------------------------------------ the split of the source range
def test_source_range_split_under_sanitizers():
    """pf::dpf::make_split (csrc/pf_dpf_plan.h), the split of the OT and the soft resampler, in a
    stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer
    (tests/host/pf_dpf_plan_host_check.cpp)."""
    exe = os.path.join(REPO, "build", "pf_dpf_plan_host_check")
    if not os.path.exists(exe):  # built by __graft_entry__.build(); here if the test runs first
        subprocess.run(["make", "-C", os.path.join(REPO, "particle_filters_amd", "csrc"), "hostcheck"],
                       check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
