"""The one-launch Sinkhorn solver, PF_OT_RESIDENT of pf_ot_resample_dev (-m gpu, MI355X): one workgroup
per problem, the cost matrix in LDS, N <= 128.

Parity is against the NumPy restatement (tests/dpf_ot_restatement.py) under the unit's bound, that of
tests/test_gpu_dpf_ot.py: particles within 1e-9 max(1, max|X_ref|), f and g within 1e-9 max(1, max|f|,
max|g|), iteration counts equal.  The solver sums in an order of its own, so it is not compared with
the launch sequence bitwise; its recorded history is compared with the launch sequence's under the
same bound, and the floor argmax rows exactly.  tests/test_dpf_ot_dev_host.py asserts on the CPU what
makes "equal" well defined for these cases (the stopping margins, one floored column with room).

Bitwise: two calls, a problem in a batch against the problem alone, a poisoned LDS against a clean
one, a reused handle against fresh ones.  Gradients: pf_ot_backward_dev on the resident history against
the autograd restatement (tests/dpf_ot_grad_restatement.py) under its 1e-9 of the scale.

Largest errors measured on an MI355X: DESIGN.md section 4.
"""

import numpy as np
import pytest
import torch

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_ot as OT
from tests import dpf_ot_grad_restatement as GR
from tests import dpf_ot_restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-9
MIN_VAL, TOL_STOP = 1e-12, 1e-6
RESIDENT = NV.PF_OT_RESIDENT

# (N, d, eps, n_iters, seed): all run their 50 iterations
FULL = [(3, 1, 0.1, 50, 0), (33, 1, 0.1, 50, 0), (64, 2, 0.1, 50, 0), (100, 2, 0.1, 50, 0), (128, 3, 0.1, 50, 0),
        (128, 17, 1.0, 50, 0), (63, 40, 2.0, 50, 0), (100, 65, 4.0, 50, 0)]
# make_case(N, d, 0.2, 1.0, seed) under n_iters = 500, eps = 0.1: (N, d, ((seed, stopping iteration), ...))
EARLY_BATCHES = [(128, 3, ((1, 33), (4, 34), (13, 38))), (100, 2, ((4, 32), (7, 36), (10, 33)))]
EARLY_EPS, EARLY_SCALE, EARLY_CONC = 0.1, 0.2, 1.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert NV.device_count() > 0, "no HIP device visible: -m gpu tests must run on an MI355X"
    assert torch.cuda.is_available()


def floor_case():
    """weight_case("zeros") at N = 100 scaled by 37.5, one particle of weight 0 far away: its column
    of every g pass is floored."""
    X, w = R.weight_case("zeros", N=100, d=3, seed=7)
    X, w = X.copy(), 37.5 * w
    X[99] = (-25.0, 10.0, 5.0)
    w[99] = 0.0
    return X, w, 0.1, 50


def early_case(N, d, seed):
    return (*R.make_case(N, d, EARLY_SCALE, EARLY_CONC, seed), EARLY_EPS, R.EARLY_ITERS)


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


_side = []


def side_stream():
    """A caller's stream: the entries enqueue on it and return; the callers synchronise the device
    before (their fills ran on torch's stream) and after."""
    if not _side:
        _side.append(torch.cuda.Stream())
    return _side[0].cuda_stream


def host(t):
    return None if t is None else t.cpu().numpy()


def solve(h, X, w, eps, n_iters, flags=RESIDENT, record=True, bufs=None):
    """[X_out, iterations, changes, f, g, stats, hist, hist_argmax] of pf_ot_resample_dev on NaN-filled
    buffers; X [B][N][d]."""
    B, N, d = X.shape
    Xd, wd = dev(X), dev(w)
    f64 = dict(dtype=torch.float64, device="cuda")
    out, ch = torch.full((B, N, d), np.nan, **f64), torch.full((B, n_iters, 2), np.nan, **f64)
    f, g, st = torch.full((B, N), np.nan, **f64), torch.full((B, N), np.nan, **f64), torch.full((B, 2), np.nan, **f64)
    its = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    hv = torch.full((B, 4, n_iters + 1, N), np.nan, **f64) if record else None
    am = torch.full((B, n_iters, N), -7, dtype=torch.int32, device="cuda") if record else None
    torch.cuda.synchronize()
    h.resample_dev(side_stream(), Xd.data_ptr(), wd.data_ptr(), eps, n_iters, MIN_VAL,
                   TOL_STOP, out.data_ptr(), its.data_ptr(), ch.data_ptr(), f.data_ptr(), g.data_ptr(), st.data_ptr(),
                   hv.data_ptr() if record else 0, am.data_ptr() if record and n_iters else 0, flags=flags)
    torch.cuda.synchronize()
    if bufs is not None:
        bufs.update(X=Xd, w=wd, its=its, hist=hv, am=am)
    return [host(t) for t in (out, its, ch, f, g, st, hv, am)]


def fresh(X, w, eps, n_iters, **kw):
    Xb, wb = (X, w) if X.ndim == 3 else (X[None], w[None])
    h = OT._Handle(Xb.shape[1], Xb.shape[2], Xb.shape[0])
    try:
        return solve(h, Xb, wb, eps, n_iters, **kw)
    finally:
        h.close()


def same_bits(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), k
        if x is not None:
            assert x.shape == y.shape and np.array_equal(x, y), f"array {k} differs in {int(np.sum(x != y))} elements"
    return True


worst = {"particles": 0.0, "duals": 0.0, "history": 0.0}


def compare(tag, res, ref, b=0, stop=None):
    """Problem b of a resident result against its restatement, under the bound of tests/test_gpu_dpf_ot.py."""
    out, its, ch, f, g, st = (v[b] for v in res[:6])
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(f)) and np.all(np.isfinite(g))
    sx = max(1.0, float(np.max(np.abs(ref["particles"]))))
    sf = max(1.0, float(np.max(np.abs(ref["f"]))), float(np.max(np.abs(ref["g"]))))
    ex = float(np.max(np.abs(out - ref["particles"])))
    ef = max(float(np.max(np.abs(f - ref["f"]))), float(np.max(np.abs(g - ref["g"]))))
    worst["particles"], worst["duals"] = max(worst["particles"], ex / sx), max(worst["duals"], ef / sf)
    print(f"OT resident {tag}: iterations {int(its)} (restatement {ref['iterations']}), particle error {ex:.3e} "
          f"(scale {sx:.3g}), dual error {ef:.3e} (scale {sf:.3g}); largest so far {worst}")
    assert int(its) == ref["iterations"]
    if stop is not None:
        assert int(its) == stop
    assert ex <= TOL * sx
    assert ef <= TOL * sf
    # the change history: iterations 1 .. K - 1, zero elsewhere
    K = int(its)
    want = np.zeros_like(ch)
    for e in ref["diagnostics"]["convergence_history"]:
        want[e["iteration"]] = (e["f_change"], e["g_change"])
    assert np.max(np.abs(ch - want)) <= TOL * sf and not ch[K:].any() and not ch[:1].any()
    # the plan statistics: sum P C to the bound; the count where no entry is within 1e-12 of the threshold
    assert st[0] == pytest.approx(float(np.sum(ref["P"] * ref["C"])), rel=1e-9, abs=1e-12)
    if float(np.min(np.abs(ref["P"] - 1e-6))) > 1e-12:
        assert st[1] == float(np.sum(ref["P"] > 1e-6))
    # the recorded history ends in the returned duals, and is 0 and -1 past the stop
    hv, am = res[6][b], res[7][b]
    assert np.array_equal(hv[0, K], f) and np.array_equal(hv[1, K], g) and not hv[:, 0].any()
    assert not hv[:, K + 1:].any() and np.all(am[K:] == -1)


# ====================================================================== parity with the restatement
@pytest.mark.parametrize("case", FULL, ids=lambda c: f"N{c[0]}-d{c[1]}")
def test_full_length_runs(case):
    N, d, eps, n_iters, seed = case
    X, w, ref = R.solved(N, d, eps, n_iters, 1.0, 1.0, seed)
    compare(f"full N={N} d={d}", fresh(X, w, eps, n_iters), ref, stop=n_iters)


@pytest.mark.parametrize("batch", EARLY_BATCHES, ids=lambda b: f"N{b[0]}-d{b[1]}")
def test_early_stops_alone_and_in_a_batch(batch):
    N, d, seeds = batch
    cases = [early_case(N, d, s) for s, _ in seeds]
    refs = [R.solved(N, d, EARLY_EPS, R.EARLY_ITERS, EARLY_SCALE, EARLY_CONC, s)[2] for s, _ in seeds]
    X, w = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    res = fresh(X, w, EARLY_EPS, R.EARLY_ITERS)
    for b, (s, stop) in enumerate(seeds):
        compare(f"early N={N} d={d} seed {s}, in the batch", res, refs[b], b, stop)
        alone = fresh(X[b], w[b], EARLY_EPS, R.EARLY_ITERS)
        assert same_bits(alone, [v[b:b + 1] for v in res]), f"problem {b} alone"


def small_cases():
    X1, w1, r1 = R.solved(1, 2, 0.1, 50)
    X2, w2, r2 = R.solved(2, 1, 0.1, 50, 1.0, 1.0, 224)
    Xe, we, ee, ne, re_ = R.solved_edge("one point")
    N, d, eps, scale, conc, seed, stop = R.EARLY[2]
    X3, w3, r3 = R.solved(N, d, eps, R.EARLY_ITERS, scale, conc, seed)
    return {"N1-d2": (X1, w1, 0.1, 50, r1, 2), "N2-d1": (X2, w2, 0.1, 50, r2, 32),
            "one-point": (Xe, we, ee, ne, re_, None), "N96-early": (X3, w3, eps, R.EARLY_ITERS, r3, stop)}


@pytest.mark.parametrize("name", ["N1-d2", "N2-d1", "one-point", "N96-early"])
def test_the_existing_small_cases(name):
    X, w, eps, n_iters, ref, stop = small_cases()[name]
    compare(name, fresh(X, w, eps, n_iters), ref, stop=stop)


def test_the_floor_case_and_its_argmax_rows():
    X, w, eps, n_iters = floor_case()
    ref = R.sinkhorn_resample(X, w, eps, n_iters)
    res = fresh(X, w, eps, n_iters)
    compare("floor", res, ref, stop=n_iters)
    launches = fresh(X, w, eps, n_iters, flags=0)
    assert np.array_equal(res[7], launches[7])
    assert np.all(res[7][0, :, 99] >= 0) and np.all(res[7][0, :, :99] == -1)  # the far particle's column, in every g pass


@pytest.mark.parametrize("case", [FULL[3], FULL[5], ("early", 128, 3, 13)], ids=["N100-d2", "N128-d17", "N128-early"])
def test_the_history_agrees_with_the_launch_sequences(case):
    if case[0] == "early":
        X, w, eps, n_iters = early_case(*case[1:])
    else:
        N, d, eps, n_iters, seed = case
        X, w = R.make_case(N, d, seed=seed)
    res, launches = fresh(X, w, eps, n_iters), fresh(X, w, eps, n_iters, flags=0)
    assert np.array_equal(res[1], launches[1])
    scale = max(1.0, float(np.max(np.abs(launches[6]))))
    err = float(np.max(np.abs(res[6] - launches[6])))
    worst["history"] = max(worst["history"], err / scale)
    print(f"OT resident history {case[:3]}: error {err:.3e} (scale {scale:.3g})")
    assert err <= TOL * scale
    assert np.array_equal(res[7], launches[7])


# ====================================================================== bitwise properties
def test_two_calls_are_equal_and_poisoned_equals_clean(monkeypatch):
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    X, w, eps, n_iters = early_case(128, 3, 13)
    Xf, wf = R.make_case(100, 65, seed=0)
    a, b = fresh(X, w, eps, n_iters), fresh(X, w, eps, n_iters)
    c = fresh(Xf, wf, 4.0, 50)
    assert same_bits(a, b)
    assert not np.array_equal(a[0], fresh(2.0 * X, w, eps, n_iters)[0])
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_LDS_POISON", "1")
    count = NV.load().pf_test_lds_poison_count
    before = int(count())
    pa, pc = fresh(X, w, eps, n_iters), fresh(Xf, wf, 4.0, 50)
    assert int(count()) >= before + 2
    assert all(np.all(np.isfinite(v)) for v in pa + pc if v.dtype == np.float64)
    assert same_bits(pa, a) and same_bits(pc, c)


def test_a_reused_handle_gives_the_bits_of_fresh_ones():
    N, d = 100, 2
    early = early_case(N, d, 7)
    full = (*R.make_case(N, d, seed=0), 0.1, 50)
    steps = [early, full, (*full[:3], 0), (*full[:3], 1), early_case(N, d, 10), (*full[:2], 0.5, 50)]
    h = OT._Handle(N, d, 1)
    try:
        got = [solve(h, X[None], w[None], eps, n) for X, w, eps, n in steps]
        mixed = solve(h, full[0][None], full[1][None], 0.1, 50, flags=0)  # the launch sequence on the same handle
    finally:
        h.close()
    for k, (X, w, eps, n) in enumerate(steps):
        assert same_bits(got[k], fresh(X, w, eps, n)), f"call {k}"
    assert int(got[0][1][0]) == 36 and int(got[2][1][0]) == 0 and int(got[3][1][0]) == 1
    assert same_bits(mixed, fresh(*full, flags=0))


# ====================================================================== gradients on the resident history
def grad_cases():
    return {"N65-d1": ("res N65-d1", *R.make_case(65, 1, seed=0), 0.1, 50),
            "N100-d2": ("res N100-d2", *R.make_case(100, 2, seed=0), 0.1, 50),
            "N128-d17": ("res N128-d17", *R.make_case(128, 17, seed=0), 1.0, 50),
            "early": ("res early N128 seed 13", *early_case(128, 3, 13)),
            "floor": ("res floor N100", *floor_case())}


@pytest.mark.parametrize("name", ["N65-d1", "N100-d2", "N128-d17", "early", "floor"])
def test_the_backward_pass_takes_the_resident_history(name):
    ref = GR.autograd(grad_cases()[name])
    X, w, G, eps, n_iters = ref["X"], ref["w"], ref["G"], ref["eps"], ref["n_iters"]
    assert float(np.max(np.abs(ref["gX"]))) > 1e-3 and float(np.max(np.abs(ref["gw"]))) > 1e-3
    h = OT._Handle(X.shape[0], X.shape[1], 1)
    try:
        bufs = {}
        res = solve(h, X[None], w[None], eps, n_iters, bufs=bufs)
        assert int(res[1][0]) == ref["K"]
        Gd = dev(G[None])
        gX, gw = torch.full_like(bufs["X"], np.nan), torch.full_like(bufs["w"], np.nan)
        torch.cuda.synchronize()
        h.backward_dev(side_stream(), bufs["X"].data_ptr(), bufs["w"].data_ptr(), eps,
                       MIN_VAL, bufs["its"].data_ptr(), n_iters, ref["K"], bufs["hist"].data_ptr(),
                       bufs["am"].data_ptr(), Gd.data_ptr(), gX.data_ptr(), gw.data_ptr())
        torch.cuda.synchronize()
    finally:
        h.close()
    gX, gw = host(gX)[0], host(gw)[0]
    assert np.all(np.isfinite(gX)) and np.all(np.isfinite(gw))
    sx, sw = max(1.0, float(np.max(np.abs(ref["gX"])))), max(1.0, float(np.max(np.abs(ref["gw"]))))
    ex, ew = float(np.max(np.abs(gX - ref["gX"]))), float(np.max(np.abs(gw - ref["gw"])))
    print(f"ot resident grad {name}: gX error {ex:.3e} (scale {sx:.3g}), gw error {ew:.3e} (scale {sw:.3g})")
    assert ex <= TOL * sx
    assert ew <= TOL * sw


# ====================================================================== refusals
def test_the_solver_is_refused_above_128_particles():
    X, w = R.make_case(129, 2, seed=0)
    for N, want in ((128, 1), (129, 0)):
        h = OT._Handle(N, 2, 1)
        try:
            assert NV.load().pf_ot_resident_supported(h.h) == want and h.resident_supported() == bool(want)
            if not want:
                Xd, wd = dev(X[None]), dev(w[None])
                out = torch.empty_like(Xd)
                a = (0, Xd.data_ptr(), wd.data_ptr(), 0.1, 5, MIN_VAL, TOL_STOP, out.data_ptr())
                with pytest.raises(ValueError, match="PF_OT_RESIDENT needs n_particles <= 128"):
                    h.resample_dev(*a, flags=RESIDENT)
                with pytest.raises(ValueError, match="flags must be 0 or PF_OT_RESIDENT"):
                    h.resample_dev(*a, flags=2)
                h.resample_dev(*a)  # the default path is what it was
                assert bool(torch.isfinite(out).all())
        finally:
            h.close()
    assert NV.load().pf_ot_resident_supported(None) == 0
