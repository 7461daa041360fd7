"""Soft (Gumbel-Softmax) resampler and DifferentiableParticleFilter on the device vs the NumPy
restatement (-m gpu, MI355X).

TensorFlow is not available, so there is no fixture of reference outputs: the device is compared
with tests/dpf_soft_restatement.py, the reference's formulas in fp64 on the same Philox draws, which
tests/test_dpf_soft_host.py checks against the literal loop.

The kernels' constants are the ones the plan names: 64 output rows per workgroup and 64 sources per
LDS tile, component chunks of 16, a split grain of 32 sources.  pf_soft_create splits the source
range from N = 33 on: S0 = min(ceil(N / 32), 8192 / ceil(N / 64), 64), chunk = ceil(N / S0) rounded
up to 32, S = ceil(N / chunk): N = 65 has S = 3, N = 130 S = 5, N = 300 S = 10, all with chunk = 32,
so unhooked no case here runs the tile loop more than once inside a split.  The hooked runs do
(PF_TEST_HOOKS=1): PF_TEST_SOFT_SPLITS=1 at N = 300 is one split of 5 tiles (64 x 4 + 44) and
nothing merged but the single partial; =2 is chunk = 160 (tiles 64 + 64 + 32 and 64 + 64 + 12), =3
chunk = 128 (64 + 64, 64 + 64, 44), each followed by a merge - what the library does unhooked from
N = 4097 on.

Bounds (fp64 engine, the 1e-9 x scale bound of the other fp64 filters): particles within
1e-9 max(1, max|X_ref|), row entropies within 1e-9 max(1, max|H_ref|), Gumbels within
1e-9 max(1, |G|); the uniforms are bitwise the restatement's.  The device sums in another order, keeps
a running maximum (an online softmax) where NumPy takes the maximum first, multiplies by 1 / T where
NumPy divides, and uses the device library's exp and log.

Largest errors measured on an MI355X: DESIGN.md section 4, "Soft resampling and
DifferentiableParticleFilter".
"""

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_soft as SO
from tests import dpf_soft_restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert NV.device_count() > 0, "no HIP device visible: -m gpu tests must run on an MI355X"


def lp_of(lw, alpha):
    return np.ascontiguousarray(SO._log_probs(SO._log_normalize(np.asarray(lw, dtype=float))[0], float(alpha)))


def _batched(X, lw):
    X = np.ascontiguousarray(X, dtype=float)
    lw = np.ascontiguousarray(lw, dtype=float)
    return (X, lw) if X.ndim == 3 else (X[None], lw[None])


def call(h, X, lw, alpha, T, seed=0, epoch=0, batch_base=0, want_entropy=True):
    Xb, lwb = _batched(X, lw)
    return h.resample(Xb, lp_of(lwb, alpha), T, seed, epoch, batch_base, want_entropy)


def device(X, lw, alpha, T, seed=0, epoch=0, batch_base=0, want_entropy=True):
    """(X_out [B][N][d], H [B][N] or None) of one pf_soft_resample call on a fresh handle."""
    Xb, lwb = _batched(X, lw)
    h = SO._Handle(Xb.shape[1], Xb.shape[2], Xb.shape[0])
    try:
        return call(h, Xb, lwb, alpha, T, seed, epoch, batch_base, want_entropy)
    finally:
        h.close()


def compare(tag, out, H, ref):
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(H))
    sx = max(1.0, float(np.max(np.abs(ref["particles"]))))
    sh = max(1.0, float(np.max(np.abs(ref["entropy"]))))
    ex = float(np.max(np.abs(out - ref["particles"])))
    eh = float(np.max(np.abs(H - ref["entropy"])))
    print(f"soft {tag}: particle error {ex:.3e} (scale {sx:.3g}), entropy error {eh:.3e} (scale {sh:.3g})")
    assert ex <= TOL * sx
    assert eh <= TOL * sh


# ------------------------------------------------------------------ 1. draws
@pytest.mark.parametrize("N", [1, 2, 3, 65])
@pytest.mark.parametrize("epoch", [0, 3])
def test_draws_are_the_restatements(N, epoch):
    seed, B, base = 0x1234567890ABCDEF, 2, 7
    for bb, nb in ((0, 1), (base, B)):
        h = SO._Handle(N, 1, nb)
        try:
            U, G = h.draws(seed, epoch, bb)
        finally:
            h.close()
        for b in range(nb):
            Ur, Gr = R.draws(N, seed, epoch, bb + b)
            assert np.array_equal(U[b], Ur), f"U differs at N={N} epoch={epoch} problem={bb + b}"
            err = float(np.max(np.abs(G[b] - Gr) / np.maximum(1.0, np.abs(Gr))))
            print(f"soft draws N={N} epoch={epoch} problem={bb + b}: G error {err:.3e}")
            assert err <= TOL


def test_draws_accepts_one_null_output_and_rejects_two():
    h = SO._Handle(3, 1, 1)
    try:
        U = np.zeros((1, 3, 3))
        lib = NV.load()
        assert lib.pf_soft_draws(h.h, 5, 0, 0, NV.dptr(U), None) == NV.PF_OK
        assert np.array_equal(U[0], R.draws(3, 5, 0, 0)[0])
        assert lib.pf_soft_draws(h.h, 5, 0, 0, None, None) == NV.PF_E_ARG
    finally:
        h.close()


# ------------------------------------------------------------------ 2. parity
@pytest.mark.parametrize("case", R.PARITY, ids=lambda c: f"N{c[0]}-d{c[1]}-a{c[2]}-T{c[3]}-{c[4]}")
def test_parity(case):
    N, d, alpha, T, kind, seed, epoch = case
    X, lw, ref = R.solved(*case)
    out, nlw, H = SO.soft_resample(X, lw, alpha, T, seed=seed, epoch=epoch, return_diagnostics=True)
    assert out.dtype == np.float64 and out.shape == (N, d) and H.shape == (N,)
    assert np.array_equal(nlw, np.log(np.full(N, 1.0 / N)))
    compare(f"N={N} d={d} alpha={alpha} T={T} {kind}", out, H, ref)
    out2, nlw2 = SO.soft_resample(X, lw, alpha, T, seed=seed, epoch=epoch)
    assert np.array_equal(out2, out)


# ------------------------------------------------------------------ 3. forced splits
@pytest.mark.parametrize("N,d,splits", [(300, 17, "1"), (300, 17, "2"), (300, 17, "3"), (130, 2, "1")])
def test_forced_splits(N, d, splits, monkeypatch):
    alpha, T, seed, epoch = 0.1, 0.2, 21, 1
    X, lw, ref = R.solved(N, d, alpha, T, "normal", seed, epoch)
    monkeypatch.delenv("PF_TEST_SOFT_SPLITS", raising=False)
    plain, Hp = device(X, lw, alpha, T, seed, epoch)
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_SOFT_SPLITS", splits)
    out, H = device(X, lw, alpha, T, seed, epoch)
    compare(f"N={N} d={d} PF_TEST_SOFT_SPLITS={splits}", out[0], H[0], ref)
    compare(f"N={N} d={d} unhooked", plain[0], Hp[0], ref)
    assert not np.array_equal(out, plain)  # the hook took effect: another summation order


# ------------------------------------------------------------------ 4. bitwise properties
BATCH = dict(N=130, d=17, alpha=0.1, T=0.2, seed=31, epoch=2)  # two component chunks, five splits


def _batch_inputs():
    c = BATCH
    cases = [R.make_case(c["N"], c["d"], seed=100 + b) for b in range(3)]
    return np.stack([x for x, _ in cases]), np.stack([w for _, w in cases])


def test_a_batch_is_bitwise_the_problems_alone_and_matches_the_restatement():
    c = BATCH
    X, lw = _batch_inputs()
    out, H = device(X, lw, c["alpha"], c["T"], c["seed"], c["epoch"])
    for b in range(3):
        o1, H1 = device(X[b], lw[b], c["alpha"], c["T"], c["seed"], c["epoch"], batch_base=b)
        assert np.array_equal(o1[0], out[b]) and np.array_equal(H1[0], H[b]), f"problem {b}"
        compare(f"batch problem {b}", out[b], H[b],
                R.soft_resample(X[b], lw[b], c["alpha"], c["T"], c["seed"], c["epoch"], b))
    assert not np.array_equal(device(X[1], lw[1], c["alpha"], c["T"], c["seed"], c["epoch"])[0][0], out[1])


def test_a_batch_with_a_base_is_the_shifted_problems():
    c = BATCH
    X, lw = _batch_inputs()
    out, H = device(X[:2], lw[:2], c["alpha"], c["T"], c["seed"], c["epoch"], batch_base=1000)
    for b in range(2):
        ref = R.soft_resample(X[b], lw[b], c["alpha"], c["T"], c["seed"], c["epoch"], 1000 + b)
        compare(f"batch_base 1000 problem {b}", out[b], H[b], ref)


def test_x_out_does_not_depend_on_the_entropy_request():
    c = BATCH
    X, lw = _batch_inputs()
    with_h, H = device(X, lw, c["alpha"], c["T"], c["seed"], c["epoch"])
    without, none = device(X, lw, c["alpha"], c["T"], c["seed"], c["epoch"], want_entropy=False)
    assert none is None and np.array_equal(with_h, without)


def test_a_reused_handle_gives_the_bits_of_a_fresh_one_and_equal_calls_are_equal():
    c = BATCH
    X, lw = _batch_inputs()
    X0 = X[0] + 30.0
    calls = [  # (X, lw, alpha, T, seed, epoch, want_entropy)
        (X[0], lw[0], 0.1, 0.2, 1, 0, True),
        (X[1], lw[1], 0.0, 1.0, 2, 5, False),
        (X0, lw[2], 1.0, 0.2, 1 << 40, 0, True),
        (X[2], 10.0 * lw[0], 0.1, 1e-3, 3, 1, True),
        (X[0], lw[0], 0.1, 0.2, 1, 0, True),   # the first call again
        (X[1], lw[2], 0.5, 5.0, 4, 0xFFFFFFFF, False),
    ]
    h = SO._Handle(c["N"], c["d"], 1)
    try:
        got = [call(h, x, w, a, T, s, e, 0, we) for x, w, a, T, s, e, we in calls]
    finally:
        h.close()
    for k, (x, w, a, T, s, e, we) in enumerate(calls):
        fresh = device(x, w, a, T, s, e, 0, we)
        assert np.array_equal(got[k][0], fresh[0]), f"call {k}"
        assert (got[k][1] is None) == (not we)
        if we:
            assert np.array_equal(got[k][1], fresh[1]), f"call {k}"
    assert np.array_equal(got[0][0], got[4][0]) and np.array_equal(got[0][1], got[4][1])


# ------------------------------------------------------------------ 5. reference-free checks
def test_equal_particles_stay_where_they_are():
    N, d = 130, 17
    _, lw = R.make_case(N, d, seed=3)
    c = 30.0 + np.arange(d) * 0.37
    X = np.tile(c, (N, 1))
    out, H = device(X, lw, 0.1, 0.2, 4, 0)
    err = float(np.max(np.abs(out[0] - c)))
    print(f"soft equal particles: error {err:.3e} (scale {np.max(np.abs(c)):.3g})")
    assert err <= TOL * float(np.max(np.abs(c)))


def test_a_constant_added_to_the_log_weights_changes_nothing():
    N, d = 130, 5
    X, lw = R.make_case(N, d, seed=6)
    a, _ = SO.soft_resample(X, lw, 0.1, 0.2, seed=7, epoch=1)
    b, _ = SO.soft_resample(X, lw + 123.456, 0.1, 0.2, seed=7, epoch=1)
    err = float(np.max(np.abs(a - b)))
    print(f"soft shifted log-weights: difference {err:.3e}")
    assert err <= TOL * max(1.0, float(np.max(np.abs(a))))


def test_hard_limit_picks_the_gumbel_max_ancestor():
    """T = 1e-3: on every row whose top-two gap in (log q + G) exceeds 0.04 the leading weight is at
    least 1 - N e^-40 and the row is X[argmax].  tests/test_dpf_soft_host.py asserts that at least 90 %
    of the rows qualify."""
    c = R.HARD
    X, lw, anc, gap = R.hard_case()
    ok = gap > c["gap"]
    assert ok.mean() >= c["share"]
    out, H = device(X, lw, c["alpha"], c["T"], c["seed"], c["epoch"])
    err = float(np.max(np.abs(out[0][ok] - X[anc[ok]])))
    scale = max(1.0, float(np.max(np.abs(X))))
    print(f"soft hard limit: {int(ok.sum())} rows, error {err:.3e} (scale {scale:.3g})")
    assert err <= TOL * scale
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(H))


def test_argument_errors_that_need_a_handle():
    lib = NV.load()
    h = SO._Handle(4, 2, 2)
    try:
        X, lp, out = np.zeros((2, 4, 2)), np.zeros((2, 4)), np.zeros((2, 4, 2))
        args = (NV.dptr(X), NV.dptr(lp))
        for T in (0.0, -1.0, float("inf"), float("nan")):
            assert lib.pf_soft_resample(h.h, *args, T, 0, 0, 0, NV.dptr(out), None) == NV.PF_E_ARG
        assert lib.pf_soft_resample(h.h, *args, 0.2, 0, 0, (1 << 24) - 1, NV.dptr(out), None) == NV.PF_E_ARG
        assert lib.pf_soft_resample(h.h, *args, 0.2, 0, 0, (1 << 24) - 2, NV.dptr(out), None) == NV.PF_OK
        assert lib.pf_soft_resample(h.h, None, args[1], 0.2, 0, 0, 0, NV.dptr(out), None) == NV.PF_E_ARG
        assert lib.pf_soft_resample(h.h, args[0], None, 0.2, 0, 0, 0, NV.dptr(out), None) == NV.PF_E_ARG
        assert lib.pf_soft_resample(h.h, *args, 0.2, 0, 0, 0, None, None) == NV.PF_E_ARG
        assert lib.pf_soft_draws(h.h, 0, 0, (1 << 24) - 1, NV.dptr(np.zeros((2, 4, 4))), None) == NV.PF_E_ARG
        assert lib.pf_soft_stream(h.h) and lib.pf_soft_synchronize(h.h) == NV.PF_OK
    finally:
        h.close()


# ------------------------------------------------------------------ 6. the class
def _filters(seed):
    N, d = 50, 2
    dev = SO.DifferentiableParticleFilter(N, d, *R.linear_model(8), seed=seed, rng=np.random.default_rng(2))
    host = SO.DifferentiableParticleFilter(N, d, *R.linear_model(8), seed=seed, rng=np.random.default_rng(2))
    host._resample = R.resample_fn
    return dev, host


def test_filter_equals_the_same_loop_with_the_restatement_as_resampler():
    B, T, N, d = 2, 5, 50, 2
    dev, host = _filters(seed=17)
    obs = np.random.default_rng(4).standard_normal((B, T, d))
    truth = np.zeros((B, T + 1, d))
    try:
        ps, lws, dg = dev.filter(obs, np.zeros(d), np.eye(d), return_diagnostics=True, ground_truth=truth)
        handle = dev._h
        assert handle is not None and (handle.B, handle.N, handle.d) == (B, N, d)
    finally:
        dev.close()
    pr, lwr, dr = host.filter(obs, np.zeros(d), np.eye(d), return_diagnostics=True, ground_truth=truth)
    assert ps.shape == (B, T + 1, N, d) and lws.shape == (B, T + 1, N) and ps.dtype == np.float64
    assert np.array_equal(ps[:, 0], pr[:, 0]) and np.array_equal(lws, lwr)
    for t in range(1, T + 1):
        scale = max(1.0, float(np.max(np.abs(pr[:, t]))))
        err = float(np.max(np.abs(ps[:, t] - pr[:, t])))
        print(f"soft filter step {t}: error {err:.3e} (scale {scale:.3g})")
        assert err <= TOL * scale
    assert dev.epoch == T and host.epoch == T
    assert set(dg) == set(dr)
    for key in ("ess_before_mean", "ess_after_mean", "entropy_before_mean", "entropy_after_mean",
                "assignment_entropy_mean_mean", "assignment_entropy_std_mean", "max_weight_before_max",
                "soft_alpha_mean", "gumbel_temperature_std", "step_time_mean", "total_time", "mean_step_time",
                "rmse_sequence", "mean_rmse", "final_rmse", "diversity_before", "diversity_after"):
        assert key in dg, key
    for key in ("assignment_entropy_mean_mean", "assignment_entropy_std_mean", "assignment_entropy_mean_min",
                "assignment_entropy_mean_max"):
        print(f"soft filter {key}: {dg[key]:.15g} vs {dr[key]:.15g}")
        assert abs(dg[key] - dr[key]) <= TOL * max(1.0, abs(dr[key]))
    assert np.max(np.abs(dg["rmse_sequence"] - dr["rmse_sequence"])) <= TOL


def test_step_equals_the_restatement_keeps_its_handle_and_rebuilds_it_for_another_batch():
    N, d = 50, 2
    dev, host = _filters(seed=5)
    try:
        p0, lw0 = dev.init_particles(2, np.zeros(d), np.eye(d))
        host.init_particles(2, np.zeros(d), np.eye(d))  # the same draw, to keep the two rngs in step
        y = np.array([[0.3, -0.1], [0.0, 0.4]])
        new, nlw, dg = dev.step(p0, lw0, y, return_diagnostics=True)
        ref, rlw, dr = host.step(p0, lw0, y, return_diagnostics=True)
        assert np.max(np.abs(new - ref)) <= TOL * max(1.0, float(np.max(np.abs(ref)))) and np.array_equal(nlw, rlw)
        assert set(dg) == set(dr) == {"ess_before", "ess_after", "entropy_before", "entropy_after",
                                      "diversity_before", "diversity_after", "assignment_entropy_mean",
                                      "assignment_entropy_std", "max_weight_before", "soft_alpha",
                                      "gumbel_temperature"}
        assert abs(dg["assignment_entropy_mean"] - dr["assignment_entropy_mean"]) <= TOL
        assert dev.epoch == 1
        first = dev._h
        dev.step(new, nlw, y)
        assert dev._h is first and dev.epoch == 2
        p3, lw3 = dev.init_particles(3, np.zeros(d), np.eye(d))
        out3, _ = dev.step(p3, lw3, np.zeros((3, d)))
        assert dev._h is not first and dev._h.B == 3 and out3.shape == (3, N, d) and dev.epoch == 3
        with pytest.raises(ValueError):
            dev.step(np.full((3, N, d), np.nan), lw3, np.zeros((3, d)))
        assert dev.epoch == 3
    finally:
        dev.close()
