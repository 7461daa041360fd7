"""HIP stochastic particle flow filter vs the reference's own outputs (-m gpu, MI355X).

tests/golden/spf_runs.npz holds the reference ``run_generalized_spf``'s runs on fixed seeds
(tests/golden/make_golden_spf.py); ``draws="numpy"`` replays the reference's stream, so the device
must return the reference's particles.  At the edge sizes the reference is the folded NumPy
restatement (tests/spf_restatement.py, checked against the reference by the generator and by
tests/test_spf_host.py) on the device's own draws restated with ``oracle.philox``.

Tolerance (fp64): the device sums a row in another order than NumPy, with fused multiply-adds, and
its Box-Muller uses the device library's log / sincospi, so agreement is to rounding carried
through the steps: particles within 1e-9 x max(1, max|x|), the tolerance of the other fp64 flows
(tests/test_gpu_edh.py, tests/test_gpu_kpf.py) and 100 x the folding gap the generator asserts.
The schedule is bitwise the reference's.
"""

import os

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import stochastic_pf as SP
from tests import spf_restatement as SR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(__file__)
GOLD = np.load(os.path.join(HERE, "golden", "spf_runs.npz"))
NAMES = [str(n) for n in GOLD["names"]]
TOL = 1e-9

# N x n x n_steps: the full cross
EDGES = [(N, n, k) for k in SR.EDGE_STEPS for N in SR.EDGE_N for n in SR.EDGE_DIM]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert NV.device_count() > 0, "no HIP device visible: -m gpu tests must run on an MI355X"


def philox_reference(model, params, seed, N):
    draw = SR.philox_draws(seed, N, model.n)
    return SR.folded(params, SR.prior(model, draw), draw, model.n)


def engine_run(model, params, seed, N, splits=None, Z=None, X0=None):
    """Engine-level run: prior on the device (or X0), then the steps in one call or split."""
    with SP.SpfEngine(N, model.n) as eng:
        if X0 is None:
            eng.draw_prior(model.m0, np.linalg.cholesky(model.P0), seed)
        else:
            eng.set_particles(X0)
        k0 = 0
        for steps in splits or [params.shape[0]]:
            eng.advance(params[k0:k0 + steps], k0, seed, None if Z is None else Z[k0:k0 + steps])
            k0 += steps
        assert k0 == params.shape[0]
        return eng.particles()


@pytest.mark.parametrize("name", NAMES)
def test_golden_case(name):
    model, kw, g = SR.golden_case(GOLD, name)
    X, x_hat, info = SP.run_generalized_spf(model, draws="numpy", **kw)
    scale = max(1.0, float(np.max(np.abs(g["X"]))))
    err = float(np.max(np.abs(X - g["X"])))
    print(f"SPF golden {name}: max particle error {err:.3e} (scale {scale:.3g})")
    assert X.shape == (kw["N"], model.n) and X.dtype == np.float64
    assert np.all(np.isfinite(X))
    assert err <= TOL * scale
    assert np.array_equal(x_hat, X.mean(axis=0))
    assert np.max(np.abs(x_hat - g["x_hat"])) <= TOL * scale
    assert sorted(info) == ["beta", "betadot", "lam"]
    for k in info:
        assert np.array_equal(info[k], g[k]), k


def test_numpy_draws_chunked_upload_is_bitwise_equal(monkeypatch):
    """The per-step normals go up in chunks of steps; 7 chunks must equal one."""
    model, kw, g = SR.golden_case(GOLD, "b_linear")
    one, _, _ = SP.run_generalized_spf(model, draws="numpy", **kw)
    monkeypatch.setattr(SP, "NUMPY_CHUNK_BYTES", 8 * kw["N"] * model.n * 8)  # 8 steps per call
    many, _, _ = SP.run_generalized_spf(model, draws="numpy", **kw)
    assert np.array_equal(one, many)


def test_schedule_argument_skips_the_solver(monkeypatch):
    model, kw, g = SR.golden_case(GOLD, "e_n9")
    monkeypatch.setattr(SP, "solve_beta_star_bisection", None)  # calling it would raise
    X, _, info = SP.run_generalized_spf(model, draws="numpy", schedule=(g["lam"], g["beta"], g["betadot"]), **kw)
    assert np.max(np.abs(X - g["X"])) <= TOL * max(1.0, float(np.max(np.abs(g["X"]))))
    assert all(np.array_equal(info[k], g[k]) for k in ("lam", "beta", "betadot"))


@pytest.mark.parametrize("N,n,n_steps", EDGES)
def test_edge_size_matches_restatement(N, n, n_steps):
    model, Q_mode, q_scale, seed, params = SR.edge_case(N, n, n_steps)
    ref = philox_reference(model, params, seed, N)
    X, x_hat, info = SP.run_generalized_spf(model, N=N, n_steps=n_steps, beta_mode="linear", Q_mode=Q_mode,
                                            q_scale=q_scale, seed=seed)
    scale = max(1.0, float(np.max(np.abs(ref))))
    err = float(np.max(np.abs(X - ref)))
    print(f"SPF edge {N}x{n}x{n_steps} {Q_mode}: max particle error {err:.3e} (scale {scale:.3g})")
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(X))
    assert err <= TOL * scale
    assert np.array_equal(info["lam"], np.linspace(0.0, 1.0, n_steps + 1))


@pytest.mark.parametrize("n", [n for n in range(1, 65) if n not in SR.EDGE_DIM])
def test_every_dimension(n):
    """The remaining dimensions (every padded instantiation, every remainder) at N = 65, two steps."""
    model, Q_mode, q_scale, seed, params = SR.edge_case(65, n, 2)
    ref = philox_reference(model, params, seed, 65)
    X = engine_run(model, params, seed, 65)
    assert np.max(np.abs(X - ref)) <= TOL * max(1.0, float(np.max(np.abs(ref))))


@pytest.mark.parametrize("N,n", [(131073, 4), (65537, 9)])
def test_wide_workgroups(N, n):
    """N large enough for the 256-lane (131073: 513 workgroups) and 128-lane (65537) launch
    geometries, with a one-particle tail."""
    model, Q_mode, q_scale, seed, params = SR.edge_case(N, n, 2)
    ref = philox_reference(model, params, seed, N)
    X = engine_run(model, params, seed, N)
    assert np.max(np.abs(X - ref)) <= TOL * max(1.0, float(np.max(np.abs(ref))))


# The workgroup is the largest of 256 / 128 / 64 lanes whose state tile fits the LDS beside the two
# parameter buffers: 256 up to n = 48, 128 up to n = 61 (where the launch takes exactly 160 KB), 64
# above; below 512 workgroups it is halved, so these sizes need N >= 65537 (128) or 131073 (256).
LDS_FIT = [(131073, 40, 256), (131073, 48, 256), (131073, 49, 128), (131073, 61, 128), (131073, 62, 64),
           (65537, 48, 128), (65537, 61, 128), (65537, 62, 64)]


@pytest.mark.parametrize("N,n,lanes", LDS_FIT)
def test_lds_fit_geometries(N, n, lanes):
    """A particle's draws depend on its index only and the geometry cannot change a result, so the
    first 1001 particles of the large run are bitwise those of an N = 1001 run (64 lanes), and the
    last 300 (the partial workgroup included) match the restatement on their slice of the draws."""
    model, _, _, seed, params = SR.edge_case(1001, n, 3)
    L0 = np.linalg.cholesky(model.P0)
    out = []
    for size, want in ((N, lanes), (1001, 64)):
        with SP.SpfEngine(size, n) as eng:
            assert eng.workgroup == want
            eng.draw_prior(model.m0, L0, seed)
            eng.advance(params, 0, seed)
            out.append(eng.particles())
    big, small = out
    assert np.all(np.isfinite(big))
    assert np.array_equal(big[:1001], small)
    draw = SR.philox_draws(seed, N, n, rows=(N - 300, N))
    ref = SR.folded(params, SR.prior(model, draw), draw, n)
    assert np.max(np.abs(big[N - 300:] - ref)) <= TOL * max(1.0, float(np.max(np.abs(ref))))


@pytest.mark.parametrize("N,n", [(65, 3), (257, 17), (64, 64)])
def test_prior_draw_matches_restatement(N, n):
    model, _, _, seed, _ = SR.edge_case(N, n, 1)
    with SP.SpfEngine(N, n) as eng:
        assert np.array_equal(eng.particles(), np.zeros((N, n)))  # a new handle's particles are zero
        eng.draw_prior(model.m0, np.linalg.cholesky(model.P0), seed)
        X0 = eng.particles()
    ref = SR.prior(model, SR.philox_draws(seed, N, n))
    assert np.max(np.abs(X0 - ref)) <= TOL * max(1.0, float(np.max(np.abs(ref))))


@pytest.mark.parametrize("N,n", [(257, 5), (65, 40), (1001, 64)])
def test_two_runs_and_split_steps_bitwise_equal(N, n):
    model, _, _, seed, params = SR.edge_case(N, n, 50)
    a = engine_run(model, params, seed, N)
    b = engine_run(model, params, seed, N)
    c = engine_run(model, params, seed, N, splits=[1, 17, 32])
    assert np.all(np.isfinite(a))
    assert np.array_equal(a, b)
    assert np.array_equal(a, c)
    # and with host normals
    rng = np.random.default_rng(3)
    Z, X0 = rng.standard_normal((50, N, n)), rng.standard_normal((N, n))
    d = engine_run(model, params, seed, N, Z=Z, X0=X0)
    e = engine_run(model, params, seed, N, Z=Z, X0=X0, splits=[1, 17, 32])
    assert np.array_equal(d, e)
    ref = SR.folded(params, X0, lambda k: Z[k - 1], n)
    assert np.max(np.abs(d - ref)) <= TOL * max(1.0, float(np.max(np.abs(ref))))


@pytest.mark.parametrize("N,n", [(65, 3), (200, 40), (65, 64)])
def test_lds_poisoned_run_is_finite_and_bitwise_equal(N, n, monkeypatch):
    """The step kernel stages the parameter blocks and the state tile in LDS; with every CU's LDS
    filled with NaN patterns in front of its launch (tests/test_gpu_lds_poison.py) no unwritten
    word (padded rows, the tail lanes of a partial workgroup) may reach a particle."""
    lib = NV.load()
    model, _, _, seed, params = SR.edge_case(N, n, 50)
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    c0 = lib.pf_test_lds_poison_count()
    clean = engine_run(model, params, seed, N)
    assert lib.pf_test_lds_poison_count() == c0
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_LDS_POISON", "1")
    got = engine_run(model, params, seed, N, splits=[1, 17, 32])
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    assert lib.pf_test_lds_poison_count() >= c0 + 3, "the poison hook never fired"
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, clean)


def test_moments_of_many_particles():
    """N = 1e5 device-drawn particles against the exact moments (m_K, P_K) of the discretised
    chain (``spf_restatement.moments``).  The final state is Gaussian, so the sample mean of
    component j has standard deviation sqrt(P_K[j, j] / N) and the sample variance has relative
    standard deviation sqrt(2 / (N - 1)); both bounds are 5 standard deviations, a false failure
    of about 6e-7 per statistic."""
    N, n, n_steps = 100_000, 4, 50
    model, Q_mode, q_scale, seed, params = SR.edge_case(N, n, n_steps)
    X, x_hat, _ = SP.run_generalized_spf(model, N=N, n_steps=n_steps, beta_mode="linear", Q_mode=Q_mode,
                                         q_scale=q_scale, seed=seed)
    m, P = SR.moments(params, model.m0, model.P0, n)
    var = X.var(axis=0, ddof=1)
    print("mean error / sd:", (x_hat - m) / np.sqrt(np.diag(P) / N), "variance ratio:", var / np.diag(P))
    assert np.all(np.abs(x_hat - m) <= 5.0 * np.sqrt(np.diag(P) / N))
    assert np.all(np.abs(var / np.diag(P) - 1.0) <= 5.0 * np.sqrt(2.0 / N))


@pytest.mark.filterwarnings("ignore:invalid value encountered")  # the mean of non-finite particles
@pytest.mark.parametrize("n_steps", [40, 120])
def test_stiff_input_returns_what_the_restatement_returns(n_steps):
    """cond(P0) = 1e6 with Q = I: the explicit Euler factor is about -1e4 per step, so the state
    is huge after 40 steps and overflows before 120.  No error is raised, and where both the
    device and the restatement are finite they agree."""
    N, n = 65, 4
    model = SR.random_model(77, n, 2, cond=1e6)
    lam = np.linspace(0.0, 1.0, n_steps + 1)
    params = SP.fold_steps(model, lam, lam.copy(), np.ones_like(lam), "scaled_identity", 1.0)
    ref = philox_reference(model, params, 5, N)
    X, x_hat, info = SP.run_generalized_spf(model, N=N, n_steps=n_steps, beta_mode="linear", Q_mode="scaled_identity",
                                            q_scale=1.0, seed=5)
    both = np.isfinite(ref) & np.isfinite(X)
    print(f"stiff {n_steps}: finite on device {np.isfinite(X).mean():.2f}, in the restatement "
          f"{np.isfinite(ref).mean():.2f}, max finite |x| {np.max(np.abs(ref[both])) if both.any() else 0:.3g}")
    assert X.shape == (N, n) and x_hat.shape == (n,)
    if n_steps == 40:
        assert both.all() and np.max(np.abs(ref)) > 1e50
    else:
        assert not np.isfinite(ref).all()
    if both.any():
        scale = max(1.0, float(np.max(np.abs(ref[both]))))
        assert np.max(np.abs(X[both] - ref[both])) <= TOL * scale


def test_unsupported_dimension_raises():
    with pytest.raises(NotImplementedError, match="1 <= n <= 64"):
        SP.SpfEngine(10, 65)
    with pytest.raises(ValueError):
        SP.SpfEngine(0, 4)
    with SP.SpfEngine(5, 3) as eng:
        with pytest.raises(ValueError):
            eng.set_particles(np.zeros((5, 4)))
        with pytest.raises(ValueError):
            eng.advance(np.zeros((2, 5)))
        eng.advance(np.zeros((0, 2 * 9 + 3)))  # no steps: a no-op
        assert np.array_equal(eng.particles(), np.zeros((5, 3)))
