"""GPU tests of the dense EDH path (sensor-network models; csrc/pf_edh_dense_kernels.h).

* reference parity: every case of tests/golden/sn_edh_runs.npz (the reference's EDHFlowPF with its
  UKF tracker) through ``EDHFlowPF.step`` with the mirrored tracker, at the EDH tolerances of
  tests/test_gpu_edh.py (particles / means 1e-9 of the state scale, covariances 1e-8, weights rtol
  1e-7, condition numbers rtol 1e-6, decisions identical); ``run()`` bitwise equal to the step loop;
* exact products: small-integer data through set_state / step, where the fp64 matrix-core product is
  exact, so a wrong fragment map or tile edge cannot hide behind a rounding tolerance;
* edge shapes on random data against the NumPy restatement (tests/sn_edh_restatement.py);
* reproducibility, the LDS poison hook, and the error paths.
"""

import ctypes as C

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import edh as E
from particle_filters_amd import models as M
from tests import sn_edh_restatement as RS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return RS.load()


# ---------------------------------------------------------------- C-ABI helpers
class Handle:
    def __init__(self, d, N, *, alpha=0.9, obs="identity", m1=1.0, m2=0.0, like="gaussian", rdiag=None, Q=None,
                 ratio=0.5):
        self.d, self.N = d, N
        self.lib = NV.load()
        Q = np.ascontiguousarray(np.eye(d) if Q is None else Q, dtype=float)
        rd = None
        if like == "gaussian":
            rd = np.ascontiguousarray(np.ones(d) if rdiag is None else rdiag, dtype=float)
        model = NV.EdhDenseModel(d, NV.PF_EDH_OBS_EXP if obs == "exp" else NV.PF_EDH_OBS_IDENTITY,
                                 NV.PF_EDH_LIKE_POISSON if like == "poisson" else NV.PF_EDH_LIKE_GAUSSIAN, 0,
                                 alpha, m1, m2, NV.dptr(rd), NV.dptr(Q))
        opts = NV.EdhDenseOpts(N, ratio, 0, 0)
        self.h = C.c_void_p()
        NV.check(self.lib.pf_edh_dense_create(C.byref(model), C.byref(opts), C.byref(self.h)), "create")

    def close(self):
        if self.h is not None:
            self.lib.pf_edh_dense_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def set_state(self, X, w):
        X = np.ascontiguousarray(X, dtype=float)
        w = np.ascontiguousarray(w, dtype=float)
        NV.check(self.lib.pf_edh_dense_set_state(self.h, NV.dptr(X), NV.dptr(w)), "set_state")

    def step(self, Mc, cc, z, u=None, v=None):
        c_ = lambda a: None if a is None else np.ascontiguousarray(a, dtype=float)  # noqa: E731
        Mc, cc, z, u, v = c_(Mc), c_(cc), c_(z), c_(u), c_(v)
        info = NV.LedhInfo()
        st = self.lib.pf_edh_dense_step(self.h, NV.dptr(Mc), NV.dptr(cc), NV.dptr(z), NV.dptr(u),
                                        NV.PF_NOISE_NONE if v is None else NV.PF_NOISE_HOST, NV.dptr(v), C.byref(info))
        return st, float(info.ess), bool(info.resample)

    def finish(self, U=None):
        mean, cov = np.empty(self.d), np.empty((self.d, self.d))
        Ua = None if U is None else np.array([float(U)])
        NV.check(self.lib.pf_edh_dense_finish(self.h, NV.dptr(Ua), NV.dptr(mean), NV.dptr(cov)), "finish")
        return mean, cov

    def particles(self):
        out = np.empty((self.N, self.d))
        NV.check(self.lib.pf_edh_dense_get_particles(self.h, NV.dptr(out)), "get_particles")
        return out

    def weights(self):
        out = np.empty(self.N)
        NV.check(self.lib.pf_edh_dense_get_weights(self.h, NV.dptr(out)), "get_weights")
        return out


# ---------------------------------------------------------------- reference parity
def _filter(c, rng):
    g, h, lt, ll, R = c.objects()
    return E.EDHFlowPF(c.tracker(g, h, R), g, h, h.jacobian, lt, ll, R, c.config(rng))


def _initial(c):
    return E.PFState(particles=c.init.copy(), weights=np.full(c.N, 1.0 / c.N), mean=np.zeros(c.d), cov=c.Q.copy())


def _step_loop(c):
    pf = _filter(c, RS.ReplayUniforms(c.U))
    noise = iter(c.V) if c.V is not None else None
    sampler = (lambda n, nx: next(noise)) if noise is not None else None
    st, out = _initial(c), []
    for t in range(c.T):
        st = pf.step(st, c.Z[t], process_noise_sampler=sampler)
        out.append(dict(mean=st.mean.copy(), cov=st.cov.copy(), ess=pf.last_ess, flag=pf.last_resampled,
                        conds=list(st.diagnostics["condition_numbers"]), weights=st.weights.copy(),
                        particles=st.particles.copy()))
    return out


@pytest.fixture(scope="module")
def step_runs(golden):
    return {name: _step_loop(RS.Case(golden, name)) for name in RS.CASES}


@pytest.mark.parametrize("name", list(RS.CASES))
def test_step_matches_the_reference(golden, step_runs, name):
    c = RS.Case(golden, name)
    covs, parts = c.stored("covs"), c.stored("particles")
    scale = max(1.0, float(np.abs(c.k("means")).max()))
    err = dict(x=0.0, cov=0.0, w=0.0)
    for t, r in enumerate(step_runs[name]):
        assert r["flag"] == bool(c.k("flags")[t]), f"t={t}: resample decision"
        err["x"] = max(err["x"], np.abs(r["mean"] - c.k("means")[t]).max() / scale)
        big = c.k("weights")[t] > 1e-6
        err["w"] = max(err["w"], (np.abs(r["weights"] - c.k("weights")[t])[big] / c.k("weights")[t][big]).max())
        if t in covs:
            err["cov"] = max(err["cov"], np.abs(r["cov"] - covs[t]).max() / max(1.0, np.abs(covs[t]).max()))
        if t in parts:
            err["x"] = max(err["x"], np.abs(r["particles"] - parts[t]).max() / scale)
    print(f"{name}: GPU vs reference x {err['x']:.2e} w(rel) {err['w']:.2e} cov {err['cov']:.2e}")
    for t, r in enumerate(step_runs[name]):
        np.testing.assert_allclose(r["mean"], c.k("means")[t], rtol=0, atol=RS.TOL_X * scale, err_msg=f"mean t={t}")
        np.testing.assert_allclose(r["weights"], c.k("weights")[t], rtol=RS.RTOL_W, atol=1e-13, err_msg=f"w t={t}")
        np.testing.assert_allclose(r["ess"], c.k("ess")[t], rtol=RS.RTOL_W, err_msg=f"ess t={t}")
        np.testing.assert_allclose(r["conds"], c.k("conds")[t], rtol=RS.RTOL_COND)
        if t in covs:
            cs = max(1.0, float(np.abs(covs[t]).max()))
            np.testing.assert_allclose(r["cov"], covs[t], rtol=0, atol=RS.TOL_COV * cs, err_msg=f"cov t={t}")
        if t in parts:
            np.testing.assert_allclose(r["particles"], parts[t], rtol=0, atol=RS.TOL_X * scale, err_msg=f"x t={t}")


@pytest.mark.parametrize("name", list(RS.CASES))
def test_run_is_bitwise_the_step_loop(golden, step_runs, name):
    c = RS.Case(golden, name)
    pf = _filter(c, np.random.default_rng(0))
    U = np.where(np.isfinite(c.U), c.U, 0.0)
    res = pf.run(_initial(c), c.Z, process_noise="host" if c.V is not None else "none", replay=(c.V, U))
    loop = step_runs[name]
    np.testing.assert_array_equal(res.means, np.array([r["mean"] for r in loop]))
    np.testing.assert_array_equal(res.covs, np.array([r["cov"] for r in loop]))
    np.testing.assert_array_equal(res.ess, np.array([r["ess"] for r in loop]))
    np.testing.assert_array_equal(res.flags, np.array([r["flag"] for r in loop]))
    np.testing.assert_array_equal(pf.state.particles, loop[-1]["particles"])
    np.testing.assert_array_equal(pf.state.weights, loop[-1]["weights"])


def test_init_from_gaussian_uploads_the_host_draw():
    d, N = 5, 33
    g, h = M.ScaleTransition(0.9, d), M.IdentityObservation(d)
    Q = np.eye(d)
    from particle_filters_amd import trackers as TR

    tr = TR.UKFTracker(TR.UnscentedKalmanFilter(g, h, Q, Q), TR.UKFState(np.zeros(d), Q.copy(), 0))
    pf = E.EDHFlowPF(tr, g, h, h.jacobian, M.GaussianTransitionDensity(g, Q), M.GaussianLikelihood(h, Q), Q,
                     E.EDHConfig(n_particles=N, rng=np.random.default_rng(4)))
    st = pf.init_from_gaussian(np.arange(d, dtype=float), 2.0 * Q)
    want = np.arange(d) + np.random.default_rng(4).multivariate_normal(np.zeros(d), 2.0 * Q, size=N)
    np.testing.assert_array_equal(st.particles, want)
    np.testing.assert_array_equal(pf._download("particles"), want)
    np.testing.assert_array_equal(pf._download("weights"), np.full(N, 1.0 / N))
    st2 = pf.step(st, np.zeros(d))
    assert np.all(np.isfinite(st2.mean)) and pf.last_ess > 0.0
    st3 = pf.step(st2, np.zeros(d))
    with pytest.raises(RuntimeError, match="stale"):
        st2.particles  # never fetched, and the filter has advanced
    assert st3.particles.shape == (N, d) and abs(st3.weights.sum() - 1.0) < 1e-12


def test_diagnostics_and_zero_prior_weights_on_the_dense_path():
    """filter_diagnostics reduces the fetched state (the dense handle is no pf_ledh_handle), and an
    all-zero prior weight vector is the reference's log(0 + 1e-300): a uniform prior, not an error."""
    from particle_filters_amd import diagnostics as DG
    from particle_filters_amd import trackers as TR

    d, N = 5, 40
    g, h, Q = M.ScaleTransition(0.9, d), M.IdentityObservation(d), np.eye(d)
    R = 25.0 * np.eye(d)
    rng = np.random.default_rng(8)
    X, z = rng.normal(size=(N, d)), rng.normal(size=d)
    out = []
    for w0 in (np.zeros(N), np.full(N, 1.0 / N)):
        tr = TR.UKFTracker(TR.UnscentedKalmanFilter(g, h, Q, R), TR.UKFState(np.zeros(d), Q.copy(), 0))
        pf = E.EDHFlowPF(tr, g, h, h.jacobian, M.GaussianTransitionDensity(g, Q), M.GaussianLikelihood(h, R), R,
                         E.EDHConfig(n_particles=N, resample_ess_ratio=0.0))
        st = pf.step(E.PFState(X.copy(), w0, np.zeros(d), Q.copy()), z)
        out.append((st.weights.copy(), st.particles.copy(), pf))
    # log(0 + 1e-300) = -690.8 against log(1 / N): the same weights after max-subtraction, up to the
    # rounding of sums of magnitude 691 (691 * 2^-53 = 7.7e-14 each, a few of them per log-weight)
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(out[0][1], out[1][1])
    pf = out[1][2]
    dg = DG.compute_diagnostics(pf, resampled=False)
    w = out[1][0]
    np.testing.assert_allclose(dg["ess"], 1.0 / np.sum(w * w), rtol=1e-9)
    np.testing.assert_allclose(dg["max_weight"], w.max(), rtol=1e-12)
    np.testing.assert_allclose(dg["posterior_spread"], np.trace(pf.state.cov), rtol=1e-12)
    assert pf.shared_jacobian_path is False


# ---------------------------------------------------------------- exact products
EXACT_D = (1, 3, 4, 15, 16, 17, 33, 64, 65)
EXACT_N = (1, 63, 64, 65, 257)


@pytest.mark.parametrize("d", EXACT_D)
def test_integer_products_are_exact(d):
    rng = np.random.default_rng(100 + d)
    for N in EXACT_N:
        X = rng.integers(-8, 9, size=(N, d)).astype(float)
        Mc = rng.integers(-4, 5, size=(d, d)).astype(float)
        cc = rng.integers(-5, 6, size=d).astype(float)
        hd = Handle(d, N, alpha=2.0, ratio=0.0)
        hd.set_state(X, np.full(N, 1.0 / N))
        st, _, flag = hd.step(Mc, cc, np.zeros(d))
        assert st == NV.PF_OK and not flag
        hd.finish()
        np.testing.assert_array_equal(hd.particles(), (2.0 * X) @ Mc.T + cc, err_msg=f"d={d} N={N}")
        hd.close()


# ---------------------------------------------------------------- edge shapes against the restatement
EDGE_D = (1, 5, 17, 65, 144)
EDGE_N = (1, 65, 257)


def _spd(rng, d, cond=1e4):
    Qm, _ = np.linalg.qr(rng.normal(size=(d, d)))
    ev = np.exp(np.linspace(0.0, -np.log(cond), d)) if d > 1 else np.ones(1)
    Q = (Qm * ev) @ Qm.T
    return 0.5 * (Q + Q.T)


def _edge_inputs(d, N, like, noisy, seed):
    rng = np.random.default_rng(seed)
    Q = _spd(rng, d)
    Lc = np.linalg.cholesky(Q)
    X = rng.standard_normal((N, d)) @ Lc.T
    w = rng.uniform(0.5, 1.5, N)
    w /= w.sum()
    Mc = np.eye(d) * 0.8 + 0.2 * rng.normal(size=(d, d)) / np.sqrt(d)
    cc = 0.1 * rng.normal(size=d)
    v = 0.3 * rng.standard_normal((N, d)) @ Lc.T if noisy else None
    u = 0.05 * rng.normal(size=d) if noisy else None
    if like == "poisson":
        model = dict(alpha=0.9, obs="exp", m1=1.0, m2=1.0 / 3.0, like="poisson", rdiag=None, Q=Q)
        z = rng.poisson(1.2, d).astype(float)
    else:
        model = dict(alpha=0.9, obs="identity", m1=1.0, m2=0.0, like="gaussian", rdiag=rng.uniform(20.0, 60.0, d), Q=Q)
        z = rng.normal(size=d)
    U = float(rng.random())
    return X, w, Mc, cc, z, u, v, U, model


@pytest.mark.parametrize("N", EDGE_N)
@pytest.mark.parametrize("d", EDGE_D)
def test_edge_shapes_match_the_restatement(d, N):
    for like in ("poisson", "gaussian"):
        for noisy in (False, True):
            for seed in range(1000 * d + N, 1000 * d + N + 50):  # the first seed with a safe decision margin
                X, w, Mc, cc, z, u, v, U, model = _edge_inputs(d, N, like, noisy, seed)
                ref = RS.dense_step(X, w, Mc, cc, z, model, v=v, u=u, ratio=0.5, U=U)
                if abs(ref["ess"] - 0.5 * N) / N >= 1e-3:
                    break
            assert abs(ref["ess"] - 0.5 * N) / N >= 1e-3
            hd = Handle(d, N, alpha=model["alpha"], obs=model["obs"], m1=model["m1"], m2=model["m2"], like=like,
                        rdiag=model["rdiag"], Q=model["Q"], ratio=0.5)
            hd.set_state(X, w)
            st, ess, flag = hd.step(Mc, cc, z, u=u, v=v)
            assert st == NV.PF_OK
            mean, cov = hd.finish(U)
            tag = f"d={d} N={N} {like} noisy={noisy} resampled={ref['flag']}"
            assert flag == ref["flag"], tag
            scale = max(1.0, float(np.abs(ref["particles"]).max()))
            np.testing.assert_allclose(ess, ref["ess"], rtol=RS.RTOL_W, err_msg=tag)
            np.testing.assert_allclose(hd.particles(), ref["particles"], rtol=0, atol=RS.TOL_X * scale, err_msg=tag)
            np.testing.assert_allclose(hd.weights(), ref["weights"], rtol=RS.RTOL_W, atol=1e-13, err_msg=tag)
            np.testing.assert_allclose(mean, ref["mean"], rtol=0, atol=RS.TOL_X * scale, err_msg=tag)
            cs = max(1.0, float(np.abs(ref["cov"]).max()))
            np.testing.assert_allclose(cov, ref["cov"], rtol=0, atol=RS.TOL_COV * cs, err_msg=tag)
            hd.close()


# ---------------------------------------------------------------- reproducibility and the LDS hook
def _one_run(seed=7):
    d, N = 65, 257
    out = []
    for like in ("poisson", "gaussian"):
        X, w, Mc, cc, z, u, v, U, model = _edge_inputs(d, N, like, True, seed)
        hd = Handle(d, N, alpha=model["alpha"], obs=model["obs"], m1=model["m1"], m2=model["m2"], like=like,
                    rdiag=model["rdiag"], Q=model["Q"], ratio=0.9)
        hd.set_state(X, w)
        st, ess, flag = hd.step(Mc, cc, z, u=u, v=v)
        assert st == NV.PF_OK
        mean, cov = hd.finish(U)
        out += [np.array([ess, float(flag)]), mean, cov, hd.particles(), hd.weights()]
        hd.close()
    return out


def test_two_runs_are_bitwise_equal_and_lds_poison_changes_nothing(monkeypatch):
    a, b = _one_run(), _one_run()
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    lib = NV.load()
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_LDS_POISON", "1")
    c0 = lib.pf_test_lds_poison_count()
    p = _one_run()
    assert lib.pf_test_lds_poison_count() > c0, "the poison hook never fired"
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    for x, y in zip(a, p):
        assert np.all(np.isfinite(y))
        np.testing.assert_array_equal(x, y)


# ---------------------------------------------------------------- errors
def test_error_paths():
    d, N = 4, 16
    Qb = np.eye(d)
    Qb[1, 1] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        Handle(d, N, Q=Qb)
    with pytest.raises(ValueError):
        Handle(0, N)
    with pytest.raises(ValueError):
        Handle(1025, N)
    hd = Handle(d, N)
    st, _, _ = hd.step(np.eye(d), np.zeros(d), np.zeros(d))
    assert st == NV.PF_E_NOT_INITIALIZED
    with pytest.raises(AssertionError, match="Filter not initialized."):
        NV.check(st)
    with pytest.raises(AssertionError, match="Filter not initialized."):
        hd.particles()
    # every log-weight is -inf: (z - x)^2 overflows for every particle
    hd.set_state(np.full((N, d), 1e200), np.full(N, 1.0 / N))
    st, _, _ = hd.step(np.eye(d), np.zeros(d), np.zeros(d))
    assert st == NV.PF_E_NAN
    with pytest.raises(FloatingPointError):
        NV.check(st)
    # the state before the failed step is kept
    np.testing.assert_array_equal(hd.particles(), np.full((N, d), 1e200))
    # a step that resamples needs its uniform
    hd.set_state(np.arange(N * d, dtype=float).reshape(N, d), np.full(N, 1.0 / N))
    st, ess, flag = hd.step(np.eye(d), np.zeros(d), np.zeros(d))
    assert st == NV.PF_OK and flag and ess < 0.5 * N
    mean, cov = np.empty(d), np.empty((d, d))
    assert hd.lib.pf_edh_dense_finish(hd.h, None, NV.dptr(mean), NV.dptr(cov)) == NV.PF_E_ARG
    hd.finish(0.25)
    assert np.all(hd.weights() == 1.0 / N)
    hd.close()
