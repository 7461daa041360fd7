"""GPU tests of the dense LEDH path (sensor-network models; csrc/pf_ledh_dense_kernels.h).

* reference parity: every case of tests/golden/sn_ledh_runs.npz (the reference's LEDHFlowPF with its
  UKF / EKF tracker) through ``ledh_dense.LEDHFlowPF.step`` with the mirrored tracker, at the bounds
  of tests/sn_edh_restatement.py (particles / means 1e-9 of the state scale, covariances 1e-8, weights
  rtol 1e-7, condition numbers rtol 1e-6, decisions identical); ``run()`` bitwise the step loop;
* edge shapes around the Cholesky panel (NB = 16), the solve block (32) and the 256-thread row loops,
  against the NumPy restatement (tests/sn_ledh_restatement.py);
* a diagonal P, where every component follows a scalar recursion written out here;
* chunked launches, reproducibility, the LDS poison hook, the identity-observation path, error paths.
"""

import ctypes as C

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import ledh_dense as LD
from particle_filters_amd import models as M
from particle_filters_amd import trackers as TR
from tests import sn_ledh_restatement as LR

pytestmark = pytest.mark.gpu

NB = 16  # csrc/pf_ledh_dense_kernels.h
ALPHA, M1, M2 = 0.9, 1.0, 1.0 / 3.0


@pytest.fixture(scope="module")
def golden():
    return LR.load()


# ---------------------------------------------------------------- C-ABI helper
class Handle:
    """A pf_edh_dense_handle of the skewed-t wiring driven through the pf_ledh_dense_* entries."""

    def __init__(self, d, N, *, Q=None, ratio=0.5, obs="exp"):
        self.d, self.N = d, N
        self.lib = NV.load()
        Q = np.ascontiguousarray(np.eye(d) if Q is None else Q, dtype=float)
        exp = obs == "exp"
        rd = None if exp else np.ones(d)
        model = NV.EdhDenseModel(d, NV.PF_EDH_OBS_EXP if exp else NV.PF_EDH_OBS_IDENTITY,
                                 NV.PF_EDH_LIKE_POISSON if exp else NV.PF_EDH_LIKE_GAUSSIAN, 0, ALPHA,
                                 M1 if exp else 1.0, M2 if exp else 0.0, NV.dptr(rd), NV.dptr(Q))
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
        X, w = np.ascontiguousarray(X, dtype=float), np.ascontiguousarray(w, dtype=float)
        NV.check(self.lib.pf_edh_dense_set_state(self.h, NV.dptr(X), NV.dptr(w)), "set_state")

    def step(self, P, rdiag, z, L, u=None, v=None, trace=None):
        c_ = lambda a: None if a is None else np.ascontiguousarray(a, dtype=float)  # noqa: E731
        P, rdiag, z, u, v = c_(P), c_(rdiag), c_(z), c_(u), c_(v)
        info = NV.LedhInfo()
        st = self.lib.pf_ledh_dense_step(self.h, NV.dptr(P), NV.dptr(rdiag), NV.dptr(z), NV.dptr(u), L,
                                         NV.PF_NOISE_NONE if v is None else NV.PF_NOISE_HOST, NV.dptr(v),
                                         C.byref(info), NV.dptr(trace))
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
    return LD.LEDHFlowPF(c.tracker(g, h, R), g, h, h.jacobian, lt, ll, R, c.config(rng))


def _initial(c):
    return LD.PFState(particles=c.init.copy(), weights=np.full(c.N, 1.0 / c.N), mean=np.zeros(c.d), cov=c.Q.copy())


def _step_loop(c):
    pf = _filter(c, LR.ReplayUniforms(c.U))
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
    return {name: _step_loop(LR.Case(golden, name)) for name in LR.CASES}


@pytest.mark.parametrize("name", list(LR.CASES))
def test_step_matches_the_reference(golden, step_runs, name):
    c = LR.Case(golden, name)
    covs, parts = c.stored("covs"), c.stored("particles")
    scale = max(1.0, float(np.abs(c.k("means")).max()))
    err = dict(x=0.0, cov=0.0, w=0.0, cond=0.0, ess=0.0)
    for t, r in enumerate(step_runs[name]):
        assert r["flag"] == bool(c.k("flags")[t]), f"t={t}: resample decision"
        err["x"] = max(err["x"], np.abs(r["mean"] - c.k("means")[t]).max() / scale)
        err["w"] = max(err["w"], (np.abs(r["weights"] - c.k("weights")[t]) / c.k("weights")[t]).max())
        err["ess"] = max(err["ess"], abs(r["ess"] - c.k("ess")[t]) / c.k("ess")[t])
        err["cond"] = max(err["cond"], (np.abs(np.array(r["conds"]) - c.k("conds")[t]) / c.k("conds")[t]).max())
        if t in covs:
            err["cov"] = max(err["cov"], np.abs(r["cov"] - covs[t]).max() / max(1.0, np.abs(covs[t]).max()))
        if t in parts:
            err["x"] = max(err["x"], np.abs(r["particles"] - parts[t]).max() / scale)
    print(f"{name}: GPU vs reference x {err['x']:.2e} w(rel) {err['w']:.2e} ess(rel) {err['ess']:.2e} "
          f"cov {err['cov']:.2e} cond(rel) {err['cond']:.2e}")
    for t, r in enumerate(step_runs[name]):
        np.testing.assert_allclose(r["mean"], c.k("means")[t], rtol=0, atol=LR.TOL_X * scale, err_msg=f"mean t={t}")
        np.testing.assert_allclose(r["weights"], c.k("weights")[t], rtol=LR.RTOL_W, atol=0, err_msg=f"w t={t}")
        np.testing.assert_allclose(r["ess"], c.k("ess")[t], rtol=LR.RTOL_W, err_msg=f"ess t={t}")
        np.testing.assert_allclose(r["conds"], c.k("conds")[t], rtol=LR.RTOL_COND)
        if t in covs:
            cs = max(1.0, float(np.abs(covs[t]).max()))
            np.testing.assert_allclose(r["cov"], covs[t], rtol=0, atol=LR.TOL_COV * cs, err_msg=f"cov t={t}")
        if t in parts:
            np.testing.assert_allclose(r["particles"], parts[t], rtol=0, atol=LR.TOL_X * scale, err_msg=f"x t={t}")


@pytest.mark.parametrize("name", list(LR.CASES))
def test_run_is_bitwise_the_step_loop(golden, step_runs, name):
    c = LR.Case(golden, name)
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
    assert pf.state.diagnostics == {}


def test_run_with_condition_numbers_equals_run(golden, step_runs):
    c = LR.Case(golden, "skewt16")
    pf = _filter(c, np.random.default_rng(0))
    res = pf.run(_initial(c), c.Z, replay=(None, np.where(np.isfinite(c.U), c.U, 0.0)), condition_numbers=True)
    loop = step_runs["skewt16"]
    np.testing.assert_array_equal(res.means, np.array([r["mean"] for r in loop]))
    np.testing.assert_array_equal(res.flags, np.array([r["flag"] for r in loop]))
    np.testing.assert_array_equal(pf.state.diagnostics["condition_numbers"], loop[-1]["conds"])


# ---------------------------------------------------------------- inputs of the shape tests
def _inputs(d, N, seed, *, diagonal=False):
    """Skewed-t wiring on random data: P SPD of unit scale (the sensor network's kernel plus a random
    low-rank part), dense SPD Q, Poisson counts, particles of the stationary spread."""
    rng = np.random.default_rng(seed)
    i = np.arange(d)
    K = np.exp(-((i[:, None] - i[None, :]) ** 2) / 8.0)
    if diagonal:
        P = np.diag(rng.uniform(0.3, 2.0, d))
    else:
        B = rng.normal(size=(d, 3))
        P = 0.6 * K + 0.1 * (B @ B.T) + 0.3 * np.eye(d)
    Q = 0.5 * K + 0.5 * np.eye(d)
    # a narrower cloud at the large shapes, where a unit spread leaves one live weight among 2 or 8
    X = rng.normal(size=(N, d)) * (1.0 if d <= 144 else 0.05) + (0.0 if d <= 144 else rng.normal(size=d))
    w = rng.uniform(0.5, 1.5, N)
    w = w / w.sum()
    z = rng.poisson(1.5, d).astype(float)
    rdiag = rng.uniform(0.8, 1.25, d)
    model = dict(alpha=ALPHA, obs="exp", m1=M1, m2=M2, like="poisson", rdiag=None, Q=Q)
    return dict(P=P, Q=Q, X=X, w=w, z=z, rdiag=rdiag, model=model)


def _device_step(d, N, L, inp, *, ratio=0.5, U=0.37, v=None, u=None, trace=None):
    hd = Handle(d, N, Q=inp["Q"], ratio=ratio)
    hd.set_state(inp["X"], inp["w"])
    st, ess, flag = hd.step(inp["P"], inp["rdiag"], inp["z"], L, u=u, v=v, trace=trace)
    assert st == NV.PF_OK, NV.load().pf_last_error().decode()
    mean, cov = hd.finish(U)
    out = dict(ess=ess, flag=flag, mean=mean, cov=cov, particles=hd.particles(), weights=hd.weights())
    hd.close()
    return out


# d around the panel (NB), the solve block (32), the wave (64) and one pass of the 256-thread loops;
# N = 1, an odd count and more than the 64 rows of a product tile; L = 1 and L > 1
EDGE = [(1, 3, 3), (2, 1, 1), (3, 65, 3), (NB - 1, 3, 3), (NB, 65, 1), (NB + 1, 3, 3), (2 * NB + 1, 65, 3),
        (63, 3, 1), (64, 1, 3), (65, 3, 3), (144, 65, 3), (144, 1, 1), (400, 8, 2), (1024, 2, 1)]


@pytest.mark.parametrize("d,N,L", EDGE)
def test_edge_shapes_match_the_restatement(d, N, L):
    inp = _inputs(d, N, 1000 + d + N + L)
    rng = np.random.default_rng(d)
    v = 0.3 * rng.normal(size=(N, d)) if N == 3 else None  # the noise and control operands on some shapes
    u = 0.1 * rng.normal(size=d) if L == 3 else None
    trace = np.empty((L, d))
    got = _device_step(d, N, L, inp, v=v, u=u, trace=trace)
    want = LR.ledh_step(inp["X"], inp["w"], inp["P"], inp["z"], inp["model"], inp["rdiag"], L, v=v, u=u, U=0.37)
    assert abs(want["ess"] - 0.5 * N) / N >= 1e-6 or N == 1, "the decision of this input hinges on rounding"
    scale = max(1.0, float(np.abs(want["particles"]).max()))
    cs = max(1.0, float(np.abs(want["cov"]).max()))
    print(f"d={d} N={N} L={L}: x {np.abs(got['particles'] - want['particles']).max() / scale:.2e} "
          f"w(rel) {(np.abs(got['weights'] - want['weights']) / want['weights']).max():.2e} "
          f"cov {np.abs(got['cov'] - want['cov']).max() / cs:.2e} flag {want['flag']}")
    assert got["flag"] == want["flag"]
    np.testing.assert_allclose(got["ess"], want["ess"], rtol=LR.RTOL_W)
    np.testing.assert_allclose(got["particles"], want["particles"], rtol=0, atol=LR.TOL_X * scale)
    np.testing.assert_allclose(got["weights"], want["weights"], rtol=LR.RTOL_W, atol=0)
    np.testing.assert_allclose(got["mean"], want["mean"], rtol=0, atol=LR.TOL_X * scale)
    np.testing.assert_allclose(got["cov"], want["cov"], rtol=0, atol=LR.TOL_COV * cs)
    # the trace is particle 0 before each lambda step: its first row is eta_0 exactly
    np.testing.assert_array_equal(trace[0], want["eta0"][0])
    conds = LD.condition_numbers(trace, inp["P"], inp["rdiag"], M1, M2)
    np.testing.assert_allclose(conds, want["conds"], rtol=LR.RTOL_COND)


@pytest.mark.parametrize("d,N,L", [(1, 3, 3), (NB + 1, 3, 3), (65, 3, 1), (144, 65, 3)])
def test_diagonal_P_follows_the_scalar_recursion(d, N, L):
    """With a diagonal P, S is diagonal and every component is a scalar flow, written out here
    independently of the restatement.  Q = I and no noise, so the other terms of the log-weight are
    elementwise sums of the flowed particles and theta can be read off the weights."""
    inp = _inputs(d, N, 77 + d, diagonal=True)
    inp["Q"] = np.eye(d)
    got = _device_step(d, N, L, inp, ratio=0.0)
    p, r, z = np.diag(inp["P"]), inp["rdiag"], inp["z"]
    eta0 = ALPHA * inp["X"]
    eta, theta = eta0.copy(), np.zeros(N)
    lam, dlam = 0.0, 1.0 / L
    for _ in range(L):
        lam = min(1.0, lam + dlam)
        hx = M1 * np.exp(M2 * eta)
        D = M2 * hx
        e = hx - D * eta
        a = -0.5 * p * D * D / (lam * D * D * p + r)
        y = p * D * (z - e) / r
        t1 = y + lam * a * y + a * eta0
        b = t1 + 2.0 * lam * a * t1
        eta = eta + dlam * (a * eta + b)
        theta += np.sum(np.log1p(dlam * a), axis=1)
    scale = max(1.0, float(np.abs(eta).max()))
    np.testing.assert_allclose(got["particles"], eta, rtol=0, atol=1e-12 * scale)
    # log w_i - log w_0 = theta_i - theta_0 + (other_i - other_0), other from the device's own particles
    xk = got["particles"]
    lamk = np.clip(M1 * np.exp(M2 * xk), 1e-10, 1e10)
    other = np.log(inp["w"] + 1e-300) - 0.5 * np.sum((xk - eta0) ** 2, axis=1) + np.sum(z * np.log(lamk) - lamk, axis=1)
    dth = np.log(got["weights"] / got["weights"][0]) - (other - other[0])
    # theta to 1e-12 relative.  It is read off the weights (the handle has no getter for it), so the
    # rounding of ``other``, a sum over d components formed here and on the device, is added on top:
    # 8 eps |other| covers the two sums, their difference and the log / exp of the normalisation
    # (5e-13 at |other| = 300, d = 144).
    tol = 1e-12 * max(1.0, float(np.abs(theta).max())) + 8.0 * np.finfo(float).eps * float(np.abs(other).max())
    print(f"d={d}: x {np.abs(got['particles'] - eta).max() / scale:.2e} theta {np.abs(dth - (theta - theta[0])).max():.2e} "
          f"(bound {tol:.2e}, |theta| {np.abs(theta).max():.1f}, |other| {np.abs(other).max():.1f})")
    np.testing.assert_allclose(dth, theta - theta[0], rtol=0, atol=tol)
    assert np.abs(theta - theta[0]).max() > 1e-3 or N == 1


# ---------------------------------------------------------------- chunks, repeatability, the poison hook
def _one_run():
    d, N, L = 33, 65, 3
    inp = _inputs(d, N, 5)
    v = 0.2 * np.random.default_rng(9).normal(size=(N, d))
    r = _device_step(d, N, L, inp, v=v)
    return [np.array([r["ess"], float(r["flag"])]), r["mean"], r["cov"], r["particles"], r["weights"]]


def test_chunked_launches_are_bitwise_the_single_launch(monkeypatch):
    a = _one_run()
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_LEDH_WS_CAP", str(7 * 16 * 33 * 33 + 8))  # chunks of 7: 9 full ones and one of 2
    b = _one_run()
    monkeypatch.setenv("PF_TEST_LEDH_WS_CAP", str(16 * 33 * 33 - 1))      # below one particle's workspace
    hd = Handle(33, 65)
    hd.set_state(np.zeros((65, 33)), np.full(65, 1.0 / 65))
    st, _, _ = hd.step(np.eye(33), np.ones(33), np.zeros(33), 1)
    assert st == NV.PF_E_ARG and "workspace" in NV.load().pf_last_error().decode()
    hd.close()
    monkeypatch.delenv("PF_TEST_LEDH_WS_CAP", raising=False)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


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


# ---------------------------------------------------------------- the identity observation
def test_identity_observation_launches_no_ledh_kernel(golden, monkeypatch):
    """The SNLG wiring is one affine map through pf_edh_dense_step / _run (its fixture is held in
    test_step_matches_the_reference): neither LEDH entry is called."""
    lib = NV.load()

    def refuse(*a):
        raise AssertionError("the LEDH entries must not be called for an identity observation")

    monkeypatch.setattr(lib, "pf_ledh_dense_step", refuse)
    monkeypatch.setattr(lib, "pf_ledh_dense_run", refuse)
    c = LR.Case(golden, "snlg64")
    pf = _filter(c, LR.ReplayUniforms(c.U))
    st = pf.step(_initial(c), c.Z[0], process_noise_sampler=lambda n, nx: c.V[0])
    np.testing.assert_allclose(st.mean, c.k("means")[0], rtol=0, atol=LR.TOL_X * max(1.0, np.abs(c.k("means")).max()))
    assert len(st.diagnostics["condition_numbers"]) == c.L
    pf2 = _filter(c, np.random.default_rng(0))
    res = pf2.run(_initial(c), c.Z, process_noise="host", replay=(c.V, np.where(np.isfinite(c.U), c.U, 0.0)))
    np.testing.assert_array_equal(res.means[0], st.mean)
    # and a skewed-t filter does call it
    c2 = LR.Case(golden, "skewt16")
    with pytest.raises(AssertionError, match="must not be called"):
        _filter(c2, LR.ReplayUniforms(c2.U)).step(_initial(c2), c2.Z[0])


# ---------------------------------------------------------------- errors
def _small_filter(d, N, L, ratio=0.5):
    g, h, Q = M.ScaleTransition(ALPHA, d), M.ExpObservation(M1, M2, d), np.eye(d)
    tr = TR.UKFTracker(TR.UnscentedKalmanFilter(g, h, Q, np.eye(d)), TR.UKFState(np.zeros(d), Q.copy(), 0))
    return LD.LEDHFlowPF(tr, g, h, h.jacobian, M.GaussianTransitionDensity(g, Q), M.PoissonLikelihood(h), np.eye(d),
                         LD.LEDHConfig(n_particles=N, n_lambda_steps=L, resample_ess_ratio=ratio,
                                       rng=np.random.default_rng(2)))


def test_overflowing_particle_is_a_linalg_error_and_the_state_is_kept():
    d, N, L = 20, 9, 2
    rng = np.random.default_rng(3)
    X = rng.normal(size=(N, d))
    Xbad = X.copy()
    Xbad[4, 7] = 3000.0  # exp(m2 alpha x) overflows: S of particle 4 is not finite
    w = np.full(N, 1.0 / N)
    z = rng.poisson(1.5, d).astype(float)
    pf = _small_filter(d, N, L)
    with pytest.raises(np.linalg.LinAlgError, match="particle 4"):
        pf.step(LD.PFState(Xbad, w, np.zeros(d), np.eye(d)), z)
    np.testing.assert_array_equal(pf._download("particles"), Xbad)  # the state from before the step
    np.testing.assert_array_equal(pf._download("weights"), w)
    # the next valid step is correct: bitwise a fresh filter's whose tracker made the same calls (the
    # failed step ended after its predict), and the restatement's on that tracker's covariance
    st = pf.step(LD.PFState(X, w, np.zeros(d), np.eye(d)), z)
    pf2 = _small_filter(d, N, L)
    pf2.tracker.predict()
    tr = _small_filter(d, N, L).tracker
    tr.predict()
    _, P = tr.predict()
    st2 = pf2.step(LD.PFState(X, w, np.zeros(d), np.eye(d)), z)
    np.testing.assert_array_equal(st.particles, st2.particles)
    np.testing.assert_array_equal(st.weights, st2.weights)
    model = dict(alpha=ALPHA, obs="exp", m1=M1, m2=M2, like="poisson", rdiag=None, Q=np.eye(d))
    U = np.random.default_rng(2).random()  # the filter's first draw, if it resampled
    want = LR.ledh_step(X, w, 0.5 * (P + P.T), z, model, np.ones(d), L, U=U)
    assert pf.last_resampled == want["flag"] and abs(want["ess"] - 0.5 * N) / N > 1e-6
    np.testing.assert_allclose(st.particles, want["particles"], rtol=0, atol=LR.TOL_X * max(1.0, np.abs(X).max()))
    np.testing.assert_allclose(st.weights, want["weights"], rtol=LR.RTOL_W)
    # a run with the bad particle fails the same way and leaves the filter uninitialised
    pf3 = _small_filter(d, N, L)
    with pytest.raises(np.linalg.LinAlgError):
        pf3.run(LD.PFState(Xbad, w, np.zeros(d), np.eye(d)), z[None, :], replay=(None, np.array([0.5])))
    with pytest.raises(AssertionError, match="Filter not initialized."):
        pf3._download("particles")


def test_dead_weights_and_argument_errors():
    d, N = 6, 8
    inp = _inputs(d, N, 11)
    hd = Handle(d, N, Q=inp["Q"])
    hd.set_state(inp["X"], inp["w"])
    zbad = inp["z"].copy()
    zbad[2] = np.nan  # with L = 1 the flow ends at a NaN position: no weight is alive
    st, _, _ = hd.step(inp["P"], inp["rdiag"], zbad, 1)
    assert st == NV.PF_E_NAN
    np.testing.assert_array_equal(hd.particles(), inp["X"])
    # argument errors, before a device is touched
    assert hd.step(inp["P"], inp["rdiag"], inp["z"], 0)[0] == NV.PF_E_ARG
    rbad = inp["rdiag"].copy()
    rbad[1] = 0.0
    assert hd.step(inp["P"], rbad, inp["z"], 2)[0] == NV.PF_E_ARG
    rbad[1] = np.inf
    assert hd.step(inp["P"], rbad, inp["z"], 2)[0] == NV.PF_E_ARG
    # a valid step still works on the same handle
    st, ess, _ = hd.step(inp["P"], inp["rdiag"], inp["z"], 2)
    assert st == NV.PF_OK and 0.0 < ess <= N
    # a second step while one is pending, then finish
    assert hd.step(inp["P"], inp["rdiag"], inp["z"], 2)[0] == NV.PF_E_ARG
    hd.finish(0.5)
    hd.close()
    # an identity handle has no per-particle flow
    hi = Handle(d, N, obs="identity")
    hi.set_state(inp["X"], inp["w"])
    assert hi.step(inp["P"], inp["rdiag"], inp["z"], 2)[0] == NV.PF_E_ARG
    assert "identity" in NV.load().pf_last_error().decode()
    hi.close()
