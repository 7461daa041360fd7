"""GPU tests of the device process noise of the sensor-network flows (csrc/pf_noise_dense_kernels.h).

* the draws against the Philox oracle (oracle/philox.normals times chol(Q)), elementwise at
  ``|dV_ij| <= 2e-12 sum_k |L_jk| (1 + |zeta_ik|)``: the project's 1e-12 pin on one fp64 normal
  (tests/test_gpu_parity.py::test_init_draws_are_philox) plus the dot-product bound d 2^-53 of either side
  for d <= 1024; a wrong index, epoch or stream is off by O(1);
* the draws do not depend on N, are bitwise reproducible, and the LDS poison hook changes nothing;
* a device-noise run is bitwise the host replay of the numbers ``process_noise_draws`` returns, on all five
  routes, and bitwise the step loop, with both resample decisions taken;
* end to end against the NumPy restatements (tests/sn_edh_restatement.py, tests/sn_ledh_restatement.py) fed a
  V computed from oracle/philox.py alone, at the bounds of
  tests/test_gpu_sn_edh.py::test_edge_shapes_match_the_restatement;
* the device initial draw, and the error paths of the C ABI.
"""

import ctypes as C
import functools

import numpy as np
import pytest

from oracle import philox as PH
from particle_filters_amd import _native as NV
from particle_filters_amd import edh as E
from particle_filters_amd import ledh_dense as LD
from particle_filters_amd import models as M
from particle_filters_amd import trackers as TR
from particle_filters_amd.noise import DeviceGaussianNoise
from tests import sn_edh_restatement as RS
from tests import sn_ledh_restatement as LRS

pytestmark = pytest.mark.gpu

ALPHA, M1, M2, NL, RATIO = 0.9, 1.0, 1.0 / 3.0, 4, 0.5
ROUTES = ("edh_host_map", "edh_device_map", "edh_device_tracker", "ledh_exp", "ledh_identity")


def _spd(rng, d, cond=1e4):
    Qm, _ = np.linalg.qr(rng.normal(size=(d, d)))
    ev = np.exp(np.linspace(0.0, -np.log(cond), d)) if d > 1 else np.ones(1)
    Q = (Qm * ev) @ Qm.T
    return 0.5 * (Q + Q.T)


def _oracle_zeta(seed, N, d, epoch, stream=PH.STREAM_PROCESS):
    return PH.normals(seed, N * d, 0, epoch, stream).reshape(N, d)


def _bound(Lc, zeta):
    return 2e-12 * ((1.0 + np.abs(zeta)) @ np.abs(Lc).T)


def _filter(route, d, N, Q, rng=None):
    """A fresh filter (and tracker) of one route on the wiring of the notebooks."""
    g = M.ScaleTransition(ALPHA, d)
    if route == "ledh_identity":
        h = M.IdentityObservation(d)
        R = 4.0 * np.eye(d)
        like = M.GaussianLikelihood(h, R)
    else:
        h = M.ExpObservation(M1, M2, d)
        R = np.eye(d) * M1
        like = M.PoissonLikelihood(h)
    ukf = TR.UnscentedKalmanFilter(g, h, Q, R, alpha=1e-3, beta=2.0, kappa=0.0)
    st = TR.UKFState(mean=np.zeros(d), cov=Q.copy(), t=0)
    trk = TR.DeviceUKFTracker(ukf, st) if route == "edh_device_tracker" else TR.UKFTracker(ukf, st)
    lt = M.GaussianTransitionDensity(g, Q)
    rng = np.random.default_rng(0) if rng is None else rng
    if route.startswith("ledh"):
        return LD.LEDHFlowPF(trk, g, h, h.jacobian, lt, like, R,
                             LD.LEDHConfig(n_particles=N, n_lambda_steps=NL, resample_ess_ratio=RATIO, rng=rng))
    return E.EDHFlowPF(trk, g, h, h.jacobian, lt, like, R,
                       E.EDHConfig(n_particles=N, n_lambda_steps=NL, resample_ess_ratio=RATIO, flow_integrator="rk4",
                                   rng=rng), flow_map="host" if route == "edh_host_map" else "device")


def _close(pf):
    pf.close()
    if isinstance(pf.tracker, TR.DeviceUKFTracker):
        pf.tracker.close()


# ---------------------------------------------------------------- 1, 2: the draws
# d % 4 != 0 (counter groups straddle rows) and == 0, less than a tile, the tile boundary with the triangular
# cut-off on either side, three column tiles; one row, a row tile and its neighbours, several row tiles
DRAW_SHAPES = [(1, 1), (1, 257), (3, 63), (5, 65), (17, 257), (63, 65), (64, 65), (65, 63), (65, 257), (144, 1),
               (144, 257)]


@pytest.mark.parametrize("d, N", DRAW_SHAPES)
def test_draws_match_the_philox_oracle(d, N):
    Q = _spd(np.random.default_rng(d), d)
    Lc = np.linalg.cholesky(Q)
    pf = _filter("edh_host_map", d, N, Q)
    got = {}
    for seed in (0x9E3779B97F4A7C15, 11):
        for epoch in (0, 2 ** 32 - 2):
            dn = DeviceGaussianNoise(seed, 7)
            V = pf.process_noise_draws(dn, epoch)
            assert V.shape == (N, d) and dn.epoch == 7
            zeta = _oracle_zeta(seed, N, d, epoch)
            err = np.abs(V - zeta @ Lc.T)
            print(f"d={d} N={N} seed={seed:#x} epoch={epoch}: max |dV| / bound = {(err / _bound(Lc, zeta)).max():.3f}")
            assert np.all(err <= _bound(Lc, zeta))
            got[seed, epoch] = V
    keys = list(got)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not np.array_equal(got[a], got[b]), (a, b)
    # the epoch defaults to the object's own
    np.testing.assert_array_equal(pf.process_noise_draws(DeviceGaussianNoise(11, 2 ** 32 - 2)), got[11, 2 ** 32 - 2])
    _close(pf)


def _draw(d, N, seed=5, epoch=3):
    pf = _filter("edh_host_map", d, N, _spd(np.random.default_rng(d), d))
    V = pf.process_noise_draws(DeviceGaussianNoise(seed, epoch))
    _close(pf)
    return V


@pytest.mark.parametrize("d", [5, 17, 65, 144])
def test_draws_do_not_depend_on_N_and_are_bitwise_reproducible(d, monkeypatch):
    big, small = _draw(d, 257), _draw(d, 63)
    np.testing.assert_array_equal(big[:63], small)
    np.testing.assert_array_equal(_draw(d, 257), big)
    lib = NV.load()
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_LDS_POISON", "1")
    c0 = lib.pf_test_lds_poison_count()
    poisoned = _draw(d, 257)
    assert lib.pf_test_lds_poison_count() > c0, "the poison hook never fired"
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    assert np.all(np.isfinite(poisoned))
    np.testing.assert_array_equal(poisoned, big)


# ---------------------------------------------------------------- 3, 4: runs
T, N_RUN, E0 = 3, 257, 5
# Q is scaled down with d so that the ESS of N_RUN particles stays around the threshold and both decisions occur
QSCALE = {17: 1.0, 65: 0.15}


class Scenario:
    """The inputs of one run and its NumPy restatement fed the oracle's V."""

    def __init__(self, family, d, seed):  # family: "edh", "ledh_exp" or "ledh_identity"
        self.route, self.d, self.seed = family, d, seed
        rng = np.random.default_rng(100 * d + len(family))
        self.Q = Q = QSCALE[d] * _spd(rng, d)
        Lc = np.linalg.cholesky(Q)
        self.X0 = np.ascontiguousarray(rng.standard_normal((N_RUN, d)) @ Lc.T)
        if family == "ledh_identity":
            self.model = dict(alpha=ALPHA, obs="identity", m1=1.0, m2=0.0, like="gaussian", rdiag=np.full(d, 4.0), Q=Q)
            self.Z = 2.0 * rng.standard_normal((T, d))
            self.rdiag = np.full(d, 4.0)
        else:
            self.model = dict(alpha=ALPHA, obs="exp", m1=M1, m2=M2, like="poisson", rdiag=None, Q=Q)
            self.Z = rng.poisson(1.2, size=(T, d)).astype(float)
            self.rdiag = np.full(d, M1)
        self.U = rng.random(T)
        self.V = np.stack([_oracle_zeta(seed, N_RUN, d, E0 + t) @ Lc.T for t in range(T)])

    def state(self):
        return E.PFState(particles=self.X0.copy(), weights=np.full(N_RUN, 1.0 / N_RUN), mean=np.zeros(self.d),
                         cov=self.Q.copy())

    @functools.cached_property
    def reference(self):
        """The T steps in NumPy: the host tracker ahead of the particles, then the restated step."""
        pf_like = _HostTracker(self)
        X, w, out = self.X0, np.full(N_RUN, 1.0 / N_RUN), []
        for t in range(T):
            P, xbar = pf_like.advance(self.Z[t])
            if self.route.startswith("ledh"):
                r = LRS.ledh_step(X, w, P, self.Z[t], self.model, self.rdiag, NL, v=self.V[t], ratio=RATIO, U=self.U[t])
            else:
                Mc, cc, _ = RS.compose(P, ALPHA * xbar, self.Z[t], self.model, np.diag(self.rdiag), NL, "rk4")
                r = RS.dense_step(X, w, Mc, cc, self.Z[t], self.model, v=self.V[t], ratio=RATIO, U=self.U[t])
            X, w = r["particles"], r["weights"]
            out.append(r)
        return out

    def safe(self):
        """Both decisions are taken, none of them within 1e-6 (relative) of the threshold."""
        ess = np.array([r["ess"] for r in self.reference])
        flags = [r["flag"] for r in self.reference]
        return any(flags) and not all(flags) and np.all(np.abs(ess - RATIO * N_RUN) > 1e-6 * RATIO * N_RUN)


class _HostTracker:
    """The notebook's UKF on the host (trackers.UKFTracker), called as the filters call it."""

    def __init__(self, sc):
        d = sc.d
        g = M.ScaleTransition(ALPHA, d)
        h = M.IdentityObservation(d) if sc.route == "ledh_identity" else M.ExpObservation(M1, M2, d)
        ukf = TR.UnscentedKalmanFilter(g, h, sc.Q, np.diag(sc.rdiag), alpha=1e-3, beta=2.0, kappa=0.0)
        self.trk = TR.UKFTracker(ukf, TR.UKFState(mean=np.zeros(d), cov=sc.Q.copy(), t=0))

    def advance(self, z):
        _, P = self.trk.predict()
        xbar = np.asarray(self.trk.get_past_mean(), float).copy()
        self.trk.update(z)
        P = np.asarray(P, float)
        return 0.5 * (P + P.T), xbar


@functools.lru_cache(maxsize=None)
def _family_scenario(family, d):
    for seed in range(1, 60):
        sc = Scenario(family, d, seed)
        if sc.safe():
            return sc
    raise AssertionError(f"no seed below 60 takes both resample decisions for {family}, d = {d}")


def scenario(route, d):
    """The first seed whose restated run takes both decisions with a margin (checked on the CPU, asserted on the
    device by the tests).  The three EDH routes compute one filter and share the scenario."""
    return _family_scenario("edh" if route.startswith("edh") else route, d)


def _outputs(pf, res):
    return [res.means, res.covs, res.ess, res.flags, pf.state.particles.copy(), pf.state.weights.copy()]


@pytest.mark.parametrize("d", [17, 65])
@pytest.mark.parametrize("route", ROUTES)
def test_device_noise_run_is_bitwise_the_host_replay_and_the_step_loop(route, d):
    sc = scenario(route, d)
    # the device draws inside the run
    pf = _filter(route, d, N_RUN, sc.Q)
    dn = DeviceGaussianNoise(sc.seed, E0)
    res = pf.run(sc.state(), sc.Z, process_noise=dn, replay=(None, sc.U))
    assert dn.epoch == E0 + T
    dev = _outputs(pf, res)
    flags = res.flags.copy()
    assert flags.any() and not flags.all(), f"{route} d={d}: flags {flags} must hold both decisions"
    V = np.stack([pf.process_noise_draws(dn, E0 + t) for t in range(T)])
    _close(pf)
    # the same numbers uploaded
    pf = _filter(route, d, N_RUN, sc.Q)
    host = _outputs(pf, pf.run(sc.state(), sc.Z, process_noise="host", replay=(V, sc.U)))
    _close(pf)
    for a, b in zip(dev, host):
        np.testing.assert_array_equal(a, b)
    # the step loop, drawing the resampling uniform only where the step resamples
    pf = _filter(route, d, N_RUN, sc.Q, rng=RS.ReplayUniforms(np.where(flags, sc.U, np.nan)))
    dn = DeviceGaussianNoise(sc.seed, E0)
    st, means, covs, ess, fl = sc.state(), [], [], [], []
    for t in range(T):
        st = pf.step(st, sc.Z[t], process_noise_sampler=dn)
        assert dn.epoch == E0 + t + 1
        means.append(st.mean), covs.append(st.cov), ess.append(pf.last_ess), fl.append(pf.last_resampled)
    loop = [np.array(means), np.array(covs), np.array(ess), np.array(fl), st.particles.copy(), st.weights.copy()]
    _close(pf)
    for a, b in zip(dev, loop):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("d", [17, 65])
@pytest.mark.parametrize("route", ROUTES)
def test_device_noise_run_matches_the_restatement_fed_the_oracle(route, d):
    sc = scenario(route, d)
    ref = sc.reference
    assert sc.safe()
    pf = _filter(route, d, N_RUN, sc.Q)
    res = pf.run(sc.state(), sc.Z, process_noise=DeviceGaussianNoise(sc.seed, E0), replay=(None, sc.U))
    X, w = pf.state.particles.copy(), pf.state.weights.copy()
    _close(pf)
    np.testing.assert_array_equal(res.flags, np.array([r["flag"] for r in ref]))
    scale = max(1.0, max(float(np.abs(r["particles"]).max()) for r in ref))
    for t, r in enumerate(ref):
        tag = f"{route} d={d} t={t}"
        np.testing.assert_allclose(res.ess[t], r["ess"], rtol=RS.RTOL_W, err_msg=tag)
        np.testing.assert_allclose(res.means[t], r["mean"], rtol=0, atol=RS.TOL_X * scale, err_msg=tag)
        cs = max(1.0, float(np.abs(r["cov"]).max()))
        np.testing.assert_allclose(res.covs[t], r["cov"], rtol=0, atol=RS.TOL_COV * cs, err_msg=tag)
    np.testing.assert_allclose(X, ref[-1]["particles"], rtol=0, atol=RS.TOL_X * scale)
    np.testing.assert_allclose(w, ref[-1]["weights"], rtol=RS.RTOL_W, atol=1e-13)


# ---------------------------------------------------------------- 5: the device initial draw
@pytest.mark.parametrize("route", ["edh_host_map", "ledh_exp"])
@pytest.mark.parametrize("d, N", [(1, 1), (5, 65), (17, 257), (65, 63), (144, 257)])
def test_device_init_from_gaussian(route, d, N):
    rng = np.random.default_rng(7 * d + N)
    Q = _spd(rng, d)
    cov0 = 2.5 * _spd(rng, d, cond=1e2)
    mean0 = rng.normal(size=d)
    pf = _filter(route, d, N, Q)
    dn = DeviceGaussianNoise(21, 9)
    st = pf.init_from_gaussian(mean0, cov0, draws=dn)
    assert dn.epoch == 9
    X, w = st.particles, st.weights
    np.testing.assert_array_equal(w, np.full(N, 1.0 / N))
    L0 = np.linalg.cholesky(cov0)
    zeta = _oracle_zeta(21, N, d, 9, PH.STREAM_INIT)
    want = mean0 + zeta @ L0.T
    # the bound of the draws plus the one rounding of adding the mean on either side
    assert np.all(np.abs(X - want) <= _bound(L0, zeta) + 2.0 ** -52 * np.abs(want))
    mean, cov = pf._weighted_stats(X, w)
    scale = max(1.0, float(np.abs(X).max()))
    np.testing.assert_allclose(st.mean, mean, rtol=0, atol=RS.TOL_X * scale)
    np.testing.assert_allclose(st.cov, cov, rtol=0, atol=RS.TOL_COV * max(1.0, float(np.abs(cov).max())))
    # the state is the device's: a step runs on it without an upload of particles
    z = np.zeros(d)
    st2 = pf.step(st, z, process_noise_sampler=DeviceGaussianNoise(21, 9))
    assert np.all(np.isfinite(st2.mean)) and pf.last_ess > 0.0
    _close(pf)


def test_device_init_refuses_a_cov0_that_is_not_positive_definite():
    d, N = 5, 33
    pf = _filter("edh_host_map", d, N, np.eye(d))
    bad = np.eye(d)
    bad[2, 2] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        pf.init_from_gaussian(np.zeros(d), bad, draws=DeviceGaussianNoise(1))
    assert pf.state is None
    with pytest.raises(AssertionError, match="Filter not initialized."):
        pf._download("particles")
    _close(pf)


# ---------------------------------------------------------------- 6: errors of the C ABI
def test_device_noise_must_be_armed_and_its_epochs_must_fit():
    d, N = 5, 33
    lib = NV.load()
    Q = np.ascontiguousarray(np.eye(d))
    rd = np.ones(d)
    model = NV.EdhDenseModel(d, NV.PF_EDH_OBS_IDENTITY, NV.PF_EDH_LIKE_GAUSSIAN, 0, ALPHA, 1.0, 0.0, NV.dptr(rd),
                             NV.dptr(Q))
    opts = NV.EdhDenseOpts(N, RATIO, 0, 0)
    h = C.c_void_p()
    NV.check(lib.pf_edh_dense_create(C.byref(model), C.byref(opts), C.byref(h)), "create")
    X = np.ascontiguousarray(np.random.default_rng(3).normal(size=(N, d)))
    w = np.full(N, 1.0 / N)
    NV.check(lib.pf_edh_dense_set_state(h, NV.dptr(X), NV.dptr(w)), "set_state")
    Mc, cc, z = np.ascontiguousarray(np.eye(d)), np.zeros(d), np.zeros(d)
    info = NV.LedhInfo()

    def step():
        return lib.pf_edh_dense_step(h, NV.dptr(Mc), NV.dptr(cc), NV.dptr(z), None, NV.PF_NOISE_DEVICE, None,
                                     C.byref(info))

    def run(Tn):
        Ms, cs, Z = np.ascontiguousarray(np.broadcast_to(Mc, (Tn, d, d))), np.zeros((Tn, d)), np.zeros((Tn, d))
        U = np.zeros(Tn)
        NV.check(lib.pf_edh_dense_set_run_replay(h, None, NV.dptr(U), Tn), "set_run_replay")
        means, covs = np.empty((Tn, d)), np.empty((Tn, d, d))
        return lib.pf_edh_dense_run(h, NV.dptr(Ms), NV.dptr(cs), NV.dptr(Z), None, Tn, NV.PF_NOISE_DEVICE,
                                    NV.dptr(means), NV.dptr(covs), None, None)

    def untouched():
        got, gw = np.empty((N, d)), np.empty(N)
        NV.check(lib.pf_edh_dense_get_particles(h, NV.dptr(got)), "get_particles")
        NV.check(lib.pf_edh_dense_get_weights(h, NV.dptr(gw)), "get_weights")
        return np.array_equal(got, X) and np.array_equal(gw, w)

    # not armed
    assert step() == NV.PF_E_ARG and "pf_edh_dense_set_noise" in lib.pf_last_error().decode()
    assert run(2) == NV.PF_E_ARG
    assert untouched()
    # the epochs of the call must fit 32 bits
    NV.check(lib.pf_edh_dense_set_noise(h, 1, 2 ** 32 - 1), "set_noise")
    assert step() == NV.PF_E_ARG and "overflows" in lib.pf_last_error().decode()
    NV.check(lib.pf_edh_dense_set_noise(h, 1, 2 ** 32 - 3), "set_noise")
    assert run(3) == NV.PF_E_ARG
    assert untouched()
    # armed once, consumed once
    NV.check(lib.pf_edh_dense_set_noise(h, 1, 2 ** 32 - 3), "set_noise")
    assert run(2) == NV.PF_OK
    assert run(2) == NV.PF_E_ARG
    lib.pf_edh_dense_destroy(h)
