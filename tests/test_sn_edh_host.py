"""CPU checks of the dense EDH path for the sensor-network models (no GPU).

* the new model classes restate the notebooks' formulas (PF_PF_results_reproduction_sn_skew.ipynb
  ``prepare_skewt_model``), and ``EDHFlowPF`` accepts / refuses their wirings at construction;
* ``trackers.UKFTracker`` reproduces every predicted covariance and past mean the reference's UKF
  tracker produced (tests/golden/sn_edh_runs.npz, made by tests/golden/make_golden_skewt.py);
* the host composition ``edh.compose_flow_map`` and the NumPy restatement
  (tests/sn_edh_restatement.py) reproduce the reference's runs at the EDH tolerances of
  tests/test_gpu_edh.py: particles and means 1e-9 of the state scale, covariances 1e-8, weights
  rtol 1e-7, condition numbers rtol 1e-6, resample decisions equal.
"""

import numpy as np
import pytest

from particle_filters_amd import edh as E
from particle_filters_amd import ledh as LE
from particle_filters_amd import models as M
from particle_filters_amd import trackers as TR
from tests import sn_edh_restatement as RS


@pytest.fixture(scope="module")
def golden():
    return RS.load()


# ---------------------------------------------------------------- models
def test_poisson_likelihood_is_the_notebook_expression():
    d, m1, m2 = 7, 1.5, 1.0 / 3.0
    h = M.ExpObservation(m1, m2, d)
    like = M.PoissonLikelihood(h)
    rng = np.random.default_rng(0)
    z = rng.poisson(3.0, d)
    for x in (rng.normal(size=d), np.full(d, 80.0), np.full(d, -80.0), np.linspace(-80.0, 80.0, d)):
        lam = np.clip(m1 * np.exp(m2 * x), 1e-10, 1e10)
        want = np.sum(z * np.log(lam) - lam - np.log(np.maximum(1, np.arange(1, len(z) + 1))))
        assert like(z, x) == want
    # the clip is active at both ends
    assert np.all(m1 * np.exp(m2 * np.full(d, 80.0)) > 1e10) and np.all(m1 * np.exp(m2 * np.full(d, -80.0)) < 1e-10)


def test_exp_observation_jacobian_matches_finite_differences():
    d = 5
    h = M.ExpObservation(0.7, 0.4, d)
    x = np.random.default_rng(1).normal(size=d)
    J = h.jacobian(x)
    np.testing.assert_array_equal(J, np.diag(0.7 * 0.4 * np.exp(0.4 * x)))
    eps = 1e-6
    for j in range(d):
        dx = np.zeros(d)
        dx[j] = eps
        np.testing.assert_allclose((h(x + dx) - h(x - dx)) / (2 * eps), J[:, j], rtol=1e-8, atol=1e-9)


def test_scale_transition_and_identity():
    g = M.ScaleTransition(0.9, 3)
    x, u, v = np.array([1.0, -2.0, 3.0]), np.array([0.5, 0.5, 0.5]), np.array([0.1, 0.2, 0.3])
    np.testing.assert_array_equal(g(x), 0.9 * x)
    np.testing.assert_array_equal(g(x, u), 0.9 * x + u)
    np.testing.assert_array_equal(g(x, None, v), 0.9 * x + v)
    np.testing.assert_array_equal(g(x, u, v), 0.9 * x + u + v)
    np.testing.assert_array_equal(g.jacobian(x), 0.9 * np.eye(3))
    h = M.IdentityObservation(3)
    np.testing.assert_array_equal(h(x), x)
    np.testing.assert_array_equal(h.jacobian(x), np.eye(3))
    # not engine models: ParticleFilter / LEDHFlowPF keep refusing them
    assert not M.is_device_model(g, h)


def _wiring(d=6, like="poisson", Q=None, R=None):
    g = M.ScaleTransition(0.9, d)
    Q = np.eye(d) if Q is None else Q
    if like == "poisson":
        h = M.ExpObservation(1.0, 1.0 / 3.0, d)
        ll = M.PoissonLikelihood(h)
    else:
        h = M.IdentityObservation(d)
        ll = M.GaussianLikelihood(h, np.eye(d) if R is None else R)
    Rf = np.eye(d)
    tracker = TR.UKFTracker(TR.UnscentedKalmanFilter(g, h, Q, Rf), TR.UKFState(np.zeros(d), Q.copy(), 0))
    return tracker, g, h, M.GaussianTransitionDensity(g, Q), ll, Rf


def test_edh_constructs_the_dense_path_without_a_device():
    for like in ("poisson", "gaussian"):
        tracker, g, h, lt, ll, R = _wiring(like=like)
        pf = E.EDHFlowPF(tracker, g, h, h.jacobian, lt, ll, R, E.EDHConfig(n_particles=10, n_lambda_steps=0))
        assert pf._dense and pf.nx == 6 and pf.n == 10 and pf.L == 1
        pf2 = E.EDHFlowPF(tracker, g, h, None, lt, ll, R, E.EDHConfig(n_particles=10))
        assert pf2.Jh.__self__ is h


def test_edh_dense_refusals():
    tracker, g, h, lt, ll, R = _wiring()
    cfg = E.EDHConfig(n_particles=10)
    with pytest.raises(NotImplementedError, match="rng_mode"):
        E.EDHFlowPF(tracker, g, h, h.jacobian, lt, ll, R, cfg, rng_mode="device")
    with pytest.raises(NotImplementedError, match="jacobian_h"):
        E.EDHFlowPF(tracker, g, h, lambda x: np.eye(6), lt, ll, R, cfg)
    with pytest.raises(NotImplementedError, match="log_like_pdf"):
        E.EDHFlowPF(tracker, g, h, h.jacobian, lt, lambda z, x: 0.0, R, cfg)
    with pytest.raises(NotImplementedError, match="log_trans_pdf"):
        E.EDHFlowPF(tracker, g, h, h.jacobian, lambda a, b: 0.0, ll, R, cfg)
    with pytest.raises(NotImplementedError, match="h must be"):
        E.EDHFlowPF(tracker, g, M.ExpHalfObservation(np.ones(6)), None, lt, ll, R, cfg)
    # a Gaussian likelihood with a dense R is not elementwise
    Rd = np.eye(6) + 0.1
    tr2, g2, h2, lt2, ll2, R2 = _wiring(like="gaussian", R=Rd)
    with pytest.raises(NotImplementedError, match="diagonal"):
        E.EDHFlowPF(tr2, g2, h2, h2.jacobian, lt2, ll2, R2, cfg)
    # Q that is not positive definite
    Qb = np.eye(6)
    Qb[0, 0] = -1.0
    tr3, g3, h3, lt3, ll3, R3 = _wiring(Q=np.eye(6))
    with pytest.raises(np.linalg.LinAlgError):
        E.EDHFlowPF(tr3, g3, h3, h3.jacobian, M.GaussianTransitionDensity(g3, Qb), ll3, R3, cfg)
    # LEDH on these models is out of scope
    with pytest.raises(NotImplementedError):
        LE.LEDHFlowPF(tracker, g, h, h.jacobian, lt, ll, R, LE.LEDHConfig(n_particles=10))
    # run(): the device tracker and device noise do not exist on this path
    pf = E.EDHFlowPF(tracker, g, h, h.jacobian, lt, ll, R, cfg)
    st = E.PFState(np.zeros((10, 6)), np.full(10, 0.1), np.zeros(6), np.eye(6))
    with pytest.raises(NotImplementedError, match="tracker"):
        pf.run(st, np.zeros((2, 6)), tracker="device")
    with pytest.raises(NotImplementedError, match="process_noise"):
        pf.run(st, np.zeros((2, 6)))


# ---------------------------------------------------------------- the UKF tracker mirror
@pytest.mark.parametrize("name", list(RS.CASES))
def test_ukf_tracker_reproduces_the_reference(golden, name):
    c = RS.Case(golden, name)
    g, h, _, _, R = c.objects()
    tr = c.tracker(g, h, R)
    stored = c.stored_P()
    assert np.all(c.k("P_asym") == 0.0)  # the UKF's predicted covariances are exactly symmetric
    bitwise = True
    for t in range(c.T):
        _, P = tr.predict()
        np.testing.assert_array_equal(P, P.T)
        past = tr.get_past_mean()
        want_past = c.k("past_means")[t]
        np.testing.assert_allclose(past, want_past, rtol=1e-12, atol=1e-14)
        if t in stored:
            np.testing.assert_allclose(P, stored[t], rtol=1e-12, atol=1e-15)
            bitwise &= bool(np.array_equal(P, stored[t]) and np.array_equal(past, want_past))
        tr.update(c.Z[t])
    print(f"{name}: tracker bitwise equal to the reference's: {bitwise}")


# ---------------------------------------------------------------- composition and restatement
def _chain(c, compose):
    """Free-running restatement chain from the stored initial particles; yields per-step results."""
    g, h, _, _, R = c.objects()
    tr = c.tracker(g, h, R)
    X, w = c.init.copy(), np.full(c.N, 1.0 / c.N)
    for t in range(c.T):
        _, P = tr.predict()
        P = 0.5 * (P + P.T)
        etabar = c.alpha * tr.get_past_mean()
        Mc, cc, conds = compose(P, etabar, c.Z[t], h, R)
        tr.update(c.Z[t])
        r = RS.dense_step(X, w, Mc, cc, c.Z[t], c.model, v=None if c.V is None else c.V[t], U=c.U[t])
        r["conds"] = conds
        X, w = r["particles"], r["weights"]
        yield t, r


def _check_chain(c, compose, label):
    covs, parts = c.stored("covs"), c.stored("particles")
    scale = max(1.0, float(np.abs(c.k("means")).max()))
    err = dict(x=0.0, w=0.0, cov=0.0, cond=0.0)
    for t, r in _chain(c, compose):
        assert r["flag"] == bool(c.k("flags")[t]), f"{c.name} t={t}: resample decision"
        np.testing.assert_allclose(r["mean"], c.k("means")[t], rtol=0, atol=RS.TOL_X * scale)
        np.testing.assert_allclose(r["weights"], c.k("weights")[t], rtol=RS.RTOL_W, atol=1e-13)
        np.testing.assert_allclose(r["conds"], c.k("conds")[t], rtol=RS.RTOL_COND)
        np.testing.assert_allclose(r["ess"], c.k("ess")[t], rtol=1e-9)
        err["x"] = max(err["x"], np.abs(r["mean"] - c.k("means")[t]).max() / scale)
        big = c.k("weights")[t] > 1e-6
        err["w"] = max(err["w"], (np.abs(r["weights"] - c.k("weights")[t])[big] / c.k("weights")[t][big]).max())
        err["cond"] = max(err["cond"], (np.abs(np.array(r["conds"]) - c.k("conds")[t]) / c.k("conds")[t]).max())
        if t in covs:
            cs = max(1.0, float(np.abs(covs[t]).max()))
            np.testing.assert_allclose(r["cov"], covs[t], rtol=0, atol=RS.TOL_COV * cs)
            err["cov"] = max(err["cov"], np.abs(r["cov"] - covs[t]).max() / cs)
        if t in parts:
            np.testing.assert_allclose(r["particles"], parts[t], rtol=0, atol=RS.TOL_X * scale)
            err["x"] = max(err["x"], np.abs(r["particles"] - parts[t]).max() / scale)
    print(f"{c.name} [{label}]: x {err['x']:.2e} w(rel) {err['w']:.2e} cov {err['cov']:.2e} cond(rel) {err['cond']:.2e}")


@pytest.mark.parametrize("name", list(RS.CASES))
def test_restatement_reproduces_the_reference(golden, name):
    c = RS.Case(golden, name)
    _check_chain(c, lambda P, eb, z, h, R: RS.compose(P, eb, z, c.model, R, c.L, c.integrator), "restatement")


@pytest.mark.parametrize("name", list(RS.CASES))
def test_host_composition_reproduces_the_reference(golden, name):
    """edh.compose_flow_map's (M, c) applied to the stored eta_0 gives the stored particles."""
    c = RS.Case(golden, name)
    _check_chain(c, lambda P, eb, z, h, R: E.compose_flow_map(P, eb, z, h, h.jacobian, R, c.L, c.integrator)[:3],
                 "compose_flow_map")


def test_composed_map_agrees_with_step_by_step_integration():
    """The map against the reference's own per-particle loop (rk4_step / Euler on every particle)."""
    rng = np.random.default_rng(3)
    d, L = 9, 5
    h = M.ExpObservation(1.0, 1.0 / 3.0, d)
    A0 = rng.normal(size=(d, d))
    P = A0 @ A0.T / d + 0.1 * np.eye(d)
    R = np.eye(d)
    z = rng.poisson(1.5, d).astype(float)
    eta0 = rng.normal(size=(20, d))
    for integ in ("rk4", "euler"):
        etabar = 0.9 * rng.normal(size=d)
        Mc, cc, _, eb_end = E.compose_flow_map(P, etabar, z, h, h.jacobian, R, L, integ)
        # step by step, edh.py:225-280
        eta, eb, lam, I = eta0.copy(), etabar.copy(), 0.0, np.eye(d)
        for _ in range(L):
            lam = min(1.0, lam + 1.0 / L)
            H = h.jacobian(eb)
            e = h(eb) - H @ eb
            S = lam * H @ P @ H.T + R
            A = -0.5 * P @ H.T @ np.linalg.solve(S, H)
            b = (I + 2.0 * lam * A) @ ((I + lam * A) @ (P @ H.T @ np.linalg.solve(R, z - e)) + A @ eb)
            f = lambda vec: A @ vec + b  # noqa: E731
            if integ == "euler":
                eta = eta + (1.0 / L) * (eta @ A.T + b)
                eb = eb + (1.0 / L) * f(eb)
            else:
                eta = np.array([E.rk4_step(x, f, 1.0 / L) for x in eta])
                eb = E.rk4_step(eb, f, 1.0 / L)
        scale = max(1.0, np.abs(eta).max())
        np.testing.assert_allclose(eta0 @ Mc.T + cc, eta, rtol=0, atol=1e-13 * scale)
        np.testing.assert_allclose(eb_end, eb, rtol=0, atol=1e-13 * scale)


# ---------------------------------------------------------------- refusals of the inherited LEDH-handle members
def test_dense_path_never_hands_its_handle_to_the_ledh_entries(monkeypatch):
    """The dense handle is not a pf_ledh_handle: the members EDHFlowPF inherits from LEDHFlowPF that
    call pf_ledh_* refuse (or answer) without touching the library, also with the SNLG notebook's
    EKF tracker over the filter's own g and h."""
    from particle_filters_amd import _native as NV
    from particle_filters_amd import diagnostics as DG

    d = 6
    g, h, Q = M.ScaleTransition(0.9, d), M.IdentityObservation(d), np.eye(d)
    ekf = TR.ExtendedKalmanFilter(g, h, Q, Q, jac_g=g.jacobian, jac_h=h.jacobian)
    tracker = TR.EKFTracker(ekf, TR.EKFState(np.zeros(d), Q.copy(), 0))
    pf = E.EDHFlowPF(tracker, g, h, h.jacobian, M.GaussianTransitionDensity(g, Q), M.GaussianLikelihood(h, Q), Q,
                     E.EDHConfig(n_particles=10))

    def no_library():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(NV, "load", no_library)
    assert pf._dense and pf._h is None
    assert pf.shared_jacobian_path is False
    with pytest.raises(NotImplementedError, match="dense EDH path"):
        pf.tracker_covariances(np.zeros((3, d)))
    with pytest.raises(NotImplementedError, match="dense EDH path"):
        pf._device_tracker()
    with pytest.raises(AssertionError, match="Filter not initialized."):
        DG.filter_diagnostics(pf)
    pf.close()
    # a Gaussian likelihood whose diagonal R is not positive is refused where Q is
    Rb = np.diag([1.0, 1.0, 0.0, 1.0, 1.0, 1.0])
    with pytest.raises(np.linalg.LinAlgError):
        E.EDHFlowPF(tracker, g, h, h.jacobian, M.GaussianTransitionDensity(g, Q), M.GaussianLikelihood(h, Rb), Q,
                    E.EDHConfig(n_particles=10))


def test_dense_create_host_algebra_under_sanitizers():
    """chol_lower + lower_inverse (pf_host.h), the host work of pf_edh_dense_create, in a stand-alone
    program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/pf_edh_dense_host_check.cpp)."""
    import os
    import subprocess

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(repo, "build", "pf_edh_dense_host_check")
    if not os.path.exists(exe):  # built by __graft_entry__.build(); here if the test runs first
        subprocess.run(["make", "-C", os.path.join(repo, "particle_filters_amd", "csrc"), "hostcheck"],
                       check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
