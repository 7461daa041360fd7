"""CPU checks of the dense LEDH path for the sensor-network models (no GPU).

* the NumPy restatement (tests/sn_ledh_restatement.py, the Cholesky-pair form) reproduces every stored
  step of the reference's LEDHFlowPF (tests/golden/sn_ledh_runs.npz, made by
  tests/golden/make_golden_sn_ledh.py) at the project's bounds for this path: particles and means
  1e-9 of the state scale, covariances 1e-8, weights rtol 1e-7, condition numbers rtol 1e-6,
  resample decisions equal;
* the restatement equals a literal per-particle transcription of the reference's formulas;
* ``ledh_dense.LEDHFlowPF`` accepts / refuses the wirings at construction, without a device;
* the chunk plan of the flow kernel, in a stand-alone program under the host sanitizers.
"""

import os
import subprocess

import numpy as np
import pytest

from particle_filters_amd import ledh as LE
from particle_filters_amd import ledh_dense as LD
from particle_filters_amd import models as M
from particle_filters_amd import trackers as TR
from tests import sn_edh_restatement as RS
from tests import sn_ledh_restatement as LR


@pytest.fixture(scope="module")
def golden():
    return LR.load()


# ---------------------------------------------------------------- the restatement against the fixtures
@pytest.mark.parametrize("name", list(LR.CASES))
def test_restatement_reproduces_the_reference(golden, name):
    """A free-running chain from the stored initial particles, with the mirrored tracker."""
    c = LR.Case(golden, name)
    g, h, _, _, R = c.objects()
    tr = c.tracker(g, h, R)
    rdiag = np.diag(R).copy()
    covs, parts, Ps = c.stored("covs"), c.stored("particles"), c.stored_P()
    scale = max(1.0, float(np.abs(c.k("means")).max()))
    err = dict(x=0.0, w=0.0, cov=0.0, cond=0.0)
    X, w = c.init.copy(), np.full(c.N, 1.0 / c.N)
    for t in range(c.T):
        _, P = tr.predict()
        P = 0.5 * (P + P.T)
        tr.update(c.Z[t])
        np.testing.assert_allclose(P, Ps[t], rtol=1e-12, atol=1e-15)  # the tracker mirror
        r = LR.ledh_step(X, w, P, c.Z[t], c.model, rdiag, c.L, v=None if c.V is None else c.V[t], U=c.U[t])
        X, w = r["particles"], r["weights"]
        assert r["flag"] == bool(c.k("flags")[t]), f"{name} t={t}: resample decision"
        want_w = c.k("weights")[t]
        err["x"] = max(err["x"], np.abs(r["mean"] - c.k("means")[t]).max() / scale)
        err["w"] = max(err["w"], (np.abs(r["weights"] - want_w) / want_w).max())
        err["cond"] = max(err["cond"], (np.abs(np.array(r["conds"]) - c.k("conds")[t]) / c.k("conds")[t]).max())
        np.testing.assert_allclose(r["mean"], c.k("means")[t], rtol=0, atol=LR.TOL_X * scale)
        np.testing.assert_allclose(r["weights"], want_w, rtol=LR.RTOL_W, atol=0)
        np.testing.assert_allclose(r["conds"], c.k("conds")[t], rtol=LR.RTOL_COND)
        np.testing.assert_allclose(r["ess"], c.k("ess")[t], rtol=LR.RTOL_W)
        if t in covs:
            cs = max(1.0, float(np.abs(covs[t]).max()))
            err["cov"] = max(err["cov"], np.abs(r["cov"] - covs[t]).max() / cs)
            np.testing.assert_allclose(r["cov"], covs[t], rtol=0, atol=LR.TOL_COV * cs)
        if t in parts:
            err["x"] = max(err["x"], np.abs(r["particles"] - parts[t]).max() / scale)
            np.testing.assert_allclose(r["particles"], parts[t], rtol=0, atol=LR.TOL_X * scale)
    print(f"{name}: x {err['x']:.2e} w(rel) {err['w']:.2e} cov {err['cov']:.2e} cond(rel) {err['cond']:.2e}")


def test_fixture_holds_resampling_and_non_resampling_steps(golden):
    for name in ("skewt16", "skewt25_noise"):  # the small cases, without and with host process noise
        flags = np.asarray(golden[f"{name}__flags"], bool)
        assert flags.any() and not flags.all(), name
    # a noisy step that starts from carried-over, non-uniform weights is stored
    f25 = np.asarray(golden["skewt25_noise__flags"], bool)
    assert np.any(~f25[:-1]) and np.ptp(golden["skewt25_noise__weights"][int(np.argmin(f25))]) > 0.0
    for name in LR.CASES:  # no decision hinges on rounding
        c = LR.Case(golden, name)
        assert np.all(np.abs(c.k("ess") - LR.RATIO * c.N) / c.N >= 1e-3)


def test_restatement_equals_the_literal_transcription():
    """The Cholesky-pair form against explicit A_i and slogdet (ledh.py:140-179) at d = 5, N = 4, L = 3."""
    rng = np.random.default_rng(5)
    d, N, L = 5, 4, 3
    h = M.ExpObservation(1.3, 0.4, d)
    model = dict(alpha=0.9, obs="exp", m1=1.3, m2=0.4, like="poisson", rdiag=None, Q=np.eye(d))
    A0 = rng.normal(size=(d, d))
    P = A0 @ A0.T / d + 0.2 * np.eye(d)
    rdiag = rng.uniform(0.5, 2.0, d)
    z = rng.poisson(2.0, d).astype(float)
    eta0 = rng.normal(size=(N, d))
    eta, theta, conds = LR.flow(eta0, P, z, model, rdiag, L)
    eta_l, theta_l, conds_l = LR.literal_flow(eta0, P, z, h, h.jacobian, np.diag(rdiag), L)
    np.testing.assert_allclose(eta, eta_l, rtol=0, atol=1e-12 * max(1.0, np.abs(eta_l).max()))
    np.testing.assert_allclose(theta, theta_l, rtol=0, atol=1e-12 * max(1.0, np.abs(theta_l).max()))
    np.testing.assert_allclose(conds, conds_l, rtol=1e-12)
    assert np.abs(theta_l).max() > 1e-2 and np.abs(eta_l - eta0).max() > 1e-2  # the flow does something


def test_identity_map_equals_the_literal_transcription():
    """ledh_dense.compose_identity_map against the reference's per-particle loop with H = I."""
    rng = np.random.default_rng(6)
    d, N, L = 6, 5, 4
    h = M.IdentityObservation(d)
    A0 = rng.normal(size=(d, d))
    P = A0 @ A0.T / d + 0.2 * np.eye(d)
    R = np.diag(rng.uniform(0.5, 2.0, d))
    z = rng.normal(size=d)
    eta0 = rng.normal(size=(N, d))
    Mc, cc, conds = LD.compose_identity_map(P, z, R, L)
    eta_l, theta_l, conds_l = LR.literal_flow(eta0, P, z, h, h.jacobian, R, L)
    np.testing.assert_allclose(eta0 @ Mc.T + cc, eta_l, rtol=0, atol=1e-12 * max(1.0, np.abs(eta_l).max()))
    np.testing.assert_allclose(conds, conds_l, rtol=1e-12)
    np.testing.assert_allclose(theta_l, theta_l[0], rtol=0, atol=1e-13)  # the same for every particle


# ---------------------------------------------------------------- wiring
def _wiring(d=6, like="poisson", R=None):
    g = M.ScaleTransition(0.9, d)
    Q = np.eye(d)
    if like == "poisson":
        h = M.ExpObservation(1.0, 1.0 / 3.0, d)
        ll = M.PoissonLikelihood(h)
    else:
        h = M.IdentityObservation(d)
        ll = M.GaussianLikelihood(h, np.eye(d))
    Rf = np.eye(d) if R is None else R
    tracker = TR.UKFTracker(TR.UnscentedKalmanFilter(g, h, Q, np.eye(d)), TR.UKFState(np.zeros(d), Q.copy(), 0))
    return tracker, g, h, M.GaussianTransitionDensity(g, Q), ll, Rf


def test_constructs_without_a_device(monkeypatch):
    from particle_filters_amd import _native as NV

    def no_library():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(NV, "load", no_library)
    for like in ("poisson", "gaussian"):
        tracker, g, h, lt, ll, R = _wiring(like=like)
        pf = LD.LEDHFlowPF(tracker, g, h, h.jacobian, lt, ll, R, LD.LEDHConfig(n_particles=10, n_lambda_steps=0))
        assert pf.nx == 6 and pf.n == 10 and pf.L == 1 and pf._dh is None
        assert pf.shared_jacobian_path is (like == "gaussian")
        pf2 = LD.LEDHFlowPF(tracker, g, h, None, lt, ll, R, LD.LEDHConfig(n_particles=10))
        assert pf2.Jh.__self__ is h
        with pytest.raises(NotImplementedError, match="dense LEDH path"):
            pf.tracker_covariances(np.zeros((3, 6)))
        with pytest.raises(NotImplementedError, match="dense LEDH path"):
            pf._device_tracker()
        st = LD.PFState(np.zeros((10, 6)), np.full(10, 0.1), np.zeros(6), np.eye(6))
        with pytest.raises(NotImplementedError, match="tracker"):
            pf.run(st, np.zeros((2, 6)), tracker="device")
        with pytest.raises(NotImplementedError, match="process_noise"):
            pf.run(st, np.zeros((2, 6)), process_noise="device")
        with pytest.raises(ValueError, match="replay"):
            pf.run(st, np.zeros((2, 6)), process_noise="host")
        pf.close()


def test_refusals():
    tracker, g, h, lt, ll, R = _wiring()
    cfg = LD.LEDHConfig(n_particles=10)
    with pytest.raises(NotImplementedError, match="diagonal flow R"):
        LD.LEDHFlowPF(tracker, g, h, h.jacobian, lt, ll, np.eye(6) + 0.1, cfg)
    with pytest.raises(np.linalg.LinAlgError):
        LD.LEDHFlowPF(tracker, g, h, h.jacobian, lt, ll, np.diag([1.0, 1.0, 0.0, 1.0, 1.0, 1.0]), cfg)
    with pytest.raises(np.linalg.LinAlgError):
        LD.LEDHFlowPF(tracker, g, h, h.jacobian, lt, ll, np.diag([1.0, -1.0, 1.0, 1.0, 1.0, 1.0]), cfg)
    with pytest.raises(NotImplementedError, match="jacobian_h"):
        LD.LEDHFlowPF(tracker, g, h, lambda x: np.eye(6), lt, ll, R, cfg)
    with pytest.raises(NotImplementedError, match="rng_mode"):
        LD.LEDHFlowPF(tracker, g, h, h.jacobian, lt, ll, R, cfg, rng_mode="device")
    with pytest.raises(NotImplementedError, match="log_like_pdf"):
        LD.LEDHFlowPF(tracker, g, h, h.jacobian, lt, lambda z, x: 0.0, R, cfg)
    with pytest.raises(NotImplementedError, match="log_trans_pdf"):
        LD.LEDHFlowPF(tracker, g, h, h.jacobian, lambda a, b: 0.0, ll, R, cfg)
    with pytest.raises(NotImplementedError, match="h must be"):
        LD.LEDHFlowPF(tracker, g, M.ExpHalfObservation(np.ones(6)), None, lt, ll, R, cfg)
    with pytest.raises(NotImplementedError, match="ScaleTransition"):
        LD.LEDHFlowPF(tracker, M.SVTransition(0.9), M.SVLogSqObservation(1.0), None, lt, ll, R, cfg)
    # the engine's class keeps refusing this wiring, and says where it runs
    with pytest.raises(NotImplementedError, match=r"particle_filters_amd\.ledh_dense"):
        LE.LEDHFlowPF(tracker, g, h, h.jacobian, lt, ll, R, LE.LEDHConfig(n_particles=10))
    assert not M.is_device_model(g, h)


# ---------------------------------------------------------------- the chunk plan
def test_chunk_plan_under_sanitizers():
    """pf::ledh_dense_plan (csrc/pf_ledh_dense_plan.h) in a stand-alone program under AddressSanitizer +
    UndefinedBehaviorSanitizer (tests/host/pf_ledh_dense_host_check.cpp): d = 1024 with N = 1048576, a cap
    below one particle's workspace, exact multiples and a remainder chunk of one."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(repo, "build", "pf_ledh_dense_host_check")
    if not os.path.exists(exe):  # built by __graft_entry__.build(); here if the test runs first
        subprocess.run(["make", "-C", os.path.join(repo, "particle_filters_amd", "csrc"), "hostcheck"],
                       check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_entries_validate_arguments_without_a_device():
    """Null handles are PF_E_ARG; the checks on n_lambda, R_diag and the handle's observation kind come
    before any device call (csrc/pf_edh_dense.hip: ledh_check), exercised on the GPU in
    tests/test_gpu_sn_ledh.py where a handle exists."""
    from particle_filters_amd import _native as NV

    lib = NV.load()
    a = np.zeros(4)
    assert lib.pf_ledh_dense_step(None, NV.dptr(a), NV.dptr(a), NV.dptr(a), None, 1, 0, None, None, None) == NV.PF_E_ARG
    assert lib.pf_ledh_dense_run(None, NV.dptr(a), NV.dptr(a), NV.dptr(a), None, 1, 1, 0, NV.dptr(a), NV.dptr(a),
                                 None, None) == NV.PF_E_ARG
