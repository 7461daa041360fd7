"""CPU checks around the device UKF tracker (``trackers.DeviceUKFTracker``, the pf_ukf_dense_* entries):

* the extended-precision restatement (tests/sn_ukf_restatement.py) restates the filter of
  ``trackers.UnscentedKalmanFilter``: on the five stored cases the host tracker stays within 1e-7 of it in
  the predicted covariances, past means and posteriors (the largest distance measured is 1.41e-8, the past
  means of skewt144: the six-digit cancellation of the unscented weights at alpha = 1e-3);
* ``DeviceUKFTracker`` rejects what it does not run at construction, without touching the library;
* the new C-ABI entries reject bad arguments before a device is touched;
* the host algebra of the tracker's create (the unscented-transform constants, the splits) passes its
  stand-alone check under the host sanitizers.
"""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import edh as E
from particle_filters_amd import ledh_dense as LD
from particle_filters_amd import models as M
from particle_filters_amd import trackers as TR
from tests import sn_edh_restatement as RS
from tests import sn_ukf_restatement as UR


@pytest.fixture(scope="module")
def golden():
    return RS.load()


@pytest.mark.parametrize("name", list(RS.CASES))
def test_host_tracker_is_the_restated_filter(golden, name):
    c = RS.Case(golden, name)
    ref, host = UR.free_run(c), UR.host_run(c)
    dist = {q: UR.rel(host[q], ref[q]) for q in UR.QUANTITIES}
    print(f"{name}: host tracker vs long double " + " ".join(f"{q} {dist[q]:.2e}" for q in UR.QUANTITIES))
    for q in UR.QUANTITIES:
        assert dist[q] <= 1e-7, f"{name} {q}: {dist[q]:.2e}"


def test_float_form_is_the_same_filter(golden):
    c = RS.Case(golden, "skewt25_odd")
    ref, flt = UR.free_run(c), UR.free_run(c, float)
    for q in UR.QUANTITIES:
        assert flt[q].dtype == np.float64 and UR.rel(flt[q], ref[q]) <= 1e-7, q


def _ukf(d=6, g=None, h=None, nq=None, nr=None):
    g = M.ScaleTransition(0.9, d) if g is None else g
    h = M.ExpObservation(1.0, 1.0 / 3.0, d) if h is None else h
    return TR.UnscentedKalmanFilter(g, h, np.eye(d if nq is None else nq), np.eye(d if nr is None else nr))


def _state(d=6):
    return TR.UKFState(mean=np.zeros(d), cov=np.eye(d), t=0)


def test_device_tracker_constructs_and_rejects_without_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(NV, "load", no_library)
    for h in (M.ExpObservation(1.0, 1.0 / 3.0, 6), M.IdentityObservation(6)):
        tr = TR.DeviceUKFTracker(_ukf(h=h), _state(), device=0)
        assert tr.nx == 6 and tr._h is None
        tr.close()
    with pytest.raises(NotImplementedError, match="UnscentedKalmanFilter"):
        TR.DeviceUKFTracker(TR.ExtendedKalmanFilter(lambda x, u: x, lambda x: x, np.eye(6), np.eye(6)), _state())
    with pytest.raises(NotImplementedError, match="ScaleTransition"):
        TR.DeviceUKFTracker(_ukf(g=lambda x, u=None: 0.9 * x), _state())
    with pytest.raises(NotImplementedError, match="ScaleTransition"):
        TR.DeviceUKFTracker(_ukf(g=M.LinearTransition(0.9 * np.eye(6))), _state())
    with pytest.raises(NotImplementedError, match="IdentityObservation"):
        TR.DeviceUKFTracker(_ukf(h=lambda x: x), _state())
    with pytest.raises(NotImplementedError, match="nz = nx"):
        TR.DeviceUKFTracker(_ukf(nr=5), _state())
    with pytest.raises(NotImplementedError, match="state dimension"):
        TR.DeviceUKFTracker(_ukf(h=M.IdentityObservation(5)), _state())
    with pytest.raises(NotImplementedError, match="1024"):
        TR.DeviceUKFTracker(_ukf(d=1025), _state(1025))
    with pytest.raises(ValueError, match="initial state"):
        TR.DeviceUKFTracker(_ukf(), _state(5))
    # a filter takes it as its tracker, and tracker="device" keeps its meaning (an EKF built by the engine)
    g, h = M.ScaleTransition(0.9, 6), M.ExpObservation(1.0, 1.0 / 3.0, 6)
    tr = TR.DeviceUKFTracker(_ukf(g=g, h=h), _state())
    lt, ll = M.GaussianTransitionDensity(g, np.eye(6)), M.PoissonLikelihood(h)
    st = E.PFState(np.zeros((10, 6)), np.full(10, 0.1), np.zeros(6), np.eye(6))
    for pf in (E.EDHFlowPF(tr, g, h, h.jacobian, lt, ll, np.eye(6), E.EDHConfig(n_particles=10), flow_map="device"),
               E.EDHFlowPF(tr, g, h, h.jacobian, lt, ll, np.eye(6), E.EDHConfig(n_particles=10)),
               LD.LEDHFlowPF(tr, g, h, h.jacobian, lt, ll, np.eye(6), LD.LEDHConfig(n_particles=10))):
        assert pf.tracker is tr
        with pytest.raises(NotImplementedError, match="tracker"):
            pf.run(st, np.zeros((2, 6)), tracker="device", process_noise="none")
        pf.close()


def _model(d=4, **kw):
    Q, R = np.eye(d), np.eye(d)
    f = dict(nx=d, obs_kind=NV.PF_EDH_OBS_EXP, g_alpha=0.9, m1=1.0, m2=1.0 / 3.0, alpha=1e-3, beta=2.0, kappa=0.0,
             jitter=0.0, Q=NV.dptr(Q), R=NV.dptr(R))
    f.update(kw)
    return NV.UkfDenseModel(**f), (Q, R)


def test_abi_entries_reject_bad_arguments_before_a_device_is_touched():
    lib = NV.load()
    h = C.c_void_p()
    bad = [dict(nx=0), dict(nx=1025), dict(obs_kind=7), dict(g_alpha=np.nan), dict(m2=np.inf), dict(alpha=0.0),
           dict(alpha=np.nan), dict(kappa=-4.0), dict(beta=np.inf), dict(jitter=-1e-9), dict(jitter=np.nan),
           dict(Q=None), dict(R=None)]
    for kw in bad:
        model, keep = _model(**kw)
        assert lib.pf_ukf_dense_create(C.byref(model), 0, C.byref(h)) == NV.PF_E_ARG, kw
        assert not h.value
    Qn = np.eye(4)
    Qn[1, 2] = np.nan
    model, keep = _model(Q=NV.dptr(Qn))
    assert lib.pf_ukf_dense_create(C.byref(model), 0, C.byref(h)) == NV.PF_E_ARG
    assert "finite" in lib.pf_last_error().decode()
    model, keep = _model()
    assert lib.pf_ukf_dense_create(C.byref(model), -1, C.byref(h)) == NV.PF_E_ARG
    assert lib.pf_ukf_dense_create(None, 0, C.byref(h)) == NV.PF_E_ARG
    assert lib.pf_ukf_dense_create(C.byref(model), 0, None) == NV.PF_E_ARG
    with pytest.raises(ValueError):
        NV.check(NV.PF_E_ARG)
    x, P = np.zeros(4), np.eye(4)
    assert lib.pf_ukf_dense_set_state(None, NV.dptr(x), NV.dptr(P)) == NV.PF_E_ARG
    assert lib.pf_ukf_dense_get_state(None, NV.dptr(x), NV.dptr(P)) == NV.PF_E_ARG
    assert lib.pf_ukf_dense_predict(None, None) == NV.PF_E_ARG
    assert lib.pf_ukf_dense_update(None, NV.dptr(x)) == NV.PF_E_ARG
    assert lib.pf_ukf_dense_get_past_mean(None, NV.dptr(x)) == NV.PF_E_ARG
    assert lib.pf_ukf_dense_sequence(None, NV.dptr(x), None, 1, None, None, None, None) == NV.PF_E_ARG
    lib.pf_ukf_dense_destroy(None)
    m, cv = np.empty((1, 4)), np.empty((1, 4, 4))
    assert lib.pf_edh_dense_flow_run_tracked(None, None, NV.dptr(x), NV.dptr(x), None, 1, 2, 0, 0, NV.dptr(m),
                                             NV.dptr(cv), None, None, None) == NV.PF_E_ARG
    assert lib.pf_edh_dense_flow_step_tracked(None, None, NV.dptr(x), NV.dptr(x), None, 2, 0, 0, None, None, None,
                                              None) == NV.PF_E_ARG


def test_unscented_constants_under_sanitizers():
    """pf::ukf_plan (csrc/pf_ukf_dense_plan.h) in a stand-alone program under AddressSanitizer +
    UndefinedBehaviorSanitizer (tests/host/pf_ukf_dense_host_check.cpp)."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(repo, "build", "pf_ukf_dense_host_check")
    if not os.path.exists(exe):  # built by __graft_entry__.build(); here if the test runs first
        subprocess.run(["make", "-C", os.path.join(repo, "particle_filters_amd", "csrc"), "hostcheck"],
                       check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
