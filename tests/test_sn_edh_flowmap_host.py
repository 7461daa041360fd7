"""CPU tests of the device-composed EDH flow map's host side: the Cholesky-form restatement
(tests/sn_edh_flowmap_restatement.py) against ``edh.compose_flow_map`` on every step of the stored
sensor-network cases, the ``flow_map`` keyword of ``EDHFlowPF``, and the new C-ABI names.
"""

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import edh as E
from particle_filters_amd import models as M
from particle_filters_amd import trackers as TR
from tests import sn_edh_flowmap_restatement as FR
from tests import sn_edh_restatement as RS


@pytest.fixture(scope="module")
def golden():
    return RS.load()


@pytest.mark.parametrize("name", list(RS.CASES))
def test_cholesky_form_matches_compose_flow_map(golden, name):
    c = RS.Case(golden, name)
    g, h, _, _, R = c.objects()
    tr = c.tracker(g, h, R)
    obs = "exp" if c.wiring == "skewt" else "identity"
    worst = dict(M=0.0, c=0.0, cond=0.0)
    for t in range(c.T):
        _, P = tr.predict()
        P = np.asarray(P, float).reshape(c.d, c.d)
        P = 0.5 * (P + P.T)
        etabar = g(np.asarray(tr.get_past_mean(), float).reshape(c.d), None, np.zeros(c.d))
        Mh, ch, conds, _ = E.compose_flow_map(P, etabar, c.Z[t], h, h.jacobian, R, c.L, c.integrator)
        Mr, cr, trace = FR.compose(P, etabar, c.Z[t], obs, c.m1, c.m2, np.diag(R), c.L, c.integrator)
        tr.update(c.Z[t])
        eM = np.abs(Mr - Mh).max() / max(1.0, np.abs(Mh).max())
        ec = np.abs(cr - ch).max() / max(1.0, np.abs(ch).max())
        worst = dict(M=max(worst["M"], eM), c=max(worst["c"], ec), cond=max(worst["cond"], max(conds)))
        assert eM <= RS.TOL_X and ec <= RS.TOL_X, f"t={t}: M {eM:.2e} c {ec:.2e}"
        np.testing.assert_array_equal(trace[0], etabar)
    print(f"{name}: Cholesky form vs compose_flow_map M {worst['M']:.2e} c {worst['c']:.2e} cond(S) {worst['cond']:.3g}")


def _wiring(d=4, R=None, **kw):
    g, h, Q = M.ScaleTransition(0.9, d), M.ExpObservation(1.0, 1.0 / 3.0, d), np.eye(d)
    R = np.eye(d) if R is None else R
    tr = TR.UKFTracker(TR.UnscentedKalmanFilter(g, h, Q, np.eye(d)), TR.UKFState(np.zeros(d), Q.copy(), 0))
    return E.EDHFlowPF(tr, g, h, h.jacobian, M.GaussianTransitionDensity(g, Q), M.PoissonLikelihood(h), R,
                       E.EDHConfig(n_particles=8), **kw)


def test_flow_map_keyword_is_validated_without_a_device():
    assert _wiring().flow_map == "host"
    assert _wiring(flow_map="device").flow_map == "device"
    with pytest.raises(ValueError, match="flow_map"):
        _wiring(flow_map="gpu")
    with pytest.raises(TypeError):  # keyword-only
        E.EDHFlowPF(None, None, None, None, None, None, np.eye(1), None, "host", 0, "device")
    full = np.eye(4)
    full[0, 1] = full[1, 0] = 0.1
    _wiring(R=full)  # the host composition takes a full flow R
    with pytest.raises(NotImplementedError, match="diagonal"):
        _wiring(R=full, flow_map="device")
    for bad in (0.0, -1.0, np.inf, np.nan):
        Rb = np.eye(4)
        Rb[2, 2] = bad
        with pytest.raises(np.linalg.LinAlgError):
            _wiring(R=Rb, flow_map="device")
    # the combinations the dense path refuses keep raising with the keyword
    with pytest.raises(NotImplementedError, match="rng_mode"):
        _wiring(flow_map="device", rng_mode="device")


def test_the_new_entries_are_bound():
    for name in ("pf_edh_dense_flow_step", "pf_edh_dense_flow_run", "pf_edh_dense_get_map"):
        assert name in NV.SIGNATURES
    assert len(NV.SIGNATURES["pf_edh_dense_flow_step"][1]) == 12
    assert len(NV.SIGNATURES["pf_edh_dense_flow_run"][1]) == 15
