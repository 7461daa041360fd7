"""Host checks of the device process noise of the sensor-network flows (no GPU, no compute calls):
``noise.DeviceGaussianNoise`` validates its position in the Philox counter space; the dense classes refuse it
together with a replayed V and keep refusing the strings ``process_noise="device"`` / ``rng_mode="device"``;
the engine-path classes refuse the object and name their own ``process_noise="device"``; the C ABI declares
and exports the three entries.
"""

import ctypes as C

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import edh as E
from particle_filters_amd import ledh as LE
from particle_filters_amd import ledh_dense as LD
from particle_filters_amd import models as M
from particle_filters_amd import trackers as TR
from particle_filters_amd.noise import DeviceGaussianNoise


# ---------------------------------------------------------------- the object
def test_seed_and_epoch_are_kept_and_the_epoch_can_move():
    dn = DeviceGaussianNoise(2 ** 64 - 1, epoch=2 ** 32 - 1)
    assert dn.seed == 2 ** 64 - 1 and dn.epoch == 2 ** 32 - 1
    dn = DeviceGaussianNoise(np.int64(7))
    assert (dn.seed, dn.epoch) == (7, 0) and type(dn.seed) is int
    dn.epoch += 3
    assert dn.epoch == 3
    assert "seed=7" in repr(dn) and "epoch=3" in repr(dn)
    with pytest.raises(AttributeError):
        dn.seed = 8


@pytest.mark.parametrize("seed, epoch, exc", [
    (-1, 0, ValueError), (2 ** 64, 0, ValueError), (0, -1, ValueError), (0, 2 ** 32, ValueError),
    (1.0, 0, TypeError), ("1", 0, TypeError), (None, 0, TypeError), (True, 0, TypeError), (0, 0.0, TypeError),
    (0, None, TypeError), (0, False, TypeError),
])
def test_anything_else_is_refused(seed, epoch, exc):
    with pytest.raises(exc):
        DeviceGaussianNoise(seed, epoch)


def test_the_epoch_cannot_be_moved_out_of_range():
    dn = DeviceGaussianNoise(1, 2 ** 32 - 1)
    with pytest.raises(ValueError):
        dn.epoch += 1
    assert dn.epoch == 2 ** 32 - 1
    with pytest.raises(TypeError):
        dn.epoch = 1.5


# ---------------------------------------------------------------- the dense classes
D, NP = 4, 8


def _wiring(exp):
    g = M.ScaleTransition(0.9, D)
    h = M.ExpObservation(1.0, 1.0 / 3.0, D) if exp else M.IdentityObservation(D)
    Q = np.eye(D)
    ll = M.PoissonLikelihood(h) if exp else M.GaussianLikelihood(h, Q)
    tr = TR.UKFTracker(TR.UnscentedKalmanFilter(g, h, Q, Q), TR.UKFState(np.zeros(D), Q.copy(), 0))
    return tr, g, h, h.jacobian, M.GaussianTransitionDensity(g, Q), ll, Q


def _dense(kind, **kw):
    if kind == "edh":
        return E.EDHFlowPF(*_wiring(True), E.EDHConfig(n_particles=NP), **kw)
    return LD.LEDHFlowPF(*_wiring(kind == "ledh_exp"), LD.LEDHConfig(n_particles=NP), **kw)


def _state():
    return E.PFState(np.zeros((NP, D)), np.full(NP, 1.0 / NP), np.zeros(D), np.eye(D))


@pytest.mark.parametrize("kind", ["edh", "ledh_exp", "ledh_identity"])
def test_a_replayed_V_beside_the_object_is_refused_before_any_device_call(kind):
    pf = _dense(kind)
    dn = DeviceGaussianNoise(3, 5)
    T = 2
    with pytest.raises(ValueError, match="replay"):
        pf.run(_state(), np.zeros((T, D)), process_noise=dn, replay=(np.zeros((T, NP, D)), np.zeros(T)))
    with pytest.raises(ValueError, match="overflows"):
        pf.run(_state(), np.zeros((T, D)), process_noise=DeviceGaussianNoise(3, 2 ** 32 - 2), replay=(None, np.zeros(T)))
    with pytest.raises(ValueError, match="overflows"):
        pf.step(_state(), np.zeros(D), process_noise_sampler=DeviceGaussianNoise(3, 2 ** 32 - 1))
    assert dn.epoch == 5 and pf._dh is None  # nothing ran: no handle was made


@pytest.mark.parametrize("kind", ["edh", "ledh_exp", "ledh_identity"])
def test_the_strings_still_raise_on_the_dense_classes(kind):
    with pytest.raises(NotImplementedError, match="rng_mode='device'"):
        _dense(kind, rng_mode="device")
    pf = _dense(kind)
    with pytest.raises(NotImplementedError, match="process_noise='device'"):
        pf.run(_state(), np.zeros((2, D)), process_noise="device")
    with pytest.raises(NotImplementedError, match="tracker='device'"):
        pf.run(_state(), np.zeros((2, D)), process_noise="none", tracker="device")
    with pytest.raises(ValueError):
        pf.run(_state(), np.zeros((2, D)), process_noise="philox")
    with pytest.raises(TypeError):
        pf.process_noise_draws("device")
    with pytest.raises(TypeError):
        pf.init_from_gaussian(np.zeros(D), np.eye(D), draws="device")
    with pytest.raises(TypeError):
        pf.init_from_gaussian(np.zeros(D), np.eye(D), DeviceGaussianNoise(1))  # draws is keyword-only
    assert pf._dh is None


# ---------------------------------------------------------------- the engine-path classes
class _Engine:
    """The members the engine classes' refusals read, without a handle (no device is touched)."""

    n, nx, nz = 4, 1, 1


@pytest.mark.parametrize("cls", [LE.LEDHFlowPF, E.EDHFlowPF])
def test_the_engine_path_classes_refuse_the_object(cls):
    dn = DeviceGaussianNoise(1)
    pf = _Engine()
    with pytest.raises(NotImplementedError, match="process_noise='device'"):
        cls._step_inputs(pf, np.zeros(1), None, dn)
    with pytest.raises(NotImplementedError, match="process_noise='device'"):
        cls._noise_mode(pf, dn, None, 3)
    pf._dense = False
    with pytest.raises(NotImplementedError):
        E.EDHFlowPF.process_noise_draws(pf, dn)
    with pytest.raises(NotImplementedError):
        E.EDHFlowPF.init_from_gaussian(pf, np.zeros(1), np.eye(1), draws=dn)
    assert dn.epoch == 0


# ---------------------------------------------------------------- the C ABI
def test_the_entries_are_declared_bound_and_exported():
    lib = C.CDLL(NV.LIB_PATH)
    for name in ("pf_edh_dense_set_noise", "pf_edh_dense_noise_draws", "pf_edh_dense_init_gaussian"):
        assert name in NV.SIGNATURES and hasattr(lib, name)
    assert NV.SIGNATURES["pf_edh_dense_set_noise"][1] == [C.c_void_p, C.c_uint64, C.c_uint32]
    # null handles are argument errors, reported without a device
    lib = NV.load()
    assert lib.pf_edh_dense_set_noise(None, 1, 0) == NV.PF_E_ARG
    assert lib.pf_edh_dense_noise_draws(None, 1, 0, None) == NV.PF_E_ARG
    assert lib.pf_edh_dense_init_gaussian(None, None, None, 1, 0, None, None) == NV.PF_E_ARG
