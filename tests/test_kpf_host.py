"""CPU checks of the kernel particle flow filter (no GPU).

* the NumPy restatement (tests/kpf_restatement.py) against the reference's own runs
  (tests/golden/kpf_runs.npz, tests/golden/make_golden_kpf.py) at 1e-12 x max(1, max|x|) - the
  bound the generator asserted; the prototype's worst difference was a few 1e-15;
* ``gaspari_cohn`` / ``build_localization_matrix`` against stored reference values (the same
  expressions in the same order: a few ulp);
* the pseudo-time schedule (steps, s, ds_history) bitwise equal to the reference's, through the
  host-only helper ``kernel_pf.pseudo_time_schedule``;
* the ValueError / NotImplementedError paths that need no device;
* the C ABI of include/pf_kpf.h: the header parses to exactly the ``pf_kpf_`` names of
  ``_native.SIGNATURES``, the library exports every name, and ``pf_kpf_create``
  rejects bad arguments before it touches a device.
"""

import ctypes as C
import os
import re

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import kernel_pf as KP
from particle_filters_amd import models as M
from tests import kpf_restatement as KR

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "kpf_runs.npz"))
NAMES = [str(n) for n in GOLD["names"]]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    h, R, cfg, X, y, ls, g = KR.golden_case(GOLD, name)
    rs = KR.analyze(h, R, cfg, X, y, ls)
    scale = max(1.0, float(np.max(np.abs(g["particles"]))))
    err = float(np.max(np.abs(rs["particles"] - g["particles"])))
    print(f"{name}: restatement vs reference {err:.3e}")
    assert err <= 1e-12 * scale
    assert rs["ds_history"] == list(g["ds_history"]) and rs["s"] == float(g["s"]) and rs["steps"] == int(g["steps"])
    assert rs["n_clipped"] == list(g["n_clipped"])
    assert rs["clip_margin"] > 1e-6  # no clip decision sits on a rounding error


def test_golden_covers_the_branches():
    g = lambda n, k: GOLD[f"{n}__{k}"]  # noqa: E731
    assert int(np.sum(g("c_clip", "n_clipped"))) > 0 and int(np.sum(g("h_small_np", "n_clipped"))) > 0
    assert len(set(g("c_clip", "ds_history").tolist())) > 1            # non-uniform ds
    assert float(g("e_capped", "s")) < 1.0 and int(g("e_capped", "steps")) == 3
    assert 0.0 in g("f_minsteps", "ds_history").tolist()               # a zero-ds step, then the early break
    assert int(g("f_minsteps", "steps")) < 8
    assert np.all(g("k_constant", "X")[:, 2] == 2.0)


@pytest.mark.parametrize("name", NAMES)
def test_schedule_bitwise(name):
    _, _, cfg, _, _, _, g = KR.golden_case(GOLD, name)
    hist, s, steps = KP.pseudo_time_schedule(cfg)
    assert steps == int(g["steps"])
    assert s == float(g["s"])
    assert np.array_equal(np.asarray(hist), g["ds_history"])


def test_localization_helpers_match_reference_values():
    np.testing.assert_allclose(KP.gaspari_cohn(GOLD["gc__r"]), GOLD["gc__values"], rtol=0, atol=4e-16)
    np.testing.assert_allclose(KP.build_localization_matrix(7, 2.0), GOLD["gc__matrix_7_2"], rtol=0, atol=4e-16)
    np.testing.assert_allclose(KP.build_localization_matrix(5, 1.5, GOLD["gc__metric"]), GOLD["gc__matrix_metric"],
                               rtol=0, atol=4e-16)
    assert np.array_equal(KP.build_localization_matrix(4, np.inf), np.ones((4, 4)))
    assert KP.gaspari_cohn(np.array([0.0]))[0] == 1.0 and KP.gaspari_cohn(np.array([2.5]))[0] == 0.0
    with pytest.raises(ValueError, match="metric must be"):
        KP.build_localization_matrix(4, 1.0, np.zeros((3, 3)))


def test_public_names_and_defaults():
    cfg = KP.KPFConfig()
    assert (cfg.ds_init, cfg.ds_min, cfg.c_move_max, cfg.min_steps, cfg.max_steps) == (0.2, 1e-3, 2.0, 5, 100)
    assert (cfg.kernel_type, cfg.lengthscale_mode, cfg.fixed_lengthscale, cfg.reg) == ("diagonal", "std", 1.0, 1e-6)
    assert np.isinf(cfg.localization_radius) and cfg.random_order is True
    st = KP.KPFState(np.zeros((2, 1)), np.full(2, 0.5), 1.0, 5)
    assert st.ds_history is None and st.n_clipped is None
    assert list(KP.KPFState.__dataclass_fields__)[-1] == "n_clipped"


def test_model_errors_without_a_device():
    R = np.eye(2)
    with pytest.raises(NotImplementedError, match="LinearObservation"):
        KP.KernelParticleFilter(KP.Model(lambda x: x[:2], lambda x: np.eye(2, 3), R))
    with pytest.raises(NotImplementedError, match="ExpHalfObservation"):
        KP.KernelParticleFilter(KP.Model(M.BearingsObservation(9), None, R))
    h = M.LinearObservation(np.ones((2, 3)))
    with pytest.raises(NotImplementedError, match="jacobian"):
        KP.KernelParticleFilter(KP.Model(h, lambda x: np.ones((2, 3)), R))
    with pytest.raises(ValueError):
        KP.KernelParticleFilter(KP.Model(h, h.jacobian, np.eye(3)))
    kf = KP.KernelParticleFilter(KP.Model(h, h.jacobian, R))
    with pytest.raises(ValueError):
        kf.analyze(np.zeros(3), np.zeros(2))            # not (Np, n)
    with pytest.raises(ValueError):
        kf.analyze(np.zeros((5, 4)), np.zeros(2))       # wrong state dimension
    with pytest.raises(ValueError):
        kf.analyze(np.zeros((5, 3)), np.zeros(3))       # wrong observation dimension
    X = np.random.default_rng(0).normal(size=(5, 3))
    with pytest.raises(ValueError, match=r"lengthscales must be shape \(n,\)"):
        kf.analyze(X, np.zeros(2), lengthscales=np.ones(2))


# ----------------------------------------------------------------------------- C ABI
def header_functions():
    src = open(os.path.join(REPO, "include", "pf_kpf.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_][A-Za-z0-9_]*\s*\*?\s*(pf_[a-z_0-9]+)\s*\(", src,
                                 flags=re.M)))


def test_kpf_binding_covers_header_exactly():
    names = header_functions()
    kpf = {n: v for n, v in NV.SIGNATURES.items() if n.startswith("pf_kpf_")}
    assert names == sorted(kpf)
    for must in ("pf_kpf_create", "pf_kpf_destroy", "pf_kpf_model_supported", "pf_kpf_analyze", "pf_kpf_stream",
                 "pf_kpf_synchronize"):
        assert must in names
    raw = C.CDLL(NV.LIB_PATH)
    assert not [n for n in names if not hasattr(raw, n)]
    lib = NV.load()
    for n, (res, args) in kpf.items():
        assert getattr(lib, n).argtypes == args and getattr(lib, n).restype == res


def test_kpf_model_registry():
    lib = NV.load()
    assert lib.pf_kpf_model_supported(40, 10, NV.PF_OBS_LINEAR)
    assert lib.pf_kpf_model_supported(3, 3, NV.PF_OBS_EXP_HALF)
    assert not lib.pf_kpf_model_supported(5, 4, NV.PF_OBS_EXP_HALF)
    assert lib.pf_kpf_model_supported(4, 9, NV.PF_OBS_ACOUSTIC)
    assert not lib.pf_kpf_model_supported(6, 9, NV.PF_OBS_ACOUSTIC)
    assert not lib.pf_kpf_model_supported(9, 2, NV.PF_OBS_BEARINGS)
    assert not lib.pf_kpf_model_supported(5, 5, NV.PF_OBS_SV_EXACT)
    assert not lib.pf_kpf_model_supported(0, 1, NV.PF_OBS_LINEAR)


def _create(n_particles=10, kernel_type=0, kind=NV.PF_OBS_LINEAR, R=None, null=None):
    h = M.LinearObservation(np.ones((2, 3)))
    op = np.ascontiguousarray(h.params())
    Rm = np.ascontiguousarray(np.eye(2) if R is None else R, dtype=float)
    d = NV.ModelDesc(3, 2, 0, kind, None, 0, NV.dptr(op), op.size, None, NV.dptr(Rm))
    o = NV.KpfOpts(n_particles, kernel_type, 0)
    hd = C.c_void_p()
    st = NV.load().pf_kpf_create(None if null == "model" else C.byref(d), None if null == "opts" else C.byref(o),
                                 None if null == "out" else C.byref(hd))
    return st, hd


def test_kpf_create_rejects_bad_arguments_before_touching_a_device():
    lib = NV.load()
    st, hd = _create(n_particles=0)
    assert st == NV.PF_E_ARG and not hd.value
    assert "n_particles" in lib.pf_last_error().decode()
    st, hd = _create(kernel_type=2)
    assert st == NV.PF_E_ARG and not hd.value
    assert "kernel_type" in lib.pf_last_error().decode()
    for null in ("model", "opts", "out"):
        assert _create(null=null)[0] == NV.PF_E_ARG
    st, hd = _create(kind=NV.PF_OBS_BEARINGS)
    assert st == NV.PF_E_UNSUPPORTED and not hd.value
    with pytest.raises(NotImplementedError):
        NV.check(st)
    st, hd = _create(R=np.array([[1.0, 2.0], [2.0, 1.0]]))
    assert st == NV.PF_E_NOT_PD and not hd.value
    assert lib.pf_kpf_analyze(None, None, None, None, None, None, None, None, 0, 1.0, None, None) == NV.PF_E_ARG
    assert lib.pf_kpf_synchronize(None) == NV.PF_E_ARG
    assert lib.pf_kpf_stream(None) is None
    lib.pf_kpf_destroy(None)
