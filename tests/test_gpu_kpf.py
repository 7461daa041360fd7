"""HIP kernel particle flow filter vs the reference's own outputs (-m gpu, MI355X).

tests/golden/kpf_runs.npz holds the reference KernelParticleFilter's runs on fixed seeds
(tests/golden/make_golden_kpf.py); at the edge sizes the reference is the NumPy restatement
(tests/kpf_restatement.py), which the generator checked against the reference at each of them.

Tolerance (fp64 engine): the all-pairs sums run in another order than NumPy's, R^-1 and 1 / l are
applied as products, and exp is the device library's, so agreement is to rounding amplified by the
flow: particles within 1e-9 x max(1, max|x|), the tolerance of the other fp64 flow filters
(tests/test_gpu_edh.py).  The schedule, the clip counts and the weights are equal.
"""

import os

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import kernel_pf as KP
from particle_filters_amd import models as M
from tests import kpf_restatement as KR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(__file__)
GOLD = np.load(os.path.join(HERE, "golden", "kpf_runs.npz"))
NAMES = [str(n) for n in GOLD["names"]]
TOL = 1e-9

# Np x nx x kernel: the full cross but for 1001 x 40, whose NumPy restatement alone costs 3 to 6 s
# of CPU per kernel.  Its paths are covered: Np = 1001 (16 tiles of 64 and a tail of 41) runs at
# nx = 1 and 3, nx = 40 at every Np up to 257 (five tiles, a tail of 1), and in the diagonal
# kernel nx is only the grid's second dimension.
EDGES = [(n, x, k) for k in ("diagonal", "scalar") for n in KR.EDGE_NP for x in KR.EDGE_NX
         if not (n == 1001 and x == 40)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert NV.device_count() > 0, "no HIP device visible: -m gpu tests must run on an MI355X"


def run_case(name, rng=None):
    h, R, cfg, X, y, ls, g = KR.golden_case(GOLD, name)
    kf = KP.KernelParticleFilter(KP.Model(h, h.jacobian, R), cfg)
    try:
        return kf.analyze(X, y, lengthscales=ls, rng=rng), g
    finally:
        kf.close()


@pytest.mark.parametrize("name", NAMES)
def test_golden_case(name):
    rng = np.random.default_rng(int(GOLD[name + "__rng_seed"])) if name + "__rng_seed" in GOLD.files else None
    st, g = run_case(name, rng)
    Np = g["particles"].shape[0]
    scale = max(1.0, float(np.max(np.abs(g["particles"]))))
    err = float(np.max(np.abs(st.particles - g["particles"])))
    print(f"KPF golden {name}: max particle error {err:.3e} (scale {scale:.3g})")
    assert np.all(np.isfinite(st.particles))
    assert err <= TOL * scale
    assert st.s == float(g["s"]) and st.steps == int(g["steps"])
    assert st.ds_history == list(g["ds_history"])
    assert st.n_clipped == list(g["n_clipped"])
    assert np.array_equal(st.weights, np.full(Np, 1.0 / Np))
    if rng is not None:  # the caller's generator was advanced exactly as the reference advances it
        assert rng.random() == float(g["next_draw"])


@pytest.mark.parametrize("Np,nx,kernel", EDGES)
def test_edge_size_matches_restatement(Np, nx, kernel):
    h, R, cfg, X, y = KR.edge_case(Np, nx, kernel)
    rs = KR.analyze(h, R, cfg, X, y)
    kf = KP.KernelParticleFilter(KP.Model(h, h.jacobian, R), cfg)
    try:
        st = kf.analyze(X, y)
    finally:
        kf.close()
    scale = max(1.0, float(np.max(np.abs(rs["particles"]))))
    err = float(np.max(np.abs(st.particles - rs["particles"])))
    print(f"KPF edge {kernel} {Np}x{nx}: max particle error {err:.3e} (scale {scale:.3g})")
    assert np.all(np.isfinite(st.particles))
    assert err <= TOL * scale
    assert (st.s, st.steps, st.ds_history) == (rs["s"], rs["steps"], rs["ds_history"])
    assert st.n_clipped == rs["n_clipped"]
    assert np.array_equal(st.weights, np.full(Np, 1.0 / Np))


@pytest.mark.parametrize("name", ["a_l96", "g_tail"])
def test_two_runs_bitwise_equal(name):
    a, _ = run_case(name)
    b, _ = run_case(name)
    assert np.array_equal(a.particles, b.particles) and a.n_clipped == b.n_clipped
    # and a second call on the same handle
    h, R, cfg, X, y, ls, _ = KR.golden_case(GOLD, name)
    kf = KP.KernelParticleFilter(KP.Model(h, h.jacobian, R), cfg)
    try:
        c = kf.analyze(X, y, lengthscales=ls)
        d = kf.analyze(X, y, lengthscales=ls)
    finally:
        kf.close()
    assert np.array_equal(c.particles, a.particles) and np.array_equal(d.particles, a.particles)


@pytest.mark.parametrize("name", ["a_l96", "b_scalar"])
def test_lds_poisoned_run_is_finite_and_bitwise_equal(name, monkeypatch):
    """The all-pairs kernels stage (x_m, G_m) tiles in LDS; with every CU's LDS filled with NaN
    patterns in front of each of their launches (tests/test_gpu_lds_poison.py) the partial tiles of
    N = 200 / 65 must not let an unwritten word into a sum.  The hook is read at every launch."""
    lib = NV.load()
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    c0 = lib.pf_test_lds_poison_count()
    clean, _ = run_case(name)
    assert lib.pf_test_lds_poison_count() == c0
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_LDS_POISON", "1")
    got, _ = run_case(name)
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    assert lib.pf_test_lds_poison_count() >= c0 + clean.steps, "the poison hook never fired"
    assert np.all(np.isfinite(got.particles))
    assert np.array_equal(got.particles, clean.particles) and got.n_clipped == clean.n_clipped


def test_unsupported_observation_raises():
    with pytest.raises(NotImplementedError, match="LinearObservation"):
        KP.KernelParticleFilter(KP.Model(M.BearingsObservation(9), None, np.eye(2)))
    with pytest.raises(NotImplementedError):
        KP.KernelParticleFilter(KP.Model(lambda x: x, None, np.eye(2)))
    op = np.zeros(3)
    d = NV.ModelDesc(9, 2, 0, NV.PF_OBS_BEARINGS, None, 0, NV.dptr(op), 3, None, NV.dptr(np.eye(2)))
    hd = NV.C.c_void_p()
    st = NV.load().pf_kpf_create(NV.C.byref(d), NV.C.byref(NV.KpfOpts(10, 0, 0)), NV.C.byref(hd))
    assert st == NV.PF_E_UNSUPPORTED and not hd.value
    with pytest.raises(NotImplementedError):
        NV.check(st)
