"""The gradient of the Sinkhorn OT resampler on the CPU (no device): the two statements of
tests/dpf_ot_grad_restatement.py against each other and against finite differences, the argument
checks of ``sinkhorn_ot_resample_vjp`` made before the library is loaded, and per case the
conditions that make the comparison of tests/test_gpu_dpf_ot_grad.py with the device well defined.

The device bound is 1e-9 max(1, max|ref|), separately for the two gradients.  The closed form and
autograd are two exact forms of one derivative and agree to a few 1e-14 relative here; they are
held to 1e-12.

A gradient through ``maximum`` is a step function of the data: where a plan entry, a column sum or
a cost entry sits at its threshold, or the maximum of a floored column is attained twice, a
rounding error decides which branch the device and the reference differentiate.  So every case must
keep its unfloored plan entries and its column sums 1e-6 relative away from ``min_val``, attain the
maximum of a floored column once with a gap, and have no off-diagonal cost of exactly 0.

max|gX_ref| and max|gw_ref| must exceed 1e-3, so that a backward pass that returns zeros cannot
pass; at N = 1 the weight gradient is of the order of ``min_val`` whatever the data (a = w / (w +
min_val)), and only gX is required there.  The "peaked" weights are left out: their a_i sit at the
floor and the gradient is ill-conditioned there (two exact CPU forms differ by 3.5e-10 relative).
"""

import subprocess
import sys

import numpy as np
import pytest
import torch

from particle_filters_amd import dpf_ot as OT
from particle_filters_amd import dpf_ot_torch as TT
from tests import dpf_ot_grad_restatement as GR
from tests import dpf_ot_restatement as R
from tests.conftest import REPO

TOL = 1e-9  # the device bound


@pytest.mark.parametrize("name", GR.CASE_NAMES)
def test_closed_form_against_autograd_and_the_conditions_of_the_device_comparison(name):
    ref = GR.autograd(GR.case(name))
    N = ref["X"].shape[0]
    info = {}
    gX, gw = GR.closed_form(ref["X"], ref["w"], ref["G"], ref["eps"], ref["K"], info=info)
    sx, sw = max(1.0, float(np.max(np.abs(ref["gX"])))), max(1.0, float(np.max(np.abs(ref["gw"]))))
    ex, ew = float(np.max(np.abs(gX - ref["gX"]))), float(np.max(np.abs(gw - ref["gw"])))
    ox = float(np.max(np.abs(ref["gX_rev"] - ref["gX"])))
    ow = float(np.max(np.abs(ref["gw_rev"] - ref["gw"])))
    print(f"ot grad {name}: K {ref['K']}, max|gX| {sx:.3g}, max|gw| {sw:.3g}, closed form - autograd {ex:.2e} / {ew:.2e}, "
          f"order sensitivity {ox:.2e} / {ow:.2e}, {info}")
    assert ex <= 1e-12 * sx and ew <= 1e-12 * sw
    assert ox <= 1e-3 * TOL * sx and ow <= 1e-3 * TOL * sw
    assert info["plan_margin"] > 1e-6
    assert info["sum_margin"] > 1e-6
    assert info["argmax_gap"] > 1e-6
    assert info["zero_offdiag"] == 0
    assert float(np.max(np.abs(ref["gX"]))) > 1e-3
    if N >= 2:
        assert float(np.max(np.abs(ref["gw"]))) > 1e-3
    if name in ("sharp", "floor eps=0.05"):
        assert info["floored_columns"] > 0  # the argmax path is taken
    if name == "zeros":
        assert np.all(ref["gw"][::3] == 0.0) and np.all(gw[::3] == 0.0)
    if name == "early":
        assert ref["K"] == R.EARLY[0][6] < ref["n_iters"]


def test_central_finite_differences_with_the_iterations_fixed():
    N, d, eps, K = 9, 2, 0.5, 7
    X, w = R.make_case(N, d, seed=3)
    G = GR.grad_out(N, d)
    gX, gw = GR.closed_form(X, w, G, eps, K)

    def loss(Xp, wp):  # tol = -1: no early stop, exactly K iterations
        return float(np.sum(G * R.sinkhorn_resample(Xp, wp, eps, K, tol=-1.0)["particles"]))

    h = 1e-6
    for i, c in ((0, 0), (4, 1), (8, 0)):
        E = np.zeros_like(X)
        E[i, c] = h
        fd = (loss(X + E, w) - loss(X - E, w)) / (2.0 * h)
        assert abs(fd - gX[i, c]) <= 1e-6 * max(1.0, abs(gX[i, c])), (i, c, fd, gX[i, c])
    for i in (1, 5):
        e = np.zeros_like(w)
        e[i] = h * w[i]
        fd = (loss(X, w + e) - loss(X, w - e)) / (2.0 * h * w[i])
        assert abs(fd - gw[i]) <= 1e-6 * max(1.0, abs(gw[i])), (i, fd, gw[i])


def test_saved_of_the_wrong_shape_raises_before_the_library_is_loaded(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(OT.NV, "load", no_library)
    N, d, K = 5, 2, 3
    X, w = R.make_case(N, d, seed=1)
    G = GR.grad_out(N, d)
    its = np.array([K], dtype=np.int32)
    hist, am = np.zeros((1, 4, K + 1, N)), np.full((1, K, N), -1, dtype=np.int32)
    bad = [(its, hist, am)[:2],  # not an OtSaved
           OT.OtSaved(its, hist[:, :, :K], am),
           OT.OtSaved(its, hist[..., :4], am),
           OT.OtSaved(its, hist, am[:, :2]),
           OT.OtSaved(np.array([K, K], dtype=np.int32), hist, am),
           OT.OtSaved(np.array([51], dtype=np.int32), np.zeros((1, 4, 52, N)), np.full((1, 51, N), -1, dtype=np.int32)),
           OT.OtSaved(np.array([-1], dtype=np.int32), hist, am),
           OT.OtSaved(its, np.where(hist == 0.0, np.nan, hist), am),
           OT.OtSaved(its, hist, am + N + 1)]
    for saved in bad:
        with pytest.raises(ValueError):
            OT.sinkhorn_ot_resample_vjp(X, w, G, saved=saved)
    with pytest.raises(ValueError):
        OT.sinkhorn_ot_resample_vjp(X, w, G[:4])
    with pytest.raises(ValueError):
        OT.sinkhorn_ot_resample_vjp(X, w, np.where(G > 0, np.inf, G))
    with pytest.raises(ValueError):
        OT.sinkhorn_ot_resample_vjp(X, w, G, epsilon=0.0)
    # a batch's saved does not fit one problem
    with pytest.raises(ValueError):
        OT.sinkhorn_ot_resample_vjp(X, w, G, saved=OT.OtSaved(np.array([K, K], dtype=np.int32),
                                                                  np.zeros((2, 4, K + 1, N)),
                                                                  np.full((2, K, N), -1, dtype=np.int32)))


def test_the_torch_wrapper_rejects_its_arguments_before_the_library_is_loaded(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(OT.NV, "load", no_library)
    X, w = R.make_case(5, 2, seed=1)
    x, wt = torch.tensor(X), torch.tensor(w)
    with pytest.raises(TypeError):
        TT.sinkhorn_ot_resample(x.float(), wt)
    with pytest.raises(TypeError):
        TT.sinkhorn_ot_resample(x, wt.float())
    with pytest.raises(TypeError):
        TT.sinkhorn_ot_resample(X, wt)
    with pytest.raises(TypeError):
        TT.sinkhorn_ot_resample(x, wt, torch.tensor(0.1, dtype=torch.float64))
    with pytest.raises(ValueError):
        TT.sinkhorn_ot_resample(x, wt[:4])
    with pytest.raises(ValueError):
        TT.sinkhorn_ot_resample(x, wt, epsilon=-1.0)
    with pytest.raises(ValueError):
        TT.DPF_OT(0, 2, None, None)


def test_dpf_ot_imports_without_torch():
    code = ("import sys; import particle_filters_amd; from particle_filters_amd import dpf_ot; "
            "assert 'torch' not in sys.modules, 'torch was imported'; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
