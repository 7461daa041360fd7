"""Backward pass of the Sinkhorn OT resampler on the device, and its PyTorch binding (-m gpu, MI355X).

The reference is PyTorch's CPU fp64 autograd of the literal forward with the iterations fixed at
those the restatement takes (tests/dpf_ot_grad_restatement.py, checked against the closed form and
finite differences by tests/test_dpf_ot_grad_host.py, which also asserts per case what makes this
comparison well defined).  Nothing here takes finite differences on the device.

Bounds.  gX within 1e-9 max(1, max|gX_ref|) and gw within 1e-9 max(1, max|gw_ref|): the bound of
the forward tests and of the soft resampler's backward pass.  The device sums in another order
(waves, splits of the source range, tiles), multiplies by 1 / eps where the reference divides, and
uses the device library's exp and log.

The cases are the shapes at which each loop can go wrong: N = 1, 2; N = 65 just past one 64-lane
tile; N = 130 five source splits; 100 iterations; d = 40 three component chunks; d = 65 / 64 the LDS
stage boundaries; zero and one iteration; an early stop (29 of 500); unnormalised weights and
weights with zeros, whose entries must get exactly 0; the two edges whose floored columns take
the argmax path; N = 2500 chunks of more than 32 sources.

The whole filter.  N = 65, d = 2, T = 3 steps, transition a x + sigma eps with a and sigma tensors
that require grad, a Gaussian likelihood, loss = sum_t |weighted mean_t - target_t|^2.  d loss / da,
d loss / dsigma and d loss / dmean0 through the device-backed filter against the same filter
written entirely in torch on the CPU.  The bound is 1e3 times the CPU filter's own sensitivity to
the summation order, floored at 1e-9 relative to the gradient.

Largest errors measured on an MI355X: DESIGN.md section 4, "Sinkhorn OT resampling: the backward pass".
"""

import numpy as np
import pytest
import torch

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_ot as OT
from particle_filters_amd import dpf_ot_torch as TT
from tests import dpf_ot_grad_restatement as GR
from tests import dpf_ot_restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert NV.device_count() > 0, "no HIP device visible: -m gpu tests must run on an MI355X"


def compare(tag, gX, gw, ref):
    assert np.all(np.isfinite(gX)) and np.all(np.isfinite(gw))
    sx, sw = max(1.0, float(np.max(np.abs(ref["gX"])))), max(1.0, float(np.max(np.abs(ref["gw"]))))
    ex, ew = float(np.max(np.abs(gX - ref["gX"]))), float(np.max(np.abs(gw - ref["gw"])))
    print(f"ot grad {tag}: gX error {ex:.3e} (scale {sx:.3g}, {ex / sx:.2e} rel), gw error {ew:.3e} (scale {sw:.3g}, "
          f"{ew / sw:.2e} rel)")
    assert ex <= TOL * sx
    assert ew <= TOL * sw


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------ a. parity
@pytest.mark.parametrize("name", GR.CASE_NAMES)
def test_parity(name):
    ref = GR.autograd(GR.case(name))
    X, w, G, eps, n_iters = ref["X"], ref["w"], ref["G"], ref["eps"], ref["n_iters"]
    N, d = X.shape
    assert float(np.max(np.abs(ref["gX"]))) > 1e-3
    if N >= 2:
        assert float(np.max(np.abs(ref["gw"]))) > 1e-3
    gX, gw = OT.sinkhorn_ot_resample_vjp(X, w, G, eps, n_iters)
    assert gX.dtype == np.float64 and gX.shape == (N, d) and gw.shape == (N,)
    compare(name, gX, gw, ref)
    if name == "zeros":
        assert np.all(gw[::3] == 0.0) and np.all(gw[1::3] != 0.0)
    # the saved results of the forward call give the same bits as finding the iterations again
    out, nw, saved = OT.sinkhorn_ot_resample(X, w, eps, n_iters, return_saved=True)
    assert isinstance(saved, OT.OtSaved) and int(saved.iterations[0]) == ref["K"]
    assert saved.hist.shape == (1, 4, ref["K"] + 1, N) and saved.hist_argmax.shape == (1, ref["K"], N)
    assert same(OT.sinkhorn_ot_resample(X, w, eps, n_iters), (out, nw))
    assert same(OT.sinkhorn_ot_resample_vjp(X, w, G, eps, n_iters, saved=saved), (gX, gw))
    if name in ("sharp", "floor eps=0.05"):
        assert np.any(saved.hist_argmax >= 0)  # the argmax path was taken
    elif ref["K"]:
        assert np.all(saved.hist_argmax == -1)


# ------------------------------------------------------------------ b. forced splits
@pytest.mark.parametrize("splits", ["1", "2", "3"])
def test_forced_splits(splits, monkeypatch):
    ref = GR.autograd(GR.case(GR.SMALL_SPLITS))
    args = (ref["X"], ref["w"], ref["G"], ref["eps"], ref["n_iters"])
    monkeypatch.delenv("PF_TEST_OT_SPLITS", raising=False)
    plain = OT.sinkhorn_ot_resample_vjp(*args)
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_OT_SPLITS", splits)
    got = OT.sinkhorn_ot_resample_vjp(*args)
    again = OT.sinkhorn_ot_resample_vjp(*args)
    compare(f"N=300 d=40 PF_TEST_OT_SPLITS={splits}", *got, ref)
    assert same(again, got)
    assert not np.array_equal(got[0], plain[0])  # the hook took effect: another summation order


# ------------------------------------------------------------------ c. bitwise properties
def _batch():
    """R.BATCH's three problems, which stop at different iterations: X, w, G, eps, n_iters."""
    c = R.BATCH
    cases = [R.make_case(c["N"], c["d"], c["scale"], c["conc"], s) for s, _ in c["seeds"]]
    G = np.stack([np.random.default_rng([c["N"], c["d"], 99, b]).standard_normal((c["N"], c["d"])) for b in range(3)])
    return np.stack([x for x, _ in cases]), np.stack([w for _, w in cases]), G, c["eps"], R.EARLY_ITERS


def _chunk_batch():
    c = R.CHUNK_BATCH
    cases = [R.solved_chunk_batch(b)[:2] for b in range(3)]
    G = np.stack([np.random.default_rng([c["N"], c["d"], 99, b]).standard_normal((c["N"], c["d"])) for b in range(3)])
    return np.stack([x for x, _ in cases]), np.stack([w for _, w in cases]), G, c["eps"], c["n_iters"]


def test_equal_calls_are_bitwise_equal():
    X, w, G, eps, n = _batch()
    a = OT.sinkhorn_ot_resample_vjp(X, w, G, eps, n)
    b = OT.sinkhorn_ot_resample_vjp(X, w, G, eps, n)
    assert same(a, b)
    assert not np.array_equal(a[0], OT.sinkhorn_ot_resample_vjp(X, w, 2.0 * G, eps, n)[0])


@pytest.mark.parametrize("which", ["early stops", "component chunks"])
def test_a_batch_is_bitwise_the_problems_alone(which):
    X, w, G, eps, n = _batch() if which == "early stops" else _chunk_batch()
    out, _, saved = OT.sinkhorn_ot_resample(X, w, eps, n, return_saved=True)
    if which == "early stops":
        assert [int(k) for k in saved.iterations] == [k for _, k in R.BATCH["seeds"]]
    gX, gw = OT.sinkhorn_ot_resample_vjp(X, w, G, eps, n)
    assert gX.shape == X.shape and gw.shape == w.shape
    assert same(OT.sinkhorn_ot_resample_vjp(X, w, G, eps, n, saved=saved), (gX, gw))
    for b in range(3):
        g1, w1 = OT.sinkhorn_ot_resample_vjp(X[b], w[b], G[b], eps, n)
        assert np.array_equal(g1, gX[b]) and np.array_equal(w1, gw[b]), f"problem {b}"
        cf = GR.closed_form(X[b], w[b], G[b], eps, int(saved.iterations[b]))
        compare(f"{which}, problem {b}", gX[b], gw[b], {"gX": cf[0], "gw": cf[1]})
    if which == "component chunks":
        assert np.all(gw[R.CHUNK_BATCH["zeros"], ::3] == 0.0)


def _steps():
    X, w, G, eps, _ = _batch()
    return [(X[0], w[0], G[0], eps, R.EARLY_ITERS), (X[1], w[1], G[1], 0.1, 50), (X[2], w[2], G[2], 0.5, 1)]


def test_a_reused_handle_gives_the_bits_of_fresh_ones_and_its_forward_is_unchanged():
    steps = _steps() + _steps()[:1] + [(_steps()[1][0], _steps()[0][1], _steps()[2][2], 0.1, 0)]
    N, d = steps[0][0].shape
    fresh_fwd = OT.sinkhorn_ot_resample(*steps[0][:2], steps[0][3], steps[0][4], return_diagnostics=True)
    h = OT._Handle(N, d, 1)
    try:
        got = [OT.sinkhorn_ot_resample_vjp(*s, _handle=h) for s in steps]
        fwd = OT.sinkhorn_ot_resample(*steps[0][:2], steps[0][3], steps[0][4], return_diagnostics=True, _handle=h)
    finally:
        h.close()
    for k, s in enumerate(steps):
        assert same(got[k], OT.sinkhorn_ot_resample_vjp(*s)), f"call {k}"
    assert same(got[0], got[3])
    # forward outputs of a handle that has run backward passes are those of a fresh handle
    assert same(fwd, fresh_fwd)
    assert fwd[2] == fresh_fwd[2]


def test_backwards_in_reverse_order_on_one_handle_are_the_fresh_ones():
    """Three forwards on one handle, then the three backwards in reverse order with each forward's
    saved history: what the handle holds is that of the last call, and a backward that read it
    instead of its own history would be wrong for the first two."""
    steps = _steps()
    N, d = steps[0][0].shape
    h = OT._Handle(N, d, 1)
    try:
        saved = [OT.sinkhorn_ot_resample(x, w, eps, n, return_saved=True, _handle=h)[2] for x, w, _, eps, n in steps]
        assert len({int(s.iterations[0]) for s in saved}) == 3
        got = {t: OT.sinkhorn_ot_resample_vjp(*steps[t], saved=saved[t], _handle=h) for t in (2, 1, 0)}
    finally:
        h.close()
    for t in range(3):
        assert same(got[t], OT.sinkhorn_ot_resample_vjp(*steps[t])), f"step {t}"


def test_the_entry_rejects_bad_arguments():
    lib = NV.load()
    i32 = NV.C.POINTER(NV.C.c_int32)
    h = OT._Handle(4, 2, 2)
    try:
        X, w, g = np.ones((2, 4, 2)), np.full((2, 4), 0.25), np.ones((2, 4, 2))
        gX, gw = np.zeros((2, 4, 2)), np.zeros((2, 4))
        its = np.array([2, 1], dtype=np.int32)
        hist, am = np.zeros((2, 4, 3, 4)), np.zeros((2, 2, 4), dtype=np.int32)
        a = (h.h, NV.dptr(X), NV.dptr(w))
        k, o = its.ctypes.data_as(i32), (NV.dptr(g), NV.dptr(gX), NV.dptr(gw))
        assert lib.pf_ot_backward(*a, 0.1, 1e-12, k, 2, None, None, *o) == NV.PF_OK
        assert np.all(np.isfinite(gX)) and np.all(np.isfinite(gw))
        assert lib.pf_ot_replay(*a, 0.1, 1e-12, k, 2, NV.dptr(hist), am.ctypes.data_as(i32)) == NV.PF_OK
        assert np.all(hist[:, :2, 0] == 0.0) and np.all(hist[1, :, 2] == 0.0) and np.all(am[1, 1] == -1)
        assert lib.pf_ot_backward(*a, 0.1, 1e-12, k, 2, NV.dptr(hist), am.ctypes.data_as(i32), *o) == NV.PF_OK
        assert lib.pf_ot_backward(*a, 0.1, 1e-12, k, 2, NV.dptr(hist), None, *o) == NV.PF_E_ARG
        assert lib.pf_ot_backward(*a, 0.1, 1e-12, k, 2, None, am.ctypes.data_as(i32), *o) == NV.PF_E_ARG
        assert lib.pf_ot_backward(*a, 0.1, 1e-12, k, 1, None, None, *o) == NV.PF_E_ARG  # iterations above k_cap
        assert lib.pf_ot_backward(*a, 0.1, 1e-12, k, -1, None, None, *o) == NV.PF_E_ARG
        assert lib.pf_ot_backward(*a, 0.1, 1e-12, None, 2, None, None, *o) == NV.PF_E_ARG
        for eps in (0.0, -1.0, float("inf"), float("nan")):
            assert lib.pf_ot_backward(*a, eps, 1e-12, k, 2, None, None, *o) == NV.PF_E_ARG
        assert lib.pf_ot_backward(*a, 0.1, 1e-12, k, 2, None, None, None, o[1], o[2]) == NV.PF_E_ARG
        assert lib.pf_ot_backward(*a, 0.1, 1e-12, k, 2, None, None, o[0], None, o[2]) == NV.PF_E_ARG
        assert lib.pf_ot_backward(*a, 0.1, 1e-12, k, 2, None, None, o[0], o[1], None) == NV.PF_E_ARG
        assert lib.pf_ot_backward(None, a[1], a[2], 0.1, 1e-12, k, 2, None, None, *o) == NV.PF_E_ARG
        assert lib.pf_ot_replay(*a, 0.1, 1e-12, k, 2, None, am.ctypes.data_as(i32)) == NV.PF_E_ARG
    finally:
        h.close()


# ------------------------------------------------------------------ d. the torch binding
def test_torch_gradients_are_the_vjps_bits():
    ref = GR.autograd(GR.case("N130-d3-eps0.1-it50"))
    X, w, G, eps, n = ref["X"], ref["w"], ref["G"], ref["eps"], ref["n_iters"]
    x = torch.tensor(X, requires_grad=True)
    wt = torch.tensor(w, requires_grad=True)
    out, nw = TT.sinkhorn_ot_resample(x, wt, eps, n)
    assert out.dtype == torch.float64 and out.shape == X.shape and out.requires_grad and not nw.requires_grad
    assert np.array_equal(nw.numpy(), np.full(X.shape[0], 1.0 / X.shape[0]))
    assert np.array_equal(out.detach().numpy(), OT.sinkhorn_ot_resample(X, w, eps, n)[0])
    (out * torch.tensor(G)).sum().backward()
    gX, gw = OT.sinkhorn_ot_resample_vjp(X, w, G, eps, n)
    assert np.array_equal(x.grad.numpy(), gX) and np.array_equal(wt.grad.numpy(), gw)
    # a batch, and only one input requiring grad
    Xb, wb, _, epsb, nb = _batch()
    xb = torch.tensor(Xb, requires_grad=True)
    outb, _ = TT.sinkhorn_ot_resample(xb, torch.tensor(wb), epsb, nb)
    outb.sum().backward()
    assert np.array_equal(xb.grad.numpy(), OT.sinkhorn_ot_resample_vjp(Xb, wb, np.ones_like(Xb), epsb, nb)[0])
    with pytest.raises(TypeError):
        TT.sinkhorn_ot_resample(x.float(), wt)
    with pytest.raises(TypeError):
        TT.sinkhorn_ot_resample(x, wt, torch.tensor(0.1))


def test_torch_double_backward_raises():
    X, w = R.make_case(5, 2, seed=1)
    x = torch.tensor(X, requires_grad=True)
    out, _ = TT.sinkhorn_ot_resample(x, torch.tensor(w))
    (gx,) = torch.autograd.grad(out.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_whole_filter_gradients_against_the_cpu_filter():
    c = GR.FILTER
    data = GR.filter_data()
    N, d, T = c["N"], c["d"], c["T"]
    a = torch.tensor(c["a"], dtype=torch.float64, requires_grad=True)
    sigma = torch.tensor(c["sigma"], dtype=torch.float64, requires_grad=True)
    mean = torch.zeros(d, dtype=torch.float64, requires_grad=True)
    tf_, lf_ = GR.model(a, sigma, torch.from_numpy(data["eps"]), c["sigma_r"])
    flt = TT.DPF_OT(N, d, tf_, lf_, c["eps"], c["iters"], rng=np.random.default_rng(c["rng"]))
    try:
        ps, ws = flt.run_filter(torch.from_numpy(data["obs"]), mean, torch.eye(d, dtype=torch.float64))
        assert len(ps) == T and ps[0].shape == (N, d) and ws[0].shape == (N,)
        loss = GR.loss_of(ps, ws, torch.from_numpy(data["targets"]))
        loss.backward()
        _, _, diag = flt.step(ps[-1].detach(), ws[-1], torch.from_numpy(data["obs"][0]), t=0, return_diagnostics=True)
        assert diag["sinkhorn_iterations"] >= 1 and np.isfinite(diag["ot_distance"])
    finally:
        flt.close()
    ref = GR.cpu_filter_grads(reverse=False)
    rev = GR.cpu_filter_grads(reverse=True)
    assert abs(float(loss.detach()) - ref[0]) <= TOL * max(1.0, abs(ref[0]))
    got = (float(a.grad), float(sigma.grad), mean.grad.numpy())
    for name, g, r, v in zip(("d loss/da", "d loss/dsigma", "d loss/dmean0"), got, ref[1:4], rev[1:4]):
        size = float(np.max(np.abs(r)))
        sens = float(np.max(np.abs(np.asarray(r) - np.asarray(v))))
        bound = max(1e3 * sens, 1e-9 * size)
        err = float(np.max(np.abs(np.asarray(g) - np.asarray(r))))
        print(f"ot filter {name}: reference {np.asarray(r)}, error {err:.3e}, CPU order sensitivity {sens:.3e}, "
              f"bound {bound:.3e}")
        assert size > 1e-3  # a gradient that is there
        assert err <= bound
