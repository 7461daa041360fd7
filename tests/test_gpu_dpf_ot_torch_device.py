"""The device path of the torch binding of the Sinkhorn OT resampler (-m gpu, MI355X): CUDA tensors
in, CUDA tensors out, the dual history recorded by the forward pass into device tensors, nothing
through host memory.

The reference is the default path of the same build on the same tensors, the host path, which
tests/test_gpu_dpf_ot_grad.py pins to the autograd restatement.  Here the comparison is bitwise: the
two paths run the same kernels on the same values, the history the forward pass records is bitwise
the replay's (tests/test_gpu_dpf_ot_dev_entries.py), and there is no torch arithmetic around the
kernels on either path.

The whole filter.  tests/dpf_ot_grad_restatement.FILTER (N = 65, d = 2, T = 3) on the device path
against the same filter written entirely in torch on the CPU, under the bound of
tests/test_gpu_dpf_ot_grad.py::test_whole_filter_gradients_against_the_cpu_filter: the loss within
1e-9 max(1, |loss|), each gradient within max(1e3 sens, 1e-9 size), sens the CPU filter's own
sensitivity to the summation order; the per-step iteration counts equal.
"""

import math

import numpy as np
import pytest
import torch

from particle_filters_amd import _dpf_common as DC
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
    assert torch.cuda.is_available()


def bits(got, ref):
    assert len(got) == len(ref)
    return all(torch.equal(g.detach().cpu(), r.detach().cpu()) for g, r in zip(got, ref))


def paths():
    return dict(DC.PATH_CALLS)


def ran(before, path, n=1):
    """``n`` calls on ``path`` since ``before``, none on the other."""
    now = paths()
    other = "host" if path == "device" else "device"
    return now[path] == before[path] + n and now[other] == before[other]


class NoHost:
    """``Tensor.cpu``, ``Tensor.item``, ``Tensor.tolist`` and ``Tensor.numpy`` raise: what runs inside
    copies nothing to the host through them."""

    def __init__(self, monkeypatch):
        self.mp = monkeypatch

    def __enter__(self):
        self.ctx = self.mp.context()
        m = self.ctx.__enter__()
        for name in ("cpu", "item", "tolist", "numpy"):
            def refuse(self, *a, _name=name, **k):
                raise AssertionError(f"Tensor.{_name}() on the device path")

            m.setattr(torch.Tensor, name, refuse)

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)


def strided(t):
    """The same values, non-contiguous: the last two axes stored transposed."""
    v = t.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


def every_other(t):
    """The same values as every other element of a buffer twice as long in the last axis."""
    buf = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    v = buf[..., ::2]
    v.copy_(t)
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


# three problems that stop at different iterations (R.BATCH, N = 130: five source splits)
def inputs(unbatched=False):
    c = R.BATCH
    cases = [R.make_case(c["N"], c["d"], c["scale"], c["conc"], s) for s, _ in c["seeds"]]
    X, w = np.stack([x for x, _ in cases]), np.stack([w for _, w in cases])
    g = np.random.default_rng([c["N"], c["d"], 5]).standard_normal(X.shape)
    return (X[1], w[1], g[1]) if unbatched else (X, w, g)


def run(X, w, g, dev_x="cuda", dev_w=None, wrap=None, **kw):
    """(new particles, new weights, grad particles, grad weights) of one sinkhorn_ot_resample and its
    backward pass, on tensors made from the arrays."""
    x = torch.tensor(X, device=dev_x)
    wt = torch.tensor(w, device=dev_w or dev_x)
    if wrap is not None:
        x, wt = wrap[0](x), wrap[1](wt)
    x.requires_grad_(True)
    wt.requires_grad_(True)
    out, nw = TT.sinkhorn_ot_resample(x, wt, R.BATCH["eps"], R.EARLY_ITERS, **kw)
    (out * torch.tensor(g, device=out.device)).sum().backward()
    return [out, nw, x.grad, wt.grad]


_ref = {}


def default_path(unbatched=False):
    """The default path on the same CUDA tensors: through host memory."""
    if unbatched not in _ref:
        before = paths()
        _ref[unbatched] = run(*inputs(unbatched))
        assert ran(before, "host")
    return _ref[unbatched]


@pytest.mark.parametrize("unbatched", [False, True], ids=["batched", "unbatched"])
def test_the_device_path_gives_the_default_paths_bits(unbatched):
    ref = default_path(unbatched)
    before = paths()
    got = run(*inputs(unbatched), device_path=True)
    assert ran(before, "device")
    assert all(t.is_cuda and t.device.index == 0 for t in got)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert float(ref[2].abs().max()) > 1e-3 and float(ref[3].abs().max()) > 1e-3  # gradients that are there
    assert bits(got, ref)
    assert bits(run(*inputs(unbatched), device_path=True, solver="launches"), ref)


def test_only_one_input_requiring_grad_and_none():
    X, w, g = inputs()
    ref = default_path()
    x, wt = torch.tensor(X, device="cuda", requires_grad=True), torch.tensor(w, device="cuda")
    out, _ = TT.sinkhorn_ot_resample(x, wt, R.BATCH["eps"], R.EARLY_ITERS, device_path=True)
    (out * torch.tensor(g, device="cuda")).sum().backward()
    assert bits([out, x.grad], [ref[0], ref[2]]) and wt.grad is None
    out, _ = TT.sinkhorn_ot_resample(x.detach(), wt, R.BATCH["eps"], R.EARLY_ITERS, device_path=True)
    assert not out.requires_grad and bits([out], [ref[0]])  # no history was recorded: nothing needs it


def test_without_value_checks_nothing_is_read_back(monkeypatch):
    X, w, g = inputs()
    ref = default_path()
    before = paths()
    with NoHost(monkeypatch):
        got = run(X, w, g, device_path=True, check_values=False)
    assert ran(before, "device")
    assert bits(got, ref)  # the sweep over all n_iters iterations gives the bits of the sweep over max K_b


@pytest.mark.parametrize("wrap", [(strided, strided), (every_other, every_other)], ids=["strided", "every_other"])
def test_layouts_give_the_contiguous_bits(wrap):
    X, w, g = inputs()
    ref = default_path()
    before = paths()
    assert bits(run(X, w, g, wrap=wrap, device_path=True), ref)
    assert ran(before, "device")


def test_cpu_and_mixed_tensors_take_the_host_path():
    X, w, g = inputs()
    eps, n = R.BATCH["eps"], R.EARLY_ITERS
    today, _, saved = OT.sinkhorn_ot_resample(X, w, eps, n, return_saved=True)
    gX, gw = OT.sinkhorn_ot_resample_vjp(X, w, g, eps, n, saved=saved)
    for dev_x, dev_w in (("cpu", "cpu"), ("cuda", "cpu"), ("cpu", "cuda")):
        before = paths()
        got = run(X, w, g, dev_x=dev_x, dev_w=dev_w, device_path=True)
        assert ran(before, "host")
        assert got[0].device.type == dev_x and got[3].device.type == dev_w
        for t, a in zip([got[0], got[2], got[3]], [today, gX, gw]):
            assert np.array_equal(t.detach().cpu().numpy(), a)


def test_value_checks_on_the_device_path():
    X, w, g = inputs()
    x, wt = torch.tensor(X, device="cuda"), torch.tensor(w, device="cuda")

    def call(x, wt, *a, **kw):
        before = paths()
        try:
            return TT.sinkhorn_ot_resample(x, wt, *a, device_path=True, **kw)
        finally:
            assert paths()["host"] == before["host"]  # nothing fell back to the host path

    bad = wt.clone()
    bad[0, 3] = math.nan
    with pytest.raises(ValueError, match="weights must be finite"):
        call(x, bad)
    bad = wt.clone()
    bad[2, 0] = math.inf
    with pytest.raises(ValueError, match="weights must be finite"):
        call(x, bad)
    bad = x.clone()
    bad[1, 2, 0] = math.nan
    with pytest.raises(ValueError, match="particles must be finite"):
        call(bad, wt)
    with pytest.raises(ValueError, match="particles must be \\(N, d\\) or \\(B, N, d\\)"):
        call(x[0, 0], wt[0, 0])
    with pytest.raises(ValueError, match="disagree on N"):
        call(x, wt[:, :-1])
    with pytest.raises(ValueError, match="epsilon must be positive"):
        call(x, wt, 0.0)
    with pytest.raises(ValueError, match="n_iters must be a non-negative integer"):
        call(x, wt, 0.1, -1)
    with pytest.raises(ValueError, match="solver must be one of"):
        call(x, wt, solver="auto")
    with pytest.raises(TypeError, match="float64"):
        call(x.float(), wt)
    xg = x.clone().requires_grad_(True)
    out, _ = call(xg, wt, 0.1, 5)
    with pytest.raises(ValueError, match="grad_new_particles must be finite"):
        out.backward(torch.full_like(out, math.inf))
    # no iteration: the plan at f = g = 0, and its backward pass
    xg = x.clone().requires_grad_(True)
    out, _ = call(xg, wt, 0.1, 0)
    out.sum().backward()
    x0 = x.clone().requires_grad_(True)
    ref, _ = TT.sinkhorn_ot_resample(x0, wt, 0.1, 0)
    ref.sum().backward()
    assert bits([out, xg.grad], [ref, x0.grad])
    # double backward is not implemented
    xg = x.clone().requires_grad_(True)
    out, _ = call(xg, wt, 0.1, 5)
    (gx,) = torch.autograd.grad(out.sum(), xg, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_the_resident_solver_through_the_binding():
    """N = 100 (two problems of R.BATCH's kind would not fit: N = 130), d = 2: the one-launch forward and
    the reverse sweep on its history, against the launch sequence on the same tensors under the unit's
    1e-9 of the scales; iteration counts equal, two calls bitwise equal."""
    X = np.stack([R.make_case(100, 2, 0.2, 1.0, s)[0] for s in (4, 7, 10)])
    w = np.stack([R.make_case(100, 2, 0.2, 1.0, s)[1] for s in (4, 7, 10)])
    g = np.random.default_rng([100, 2, 5]).standard_normal(X.shape)

    def go(**kw):
        x, wt = torch.tensor(X, device="cuda", requires_grad=True), torch.tensor(w, device="cuda", requires_grad=True)
        h = OT._Handle(100, 2, 3)
        try:
            out, _ = TT.sinkhorn_ot_resample(x, wt, 0.1, R.EARLY_ITERS, device_path=True, _handle=h, **kw)
            (out * torch.tensor(g, device="cuda")).sum().backward()
            return [out, x.grad, wt.grad], h.last_iterations.cpu().tolist()
        finally:
            h.close()

    ref, its_ref = go()
    before = paths()
    got, its = go(solver="resident")
    assert ran(before, "device")
    assert its == its_ref == [32, 36, 33]
    for name, a, r in zip(("particles", "grad particles", "grad weights"), got, ref):
        scale = max(1.0, float(r.abs().max()))
        err = float((a - r).abs().max())
        print(f"ot resident through torch, {name}: error {err:.3e} (scale {scale:.3g})")
        assert bool(torch.isfinite(a).all()) and err <= TOL * scale
    assert bits(go(solver="resident", check_values=False)[0], got)
    x129 = torch.zeros(129, 2, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match=r'solver="resident" needs N <= 128'):
        TT.sinkhorn_ot_resample(x129, torch.ones(129, dtype=torch.float64, device="cuda"), device_path=True,
                                solver="resident")


@pytest.mark.parametrize("solver, check_values", [("launches", True), ("launches", False), ("resident", True)],
                         ids=["launches-checked", "launches-unchecked", "resident-checked"])
def test_whole_filter_on_the_device_path(solver, check_values):
    c = GR.FILTER
    data = GR.filter_data()
    N, d, T = c["N"], c["d"], c["T"]
    cuda = dict(dtype=torch.float64, device="cuda")
    a = torch.tensor(c["a"], requires_grad=True, **cuda)
    sigma = torch.tensor(c["sigma"], requires_grad=True, **cuda)
    mean = torch.zeros(d, requires_grad=True, **cuda)
    tf_, lf_ = GR.model(a, sigma, torch.tensor(data["eps"], device="cuda"), c["sigma_r"])
    obs = torch.tensor(data["obs"], device="cuda")
    flt = TT.DPF_OT(N, d, tf_, lf_, c["eps"], c["iters"], rng=np.random.default_rng(c["rng"]), device_path=True,
                    check_values=check_values, solver=solver)
    before = paths()
    try:
        particles, weights = flt.init_particles(mean, torch.eye(d, **cuda))
        ps, ws, its = [], [], []
        for t in range(T):
            particles, weights = flt.step(particles, weights, obs[t], t=t)
            ps.append(particles)
            ws.append(weights)
            its.append(flt.last_iterations)
        loss = GR.loss_of(ps, ws, torch.tensor(data["targets"], device="cuda"))
        loss.backward()
        assert ran(before, "device", T)
        _, _, diag = flt.step(ps[-1].detach(), ws[-1], obs[0], t=0, return_diagnostics=True)
        assert diag["sinkhorn_iterations"] >= 1 and np.isfinite(diag["ot_distance"])
    finally:
        flt.close()
    ref = GR.cpu_filter_grads(reverse=False)
    rev = GR.cpu_filter_grads(reverse=True)
    assert [int(k.cpu()[0]) for k in its] == ref[4]
    assert all(p.is_cuda for p in ps) and a.grad.is_cuda and mean.grad.is_cuda
    assert abs(float(loss.detach()) - ref[0]) <= TOL * max(1.0, abs(ref[0]))
    got = (float(a.grad), float(sigma.grad), mean.grad.cpu().numpy())
    for name, g, r, v in zip(("d loss/da", "d loss/dsigma", "d loss/dmean0"), got, ref[1:4], rev[1:4]):
        size = float(np.max(np.abs(r)))
        sens = float(np.max(np.abs(np.asarray(r) - np.asarray(v))))
        bound = max(1e3 * sens, 1e-9 * size)
        err = float(np.max(np.abs(np.asarray(g) - np.asarray(r))))
        print(f"ot device filter {name}: reference {np.asarray(r)}, error {err:.3e}, CPU order sensitivity {sens:.3e}, "
              f"bound {bound:.3e}")
        assert size > 1e-3  # a gradient that is there
        assert err <= bound
