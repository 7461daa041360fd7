"""The device path of the torch bindings of the soft and the RNN resampler (-m gpu, MI355X): CUDA
tensors in, CUDA tensors out, nothing through host memory.  The RNN binding takes it by the tensors'
placement; the soft binding when asked (``device_path=True``), because its default for tensors on the
device, the bits of CPU tensors, is pinned by tests/test_gpu_dpf_soft_grad.py.

The reference is the CPU-tensor path of the same build, the host path, which the existing tests pin
to the restatements (tests/test_gpu_dpf_soft_grad.py, tests/test_gpu_dpf_rnn_grad.py).  The bound is
theirs, TOL = 1e-9 max(1, max|ref|).  Bitwise equality is not expected between the paths: the O(B N)
chains around the kernels (exp of the log-weights, the mixture with the uniform, their chain rules)
are torch's on the device and NumPy's on the host.  Within one path it is: a non-contiguous input or
a view at a storage offset gives the contiguous input's bits, and CPU or mixed tensors give the bits
of the NumPy functions.

Training.  Five plain-SGD steps of the whole RNN filter on the device path against the same filter on
CPU tensors, losses and every parameter, under the bound of
tests/test_gpu_dpf_rnn_grad.py::test_training_follows_the_cpu_filter: max(1e3 sens, 1e-9 size), with
sens the sensitivity of the torch CPU filter's training losses to the summation order (the hidden
units renumbered), measured here as there; for a parameter, size is its largest entry.
"""

import math

import numpy as np
import pytest
import torch

from particle_filters_amd import _dpf_common as DC
from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_rnn as RN
from particle_filters_amd import dpf_rnn_torch as RT
from particle_filters_amd import dpf_soft as SO
from particle_filters_amd import dpf_soft_torch as ST
from tests import dpf_rnn_grad_restatement as G
from tests import dpf_rnn_restatement as R
from tests import dpf_soft_grad_restatement as GR
from tests import dpf_soft_restatement as S

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert NV.device_count() > 0, "no HIP device visible: -m gpu tests must run on an MI355X"
    assert torch.cuda.is_available()


def close(tag, got, ref):
    """Every tensor of ``got`` within TOL max(1, max|ref|) of ``ref``; prints the errors."""
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        g, r = g.detach().cpu().numpy(), r.detach().cpu().numpy()
        assert g.shape == r.shape and np.all(np.isfinite(g)), (tag, k)
        scale = max(1.0, float(np.max(np.abs(r)))) if r.size else 1.0
        err = float(np.max(np.abs(g - r))) if r.size else 0.0
        print(f"{tag} [{k}]: error {err:.3e} (max |ref| {scale:.3g})")
        assert err <= TOL * scale, f"{tag} [{k}]: {err:.3e} > {TOL * scale:.3e}"


def bits(got, ref):
    return all(torch.equal(g.detach().cpu(), r.detach().cpu()) for g, r in zip(got, ref))


def paths():
    return dict(DC.PATH_CALLS)


def ran(before, path, n=1):
    """``n`` calls on ``path`` since ``before``, none on the other."""
    now = paths()
    other = "host" if path == "device" else "device"
    return now[path] == before[path] + n and now[other] == before[other]


class NoCpu:
    """``Tensor.cpu`` raises: what runs inside makes no copy to the host through it."""

    def __init__(self, monkeypatch):
        self.mp = monkeypatch

    def __enter__(self):
        self.ctx = self.mp.context()
        m = self.ctx.__enter__()

        def cpu(self, *a, **k):
            raise AssertionError("Tensor.cpu() on the device path")

        m.setattr(torch.Tensor, "cpu", cpu)

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)


def offset_view(t):
    """The same values as a view at storage offset 1 (8-byte aligned only)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.storage_offset() == 1 and v.is_contiguous()
    return v


def strided(t):
    """The same values, non-contiguous: the last two axes stored transposed."""
    v = t.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


# ====================================================================== the soft unit
SOFT = dict(N=65, d=3, B=2, alpha=0.1, T=0.2, seed=9, epoch=1)


def soft_inputs(unbatched=False):
    c = SOFT
    X = np.stack([S.make_case(c["N"], c["d"], seed=4 + b)[0] for b in range(c["B"])])
    lw = np.stack([S.make_case(c["N"], c["d"], seed=4 + b)[1] for b in range(c["B"])])
    g = np.random.default_rng([c["N"], c["d"], 5]).standard_normal(X.shape)
    return (X[0], lw[0], g[0]) if unbatched else (X, lw, g)


def soft_run(X, lw, g, dev_x="cuda", dev_w=None, check_values=True, wrap=None, device_path=True):
    """(new particles, new log-weights, grad particles, grad log-weights) of one soft_resample and
    its backward pass, on tensors made from the arrays."""
    c = SOFT
    x = torch.tensor(X, device=dev_x)
    w = torch.tensor(lw, device=dev_w or dev_x)
    if wrap is not None:
        x, w = wrap(x), wrap(w)
    x.requires_grad_(True)
    w.requires_grad_(True)
    out, nlw = ST.soft_resample(x, w, c["alpha"], c["T"], seed=c["seed"], epoch=c["epoch"], device_path=device_path,
                                check_values=check_values)
    (out * torch.tensor(g, device=out.device)).sum().backward()
    return [out, nlw, x.grad, w.grad]


_soft_ref = {}


def soft_ref(unbatched=False):
    if unbatched not in _soft_ref:
        _soft_ref[unbatched] = soft_run(*soft_inputs(unbatched), dev_x="cpu")
    return _soft_ref[unbatched]


@pytest.mark.parametrize("unbatched", [False, True])
def test_soft_resample_on_cuda_tensors(unbatched):
    ref = soft_ref(unbatched)
    before = paths()
    got = soft_run(*soft_inputs(unbatched))
    assert ran(before, "device")
    assert all(t.is_cuda and t.device.index == 0 for t in got)
    close("soft device path", got, ref)


def test_soft_resample_without_value_checks_never_touches_the_host(monkeypatch):
    X, lw, g = soft_inputs()
    ref = soft_run(X, lw, g)
    before = paths()
    with NoCpu(monkeypatch):
        got = soft_run(X, lw, g, check_values=False)
    assert ran(before, "device")
    assert bits(got, ref)


@pytest.mark.parametrize("wrap", [strided, offset_view], ids=["non_contiguous", "storage_offset_1"])
def test_soft_resample_layouts_give_the_contiguous_bits(wrap):
    X, lw, g = soft_inputs()
    before = paths()
    assert bits(soft_run(X, lw, g, wrap=wrap), soft_run(X, lw, g))
    assert ran(before, "device", 2)


def test_soft_cuda_tensors_take_the_host_path_unless_the_device_path_is_asked_for():
    """The default keeps what tests/test_gpu_dpf_soft_grad.py pins: tensors on the device go through host
    memory and give the bits of CPU tensors."""
    X, lw, g = soft_inputs()
    before = paths()
    got = soft_run(X, lw, g, device_path=False)
    assert ran(before, "host")
    assert all(t.is_cuda for t in got)
    assert bits(got, soft_ref())


def test_soft_cpu_and_mixed_tensors_take_the_host_path():
    c = SOFT
    X, lw, g = soft_inputs()
    today, _, saved = SO.soft_resample(X, lw, c["alpha"], c["T"], seed=c["seed"], epoch=c["epoch"], return_saved=True)
    gX, glw = SO.soft_resample_vjp(X, lw, g, c["alpha"], c["T"], seed=c["seed"], epoch=c["epoch"], saved=saved)
    for dev_x, dev_w in (("cpu", "cpu"), ("cuda", "cpu"), ("cpu", "cuda")):
        before = paths()
        got = soft_run(X, lw, g, dev_x=dev_x, dev_w=dev_w)
        assert ran(before, "host")
        assert got[0].device.type == dev_x and got[3].device.type == dev_w
        for t, a in zip([got[0], got[2], got[3]], [today, gX, glw]):
            assert np.array_equal(t.detach().cpu().numpy(), a)


# ====================================================================== the RNN unit
RNN_CASES = [R.PARITY[11], R.PARITY[1]]  # LSTM L = 2, B = 3, N = 17; GRU L = 2, N = 3, run unbatched


def rnn_run(c, dev="cuda", dev_W=None, check_values=True, wrap=None, only_particles=False):
    """[new particles, A, grad particles, grad log-weights, weight gradients...] of one rnn_resample and
    its backward pass through both outputs."""
    X, lw, W = R.case_inputs(c)
    gXo, gA = G.cotangents(c)
    if c["B"] == 1:
        X, lw, gXo, gA = X[0], lw[0], gXo[0], gA[0]
    x, w = torch.tensor(X, device=dev), torch.tensor(lw, device=dev)
    Wt = [torch.tensor(a, device=dev_W or dev, requires_grad=True) for a in W]
    if wrap is not None:
        x, w = wrap(x), wrap(w)
    x.requires_grad_(True)
    w.requires_grad_(True)
    new, A = RT.rnn_resample(x, w, Wt, c["cell"], c["T"], use_weight_features=c["uw"], use_particle_features=c["up"],
                             check_values=check_values)
    loss = (new * torch.tensor(gXo, device=new.device)).sum()
    if not only_particles:
        loss = loss + (A * torch.tensor(gA, device=A.device)).sum()
    loss.backward()
    return [new, A, x.grad, w.grad] + [p.grad for p in Wt]


_rnn_ref = {}


def rnn_ref(c):
    key = R.case_id(c)
    if key not in _rnn_ref:
        _rnn_ref[key] = rnn_run(c, dev="cpu")
    return _rnn_ref[key]


@pytest.mark.parametrize("c", RNN_CASES, ids=R.case_id)
def test_rnn_resample_on_cuda_tensors(c):
    ref = rnn_ref(c)
    before = paths()
    got = rnn_run(c)
    assert ran(before, "device")
    assert all(t.is_cuda and t.device.index == 0 for t in got)
    close("rnn device path " + R.case_id(c), got, ref)
    # one output alone: the other's cotangent is zero
    close("rnn device path, particles only", rnn_run(c, only_particles=True)[2:],
          rnn_run(c, dev="cpu", only_particles=True)[2:])


def test_rnn_resample_without_value_checks_never_touches_the_host(monkeypatch):
    c = RNN_CASES[0]
    ref = rnn_run(c)
    before = paths()
    with NoCpu(monkeypatch):
        got = rnn_run(c, check_values=False)
    assert ran(before, "device")
    assert bits(got, ref)


@pytest.mark.parametrize("wrap", [strided, offset_view], ids=["non_contiguous", "storage_offset_1"])
def test_rnn_resample_layouts_give_the_contiguous_bits(wrap):
    c = RNN_CASES[0]
    assert bits(rnn_run(c, wrap=wrap), rnn_run(c))


def test_rnn_cpu_and_mixed_tensors_take_the_host_path():
    c = RNN_CASES[0]
    X, lw, W = R.case_inputs(c)
    gXo, gA = G.cotangents(c)
    new, A = RN.rnn_resample(X, lw, W, c["cell"], c["T"])
    gX, glw, gW = RN.rnn_resample_vjp(X, lw, W, gXo, gA, c["cell"], c["T"])
    for dev, dev_W in (("cpu", "cpu"), ("cuda", "cpu")):
        before = paths()
        got = rnn_run(c, dev=dev, dev_W=dev_W)
        assert ran(before, "host")
        assert got[0].device.type == dev and got[4].device.type == dev_W
        for t, a in zip(got, [new, A, gX, glw] + gW):
            assert np.array_equal(t.detach().cpu().numpy(), a)


# ====================================================================== 8. the value checks on the device path
def test_soft_value_checks_on_the_device_path():
    c = SOFT
    X, lw, g = soft_inputs()
    x, w = torch.tensor(X, device="cuda"), torch.tensor(lw, device="cuda")

    def call(x, w, **kw):
        before = paths()
        try:
            return ST.soft_resample(x, w, c["alpha"], c["T"], seed=c["seed"], epoch=c["epoch"], device_path=True, **kw)
        finally:
            assert paths()["host"] == before["host"]  # nothing fell back to the host path

    bad = x.clone()
    bad[1, 2, 0] = math.nan
    with pytest.raises(ValueError, match="particles must be finite"):
        call(bad, w)
    bad = w.clone()
    bad[0, 3] = math.nan
    with pytest.raises(ValueError, match="log_weights must not hold NaN or \\+inf"):
        call(x, bad)
    bad = w.clone()
    bad[1] = -math.inf
    with pytest.raises(ValueError, match="every problem needs at least one finite log-weight"):
        call(x, bad)
    with pytest.raises(ValueError, match="particles must be \\(N, d\\) or \\(B, N, d\\)"):
        call(x[0, 0], w[0, 0])
    with pytest.raises(ValueError, match="disagree on N"):
        call(x, w[:, :-1])
    with pytest.raises(ValueError, match="soft_alpha must be in \\[0, 1\\]"):
        ST.soft_resample(x, w, 1.5, c["T"], device_path=True)
    with pytest.raises(TypeError, match="float64"):
        call(x.float(), w)
    xg = x.clone().requires_grad_(True)
    out, _ = call(xg, w)
    with pytest.raises(ValueError, match="grad_new_particles must be finite"):
        out.backward(torch.full_like(out, math.inf))
    # a log-weight of -inf gets the gradient exactly 0
    lwi = w.clone()
    lwi[:, 1::3] = -math.inf
    lwi.requires_grad_(True)
    out, _ = call(x, lwi)
    (out * torch.tensor(g, device="cuda")).sum().backward()
    grad = lwi.grad.cpu().numpy()
    assert np.all(np.isfinite(grad)) and np.array_equal(grad == 0.0, np.isinf(lwi.detach().cpu().numpy()))
    # double backward is not implemented
    xg = x.clone().requires_grad_(True)
    out, _ = call(xg, w)
    (gx,) = torch.autograd.grad(out.sum(), xg, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_rnn_value_checks_on_the_device_path():
    c = R.PARITY[13]  # GRU, L = 2, N = 17, every third log-weight -inf
    assert c["kind"] == "neginf"
    X, lw, W = R.case_inputs(c)
    gXo, gA = G.cotangents(c)
    x, w = torch.tensor(X[0], device="cuda"), torch.tensor(lw[0], device="cuda")
    Wt = [torch.tensor(a, device="cuda", requires_grad=True) for a in W]

    def call(x, w, Wt=Wt, **kw):
        before = paths()
        try:
            return RT.rnn_resample(x, w, Wt, c["cell"], c["T"], **kw)
        finally:
            assert paths()["host"] == before["host"]

    bad = x.clone()
    bad[2, 1] = math.inf
    with pytest.raises(ValueError, match="particles must be finite"):
        call(bad, w)
    bad = w.clone()
    bad[0] = math.nan
    with pytest.raises(ValueError, match="log_weights must not hold NaN or \\+inf"):
        call(x, bad)
    with pytest.raises(ValueError, match="every problem needs at least one finite log-weight"):
        call(x, torch.full_like(w, -math.inf))
    badW = [a.detach().clone() for a in Wt]
    badW[4][0, 0] = math.nan
    with pytest.raises(ValueError, match="weight array 4 must be finite"):
        call(x, w, badW)
    with pytest.raises(ValueError, match="weight array 1 has shape"):
        call(x, w, [Wt[0], Wt[1][:, :-1]] + Wt[2:])
    with pytest.raises(ValueError, match="temperature must be positive"):
        RT.rnn_resample(x, w, Wt, c["cell"], 0.0)
    with pytest.raises(TypeError, match="float64"):
        call(x.float(), w)
    with pytest.raises(TypeError, match="float64"):
        call(x, w, [a.float() for a in Wt])
    xg = x.clone().requires_grad_(True)
    new, A = call(xg, w)
    with pytest.raises(ValueError, match="grad_new_particles must be finite"):
        new.backward(torch.full_like(new, math.nan), retain_graph=True)
    with pytest.raises(ValueError, match="grad_assignment must be finite"):
        A.backward(torch.full_like(A, math.inf))
    # a log-weight of -inf gets the gradient exactly 0
    wg = w.clone().requires_grad_(True)
    new, A = call(x, wg)
    ((new * torch.tensor(gXo[0], device="cuda")).sum() + (A * torch.tensor(gA[0], device="cuda")).sum()).backward()
    grad = wg.grad.cpu().numpy()
    assert np.all(np.isfinite(grad)) and np.all(grad[np.isinf(lw[0])] == 0.0) and np.any(grad != 0.0)
    # double backward is not implemented
    xg = x.clone().requires_grad_(True)
    new, _ = call(xg, w)
    (gx,) = torch.autograd.grad(new.sum(), xg, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


# ====================================================================== the whole filters
def lgssm(noise, a, device, sigma_q=0.5, sigma_r=0.5):
    """tests/dpf_rnn_grad_restatement.lgssm with the noise on ``device``."""
    noise = [torch.tensor(e, device=device) for e in noise]
    calls = {"k": 0}

    def transition_fn(x, params):
        eps = noise[calls["k"] % len(noise)]
        calls["k"] += 1
        return a * x + sigma_q * eps

    def log_likelihood_fn(x, y, params):
        var = sigma_r ** 2
        diff = y[:, None, :] - x
        return torch.sum(-0.5 * math.log(2.0 * math.pi * var) - 0.5 * diff ** 2 / var, dim=-1)

    return transition_fn, log_likelihood_fn


def rnn_filter(cell, device, weights=None, **kw):
    obs, noise, _ = G.filter_problem(cell)
    a = torch.tensor(0.9, dtype=torch.float64, device=device, requires_grad=True)
    tf, lf = lgssm(noise, a, device)
    dpf = RT.DifferentiableParticleFilterRNN(G.FN, G.FD, tf, lf, rnn_type=cell, rnn_hidden_dim=G.FH,
                                             rnn_num_layers=G.FL, weights=weights,
                                             rng=np.random.default_rng(G.FSEED), **kw)
    assert dpf.to(device) is dpf
    return dpf, a, torch.tensor(obs, device=device), noise


def rnn_filter_grads(cell, device):
    """[particles, log-weights, assignments, loss, d/da, d/d init_mean, d/d every parameter]"""
    _, _, W = G.filter_problem(cell)
    dpf, a, obs, _ = rnn_filter(cell, device, W)
    try:
        params = dpf.parameters()
        mean = torch.zeros(G.FD, dtype=torch.float64, device=device, requires_grad=True)
        before = paths()
        ps, lws, As = dpf.filter(obs, mean, torch.eye(G.FD, dtype=torch.float64, device=device))
        assert ran(before, "device" if device == "cuda" else "host", G.FSTEPS)
        loss = G.filter_loss(ps, As, obs)
        loss.backward()
        assert all(p is q for p, q in zip(params, dpf.parameters()))  # .to() kept the Parameter objects
        packs = dpf._h.packs
    finally:
        dpf.close()
    return [ps, lws, As, loss, a.grad, mean.grad] + [p.grad for p in params], packs


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_whole_rnn_filter_on_the_device(cell):
    ref, _ = rnn_filter_grads(cell, "cpu")
    got, packs = rnn_filter_grads(cell, "cuda")
    assert all(t.is_cuda for t in got)
    assert got[0].shape == (G.FB, G.FSTEPS + 1, G.FN, G.FD) and got[2].shape == (G.FB, G.FSTEPS, G.FN, G.FN)
    assert all(float(r.abs().max()) > 1e-3 for r in ref[4:])  # gradients that are there
    close("rnn filter on the device, " + cell, got, ref)
    # 9. the frozen weights were packed once for the T forward and the T backward passes
    assert packs == 1


def test_the_rnn_binding_repacks_when_a_parameter_changes():
    cell = "gru"
    _, _, W = G.filter_problem(cell)
    dev, a, obs, _ = rnn_filter(cell, "cuda", W)
    cpu, _, obs_c, _ = rnn_filter(cell, "cpu", W)
    try:
        mean, eye = torch.zeros(G.FD, dtype=torch.float64), torch.eye(G.FD, dtype=torch.float64)
        with torch.no_grad():
            first = dev.filter(obs, mean.cuda(), eye.cuda())
            assert dev._h.packs == 1
            dev.rng = np.random.default_rng(G.FSEED)
            assert bits(dev.filter(obs, mean.cuda(), eye.cuda()), first)
            assert dev._h.packs == 1  # nothing changed: no repack
            for p, q in zip(dev.parameters(), cpu.parameters()):
                p.add_(0.25)
                q.add_(0.25)
            dev.rng = np.random.default_rng(G.FSEED)
            got = dev.filter(obs, mean.cuda(), eye.cuda())
            assert dev._h.packs == 2  # one repack for the T steps at the new weights
            ref = cpu.filter(obs_c, mean, eye)
        close("rnn filter after an in-place update", got, ref)
        assert float((got[2] - first[2]).abs().max()) > 1e-6  # and the new weights did change the result
    finally:
        dev.close()
        cpu.close()


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_training_on_the_device_follows_the_cpu_tensor_filter(cell):
    def train(device):
        dpf, _, obs, noise = rnn_filter(cell, device)  # the default initialisation, from default_rng(FSEED)
        losses = []
        try:
            opt = torch.optim.SGD(dpf.parameters(), lr=G.LR)  # built after .to(), as with nn.Module
            for _ in range(G.TRAIN_STEPS):
                dpf.transition_fn, dpf.log_likelihood_fn = lgssm(
                    noise, torch.tensor(0.9, dtype=torch.float64, device=device), device)
                dpf.rng = np.random.default_rng(G.FSEED)
                opt.zero_grad()
                ps, _, As = dpf.filter(obs, torch.zeros(G.FD, dtype=torch.float64, device=device),
                                       torch.eye(G.FD, dtype=torch.float64, device=device))
                loss = G.filter_loss(ps, As, obs)
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
            packs = dpf._h.packs
            return np.array(losses), [p.detach().cpu().numpy() for p in dpf.parameters()], packs
        finally:
            dpf.close()

    ref_losses, ref_params, _ = train("cpu")
    losses, params, packs = train("cuda")
    assert packs == G.TRAIN_STEPS  # one packing per optimizer step
    sens = float(np.max(np.abs(np.array(G.cpu_training(cell)) - np.array(G.cpu_training(cell, permute=True)))))
    for name, g, r in [("losses", losses, ref_losses)] + list(zip(G.names(G.FL), params, ref_params)):
        size = float(np.max(np.abs(r)))
        bound = max(1e3 * sens, 1e-9 * size)
        err = float(np.max(np.abs(g - r)))
        print(f"rnn training on the device, {cell} {name}: max |ref| {size:.4g}, error {err:.3e}, CPU order "
              f"sensitivity {sens:.3e}, bound {bound:.3e}")
        assert err <= bound
    assert losses[-1] < losses[0]


SOFT_FILTER = dict(B=2, N=17, d=2, T=3, alpha=0.1, temp=0.2, seed=23, a=0.9, sigma=0.3, sigma_r=0.5, rng=41)


def soft_filter_grads(device, **kw):
    """[particles, log-weights, loss, d/da, d/dsigma, d/d init_mean] of the soft filter with the model of
    tests/dpf_soft_grad_restatement.py at B = 2, N = 17, T = 3."""
    c = SOFT_FILTER
    B, N, d, T = c["B"], c["N"], c["d"], c["T"]
    rng = np.random.default_rng([B, N, d, T])
    eps = torch.tensor(rng.standard_normal((T, B, N, d)), device=device)
    obs = torch.tensor(rng.standard_normal((B, T, d)), device=device)
    targets = torch.tensor(0.5 * rng.standard_normal((B, T + 1, d)), device=device)
    a = torch.tensor(c["a"], dtype=torch.float64, device=device, requires_grad=True)
    sigma = torch.tensor(c["sigma"], dtype=torch.float64, device=device, requires_grad=True)
    mean = torch.zeros(d, dtype=torch.float64, device=device, requires_grad=True)
    tf_, lf_ = GR.model(a, sigma, eps, c["sigma_r"])
    flt = ST.DifferentiableParticleFilter(N, d, tf_, lf_, c["alpha"], c["temp"], seed=c["seed"],
                                          rng=np.random.default_rng(c["rng"]), device_path=True, **kw)
    try:
        before = paths()
        ps, lws = flt.filter(obs, mean, torch.eye(d, dtype=torch.float64, device=device))
        assert ran(before, "device" if device == "cuda" else "host", T) and flt.epoch == T
        loss = GR.loss_of(ps, lws, targets)
        loss.backward()
    finally:
        flt.close()
    return [ps, lws, loss, a.grad, sigma.grad, mean.grad]


def test_whole_soft_filter_on_the_device(monkeypatch):
    ref = soft_filter_grads("cpu")
    got = soft_filter_grads("cuda")
    assert all(t.is_cuda for t in got)
    assert all(float(r.abs().max()) > 1e-3 for r in ref[3:])  # gradients that are there
    close("soft filter on the device", got, ref)
    with NoCpu(monkeypatch):  # with the value checks off a whole filter and its backward pass stay on the device
        unchecked = soft_filter_grads("cuda", check_values=False)
    assert bits(unchecked, got)
