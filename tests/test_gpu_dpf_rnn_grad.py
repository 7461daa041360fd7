"""The backward pass of the RNN resampler (pf_rnn_backward) and its PyTorch binding on the device
(-m gpu, MI355X).

The reference is PyTorch's CPU fp64 autograd of tests/dpf_rnn_grad_restatement.py, the torch
restatement of tests/dpf_rnn_restatement.resample, with the loss sum gXo . X' + sum gA . A for fixed
random gXo and gA; tests/test_dpf_rnn_grad_host.py checks that restatement against the NumPy one,
against central differences, that no reference gradient vanishes, and its conditioning (the hidden
units of every layer renumbered move a gradient by at most 3.5e-14 relative; asserted there at 1e-12
for every case used here).  Nothing takes finite differences on the device.

Parity.  The cases of R.PARITY, the smallest shapes at which each tiling of the forward and so of the
backward recurrence can go wrong (tests/dpf_rnn_restatement.py lists what each exercises).  Every
returned array - grad_X, grad_log_weights and the 3 L + 2 weight gradients - within the project's
1e-9 max(1, max|ref|), four orders above the conditioning.

Bitwise properties: no floating-point atomics and every summation order fixed by (N, d, H, L), so two
calls, forced streaming against resident, a problem in a batch against alone, the batch's weight
gradients against the alone ones added in ascending b, and any order of backward calls agree in every
bit, and pf_rnn_resample returns after a backward pass the bits it returned before.

N = 16 against 17.  At N = 17 the second row tile holds one particle and 15 padding rows, which
re-form row 16: its own gradient gK0[F0 + 16] must be that row's alone, and no sum may pick up a
second copy of it.

The whole filter.  B = 2, N = 17, d = 1, H = 8, L = 1, GRU and LSTM, T = 3 steps, the LGSSM with a
tensor ``a`` that requires grad; loss = sum_t |mean particle_t - y_t|^2 + 0.1 sum A^2, which uses both
results of the resampler.  d loss / d(every parameter, a, init_mean) through the device-backed filter
against the same filter written entirely in torch on the CPU.  The bound is 1e3 times the CPU filter's
own sensitivity to the summation order (the same CPU filter with the hidden units renumbered), floored
at 1e-9 relative to the gradient.  Measured on the CPU: the two orders differ by at most 1.1e-15
(gK0 of the LSTM, value 0.67; every other gradient below 1e-15, values 0.22 .. 2.84), 1e3 times that
is 1.1e-12, so the floor, 1e-9 relative, is the bound in force for all of them.  Training: five
plain-SGD steps (rate 0.5) from the default initialisation; the losses against the CPU filter's within
the same bound (the CPU's two orders agree to 1e-15 on them).

Largest errors measured on an MI355X: DESIGN.md section 4, "RNN resampling: the backward pass".
"""

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_rnn as RN
from tests import dpf_rnn_grad_restatement as G
from tests import dpf_rnn_restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert NV.device_count() > 0, "no HIP device visible: -m gpu tests must run on an MI355X"


def kw(c):
    return dict(rnn_type=c["cell"], temperature=c["T"], use_weight_features=c["uw"], use_particle_features=c["up"])


def device(c, X, lw, W, gXo, gA, handle=None):
    """[gX, glw, gW...] (batched) of one rnn_resample_vjp."""
    gX, glw, gW = RN.rnn_resample_vjp(X, lw, W, gXo, gA, _handle=handle, **kw(c))
    return [gX, glw] + gW


def handle(c, B=None):
    return RN._Handle(c["N"], c["d"], c["B"] if B is None else B, c["H"], c["L"], c["cell"], c["uw"], c["up"])


def compare(tag, got, ref, L):
    """Every array within 1e-9 max(1, max|ref|); prints the errors."""
    worst = 0.0
    for name, g, r in zip(["gX", "glw"] + G.names(L), got, ref):
        assert g.shape == r.shape and np.all(np.isfinite(g)), name
        scale = max(1.0, float(np.max(np.abs(r)))) if r.size else 1.0
        err = float(np.max(np.abs(g - r))) if r.size else 0.0
        print(f"rnn grad {tag} {name}: error {err:.3e} (max |ref| {float(np.max(np.abs(r))):.3g})")
        worst = max(worst, err / scale)
        assert err <= TOL * scale, f"{tag} {name}: {err:.3e} > {TOL * scale:.3e}"
    return worst


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("c", R.PARITY, ids=lambda c: R.case_id(c))
def test_parity(c):
    X, lw, W, gXo, gA, ref = G.solved(c)
    if c["B"] == 1:  # the unbatched form
        gX, glw, gW = RN.rnn_resample_vjp(X[0], lw[0], W, gXo[0], gA[0], **kw(c))
        assert gX.shape == (c["N"], c["d"]) and glw.shape == (c["N"],)
        got = [gX[None], glw[None]] + gW
    else:
        got = device(c, X, lw, W, gXo, gA)
    compare(R.case_id(c), got, [ref[2], ref[3]] + list(ref[4]), c["L"])
    if c["kind"] == "neginf":
        assert np.all(got[1][~np.isfinite(lw)] == 0.0)
    if not c["uw"]:
        assert np.all(got[1] == 0.0)


# ------------------------------------------------------------------ 2. grad_A
BITS = [R.PARITY[4], R.PARITY[8], R.PARITY[11]]  # LSTM L = 3 with a partial tile; GRU L = 2, N = 35; LSTM B = 3


@pytest.mark.parametrize("c", BITS[:2], ids=lambda c: R.case_id(c))
def test_no_grad_A_is_zero_grad_A(c):
    X, lw, W, gXo, gA, _ = G.solved(c)
    assert same_bits(device(c, X, lw, W, gXo, None), device(c, X, lw, W, gXo, np.zeros_like(gA)))


# ------------------------------------------------------------------ 3. bitwise properties
@pytest.mark.parametrize("c", BITS, ids=lambda c: R.case_id(c))
def test_two_calls_and_forced_streaming_agree_bitwise(c, monkeypatch):
    X, lw, W, gXo, gA, _ = G.solved(c)
    monkeypatch.delenv("PF_TEST_RNN_STREAM", raising=False)
    h = handle(c)
    try:
        assert h.resident
        first = device(c, X, lw, W, gXo, gA, h)
        assert same_bits(first, device(c, X, lw, W, gXo, gA, h))
    finally:
        h.close()
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_RNN_STREAM", "1")
    h = handle(c)
    try:
        assert not h.resident
        assert same_bits(first, device(c, X, lw, W, gXo, gA, h))
    finally:
        h.close()


def test_batch_against_alone():
    c = R.PARITY[11]  # B = 3
    X, lw, W, gXo, gA, _ = G.solved(c)
    batch = device(c, X, lw, W, gXo, gA)
    alone = [device(c, X[b:b + 1], lw[b:b + 1], W, gXo[b:b + 1], gA[b:b + 1]) for b in range(c["B"])]
    for b in range(c["B"]):
        assert np.array_equal(batch[0][b], alone[b][0][0]) and np.array_equal(batch[1][b], alone[b][1][0])
    for k in range(2, len(batch)):  # the weight gradients: the alone ones added in ascending b
        total = alone[0][k]
        for b in range(1, c["B"]):
            total = total + alone[b][k]
        assert np.array_equal(batch[k], total), G.names(c["L"])[k - 2]


def test_order_of_backward_calls_and_forward_after_backward():
    c = R.PARITY[8]
    X, lw, W, gXo, gA, _ = G.solved(c)
    W2 = [np.ascontiguousarray(0.5 * a[::-1]) for a in W]
    w = np.ascontiguousarray(np.exp(lw))
    h = handle(c)
    try:
        h.set_weights(W)
        fwd = h.resample(X, w, c["T"], want_hidden=True)
        a1 = device(c, X, lw, W, gXo, gA, h)
        h.set_weights(W)
        assert same_bits(fwd, h.resample(X, w, c["T"], want_hidden=True))  # the forward pass after a backward pass
        a2 = device(c, X, lw, W2, gXo, gA, h)
        # backward calls in the reverse order of their forward passes, after another network's
        h.set_weights(W)
        h.resample(X, w, c["T"])
        h.set_weights(W2)
        h.resample(X, w, c["T"])
        assert same_bits(a1, device(c, X, lw, W, gXo, gA, h))
        assert same_bits(a2, device(c, X, lw, W2, gXo, gA, h))
        assert h.backward_bytes > 0
    finally:
        h.close()
    assert not same_bits(a1, a2)


# ------------------------------------------------------------------ 4. N = 16 against 17
def test_padded_row_of_the_second_tile():
    """N = 17: row 16 is alone in its tile, beside 15 padding rows that re-form it.  The network's
    function of row 16 does not change when the padding rows are there, so compare with the reference
    per array, and pin gK0[F0 + 16], that row's own gradient: a second copy would double it."""
    c = R.case(17, 2, 16, 1, "lstm", seed=51)
    X, lw, W, gXo, gA, ref = G.solved(c)
    got = device(c, X, lw, W, gXo, gA)
    compare("N17 padded tile", got, [ref[2], ref[3]] + list(ref[4]), 1)
    F0 = 3
    own, want = got[2][F0 + 16], ref[4][0][F0 + 16]
    assert np.max(np.abs(want)) > 1e-3
    assert np.max(np.abs(own - want)) <= TOL * max(1.0, np.max(np.abs(want)))
    assert np.max(np.abs(2.0 * want - own)) > 1e-4  # and not the doubled one
    c16 = R.case(16, 2, 16, 1, "lstm", seed=51)  # an exact tile beside it
    X, lw, W, gXo, gA, ref = G.solved(c16)
    compare("N16 exact tile", device(c16, X, lw, W, gXo, gA), [ref[2], ref[3]] + list(ref[4]), 1)


# ------------------------------------------------------------------ 5. torch
def test_torch_function_through_both_outputs():
    import torch

    from particle_filters_amd import dpf_rnn_torch as RT

    c = R.PARITY[4]
    X, lw, W, gXo, gA, ref = G.solved(c)
    Xt = torch.tensor(np.array(X[0]), requires_grad=True)
    lwt = torch.tensor(np.array(lw[0]), requires_grad=True)
    Wt = [torch.tensor(np.array(a), requires_grad=True) for a in W]
    new, A = RT.rnn_resample(Xt, lwt, Wt, c["cell"], c["T"])
    assert np.max(np.abs(new.detach().numpy() - ref[0][0])) <= TOL * max(1.0, np.max(np.abs(ref[0])))
    assert np.max(np.abs(A.detach().numpy() - ref[1][0])) <= TOL
    ((torch.tensor(gXo[0]) * new).sum() + (torch.tensor(gA[0]) * A).sum()).backward()
    compare("torch " + R.case_id(c), [Xt.grad.numpy()[None], lwt.grad.numpy()[None]] + [p.grad.numpy() for p in Wt],
            [ref[2], ref[3]] + list(ref[4]), c["L"])
    # one output alone: the other's cotangent is zero
    Xt.grad = None
    new, A = RT.rnn_resample(Xt, lwt, Wt, c["cell"], c["T"])
    (torch.tensor(gXo[0]) * new).sum().backward()
    only = RN.rnn_resample_vjp(X[0], lw[0], W, gXo[0], None, **kw(c))[0]
    assert np.array_equal(Xt.grad.numpy(), only)


def test_torch_dtype_and_double_backward_errors():
    import torch

    from particle_filters_amd import dpf_rnn_torch as RT

    c = R.PARITY[1]
    X, lw, W, _, _, _ = G.solved(c)
    Wt = [torch.tensor(np.array(a), requires_grad=True) for a in W]
    with pytest.raises(TypeError, match="float64"):
        RT.rnn_resample(torch.tensor(np.array(X[0]), dtype=torch.float32), torch.tensor(np.array(lw[0])), Wt, c["cell"])
    with pytest.raises(TypeError, match="float64"):
        RT.rnn_resample(torch.tensor(np.array(X[0])), torch.tensor(np.array(lw[0])),
                        [a.float() for a in Wt], c["cell"])
    Xt = torch.tensor(np.array(X[0]), requires_grad=True)
    new, _ = RT.rnn_resample(Xt, torch.tensor(np.array(lw[0])), Wt, c["cell"])
    (g,) = torch.autograd.grad(new.sum(), Xt, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def _device_filter(cell, weights=None):
    import torch

    from particle_filters_amd import dpf_rnn_torch as RT

    obs, noise, _ = G.filter_problem(cell)
    a = torch.tensor(0.9, dtype=torch.float64, requires_grad=True)
    tf, lf = G.lgssm(noise, a)
    dpf = RT.DifferentiableParticleFilterRNN(G.FN, G.FD, tf, lf, rnn_type=cell, rnn_hidden_dim=G.FH,
                                             rnn_num_layers=G.FL, weights=weights,
                                             rng=np.random.default_rng(G.FSEED))
    return dpf, a, obs, noise


def _bound(name, got, ref, other):
    size = float(np.max(np.abs(ref)))
    sens = float(np.max(np.abs(np.asarray(ref) - np.asarray(other))))
    bound = max(1e3 * sens, 1e-9 * size)
    err = float(np.max(np.abs(np.asarray(got) - np.asarray(ref))))
    print(f"rnn filter {name}: max |ref| {size:.4g}, error {err:.3e}, CPU order sensitivity {sens:.3e}, "
          f"bound {bound:.3e}")
    return err, bound, size


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_whole_filter_gradients(cell):
    import torch

    _, _, W = G.filter_problem(cell)
    dpf, a, obs, _ = _device_filter(cell, W)
    try:
        mean = torch.zeros(G.FD, dtype=torch.float64, requires_grad=True)
        ps, lws, As = dpf.filter(obs, mean, torch.eye(G.FD, dtype=torch.float64))
        assert ps.shape == (G.FB, G.FSTEPS + 1, G.FN, G.FD) and As.shape == (G.FB, G.FSTEPS, G.FN, G.FN)
        loss = G.filter_loss(ps, As, obs)
        loss.backward()
    finally:
        dpf.close()
    ref_loss, ref = G.cpu_filter_grads(cell, W)
    rev_loss, rev = G.cpu_filter_grads(cell, W, permute=True)
    err, bound, _ = _bound("loss", float(loss.detach()), ref_loss, rev_loss)
    assert err <= bound
    got = {"a": a.grad.numpy(), "init_mean": mean.grad.numpy()}
    got.update(zip(G.names(G.FL), [p.grad.numpy() for p in dpf.parameters()]))
    for name in ref:
        err, bound, size = _bound("d loss/d " + name, got[name], ref[name], rev[name])
        assert size > 1e-3  # a gradient that is there
        assert err <= bound


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_training_follows_the_cpu_filter(cell):
    import torch

    dpf, _, obs, noise = _device_filter(cell)  # the default initialisation, from default_rng(FSEED)
    losses = []
    try:
        opt = torch.optim.SGD(dpf.parameters(), lr=G.LR)
        for _ in range(G.TRAIN_STEPS):
            dpf.transition_fn, dpf.log_likelihood_fn = G.lgssm(noise, torch.tensor(0.9, dtype=torch.float64))
            dpf.rng = np.random.default_rng(G.FSEED)
            opt.zero_grad()
            ps, _, As = dpf.filter(obs, torch.zeros(G.FD, dtype=torch.float64), torch.eye(G.FD, dtype=torch.float64))
            loss = G.filter_loss(ps, As, obs)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    finally:
        dpf.close()
    ref, rev = G.cpu_training(cell), G.cpu_training(cell, permute=True)
    err, bound, _ = _bound("training losses", losses, ref, rev)
    assert err <= bound
    assert losses[-1] < losses[0]
