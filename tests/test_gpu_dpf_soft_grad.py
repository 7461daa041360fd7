"""Backward pass of the soft (Gumbel-Softmax) resampler on the device, and its PyTorch binding
(-m gpu, MI355X).

The reference is PyTorch's CPU fp64 autograd of the literal forward on the same Philox draws
(tests/dpf_soft_grad_restatement.py, checked against the closed form by
tests/test_dpf_soft_grad_host.py).  Nothing here takes finite differences on the device.

Bounds.  g log_weights within 1e-9 sc, where sc = max(1, max_j sum_i a_ij (|gX'_i| . |X_j| + |r_i|) / T)
is the size of the terms that every form of the gradient sums; gX within 1e-9 max(1, max|gX_ref|).
1e-9 x scale is the bound of this resampler's forward pass.  The device sums over the rows in
another order (splits of the row range, tiles), multiplies by 1 / T and 1 / L_i where the reference
divides, forms glp as (X_j . gX_j - sum_i a_ij r_i) / T, and uses the device library's exp and log.
Every case with alpha < 1 and N >= 2 must have max|g log_weights_ref| > 1e-3 sc, so a backward pass
that returns zeros cannot pass (on the CPU the smallest ratio is 4.8e-3, at N = 63, d = 16).

The cases are the twelve PARITY cases of the forward pass, the smallest shapes at which each loop of
k_soft_bwd_pass can go wrong: N = 1, 2, 3 the dropped half of the last Philox pair and a lane's
missing second column; N = 63 / 64 / 65 one tile of rows and its tails; N = 130 / 300 two and three
workgroups of 128 columns, the last one partly padding, and 5 / 10 row splits; d = 16 / 17 / 40 the
chunk boundary and three chunks with the r column riding on chunk 0.  PF_TEST_SOFT_SPLITS = 1, 2, 3 at
N = 300 runs the tile loop more than once inside a split (tiles 64 x 4 + 44; 64 + 64 + 32 and
64 + 64 + 12; 64 + 64 twice and 44).

The whole filter.  B = 2, N = 65, d = 2, T = 3 steps, transition a x + sigma eps with a and sigma
tensors that require grad, a Gaussian likelihood, loss = sum_t |weighted mean_t - target_t|^2.
d loss / da, d loss / dsigma and d loss / dinit_mean through the device-backed filter against the
same filter written entirely in torch on the CPU with the restatement's draws.  The bound is 1e3
times the CPU filter's own sensitivity to the summation order (the same CPU filter with the sources
visited in reverse), floored at 1e-9 relative to the gradient.  Measured on the CPU: the two orders
differ by 1.1e-14 (d/da, value 13.96), 5.7e-14 (d/dsigma, 17.88) and 1.3e-14 (d/dinit_mean, largest
7.97); 1e3 times that is at most 5.7e-11, so the floor, 1e-9 relative (1.4e-8, 1.8e-8, 8.0e-9), is
the bound in force for all three.

Largest errors measured on an MI355X: DESIGN.md section 4, "Soft resampling: the backward pass".
"""

import numpy as np
import pytest
import torch

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_soft as SO
from particle_filters_amd import dpf_soft_torch as ST
from tests import dpf_soft_grad_restatement as GR
from tests import dpf_soft_restatement as R
from tests import test_gpu_dpf_soft as TS

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert NV.device_count() > 0, "no HIP device visible: -m gpu tests must run on an MI355X"


def forward(h, X, lw, alpha, T, seed=0, epoch=0, batch_base=0):
    """(X_out, row_max, row_sum) of one pf_soft_resample on handle h."""
    out, _ = TS.call(h, X, lw, alpha, T, seed, epoch, batch_base, want_entropy=False)
    return (out,) + h.row_stats()


def backward(h, X, lw, g, alpha, T, seed=0, epoch=0, batch_base=0, saved=None):
    """(grad_X [B][N][d], grad_log_probs [B][N]) of one pf_soft_backward on handle h."""
    Xb, lwb = TS._batched(X, lw)
    gb = np.ascontiguousarray(g, dtype=float).reshape(Xb.shape)
    return h.backward(Xb, TS.lp_of(lwb, alpha), T, gb, seed, epoch, batch_base, saved)


def fresh(fn, X, *args, **kw):
    Xb = np.asarray(X)
    Xb = Xb if Xb.ndim == 3 else Xb[None]
    h = SO._Handle(Xb.shape[1], Xb.shape[2], Xb.shape[0])
    try:
        return fn(h, X, *args, **kw)
    finally:
        h.close()


def compare(tag, gX, glw, ref):
    assert np.all(np.isfinite(gX)) and np.all(np.isfinite(glw))
    sx, sc = max(1.0, float(np.max(np.abs(ref["gX"])))), ref["sc"]
    ex = float(np.max(np.abs(gX - ref["gX"])))
    ew = float(np.max(np.abs(glw - ref["glw"])))
    print(f"soft grad {tag}: gX error {ex:.3e} (scale {sx:.3g}, {ex / sx:.2e} rel), g log_weights error {ew:.3e} "
          f"(sc {sc:.3g}, {ew / sc:.2e} rel, max|ref| {np.max(np.abs(ref['glw'])):.3e})")
    assert ex <= TOL * sx
    assert ew <= TOL * sc


# ------------------------------------------------------------------ a. parity
@pytest.mark.parametrize("case", R.PARITY, ids=lambda c: f"N{c[0]}-d{c[1]}-a{c[2]}-T{c[3]}-{c[4]}")
def test_parity(case):
    N, d, alpha, T, kind, seed, epoch = case
    ref = GR.autograd(*case)
    if alpha < 1.0 and N >= 2:
        assert float(np.max(np.abs(ref["glw"]))) > 1e-3 * ref["sc"]
    assert float(np.max(np.abs(ref["gX"]))) > 1e-3
    gX, glw = SO.soft_resample_vjp(ref["X"], ref["lw"], ref["gXo"], alpha, T, seed=seed, epoch=epoch)
    assert gX.dtype == np.float64 and gX.shape == (N, d) and glw.shape == (N,)
    compare(f"N={N} d={d} alpha={alpha} T={T} {kind}", gX, glw, ref)
    if alpha == 1.0:
        assert np.all(glw == 0.0)
    # the saved results of the forward call give the same bits as running the forward again
    out, nlw, saved = SO.soft_resample(ref["X"], ref["lw"], alpha, T, seed=seed, epoch=epoch, return_saved=True)
    assert isinstance(saved, SO.SoftSaved) and saved.X_out.shape == (1, N, d) and saved.row_max.shape == (1, N)
    assert np.array_equal(saved.X_out[0], out) and (saved.seed, saved.epoch) == (seed, epoch)
    gX2, glw2 = SO.soft_resample_vjp(ref["X"], ref["lw"], ref["gXo"], alpha, T, seed=seed, epoch=epoch, saved=saved)
    assert np.array_equal(gX2, gX) and np.array_equal(glw2, glw)


def test_a_minus_inf_log_weight_gets_exactly_zero_on_the_device():
    N, d = 65, 5
    X, lw = R.make_case(N, d, seed=2)
    lw = lw.copy()
    lw[[0, 64]] = -np.inf
    gX, glw = SO.soft_resample_vjp(X, lw, GR.grad_out(N, d), 0.1, 0.2, seed=4, epoch=1)
    assert glw[0] == 0.0 and glw[64] == 0.0 and np.all(np.isfinite(glw)) and np.all(np.isfinite(gX))
    assert np.array_equal(glw == 0.0, np.isinf(lw))


# ------------------------------------------------------------------ b. forced splits
@pytest.mark.parametrize("splits", ["1", "2", "3"])
def test_forced_splits(splits, monkeypatch):
    N, d, alpha, T, seed, epoch = 300, 17, 0.1, 0.2, 21, 1
    ref = GR.autograd(N, d, alpha, T, "normal", seed, epoch)
    monkeypatch.delenv("PF_TEST_SOFT_SPLITS", raising=False)
    plain = SO.soft_resample_vjp(ref["X"], ref["lw"], ref["gXo"], alpha, T, seed=seed, epoch=epoch)
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_SOFT_SPLITS", splits)
    gX, glw = SO.soft_resample_vjp(ref["X"], ref["lw"], ref["gXo"], alpha, T, seed=seed, epoch=epoch)
    again = SO.soft_resample_vjp(ref["X"], ref["lw"], ref["gXo"], alpha, T, seed=seed, epoch=epoch)
    compare(f"N={N} d={d} PF_TEST_SOFT_SPLITS={splits}", gX, glw, ref)
    compare(f"N={N} d={d} unhooked", plain[0], plain[1], ref)
    assert np.array_equal(again[0], gX) and np.array_equal(again[1], glw)
    assert not np.array_equal(gX, plain[0])  # the hook took effect: another summation order


# ------------------------------------------------------------------ c. bitwise properties
BATCH = dict(N=130, d=17, alpha=0.1, T=0.2, seed=31, epoch=2)  # two component chunks, five splits


def _batch_inputs():
    c = BATCH
    X, lw = TS._batch_inputs()
    g = np.stack([np.random.default_rng([c["N"], c["d"], 99, b]).standard_normal((c["N"], c["d"])) for b in range(3)])
    return X, lw, g


def test_equal_calls_are_bitwise_equal():
    c = BATCH
    X, lw, g = _batch_inputs()
    a = fresh(backward, X, lw, g, c["alpha"], c["T"], c["seed"], c["epoch"])
    b = fresh(backward, X, lw, g, c["alpha"], c["T"], c["seed"], c["epoch"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    other = fresh(backward, X, lw, g, c["alpha"], c["T"], c["seed"], c["epoch"] + 1)
    assert not np.array_equal(a[0], other[0])


def test_a_batch_is_bitwise_the_problems_alone():
    c = BATCH
    X, lw, g = _batch_inputs()
    gX, glp = fresh(backward, X, lw, g, c["alpha"], c["T"], c["seed"], c["epoch"])
    for b in range(3):
        g1, l1 = fresh(backward, X[b], lw[b], g[b], c["alpha"], c["T"], c["seed"], c["epoch"], batch_base=b)
        assert np.array_equal(g1[0], gX[b]) and np.array_equal(l1[0], glp[b]), f"problem {b}"
    g0, _ = fresh(backward, X[1], lw[1], g[1], c["alpha"], c["T"], c["seed"], c["epoch"])
    assert not np.array_equal(g0[0], gX[1])  # problem 1 with the draws of problem 0
    # and the batch through the public function against the reference, problem by problem
    gXp, glw = SO.soft_resample_vjp(X, lw, g, c["alpha"], c["T"], seed=c["seed"], epoch=c["epoch"])
    assert np.array_equal(gXp, gX)
    for b in range(3):
        res = R.soft_resample(X[b], lw[b], c["alpha"], c["T"], c["seed"], c["epoch"], b)
        cf = GR.closed_form(X[b], lw[b], g[b], c["alpha"], c["T"], res["A"])
        ref = {"gX": cf["gX"], "glw": cf["glw_pairs"], "sc": GR.scale(X[b], g[b], c["T"], res["A"])}
        compare(f"batch problem {b}", gXp[b], glw[b], ref)


def test_saved_results_give_the_bits_of_recomputed_ones():
    c = BATCH
    X, lw, g = _batch_inputs()
    null = fresh(backward, X, lw, g, c["alpha"], c["T"], c["seed"], c["epoch"])
    saved = fresh(forward, X, lw, c["alpha"], c["T"], c["seed"], c["epoch"])
    got = fresh(backward, X, lw, g, c["alpha"], c["T"], c["seed"], c["epoch"], saved=saved)
    assert np.array_equal(got[0], null[0]) and np.array_equal(got[1], null[1])


def test_a_reused_handle_gives_the_bits_of_fresh_ones():
    c = BATCH
    X, lw, g = _batch_inputs()
    calls = [  # (X, lw, g, alpha, T, seed, epoch)
        (X[0], lw[0], g[0], 0.1, 0.2, 1, 0),
        (X[1], lw[1], g[1], 0.0, 1.0, 2, 5),
        (X[0] + 30.0, lw[2], g[2], 1.0, 0.2, 1 << 40, 0),
        (X[0], lw[0], g[0], 0.1, 0.2, 1, 0),   # the first call again
        (X[2], lw[0], 100.0 * g[1], 0.5, 5.0, 4, 0xFFFFFFFF),
    ]
    h = SO._Handle(c["N"], c["d"], 1)
    try:
        got = [backward(h, *a) for a in calls]
    finally:
        h.close()
    for k, a in enumerate(calls):
        want = fresh(backward, *a)
        assert np.array_equal(got[k][0], want[0]) and np.array_equal(got[k][1], want[1]), f"call {k}"
    assert np.array_equal(got[0][0], got[3][0]) and np.array_equal(got[0][1], got[3][1])


def test_row_stats_need_a_forward_pass_and_the_saved_results_come_all_or_none():
    lib = NV.load()
    h = SO._Handle(4, 2, 2)
    try:
        M, L = np.zeros((2, 4)), np.zeros((2, 4))
        assert lib.pf_soft_row_stats(h.h, NV.dptr(M), NV.dptr(L)) == NV.PF_E_ARG  # nothing has run yet
        X, lp, g = np.ones((2, 4, 2)), np.zeros((2, 4)), np.ones((2, 4, 2))
        Xo, gX, glp = np.zeros((2, 4, 2)), np.zeros((2, 4, 2)), np.zeros((2, 4))
        assert lib.pf_soft_resample(h.h, NV.dptr(X), NV.dptr(lp), 0.2, 0, 0, 0, NV.dptr(Xo), None) == NV.PF_OK
        assert lib.pf_soft_row_stats(h.h, NV.dptr(M), NV.dptr(L)) == NV.PF_OK
        assert np.all(np.isfinite(M)) and np.all(L >= 1.0) and np.all(L <= 4.0)
        assert lib.pf_soft_row_stats(h.h, None, NV.dptr(L)) == NV.PF_E_ARG
        a = (h.h, NV.dptr(X), NV.dptr(lp))
        o = (NV.dptr(g), NV.dptr(gX), NV.dptr(glp))
        ok = lib.pf_soft_backward(*a, 0.2, 0, 0, 0, NV.dptr(Xo), NV.dptr(M), NV.dptr(L), *o)
        assert ok == NV.PF_OK and np.all(np.isfinite(gX)) and np.all(np.isfinite(glp))
        assert lib.pf_soft_backward(*a, 0.2, 0, 0, 0, None, None, None, *o) == NV.PF_OK
        for sv in ((NV.dptr(Xo), None, None), (None, NV.dptr(M), NV.dptr(L)), (NV.dptr(Xo), NV.dptr(M), None)):
            assert lib.pf_soft_backward(*a, 0.2, 0, 0, 0, *sv, *o) == NV.PF_E_ARG
        for T in (0.0, -1.0, float("inf"), float("nan")):
            assert lib.pf_soft_backward(*a, T, 0, 0, 0, None, None, None, *o) == NV.PF_E_ARG
        assert lib.pf_soft_backward(*a, 0.2, 0, 0, (1 << 24) - 1, None, None, None, *o) == NV.PF_E_ARG
        assert lib.pf_soft_backward(*a, 0.2, 0, 0, 0, None, None, None, None, o[1], o[2]) == NV.PF_E_ARG
        assert lib.pf_soft_backward(*a, 0.2, 0, 0, 0, None, None, None, o[0], None, o[2]) == NV.PF_E_ARG
        assert lib.pf_soft_backward(*a, 0.2, 0, 0, 0, None, None, None, o[0], o[1], None) == NV.PF_E_ARG
        assert lib.pf_soft_backward(None, a[1], a[2], 0.2, 0, 0, 0, None, None, None, *o) == NV.PF_E_ARG
    finally:
        h.close()
    # equal particles and a constant upstream gradient: gX sums to the upstream total, glp is 0
    assert np.allclose(gX.sum(axis=1), 4.0, rtol=0, atol=1e-12) and np.max(np.abs(glp)) <= 1e-12


# ------------------------------------------------------------------ d. BPTT order
def test_backwards_in_reverse_order_on_one_handle_are_the_fresh_ones():
    """Three forwards with different inputs and epochs on one handle, then the three backwards in
    reverse order with each forward's saved results: the row statistics in the handle are those of
    the last forward, and a backward that read them instead of its own would be wrong for the
    first two."""
    c = BATCH
    X, lw, g = _batch_inputs()
    steps = [(X[t], lw[t], g[t], 0.1, 0.2, 7, t) for t in range(3)]
    h = SO._Handle(c["N"], c["d"], 1)
    try:
        saved = [forward(h, x, w, a, T, s, e) for x, w, _, a, T, s, e in steps]
        assert not np.array_equal(saved[0][1], saved[2][1])
        got = {t: backward(h, *steps[t], saved=saved[t]) for t in (2, 1, 0)}
    finally:
        h.close()
    for t in range(3):
        want = fresh(backward, *steps[t])
        assert np.array_equal(got[t][0], want[0]) and np.array_equal(got[t][1], want[1]), f"step {t}"


# ------------------------------------------------------------------ e. the torch binding
def test_torch_gradients_are_the_vjps_bits():
    N, d, alpha, T, seed, epoch = 130, 17, 0.1, 0.2, 8, 3
    X, lw = R.make_case(N, d, seed=seed)
    Cw = GR.grad_out(N, d)
    x = torch.tensor(X, requires_grad=True)
    w = torch.tensor(lw, requires_grad=True)
    out, nlw = ST.soft_resample(x, w, alpha, T, seed=seed, epoch=epoch)
    assert out.dtype == torch.float64 and out.shape == (N, d) and out.requires_grad and not nlw.requires_grad
    assert np.array_equal(nlw.numpy(), np.log(np.full(N, 1.0 / N)))
    want_out, _ = SO.soft_resample(X, lw, alpha, T, seed=seed, epoch=epoch)
    assert np.array_equal(out.detach().numpy(), want_out)
    (out * torch.from_numpy(Cw)).sum().backward()
    gX, glw = SO.soft_resample_vjp(X, lw, Cw, alpha, T, seed=seed, epoch=epoch)
    assert np.array_equal(x.grad.numpy(), gX) and np.array_equal(w.grad.numpy(), glw)
    # a batch, and only one input requiring grad
    Xb, lwb = TS._batch_inputs()
    xb = torch.tensor(Xb, requires_grad=True)
    outb, _ = ST.soft_resample(xb, torch.tensor(lwb), alpha, T, seed=seed, epoch=epoch)
    outb.sum().backward()
    gXb, _ = SO.soft_resample_vjp(Xb, lwb, np.ones_like(Xb), alpha, T, seed=seed, epoch=epoch)
    assert np.array_equal(xb.grad.numpy(), gXb)


def test_torch_double_backward_raises():
    X, lw = R.make_case(5, 2, seed=1)
    x = torch.tensor(X, requires_grad=True)
    out, _ = ST.soft_resample(x, torch.tensor(lw), 0.1, 0.2, seed=1)
    (gx,) = torch.autograd.grad(out.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_torch_tensors_on_the_device_give_the_same_bits():
    assert torch.cuda.is_available()
    N, d = 65, 3
    X, lw = R.make_case(N, d, seed=4)
    grads = []
    for dev in ("cpu", "cuda"):
        x = torch.tensor(X, device=dev, requires_grad=True)
        w = torch.tensor(lw, device=dev, requires_grad=True)
        out, nlw = ST.soft_resample(x, w, 0.1, 0.2, seed=9, epoch=1)
        assert out.device.type == dev and nlw.device.type == dev
        (out ** 2).sum().backward()
        assert x.grad.device.type == dev and w.grad.device.type == dev
        grads.append((x.grad.cpu().numpy(), w.grad.cpu().numpy()))
    assert np.array_equal(grads[0][0], grads[1][0]) and np.array_equal(grads[0][1], grads[1][1])


def test_whole_filter_gradients_against_the_cpu_filter():
    c = GR.FILTER
    data = GR.filter_data()
    B, N, d, T = c["B"], c["N"], c["d"], c["T"]
    a = torch.tensor(c["a"], dtype=torch.float64, requires_grad=True)
    sigma = torch.tensor(c["sigma"], dtype=torch.float64, requires_grad=True)
    mean = torch.zeros(d, dtype=torch.float64, requires_grad=True)
    tf_, lf_ = GR.model(a, sigma, torch.from_numpy(data["eps"]), c["sigma_r"])
    flt = ST.DifferentiableParticleFilter(N, d, tf_, lf_, c["alpha"], c["temp"], seed=c["seed"],
                                          rng=np.random.default_rng(c["rng"]))
    try:
        ps, lws = flt.filter(torch.from_numpy(data["obs"]), mean, torch.eye(d, dtype=torch.float64))
        assert ps.shape == (B, T + 1, N, d) and lws.shape == (B, T + 1, N) and flt.epoch == T
        loss = GR.loss_of(ps, lws, torch.from_numpy(data["targets"]))
        loss.backward()
    finally:
        flt.close()
    ref = GR.cpu_filter_grads(reverse=False)
    rev = GR.cpu_filter_grads(reverse=True)
    assert abs(float(loss.detach()) - ref[0]) <= TOL * max(1.0, abs(ref[0]))
    got = (float(a.grad), float(sigma.grad), mean.grad.numpy())
    for name, g, r, v in zip(("d loss/da", "d loss/dsigma", "d loss/dinit_mean"), got, ref[1:], rev[1:]):
        size = float(np.max(np.abs(r)))
        sens = float(np.max(np.abs(np.asarray(r) - np.asarray(v))))
        bound = max(1e3 * sens, 1e-9 * size)
        err = float(np.max(np.abs(np.asarray(g) - np.asarray(r))))
        print(f"soft filter {name}: reference {np.asarray(r)}, error {err:.3e}, CPU order sensitivity {sens:.3e}, "
              f"bound {bound:.3e}")
        assert size > 1e-3  # a gradient that is there
        assert err <= bound
