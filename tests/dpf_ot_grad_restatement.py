"""Backward pass of the Sinkhorn OT resampler on the CPU - TEST INFRASTRUCTURE ONLY.

Two independent statements of the gradient of ``sinkhorn_resample`` (tests/dpf_ot_restatement.py)
with respect to the particles X (N, d) and the weights w (N,), given the gradient G (N, d) of a
scalar with respect to the new particles:

* ``torch_forward``: the literal forward (floor and normalise the weights, the cost by the
  expansion clamped at 0, K damped iterations of the two Tau passes with ``amax`` for the maximum
  and ``clamp`` for the floor, the floored plan, the projection) in PyTorch CPU fp64 with K fixed,
  whose autograd is the reference (``autograd``): what ``tf.GradientTape`` forms in the reference;
* ``closed_form``: the five steps the device implements (projection, the g and f passes of every
  iteration in reverse, the cost, the weights), in NumPy with stored (N, N) matrices.

Also the whole ``DPF_OT`` filter in torch on the CPU (``cpu_filter_grads``), which
tests/test_gpu_dpf_ot_grad.py compares the device-backed filter's gradients with.
"""

from __future__ import annotations

import numpy as np
import torch

from tests import dpf_ot_restatement as R

MIN_VAL = 1e-12


def grad_out(N, d):
    """The incoming gradient of a case."""
    return np.random.default_rng([N, d, 99]).standard_normal((N, d))


def torch_forward(X, w, eps, K, min_val=MIN_VAL, reverse=False):
    """The literal forward on tensors X (N, d), w (N,) -> new particles (N, d), K iterations.  With
    ``reverse`` every Tau sum visits its terms in the opposite order (another rounding of the same
    sums)."""
    N = X.shape[0]
    wt = torch.maximum(w, torch.tensor(min_val, dtype=torch.float64))
    a = wt / (wt.sum() + min_val)
    b = torch.full((N,), 1.0 / N, dtype=torch.float64)
    x2 = (X * X).sum(1, keepdim=True)
    C = torch.clamp(x2 - 2.0 * X @ X.T + x2.T, min=0.0)
    f = torch.zeros(N, dtype=torch.float64)
    g = torch.zeros(N, dtype=torch.float64)

    def tau(mass, h, dim):
        e = (h - C) / eps
        mx = e.amax(dim=dim, keepdim=True)
        t = mass * torch.exp(e - mx)
        if reverse:
            t = t.flip(dim)
        return -eps * (torch.log(torch.clamp(t.sum(dim=dim), min=min_val)) + mx.squeeze(dim))

    for _ in range(K):
        f = 0.5 * (f + tau(b[None, :], g[None, :], 1))
        g = 0.5 * (g + tau(a[:, None], f[:, None], 0))
    P = torch.clamp(a[:, None] * b[None, :] * torch.exp((f[:, None] + g[None, :] - C) / eps), min=min_val)
    return (P.T @ X) / b[:, None]


def closed_form(X, w, G, eps, K, min_val=MIN_VAL, info=None):
    """(gX, gw) by the five steps of the device, K iterations.  ``info``, a dict, receives what the
    well-posedness checks of tests/test_dpf_ot_grad_host.py look at."""
    X = np.asarray(X, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    N = X.shape[0]
    _, a, b, C = R.prepare(X, w, min_val)
    F, Gd, TF, TG = [np.zeros(N)], [np.zeros(N)], [], []
    f, g = np.zeros(N), np.zeros(N)
    for _ in range(K):
        tf_ = R._tau_rows(b, g, C, eps, min_val)
        f = 0.5 * (f + tf_)
        tg_ = R._tau_cols(a, f, C, eps, min_val)
        g = 0.5 * (g + tg_)
        F.append(f), Gd.append(g), TF.append(tf_), TG.append(tg_)
    bN = 1.0 / N
    # 1. projection
    raw = a[:, None] * bN * np.exp((f[:, None] + g[None, :] - C) / eps)
    u = raw > min_val
    P = np.maximum(raw, min_val)
    q = N * (X @ G.T)
    gX = N * (P @ G)
    D = np.where(u, P * q, 0.0) / eps
    fb, gb, Cb = D.sum(1), D.sum(0), -D
    ab = eps * D.sum(1) / a
    plan_margin = float(np.min(np.abs(raw[u] / min_val - 1.0))) if np.any(u) else np.inf
    sum_margin, gap, floored = np.inf, np.inf, 0
    for k in range(K, 0, -1):
        # 2. the g pass
        t = 0.5 * gb
        gb = 0.5 * gb
        e = (F[k][:, None] - C) / eps
        mx = e.max(0)
        S = (a[:, None] * np.exp(e - mx[None, :])).sum(0)
        fl = S < min_val
        s = a[:, None] * np.exp((F[k][:, None] + TG[k - 1][None, :] - C) / eps)
        ind = np.zeros_like(s)
        ind[e.argmax(0), np.arange(N)] = 1.0
        s_sum = np.where(fl[None, :], 0.0, s)
        s_all = np.where(fl[None, :], ind, s)
        fb = fb - (s_all * t[None, :]).sum(1)
        ab = ab - eps * (s_sum * t[None, :]).sum(1) / a
        Cb = Cb + s_all * t[None, :]
        sum_margin = min(sum_margin, float(np.min(np.abs(S / min_val - 1.0))))
        floored += int(fl.sum())
        if np.any(fl) and N > 1:
            top = np.sort(e[:, fl], axis=0)
            gap = min(gap, float(np.min(top[-1] - top[-2])))
        # 3. the f pass
        t = 0.5 * fb
        fb = 0.5 * fb
        r = bN * np.exp((Gd[k - 1][None, :] + TF[k - 1][:, None] - C) / eps)
        gb = gb - (r * t[:, None]).sum(0)
        Cb = Cb + r * t[:, None]
    # 4. cost
    Cb = np.where(C == 0.0, 0.0, Cb)
    W = Cb + Cb.T
    gX = gX + 2.0 * (W.sum(1)[:, None] * X - W @ X)
    # 5. weights
    tot = np.maximum(w, min_val).sum() + min_val
    gw = np.where(w > min_val, (ab - np.sum(ab * a)) / tot, 0.0)
    if info is not None:
        off = ~np.eye(N, dtype=bool)
        info.update(plan_margin=plan_margin, sum_margin=sum_margin, argmax_gap=gap, floored_columns=floored,
                    zero_offdiag=int(np.sum(C[off] == 0.0)))
    return gX, gw


_cache = {}


def autograd(case):
    """dict(X, w, G, eps, n_iters, K, gX, gw, gX_rev, gw_rev) of a case ``(name, X, w, eps, n_iters)``: the
    autograd reference at the K iterations the restatement takes, in both summation orders, computed
    once per name; do not modify the arrays."""
    name, X, w, eps, n_iters = case
    if name in _cache:
        return _cache[name]
    res = R.sinkhorn_resample(X, w, eps, n_iters)
    K = int(res["iterations"])
    N, d = X.shape
    G = grad_out(N, d)
    grads = []
    for reverse in (False, True):
        Xt = torch.tensor(X, dtype=torch.float64, requires_grad=True)
        wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
        out = torch_forward(Xt, wt, eps, K, reverse=reverse)
        out.backward(torch.from_numpy(G))
        scale = max(1.0, float(np.max(np.abs(res["particles"]))))
        assert float(np.max(np.abs(out.detach().numpy() - res["particles"]))) <= 1e-12 * scale, name
        grads.append((Xt.grad.numpy().copy(), wt.grad.numpy().copy()))
    ref = {"X": np.array(X), "w": np.array(w), "G": G, "eps": eps, "n_iters": n_iters, "K": K,
           "gX": grads[0][0], "gw": grads[0][1], "gX_rev": grads[1][0], "gw_rev": grads[1][1]}
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[name] = ref
    return ref


def cases():
    """The parity cases of tests/test_gpu_dpf_ot_grad.py as (name, X, w, eps, n_iters)."""
    out = []
    for N, d, eps, n_iters in [(1, 2, 0.1, 50), (2, 1, 0.1, 50), (65, 1, 0.1, 50), (130, 3, 0.1, 50), (257, 5, 0.5, 100),
                               (300, 40, 2.0, 50), (70, 65, 4.0, 50), (97, 64, 4.0, 50), (130, 3, 0.1, 0),
                               (130, 3, 0.1, 1)]:
        seed = {c[:2]: c[4] for c in R.FULL}[(N, d)]
        out.append((f"N{N}-d{d}-eps{eps}-it{n_iters}", *R.make_case(N, d, seed=seed), eps, n_iters))
    N, d, eps, scale, conc, seed, _ = R.EARLY[0]
    out.append(("early", *R.make_case(N, d, scale, conc, seed), eps, R.EARLY_ITERS))
    for kind in ("unnormalised", "zeros"):
        out.append((kind, *R.weight_case(kind), 0.1, 50))
    for name in ("sharp", "floor eps=0.05"):
        out.append((name, *R.edge_case(name)))
    N, d, eps, n_iters, scale, conc, seed = R.SPLIT
    out.append(("split", *R.make_case(N, d, scale, conc, seed), eps, n_iters))
    return out


CASE_NAMES = [c[0] for c in cases()]
SMALL_SPLITS = "N300-d40-eps2.0-it50"  # the N = 300 case of the forced splits


def case(name):
    return next(c for c in cases() if c[0] == name)


# ------------------------------------------------------------------ the whole filter on the CPU
FILTER = dict(N=65, d=2, T=3, eps=0.1, iters=50, a=0.9, sigma=0.3, sigma_r=0.5, rng=41)


def filter_data():
    """Fixed inputs of the whole-filter test: process noise (T, N, d), observations (T, d), targets
    (T, d), the prior draw's noise (N, d) as ``default_rng(rng)`` gives it."""
    c = FILTER
    g = np.random.default_rng([c["N"], c["d"], c["T"]])
    return {"eps": g.standard_normal((c["T"], c["N"], c["d"])), "obs": g.standard_normal((c["T"], c["d"])),
            "targets": 0.5 * g.standard_normal((c["T"], c["d"])),
            "prior": np.random.default_rng(c["rng"]).standard_normal((c["N"], c["d"]))}


def model(a, sigma, eps, sigma_r):
    """transition_fn(x, t) = a x + sigma eps_t (eps fixed in advance) and a Gaussian log-likelihood, as
    torch callables on (N, d)."""

    def transition_fn(x, t):
        return a * x + sigma * eps[t]

    def obs_loglik_fn(x, y, t):
        return -0.5 * torch.sum((y[None, :] - x) ** 2, dim=-1) / sigma_r ** 2

    return transition_fn, obs_loglik_fn


def loss_of(particles_seq, weights_seq, targets):
    """sum over t of the squared error of the weighted mean against the targets."""
    means = torch.stack([torch.sum(w[:, None] * p, dim=0) for p, w in zip(particles_seq, weights_seq)])
    return torch.sum((means - targets) ** 2)


def cpu_filter_grads(reverse=False):
    """(loss, d loss / da, d loss / dsigma, d loss / dmean0 (d,), iterations per step) of the filter
    written entirely in torch on the CPU; every step runs the iterations the restatement takes on its
    inputs."""
    c = FILTER
    data = filter_data()
    N, d, T = c["N"], c["d"], c["T"]
    a = torch.tensor(c["a"], dtype=torch.float64, requires_grad=True)
    sigma = torch.tensor(c["sigma"], dtype=torch.float64, requires_grad=True)
    mean = torch.zeros(d, dtype=torch.float64, requires_grad=True)
    tf_, lf_ = model(a, sigma, torch.from_numpy(data["eps"]), c["sigma_r"])
    obs = torch.from_numpy(data["obs"])
    x = mean[None, :] + torch.from_numpy(data["prior"]) @ torch.eye(d, dtype=torch.float64).T
    w = torch.full((N,), 1.0 / N, dtype=torch.float64)
    xs, ws, its = [], [], []
    for t in range(T):
        pred = tf_(x, t)
        uw = torch.clamp(w * torch.exp(lf_(pred, obs[t], t)), min=0.0)
        nw = uw / (torch.sum(uw) + 1e-12)
        K = int(R.sinkhorn_resample(pred.detach().numpy(), nw.detach().numpy(), c["eps"], c["iters"])["iterations"])
        its.append(K)
        x = torch_forward(pred, nw, c["eps"], K, reverse=reverse)
        w = torch.full((N,), 1.0 / N, dtype=torch.float64)
        xs.append(x)
        ws.append(w)
    loss = loss_of(xs, ws, torch.from_numpy(data["targets"]))
    loss.backward()
    return float(loss.detach()), float(a.grad), float(sigma.grad), mean.grad.numpy().copy(), its
