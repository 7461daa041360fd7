"""Backward pass of the soft (Gumbel-Softmax) resampler on the CPU - TEST INFRASTRUCTURE ONLY.

Two independent statements of the gradient of ``soft_resample`` (tests/dpf_soft_restatement.py)
with respect to the particles X (N, d) and the unnormalised log-weights (N,), given the gradient
gX' (N, d) of a scalar with respect to the new particles:

* ``closed_form``: the formulas the device implements, in NumPy with the stored (N, N) matrix A:
  gX = A^T gX', r_i = gX'_i . X'_i, glp_j in both algebraically equal forms,
      "pairs":  (1 / T) sum_i a_ij (gX'_i . X_j - r_i)
      "sums":   (1 / T) (X_j . gX_j - sum_i a_ij r_i)        (the form the device uses)
  and the chain to the log-weights: gw = (1 - alpha) glp / (q + 1e-20), u = gw w,
  g log_weights = u - w sum(u);
* ``torch_forward``: the literal forward (normalise, mix with the uniform, log, add the Gumbels,
  divide by T, softmax, matrix product) in PyTorch CPU fp64 on the same draws, whose autograd is the
  reference (``autograd``).

``scale`` is the size of the terms every form of glp sums,
  sc = max(1, max_j sum_i a_ij (|gX'_i| . |X_j| + |r_i|) / T),
so the rounding of any summation order is bounded by a small multiple of N 2^-53 sc.

Also the whole filter in torch on the CPU with the restatement's draws (``cpu_filter_loss``), which
tests/test_gpu_dpf_soft_grad.py compares the device-backed filter's gradients with.
"""

from __future__ import annotations

import numpy as np
import torch

from tests import dpf_soft_restatement as R

OFFSET_CASE = (300, 16, 0.1, 0.2, "normal", 13, 0)  # run with make_case(..., offset=30)


def grad_out(N, d):
    """The incoming gradient of a case."""
    return np.random.default_rng([N, d, 99]).standard_normal((N, d))


def chain(lw, alpha, glp):
    """g log_weights (unnormalised) from g log_probs, one problem."""
    lw = np.asarray(lw, dtype=np.float64)
    N = lw.shape[-1]
    mx = np.max(lw)
    w = np.exp(lw - (mx + np.log(np.sum(np.exp(lw - mx)))))
    q = (1.0 - alpha) * w + alpha / N
    u = (1.0 - alpha) * glp / (q + 1e-20) * w
    return u - w * np.sum(u)


def closed_form(X, lw, gXo, alpha, T, A):
    """dict(gX, r, glp_pairs, glp_sums, glw_pairs, glw_sums) from the stored matrix A (N, N)."""
    X = np.asarray(X, dtype=np.float64)
    Xo = A @ X
    gX = A.T @ gXo
    r = np.sum(gXo * Xo, axis=-1)
    glp_pairs = np.sum(A * (gXo @ X.T - r[:, None]), axis=0) / T
    glp_sums = (np.sum(X * gX, axis=-1) - A.T @ r) / T
    return {"gX": gX, "r": r, "glp_pairs": glp_pairs, "glp_sums": glp_sums,
            "glw_pairs": chain(lw, alpha, glp_pairs), "glw_sums": chain(lw, alpha, glp_sums)}


def scale(X, gXo, T, A):
    Xo = A @ np.asarray(X, dtype=np.float64)
    r = np.sum(gXo * Xo, axis=-1)
    terms = A * (np.abs(gXo) @ np.abs(X).T + np.abs(r)[:, None])
    return max(1.0, float(np.max(np.sum(terms, axis=0))) / T)


def torch_forward(X, lw, alpha, T, G, reverse=False):
    """The literal forward on tensors X (N, d), lw (N,), G (N, N) -> new particles (N, d).  With
    ``reverse`` the sources are visited in the opposite order (another rounding of the same sums)."""
    N = X.shape[0]
    lwn = lw - torch.logsumexp(lw, dim=-1, keepdim=True)
    w = torch.exp(lwn)
    probs = (1.0 - alpha) * w + alpha * torch.full_like(w, 1.0 / N)
    lp = torch.log(probs + 1e-20)
    z = (lp[None, :] + G) / T
    if reverse:
        return torch.softmax(z.flip(-1), dim=-1) @ X.flip(0)
    return torch.softmax(z, dim=-1) @ X


_cache = {}


def autograd(N, d, alpha, T, kind, seed, epoch, offset=0.0):
    """dict(X, lw, gXo, gX, glw, sc, A) of a case: the autograd reference, computed once; do not
    modify the arrays."""
    key = (N, d, alpha, T, kind, seed, epoch, offset)
    if key in _cache:
        return _cache[key]
    if offset:
        X, lw = R.make_case(N, d, seed, offset=offset)
        res = R.soft_resample(X, lw, alpha, T, seed, epoch, 0)
    else:
        X, lw, res = R.solved(N, d, alpha, T, kind, seed, epoch)
    gXo = grad_out(N, d)
    Xt = torch.tensor(X, dtype=torch.float64, requires_grad=True)
    lwt = torch.tensor(lw, dtype=torch.float64, requires_grad=True)
    out = torch_forward(Xt, lwt, alpha, T, torch.from_numpy(res["G"]))
    out.backward(torch.from_numpy(gXo))
    assert float(np.max(np.abs(out.detach().numpy() - res["particles"]))) <= 1e-12 * max(1.0, float(np.max(np.abs(X))))
    ref = {"X": X, "lw": lw, "gXo": gXo, "gX": Xt.grad.numpy().copy(), "glw": lwt.grad.numpy().copy(),
           "sc": scale(X, gXo, T, res["A"]), "A": res["A"]}
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[key] = ref
    return ref


# ------------------------------------------------------------------ the whole filter on the CPU
FILTER = dict(B=2, N=65, d=2, T=3, alpha=0.1, temp=0.2, seed=23, a=0.9, sigma=0.3, sigma_r=0.5, rng=41)


def filter_data():
    """Fixed inputs of the whole-filter test: process noise eps (T, B, N, d), observations (B, T, d),
    targets (B, T + 1, d), the prior draw's noise (B, N, d) as ``default_rng(rng)`` gives it."""
    c = FILTER
    g = np.random.default_rng([c["B"], c["N"], c["d"], c["T"]])
    return {"eps": g.standard_normal((c["T"], c["B"], c["N"], c["d"])),
            "obs": g.standard_normal((c["B"], c["T"], c["d"])),
            "targets": 0.5 * g.standard_normal((c["B"], c["T"] + 1, c["d"])),
            "prior": np.random.default_rng(c["rng"]).standard_normal((c["B"], c["N"], c["d"]))}


def model(a, sigma, eps, sigma_r):
    """transition_fn(x) = a x + sigma eps_t (eps fixed in advance, one slice per call) and a Gaussian
    log-likelihood, as torch callables on (B, N, d)."""
    calls = iter(range(len(eps)))

    def transition_fn(x, params):
        return a * x + sigma * eps[next(calls)]

    def log_likelihood_fn(x, y, params):
        diff = y[:, None, :] - x
        return -0.5 * np.log(2.0 * np.pi * sigma_r ** 2) - 0.5 * torch.sum(diff ** 2, dim=-1) / sigma_r ** 2

    return transition_fn, log_likelihood_fn


def loss_of(particles_seq, logw_seq, targets):
    """sum over t of the squared error of the weighted mean against the targets."""
    w = torch.softmax(logw_seq, dim=-1)
    mean = torch.sum(w[..., None] * particles_seq, dim=2)
    return torch.sum((mean - targets) ** 2)


def cpu_filter_grads(reverse=False):
    """(loss, d loss / da, d loss / dsigma, d loss / dinit_mean (d,)) of the filter written entirely in
    torch on the CPU, the Gumbels those of the restatement for (seed, epoch = t, problem = b)."""
    c = FILTER
    data = filter_data()
    B, N, d, T = c["B"], c["N"], c["d"], c["T"]
    a = torch.tensor(c["a"], dtype=torch.float64, requires_grad=True)
    sigma = torch.tensor(c["sigma"], dtype=torch.float64, requires_grad=True)
    mean = torch.zeros(d, dtype=torch.float64, requires_grad=True)
    eps = torch.from_numpy(data["eps"])
    obs = torch.from_numpy(data["obs"])
    tf_, lf_ = model(a, sigma, eps, c["sigma_r"])
    x = mean[None, None, :] + torch.from_numpy(data["prior"]) @ torch.eye(d, dtype=torch.float64)
    logw = torch.full((B, N), float(np.log(1.0 / N)), dtype=torch.float64)
    xs, lws = [x], [logw]
    for t in range(T):
        pred = tf_(x, {})
        lw = logw + lf_(pred, obs[:, t, :], {})
        lw = lw - torch.logsumexp(lw, dim=-1, keepdim=True)
        x = torch.stack([torch_forward(pred[b], lw[b], c["alpha"], c["temp"],
                                       torch.from_numpy(R.draws(N, c["seed"], t, b)[1]), reverse) for b in range(B)])
        xs.append(x)
        lws.append(logw)
    loss = loss_of(torch.stack(xs, dim=1), torch.stack(lws, dim=1), torch.from_numpy(data["targets"]))
    loss.backward()
    return float(loss.detach()), float(a.grad), float(sigma.grad), mean.grad.numpy().copy()
