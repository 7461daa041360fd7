"""Vectorised fp64 NumPy restatement of the reference's Sinkhorn OT resampler.

``models/DPF_OT_resampling.py:119-234`` (cited "ot.py:LINE") runs every half-iteration as a Python
loop of ``tau_epsilon`` calls, one per row or column of the cost matrix.  Here each half-iteration is
one (N, N) expression with the same arithmetic per entry: the exponent ``(f - C) / eps``, its
maximum, ``a * exp(exponent - max)`` summed, ``-eps * (log(max(sum, min_val)) + max)``.  Only the
order of the sums differs (NumPy's pairwise reduction along an axis against the reduction of a
1-D vector), which ``tests/test_dpf_ot_host.py`` bounds against :func:`loop_resample`, the literal
per-row transcription.

Arithmetic is fp64 throughout (the reference casts to float32; TensorFlow is not available, so the
device code is pinned to these formulas, not to reference outputs).
"""

import functools

import numpy as np

from particle_filters_amd.dpf_ot import pairwise_squared_distances, tau_epsilon


def make_case(N, d, scale=1.0, conc=1.0, seed=0):
    """X = scale * standard normal (N, d); weights = softmax of conc * standard normal."""
    rng = np.random.default_rng([seed, N, d])
    X = scale * rng.standard_normal((N, d))
    lw = conc * rng.standard_normal(N)
    w = np.exp(lw - lw.max())
    return X, w / w.sum()


def prepare(particles, weights, min_val):
    """ot.py:119-139: floored and normalised weights a, uniform b, cost C."""
    X = np.asarray(particles, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    N = X.shape[0]
    w = np.maximum(w, min_val)
    a = w / (np.sum(w) + min_val)
    b = np.full(N, 1.0 / float(N))
    C = pairwise_squared_distances(X, X)
    return X, a, b, C


def finish(X, a, b, C, f, g, epsilon, min_val, n_iters, iterations, history):
    """ot.py:184-232: plan, barycentric projection and diagnostics."""
    N = X.shape[0]
    P = a[:, None] * b[None, :] * np.exp((f[:, None] + g[None, :] - C) / epsilon)
    P = np.maximum(P, min_val)
    new = (P.T @ X) / b[:, None]
    diag = {
        "sinkhorn_iterations": iterations,
        "converged": iterations < n_iters,
        "ot_distance": float(np.sum(P * C)),
        "transport_plan_sparsity": float(np.sum(P > 1e-6)) / float(N * N),
        "dual_variables": {"f_mean": float(np.mean(f)), "f_std": float(np.std(f)),
                           "g_mean": float(np.mean(g)), "g_std": float(np.std(g))},
        "convergence_history": history,
        "epsilon": epsilon,
    }
    return dict(particles=new, weights=b, diagnostics=diag, f=f, g=g, P=P, C=C, a=a, iterations=iterations)


def _tau_rows(m, h, C, epsilon, min_val):
    """Tau(m, h, C[i, :]) for every i: the reduced index is the second one."""
    e = (h[None, :] - C) / epsilon
    mx = np.max(e, axis=1)
    s = np.sum(m[None, :] * np.exp(e - mx[:, None]), axis=1)
    return -epsilon * (np.log(np.maximum(s, min_val)) + mx)


def _tau_cols(m, h, C, epsilon, min_val):
    """Tau(m, h, C[:, j]) for every j: the reduced index is the first one."""
    e = (h[:, None] - C) / epsilon
    mx = np.max(e, axis=0)
    s = np.sum(m[:, None] * np.exp(e - mx[None, :]), axis=0)
    return -epsilon * (np.log(np.maximum(s, min_val)) + mx)


def sinkhorn_resample(particles, weights, epsilon=0.1, n_iters=50, min_val=1e-12, tol=1e-6):
    """The whole of ot.py:119-232 in fp64; returns the dict of :func:`finish`."""
    X, a, b, C = prepare(particles, weights, min_val)
    N = X.shape[0]
    f = np.zeros(N)
    g = np.zeros(N)
    iterations = 0
    history = []
    for it in range(n_iters):
        f_old, g_old = f, g
        f = 0.5 * (f + _tau_rows(b, g, C, epsilon, min_val))
        g = 0.5 * (g + _tau_cols(a, f, C, epsilon, min_val))
        iterations = it + 1
        if it > 0:
            fc = float(np.max(np.abs(f - f_old)))
            gc = float(np.max(np.abs(g - g_old)))
            history.append({"iteration": it, "f_change": fc, "g_change": gc})
            if fc < tol and gc < tol:
                break
    return finish(X, a, b, C, f, g, epsilon, min_val, n_iters, iterations, history)


def loop_resample(particles, weights, epsilon=0.1, n_iters=50, min_val=1e-12, tol=1e-6):
    """Literal transcription of the per-row loop of ot.py:146-181: tau_epsilon once per i and per j."""
    X, a, b, C = prepare(particles, weights, min_val)
    N = X.shape[0]
    f = np.zeros(N)
    g = np.zeros(N)
    iterations = 0
    history = []
    for it in range(n_iters):
        f_old, g_old = f, g
        f_new = np.empty(N)
        for i in range(N):
            f_new[i] = 0.5 * (f[i] + tau_epsilon(b, g, C[i, :], epsilon, min_val))
        f = f_new
        g_new = np.empty(N)
        for j in range(N):
            g_new[j] = 0.5 * (g[j] + tau_epsilon(a, f, C[:, j], epsilon, min_val))
        g = g_new
        iterations = it + 1
        if it > 0:
            fc = float(np.max(np.abs(f - f_old)))
            gc = float(np.max(np.abs(g - g_old)))
            history.append({"iteration": it, "f_change": fc, "g_change": gc})
            if fc < tol and gc < tol:
                break
    return finish(X, a, b, C, f, g, epsilon, min_val, n_iters, iterations, history)


def resample_fn(particles, weights, epsilon=0.1, n_iters=50, min_val=1e-12, tol=1e-6, return_diagnostics=False,
                **_):
    """The restatement with the call shape of ``dpf_ot.sinkhorn_ot_resample`` (a stub resampler)."""
    r = sinkhorn_resample(particles, weights, epsilon, n_iters, min_val, tol)
    if return_diagnostics:
        return r["particles"], r["weights"], r["diagnostics"]
    return r["particles"], r["weights"]


# The cases of tests/test_gpu_dpf_ot.py; tests/test_dpf_ot_host.py asserts on the CPU what the GPU
# tests rely on (the stopping iterations and their margins, the sparsity margin).
# N, d, eps, n_iters, seed: full-length runs.  (1, 2) stops at 2 (nothing changes) and (2, 1), with
# this seed, at iteration 32; the others run all their iterations.
FULL = [(1, 2, 0.1, 50, 0), (2, 1, 0.1, 50, 224), (65, 1, 0.1, 50, 0), (130, 3, 0.1, 50, 0), (257, 5, 0.5, 100, 0),
        (300, 40, 2.0, 50, 0), (513, 16, 1.0, 50, 0)]
FULL_STOPS = {(1, 2): 2, (2, 1): 32}
# N, d, eps, scale, conc, seed, the iteration at which the restatement stops (n_iters = 500)
EARLY = [(130, 3, 0.1, 0.2, 1.0, 45, 29), (257, 2, 0.1, 0.1, 2.0, 2, 18), (96, 1, 0.5, 0.3, 1.0, 16, 22)]
EARLY_ITERS = 500
# (N, d, eps, n_iters, scale, conc, seed) of the diagnostics comparisons
DIAG = [(130, 3, 0.1, 50, 1.0, 1.0, 0), (300, 40, 2.0, 50, 1.0, 1.0, 0), (130, 3, 0.1, 500, 0.2, 1.0, 45),
        (96, 1, 0.5, 500, 0.3, 1.0, 16)]


@functools.lru_cache(maxsize=None)
def solved(N, d, eps, n_iters, scale=1.0, conc=1.0, seed=0):
    """(X, w, restatement result) of one case, computed once per process; treat it as read-only."""
    X, w = make_case(N, d, scale, conc, seed)
    return X, w, sinkhorn_resample(X, w, eps, n_iters)


WEIGHT_KINDS = ("unnormalised", "zeros", "peaked")


def weight_case(kind, N=130, d=3, seed=7):
    """Weights the normalisation of ot.py:127-128 has to deal with, on one particle set."""
    X, w = make_case(N, d, seed=seed)
    if kind == "unnormalised":
        w = 37.5 * w
    elif kind == "zeros":
        w = w.copy()
        w[::3] = 0.0
    elif kind == "peaked":  # one weight of 1 - 1e-9
        w = np.full(N, 1e-9 / (N - 1))
        w[5] = 1.0 - 1e-9
    else:
        raise ValueError(kind)
    return X, w


@functools.lru_cache(maxsize=None)
def solved_weights(kind):
    X, w = weight_case(kind)
    return X, w, sinkhorn_resample(X, w, 0.1, 50)


# three problems of one shape that stop at different iterations (the batch test): EARLY[0]'s
# parameters under three seeds -> (seed, stopping iteration)
BATCH = dict(N=130, d=3, eps=0.1, scale=0.2, conc=1.0, seeds=((45, 29), (1, 38), (3, 32)))
# the source-split case: 25 MB of C, large enough that the source range is split
SPLIT = (2500, 2, 0.1, 3, 1.0, 1.0, 0)
