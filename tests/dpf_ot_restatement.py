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


def _tau_cols(m, h, C, epsilon, min_val, sums=None):
    """Tau(m, h, C[:, j]) for every j: the reduced index is the first one.  ``sums``, a list, receives
    the sums that the floor ``max(sum, min_val)`` is applied to."""
    e = (h[:, None] - C) / epsilon
    mx = np.max(e, axis=0)
    s = np.sum(m[:, None] * np.exp(e - mx[None, :]), axis=0)
    if sums is not None:
        sums.append(s)
    return -epsilon * (np.log(np.maximum(s, min_val)) + mx)


def sinkhorn_resample(particles, weights, epsilon=0.1, n_iters=50, min_val=1e-12, tol=1e-6, cost=None,
                      col_sums=None):
    """The whole of ot.py:119-232 in fp64; returns the dict of :func:`finish`.  ``cost`` replaces the
    cost matrix of ot.py:139 (:func:`exact_cost`); ``col_sums``, a list, receives the column sums of
    every g pass before their floor (the well-posedness checks of tests/test_dpf_ot_host.py)."""
    X, a, b, C = prepare(particles, weights, min_val)
    if cost is not None:
        C = cost
    N = X.shape[0]
    f = np.zeros(N)
    g = np.zeros(N)
    iterations = 0
    history = []
    for it in range(n_iters):
        f_old, g_old = f, g
        f = 0.5 * (f + _tau_rows(b, g, C, epsilon, min_val))
        g = 0.5 * (g + _tau_cols(a, f, C, epsilon, min_val, col_sums))
        iterations = it + 1
        if it > 0:
            fc = float(np.max(np.abs(f - f_old)))
            gc = float(np.max(np.abs(g - g_old)))
            history.append({"iteration": it, "f_change": fc, "g_change": gc})
            if fc < tol and gc < tol:
                break
    return finish(X, a, b, C, f, g, epsilon, min_val, n_iters, iterations, history)


def exact_cost(particles):
    """|x_i - x_j|^2 from the differences, formed in extended precision and rounded to fp64: the cost
    matrix without the cancellation of the expansion of ot.py:25-31."""
    X = np.asarray(particles, dtype=np.longdouble)
    D = X[:, None, :] - X[None, :, :]
    return np.asarray(np.sum(D * D, axis=-1), dtype=np.float64)


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
# the LDS stages of 64 components of k_ot_cost and the chunks of 16 of k_ot_project: d = 65 is a
# second stage of one component and five chunks, the last of one; d = 64 exactly one full stage
# and four full chunks; d = 130 stages of 64 + 64 + 2, nine chunks, the last of two, five splits
STAGES = [(70, 65, 4.0, 50, 0), (97, 64, 4.0, 50, 0), (130, 130, 8.0, 50, 0)]
FULL += STAGES
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
# The source-split case.  pf_ot_create splits the source range from N = 33 on (S = min(ceil(N / 32),
# 8192 / ceil(N / 64), 64), chunk = ceil(N / S) rounded up to 32), so every case above with N > 32 is
# split already; what this one adds is its size (25 MB of C, 40 column tiles) and chunks of more
# than 32 sources: S = 64 requested, chunk = 64, 40 splits of 64 sources (the last of 4).  With
# PF_TEST_OT_SPLITS=1 it is the one run whose tile loops take 2500 sources in tiles of 128 and 64.
SPLIT = (2500, 2, 0.1, 3, 1.0, 1.0, 0)

# (N, d, eps, n_iters, seed) of the runs that combine a source split with several LDS tiles per
# split (PF_TEST_OT_SPLITS = 2 and 3 at N = 300: chunks of 160 and 128 sources); the second adds the
# three component chunks of d = 40
TILES = [(300, 3, 0.1, 50, 0), (300, 40, 2.0, 50, 0)]

# a batch whose problems have three component chunks (d = 40) and five source splits (N = 130):
# seed per problem, and the problem whose weights get the zeros of weight_case("zeros")
CHUNK_BATCH = dict(N=130, d=40, eps=2.0, n_iters=50, seeds=(0, 1, 2), zeros=1)


@functools.lru_cache(maxsize=None)
def solved_chunk_batch(b):
    c = CHUNK_BATCH
    X, w = make_case(c["N"], c["d"], seed=c["seeds"][b])
    if b == c["zeros"]:
        w = w.copy()
        w[::3] = 0.0
    return X, w, sinkhorn_resample(X, w, c["eps"], c["n_iters"])


# (N, d, eps, n_iters, scale, conc, seed) of the calls without diagnostics
NODIAG = [(130, 3, 0.1, 50, 1.0, 1.0, 0), (300, 40, 2.0, 50, 1.0, 1.0, 0),
          (130, 3, 0.1, EARLY_ITERS, 0.2, 1.0, 45)]


def handle_sequence(batch=False):
    """The calls made one after the other on one handle: (tag, X, w, eps, n_iters).  An early stop,
    a full-length run, no iteration, one iteration, a longer history again, another eps.  With
    ``batch`` every call has three problems; those of the calls with 500 iterations stop at
    different iterations (BATCH)."""
    c = BATCH
    seeds = [s for s, _ in c["seeds"]]

    def pick(cases):
        X, w = zip(*cases)
        return (np.stack(X), np.stack(w)) if batch else (X[0], w[0])
    early = pick([make_case(c["N"], c["d"], c["scale"], c["conc"], s) for s in seeds])
    other = pick([make_case(c["N"], c["d"], c["scale"], c["conc"], s) for s in seeds[1:] + seeds[:1]])
    full = pick([make_case(c["N"], c["d"], seed=s) for s in (0, 1, 2)])
    return [("early stop", *early, c["eps"], EARLY_ITERS), ("full length", *full, 0.1, 50),
            ("no iteration", *full, 0.1, 0), ("one iteration", *full, 0.1, 1),
            ("early stop, other seed", *other, c["eps"], EARLY_ITERS), ("eps 0.5", *full, 0.5, 50)]


# Numerical edges: name -> (X, w, eps, n_iters).  tests/test_dpf_ot_host.py asserts for each what makes
# the comparison with the device well defined.
EDGES = ("floor eps=0.1", "floor eps=0.05", "far", "ten points", "one point", "sharp")
DUP_SEED = 0  # of the draw with repetition from ten points


def floor_particles():
    """weight_case("zeros") scaled by 37.5, with one particle of weight 0 far from the others: its
    column of the g pass sums to less than min_val, so the floor inside Tau binds."""
    X, w = weight_case("zeros")
    X, w = X.copy(), 37.5 * w
    X[129] = (-25.0, 10.0, 5.0)
    w[129] = 0.0
    return X, w


def edge_case(name):
    if name.startswith("floor eps="):
        return (*floor_particles(), float(name.split("=")[1]), 50)
    if name == "far":  # the expansion of |x_i - x_j|^2 cancels; the clamp at 0 acts on the diagonal
        X, w = make_case(130, 3, seed=0)
        return X + 30.0, w, 0.1, 50
    if name == "ten points":  # 130 rows drawn with repetition from 10 distinct points
        rng = np.random.default_rng([DUP_SEED, 130, 10])
        points = rng.standard_normal((10, 3))
        _, w = make_case(130, 3, seed=DUP_SEED)
        return points[rng.integers(0, 10, size=130)], w, 0.1, 50
    if name == "one point":  # every row the same: C = 0
        X, w = make_case(70, 3, seed=DUP_SEED)
        return np.tile(X[:1], (70, 1)), w, 0.1, 50
    if name == "sharp":  # almost the whole plan at the min_val floor
        return (*floor_particles(), 0.02, 50)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def solved_edge(name):
    X, w, eps, n_iters = edge_case(name)
    return X, w, eps, n_iters, sinkhorn_resample(X, w, eps, n_iters)


# (N, d, eps, n_iters, seed) of the permutation check (and the CHUNK_BATCH problems), with the seed
# of the permutation
PERMUTED = [(130, 3, 0.1, 50, 0), (300, 40, 2.0, 50, 0)]
PERMUTATION_SEED = 5
