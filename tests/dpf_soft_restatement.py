"""NumPy restatement of the soft (Gumbel-Softmax) resampler - TEST INFRASTRUCTURE ONLY.

The reference (models/DPF_soft_resampling.py, "soft.py") draws its N^2 Gumbels from TensorFlow's
global generator; the device draws them from Philox counters (include/pf_engine.h, the pf_soft_*
block).  This file restates

* the draw definition, from ``oracle.philox.philox4x32_10`` (which broadcasts counter arrays):
  counter (j >> 1, i, epoch, 5 + 256 problem), key (lo32(seed), hi32(seed)), even j takes the words
  (x, y), odd j (z, w) as (hi, lo), m = ((hi >> 6) << 26) | (lo >> 6), u = (2 m + 1) 2^-53,
  G = -log(-log(u));
* soft.py:306-334 (normalise, mix with the uniform, Gumbel-Softmax, barycentres) and 348-350 (row
  entropies) in fp64 with a stored (N, N) matrix: ``soft_resample``;
* the same as a literal loop over rows and sources with scalar arithmetic: ``loop_resample``, which
  tests/test_dpf_soft_host.py checks the vectorised form against;
* ``resample_fn``, a host resampler with the signature of
  ``DifferentiableParticleFilter._resample``, for the tests that swap the device call out.
"""

from __future__ import annotations

import math

import numpy as np

from oracle.philox import philox4x32_10

STREAM_GUMBEL = 5
TWO_M53 = 1.0 / 9007199254740992.0


def _key(seed: int):
    return int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF


def mantissas(rows, cols, seed=0, epoch=0, problem=0):
    """The 52-bit integers m of the draws at output rows ``rows`` x sources ``cols`` (uint64)."""
    i = np.asarray(rows, dtype=np.uint64)[:, None]
    j = np.asarray(cols, dtype=np.uint64)[None, :]
    k0, k1 = _key(seed)
    x, y, z, w = philox4x32_10(j >> np.uint64(1), i, int(epoch), STREAM_GUMBEL + 256 * int(problem), k0, k1)
    odd = (j & np.uint64(1)).astype(bool)
    odd = np.broadcast_to(odd, x.shape)
    hi = np.where(odd, z, x).astype(np.uint64)
    lo = np.where(odd, w, y).astype(np.uint64)
    return ((hi >> np.uint64(6)) << np.uint64(26)) | (lo >> np.uint64(6))


def uniforms(rows, cols, seed=0, epoch=0, problem=0):
    m = mantissas(rows, cols, seed, epoch, problem)
    return (np.uint64(2) * m + np.uint64(1)).astype(np.float64) * TWO_M53


def draws(N, seed=0, epoch=0, problem=0):
    """(U, G) of shape (N, N): row i, source j."""
    U = uniforms(np.arange(N), np.arange(N), seed, epoch, problem)
    return U, -np.log(-np.log(U))


def log_probs(log_weights, alpha):
    """soft.py:305-317 from unnormalised log-weights (last axis)."""
    lw = np.asarray(log_weights, dtype=np.float64)
    mx = np.max(lw, axis=-1, keepdims=True)
    lw = lw - (mx + np.log(np.sum(np.exp(lw - mx), axis=-1, keepdims=True)))
    w = np.exp(lw)
    N = lw.shape[-1]
    return np.log((1.0 - alpha) * w + alpha * np.full(w.shape, 1.0 / N) + 1e-20)


def assignment(lp, G, T):
    """softmax along the last axis of (lp_j + G_ij) / T, as tf.nn.softmax: (N, N)."""
    z = (lp[None, :] + G) / T
    e = np.exp(z - np.max(z, axis=-1, keepdims=True))
    return e / np.sum(e, axis=-1, keepdims=True)


def soft_resample(X, log_weights, alpha=0.1, T=0.2, seed=0, epoch=0, problem=0):
    """One problem (N, d): dict(particles, entropy (N,), A (N, N), log_probs, G, U)."""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    lp = log_probs(log_weights, alpha)
    U, G = draws(N, seed, epoch, problem)
    A = assignment(lp, G, T)
    return {"particles": A @ X, "entropy": -np.sum(A * np.log(A + 1e-10), axis=-1), "A": A, "log_probs": lp,
            "G": G, "U": U}


def loop_resample(X, log_weights, alpha=0.1, T=0.2, seed=0, epoch=0, problem=0):
    """The same, one row and one source at a time in scalar arithmetic."""
    X = np.asarray(X, dtype=np.float64)
    N, d = X.shape
    lw = [float(v) for v in np.asarray(log_weights, dtype=np.float64)]
    mx = max(lw)
    log_z = mx + math.log(sum(math.exp(v - mx) for v in lw))
    lp = [math.log((1.0 - alpha) * math.exp(v - log_z) + alpha * (1.0 / N) + 1e-20) for v in lw]
    k0, k1 = _key(seed)
    out = np.zeros((N, d))
    ent = np.zeros(N)
    for i in range(N):
        z = []
        for j in range(N):
            x, y, zz, w = (int(v) for v in philox4x32_10(j >> 1, i, int(epoch), STREAM_GUMBEL + 256 * int(problem),
                                                         k0, k1))
            hi, lo = (zz, w) if j & 1 else (x, y)
            m = ((hi >> 6) << 26) | (lo >> 6)
            u = (2 * m + 1) * TWO_M53
            z.append((lp[j] + -math.log(-math.log(u))) / T)
        zmax = max(z)
        e = [math.exp(v - zmax) for v in z]
        tot = sum(e)
        a = [v / tot for v in e]
        for k in range(d):
            out[i, k] = sum(a[j] * X[j, k] for j in range(N))
        ent[i] = -sum(v * math.log(v + 1e-10) for v in a)
    return {"particles": out, "entropy": ent, "log_probs": np.array(lp)}


def resample_fn(particles, log_weights, soft_alpha, gumbel_temperature, seed, epoch, want_entropy):
    """Host stand-in for ``DifferentiableParticleFilter._resample``: (B, N, d), (B, N) -> (new, H)."""
    X = np.asarray(particles, dtype=np.float64)
    res = [soft_resample(X[b], log_weights[b], soft_alpha, gumbel_temperature, seed, epoch, b)
           for b in range(X.shape[0])]
    new = np.stack([r["particles"] for r in res])
    return new, (np.stack([r["entropy"] for r in res]) if want_entropy else None)


# ------------------------------------------------------------------ cases shared by the tests
def make_case(N, d, seed=0, spread=3.0, offset=0.0):
    """Particles (N, d) and unnormalised log-weights (N,) whose range is ``spread`` standard deviations
    of a normal; ``spread = 0`` gives uniform weights."""
    rng = np.random.default_rng([N, d, seed])
    X = offset + rng.standard_normal((N, d))
    lw = spread * rng.standard_normal(N) - 1.7
    return X, lw


def dominant_case(N, d, seed=0):
    """``log w`` spread over 30: one particle carries almost all the weight."""
    rng = np.random.default_rng([N, d, seed, 77])
    X = rng.standard_normal((N, d))
    lw = np.linspace(-30.0, 0.0, N)
    rng.shuffle(lw)
    return X, lw


# Parity cases of tests/test_gpu_dpf_soft.py: (N, d, alpha, T, kind, seed, epoch).  The constants of
# the kernels are 64 rows per workgroup and 64 sources per LDS tile, component chunks of 16 and a
# split grain of 32 sources; N = 1, 2, 3 are the odd tail of a Philox pair, 63 / 64 / 65 one tile of
# rows and its tails (65: two workgroups, three splits), 130 and 300 several splits (5 and 10);
# d = 16 / 17 the chunk boundary and 40 three chunks.
PARITY = [
    (1, 1, 0.1, 0.2, "normal", 0, 0),
    (2, 2, 0.1, 0.2, "normal", 1, 0),
    (3, 5, 0.0, 1.0, "normal", 2, 1),
    (63, 16, 0.1, 0.2, "normal", 3, 0),
    (64, 17, 1.0, 0.2, "normal", 4, 2),
    (65, 1, 0.1, 1.0, "dominant", 5, 0),
    (65, 40, 0.0, 0.2, "dominant", 6, 3),
    (130, 5, 0.1, 0.2, "uniform", 7, 0),
    (130, 17, 0.1, 1.0, "normal", 8, 0),
    (300, 2, 0.0, 0.2, "dominant", 9, 4),
    (300, 40, 0.1, 0.2, "normal", 10, 0),
    (300, 16, 1.0, 1.0, "dominant", 11, 0),
]


def parity_inputs(N, d, kind, seed):
    if kind == "dominant":
        return dominant_case(N, d, seed)
    return make_case(N, d, seed, spread=0.0 if kind == "uniform" else 3.0)


_cache = {}


def solved(N, d, alpha, T, kind, seed, epoch, problem=0):
    """(X, lw, restatement result) of a parity case, computed once; do not modify the arrays."""
    key = (N, d, alpha, T, kind, seed, epoch, problem)
    if key not in _cache:
        X, lw = parity_inputs(N, d, kind, seed)
        X.setflags(write=False)
        lw.setflags(write=False)
        _cache[key] = (X, lw, soft_resample(X, lw, alpha, T, seed, epoch, problem))
    return _cache[key]


# the hard-limit check (tests/test_gpu_dpf_soft.py item 5, condition asserted in test_dpf_soft_host.py)
HARD = dict(N=256, d=3, alpha=0.1, T=1e-3, seed=12, epoch=0, gap=0.04, share=0.9)


def hard_case():
    c = HARD
    X, lw = make_case(c["N"], c["d"], seed=c["seed"], spread=1.0)
    lp = log_probs(lw, c["alpha"])
    _, G = draws(c["N"], c["seed"], c["epoch"], 0)
    s = lp[None, :] + G
    order = np.sort(s, axis=-1)
    gap = order[:, -1] - order[:, -2]
    return X, lw, np.argmax(s, axis=-1), gap


# the class test: the reference's own unit-test model (linear transition, Gaussian likelihood)
def linear_model(noise_seed):
    rng = np.random.default_rng(noise_seed)

    def transition_fn(x, params):
        return 0.9 * x + 0.1 * rng.standard_normal(x.shape)

    def log_likelihood_fn(x, y, params):
        var = params.get("sigma_r", 0.5) ** 2
        diff = y[:, None, :] - x
        return -0.5 * np.log(2.0 * np.pi * var) - 0.5 * np.sum(diff ** 2, axis=-1) / var

    return transition_fn, log_likelihood_fn
