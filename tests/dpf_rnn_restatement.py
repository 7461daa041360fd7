"""NumPy restatement of the RNN resampler - TEST INFRASTRUCTURE ONLY.

The reference (models/DPF_RNN_resampling.py, "rnn.py") needs TensorFlow, which is not available, so
parity of the device code is pinned to this file.  It restates, in fp64 (or any NumPy float type:
``dtype=np.longdouble`` is the conditioning check of tests/test_dpf_rnn_host.py),

* the Keras cells the reference builds: ``LSTMCell`` (gate order i, f, c, o; ``z = x kernel + h
  recurrent_kernel + bias``; ``c' = sigma(z_f) c + sigma(z_i) tanh(z_c)``; ``h' = sigma(z_o)
  tanh(c')``) and ``GRUCell`` with ``reset_after=True`` (gate order z, r, h; bias of shape (2, 3H);
  ``xm = x kernel + bias[0]``, ``hm = h recurrent_kernel + bias[1]``; ``z = sigma(xm_z + hm_z)``,
  ``r = sigma(xm_r + hm_r)``, ``hh = tanh(xm_h + r hm_h)``, ``h' = z h + (1 - z) hh``);
* rnn.py:289-347 literally - for each new particle i the features ``[w_j, x_j, onehot(i)]`` are
  concatenated and every (i, layer, t) is one cell call on vectors: ``literal_resample``;
* the same vectorised over i, the one-hot product taken as the row ``kernel0[F0 + i]``:
  ``resample``;
* the baseline resampler rnn.py:217-261 on the Philox Gumbels of the soft resampler: ``baseline``;
* the filter loop rnn.py:478-638: ``filter``.

Weights are lists in the order of Keras' ``get_weights()``: per layer kernel, recurrent_kernel,
bias; then the output layer's kernel and bias.
"""

from __future__ import annotations

import numpy as np

from tests import dpf_soft_restatement as SR

GATES = {"lstm": 4, "gru": 3}


def feature_dim(d, use_weight=True, use_particle=True):
    return (1 if use_weight else 0) + (d if use_particle else 0)


def make_weights(rng, N, d, H, L, cell, use_weight=True, use_particle=True, dense_scale=1.0):
    """Test weights of O(1) effect everywhere: a Dense kernel of scale ``dense_scale`` (the reference's
    0.001 makes every row of A uniform and hides everything), biases away from zero."""
    G, F0 = GATES[cell], feature_dim(d, use_weight, use_particle)
    out = []
    for l in range(L):
        if l == 0:
            K = np.concatenate([0.5 * rng.standard_normal((F0, G * H)), rng.standard_normal((N, G * H))])
        else:
            K = 1.5 * rng.standard_normal((H, G * H)) / np.sqrt(H)
        R = rng.standard_normal((H, G * H)) / np.sqrt(H)
        if cell == "lstm":
            b = 0.1 * rng.standard_normal(4 * H)
            b[H:2 * H] += 1.0
        else:
            b = 0.1 * rng.standard_normal((2, 3 * H))
        out += [K, R, b]
    out += [dense_scale * rng.standard_normal((H, N)), 0.1 * rng.standard_normal(N)]
    return out


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def lstm_cell(x, h, c, K, R, b):
    """One LSTMCell call; x (..., in), h and c (..., H)."""
    H = h.shape[-1]
    z = x @ K + h @ R + b
    i, f, g, o = (z[..., k * H:(k + 1) * H] for k in range(4))
    c = _sigmoid(f) * c + _sigmoid(i) * np.tanh(g)
    return _sigmoid(o) * np.tanh(c), c


def gru_cell(x, h, K, R, b):
    """One GRUCell(reset_after=True) call."""
    H = h.shape[-1]
    xm = x @ K + b[0]
    hm = h @ R + b[1]
    z = _sigmoid(xm[..., :H] + hm[..., :H])
    r = _sigmoid(xm[..., H:2 * H] + hm[..., H:2 * H])
    hh = np.tanh(xm[..., 2 * H:] + r * hm[..., 2 * H:])
    return z * h + (1.0 - z) * hh


def features(X, log_w, use_weight=True, use_particle=True, dtype=np.float64):
    """(N, F0): [exp(log_w_j)], x_j."""
    parts = []
    if use_weight:
        parts.append(np.exp(np.asarray(log_w, dtype=dtype))[:, None])
    if use_particle:
        parts.append(np.asarray(X, dtype=dtype))
    return np.concatenate(parts, axis=-1)


def _softmax(z):
    e = np.exp(z - np.max(z, axis=-1, keepdims=True))
    return e / np.sum(e, axis=-1, keepdims=True)


def _finish(hid, X, weights, T, dtype):
    Kd, bd = (np.asarray(a, dtype=dtype) for a in weights[-2:])
    A = _softmax((hid @ Kd + bd) / dtype(T))
    return {"particles": A @ np.asarray(X, dtype=dtype), "A": A, "hid": hid}


def resample(X, log_w, weights, cell="lstm", T=1.0, use_weight=True, use_particle=True, dtype=np.float64):
    """One problem, vectorised over the new particle i.  X (N, d), log_w (N,) normalised log-weights."""
    W = [np.asarray(a, dtype=dtype) for a in weights]
    L = (len(W) - 2) // 3
    N = np.shape(X)[0]
    H = W[1].shape[0]
    feat = features(X, log_w, use_weight, use_particle, dtype)
    F0 = feat.shape[1]
    h = [np.zeros((N, H), dtype=dtype) for _ in range(L)]
    c = [np.zeros((N, H), dtype=dtype) for _ in range(L)]
    eye = np.eye(N, dtype=dtype)
    for t in range(N):
        for l in range(L):
            K, R, b = W[3 * l:3 * l + 3]
            # layer 0: x kernel0 = feat_t kernel0[:F0] + kernel0[F0 + i], as one product with [feat_t, I]
            x = np.concatenate([np.broadcast_to(feat[t], (N, F0)), eye], axis=-1) if l == 0 else h[l - 1]
            if cell == "lstm":
                h[l], c[l] = lstm_cell(x, h[l], c[l], K, R, b)
            else:
                h[l] = gru_cell(x, h[l], K, R, b)
    return _finish(h[-1], X, W, T, dtype)


def literal_resample(X, log_w, weights, cell="lstm", T=1.0, use_weight=True, use_particle=True):
    """rnn.py:289-347 as written: per new particle i the concatenated features, then layer by layer a
    cell call per timestep, the outputs of a layer stacked as the next layer's inputs."""
    W = [np.asarray(a, dtype=np.float64) for a in weights]
    L = (len(W) - 2) // 3
    N = np.shape(X)[0]
    H = W[1].shape[0]
    feat = features(X, log_w, use_weight, use_particle)
    hid = np.zeros((N, H))
    for i in range(N):
        onehot = np.zeros(N)
        onehot[i] = 1.0
        rnn_input = [np.concatenate([feat[t], onehot]) for t in range(N)]
        for l in range(L):
            K, R, b = W[3 * l:3 * l + 3]
            h, c = np.zeros(H), np.zeros(H)
            outputs = []
            for t in range(N):
                if cell == "lstm":
                    h, c = lstm_cell(rnn_input[t], h, c, K, R, b)
                else:
                    h = gru_cell(rnn_input[t], h, K, R, b)
                outputs.append(h)
            rnn_input = outputs
        hid[i] = rnn_input[-1]
    return _finish(hid, X, W, T, np.float64)


def baseline(X, log_w, T=1.0, seed=0, epoch=0, problem=0):
    """rnn.py:217-261 with the Gumbels of the soft resampler's Philox counters."""
    X = np.asarray(X, dtype=np.float64)
    w = np.exp(np.asarray(log_w, dtype=np.float64))
    w = w / np.sum(w)
    lp = np.log(w + 1e-10) / T
    _, G = SR.draws(X.shape[0], seed, epoch, problem)
    A = _softmax(lp[None, :] + 0.1 * G)
    return {"particles": A @ X, "A": A, "lp": lp}


def log_normalize(lw):
    m = np.max(lw, axis=-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    return lw - (m + np.log(np.sum(np.exp(lw - m), axis=-1, keepdims=True)))


def filter(observations, init_mean, init_cov_chol, transition_fn, log_likelihood_fn, N, d, weights, cell, rng,
           T=1.0, use_weight=True, use_particle=True, params=None):
    """rnn.py:543-638: (particles (B, T+1, N, d), log-weights (B, T+1, N), assignments (B, T, N, N))."""
    params = params or {}
    obs = np.asarray(observations, dtype=np.float64)
    B, steps = obs.shape[:2]
    mean = np.broadcast_to(np.asarray(init_mean, dtype=np.float64), (B, d))
    chol = np.broadcast_to(np.asarray(init_cov_chol, dtype=np.float64), (B, d, d))
    particles = mean[:, None, :] + np.einsum("bnd,bdk->bnk", rng.standard_normal((B, N, d)), chol)
    logw = np.log(np.full((B, N), 1.0 / N))
    ps, lws, As = [particles], [logw], []
    for t in range(steps):
        pred = np.asarray(transition_fn(particles, params), dtype=np.float64)
        lw = log_normalize(logw + log_likelihood_fn(pred, obs[:, t, :], params))
        res = [resample(pred[b], lw[b], weights, cell, T, use_weight, use_particle) for b in range(B)]
        particles = np.stack([r["particles"] for r in res])
        logw = np.log(np.full((B, N), 1.0 / N))
        ps.append(particles)
        lws.append(logw)
        As.append(np.stack([r["A"] for r in res]))
    return np.stack(ps, axis=1), np.stack(lws, axis=1), np.stack(As, axis=1)


def resample_fn(weights, cell, use_weight=True, use_particle=True):
    """Host stand-in for ``DifferentiableParticleFilterRNN._resample``: (B, N, d), (B, N) -> (new, A)."""
    def fn(particles, log_weights, temperature):
        res = [resample(particles[b], log_weights[b], weights, cell, temperature, use_weight, use_particle)
               for b in range(np.shape(particles)[0])]
        return np.stack([r["particles"] for r in res]), np.stack([r["A"] for r in res])
    return fn


# ------------------------------------------------------------------ cases shared by the tests
# The recurrence kernel gives a workgroup 16 new particles, a wave 16 hidden units, and an MFMA
# k-step 4 hidden units: N = 1, 3 one partial tile, 16 an exact one, 17 a tile and one row, 33 three
# tiles; H = 1, 5 one partial unit tile (k-steps 1 and 2, not multiples of 4), 16 an exact one, 24 and
# 28 two tiles, 64 four.  N = 30 / H = 32 and N = 35 / H = 28 / L = 2 are the reference's own tests'.
# kind: "normal"; "neginf" (log-weights with -inf entries); "big" (two particles of magnitude 1e6: saturated gates;
# a longer run of them would close every forget gate at some step and erase particle 0 from A).
#
# The workgroup has HT = ceil(H / 16) unit tiles (64 lanes each from HT = 3 on), and the weights leave
# LDS once states and fragments pass 160 KiB (res = False: the residency make_plan must choose).
# H = 48 is HT = 3 (192 lanes) resident, H = 40 / L = 2 HT = 3 with 10 k-steps streaming on its own;
# H = 65 HT = 5 with 15 padded units and 17 k-steps (H % 4 = 1), its 4 Hp = 320 pre-activation
# columns two blocks of the projection, the second partial; H = 100 HT = 7 with 25 k-steps; H = 128
# HT = 8 (512 lanes), 4 Hp = 512 two exact blocks.  H = 128 / L = 4 is the largest network the library
# accepts (four layers streamed), H = 8 / L = 4 four layers resident.  H = 64 / L = 2 / B = 2 streams on
# its own with three row tiles and a batch; H = 32 / L = 3 is the first (H, L) past "H <= 32 with
# L <= 2" (191488 B).  N = 260 is 17 row tiles and, in the assignment kernel of 256 lanes, two trips
# of every loop over j, the second for 4 lanes only, and five trips of a wave's loop over j in A X
# (a GRU: an LSTM forgets particle 0 down to 1e-7 over 257 steps); d = 9 is three trips of that
# kernel's loop over the coordinates, the last with one wave.  H = 90 is the one tile count left,
# HT = 6, with 23 k-steps (the remainder 3 modulo 4 no other case has).
def case(N, d, H, L, cell, uw=True, up=True, T=1.0, kind="normal", B=1, seed=0, res=True):
    return dict(N=N, d=d, H=H, L=L, cell=cell, uw=uw, up=up, T=T, kind=kind, B=B, seed=seed, res=res)


PARITY = [
    case(1, 1, 1, 1, "lstm", seed=1),
    case(3, 2, 5, 2, "gru", seed=2),
    case(3, 1, 5, 3, "gru", seed=3),
    case(16, 5, 16, 1, "gru", seed=4),
    case(17, 2, 24, 3, "lstm", seed=5),
    case(33, 1, 64, 1, "lstm", seed=6),
    case(33, 2, 64, 1, "gru", seed=7),
    case(30, 1, 32, 1, "lstm", seed=8),
    case(35, 2, 28, 2, "gru", seed=9),
    case(17, 2, 5, 1, "lstm", up=False, seed=10),
    case(17, 5, 5, 1, "gru", uw=False, seed=11),
    case(17, 2, 16, 2, "lstm", B=3, seed=12),
    case(16, 1, 24, 1, "gru", T=0.1, seed=14),
    case(17, 2, 5, 2, "gru", kind="neginf", seed=14),
    case(17, 2, 16, 1, "lstm", kind="big", seed=15),
    case(17, 2, 48, 1, "lstm", seed=31),
    case(17, 2, 40, 2, "gru", seed=32, res=False),
    case(18, 1, 65, 1, "gru", seed=33, res=False),
    case(17, 2, 100, 1, "lstm", seed=34, res=False),
    case(16, 1, 128, 1, "gru", seed=35, res=False),
    case(17, 2, 128, 4, "lstm", seed=36, res=False),
    case(17, 1, 8, 4, "gru", seed=37),
    case(33, 2, 64, 2, "lstm", B=2, seed=38, res=False),
    case(17, 2, 32, 3, "gru", seed=42, res=False),
    case(260, 2, 8, 1, "gru", seed=39),
    case(17, 9, 16, 1, "gru", seed=41),
    case(17, 2, 90, 1, "gru", seed=43, res=False),
]


def case_id(c):
    tag = f"N{c['N']}-d{c['d']}-H{c['H']}-L{c['L']}-{c['cell']}"
    if not c["uw"]:
        tag += "-particle_only"
    if not c["up"]:
        tag += "-weight_only"
    if c["T"] != 1.0:
        tag += f"-T{c['T']}"
    if c["kind"] != "normal":
        tag += "-" + c["kind"]
    if c["B"] != 1:
        tag += f"-B{c['B']}"
    return tag


def case_inputs(c):
    """(X (B, N, d), normalised log-weights (B, N), weights) of a case."""
    rng = np.random.default_rng([c["N"], c["d"], c["H"], c["L"], c["seed"]])
    B, N, d = c["B"], c["N"], c["d"]
    X = rng.standard_normal((B, N, d))
    lw = 1.5 * rng.standard_normal((B, N))
    if c["kind"] == "neginf":
        lw[:, 1::3] = -np.inf
    if c["kind"] == "big":
        X[:, [1, N // 2]] *= 1e6
    lw = log_normalize(lw)
    W = make_weights(rng, N, d, c["H"], c["L"], c["cell"], c["uw"], c["up"])
    return X, lw, W


_cache = {}


def solved(c):
    """(X, lw, weights, [restatement result per problem]) of a case, computed once; do not modify."""
    key = case_id(c) + f"-s{c['seed']}"
    if key not in _cache:
        X, lw, W = case_inputs(c)
        for a in [X, lw] + W:
            a.setflags(write=False)
        ref = [resample(X[b], lw[b], W, c["cell"], c["T"], c["uw"], c["up"]) for b in range(c["B"])]
        _cache[key] = (X, lw, W, ref)
    return _cache[key]


# the LGSSM of the reference's integration test: x' = 0.9 x + 0.5 eps, y = x + 0.5 eta
def lgssm(noise_seed):
    rng = np.random.default_rng(noise_seed)

    def transition_fn(x, params):
        return params.get("a", 0.9) * x + params.get("sigma_q", 0.5) * rng.standard_normal(np.shape(x))

    def log_likelihood_fn(x, y, params):
        var = params.get("sigma_r", 0.5) ** 2
        diff = y[:, None, :] - x
        return np.sum(-0.5 * np.log(2.0 * np.pi * var) - 0.5 * diff ** 2 / var, axis=-1)

    return transition_fn, log_likelihood_fn
