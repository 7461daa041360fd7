"""RNN resampling and the ``DifferentiableParticleFilterRNN`` on the MI355X.

Mirrors the reference's ``models/DPF_RNN_resampling.py`` (cited ``rnn.py:LINE``):
``DifferentiableParticleFilterRNN`` (9-638) with the same constructor arguments, defaults, attribute
names, return tuples and dictionary keys, and its resampling step (rnn.py:263-349) as the function
``rnn_resample``.  This module is NumPy: it runs the forward pass, and ``rnn_resample_vjp`` is the
backward pass of one resampling (``pf_rnn_backward``: the gradients to the particles, the log-weights
and every weight array).  The trainable filter, with ``loss.backward()`` and an optimizer over the
network, is ``dpf_rnn_torch.DifferentiableParticleFilterRNN``.  A model trained under TensorFlow is
carried over as::

    weights = [np.asarray(a, dtype=np.float64) for a in np.load("rnn_weights.npy", allow_pickle=True)]
    dpf = DifferentiableParticleFilterRNN(N, d, transition_fn, log_likelihood_fn, rnn_type="lstm",
                                          rnn_hidden_dim=32, weights=weights)

with ``weights`` in the order of Keras' ``get_weights()``: for every layer ``kernel``,
``recurrent_kernel``, ``bias``, then the output layer's ``kernel`` and ``bias`` (that is
``sum((c.get_weights() for c in ref.rnn_cells), []) + ref.output_layer.get_weights()``).

What runs where.  For each of the N new particles the reference runs a fresh LSTM / GRU over all N
old particles: N^2 eager cell calls per filter step.  On the device that is one persistent
recurrence launch (``pf_rnn_resample``, ``csrc/pf_rnn_kernels.h``): 16 sequences per workgroup, the
hidden state and the recurrent weights on chip for all N timesteps, each timestep a small fp64
matrix-core product and the gate activations.  There is no CPU fallback.  Exponentiating the
normalised log-weights is O(B N) and done in NumPy.  The user's ``transition_fn(particles, params)``
and ``log_likelihood_fn(particles, observation, params)`` are vectorised NumPy callables on
(B, N, d) and run on the host, as they are the user's TensorFlow code in the reference.

Differences from the reference:

* arithmetic is fp64 and results are NumPy float64 arrays; the reference computes in float32;
* without ``weights`` the network is initialised from ``rng`` with Keras' defaults (Glorot-uniform
  kernels, orthogonal recurrent kernels, zero biases with the LSTM forget block at 1) and
  rnn.py:155-162 (output kernel ``0.001 N(0, 1)``, output bias 0); the reference draws from
  TensorFlow's and NumPy's global generators;
* layer 0's kernel has ``F0 + N`` rows (``F0 = [1] + [d]``): the one-hot block of length N that
  rnn.py:203-210 appends is part of the input the lazily built Keras cell sees;
* with ``use_baseline_resampling=True`` the Gumbel draws are a pure function of ``(seed, epoch,
  problem, i, j)``, the draws of ``dpf_soft`` (``include/pf_engine.h``); ``step`` uses
  ``(self.seed, self.epoch)`` and advances ``self.epoch`` by one when it succeeds.  The uniform
  behind a draw is strictly inside (0, 1), where the reference clamps to [1e-10, 1);
* the reference's banner lines are not printed;
* TensorFlow is not available where this was developed, so parity is pinned to a NumPy restatement
  of the reference's formulas and Keras' cell conventions (``tests/dpf_rnn_restatement.py``).
"""

from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np

from . import _dpf_common as DC
from . import _native as NV
from ._dpf_common import MAX_BATCH, MAX_DIM  # noqa: F401  (pf_rnn_create's limits on B and d)
from ._dpf_common import log_normalize as _log_normalize

Array = np.ndarray

__all__ = ["rnn_resample", "rnn_resample_vjp", "DifferentiableParticleFilterRNN"]

MAX_HIDDEN = 128  # pf_rnn_create's limits
MAX_LAYERS = 4
MAX_PAIRS = 1 << 28  # B N^2
CELLS = {"lstm": 0, "gru": 1}
GATES = {"lstm": 4, "gru": 3}


def weight_shapes(n_particles, state_dim, rnn_type="lstm", rnn_hidden_dim=64, rnn_num_layers=1,
                  use_weight_features=True, use_particle_features=True):
    """The shapes of ``get_weights()``, in its order."""
    N, H, G = int(n_particles), int(rnn_hidden_dim), GATES[rnn_type]
    F0 = (1 if use_weight_features else 0) + (int(state_dim) if use_particle_features else 0)
    shapes = []
    for l in range(int(rnn_num_layers)):
        shapes += [((F0 + N) if l == 0 else H, G * H), (H, G * H), (4 * H,) if rnn_type == "lstm" else (2, 3 * H)]
    return shapes + [(H, N), (N,)]


def init_weights(rng, n_particles, state_dim, rnn_type="lstm", rnn_hidden_dim=64, rnn_num_layers=1,
                 use_weight_features=True, use_particle_features=True) -> List[Array]:
    """Keras' default initialisation of the cells and rnn.py:155-162 for the output layer."""
    H = int(rnn_hidden_dim)
    out = []
    for shape in weight_shapes(n_particles, state_dim, rnn_type, H, rnn_num_layers, use_weight_features,
                               use_particle_features)[:-2]:
        k = len(out) % 3
        if k == 0:  # glorot_uniform
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            out.append(rng.uniform(-lim, lim, size=shape))
        elif k == 1:  # orthogonal: Q of a (G H, H) normal matrix, signs from R's diagonal, transposed
            q, r = np.linalg.qr(rng.standard_normal((shape[1], shape[0])))
            out.append(np.ascontiguousarray((q * np.sign(np.diag(r))).T))
        else:
            b = np.zeros(shape)
            if rnn_type == "lstm":
                b[H:2 * H] = 1.0  # unit_forget_bias
            out.append(b)
    N = int(n_particles)
    return out + [0.001 * rng.standard_normal((H, N)), np.zeros(N)]


def _check_weights(weights, shapes) -> List[Array]:
    weights = list(weights)
    if len(weights) != len(shapes):
        raise ValueError(f"expected {len(shapes)} weight arrays (kernel, recurrent_kernel, bias per layer, then the "
                         f"output kernel and bias), got {len(weights)}")
    out = []
    for k, (a, shape) in enumerate(zip(weights, shapes)):
        a = np.array(a, dtype=np.float64, order="C")  # a copy: the caller's array stays the caller's
        if a.shape != tuple(shape):
            raise ValueError(f"weight array {k} has shape {a.shape}, expected {tuple(shape)}")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"weight array {k} must be finite")
        out.append(a)
    return out


def _validate(particles, log_weights, temperature):
    """The checks made before the library is loaded; returns (X [B,N,d], lw [B,N], batched)."""
    X, lw, batched = DC.as_batched(particles, log_weights, "log_weights", MAX_BATCH, batch_range=True,
                                   max_pairs=MAX_PAIRS)
    DC.check_log_weights(lw)
    DC.check_positive("temperature", temperature)
    return np.ascontiguousarray(X), np.ascontiguousarray(lw), batched


class _Handle(DC.NativeHandle):
    """One pf_rnn handle: (B, N, d) and a network shape on one device."""

    unit = "rnn"

    def __init__(self, N, d, B=1, hidden=64, layers=1, rnn_type="lstm", use_weight=True, use_particle=True, device=0):
        self.N, self.d, self.B = int(N), int(d), int(B)
        self.hidden, self.layers, self.rnn_type = int(hidden), int(layers), rnn_type
        self.use_weight, self.use_particle = bool(use_weight), bool(use_particle)
        self._create(NV.RnnOpts(self.N, self.d, self.B, self.hidden, self.layers, CELLS[rnn_type], int(self.use_weight),
                                int(self.use_particle), int(device)))

    def key(self):
        return (self.N, self.d, self.B, self.hidden, self.layers, self.rnn_type, self.use_weight, self.use_particle)

    @property
    def resident(self) -> bool:
        return bool(NV.load().pf_rnn_resident(self.h))

    def set_weights(self, weights) -> None:
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in weights]
        ptrs = (NV._dp * len(arrs))(*[NV.dptr(a) for a in arrs])
        sizes = (NV.C.c_int64 * len(arrs))(*[a.size for a in arrs])
        NV.check(NV.load().pf_rnn_set_weights(self.h, ptrs, sizes, len(arrs)), "pf_rnn_set_weights")
        self._packed = None

    # the device-pointer entries: every pointer an integer address of contiguous float64 device memory on
    # the handle's device (0 for a nullable one), ``stream`` a hipStream_t as an integer (0: the handle's
    # own stream, and the call synchronises); with a stream the calls enqueue and return
    packs = 0       # pf_rnn_set_weights_dev calls of this handle
    _packed = None  # what the weights on the device were packed from (set_weights_dev's ``key``)

    def set_weights_dev(self, stream, ptrs, sizes, key=None) -> bool:
        """Pack the network from the device arrays at ``ptrs`` (k_rnn_pack).  With a ``key`` - the torch
        binding's ``(data_ptr, version)`` of every parameter - a call whose key is that of the weights
        already packed does nothing and returns False."""
        if key is not None and key == self._packed:
            return False
        p = (NV._vp * len(ptrs))(*ptrs)
        n = (NV.C.c_int64 * len(ptrs))(*sizes)
        self._packed = None
        NV.check(NV.load().pf_rnn_set_weights_dev(self.h, stream, p, n, len(ptrs)), "pf_rnn_set_weights_dev")
        self._packed = key
        self.packs += 1
        return True

    def resample_dev(self, stream, X, w, temperature, out, A=0, hid=0) -> None:
        NV.check(NV.load().pf_rnn_resample_dev(self.h, stream, X, w, float(temperature), out, A, hid),
                 "pf_rnn_resample_dev")

    def backward_dev(self, stream, X, w, temperature, grad_out, grad_A, grad_X, grad_w, grad_ptrs, sizes) -> None:
        p = (NV._vp * len(grad_ptrs))(*grad_ptrs)
        n = (NV.C.c_int64 * len(grad_ptrs))(*sizes)
        NV.check(NV.load().pf_rnn_backward_dev(self.h, stream, X, w, float(temperature), grad_out, grad_A, grad_X,
                                               grad_w, p, n, len(grad_ptrs)), "pf_rnn_backward_dev")

    def resample(self, X: Array, w: Array, temperature, want_hidden: bool = False):
        """X [B][N][d], normalised weights w [B][N] -> (X_out, A [B][N][N], hid [B][N][H] or None)."""
        out = np.empty_like(X)
        A = np.empty((self.B, self.N, self.N))
        hid = np.empty((self.B, self.N, self.hidden)) if want_hidden else None
        NV.check(NV.load().pf_rnn_resample(self.h, NV.dptr(X), NV.dptr(w), float(temperature), NV.dptr(out),
                                           NV.dptr(A), NV.dptr(hid)), "pf_rnn_resample")
        return out, A, hid

    @property
    def backward_bytes(self) -> int:
        """The device workspace the first ``backward`` of this handle allocates."""
        return int(NV.load().pf_rnn_backward_bytes(self.h))

    def backward(self, X: Array, w: Array, temperature, grad_out: Array, grad_A: Optional[Array], shapes):
        """X, w as in ``resample``; grad_out [B][N][d]; grad_A [B][N][N] or None -> (grad_X, grad_w [B][N],
        [gradient per weight array, of ``shapes``]), the weight gradients summed over the B problems."""
        gX, gw = np.empty_like(X), np.empty((self.B, self.N))
        gW = [np.empty(shape) for shape in shapes]
        ptrs = (NV._dp * len(gW))(*[NV.dptr(a) for a in gW])
        sizes = (NV.C.c_int64 * len(gW))(*[a.size for a in gW])
        NV.check(NV.load().pf_rnn_backward(self.h, NV.dptr(X), NV.dptr(w), float(temperature), NV.dptr(grad_out),
                                           NV.dptr(grad_A), NV.dptr(gX), NV.dptr(gw), ptrs, sizes, len(gW)),
                 "pf_rnn_backward")
        return gX, gw, gW

    def baseline(self, X: Array, lp: Array, seed=0, epoch=0, batch_base=0):
        """X [B][N][d], lp [B][N] = log(w + 1e-10) / T -> (X_out, A)."""
        out = np.empty_like(X)
        A = np.empty((self.B, self.N, self.N))
        NV.check(NV.load().pf_rnn_baseline(self.h, NV.dptr(X), NV.dptr(lp), int(seed), int(epoch), int(batch_base),
                                           NV.dptr(out), NV.dptr(A)), "pf_rnn_baseline")
        return out, A


def _baseline_log_probs(log_weights, temperature) -> Array:
    """rnn.py:237-245: ``log(w / sum w + 1e-10) / temperature``."""
    w = np.exp(np.asarray(log_weights, dtype=np.float64))
    w = w / np.sum(w, axis=-1, keepdims=True)
    return np.ascontiguousarray(np.log(w + 1e-10) / float(temperature))


def rnn_resample(particles, log_weights, weights, rnn_type="lstm", temperature=1.0, *, use_weight_features=True,
                 use_particle_features=True, return_hidden=False, device=0, _handle: Optional["_Handle"] = None):
    """The RNN resampling of rnn.py:263-349 on the device.

    ``particles`` (N, d) with ``log_weights`` (N,), or (B, N, d) with (B, N) for B independent
    problems; the features use ``exp(log_weights)`` as given (``step`` passes normalised ones).
    ``weights`` is the network in Keras' ``get_weights()`` order; the hidden size and the number of
    layers are read from it.  Returns ``(new_particles, assignment_probs)``, with ``return_hidden``
    also the last hidden states (N, H) or (B, N, H)."""
    rnn_type = str(rnn_type).lower()
    if rnn_type not in CELLS:
        raise ValueError(f"Unknown RNN type: {rnn_type}. Use 'lstm' or 'gru'")
    if not use_weight_features and not use_particle_features:
        raise ValueError("Must use at least one of weight_features or particle_features")
    X, lw, batched = _validate(particles, log_weights, temperature)
    B, N, d = X.shape
    weights = list(weights)
    if len(weights) < 5 or (len(weights) - 2) % 3 or np.ndim(weights[1]) != 2:
        raise ValueError("weights must be kernel, recurrent_kernel, bias per layer, then the output kernel and bias")
    H, L = int(np.shape(weights[1])[0]), (len(weights) - 2) // 3
    W = _check_weights(weights, weight_shapes(N, d, rnn_type, H, L, use_weight_features, use_particle_features))
    h = _handle
    own = h is None or h.h is None or h.key() != (N, d, B, H, L, rnn_type, bool(use_weight_features),
                                                  bool(use_particle_features))
    if own:
        h = _Handle(N, d, B, H, L, rnn_type, use_weight_features, use_particle_features, device)
    try:
        h.set_weights(W)
        out, A, hid = h.resample(X, np.ascontiguousarray(np.exp(lw)), temperature, bool(return_hidden))
    finally:
        if own:
            h.close()
    if not batched:
        out, A = out[0], A[0]
        hid = hid[0] if hid is not None else None
    return (out, A, hid) if return_hidden else (out, A)


def _network(weights, N, d, rnn_type, use_weight_features, use_particle_features):
    """(rnn_type, H, L, checked copies of the weights): the network's shape is read from the arrays."""
    rnn_type = str(rnn_type).lower()
    if rnn_type not in CELLS:
        raise ValueError(f"Unknown RNN type: {rnn_type}. Use 'lstm' or 'gru'")
    if not use_weight_features and not use_particle_features:
        raise ValueError("Must use at least one of weight_features or particle_features")
    weights = list(weights)
    if len(weights) < 5 or (len(weights) - 2) % 3 or np.ndim(weights[1]) != 2:
        raise ValueError("weights must be kernel, recurrent_kernel, bias per layer, then the output kernel and bias")
    H, L = int(np.shape(weights[1])[0]), (len(weights) - 2) // 3
    if not (1 <= H <= MAX_HIDDEN) or not (1 <= L <= MAX_LAYERS):
        raise ValueError(f"the network must have 1 .. {MAX_HIDDEN} hidden units and 1 .. {MAX_LAYERS} layers, "
                         f"got {H} and {L}")
    W = _check_weights(weights, weight_shapes(N, d, rnn_type, H, L, use_weight_features, use_particle_features))
    return rnn_type, H, L, W


def _network_of_shapes(shapes, N, d, rnn_type, use_weight_features, use_particle_features):
    """``_network``'s checks on the arrays' shapes alone, with its messages: (rnn_type, H, L).  For
    callers whose arrays are on the device; the values are theirs to check."""
    rnn_type = str(rnn_type).lower()
    if rnn_type not in CELLS:
        raise ValueError(f"Unknown RNN type: {rnn_type}. Use 'lstm' or 'gru'")
    if not use_weight_features and not use_particle_features:
        raise ValueError("Must use at least one of weight_features or particle_features")
    shapes = [tuple(s) for s in shapes]
    if len(shapes) < 5 or (len(shapes) - 2) % 3 or len(shapes[1]) != 2:
        raise ValueError("weights must be kernel, recurrent_kernel, bias per layer, then the output kernel and bias")
    H, L = int(shapes[1][0]), (len(shapes) - 2) // 3
    if not (1 <= H <= MAX_HIDDEN) or not (1 <= L <= MAX_LAYERS):
        raise ValueError(f"the network must have 1 .. {MAX_HIDDEN} hidden units and 1 .. {MAX_LAYERS} layers, "
                         f"got {H} and {L}")
    for k, (got, want) in enumerate(zip(shapes, weight_shapes(N, d, rnn_type, H, L, use_weight_features,
                                                              use_particle_features))):
        if got != tuple(want):
            raise ValueError(f"weight array {k} has shape {got}, expected {tuple(want)}")
    return rnn_type, H, L


def rnn_resample_vjp(particles, log_weights, weights, grad_new_particles, grad_assignment=None, rnn_type="lstm",
                     temperature=1.0, *, use_weight_features=True, use_particle_features=True, device=0,
                     _handle: Optional[_Handle] = None):
    """The backward pass of ``rnn_resample`` at the same arguments.  Given ``grad_new_particles`` and
    (optionally) ``grad_assignment``, the gradients of a scalar with respect to the two results of
    ``rnn_resample`` (the particles' shape, and (N, N) or (B, N, N)), returns ``(g_particles,
    g_log_weights, [g_weights...])``: the gradients with respect to ``particles``, to ``log_weights``
    and to every array of ``weights``, in their shapes and order; a weight's gradient is summed over
    the B problems.  There is no gradient with respect to the temperature.

    One ``pf_rnn_backward``: the device runs the forward pass again, keeping every hidden state, and
    back-propagates through the N timesteps of the N sequences.  Its workspace grows as
    B N^2 L hidden (``_Handle.backward_bytes``).  The O(B N) chain from the weights ``exp(log_weights)``
    to the log-weights, ``g_log_weights = g_w exp(log_weights)``, is NumPy; a log-weight of -inf gets
    exactly 0."""
    X, lw, batched = _validate(particles, log_weights, temperature)
    B, N, d = X.shape
    rnn_type, H, L, W = _network(weights, N, d, rnn_type, use_weight_features, use_particle_features)
    g = np.asarray(grad_new_particles, dtype=np.float64)
    if g.shape != (X.shape if batched else X.shape[1:]):
        raise ValueError(f"grad_new_particles must have the particles' shape {np.shape(particles)}, got {g.shape}")
    if not np.all(np.isfinite(g)):
        raise ValueError("grad_new_particles must be finite")
    g = np.ascontiguousarray(g.reshape(X.shape))
    gA = None
    if grad_assignment is not None:
        gA = np.asarray(grad_assignment, dtype=np.float64)
        if gA.shape != ((B, N, N) if batched else (N, N)):
            raise ValueError(f"grad_assignment must be {(B, N, N) if batched else (N, N)}, got {gA.shape}")
        if not np.all(np.isfinite(gA)):
            raise ValueError("grad_assignment must be finite")
        gA = np.ascontiguousarray(gA.reshape(B, N, N))
    w = np.ascontiguousarray(np.exp(lw))
    h = _handle
    key = (N, d, B, H, L, rnn_type, bool(use_weight_features), bool(use_particle_features))
    own = h is None or h.h is None or h.key() != key
    if own:
        h = _Handle(N, d, B, H, L, rnn_type, use_weight_features, use_particle_features, device)
    try:
        h.set_weights(W)
        gX, gw, gW = h.backward(X, w, temperature, g, gA, [a.shape for a in W])
    finally:
        if own:
            h.close()
    glw = np.where(w > 0.0, gw * w, 0.0)
    return (gX, glw, gW) if batched else (gX[0], glw[0], gW)


class DifferentiableParticleFilterRNN(DC.HandleCache):
    """Particle filter with RNN resampling at every step (drop-in for rnn.py:9-638), NumPy and forward
    only; ``dpf_rnn_torch`` has the differentiable one."""

    def __init__(self, n_particles, state_dim, transition_fn: Callable, log_likelihood_fn: Callable, rnn_type="lstm",
                 rnn_hidden_dim=64, rnn_num_layers=1, use_weight_features=True, use_particle_features=True,
                 temperature=1.0, use_baseline_resampling=False, name=None, *, weights=None,
                 rng: Optional[np.random.Generator] = None, seed=0, device=0):
        self.name = name
        self.n_particles = int(n_particles)
        self.state_dim = int(state_dim)
        if self.n_particles < 1 or self.state_dim < 1:
            raise ValueError(f"need n_particles >= 1 and state_dim >= 1, got {n_particles}, {state_dim}")
        DC.check_seed(seed)
        self.transition_fn = transition_fn
        self.log_likelihood_fn = log_likelihood_fn
        self.rnn_type = str(rnn_type).lower()
        self.rnn_hidden_dim = int(rnn_hidden_dim)
        self.rnn_num_layers = int(rnn_num_layers)
        self.use_weight_features = bool(use_weight_features)
        self.use_particle_features = bool(use_particle_features)
        self.temperature = temperature
        self.use_baseline_resampling = bool(use_baseline_resampling)
        self.seed = int(seed)
        self.epoch = 0
        self.rng = rng if rng is not None else np.random.default_rng()
        self.device = int(device)
        self._h: Optional[_Handle] = None
        self._weights: Optional[List[Array]] = None
        self._resample = self._device_resample  # the tests swap in a host resampler here
        if not self.use_baseline_resampling:
            # rnn.py:96-97 and 115, in the order _build_rnn_resampler raises them
            if not self.use_weight_features and not self.use_particle_features:
                raise ValueError("Must use at least one of weight_features or particle_features")
            if self.rnn_type not in CELLS:
                raise ValueError(f"Unknown RNN type: {self.rnn_type}. Use 'lstm' or 'gru'")
            if not (1 <= self.rnn_hidden_dim <= MAX_HIDDEN):
                raise ValueError(f"rnn_hidden_dim must be in 1 .. {MAX_HIDDEN}, got {rnn_hidden_dim}")
            if not (1 <= self.rnn_num_layers <= MAX_LAYERS):
                raise ValueError(f"rnn_num_layers must be in 1 .. {MAX_LAYERS}, got {rnn_num_layers}")
            self.set_weights(weights if weights is not None else init_weights(self.rng, *self._net()))

    # ------------------------------------------------------------------ the network
    def _net(self):
        return (self.n_particles, self.state_dim, self.rnn_type, self.rnn_hidden_dim, self.rnn_num_layers,
                self.use_weight_features, self.use_particle_features)

    def get_weights(self) -> List[Array]:
        """Copies of the network's arrays in Keras' order (empty with ``use_baseline_resampling``)."""
        return [a.copy() for a in (self._weights or [])]

    def set_weights(self, weights) -> None:
        """Replace the network; shapes are checked against ``weight_shapes``."""
        if self.use_baseline_resampling:
            raise ValueError("the baseline resampler has no network")
        self._weights = _check_weights(weights, weight_shapes(*self._net()))
        if self._h is not None:
            self._h.set_weights(self._weights)

    # ------------------------------------------------------------------ device handle
    def _handle(self, B: int) -> _Handle:
        N, d = self.n_particles, self.state_dim
        base = self.use_baseline_resampling
        want = (N, d, B, 1 if base else self.rnn_hidden_dim, 1 if base else self.rnn_num_layers,
                "lstm" if base else self.rnn_type, True if base else self.use_weight_features,
                True if base else self.use_particle_features)
        fresh = self._h is None or self._h.key() != want
        h = self._cached(want, lambda: _Handle(*want, device=self.device))
        if fresh and not base:
            h.set_weights(self._weights)
        return h

    def _device_resample(self, particles, log_weights, temperature):
        X, lw, _ = _validate(particles, log_weights, temperature)
        if X.shape[1:] != (self.n_particles, self.state_dim):
            raise ValueError(f"particles must be (B, {self.n_particles}, {self.state_dim}), got {X.shape}")
        out, A, _ = self._handle(X.shape[0]).resample(X, np.ascontiguousarray(np.exp(lw)), temperature)
        return out, A

    # ------------------------------------------------------------------ resamplers
    def _compute_rnn_features(self, particles, log_weights, target_particle_idx=None):
        """rnn.py:169-215 on the host, for API parity: (B, N, F0 [+ N])."""
        particles = np.asarray(particles, dtype=np.float64)
        B, N = particles.shape[0], self.n_particles
        features = []
        if self.use_weight_features:
            features.append(np.exp(np.asarray(log_weights, dtype=np.float64))[..., None])
        if self.use_particle_features:
            features.append(particles)
        if target_particle_idx is not None:
            onehot = np.zeros(N)
            onehot[int(target_particle_idx)] = 1.0
            features.append(np.broadcast_to(onehot[None, None, :], (B, N, N)))
        return np.concatenate(features, axis=-1)

    def _baseline_resample(self, particles, log_weights):
        """rnn.py:217-261 on the device, with the draws of ``(self.seed, self.epoch)``; returns
        ``(new_particles, assignment_probs)``.  ``self.epoch`` is advanced by ``step``."""
        X, lw, _ = _validate(particles, log_weights, self.temperature)
        if X.shape[1:] != (self.n_particles, self.state_dim):
            raise ValueError(f"particles must be (B, {self.n_particles}, {self.state_dim}), got {X.shape}")
        return self._handle(X.shape[0]).baseline(X, _baseline_log_probs(lw, self.temperature), self.seed, self.epoch)

    def _rnn_resample(self, particles, log_weights):
        """rnn.py:263-349: ``(new_particles (B, N, d), assignment_probs (B, N, N))``."""
        if self.use_baseline_resampling:
            return self._baseline_resample(particles, log_weights)
        return self._resample(particles, log_weights, self.temperature)

    # ------------------------------------------------------------------ utilities
    _log_normalize = staticmethod(_log_normalize)

    compute_ess = staticmethod(DC.ess_of_log_weights)

    @staticmethod
    def compute_weight_entropy(log_weights):
        """rnn.py:399-423: -sum w log w of the renormalised weights clipped to [1e-10, 1], shape (B,)."""
        weights = np.exp(np.asarray(log_weights, dtype=np.float64))
        weights = weights / np.sum(weights, axis=-1, keepdims=True)
        weights = np.clip(weights, 1e-10, 1.0)
        return -np.sum(weights * np.log(weights), axis=-1)

    # ------------------------------------------------------------------ the filter
    def init_particles(self, batch_size, init_mean, init_cov_chol):
        """rnn.py:428-473: (B, N, d) draws ``mean + eps @ L`` from ``self.rng`` and log-weights log(1 / N)."""
        return DC.init_particles_batched(self.rng, batch_size, self.n_particles, self.state_dim, init_mean,
                                         init_cov_chol)

    def step(self, particles, log_weights, observation, params=None, return_ess=False):
        """rnn.py:478-539: propagate, reweight (host NumPy), resample (device).  Returns
        ``(new_particles, new_log_weights, assignment_matrix)`` and with ``return_ess`` a dictionary
        with ``ess_before``, ``ess_after``, ``entropy_before``, ``entropy_after``."""
        if params is None:
            params = {}
        pred_particles = np.asarray(self.transition_fn(particles, params), dtype=np.float64)
        log_lik = np.asarray(self.log_likelihood_fn(pred_particles, observation, params), dtype=np.float64)
        log_weights = np.asarray(log_weights, dtype=np.float64) + log_lik
        log_weights, _ = self._log_normalize(log_weights, axis=-1, keepdims=False)
        if return_ess:
            ess_before = self.compute_ess(log_weights)
            entropy_before = self.compute_weight_entropy(log_weights)
        new_particles, assignment_matrix = self._rnn_resample(pred_particles, log_weights)
        if self.use_baseline_resampling:
            self.epoch += 1
        new_log_weights = np.log(np.full((np.shape(particles)[0], self.n_particles), 1.0 / self.n_particles))
        if not return_ess:
            return new_particles, new_log_weights, assignment_matrix
        ess_dict = {
            "ess_before": ess_before,
            "ess_after": self.compute_ess(new_log_weights),
            "entropy_before": entropy_before,
            "entropy_after": self.compute_weight_entropy(new_log_weights),
        }
        return new_particles, new_log_weights, assignment_matrix, ess_dict

    def filter(self, observations, init_mean, init_cov_chol, params=None, return_ess=False):
        """rnn.py:543-638: the filter over ``observations`` (B, T, obs_dim); returns particles
        (B, T + 1, N, d), log-weights (B, T + 1, N), the prior draw first, and the assignment matrices
        (B, T, N, N); with ``return_ess`` also the reference's statistics dictionary."""
        if params is None:
            params = {}
        observations = np.asarray(observations, dtype=np.float64)
        B, T = observations.shape[0], observations.shape[1]
        particles, logw = self.init_particles(batch_size=B, init_mean=init_mean, init_cov_chol=init_cov_chol)
        particles_list, logw_list, assignment_matrices = [particles], [logw], []
        stats = {"ess_before": [], "ess_after": [], "entropy_before": [], "entropy_after": []}
        for t in range(T):
            y_t = observations[:, t, :]
            if return_ess:
                particles, logw, assignment, ess_dict = self.step(particles, logw, y_t, params=params, return_ess=True)
                for key in stats:
                    stats[key].append(ess_dict[key])
            else:
                particles, logw, assignment = self.step(particles, logw, y_t, params=params)
            particles_list.append(particles)
            logw_list.append(logw)
            assignment_matrices.append(assignment)
        N = self.n_particles
        particles_seq = np.stack(particles_list, axis=1)
        logw_seq = np.stack(logw_list, axis=1)
        assignment_seq = np.stack(assignment_matrices, axis=1) if T else np.zeros((B, 0, N, N))
        if not return_ess:
            return particles_seq, logw_seq, assignment_seq
        ess_before, ess_after, entropy_before, entropy_after = (
            np.stack(stats[k], axis=1) if T else np.zeros((B, 0))
            for k in ("ess_before", "ess_after", "entropy_before", "entropy_after"))
        ess_stats = {
            "ess_before_resampling": ess_before,
            "ess_after_resampling": ess_after,
            "entropy_before_resampling": entropy_before,
            "entropy_after_resampling": entropy_after,
            "mean_ess_before": np.mean(ess_before) if T else np.nan,
            "mean_ess_after": np.mean(ess_after) if T else np.nan,
            "mean_entropy_before": np.mean(entropy_before) if T else np.nan,
            "mean_entropy_after": np.mean(entropy_after) if T else np.nan,
            "min_ess_before": np.min(ess_before) if T else np.nan,
            "min_ess_after": np.min(ess_after) if T else np.nan,
        }
        return particles_seq, logw_seq, assignment_seq, ess_stats
