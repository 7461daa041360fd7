"""What the three resampler modules of the DPF family (``dpf_ot``, ``dpf_soft``, ``dpf_rnn``, and
``dpf_soft_torch``) share: the argument checks made before the library is loaded, the owner of a
native handle, the handle a filter keeps between steps, the choice between the host and the device
path of the torch bindings with a counter of the calls per path, and the small NumPy utilities that
are the same expression in more than one of the reference's files.  Internal: not exported by the
package.
"""

from __future__ import annotations

import numpy as np

from . import _native as NV

MAX_DIM = 1024  # pf_ot_create's, pf_soft_create's and pf_rnn_create's limit on d
MAX_BATCH = 65535


def log_normalize(log_w, axis=-1, keepdims=False):
    """soft.py:60-81, rnn.py:353-375: ``(log_w - logsumexp(log_w), logsumexp(log_w))``."""
    log_w = np.asarray(log_w, dtype=np.float64)
    m = np.max(log_w, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    log_z = m + np.log(np.sum(np.exp(log_w - m), axis=axis, keepdims=True))
    log_w_norm = log_w - log_z
    if not keepdims:
        log_z = np.squeeze(log_z, axis=axis)
    return log_w_norm, log_z


# ---------------------------------------------------------------------- argument checks
def as_batched(particles, weights, weights_name, max_batch=None, batch_range=False, max_pairs=None):
    """The front of every ``_validate``: float64 ``particles`` (N, d) or (B, N, d) and ``weights``
    (N,) or (B, N) as ``(X [B, N, d], w [B, N], batched)`` after the checks of rank, agreement, B,
    N, d and of finite particles.  ``max_batch`` bounds B; with ``batch_range`` one message covers
    both ends of B (``dpf_rnn``'s wording).  ``max_pairs`` bounds B N^2."""
    X = np.asarray(particles, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    batched = check_batched_shapes(X.shape, w.shape, weights_name, max_batch, batch_range, max_pairs)
    if not batched:
        X, w = X[None], w[None]
    if not np.all(np.isfinite(X)):
        raise ValueError("particles must be finite")
    return X, w, batched


def check_batched_shapes(X_shape, w_shape, weights_name, max_batch=None, batch_range=False, max_pairs=None) -> bool:
    """The checks of ``as_batched`` that need the shapes only (the device path of the torch bindings
    makes them on metadata); returns ``batched``."""
    X_shape, w_shape = tuple(X_shape), tuple(w_shape)
    if len(X_shape) not in (2, 3):
        raise ValueError(f"particles must be (N, d) or (B, N, d), got shape {X_shape}")
    if len(w_shape) != len(X_shape) - 1:
        raise ValueError(f"{weights_name} must be {'(N,)' if len(X_shape) == 2 else '(B, N)'} for particles of shape "
                         f"{X_shape}, got shape {w_shape}")
    batched = len(X_shape) == 3
    if not batched:
        X_shape, w_shape = (1,) + X_shape, (1,) + w_shape
    B, N, d = X_shape
    if w_shape != (B, N):
        raise ValueError(f"particles {X_shape[-2:]} and {weights_name} {w_shape[-1:]} disagree on N (or on the batch)")
    if batch_range:
        if B < 1 or B > max_batch:
            raise ValueError(f"the batch must hold 1 .. {max_batch} problems, got {B}")
    elif B < 1:
        raise ValueError("the batch must hold at least one problem")
    elif max_batch is not None and B > max_batch:
        raise ValueError(f"B = {B} is above the device limit of {max_batch}")
    if N < 1 or d < 1:
        raise ValueError(f"need N >= 1 and d >= 1, got N = {N}, d = {d}")
    if d > MAX_DIM:
        raise ValueError(f"d = {d} is above the device limit of {MAX_DIM}")
    if max_pairs is not None and B * N * N > max_pairs:
        raise ValueError(f"B N^2 = {B * N * N} is above the device limit of {max_pairs}")
    return batched


# ---------------------------------------------------------------------- the two paths of the torch bindings
PATH_CALLS = {"host": 0, "device": 0}  # resampling calls of the torch bindings (dpf_ot_torch, dpf_soft_torch, dpf_rnn_torch) per path (for tests)


def on_device(tensors, device) -> bool:
    """The device path applies: every tensor is a CUDA tensor on HIP device ``device``, the one that
    computes.  (The bindings have checked that they are float64 tensors.)  Anything else - CPU
    tensors, mixed placement, another GPU - takes the host path."""
    return all(t.is_cuda and t.device.index == int(device) for t in tensors)


def count_path(device_path: bool) -> None:
    PATH_CALLS["device" if device_path else "host"] += 1


def raise_first(code: int, messages) -> None:
    """The device path folds its value checks into one integer, bit k set when check k failed:
    raise the ``ValueError`` of the first that did, in the order the host path makes them."""
    for k, msg in enumerate(messages):
        if code >> k & 1:
            raise ValueError(msg)


def check_log_weights(lw) -> None:
    if np.any(np.isnan(lw)) or np.any(lw == np.inf):
        raise ValueError("log_weights must not hold NaN or +inf")
    if not np.all(np.any(np.isfinite(lw), axis=-1)):
        raise ValueError("every problem needs at least one finite log-weight")


def check_positive(name, value) -> None:
    if not (float(value) > 0.0) or not np.isfinite(float(value)):
        raise ValueError(f"{name} must be positive, got {value}")


def check_seed(seed) -> None:
    if int(seed) != seed or not (0 <= int(seed) < 1 << 64):
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed}")


def check_epoch(epoch) -> None:
    if int(epoch) != epoch or not (0 <= int(epoch) < 1 << 32):
        raise ValueError(f"epoch must be an integer in [0, 2^32), got {epoch}")


# ---------------------------------------------------------------------- handles
class NativeHandle:
    """Owner of one ``pf_<unit>_*`` handle for (B, N, d) problems.  A subclass names its ``unit``,
    sets ``N, d, B``, passes its opts struct to ``_create`` and adds the unit's calls."""

    unit = ""
    h = None

    def _create(self, opts) -> None:
        name = f"pf_{self.unit}_create"
        hd = NV.C.c_void_p()
        NV.check(getattr(NV.load(), name)(NV.C.byref(opts), NV.C.byref(hd)), name)
        self.h = hd

    def key(self):
        """What a cached handle must agree on to be used again."""
        return (self.N, self.d, self.B)

    def close(self) -> None:
        if self.h is not None:
            getattr(NV.load(), f"pf_{self.unit}_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HandleCache:
    """For a filter that keeps one device handle in ``self._h`` between steps."""

    _h = None

    def _cached(self, key, make):
        """``self._h`` if its ``key()`` is ``key``, otherwise ``make()`` in its place."""
        if self._h is None or self._h.key() != key:
            self.close()
            self._h = make()
        return self._h

    def close(self) -> None:
        if self._h is not None:
            self._h.close()
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------- filter utilities
def init_particles_batched(rng, B, N, d, mean, chol):
    """soft.py:216-261, rnn.py:428-473: (B, N, d) draws ``mean + eps @ L`` from ``rng`` and
    log-weights log(1 / N); ``mean`` (d,) or (B, d), ``chol`` (d, d) or (B, d, d)."""
    B = int(B)
    mean = np.asarray(mean, dtype=np.float64)
    chol = np.asarray(chol, dtype=np.float64)
    if mean.ndim == 1:
        mean = np.broadcast_to(mean[None, :], (B, d))
    if chol.ndim == 2:
        chol = np.broadcast_to(chol[None, :, :], (B, d, d))
    eps = rng.standard_normal((B, N, d))
    noise = np.einsum("bnd,bdk->bnk", eps, chol)
    return mean[:, None, :] + noise, np.log(np.full((B, N), 1.0 / N))


def ess_of_log_weights(log_weights):
    """soft.py:83-103, rnn.py:377-397: 1 / sum w^2 of the renormalised weights, shape (B,)."""
    weights = np.exp(np.asarray(log_weights, dtype=np.float64))
    weights = weights / np.sum(weights, axis=-1, keepdims=True)
    return 1.0 / np.sum(weights ** 2, axis=-1)


def masked_distance_blocks(P, block):
    """The pairwise distances of one particle set ``P`` (N, d) in blocks of ``block`` rows, the
    diagonal zeroed (the reference's (1 - eye) mask); never an (N, N, d) array."""
    N, d = P.shape
    for r0 in range(0, N, block):
        rows = P[r0:r0 + block]
        d2 = np.zeros((rows.shape[0], N))
        for k in range(d):
            d2 += np.square(rows[:, k, None] - P[None, :, k])
        dist = np.sqrt(d2)
        idx = np.arange(rows.shape[0])
        dist[idx, r0 + idx] = 0.0
        yield dist
