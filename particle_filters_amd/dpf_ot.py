"""Sinkhorn optimal-transport resampling and the ``DPF_OT`` filter on the MI355X.

Mirrors the reference's ``models/DPF_OT_resampling.py`` (cited ``ot.py:LINE``):
``pairwise_squared_distances`` (8-31), ``tau_epsilon`` (36-68), ``sinkhorn_ot_resample`` (71-234)
and ``DPF_OT`` (238-634), with the same names, arguments and defaults.  The backward pass of the
resampler is ``sinkhorn_ot_resample_vjp`` (``pf_ot_backward``): the derivative of the unrolled
damped loop as ``tf.GradientTape`` forms it in the reference, with respect to the particles and the
weights; ``particle_filters_amd.dpf_ot_torch`` binds it to PyTorch's autograd.  The soft resampler
of the DPF family is ``particle_filters_amd.dpf_soft`` and the RNN resampler
``particle_filters_amd.dpf_rnn``.

What runs where.  The resampler is the hot path: 2 x n_iters dependent log-sum-exp passes over
the N x N cost matrix and one N x N plan applied to the particles.  All of it is one
stream-ordered sequence of HIP launches (``pf_ot_resample``, ``csrc/pf_ot_kernels.h``); the
stopping rule of ot.py:169-181 is decided on the device.  There is no CPU fallback.
``pairwise_squared_distances`` and ``tau_epsilon`` are the reference's expressions in NumPy (they
are small and serve user code and the tests).  ``DPF_OT`` calls the user's ``transition_fn(particles,
t)`` and ``obs_loglik_fn(particles, y_t, t)`` on the host: they are vectorised callables on (N, d)
NumPy arrays, as they are the user's TensorFlow code in the reference, and O(N d) against the
resampler's O(N^2).

Two differences from the reference:

* arithmetic is fp64, as in every flow filter of this package; the reference casts to float32;
* TensorFlow is not available where this was developed, so no fixture of reference outputs exists:
  parity is pinned to a NumPy restatement of the reference's formulas
  (``tests/dpf_ot_restatement.py``), not to reference outputs.

``init_particles`` draws ``rng.standard_normal((N, d)) @ cov_chol.T + mean`` from the filter's
``rng``; the reference draws from TensorFlow's global generator, whose stream cannot be replayed.

One extension: ``sinkhorn_ot_resample`` also takes ``particles`` (B, N, d) with ``weights`` (B, N),
B independent problems in one call, each with its own stopping iteration; diagnostics are then a
list of B dicts.
"""

from __future__ import annotations

import time
from typing import Callable, NamedTuple, Optional

import numpy as np

from . import _dpf_common as DC
from . import _native as NV
from ._dpf_common import MAX_DIM  # noqa: F401  (pf_ot_create's limit on d)

Array = np.ndarray
RESIDENT_MAX_N = 128  # of the one-launch solver (csrc/pf_ot_resident_plan.h)

__all__ = ["pairwise_squared_distances", "tau_epsilon", "sinkhorn_ot_resample", "sinkhorn_ot_resample_vjp", "OtSaved",
           "DPF_OT"]


def pairwise_squared_distances(x, y) -> Array:
    """ot.py:8-31: ``dist[i, j] = |x_i - y_j|^2`` by the expansion, floored at 0."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    x_sq = np.sum(np.square(x), axis=1, keepdims=True)
    y_sq = np.sum(np.square(y), axis=1, keepdims=True)
    xy = x @ y.T
    dist = x_sq - 2.0 * xy + y_sq.T
    return np.maximum(dist, 0.0)


def tau_epsilon(a, f, C_vec, epsilon, min_val=1e-12):
    """ot.py:36-68: ``-eps * log(sum_k a_k exp((f_k - C_k) / eps))`` with the maximum factored out."""
    exponent = (np.asarray(f, dtype=np.float64) - np.asarray(C_vec, dtype=np.float64)) / epsilon
    max_exp = np.max(exponent)
    exp_shifted = np.exp(exponent - max_exp)
    weighted_sum = np.sum(np.asarray(a, dtype=np.float64) * exp_shifted)
    return -epsilon * (np.log(np.maximum(weighted_sum, min_val)) + max_exp)


def _validate(particles, weights, epsilon, n_iters):
    """The checks made before the library is loaded; returns (X [B,N,d], w [B,N], batched)."""
    X, w, batched = DC.as_batched(particles, weights, "weights")
    if not np.all(np.isfinite(w)):
        raise ValueError("weights must be finite")
    DC.check_positive("epsilon", epsilon)
    if int(n_iters) != n_iters or int(n_iters) < 0:
        raise ValueError(f"n_iters must be a non-negative integer, got {n_iters}")
    return np.ascontiguousarray(X), np.ascontiguousarray(w), batched


class OtSaved(NamedTuple):
    """What a forward ``sinkhorn_ot_resample`` keeps for ``sinkhorn_ot_resample_vjp``, as host arrays:
    the iterations each problem took (B,) int32, the dual history (B, 4, K + 1, N) - f^k, g^k and the
    two Tau vectors of every iteration k = 0 .. K, K the largest of the iterations - and per column
    of every g pass the index of the maximum where the floor inside Tau bound, -1 elsewhere
    (B, K, N) int32."""
    iterations: Array
    hist: Array
    hist_argmax: Array


def _validate_grad(grad_new_particles, shape, batched):
    """The incoming gradient as [B, N, d]: the particles' shape, finite."""
    g = np.asarray(grad_new_particles, dtype=np.float64)
    want = shape if batched else shape[1:]
    if g.shape != want:
        raise ValueError(f"grad_new_particles must have the particles' shape {want}, got {g.shape}")
    if not np.all(np.isfinite(g)):
        raise ValueError("grad_new_particles must be finite")
    return np.ascontiguousarray(g.reshape(shape))


def _validate_saved(saved, shape, n_iters):
    """(iterations, hist, hist_argmax) of an ``OtSaved`` that fits problems of ``shape``."""
    if not isinstance(saved, OtSaved):
        raise ValueError("saved must be the OtSaved that sinkhorn_ot_resample(..., return_saved=True) returned")
    B, N, _ = shape
    its = np.ascontiguousarray(np.asarray(saved.iterations, dtype=np.int32))
    hist = np.ascontiguousarray(np.asarray(saved.hist, dtype=np.float64))
    am = np.ascontiguousarray(np.asarray(saved.hist_argmax, dtype=np.int32))
    if its.shape != (B,) or np.any(its < 0) or np.any(its > int(n_iters)):
        raise ValueError(f"saved.iterations must be {B} counts in 0 .. n_iters = {int(n_iters)}, got {its}")
    K = int(its.max())
    if hist.shape != (B, 4, K + 1, N) or am.shape != (B, K, N):
        raise ValueError(f"saved holds a history of shapes {hist.shape}, {am.shape}; these inputs and iterations "
                         f"need {(B, 4, K + 1, N)}, {(B, K, N)}")
    if not np.all(np.isfinite(hist)) or np.any(am < -1) or np.any(am >= N):
        raise ValueError("saved must hold a finite history and indices in -1 .. N - 1")
    return its, hist, am


class _Handle(DC.NativeHandle):
    """One pf_ot handle: (B, N, d) on one device, with the cost matrices it owns."""

    unit = "ot"
    # the iteration counts [B] of the latest forward pass ``dpf_ot_torch`` ran on this handle on its
    # device path: an int32 tensor on the device, for a caller who wants them without a second pass
    last_iterations = None

    def __init__(self, N: int, d: int, B: int = 1, device: int = 0):
        self.N, self.d, self.B = int(N), int(d), int(B)
        self._create(NV.OtOpts(self.N, self.d, self.B, int(device)))

    def resample(self, X: Array, w: Array, epsilon, n_iters, min_val, tol, want_diag: bool):
        """X [B][N][d], w [B][N] -> (X_out, iterations [B], history, f, g, plan_stats)."""
        B, N = self.B, self.N
        out = np.empty_like(X)
        its = np.zeros(B, dtype=np.int32)
        hist = f = g = stats = None
        if want_diag:
            hist = np.zeros((B, max(1, n_iters), 2))
            f, g, stats = np.zeros((B, N)), np.zeros((B, N)), np.zeros((B, 2))
        NV.check(NV.load().pf_ot_resample(
            self.h, NV.dptr(X), NV.dptr(w), float(epsilon), int(n_iters), float(min_val), float(tol), NV.dptr(out),
            its.ctypes.data_as(NV.C.POINTER(NV.C.c_int32)), NV.dptr(hist), NV.dptr(f), NV.dptr(g), NV.dptr(stats)),
            "pf_ot_resample")
        return out, its, hist, f, g, stats

    def replay(self, X: Array, w: Array, epsilon, min_val, its: Array) -> OtSaved:
        """The dual history of the ``its`` [B] iterations of X [B][N][d], w [B][N]."""
        its = np.ascontiguousarray(its, dtype=np.int32)
        K = int(its.max())
        hist = np.zeros((self.B, 4, K + 1, self.N))
        am = np.full((self.B, K, self.N), -1, dtype=np.int32)
        i32 = NV.C.POINTER(NV.C.c_int32)
        NV.check(NV.load().pf_ot_replay(self.h, NV.dptr(X), NV.dptr(w), float(epsilon), float(min_val),
                                        its.ctypes.data_as(i32), K, NV.dptr(hist), am.ctypes.data_as(i32) if K else None),
                 "pf_ot_replay")
        return OtSaved(its, hist, am)

    def backward(self, X: Array, w: Array, grad_out: Array, epsilon, min_val, its: Array, hist=None, am=None):
        """X, grad_out [B][N][d], w [B][N], its [B], the history or None -> (grad_X, grad_w)."""
        its = np.ascontiguousarray(its, dtype=np.int32)
        K = int(its.max())
        gX, gw = np.empty_like(X), np.zeros((self.B, self.N))
        i32 = NV.C.POINTER(NV.C.c_int32)
        NV.check(NV.load().pf_ot_backward(
            self.h, NV.dptr(X), NV.dptr(w), float(epsilon), float(min_val), its.ctypes.data_as(i32), K, NV.dptr(hist),
            am.ctypes.data_as(i32) if hist is not None and K else None, NV.dptr(grad_out), NV.dptr(gX), NV.dptr(gw)),
            "pf_ot_backward")
        return gX, gw

    # the device-pointer entries: raw device addresses (0 = null) and a hipStream_t (0 = the handle's
    # stream, synchronised before the return); layouts in include/pf_engine.h
    def resample_dev(self, stream, X, w, epsilon, n_iters, min_val, tol, out, iterations=0, history=0, f=0, g=0,
                     plan_stats=0, hist=0, hist_argmax=0, flags=0) -> None:
        NV.check(NV.load().pf_ot_resample_dev(self.h, stream, X, w, float(epsilon), int(n_iters), float(min_val),
                                              float(tol), int(flags), out, iterations, history, f, g, plan_stats,
                                              hist, hist_argmax), "pf_ot_resample_dev")

    def resident_supported(self) -> bool:
        """``PF_OT_RESIDENT`` (the one-launch solver) is available on this handle: N <= ``RESIDENT_MAX_N``."""
        return bool(NV.load().pf_ot_resident_supported(self.h))

    def backward_dev(self, stream, X, w, epsilon, min_val, iterations, k_cap, k_sweep, hist, hist_argmax, grad_out,
                     grad_X, grad_w) -> None:
        NV.check(NV.load().pf_ot_backward_dev(self.h, stream, X, w, float(epsilon), float(min_val), iterations,
                                              int(k_cap), int(k_sweep), hist, hist_argmax, grad_out, grad_X, grad_w),
                 "pf_ot_backward_dev")


def _diagnostics(N, epsilon, n_iters, its, hist, f, g, stats):
    """ot.py:206-230 from what the device returned for one problem."""
    return {
        "sinkhorn_iterations": int(its),
        "converged": int(its) < int(n_iters),
        "ot_distance": float(stats[0]),
        "transport_plan_sparsity": float(stats[1]) / float(N * N),
        "dual_variables": {"f_mean": float(np.mean(f)), "f_std": float(np.std(f)),
                           "g_mean": float(np.mean(g)), "g_std": float(np.std(g))},
        "convergence_history": [{"iteration": it, "f_change": float(hist[it, 0]), "g_change": float(hist[it, 1])}
                                for it in range(1, int(its))],
        "epsilon": epsilon,
    }


def sinkhorn_ot_resample(particles, weights, epsilon=0.1, n_iters=50, min_val=1e-12, tol=1e-6,
                         return_diagnostics=False, *, return_saved=False, device=0,
                         _handle: Optional[_Handle] = None):
    """Entropy-regularised OT resampling (ot.py:71-234) on the device.

    ``particles`` (N, d) with ``weights`` (N,), or (B, N, d) with (B, N) for B independent
    problems.  Returns ``(new_particles, new_weights)`` as float64 arrays, the new weights being
    1/N, and with ``return_diagnostics`` a third element: the reference's diagnostics dict (a list
    of B dicts for a batched call).  ``n_iters = 0`` gives the plan at ``f = g = 0``.  With
    ``return_saved`` the last element of the tuple is one more, an ``OtSaved``: the iterations and the
    dual history ``sinkhorn_ot_resample_vjp`` needs of this forward pass (one more run of the
    iterations, recorded; host arrays, not handle state).
    """
    X, w, batched = _validate(particles, weights, epsilon, n_iters)
    B, N, d = X.shape
    n_iters = int(n_iters)
    h = _handle
    own = h is None or h.key() != (N, d, B)
    if own:
        h = _Handle(N, d, B, device)
    try:
        out, its, hist, f, g, stats = h.resample(X, w, epsilon, n_iters, min_val, tol, bool(return_diagnostics))
        saved = h.replay(X, w, epsilon, min_val, its) if return_saved else None
    finally:
        if own:
            h.close()
    new_w = np.full((B, N), 1.0 / float(N))
    if not batched:
        out, new_w = out[0], new_w[0]
    tail = (saved,) if return_saved else ()
    if not return_diagnostics:
        return (out, new_w) + tail
    diags = [_diagnostics(N, epsilon, n_iters, its[b], hist[b], f[b], g[b], stats[b]) for b in range(B)]
    return (out, new_w, (diags if batched else diags[0])) + tail


def sinkhorn_ot_resample_vjp(particles, weights, grad_new_particles, epsilon=0.1, n_iters=50, min_val=1e-12, tol=1e-6,
                             *, saved: Optional[OtSaved] = None, device=0, _handle: Optional[_Handle] = None):
    """The backward pass of ``sinkhorn_ot_resample`` at the same arguments: given
    ``grad_new_particles``, the gradient of a scalar with respect to the new particles ((N, d) or
    (B, N, d), as ``particles``), returns ``(grad_particles, grad_weights)``.  There is no gradient
    with respect to ``epsilon``.

    The derivative is that of the reference's computation as its tape would form it: the unrolled
    damped loop over the iterations the forward pass took (the stopping rule is control flow), the
    plan, the projection, the cost and the weight normalisation, each ``maximum`` passing its
    gradient where its first argument is the larger.  It is not the implicit derivative at the
    fixed point.  The device sweeps the iterations in reverse with the plan recomputed
    (``pf_ot_backward``), keeping the dual history and one more N x N matrix.  ``saved`` is the
    ``OtSaved`` of the forward call; without it a forward pass is run first to find the iterations,
    and then they are replayed.  A weight at or below ``min_val`` gets exactly 0.
    """
    X, w, batched = _validate(particles, weights, epsilon, n_iters)
    B, N, d = X.shape
    g = _validate_grad(grad_new_particles, X.shape, batched)
    sv = _validate_saved(saved, X.shape, n_iters) if saved is not None else None
    h = _handle
    own = h is None or h.h is None or h.key() != (N, d, B)  # a handle closed since the forward pass
    if own:
        h = _Handle(N, d, B, device)
    try:
        if sv is None:
            its = h.resample(X, w, epsilon, int(n_iters), min_val, tol, False)[1]
            gX, gw = h.backward(X, w, g, epsilon, min_val, its)
        else:
            gX, gw = h.backward(X, w, g, epsilon, min_val, *sv)
    finally:
        if own:
            h.close()
    return (gX, gw) if batched else (gX[0], gw[0])


class DPF_OT(DC.HandleCache):
    """Particle filter with OT resampling at every step (drop-in for ot.py:238-634) on NumPy arrays;
    ``dpf_ot_torch.DPF_OT`` is the one whose outputs can be differentiated."""

    def __init__(self, N_particles, state_dim, transition_fn: Callable, obs_loglik_fn: Callable, epsilon=0.1,
                 sinkhorn_iters=50, name=None, *, rng: Optional[np.random.Generator] = None, device=0):
        self.name = name
        self.N = int(N_particles)
        self.d = int(state_dim)
        if self.N < 1 or self.d < 1:
            raise ValueError(f"need N_particles >= 1 and state_dim >= 1, got {N_particles}, {state_dim}")
        self.transition_fn = transition_fn
        self.obs_loglik_fn = obs_loglik_fn
        self.epsilon = epsilon
        self.sinkhorn_iters = sinkhorn_iters
        self.rng = rng if rng is not None else np.random.default_rng()
        self.device = int(device)
        self._h: Optional[_Handle] = None
        self._resample = self._device_resample  # the tests swap in a host resampler here

    # ------------------------------------------------------------------ device handle
    def _device_resample(self, particles, weights, **kw):
        X = np.asarray(particles)
        if self._h is None and X.shape == (self.N, self.d):
            _validate(X, weights, kw.get("epsilon", 0.1), kw.get("n_iters", 50))
            self._h = _Handle(self.N, self.d, 1, self.device)
        return sinkhorn_ot_resample(particles, weights, device=self.device, _handle=self._h, **kw)

    # ------------------------------------------------------------------ diagnostics helpers
    @staticmethod
    def compute_ess(weights):
        """ot.py:282-305: 1 / sum w^2 of the renormalised weights, (N,) or (B, N)."""
        w = np.asarray(weights, dtype=np.float64)
        w = w / (np.sum(w, axis=-1, keepdims=True) + 1e-12)
        return 1.0 / np.sum(w ** 2, axis=-1)

    @staticmethod
    def compute_weight_entropy(weights):
        """ot.py:307-325: -sum w log(w + 1e-10)."""
        w = np.asarray(weights, dtype=np.float64)
        w = w / (np.sum(w, axis=-1, keepdims=True) + 1e-12)
        return -np.sum(w * np.log(w + 1e-10), axis=-1)

    @staticmethod
    def compute_particle_diversity(particles, block: int = 256):
        """ot.py:327-372: mean pairwise distance and trace of the population covariance, (N, d) or
        (B, N, d).  The distances are formed in row blocks, never as an (N, N, d) array."""
        P = np.asarray(particles, dtype=np.float64)
        squeeze = P.ndim == 2
        if squeeze:
            P = P[None]
        B, N, d = P.shape
        mean_dist = np.zeros(B)
        for b in range(B):
            total = sum((float(np.sum(dist)) for dist in DC.masked_distance_blocks(P[b], block)), 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                mean_dist[b] = np.float64(total) / np.float64(N * (N - 1))
        centered = P - np.mean(P, axis=1, keepdims=True)
        spread = np.sum(np.mean(np.square(centered), axis=1), axis=-1)
        return {"mean_pairwise_dist": mean_dist[0] if squeeze else mean_dist,
                "particle_spread": spread[0] if squeeze else spread}

    # ------------------------------------------------------------------ the filter
    def init_particles(self, mean, cov_chol):
        """ot.py:374-398: N draws of N(mean, cov_chol cov_chol^T) from ``self.rng`` and weights 1/N."""
        mean = np.asarray(mean, dtype=np.float64)
        cov_chol = np.asarray(cov_chol, dtype=np.float64)
        eps = self.rng.standard_normal((self.N, self.d))
        particles = mean[None, :] + eps @ cov_chol.T
        return particles, np.full(self.N, 1.0 / float(self.N))

    def step(self, particles, weights, y_t, t=None, return_diagnostics=False):
        """ot.py:400-487: propagate, reweight (host NumPy), resample (device)."""
        if return_diagnostics:
            start_time = time.time()
            ess_before = self.compute_ess(weights)
            entropy_before = self.compute_weight_entropy(weights)
            diversity_before = self.compute_particle_diversity(particles)

        pred_particles = np.asarray(self.transition_fn(particles, t), dtype=np.float64)
        log_liks = np.asarray(self.obs_loglik_fn(pred_particles, y_t, t), dtype=np.float64)

        # ot.py:438-445
        weights = np.asarray(weights, dtype=np.float64)
        unnorm_w = weights * np.exp(log_liks)
        unnorm_w = np.maximum(unnorm_w, 0.0)
        norm_const = np.sum(unnorm_w) + 1e-12
        new_weights = unnorm_w / norm_const

        if not return_diagnostics:
            return self._resample(pred_particles, new_weights, epsilon=self.epsilon, n_iters=self.sinkhorn_iters,
                                  return_diagnostics=False)
        res_particles, res_weights, resample_diag = self._resample(
            pred_particles, new_weights, epsilon=self.epsilon, n_iters=self.sinkhorn_iters, return_diagnostics=True)
        ess_after = self.compute_ess(res_weights)
        entropy_after = self.compute_weight_entropy(res_weights)
        diversity_after = self.compute_particle_diversity(res_particles)
        end_time = time.time()
        diagnostics = {
            "ess_before": ess_before,
            "ess_after": ess_after,
            "entropy_before": entropy_before,
            "entropy_after": entropy_after,
            "diversity_before": diversity_before,
            "diversity_after": diversity_after,
            "max_weight_before": np.max(new_weights),
            "step_time": end_time - start_time,
            **resample_diag,
        }
        return res_particles, res_weights, diagnostics

    def run_filter(self, y_seq, mean0, cov0_chol, return_diagnostics=False, ground_truth=None):
        """ot.py:489-556: the filter over ``y_seq``; lists of T particle sets (N, d) and weights (N,)."""
        particles, weights = self.init_particles(mean0, cov0_chol)
        particles_seq, weights_seq = [], []
        diagnostics_list, times = [], []
        for t in range(len(y_seq)):
            y_t = y_seq[t]
            if return_diagnostics:
                start_time = time.time()
                particles, weights, step_diag = self.step(particles, weights, y_t, t=t, return_diagnostics=True)
                times.append(time.time() - start_time)
                diagnostics_list.append(step_diag)
            else:
                particles, weights = self.step(particles, weights, y_t, t=t, return_diagnostics=False)
            particles_seq.append(particles)
            weights_seq.append(weights)
        if not return_diagnostics:
            return particles_seq, weights_seq
        diagnostics = self._aggregate_diagnostics(diagnostics_list)
        diagnostics["total_time"] = sum(times)
        diagnostics["mean_step_time"] = sum(times) / len(times) if times else 0.0
        if ground_truth is not None:
            ground_truth = np.asarray(ground_truth, dtype=np.float64)
            rmse_seq = self._compute_rmse_sequence(particles_seq, weights_seq, ground_truth)
            diagnostics["rmse_sequence"] = rmse_seq
            diagnostics["mean_rmse"] = np.mean(rmse_seq)
            diagnostics["final_rmse"] = rmse_seq[-1]
        return particles_seq, weights_seq, diagnostics

    def _aggregate_diagnostics(self, diagnostics_list):
        """ot.py:558-601: mean / std / min / max over the steps (population std, as reduce_std)."""
        if not diagnostics_list:
            return {}
        aggregated = {}
        for key in diagnostics_list[0].keys():
            values = [d[key] for d in diagnostics_list]
            if key == "convergence_history":
                continue
            if isinstance(values[0], dict):
                aggregated[key] = {}
                for subkey in values[0].keys():
                    subvalues = np.stack([np.asarray(v[subkey], dtype=np.float64) for v in values])
                    aggregated[key][subkey + "_mean"] = np.mean(subvalues)
                    aggregated[key][subkey + "_std"] = np.std(subvalues)
            elif isinstance(values[0], (bool, np.bool_)):
                aggregated[key + "_rate"] = sum(bool(v) for v in values) / len(values)
            elif isinstance(values[0], (int, float, np.integer, np.floating)) or np.ndim(values[0]) == 0:
                values_list = [float(v) for v in values]
                aggregated[key + "_mean"] = sum(values_list) / len(values_list)
                aggregated[key + "_std"] = np.std(np.asarray(values_list, dtype=np.float64))
                aggregated[key + "_min"] = min(values_list)
                aggregated[key + "_max"] = max(values_list)
        return aggregated

    def _compute_rmse_sequence(self, particles_seq, weights_seq, ground_truth):
        """ot.py:603-634: |weighted mean - ground_truth[t + 1]| per step, shape (T,)."""
        rmse_list = []
        for t, (particles, weights) in enumerate(zip(particles_seq, weights_seq)):
            weights = weights / (np.sum(weights) + 1e-12)
            particle_mean = np.sum(weights[:, None] * particles, axis=0)
            squared_error = np.sum((particle_mean - ground_truth[t + 1]) ** 2)
            rmse_list.append(np.sqrt(squared_error))
        return np.stack(rmse_list)
