"""Soft (Gumbel-Softmax) resampling and the ``DifferentiableParticleFilter`` on the MI355X.

Mirrors the reference's ``models/DPF_soft_resampling.py`` (cited ``soft.py:LINE``):
``DifferentiableParticleFilter`` (8-547) with the same names, arguments, defaults and diagnostics
keys, and its resampling step (soft.py:309-334) as the function ``soft_resample``.  The class here
is the forward pass on NumPy arrays.  The resampling step has a backward pass on the device,
``soft_resample_vjp`` (``pf_soft_backward``): the gradient with respect to the particles and the
log-weights, not to ``soft_alpha`` or the temperature.  ``dpf_soft_torch.py`` binds the two to
PyTorch's autograd and holds the filter class whose outputs can be differentiated.  The RNN
resampler of the DPF family is ``dpf_rnn.py``.

What runs where.  Every step builds an (B, N, N) assignment matrix ``softmax_j((log q_j + G_ij) /
T)`` from N^2 independent Gumbel draws and multiplies it into the particles.  On the device that
is one all-pairs pass (``pf_soft_resample``, ``csrc/pf_soft_kernels.h``) in which the draws come
from Philox counters, generated where they are used, and the matrix is never stored.  There is no
CPU fallback.  The mixture ``log q = log((1 - alpha) w + alpha / N + 1e-20)`` is O(B N) and formed
in NumPy.  The user's ``transition_fn(particles, params)`` and ``log_likelihood_fn(particles,
observation, params)`` are vectorised NumPy callables on (B, N, d) and run on the host, as they are
the user's TensorFlow code in the reference.

Differences from the reference:

* arithmetic is fp64 and results are NumPy float64 arrays; the reference computes in float32;
* the Gumbel draws of a step are a pure function of ``(seed, epoch, problem, i, j)``
  (``include/pf_engine.h``), so a step can be replayed bit for bit; the reference draws from
  TensorFlow's global generator.  The uniform behind a draw is an odd multiple of 2^-53, strictly
  inside (0, 1), which replaces the reference's clamp to [1e-20, 1 - 1e-20] (soft.py:191);
* ``step`` uses ``(self.seed, self.epoch)`` and advances ``self.epoch`` by one when it succeeds;
* ``init_particles`` and the small utilities ``_sample_gumbel`` / ``_gumbel_softmax`` draw from the
  filter's ``rng``;
* TensorFlow is not available where this was developed, so parity is pinned to a NumPy restatement
  of the reference's formulas with the same draws (``tests/dpf_soft_restatement.py``).

``init_particles`` forms its noise as ``einsum("bnd,bdk->bnk", eps, L)``, that is ``eps @ L``, as
the reference's code does (soft.py:251), whatever its comment says.
"""

from __future__ import annotations

import time
from typing import Callable, NamedTuple, Optional

import numpy as np

from . import _dpf_common as DC
from . import _native as NV
from ._dpf_common import MAX_BATCH, MAX_DIM  # noqa: F401  (pf_soft_create's limits on B and d)
from ._dpf_common import log_normalize as _log_normalize

Array = np.ndarray

__all__ = ["soft_resample", "soft_resample_vjp", "SoftSaved", "DifferentiableParticleFilter"]


def _log_probs(log_w_norm: Array, alpha: float) -> Array:
    """soft.py:307-317: ``log((1 - alpha) w + alpha / N + 1e-20)`` of normalised log-weights."""
    N = log_w_norm.shape[-1]
    weights = np.exp(log_w_norm)
    uniform = np.full(weights.shape, 1.0 / N)
    probs = (1.0 - alpha) * weights + alpha * uniform
    return np.log(probs + 1e-20)


def _validate(particles, log_weights, soft_alpha, gumbel_temperature, seed=0, epoch=0):
    """The checks made before the library is loaded; returns (X [B,N,d], lw [B,N], batched)."""
    X, lw, batched = DC.as_batched(particles, log_weights, "log_weights", MAX_BATCH)
    DC.check_log_weights(lw)
    if not (0.0 <= float(soft_alpha) <= 1.0):
        raise ValueError(f"soft_alpha must be in [0, 1], got {soft_alpha}")
    DC.check_positive("gumbel_temperature", gumbel_temperature)
    DC.check_seed(seed)
    DC.check_epoch(epoch)
    return np.ascontiguousarray(X), np.ascontiguousarray(lw), batched


class SoftSaved(NamedTuple):
    """What a forward ``soft_resample`` keeps for ``soft_resample_vjp``: the new particles (B, N, d),
    the row maxima and row sums (B, N) of the assignment matrix's softmax, and the draws' (seed, epoch)."""
    X_out: Array
    row_max: Array
    row_sum: Array
    seed: int
    epoch: int


def _validate_grad(grad_new_particles, shape, batched):
    """The incoming gradient as [B, N, d]: the particles' shape, finite."""
    g = np.asarray(grad_new_particles, dtype=np.float64)
    want = shape if batched else shape[1:]
    if g.shape != want:
        raise ValueError(f"grad_new_particles must have the particles' shape {want}, got {g.shape}")
    if not np.all(np.isfinite(g)):
        raise ValueError("grad_new_particles must be finite")
    return np.ascontiguousarray(g.reshape(shape))


def _validate_saved(saved, shape, seed, epoch):
    if not isinstance(saved, SoftSaved):
        raise ValueError("saved must be the SoftSaved that soft_resample(..., return_saved=True) returned")
    B, N, d = shape
    Xo, M, L = (np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in saved[:3])
    if Xo.shape != (B, N, d) or M.shape != (B, N) or L.shape != (B, N):
        raise ValueError(f"saved holds shapes {Xo.shape}, {M.shape}, {L.shape}; these inputs need {(B, N, d)}, "
                         f"{(B, N)}, {(B, N)}")
    if (int(saved.seed), int(saved.epoch)) != (int(seed), int(epoch)):
        raise ValueError(f"saved was made with (seed, epoch) = ({saved.seed}, {saved.epoch}), the call names "
                         f"({seed}, {epoch})")
    if not (np.all(np.isfinite(Xo)) and np.all(np.isfinite(M)) and np.all(np.isfinite(L)) and np.all(L > 0.0)):
        raise ValueError("saved must hold finite values and positive row sums")
    return Xo, M, L


def _log_weights_grad(lw: Array, alpha: float, glp: Array) -> Array:
    """The chain from the gradient of ``log_probs`` (B, N) to the gradient of the unnormalised
    log-weights ``lw``: through ``log((1 - alpha) w + alpha / N + 1e-20)`` and ``_log_normalize``.  A
    log-weight of -inf gets exactly 0, and so does everything when ``alpha = 1``."""
    N = lw.shape[-1]
    w = np.exp(_log_normalize(lw, axis=-1)[0])
    q = (1.0 - alpha) * w + alpha * (1.0 / N)
    u = ((1.0 - alpha) * glp / (q + 1e-20)) * w
    return u - w * np.sum(u, axis=-1, keepdims=True)


class _Handle(DC.NativeHandle):
    """One pf_soft handle: (B, N, d) on one device, with the partial sums it owns."""

    unit = "soft"

    def __init__(self, N: int, d: int, B: int = 1, device: int = 0):
        self.N, self.d, self.B = int(N), int(d), int(B)
        self._create(NV.SoftOpts(self.N, self.d, self.B, int(device)))

    def resample(self, X: Array, log_probs: Array, temperature, seed=0, epoch=0, batch_base=0,
                 want_entropy: bool = False):
        """X [B][N][d], log_probs [B][N] -> (X_out, row_entropy [B][N] or None)."""
        out = np.empty_like(X)
        H = np.zeros((self.B, self.N)) if want_entropy else None
        NV.check(NV.load().pf_soft_resample(self.h, NV.dptr(X), NV.dptr(log_probs), float(temperature), int(seed),
                                            int(epoch), int(batch_base), NV.dptr(out), NV.dptr(H)),
                 "pf_soft_resample")
        return out, H

    def row_stats(self):
        """(row_max, row_sum) [B][N] of the handle's latest forward pass."""
        M, L = np.zeros((self.B, self.N)), np.zeros((self.B, self.N))
        NV.check(NV.load().pf_soft_row_stats(self.h, NV.dptr(M), NV.dptr(L)), "pf_soft_row_stats")
        return M, L

    def backward(self, X: Array, log_probs: Array, temperature, grad_out: Array, seed=0, epoch=0, batch_base=0,
                 saved=None):
        """X, grad_out [B][N][d], log_probs [B][N], saved (X_out, row_max, row_sum) or None ->
        (grad_X [B][N][d], grad_log_probs [B][N])."""
        gX, glp = np.empty_like(X), np.zeros((self.B, self.N))
        Xo, M, L = saved if saved is not None else (None, None, None)
        NV.check(NV.load().pf_soft_backward(self.h, NV.dptr(X), NV.dptr(log_probs), float(temperature), int(seed),
                                            int(epoch), int(batch_base), NV.dptr(Xo), NV.dptr(M), NV.dptr(L),
                                            NV.dptr(grad_out), NV.dptr(gX), NV.dptr(glp)), "pf_soft_backward")
        return gX, glp

    # the device-pointer entries: every pointer an integer address of contiguous float64 device memory on
    # the handle's device (0 for a nullable one), ``stream`` a hipStream_t as an integer (0: the handle's
    # own stream, and the call synchronises); with a stream the calls enqueue and return
    def resample_dev(self, stream, X, log_probs, temperature, seed, epoch, batch_base, out, entropy=0, row_max=0,
                     row_sum=0) -> None:
        NV.check(NV.load().pf_soft_resample_dev(self.h, stream, X, log_probs, float(temperature), int(seed),
                                                int(epoch), int(batch_base), out, entropy, row_max, row_sum),
                 "pf_soft_resample_dev")

    def backward_dev(self, stream, X, log_probs, temperature, seed, epoch, batch_base, X_out, row_max, row_sum,
                     grad_out, grad_X, grad_log_probs) -> None:
        NV.check(NV.load().pf_soft_backward_dev(self.h, stream, X, log_probs, float(temperature), int(seed),
                                                int(epoch), int(batch_base), X_out, row_max, row_sum, grad_out,
                                                grad_X, grad_log_probs), "pf_soft_backward_dev")

    def draws(self, seed=0, epoch=0, batch_base=0):
        """(U, G) [B][N][N]: the uniforms and Gumbels pf_soft_resample uses for these arguments."""
        U = np.zeros((self.B, self.N, self.N))
        G = np.zeros((self.B, self.N, self.N))
        NV.check(NV.load().pf_soft_draws(self.h, int(seed), int(epoch), int(batch_base), NV.dptr(U), NV.dptr(G)),
                 "pf_soft_draws")
        return U, G


def soft_resample(particles, log_weights, soft_alpha=0.1, gumbel_temperature=0.2, *, seed=0, epoch=0,
                  return_diagnostics=False, return_saved=False, device=0, _handle: Optional[_Handle] = None):
    """The soft resampling of soft.py:306-339 on the device.

    ``particles`` (N, d) with ``log_weights`` (N,), or (B, N, d) with (B, N) for B independent
    problems; the log-weights need not be normalised.  Returns ``(new_particles, new_log_weights)``
    as float64 arrays, the new log-weights being ``log(1 / N)``, and with ``return_diagnostics`` a
    third element: the entropies ``-sum_j a_ij log(a_ij + 1e-10)`` of the rows of the assignment
    matrix, (N,) or (B, N) (soft.py:348-350).  Problem ``b`` of a batch uses the draws of
    ``(seed, epoch, b)``.  With ``return_saved`` the last element of the tuple is one more, a
    ``SoftSaved``: what ``soft_resample_vjp`` needs of this forward pass to skip running it again.
    """
    X, lw, batched = _validate(particles, log_weights, soft_alpha, gumbel_temperature, seed, epoch)
    B, N, d = X.shape
    lw, _ = _log_normalize(lw, axis=-1)
    lp = np.ascontiguousarray(_log_probs(lw, float(soft_alpha)))
    h = _handle
    own = h is None or h.key() != (N, d, B)
    if own:
        h = _Handle(N, d, B, device)
    try:
        out, H = h.resample(X, lp, gumbel_temperature, seed, epoch, 0, bool(return_diagnostics))
        saved = SoftSaved(out, *h.row_stats(), int(seed), int(epoch)) if return_saved else None
    finally:
        if own:
            h.close()
    new_lw = np.log(np.full((B, N), 1.0 / float(N)))
    if not batched:
        out, new_lw = out[0], new_lw[0]
        H = H[0] if H is not None else None
    return (out, new_lw) + ((H,) if return_diagnostics else ()) + ((saved,) if return_saved else ())


def soft_resample_vjp(particles, log_weights, grad_new_particles, soft_alpha=0.1, gumbel_temperature=0.2, *, seed=0,
                      epoch=0, saved: Optional[SoftSaved] = None, device=0, _handle: Optional[_Handle] = None):
    """The backward pass of ``soft_resample`` at the same arguments: given ``grad_new_particles``, the
    gradient of a scalar with respect to the new particles ((N, d) or (B, N, d), as ``particles``),
    returns ``(grad_particles, grad_log_weights)``, the gradients with respect to ``particles`` and to
    the unnormalised ``log_weights``.  There is none with respect to ``soft_alpha`` or the temperature.

    The assignment matrix is regenerated on the device from the draws of ``(seed, epoch)`` in one more
    all-pairs pass (``pf_soft_backward``); the O(B N) chain from ``log q`` back to the log-weights is
    NumPy.  ``saved`` is the ``SoftSaved`` of the forward call (``soft_resample(...,
    return_saved=True)``) with the same ``(seed, epoch)``; without it the forward pass is run again
    first.  A log-weight of -inf gets the gradient 0, and with ``soft_alpha = 1`` all of them do.
    """
    X, lw, batched = _validate(particles, log_weights, soft_alpha, gumbel_temperature, seed, epoch)
    B, N, d = X.shape
    g = _validate_grad(grad_new_particles, X.shape, batched)
    sv = _validate_saved(saved, X.shape, seed, epoch) if saved is not None else None
    alpha = float(soft_alpha)
    lp = np.ascontiguousarray(_log_probs(_log_normalize(lw, axis=-1)[0], alpha))
    h = _handle
    own = h is None or h.h is None or h.key() != (N, d, B)  # a handle closed since the forward pass
    if own:
        h = _Handle(N, d, B, device)
    try:
        gX, glp = h.backward(X, lp, gumbel_temperature, g, seed, epoch, 0, sv)
    finally:
        if own:
            h.close()
    glw = _log_weights_grad(lw, alpha, glp)
    return (gX, glw) if batched else (gX[0], glw[0])


class DifferentiableParticleFilter(DC.HandleCache):
    """Particle filter with soft resampling at every step (drop-in for soft.py:8-547, forward only)."""

    def __init__(self, n_particles, state_dim, transition_fn: Callable, log_likelihood_fn: Callable, soft_alpha=0.1,
                 gumbel_temperature=0.2, name=None, *, seed=0, rng: Optional[np.random.Generator] = None, device=0):
        self.name = name
        self.n_particles = int(n_particles)
        self.state_dim = int(state_dim)
        if self.n_particles < 1 or self.state_dim < 1:
            raise ValueError(f"need n_particles >= 1 and state_dim >= 1, got {n_particles}, {state_dim}")
        DC.check_seed(seed)
        self.transition_fn = transition_fn
        self.log_likelihood_fn = log_likelihood_fn
        self.soft_alpha = soft_alpha
        self.gumbel_temperature = gumbel_temperature
        self.seed = int(seed)
        self.epoch = 0
        self.rng = rng if rng is not None else np.random.default_rng()
        self.device = int(device)
        self._h: Optional[_Handle] = None
        self._resample = self._device_resample  # the tests swap in a host resampler here

    # ------------------------------------------------------------------ device handle
    def _device_resample(self, particles, log_weights, soft_alpha, gumbel_temperature, seed, epoch, want_entropy):
        """(new_particles (B, N, d), row entropies (B, N) or None) of normalised log-weights."""
        X, lw, _ = _validate(particles, log_weights, soft_alpha, gumbel_temperature, seed, epoch)
        B, N, d = X.shape
        h = self._cached((N, d, B), lambda: _Handle(N, d, B, self.device))
        lp = np.ascontiguousarray(_log_probs(lw, float(soft_alpha)))
        return h.resample(X, lp, gumbel_temperature, seed, epoch, 0, bool(want_entropy))

    # ------------------------------------------------------------------ utilities
    _log_normalize = staticmethod(_log_normalize)

    compute_ess = staticmethod(DC.ess_of_log_weights)

    @staticmethod
    def compute_weight_entropy(log_weights):
        """soft.py:105-124: -sum w log(w + 1e-10), shape (B,)."""
        weights = np.exp(np.asarray(log_weights, dtype=np.float64))
        weights = weights / np.sum(weights, axis=-1, keepdims=True)
        return -np.sum(weights * np.log(weights + 1e-10), axis=-1)

    @staticmethod
    def compute_particle_diversity(particles, block: int = 256):
        """soft.py:126-173 for (B, N, d): mean and standard deviation of the pairwise distances and the
        trace of the population covariance, each of shape (B,).  As in the reference the mean is over
        the N (N - 1) ordered pairs, and the standard deviation over the masked N x N array, its N
        diagonal zeros included.  The distances are formed in row blocks, never as (N, N, d)."""
        P = np.asarray(particles, dtype=np.float64)
        B, N, d = P.shape
        mean_dist, std_dist = np.zeros(B), np.zeros(B)
        for b in range(B):
            total = sum(float(np.sum(dist)) for dist in DC.masked_distance_blocks(P[b], block))
            with np.errstate(divide="ignore", invalid="ignore"):
                mean_dist[b] = np.float64(total) / np.float64(N * (N - 1))
            flat_mean = total / float(N * N)
            sq = sum(float(np.sum(np.square(dist - flat_mean))) for dist in DC.masked_distance_blocks(P[b], block))
            std_dist[b] = np.sqrt(sq / float(N * N))
        centered = P - np.mean(P, axis=1, keepdims=True)
        spread = np.sum(np.mean(np.square(centered), axis=1), axis=-1)
        return {"mean_pairwise_dist": mean_dist, "std_pairwise_dist": std_dist, "particle_spread": spread}

    def _sample_gumbel(self, shape, eps=1e-20):
        """soft.py:175-192: i.i.d. Gumbel(0, 1) draws from ``self.rng``."""
        u = self.rng.uniform(eps, 1.0 - eps, size=tuple(shape))  # [eps, 1): never 0 or 1 in fp64
        return -np.log(-np.log(u))

    def _gumbel_softmax(self, log_probs, temperature):
        """soft.py:194-211: a Gumbel-Softmax sample along the last axis (host utility; ``step`` does
        this on the device)."""
        log_probs = np.asarray(log_probs, dtype=np.float64)
        g = self._sample_gumbel(log_probs.shape)
        z = (log_probs + g) / temperature
        e = np.exp(z - np.max(z, axis=-1, keepdims=True))
        return e / np.sum(e, axis=-1, keepdims=True)

    # ------------------------------------------------------------------ the filter
    def init_particles(self, batch_size, init_mean, init_cov_chol):
        """soft.py:216-261: (B, N, d) draws ``mean + eps @ L`` from ``self.rng`` and log-weights log(1 / N)."""
        return DC.init_particles_batched(self.rng, batch_size, self.n_particles, self.state_dim, init_mean,
                                         init_cov_chol)

    def step(self, particles, log_weights, observation, params=None, return_diagnostics=False):
        """soft.py:266-367: propagate, reweight (host NumPy), soft-resample (device)."""
        if params is None:
            params = {}
        if return_diagnostics:
            ess_before = self.compute_ess(log_weights)
            entropy_before = self.compute_weight_entropy(log_weights)
            diversity_before = self.compute_particle_diversity(particles)

        pred_particles = np.asarray(self.transition_fn(particles, params), dtype=np.float64)
        log_lik = np.asarray(self.log_likelihood_fn(pred_particles, observation, params), dtype=np.float64)
        log_weights = np.asarray(log_weights, dtype=np.float64) + log_lik
        log_weights, _ = self._log_normalize(log_weights, axis=-1, keepdims=False)
        weights = np.exp(log_weights)

        N = self.n_particles
        new_particles, assign_entropy = self._resample(pred_particles, log_weights, self.soft_alpha,
                                                       self.gumbel_temperature, self.seed, self.epoch,
                                                       bool(return_diagnostics))
        self.epoch += 1
        new_log_weights = np.log(np.full((np.shape(particles)[0], N), 1.0 / N))
        if not return_diagnostics:
            return new_particles, new_log_weights
        diagnostics = {
            "ess_before": ess_before,
            "ess_after": self.compute_ess(new_log_weights),
            "entropy_before": entropy_before,
            "entropy_after": self.compute_weight_entropy(new_log_weights),
            "diversity_before": diversity_before,
            "diversity_after": self.compute_particle_diversity(new_particles),
            "assignment_entropy_mean": np.mean(assign_entropy),
            "assignment_entropy_std": np.std(assign_entropy),
            "max_weight_before": np.max(weights, axis=-1),
            "soft_alpha": self.soft_alpha,
            "gumbel_temperature": self.gumbel_temperature,
        }
        return new_particles, new_log_weights, diagnostics

    def filter(self, observations, init_mean, init_cov_chol, params=None, return_diagnostics=False,
               ground_truth=None):
        """soft.py:371-464: the filter over ``observations`` (B, T, obs_dim); returns particles
        (B, T + 1, N, d) and log-weights (B, T + 1, N), the prior draw first."""
        if params is None:
            params = {}
        observations = np.asarray(observations, dtype=np.float64)
        B, T = observations.shape[0], observations.shape[1]
        particles, logw = self.init_particles(batch_size=B, init_mean=init_mean, init_cov_chol=init_cov_chol)
        particles_list, logw_list = [particles], [logw]
        diagnostics_list, times = [], []
        for t in range(T):
            y_t = observations[:, t, :]
            if return_diagnostics:
                start_time = time.time()
                particles, logw, step_diag = self.step(particles, logw, y_t, params=params, return_diagnostics=True)
                end_time = time.time()
                step_diag["step_time"] = end_time - start_time
                times.append(end_time - start_time)
                diagnostics_list.append(step_diag)
            else:
                particles, logw = self.step(particles, logw, y_t, params=params, return_diagnostics=False)
            particles_list.append(particles)
            logw_list.append(logw)
        particles_seq = np.stack(particles_list, axis=1)
        logw_seq = np.stack(logw_list, axis=1)
        if not return_diagnostics:
            return particles_seq, logw_seq
        diagnostics = self._aggregate_diagnostics(diagnostics_list)
        diagnostics["total_time"] = sum(times)
        diagnostics["mean_step_time"] = sum(times) / len(times) if times else 0.0
        if ground_truth is not None:
            ground_truth = np.asarray(ground_truth, dtype=np.float64)
            rmse_seq = self._compute_rmse_sequence(particles_seq, logw_seq, ground_truth)
            diagnostics["rmse_sequence"] = rmse_seq
            diagnostics["mean_rmse"] = np.mean(rmse_seq)
            diagnostics["final_rmse"] = rmse_seq[-1]
        return particles_seq, logw_seq, diagnostics

    def _aggregate_diagnostics(self, diagnostics_list):
        """soft.py:466-511: nested dicts and arrays get mean / std / min / max over the steps, plain
        Python numbers (soft_alpha, gumbel_temperature, step_time) mean and std (population std, as
        reduce_std)."""
        if not diagnostics_list:
            return {}
        aggregated = {}
        for key in diagnostics_list[0].keys():
            values = [d[key] for d in diagnostics_list]
            if isinstance(values[0], dict):
                aggregated[key] = {}
                for subkey in values[0].keys():
                    subvalues = np.stack([np.asarray(v[subkey], dtype=np.float64) for v in values])
                    aggregated[key][subkey + "_mean"] = np.mean(subvalues)
                    aggregated[key][subkey + "_std"] = np.std(subvalues)
                    aggregated[key][subkey + "_min"] = np.min(subvalues)
                    aggregated[key][subkey + "_max"] = np.max(subvalues)
            elif isinstance(values[0], (int, float)) and not isinstance(values[0], np.generic):
                aggregated[key + "_mean"] = sum(values) / len(values)
                aggregated[key + "_std"] = np.std(np.asarray(values, dtype=np.float64))
            else:
                values_arr = np.stack([np.asarray(v, dtype=np.float64) for v in values])
                aggregated[key + "_mean"] = np.mean(values_arr)
                aggregated[key + "_std"] = np.std(values_arr)
                aggregated[key + "_min"] = np.min(values_arr)
                aggregated[key + "_max"] = np.max(values_arr)
        return aggregated

    def _compute_rmse_sequence(self, particles_seq, logw_seq, ground_truth):
        """soft.py:513-547: the error of the weighted mean against ``ground_truth`` (B, T + 1, d),
        root mean square over the batch, shape (T + 1,)."""
        weights = np.exp(np.asarray(logw_seq, dtype=np.float64))
        weights = weights / np.sum(weights, axis=-1, keepdims=True)
        particle_means = np.sum(weights[..., None] * np.asarray(particles_seq, dtype=np.float64), axis=2)
        squared_errors = np.sum((particle_means - ground_truth) ** 2, axis=-1)
        return np.sqrt(np.mean(squared_errors, axis=0))
