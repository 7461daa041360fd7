"""PyTorch autograd binding of the Sinkhorn OT resampler, and the ``DPF_OT`` filter whose outputs
can be differentiated.

``sinkhorn_ot_resample`` is ``dpf_ot.sinkhorn_ot_resample`` as a differentiable torch operation
(``SinkhornResample``, a ``torch.autograd.Function``): the forward pass is ``pf_ot_resample`` with
its dual history kept (``OtSaved``), the backward pass ``pf_ot_backward``
(``dpf_ot.sinkhorn_ot_resample_vjp``), the reverse sweep over the iterations with the plan
recomputed, where autodiff of the unrolled loop would keep about 4 K matrices of N x N alive for
every step of a filter.  Gradients flow to the particles and the weights; ``epsilon`` is a plain
float.  Double backward is not implemented and raises.

Tensors must be float64 (another dtype is a ``TypeError``) and may live on any device.  In this
version the data goes through host memory: a tensor is detached, copied to the CPU, handed to the
C ABI as a NumPy array, and the result is copied back to the tensor's device.

``DPF_OT`` has the constructor of ``dpf_ot.DPF_OT``; its ``transition_fn(particles, t)`` and
``obs_loglik_fn(particles, y_t, t)`` are torch callables on (N, d), and everything between them
and the resampler is torch (ot.py:400-556), so a loss on the outputs of ``step`` or ``run_filter``
backpropagates to every tensor the callables close over, to ``mean0`` and to ``cov0_chol``.

torch is imported by this module, not by the package: ``import particle_filters_amd`` and
``dpf_ot`` work without it.
"""

from __future__ import annotations

import time
from typing import Callable, Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import dpf_ot as OT
from ._dpf_common import HandleCache

__all__ = ["SinkhornResample", "sinkhorn_ot_resample", "DPF_OT"]


def _as_f64(name: str, t) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float64:
        raise TypeError(f"{name} must be float64, got {t.dtype}")
    return t


def _host(t: torch.Tensor) -> np.ndarray:
    return np.ascontiguousarray(t.detach().cpu().numpy())


class SinkhornResample(torch.autograd.Function):
    """``new_particles = SinkhornResample.apply(particles, weights, epsilon, n_iters, min_val, tol,
    device, handle)``: (N, d) with (N,), or (B, N, d) with (B, N), float64.  ``ctx`` keeps the inputs
    and the forward pass's ``OtSaved``; ``backward`` is one ``pf_ot_backward``."""

    @staticmethod
    def forward(ctx, particles, weights, epsilon, n_iters, min_val, tol, device, handle):
        out, _, saved = OT.sinkhorn_ot_resample(_host(particles), _host(weights), epsilon, n_iters, min_val, tol,
                                                return_saved=True, device=device, _handle=handle)
        ctx.save_for_backward(particles, weights)
        ctx.ot = (float(epsilon), int(n_iters), float(min_val), float(tol), int(device), handle, saved)
        return torch.from_numpy(out).to(particles.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_new_particles):
        particles, weights = ctx.saved_tensors
        epsilon, n_iters, min_val, tol, device, handle, saved = ctx.ot
        gX, gw = OT.sinkhorn_ot_resample_vjp(_host(particles), _host(weights), _host(grad_new_particles), epsilon,
                                             n_iters, min_val, tol, saved=saved, device=device, _handle=handle)
        gX = torch.from_numpy(gX).to(particles.device) if ctx.needs_input_grad[0] else None
        gw = torch.from_numpy(gw).to(weights.device) if ctx.needs_input_grad[1] else None
        return gX, gw, None, None, None, None, None, None


def sinkhorn_ot_resample(particles, weights, epsilon=0.1, n_iters=50, min_val=1e-12, tol=1e-6, *, device=0,
                         _handle: Optional[OT._Handle] = None):
    """``dpf_ot.sinkhorn_ot_resample`` on float64 tensors, differentiable with respect to
    ``particles`` and ``weights``: returns ``(new_particles, new_weights)``, the new weights being
    the constant 1 / N.  ``device`` is the HIP device that computes, whichever device the tensors are
    on; the data goes through host memory (see the module's docstring)."""
    particles = _as_f64("particles", particles)
    weights = _as_f64("weights", weights)
    if isinstance(epsilon, torch.Tensor):
        raise TypeError("epsilon is a plain float: there is no gradient with respect to it")
    OT._validate(_host(particles), _host(weights), epsilon, n_iters)
    new = SinkhornResample.apply(particles, weights, float(epsilon), int(n_iters), float(min_val), float(tol),
                                 int(device), _handle)
    N = particles.shape[-2]
    new_w = torch.full(weights.shape, 1.0 / float(N), dtype=torch.float64, device=weights.device)
    return new, new_w


class DPF_OT(HandleCache):
    """Particle filter with OT resampling at every step (ot.py:238-634) on torch tensors, with
    gradients.  ``init_particles``, ``step`` and ``run_filter`` follow ``dpf_ot.DPF_OT``'s
    conventions and return the same shapes.  ``init_particles`` draws from ``rng`` (a NumPy
    generator, as in ``dpf_ot``).  Diagnostics are computed by ``dpf_ot``'s class on detached values
    and are NumPy numbers."""

    def __init__(self, N_particles, state_dim, transition_fn: Callable, obs_loglik_fn: Callable, epsilon=0.1,
                 sinkhorn_iters=50, name=None, *, rng: Optional[np.random.Generator] = None, device=0):
        # the NumPy class checks the arguments and owns the diagnostics; its callables are never called
        self._np = OT.DPF_OT(N_particles, state_dim, transition_fn, obs_loglik_fn, epsilon, sinkhorn_iters, name,
                             rng=rng, device=device)
        self.name = name
        self.N, self.d = self._np.N, self._np.d
        self.transition_fn = transition_fn
        self.obs_loglik_fn = obs_loglik_fn
        self.epsilon = epsilon
        self.sinkhorn_iters = sinkhorn_iters
        self.rng = self._np.rng
        self.device = int(device)
        self._h: Optional[OT._Handle] = None

    def _handle(self) -> OT._Handle:
        return self._cached((self.N, self.d, 1), lambda: OT._Handle(self.N, self.d, 1, self.device))

    def init_particles(self, mean, cov_chol):
        """ot.py:374-398: N draws ``mean + eps @ cov_chol^T`` with eps from ``self.rng``, differentiable
        with respect to ``mean`` and ``cov_chol``, and weights 1 / N."""
        mean = torch.as_tensor(mean, dtype=torch.float64)
        cov_chol = torch.as_tensor(cov_chol, dtype=torch.float64, device=mean.device)
        eps = torch.from_numpy(self.rng.standard_normal((self.N, self.d))).to(mean.device)
        particles = mean[None, :] + eps @ cov_chol.T
        weights = torch.full((self.N,), 1.0 / float(self.N), dtype=torch.float64, device=mean.device)
        return particles, weights

    def step(self, particles, weights, y_t, t=None, return_diagnostics=False):
        """ot.py:400-487: propagate and reweight (the user's torch callables), resample (device)."""
        particles = _as_f64("particles", particles)
        weights = _as_f64("weights", weights)
        F = OT.DPF_OT
        if return_diagnostics:
            start_time = time.time()
            ess_before = F.compute_ess(_host(weights))
            entropy_before = F.compute_weight_entropy(_host(weights))
            diversity_before = F.compute_particle_diversity(_host(particles))

        pred = _as_f64("transition_fn's result", self.transition_fn(particles, t))
        log_liks = _as_f64("obs_loglik_fn's result", self.obs_loglik_fn(pred, y_t, t))

        # ot.py:438-445
        unnorm_w = torch.clamp(weights * torch.exp(log_liks), min=0.0)
        new_weights = unnorm_w / (torch.sum(unnorm_w) + 1e-12)

        # the arguments are checked before a handle is made
        OT._validate(_host(pred), _host(new_weights), self.epsilon, self.sinkhorn_iters)
        res_particles, res_weights = sinkhorn_ot_resample(pred, new_weights, self.epsilon, self.sinkhorn_iters,
                                                          device=self.device, _handle=self._handle())
        if not return_diagnostics:
            return res_particles, res_weights
        # a second forward pass on detached values, with the resampler's diagnostics
        resample_diag = OT.sinkhorn_ot_resample(_host(pred), _host(new_weights), self.epsilon, self.sinkhorn_iters,
                                                return_diagnostics=True, device=self.device, _handle=self._h)[2]
        diagnostics = {
            "ess_before": ess_before,
            "ess_after": F.compute_ess(_host(res_weights)),
            "entropy_before": entropy_before,
            "entropy_after": F.compute_weight_entropy(_host(res_weights)),
            "diversity_before": diversity_before,
            "diversity_after": F.compute_particle_diversity(_host(res_particles)),
            "max_weight_before": np.max(_host(new_weights)),
            "step_time": time.time() - start_time,
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
        diagnostics = self._np._aggregate_diagnostics(diagnostics_list)
        diagnostics["total_time"] = sum(times)
        diagnostics["mean_step_time"] = sum(times) / len(times) if times else 0.0
        if ground_truth is not None:
            truth = np.asarray(ground_truth.detach().cpu() if isinstance(ground_truth, torch.Tensor) else ground_truth,
                               dtype=np.float64)
            rmse_seq = self._np._compute_rmse_sequence([_host(p) for p in particles_seq],
                                                       [_host(w) for w in weights_seq], truth)
            diagnostics["rmse_sequence"] = rmse_seq
            diagnostics["mean_rmse"] = np.mean(rmse_seq)
            diagnostics["final_rmse"] = rmse_seq[-1]
        return particles_seq, weights_seq, diagnostics
