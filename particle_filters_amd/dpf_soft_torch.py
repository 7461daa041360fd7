"""PyTorch autograd binding of the soft (Gumbel-Softmax) resampler, and the
``DifferentiableParticleFilter`` whose outputs can be differentiated.

``soft_resample`` is ``dpf_soft.soft_resample`` as a differentiable torch operation
(``SoftResample``, a ``torch.autograd.Function``): the forward pass is ``pf_soft_resample``, the
backward pass ``pf_soft_backward`` (``dpf_soft.soft_resample_vjp``), which regenerates the assignment
matrix from the Philox counters of ``(seed, epoch)`` where autodiff would keep (B, N, N) tensors
alive for every step of a filter.  Gradients flow to the particles and the log-weights;
``soft_alpha`` and the temperature are plain floats.  Double backward is not implemented and raises.

Tensors must be float64 (another dtype is a ``TypeError``) and may live on any device.  Two paths:

* the device path, when the caller asks for it (``device_path=True`` on ``soft_resample`` and on the
  filter's constructor) and every tensor of a call is on the HIP device that computes (``device``): the
  device-pointer entries ``pf_soft_resample_dev`` / ``pf_soft_backward_dev`` run on torch's current
  stream on the tensors where they lie, results and gradients are torch tensors on that device, the
  saved forward results stay there, and the O(B N) chains around the kernels are torch ops.  Nothing
  goes through host memory.  The value checks (finite particles and gradients, no NaN or +inf
  log-weight, a finite log-weight per problem) are torch reductions folded into one scalar that is
  read back, one per call; ``check_values=False`` turns them off, and a step then enqueues and
  returns.  Non-contiguous tensors are made contiguous first;
* the host path, the default, and for anything else (CPU tensors, mixed placement, another GPU): a
  tensor is detached, copied to the CPU, handed to the C ABI as a NumPy array, and the result is
  copied back to the tensor's device.  Tensors on the device then give the bits of CPU tensors
  (tests/test_gpu_dpf_soft_grad.py pins that), which the device path cannot: its O(B N) chains are
  torch's exp, log and sums on the device where the host path's are NumPy's, and the two paths agree
  to 1e-9 of the results' scale, not in every bit.  That is why the device path is asked for and not
  chosen by the tensors' placement alone, as it is in ``dpf_rnn_torch``.

``_dpf_common.PATH_CALLS`` counts the calls per path.

``DifferentiableParticleFilter`` has the constructor of ``dpf_soft.DifferentiableParticleFilter``;
its ``transition_fn(particles, params)`` and ``log_likelihood_fn(particles, observation, params)``
are torch callables on (B, N, d), and everything between them and the resampler is torch, so a
loss on the outputs of ``step`` or ``filter`` backpropagates to every tensor the callables close
over, to ``init_mean`` and to ``init_cov_chol``.

torch is imported by this module, not by the package: ``import particle_filters_amd`` and
``dpf_soft`` work without it.
"""

from __future__ import annotations

import math
import time
from typing import Callable, Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _dpf_common as DC
from . import dpf_soft as SO
from ._dpf_common import HandleCache

__all__ = ["SoftResample", "soft_resample", "DifferentiableParticleFilter"]


def _as_f64(name: str, t) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float64:
        raise TypeError(f"{name} must be float64, got {t.dtype}")
    return t


def _host(t: torch.Tensor) -> np.ndarray:
    return np.ascontiguousarray(t.detach().cpu().numpy())


_VALUE_ERRORS = ("particles must be finite", "log_weights must not hold NaN or +inf",
                 "every problem needs at least one finite log-weight")


def _value_code(particles, log_weights) -> int:
    """``_validate``'s value checks as torch reductions on the tensors' device, folded into one
    scalar, the only value the device path reads back: bit k set when check k of ``_VALUE_ERRORS``
    fails."""
    bad = torch.stack([~torch.isfinite(particles).all(),
                       (torch.isnan(log_weights) | (log_weights == math.inf)).any(),
                       ~torch.isfinite(log_weights).any(dim=-1).all()])
    return int((bad * torch.tensor([1, 2, 4], device=bad.device)).sum().item())


def _stream(device: int) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _log_norm(lw):
    """``_dpf_common.log_normalize`` in torch: the normalised log-weights."""
    m = lw.max(dim=-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    return lw - (m + torch.log(torch.exp(lw - m).sum(dim=-1, keepdim=True)))


class SoftResample(torch.autograd.Function):
    """``new_particles = SoftResample.apply(particles, log_weights, soft_alpha, gumbel_temperature,
    seed, epoch, device, handle)``: (N, d) with (N,), or (B, N, d) with (B, N), float64.  ``ctx`` keeps
    the inputs and the forward pass's ``SoftSaved``; ``backward`` is one ``pf_soft_backward``.

    With ``device_path`` (a class attribute, off in this class) and both tensors on the HIP device
    ``device`` the pass runs on the device path:
    ``pf_soft_resample_dev`` / ``pf_soft_backward_dev`` on torch's current stream, on the tensors where
    they lie, with the saved results kept as device tensors and the O(B N) chains as torch ops; nothing
    goes through host memory.  ``check_values`` (a class attribute; ``soft_resample`` picks the class)
    says whether ``backward`` checks the incoming gradient, which reads one scalar back."""

    device_path = False  # asked for by ``soft_resample(..., device_path=True)``, which picks the class
    check_values = True

    @staticmethod
    def forward(ctx, particles, log_weights, soft_alpha, gumbel_temperature, seed, epoch, device, handle):
        dev = ctx._forward_cls.device_path and DC.on_device((particles, log_weights), device)
        DC.count_path(dev)
        ctx.dev = dev
        if dev:
            return SoftResample._forward_dev(ctx, particles, log_weights, soft_alpha, gumbel_temperature, seed, epoch,
                                             device, handle)
        X, lw = _host(particles), _host(log_weights)
        out, _, saved = SO.soft_resample(X, lw, soft_alpha, gumbel_temperature, seed=seed, epoch=epoch,
                                         return_saved=True, device=device, _handle=handle)
        ctx.save_for_backward(particles, log_weights)
        ctx.soft = (float(soft_alpha), float(gumbel_temperature), int(device), handle, saved)
        return torch.from_numpy(out).to(particles.device)

    @staticmethod
    def _forward_dev(ctx, particles, log_weights, alpha, T, seed, epoch, device, handle):
        batched = particles.ndim == 3
        X = (particles if batched else particles[None]).detach().contiguous()
        lw = (log_weights if batched else log_weights[None]).detach().contiguous()
        B, N, d = X.shape
        lp = torch.log((1.0 - alpha) * torch.exp(_log_norm(lw)) + alpha * (1.0 / N) + 1e-20).contiguous()
        out = torch.empty_like(X)
        M, L = torch.empty_like(lw), torch.empty_like(lw)
        h = handle
        own = h is None or h.h is None or h.key() != (N, d, B)
        if own:
            h = SO._Handle(N, d, B, device)
        try:
            h.resample_dev(_stream(device), X.data_ptr(), lp.data_ptr(), T, seed, epoch, 0, out.data_ptr(), 0,
                           M.data_ptr(), L.data_ptr())
        finally:
            if own:
                h.close()  # waits for the call: the outputs are the caller's, the scratch the handle's
        ctx.save_for_backward(particles, log_weights, out)  # the saved results stay device tensors
        ctx.soft = (float(alpha), float(T), int(device), handle, (M, L, int(seed), int(epoch)))
        return out if batched else out[0]

    @staticmethod
    def _backward_dev(ctx, grad_new_particles):
        particles, log_weights, Xo = ctx.saved_tensors
        alpha, T, device, handle, (M, L, seed, epoch) = ctx.soft
        batched = particles.ndim == 3
        X = (particles if batched else particles[None]).detach().contiguous()
        lw = (log_weights if batched else log_weights[None]).detach().contiguous()
        g = (grad_new_particles if batched else grad_new_particles[None]).contiguous()
        B, N, d = X.shape
        if ctx._forward_cls.check_values and not bool(torch.isfinite(g).all().item()):
            raise ValueError("grad_new_particles must be finite")
        w = torch.exp(_log_norm(lw))
        q = (1.0 - alpha) * w + alpha * (1.0 / N)
        lp = torch.log(q + 1e-20).contiguous()
        gX, glp = torch.empty_like(X), torch.empty_like(lw)
        h = handle
        own = h is None or h.h is None or h.key() != (N, d, B)
        if own:
            h = SO._Handle(N, d, B, device)
        try:
            h.backward_dev(_stream(device), X.data_ptr(), lp.data_ptr(), T, seed, epoch, 0, Xo.data_ptr(), M.data_ptr(),
                           L.data_ptr(), g.data_ptr(), gX.data_ptr(), glp.data_ptr())
        finally:
            if own:
                h.close()
        # dpf_soft._log_weights_grad: through log((1 - alpha) w + alpha / N + 1e-20) and the normalisation
        u = ((1.0 - alpha) * glp / (q + 1e-20)) * w
        glw = u - w * u.sum(dim=-1, keepdim=True)
        gX = (gX if batched else gX[0]) if ctx.needs_input_grad[0] else None
        glw = (glw if batched else glw[0]) if ctx.needs_input_grad[1] else None
        return gX, glw, None, None, None, None, None, None

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_new_particles):
        if ctx.dev:
            return SoftResample._backward_dev(ctx, grad_new_particles)
        particles, log_weights = ctx.saved_tensors
        alpha, T, device, handle, saved = ctx.soft
        gX, glw = SO.soft_resample_vjp(_host(particles), _host(log_weights), _host(grad_new_particles), alpha, T,
                                       seed=saved.seed, epoch=saved.epoch, saved=saved, device=device, _handle=handle)
        gX = torch.from_numpy(gX).to(particles.device) if ctx.needs_input_grad[0] else None
        glw = torch.from_numpy(glw).to(log_weights.device) if ctx.needs_input_grad[1] else None
        return gX, glw, None, None, None, None, None, None


class _SoftResampleDevice(SoftResample):
    device_path = True


class _SoftResampleDeviceUnchecked(_SoftResampleDevice):
    check_values = False


def _validate_dev(particles, log_weights, soft_alpha, gumbel_temperature, seed, epoch, check_values) -> None:
    """``dpf_soft._validate`` for tensors on the device: the shapes and the scalars from metadata, in
    its order and with its messages; the values by ``_value_code``, one scalar read back."""
    DC.check_batched_shapes(particles.shape, log_weights.shape, "log_weights", SO.MAX_BATCH)
    if check_values:
        DC.raise_first(_value_code(particles, log_weights), _VALUE_ERRORS)
    if not (0.0 <= float(soft_alpha) <= 1.0):
        raise ValueError(f"soft_alpha must be in [0, 1], got {soft_alpha}")
    DC.check_positive("gumbel_temperature", gumbel_temperature)
    DC.check_seed(seed)
    DC.check_epoch(epoch)


def soft_resample(particles, log_weights, soft_alpha=0.1, gumbel_temperature=0.2, *, seed=0, epoch=0, device=0,
                  device_path=False, check_values=True, _handle: Optional[SO._Handle] = None):
    """``dpf_soft.soft_resample`` on float64 tensors, differentiable with respect to ``particles`` and
    ``log_weights``: returns ``(new_particles, new_log_weights)``, the new log-weights being the
    constant ``log(1 / N)``.  ``device`` is the HIP device that computes.  With ``device_path=True``,
    tensors that are both on that device take the device path (see the module's docstring): the
    results are tensors there, and with ``check_values=False`` the call enqueues and returns without
    reading anything back (the values are then the caller's responsibility: a NaN goes through the
    kernels as a NaN).  Without it, and for any other placement, the data goes through host memory,
    whichever device the tensors are on, and tensors on the device give the bits of CPU tensors;
    ``check_values`` has no effect there."""
    particles = _as_f64("particles", particles)
    log_weights = _as_f64("log_weights", log_weights)
    if isinstance(soft_alpha, torch.Tensor) or isinstance(gumbel_temperature, torch.Tensor):
        raise TypeError("soft_alpha and gumbel_temperature are plain floats: there is no gradient with respect to them")
    if device_path and DC.on_device((particles, log_weights), device):
        _validate_dev(particles, log_weights, soft_alpha, gumbel_temperature, seed, epoch, check_values)
    else:
        SO._validate(_host(particles), _host(log_weights), soft_alpha, gumbel_temperature, seed, epoch)
    fn = SoftResample if not device_path else _SoftResampleDevice if check_values else _SoftResampleDeviceUnchecked
    new = fn.apply(particles, log_weights, float(soft_alpha), float(gumbel_temperature), int(seed), int(epoch),
                   int(device), _handle)
    N = particles.shape[-2]
    new_lw = torch.full(log_weights.shape, math.log(1.0 / float(N)), dtype=torch.float64, device=log_weights.device)
    return new, new_lw


class DifferentiableParticleFilter(HandleCache):
    """Particle filter with soft resampling at every step (soft.py:8-547) on torch tensors, with
    gradients.  ``init_particles``, ``step`` and ``filter`` follow ``dpf_soft``'s conventions: the
    draws of a step are those of ``(self.seed, self.epoch)``, the epoch advances by one when a step
    succeeds, and the shapes returned are the same.  ``init_particles`` draws from ``rng`` (a NumPy
    generator, as in ``dpf_soft``).  Diagnostics are computed by ``dpf_soft``'s class on detached
    values and are NumPy numbers."""

    def __init__(self, n_particles, state_dim, transition_fn: Callable, log_likelihood_fn: Callable, soft_alpha=0.1,
                 gumbel_temperature=0.2, name=None, *, seed=0, rng: Optional[np.random.Generator] = None, device=0,
                 device_path=False, check_values=True):
        self.device_path = bool(device_path)    # soft_resample's: the device path for tensors on the device
        self.check_values = bool(check_values)  # of the device path
        # the NumPy class checks the arguments and owns the diagnostics; its callables are never called
        self._np = SO.DifferentiableParticleFilter(n_particles, state_dim, transition_fn, log_likelihood_fn,
                                                   soft_alpha, gumbel_temperature, name, seed=seed, rng=rng,
                                                   device=device)
        self.name = name
        self.n_particles, self.state_dim = self._np.n_particles, self._np.state_dim
        self.transition_fn = transition_fn
        self.log_likelihood_fn = log_likelihood_fn
        self.soft_alpha = soft_alpha
        self.gumbel_temperature = gumbel_temperature
        self.seed = self._np.seed
        self.epoch = 0
        self.rng = self._np.rng
        self.device = int(device)
        self._h: Optional[SO._Handle] = None

    def _handle(self, B: int) -> SO._Handle:
        N, d = self.n_particles, self.state_dim
        return self._cached((N, d, B), lambda: SO._Handle(N, d, B, self.device))

    def init_particles(self, batch_size, init_mean, init_cov_chol):
        """soft.py:216-261: (B, N, d) draws ``mean + eps @ L`` with eps from ``self.rng``, differentiable
        with respect to ``init_mean`` and ``init_cov_chol``, and log-weights log(1 / N)."""
        N, d = self.n_particles, self.state_dim
        B = int(batch_size)
        init_mean = torch.as_tensor(init_mean, dtype=torch.float64)
        init_cov_chol = torch.as_tensor(init_cov_chol, dtype=torch.float64, device=init_mean.device)
        if init_mean.ndim == 1:
            init_mean = init_mean[None, :].expand(B, d)
        if init_cov_chol.ndim == 2:
            init_cov_chol = init_cov_chol[None, :, :].expand(B, d, d)
        eps = torch.from_numpy(self.rng.standard_normal((B, N, d))).to(init_mean.device)
        particles = init_mean[:, None, :] + torch.einsum("bnd,bdk->bnk", eps, init_cov_chol)
        log_weights = torch.full((B, N), math.log(1.0 / N), dtype=torch.float64, device=init_mean.device)
        return particles, log_weights

    def step(self, particles, log_weights, observation, params=None, return_diagnostics=False):
        """soft.py:266-367: propagate and reweight (the user's torch callables), soft-resample (device)."""
        if params is None:
            params = {}
        particles = _as_f64("particles", particles)
        log_weights = _as_f64("log_weights", log_weights)
        F = SO.DifferentiableParticleFilter
        if return_diagnostics:
            ess_before = F.compute_ess(_host(log_weights))
            entropy_before = F.compute_weight_entropy(_host(log_weights))
            diversity_before = F.compute_particle_diversity(_host(particles))

        pred = _as_f64("transition_fn's result", self.transition_fn(particles, params))
        log_lik = _as_f64("log_likelihood_fn's result", self.log_likelihood_fn(pred, observation, params))
        log_weights = log_weights + log_lik
        log_weights = log_weights - torch.logsumexp(log_weights, dim=-1, keepdim=True)

        # the arguments are checked before a handle is made
        dev = self.device_path and DC.on_device((pred, log_weights), self.device)
        if dev:  # the values are checked by soft_resample, in its one readback
            _validate_dev(pred, log_weights, self.soft_alpha, self.gumbel_temperature, self.seed, self.epoch, False)
        else:
            SO._validate(_host(pred), _host(log_weights), self.soft_alpha, self.gumbel_temperature, self.seed,
                         self.epoch)
        new_particles, new_log_weights = soft_resample(pred, log_weights, self.soft_alpha, self.gumbel_temperature,
                                                       seed=self.seed, epoch=self.epoch, device=self.device,
                                                       device_path=self.device_path,
                                                       check_values=self.check_values,
                                                       _handle=self._handle(int(pred.shape[0])))
        assign_entropy = None
        if return_diagnostics:  # a second forward pass on detached values, with the row entropies
            assign_entropy = SO.soft_resample(_host(pred), _host(log_weights), self.soft_alpha,
                                              self.gumbel_temperature, seed=self.seed, epoch=self.epoch,
                                              return_diagnostics=True, device=self.device, _handle=self._h)[2]
        self.epoch += 1
        if not return_diagnostics:
            return new_particles, new_log_weights
        nlw = _host(new_log_weights)
        diagnostics = {
            "ess_before": ess_before,
            "ess_after": F.compute_ess(nlw),
            "entropy_before": entropy_before,
            "entropy_after": F.compute_weight_entropy(nlw),
            "diversity_before": diversity_before,
            "diversity_after": F.compute_particle_diversity(_host(new_particles)),
            "assignment_entropy_mean": np.mean(assign_entropy),
            "assignment_entropy_std": np.std(assign_entropy),
            "max_weight_before": np.max(np.exp(_host(log_weights)), axis=-1),
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
        observations = torch.as_tensor(observations, dtype=torch.float64)
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
        particles_seq = torch.stack(particles_list, dim=1)
        logw_seq = torch.stack(logw_list, dim=1)
        if not return_diagnostics:
            return particles_seq, logw_seq
        diagnostics = self._np._aggregate_diagnostics(diagnostics_list)
        diagnostics["total_time"] = sum(times)
        diagnostics["mean_step_time"] = sum(times) / len(times) if times else 0.0
        if ground_truth is not None:
            truth = np.asarray(ground_truth.detach().cpu() if isinstance(ground_truth, torch.Tensor) else ground_truth,
                               dtype=np.float64)
            rmse_seq = self._np._compute_rmse_sequence(_host(particles_seq), _host(logw_seq), truth)
            diagnostics["rmse_sequence"] = rmse_seq
            diagnostics["mean_rmse"] = np.mean(rmse_seq)
            diagnostics["final_rmse"] = rmse_seq[-1]
        return particles_seq, logw_seq, diagnostics
