"""PyTorch autograd binding of the RNN resampler, and the ``DifferentiableParticleFilterRNN`` whose
network can be trained.

``rnn_resample`` is ``dpf_rnn.rnn_resample`` as a differentiable torch operation (``RnnResample``, a
``torch.autograd.Function``): the forward pass is ``pf_rnn_resample``, the backward pass
``pf_rnn_backward`` (``dpf_rnn.rnn_resample_vjp``), which runs the recurrences again on the device,
keeping every hidden state, and back-propagates through the N timesteps of the N sequences there.
Gradients flow to the particles, the log-weights and every weight tensor, through both results, the
new particles and the assignment matrix; the temperature is a plain float.  Double backward is not
implemented and raises.

Tensors must be float64 (another dtype is a ``TypeError``) and may live on any device.  Two paths:

* the device path, when every tensor of a call - particles, log-weights and the network - is on the
  HIP device that computes (``device``; ``DifferentiableParticleFilterRNN.to("cuda")`` moves the
  network): the device-pointer entries ``pf_rnn_resample_dev`` / ``pf_rnn_backward_dev`` run on torch's
  current stream on the tensors where they lie, results and gradients are torch tensors on that
  device, and ``exp(log_weights)`` and its chain rule are torch ops.  The network is packed on the
  device (``pf_rnn_set_weights_dev``) and only when a parameter's storage or version changed: once
  for a filter with frozen weights, once per optimizer step in training.  Nothing goes through host
  memory.  The value checks (finite particles, weights and gradients, no NaN or +inf log-weight, a
  finite log-weight per problem) are torch reductions folded into one scalar that is read back, one
  per call; ``check_values=False`` turns them off, and a step then enqueues and returns.
  Non-contiguous tensors are made contiguous first;
* the host path, for anything else (CPU tensors, mixed placement, another GPU): a tensor is detached,
  copied to the CPU, handed to the C ABI as a NumPy array, and the result is copied back to the
  tensor's device.

``_dpf_common.PATH_CALLS`` counts the calls per path.

``DifferentiableParticleFilterRNN`` has the constructor and the return tuples of
``dpf_rnn.DifferentiableParticleFilterRNN``; its ``transition_fn(particles, params)`` and
``log_likelihood_fn(particles, observation, params)`` are torch callables on (B, N, d), and the
network is a list of ``torch.nn.Parameter`` in Keras' ``get_weights()`` order, so
``torch.optim.Adam(dpf.parameters())`` trains it.  A loss on the outputs of ``step`` or ``filter``
backpropagates to the parameters, to every tensor the callables close over, to ``init_mean`` and to
``init_cov_chol``.  The baseline resampler (``use_baseline_resampling=True``) has no backward pass:
the constructor raises.

torch is imported by this module, not by the package: ``import particle_filters_amd`` and
``dpf_rnn`` work without it.
"""

from __future__ import annotations

import math
from typing import Callable, List, Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _dpf_common as DC
from . import dpf_rnn as RN
from ._dpf_common import HandleCache

__all__ = ["RnnResample", "rnn_resample", "DifferentiableParticleFilterRNN"]


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


def _value_code(particles, log_weights, weights) -> int:
    """The value checks of ``dpf_rnn._validate`` and ``_check_weights`` as torch reductions on the
    tensors' device, folded into one scalar, the only value the device path reads back: bit k for
    check k of ``_VALUE_ERRORS``, bit 3 + k for a weight array k that is not finite."""
    bad = [~torch.isfinite(particles).all(), (torch.isnan(log_weights) | (log_weights == math.inf)).any(),
           ~torch.isfinite(log_weights).any(dim=-1).all()] + [~torch.isfinite(a).all() for a in weights]
    bits = torch.tensor([1 << k for k in range(len(bad))], device=particles.device)
    return int((torch.stack(bad) * bits).sum().item())


def _stream(device: int) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _pack(h: RN._Handle, device: int, weights) -> None:
    """The network on the device, packed by ``pf_rnn_set_weights_dev`` - only when the parameters
    changed: the handle's packed state is keyed on every tensor's storage and version, so a filter
    over T steps with frozen weights packs once and a training loop once per optimizer step."""
    W = [a.detach().contiguous() for a in weights]
    key = tuple((a.data_ptr(), a._version) for a in W)
    h.set_weights_dev(_stream(device), [a.data_ptr() for a in W], [a.numel() for a in W], key)


class RnnResample(torch.autograd.Function):
    """``new_particles, A = RnnResample.apply(particles, log_weights, rnn_type, temperature, use_weight,
    use_particle, device, handle, *weights)``: (N, d) with (N,), or (B, N, d) with (B, N), float64.
    ``ctx`` keeps the inputs; ``backward`` is one ``pf_rnn_backward`` at them.

    When every tensor is on the HIP device ``device`` the pass runs on the device path:
    ``pf_rnn_set_weights_dev`` (when the parameters changed), ``pf_rnn_resample_dev`` and
    ``pf_rnn_backward_dev`` on torch's current stream, on the tensors where they lie; nothing goes
    through host memory.  ``check_values`` (a class attribute; ``rnn_resample`` picks the class) says
    whether ``backward`` checks the incoming gradients, which reads one scalar back."""

    check_values = True

    @staticmethod
    def forward(ctx, particles, log_weights, rnn_type, temperature, use_weight, use_particle, device, handle,
                *weights):
        ctx.dev = DC.on_device((particles, log_weights, *weights), device)
        DC.count_path(ctx.dev)
        if ctx.dev:
            return RnnResample._forward_dev(ctx, particles, log_weights, rnn_type, temperature, use_weight,
                                            use_particle, device, handle, weights)
        out, A = RN.rnn_resample(_host(particles), _host(log_weights), [_host(a) for a in weights], rnn_type,
                                 temperature, use_weight_features=use_weight, use_particle_features=use_particle,
                                 device=device, _handle=handle)
        ctx.save_for_backward(particles, log_weights, *weights)
        ctx.rnn = (rnn_type, float(temperature), bool(use_weight), bool(use_particle), int(device), handle)
        return torch.from_numpy(out).to(particles.device), torch.from_numpy(A).to(particles.device)

    @staticmethod
    def _handle_for(handle, X, weights, rnn_type, use_weight, use_particle, device):
        """(handle, own): ``handle`` if it fits these shapes, otherwise one of the call's own."""
        B, N, d = X.shape
        H, L = int(weights[1].shape[0]), (len(weights) - 2) // 3
        key = (N, d, B, H, L, rnn_type, bool(use_weight), bool(use_particle))
        if handle is not None and handle.h is not None and handle.key() == key:
            return handle, False
        return RN._Handle(N, d, B, H, L, rnn_type, use_weight, use_particle, device), True

    @staticmethod
    def _forward_dev(ctx, particles, log_weights, rnn_type, temperature, use_weight, use_particle, device, handle,
                     weights):
        batched = particles.ndim == 3
        X = (particles if batched else particles[None]).detach().contiguous()
        lw = (log_weights if batched else log_weights[None]).detach()
        B, N, d = X.shape
        w = torch.exp(lw).contiguous()
        out, A = torch.empty_like(X), torch.empty((B, N, N), dtype=torch.float64, device=X.device)
        h, own = RnnResample._handle_for(handle, X, weights, rnn_type, use_weight, use_particle, device)
        try:
            _pack(h, device, weights)
            h.resample_dev(_stream(device), X.data_ptr(), w.data_ptr(), temperature, out.data_ptr(), A.data_ptr(), 0)
        finally:
            if own:
                h.close()  # waits for the call: the outputs are the caller's, the scratch the handle's
        ctx.save_for_backward(particles, log_weights, *weights)
        ctx.rnn = (rnn_type, float(temperature), bool(use_weight), bool(use_particle), int(device), handle)
        return (out, A) if batched else (out[0], A[0])

    @staticmethod
    def _backward_dev(ctx, grad_new_particles, grad_assignment):
        particles, log_weights, *weights = ctx.saved_tensors
        rnn_type, T, use_weight, use_particle, device, handle = ctx.rnn
        batched = particles.ndim == 3
        X = (particles if batched else particles[None]).detach().contiguous()
        lw = (log_weights if batched else log_weights[None]).detach()
        g = (grad_new_particles if batched else grad_new_particles[None]).contiguous()
        gA = (grad_assignment if batched else grad_assignment[None]).contiguous()
        B, N, d = X.shape
        if ctx._forward_cls.check_values:
            code = int((torch.stack([~torch.isfinite(g).all(), ~torch.isfinite(gA).all()]) *
                        torch.tensor([1, 2], device=g.device)).sum().item())
            DC.raise_first(code, ("grad_new_particles must be finite", "grad_assignment must be finite"))
        w = torch.exp(lw).contiguous()
        gX, gw = torch.empty_like(X), torch.empty_like(w)
        gW = [torch.empty_like(a, memory_format=torch.contiguous_format) for a in weights]
        h, own = RnnResample._handle_for(handle, X, weights, rnn_type, use_weight, use_particle, device)
        try:
            _pack(h, device, weights)
            h.backward_dev(_stream(device), X.data_ptr(), w.data_ptr(), T, g.data_ptr(), gA.data_ptr(), gX.data_ptr(),
                           gw.data_ptr(), [a.data_ptr() for a in gW], [a.numel() for a in gW])
        finally:
            if own:
                h.close()
        glw = torch.where(w > 0.0, gw * w, torch.zeros_like(w))  # a log-weight of -inf gets exactly 0
        need = ctx.needs_input_grad
        gX = (gX if batched else gX[0]) if need[0] else None
        glw = (glw if batched else glw[0]) if need[1] else None
        gW = [a if n else None for a, n in zip(gW, need[8:])]
        return (gX, glw, None, None, None, None, None, None, *gW)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_new_particles, grad_assignment):
        if ctx.dev:
            return RnnResample._backward_dev(ctx, grad_new_particles, grad_assignment)
        particles, log_weights, *weights = ctx.saved_tensors
        rnn_type, T, use_weight, use_particle, device, handle = ctx.rnn
        gX, glw, gW = RN.rnn_resample_vjp(_host(particles), _host(log_weights), [_host(a) for a in weights],
                                          _host(grad_new_particles), _host(grad_assignment), rnn_type, T,
                                          use_weight_features=use_weight, use_particle_features=use_particle,
                                          device=device, _handle=handle)
        need = ctx.needs_input_grad
        gX = torch.from_numpy(gX).to(particles.device) if need[0] else None
        glw = torch.from_numpy(glw).to(log_weights.device) if need[1] else None
        gW = [torch.from_numpy(g).to(a.device) if n else None for g, a, n in zip(gW, weights, need[8:])]
        return (gX, glw, None, None, None, None, None, None, *gW)


class _RnnResampleUnchecked(RnnResample):
    check_values = False


def _validate_dev(particles, log_weights, weights, rnn_type, temperature, use_weight_features, use_particle_features,
                  check_values) -> None:
    """``dpf_rnn._validate`` and ``_network`` for tensors on the device: the shapes and the scalars
    from metadata, in their order and with their messages; the values by ``_value_code``, one scalar
    read back."""
    DC.check_batched_shapes(particles.shape, log_weights.shape, "log_weights", RN.MAX_BATCH, batch_range=True,
                            max_pairs=RN.MAX_PAIRS)
    code = _value_code(particles, log_weights, weights) if check_values else 0
    DC.raise_first(code, _VALUE_ERRORS)
    DC.check_positive("temperature", temperature)
    N, d = particles.shape[-2:]
    RN._network_of_shapes([a.shape for a in weights], N, d, rnn_type, use_weight_features, use_particle_features)
    DC.raise_first(code >> 3, [f"weight array {k} must be finite" for k in range(len(weights))])


def rnn_resample(particles, log_weights, weights, rnn_type="lstm", temperature=1.0, *, use_weight_features=True,
                 use_particle_features=True, device=0, check_values=True, _handle: Optional[RN._Handle] = None):
    """``dpf_rnn.rnn_resample`` on float64 tensors, differentiable with respect to ``particles``,
    ``log_weights`` and every tensor of ``weights``: returns ``(new_particles, assignment_probs)``.
    ``device`` is the HIP device that computes.  Tensors that are all on that device take the device
    path (see the module's docstring): the results are tensors there, and with ``check_values=False``
    the call enqueues and returns without reading anything back (the values are then the caller's
    responsibility: a NaN goes through the kernels as a NaN).  Any other placement goes through host
    memory, where ``check_values`` has no effect."""
    particles = _as_f64("particles", particles)
    log_weights = _as_f64("log_weights", log_weights)
    weights = [_as_f64(f"weight array {k}", a) for k, a in enumerate(weights)]
    if isinstance(temperature, torch.Tensor):
        raise TypeError("temperature is a plain float: there is no gradient with respect to it")
    if DC.on_device((particles, log_weights, *weights), device):
        _validate_dev(particles, log_weights, weights, rnn_type, temperature, use_weight_features,
                      use_particle_features, check_values)
    else:
        X, _, _ = RN._validate(_host(particles), _host(log_weights), temperature)  # before the library is loaded
        RN._network([_host(a) for a in weights], X.shape[1], X.shape[2], rnn_type, use_weight_features,
                    use_particle_features)
    fn = RnnResample if check_values else _RnnResampleUnchecked
    return fn.apply(particles, log_weights, str(rnn_type).lower(), float(temperature), bool(use_weight_features),
                    bool(use_particle_features), int(device), _handle, *weights)


class DifferentiableParticleFilterRNN(HandleCache):
    """Particle filter with RNN resampling at every step (rnn.py:9-638) on torch tensors, with
    gradients: the constructor, ``init_particles``, ``step`` and ``filter`` of
    ``dpf_rnn.DifferentiableParticleFilterRNN`` with the same shapes returned.  ``init_particles`` and
    the default initialisation of the network draw from ``rng`` (a NumPy generator, as in ``dpf_rnn``).
    The statistics of ``return_ess`` are computed by ``dpf_rnn``'s class on detached values and are
    NumPy numbers."""

    def __init__(self, n_particles, state_dim, transition_fn: Callable, log_likelihood_fn: Callable, rnn_type="lstm",
                 rnn_hidden_dim=64, rnn_num_layers=1, use_weight_features=True, use_particle_features=True,
                 temperature=1.0, use_baseline_resampling=False, name=None, *, weights=None,
                 rng: Optional[np.random.Generator] = None, seed=0, device=0, check_values=True):
        self.check_values = bool(check_values)  # of the device path (rnn_resample)
        if use_baseline_resampling:
            raise ValueError("use_baseline_resampling=True has no backward pass (there is no pf_rnn_baseline "
                             "gradient): use dpf_rnn.DifferentiableParticleFilterRNN for the baseline resampler")
        if weights is not None:
            weights = [_host(a) if isinstance(a, torch.Tensor) else a for a in weights]
        # the NumPy class checks the arguments, initialises the network and owns the statistics; its
        # callables are never called
        self._np = RN.DifferentiableParticleFilterRNN(
            n_particles, state_dim, transition_fn, log_likelihood_fn, rnn_type, rnn_hidden_dim, rnn_num_layers,
            use_weight_features, use_particle_features, temperature, False, name, weights=weights, rng=rng, seed=seed,
            device=device)
        n = self._np
        self.name = name
        self.n_particles, self.state_dim = n.n_particles, n.state_dim
        self.transition_fn = transition_fn
        self.log_likelihood_fn = log_likelihood_fn
        self.rnn_type, self.rnn_hidden_dim, self.rnn_num_layers = n.rnn_type, n.rnn_hidden_dim, n.rnn_num_layers
        self.use_weight_features, self.use_particle_features = n.use_weight_features, n.use_particle_features
        self.temperature = temperature
        self.use_baseline_resampling = False
        self.seed, self.epoch, self.rng = n.seed, 0, n.rng
        self.device = int(device)
        self._h: Optional[RN._Handle] = None
        self._params: List[torch.nn.Parameter] = [torch.nn.Parameter(torch.from_numpy(a)) for a in n.get_weights()]

    # ------------------------------------------------------------------ the network
    def parameters(self):
        """The network as ``torch.nn.Parameter``s in Keras' ``get_weights()`` order."""
        return list(self._params)

    def to(self, device):
        """Move the parameters' storage to a torch device (``"cuda"``, ``"cuda:0"``, ``"cpu"``) and return
        ``self``.  The ``Parameter`` objects stay, their ``.data`` is replaced: call it before building
        the optimizer, as with ``nn.Module``.  With the parameters, the observations and what the
        callables close over on the HIP device that computes, ``step`` and ``filter`` run on the device
        path.  ``init_particles`` still draws from the NumPy ``rng`` and the statistics of
        ``return_ess`` are host NumPy on detached copies."""
        device = torch.device(device)
        with torch.no_grad():
            for p in self._params:
                p.data = p.data.to(device)
        return self

    def get_weights(self) -> List[np.ndarray]:
        """Copies of the network's arrays in Keras' order."""
        return [_host(p).copy() for p in self._params]

    def set_weights(self, weights) -> None:
        """Replace the values of the parameters (the ``Parameter`` objects stay, so an optimizer keeps
        them); shapes are checked against ``dpf_rnn.weight_shapes``."""
        W = RN._check_weights([_host(a) if isinstance(a, torch.Tensor) else a for a in weights],
                              RN.weight_shapes(*self._np._net()))
        with torch.no_grad():
            for p, a in zip(self._params, W):
                p.copy_(torch.from_numpy(a))

    def _handle(self, B: int) -> RN._Handle:
        want = (self.n_particles, self.state_dim, B, self.rnn_hidden_dim, self.rnn_num_layers, self.rnn_type,
                self.use_weight_features, self.use_particle_features)
        return self._cached(want, lambda: RN._Handle(*want, device=self.device))

    def _rnn_resample(self, particles, log_weights):
        """rnn.py:263-349: ``(new_particles (B, N, d), assignment_probs (B, N, N))``, differentiable."""
        if tuple(particles.shape[1:]) != (self.n_particles, self.state_dim):
            raise ValueError(f"particles must be (B, {self.n_particles}, {self.state_dim}), got {tuple(particles.shape)}")
        # before a handle is made (on the device path the values are checked by rnn_resample, in its one readback)
        if DC.on_device((particles, log_weights, *self._params), self.device):
            _validate_dev(particles, log_weights, self._params, self.rnn_type, self.temperature,
                          self.use_weight_features, self.use_particle_features, False)
        else:
            RN._validate(_host(particles), _host(log_weights), self.temperature)
        return rnn_resample(particles, log_weights, self._params, self.rnn_type, self.temperature,
                            use_weight_features=self.use_weight_features,
                            use_particle_features=self.use_particle_features, device=self.device,
                            check_values=self.check_values, _handle=self._handle(int(particles.shape[0])))

    # ------------------------------------------------------------------ the filter
    def init_particles(self, batch_size, init_mean, init_cov_chol):
        """rnn.py:428-473: (B, N, d) draws ``mean + eps @ L`` with eps from ``self.rng``, differentiable
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

    def step(self, particles, log_weights, observation, params=None, return_ess=False):
        """rnn.py:478-539: propagate and reweight (the user's torch callables), resample (device).
        Returns ``(new_particles, new_log_weights, assignment_matrix)`` and with ``return_ess`` the
        dictionary of ``dpf_rnn``'s ``step``."""
        if params is None:
            params = {}
        particles = _as_f64("particles", particles)
        log_weights = _as_f64("log_weights", log_weights)
        pred = _as_f64("transition_fn's result", self.transition_fn(particles, params))
        log_lik = _as_f64("log_likelihood_fn's result", self.log_likelihood_fn(pred, observation, params))
        log_weights = log_weights + log_lik
        log_weights = log_weights - torch.logsumexp(log_weights, dim=-1, keepdim=True)
        new_particles, assignment = self._rnn_resample(pred, log_weights)
        new_log_weights = torch.full(tuple(log_weights.shape), math.log(1.0 / self.n_particles), dtype=torch.float64,
                                     device=log_weights.device)
        if not return_ess:
            return new_particles, new_log_weights, assignment
        F = RN.DifferentiableParticleFilterRNN
        lw, nlw = _host(log_weights), _host(new_log_weights)
        ess_dict = {
            "ess_before": F.compute_ess(lw),
            "ess_after": F.compute_ess(nlw),
            "entropy_before": F.compute_weight_entropy(lw),
            "entropy_after": F.compute_weight_entropy(nlw),
        }
        return new_particles, new_log_weights, assignment, ess_dict

    def filter(self, observations, init_mean, init_cov_chol, params=None, return_ess=False):
        """rnn.py:543-638: the filter over ``observations`` (B, T, obs_dim); returns particles
        (B, T + 1, N, d), log-weights (B, T + 1, N), the prior draw first, and the assignment matrices
        (B, T, N, N); with ``return_ess`` also the statistics dictionary of ``dpf_rnn``'s ``filter``."""
        if params is None:
            params = {}
        observations = torch.as_tensor(observations, dtype=torch.float64)
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
        particles_seq = torch.stack(particles_list, dim=1)
        logw_seq = torch.stack(logw_list, dim=1)
        assignment_seq = (torch.stack(assignment_matrices, dim=1) if T
                          else torch.zeros((B, 0, N, N), dtype=torch.float64))
        if not return_ess:
            return particles_seq, logw_seq, assignment_seq
        before, after, ent_before, ent_after = (
            np.stack(stats[k], axis=1) if T else np.zeros((B, 0))
            for k in ("ess_before", "ess_after", "entropy_before", "entropy_after"))
        ess_stats = {
            "ess_before_resampling": before,
            "ess_after_resampling": after,
            "entropy_before_resampling": ent_before,
            "entropy_after_resampling": ent_after,
            "mean_ess_before": np.mean(before) if T else np.nan,
            "mean_ess_after": np.mean(after) if T else np.nan,
            "mean_entropy_before": np.mean(ent_before) if T else np.nan,
            "mean_entropy_after": np.mean(ent_after) if T else np.nan,
            "min_ess_before": np.min(before) if T else np.nan,
            "min_ess_after": np.min(after) if T else np.nan,
        }
        return particles_seq, logw_seq, assignment_seq, ess_stats
