"""PyTorch autograd binding of the Sinkhorn OT resampler, and the ``DPF_OT`` filter whose outputs
can be differentiated.

``sinkhorn_ot_resample`` is ``dpf_ot.sinkhorn_ot_resample`` as a differentiable torch operation
(``SinkhornResample``, a ``torch.autograd.Function``): the forward pass is ``pf_ot_resample`` with
its dual history kept (``OtSaved``), the backward pass ``pf_ot_backward``
(``dpf_ot.sinkhorn_ot_resample_vjp``), the reverse sweep over the iterations with the plan
recomputed, where autodiff of the unrolled loop would keep about 4 K matrices of N x N alive for
every step of a filter.  Gradients flow to the particles and the weights; ``epsilon`` is a plain
float.  Double backward is not implemented and raises.

Tensors must be float64 (another dtype is a ``TypeError``) and may live on any device.  Two paths:

* the device path, when the caller asks for it (``device_path=True`` on ``sinkhorn_ot_resample`` and on
  the filter's constructor) and every tensor of a call is on the HIP device that computes
  (``device``): the device-pointer entries ``pf_ot_resample_dev`` / ``pf_ot_backward_dev`` run on
  torch's current stream on the tensors where they lie.  The forward pass records its own dual history
  straight into tensors that ``ctx`` keeps on the device, with the iteration counts (no replay, and no
  host copy in either direction); results and gradients are tensors on that device, bitwise those of
  the host path on the same values.  With ``check_values=True`` the finiteness checks of the host path
  and the largest iteration count are folded into one small read-back per call, and that count
  bounds the reverse sweep of the backward call, so an early stop does not pay the empty launches;
  with ``check_values=False`` nothing is read back, a call enqueues and returns, and the sweep is
  enqueued for all ``n_iters`` iterations.  Non-contiguous tensors are made contiguous first;
* the host path, the default, and for anything else (CPU tensors, mixed placement, another GPU): a
  tensor is detached, copied to the CPU, handed to the C ABI as a NumPy array, and the result is
  copied back to the tensor's device.

``_dpf_common.PATH_CALLS`` counts the calls per path.

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

from . import _dpf_common as DC
from . import _native as NV
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


_VALUE_ERRORS = ("particles must be finite", "weights must be finite")
SOLVERS = ("launches", "resident")


_side_streams = {}


class _OnStream:
    """``with _OnStream(device) as stream:`` gives the hipStream_t the entries enqueue on, ordered
    behind what torch's current stream holds and in front of what it is given next.  That is the
    current stream itself, unless it is the null stream: a null ``stream`` argument means the handle's
    own stream to the entries, which the null stream does not order, so the work then goes to a side
    stream of this module between two event waits (nothing blocks the host)."""

    def __init__(self, device: int):
        self.cur = torch.cuda.current_stream(device)
        self.side = None
        if self.cur.cuda_stream == 0:
            if device not in _side_streams:
                _side_streams[device] = torch.cuda.Stream(device)
            self.side = _side_streams[device]

    def __enter__(self) -> int:
        if self.side is None:
            return self.cur.cuda_stream
        self.side.wait_stream(self.cur)
        return self.side.cuda_stream

    def __exit__(self, *exc):
        if self.side is not None:  # also what frees the call's temporaries for reuse on the current stream
            self.cur.wait_stream(self.side)
        return False


def _check_solver(solver, device_path=True, on_device=True, N=1) -> None:
    """``solver`` is known, and ``"resident"`` has what it needs: checked on the CPU, before any
    handle exists."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    if solver == "resident":
        if not device_path:
            raise ValueError('solver="resident" needs device_path=True')
        if N > OT.RESIDENT_MAX_N:
            raise ValueError(f'solver="resident" needs N <= {OT.RESIDENT_MAX_N}, got N = {N}')
        if not on_device:
            raise ValueError('solver="resident" needs every tensor on the device that computes')


class SinkhornResample(torch.autograd.Function):
    """``new_particles = SinkhornResample.apply(particles, weights, epsilon, n_iters, min_val, tol,
    device, handle)``: (N, d) with (N,), or (B, N, d) with (B, N), float64.  ``ctx`` keeps the inputs
    and the forward pass's ``OtSaved``; ``backward`` is one ``pf_ot_backward``.

    With ``device_path`` (a class attribute, off in this class) and both tensors on the HIP device
    ``device`` the pass runs on the device path: ``pf_ot_resample_dev`` / ``pf_ot_backward_dev`` on
    torch's current stream, on the tensors where they lie, the dual history recorded by the forward
    pass into device tensors that ``ctx`` keeps.  ``check_values`` (a class attribute;
    ``sinkhorn_ot_resample`` picks the class) says whether a call reads its one small tensor back."""

    device_path = False  # asked for by ``sinkhorn_ot_resample(..., device_path=True)``, which picks the class
    check_values = True

    @staticmethod
    def forward(ctx, particles, weights, epsilon, n_iters, min_val, tol, device, handle, flags=0):
        dev = ctx._forward_cls.device_path and DC.on_device((particles, weights), device)
        DC.count_path(dev)
        ctx.dev = dev
        if dev:  # flags: pf_ot_resample_dev's (``sinkhorn_ot_resample`` sets them from ``solver``)
            return SinkhornResample._forward_dev(ctx, particles, weights, epsilon, n_iters, min_val, tol, device, handle,
                                                 flags)
        out, _, saved = OT.sinkhorn_ot_resample(_host(particles), _host(weights), epsilon, n_iters, min_val, tol,
                                                return_saved=True, device=device, _handle=handle)
        ctx.save_for_backward(particles, weights)
        ctx.ot = (float(epsilon), int(n_iters), float(min_val), float(tol), int(device), handle, saved)
        return torch.from_numpy(out).to(particles.device)

    @staticmethod
    def _forward_dev(ctx, particles, weights, epsilon, n_iters, min_val, tol, device, handle, flags):
        batched = particles.ndim == 3
        X = (particles if batched else particles[None]).detach().contiguous()
        w = (weights if batched else weights[None]).detach().contiguous()
        B, N, d = X.shape
        out = torch.empty_like(X)
        its = torch.empty(B, dtype=torch.int32, device=X.device)
        hist = am = None
        if any(ctx.needs_input_grad[:2]):  # the forward pass records what the backward pass needs
            hist = torch.empty((B, 4, n_iters + 1, N), dtype=torch.float64, device=X.device)
            am = torch.empty((B, n_iters, N), dtype=torch.int32, device=X.device)
        h = handle
        own = h is None or h.h is None or h.key() != (N, d, B)
        if own:
            h = OT._Handle(N, d, B, device)
        try:
            with _OnStream(device) as stream:
                h.resample_dev(stream, X.data_ptr(), w.data_ptr(), epsilon, n_iters, min_val, tol, out.data_ptr(),
                               iterations=its.data_ptr(), hist=0 if hist is None else hist.data_ptr(),
                               hist_argmax=am.data_ptr() if hist is not None and n_iters else 0, flags=flags)
        finally:
            if own:
                h.close()  # waits for the call: the outputs are the caller's, the scratch the handle's
        h.last_iterations = its
        k_sweep = n_iters
        if ctx._forward_cls.check_values:  # the one read-back: the value checks and the largest count
            bad_X, bad_w, kmax = torch.stack([(~torch.isfinite(X).all()).to(torch.int32),
                                              (~torch.isfinite(w).all()).to(torch.int32), its.max()]).tolist()
            DC.raise_first(bad_X | bad_w << 1, _VALUE_ERRORS)
            k_sweep = max(kmax, 1) if n_iters else 0
        ctx.save_for_backward(particles, weights)
        ctx.ot = (float(epsilon), int(n_iters), float(min_val), int(device), handle, (its, hist, am, k_sweep))
        return out if batched else out[0]

    @staticmethod
    def _backward_dev(ctx, grad_new_particles):
        particles, weights = ctx.saved_tensors
        epsilon, n_iters, min_val, device, handle, (its, hist, am, k_sweep) = ctx.ot
        batched = particles.ndim == 3
        X = (particles if batched else particles[None]).detach().contiguous()
        w = (weights if batched else weights[None]).detach().contiguous()
        g = (grad_new_particles if batched else grad_new_particles[None]).contiguous()
        B, N, d = X.shape
        if ctx._forward_cls.check_values and not bool(torch.isfinite(g).all().item()):
            raise ValueError("grad_new_particles must be finite")
        gX, gw = torch.empty_like(X), torch.empty_like(w)
        h = handle
        own = h is None or h.h is None or h.key() != (N, d, B)
        if own:
            h = OT._Handle(N, d, B, device)
        try:
            with _OnStream(device) as stream:
                h.backward_dev(stream, X.data_ptr(), w.data_ptr(), epsilon, min_val, its.data_ptr(), n_iters,
                               k_sweep, hist.data_ptr(), am.data_ptr() if n_iters else 0, g.data_ptr(), gX.data_ptr(),
                               gw.data_ptr())
        finally:
            if own:
                h.close()
        gX = (gX if batched else gX[0]) if ctx.needs_input_grad[0] else None
        gw = (gw if batched else gw[0]) if ctx.needs_input_grad[1] else None
        return gX, gw, None, None, None, None, None, None, None

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_new_particles):
        if ctx.dev:
            return SinkhornResample._backward_dev(ctx, grad_new_particles)
        particles, weights = ctx.saved_tensors
        epsilon, n_iters, min_val, tol, device, handle, saved = ctx.ot
        gX, gw = OT.sinkhorn_ot_resample_vjp(_host(particles), _host(weights), _host(grad_new_particles), epsilon,
                                             n_iters, min_val, tol, saved=saved, device=device, _handle=handle)
        gX = torch.from_numpy(gX).to(particles.device) if ctx.needs_input_grad[0] else None
        gw = torch.from_numpy(gw).to(weights.device) if ctx.needs_input_grad[1] else None
        return gX, gw, None, None, None, None, None, None, None


class _SinkhornResampleDevice(SinkhornResample):
    device_path = True


class _SinkhornResampleDeviceUnchecked(_SinkhornResampleDevice):
    check_values = False


def _validate_dev(particles, weights, epsilon, n_iters) -> None:
    """``dpf_ot._validate`` for tensors on the device: the shapes and the scalars from metadata, with
    its messages; the values are checked by the forward pass, in its one read-back."""
    DC.check_batched_shapes(particles.shape, weights.shape, "weights")
    DC.check_positive("epsilon", epsilon)
    if int(n_iters) != n_iters or int(n_iters) < 0:
        raise ValueError(f"n_iters must be a non-negative integer, got {n_iters}")


def sinkhorn_ot_resample(particles, weights, epsilon=0.1, n_iters=50, min_val=1e-12, tol=1e-6, *, device=0,
                         device_path=False, check_values=True, solver="launches",
                         _handle: Optional[OT._Handle] = None):
    """``dpf_ot.sinkhorn_ot_resample`` on float64 tensors, differentiable with respect to
    ``particles`` and ``weights``: returns ``(new_particles, new_weights)``, the new weights being
    the constant 1 / N.  ``device`` is the HIP device that computes.  With ``device_path=True``,
    tensors that are both on that device take the device path (see the module's docstring): the
    results are tensors there, bitwise those of the host path, and with ``check_values=False`` the
    call enqueues and returns without reading anything back (the values are then the caller's
    responsibility: a NaN goes through the kernels as a NaN).  Without it, and for any other
    placement, the data goes through host memory, whichever device the tensors are on;
    ``check_values`` has no effect there.  ``solver`` names how the forward pass runs: ``"launches"``,
    the stream-ordered launch sequence, or ``"resident"``, the whole resampling in one launch with the
    cost matrix in LDS (``PF_OT_RESIDENT``), which needs ``device_path=True``, tensors on the device and
    N <= 128 (a ``ValueError`` otherwise: nothing falls back) and agrees with the launch sequence to
    rounding, not bitwise.  The backward pass is the reverse sweep for both."""
    particles = _as_f64("particles", particles)
    weights = _as_f64("weights", weights)
    if isinstance(epsilon, torch.Tensor):
        raise TypeError("epsilon is a plain float: there is no gradient with respect to it")
    on_dev = DC.on_device((particles, weights), device)
    _check_solver(solver, device_path, on_dev, particles.shape[-2] if particles.ndim >= 2 else 1)
    if device_path and on_dev:
        _validate_dev(particles, weights, epsilon, n_iters)
    else:
        OT._validate(_host(particles), _host(weights), epsilon, n_iters)
    fn = (SinkhornResample if not device_path else
          _SinkhornResampleDevice if check_values else _SinkhornResampleDeviceUnchecked)
    new = fn.apply(particles, weights, float(epsilon), int(n_iters), float(min_val), float(tol), int(device), _handle,
                   NV.PF_OT_RESIDENT if solver == "resident" else 0)
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
                 sinkhorn_iters=50, name=None, *, rng: Optional[np.random.Generator] = None, device=0,
                 device_path=False, check_values=True, solver="launches"):
        _check_solver(solver, device_path, True, int(N_particles))
        self.device_path = bool(device_path)    # sinkhorn_ot_resample's: the device path for tensors on the device
        self.check_values = bool(check_values)  # of the device path
        self.solver = solver
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

    @property
    def last_iterations(self):
        """The Sinkhorn iterations of the latest step on the device path: an int32 tensor (1,) on the
        device, or None when no step has taken that path."""
        return None if self._h is None else self._h.last_iterations

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
        if self.device_path and DC.on_device((pred, new_weights), self.device):
            _validate_dev(pred, new_weights, self.epsilon, self.sinkhorn_iters)  # the values: by the forward pass
        else:
            OT._validate(_host(pred), _host(new_weights), self.epsilon, self.sinkhorn_iters)
        res_particles, res_weights = sinkhorn_ot_resample(pred, new_weights, self.epsilon, self.sinkhorn_iters,
                                                          device=self.device, device_path=self.device_path,
                                                          check_values=self.check_values, solver=self.solver,
                                                          _handle=self._handle())
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
