"""Drop-in ``LEDHFlowPF`` for the sensor-network models (d up to 1024) on an MI355X.

Mirrors ``/root/reference/models/LEDH_particle_filter.py`` (cited ``ledh.py:LINE``) for the wiring
of ``PF_PF_results_reproduction_sn_skew.ipynb`` / ``_snlg.ipynb``: ``models.ScaleTransition``,
``models.ExpObservation`` with ``PoissonLikelihood`` (or ``GaussianLikelihood`` with diagonal R),
``GaussianTransitionDensity(g, Q)``, ``jacobian_h`` ``None`` or ``h.jacobian``, and a diagonal,
positive flow ``R``.  Same constructor, ``init_from_gaussian`` and ``step(state, z_k, u_km1,
process_noise_sampler)`` as the reference; ``run`` adds the device loop.

LEDH linearises h at every particle (ledh.py:140-171), so each particle has its own flow matrices.
With ``h(x) = m1 exp(m2 x)`` the Jacobian is diagonal and ``S_i`` is an elementwise scaling of the
tracker's P: the device factors ``S_i`` and ``S'_i`` (whose determinants give ``det(I + dlam A_i)``)
per particle and lambda step and applies ``A_i`` through triangular solves and products with P
(``csrc/pf_ledh_dense_kernels.h``).  The weights, the resampling and the moments are the dense EDH
path's kernels.  The tracker stays on the host, called as the reference calls it, unless it is a
``trackers.DeviceUKFTracker``, which ``run`` runs ahead on the device in one call.

With ``models.IdentityObservation`` (the SNLG notebook) the Jacobian does not depend on the
particle: the whole step is one affine map of eta_0, composed here in NumPy
(:func:`compose_identity_map`) and applied by ``pf_edh_dense_step``; theta is the same for every
particle and cancels in the normalisation.

``ledh.LEDHFlowPF`` keeps refusing this wiring; this class is the one to use.  There is no CPU
fallback, no ``rng_mode="device"`` and no device EKF tracker (``tracker="device"``) on this path; process
noise is drawn on the device when a ``noise.DeviceGaussianNoise`` stands in the sampler's place.
"""

from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from . import _native as N
from . import ledh as _ledh
from . import models as M
from ._dense import DensePlumbing
from .ledh import LEDHConfig, LEDHRunResult, PFState
from .trackers import DeviceUKFTracker

Array = np.ndarray

__all__ = ["LEDHConfig", "LEDHFlowPF", "LEDHRunResult", "PFState", "compose_identity_map", "condition_numbers"]


def compose_identity_map(P: Array, z: Array, R: Array, n_steps: int):
    """The lambda loop of ledh.py:136-171 for ``h(x) = x`` as one map ``eta_L = M eta_0 + c``.

    With H = I and e = 0: ``S = lam P + R``, ``A = -1/2 P S^-1`` and ``b = (I + 2 lam A)((I + lam A)
    P R^-1 z + A eta_0)``, so one Euler step is ``eta -> (I + dlam A) eta + dlam (I + 2 lam A) A
    eta_0 + dlam (I + 2 lam A)(I + lam A) P R^-1 z``.  Returns ``(M, c, condition_numbers)``."""
    d = P.shape[0]
    I = np.eye(d)
    n_steps = max(1, int(n_steps))
    dlam = 1.0 / float(n_steps)
    lam = 0.0
    Mc, cc, conds = np.eye(d), np.zeros(d), []
    PRz = P @ np.linalg.solve(R, z)
    for _ in range(n_steps):
        lam = min(1.0, lam + dlam)
        S = lam * P + R
        try:
            conds.append(float(np.linalg.cond(S)))
        except Exception:
            conds.append(np.nan)
        A = -0.5 * P @ np.linalg.solve(S, I)
        B = I + 2.0 * lam * A
        Mc = (I + dlam * A) @ Mc + dlam * (B @ A)
        cc = (I + dlam * A) @ cc + dlam * (B @ ((I + lam * A) @ PRz))
    return np.ascontiguousarray(Mc), np.ascontiguousarray(cc), conds


def condition_numbers(trace: Array, P: Array, rdiag: Array, m1: float, m2: float) -> list:
    """``cond(S)`` of particle 0 per lambda step (ledh.py:152-157) from its positions before each step."""
    L = trace.shape[0]
    dlam = 1.0 / float(L)
    lam, out = 0.0, []
    for j in range(L):
        lam = min(1.0, lam + dlam)
        D = m1 * m2 * np.exp(m2 * trace[j])
        S = lam * (D[:, None] * P * D[None, :]) + np.diag(rdiag)
        try:
            out.append(float(np.linalg.cond(S)))
        except Exception:
            out.append(np.nan)
    return out


class LEDHFlowPF(_ledh.LEDHFlowPF, DensePlumbing):
    """EKF/UKF-assisted LEDH particle-flow PF for the sensor-network models (ledh.py:60-224)."""

    _path = "dense LEDH path"

    def __init__(self, tracker, g, h, jacobian_h, log_trans_pdf, log_like_pdf, R,
                 config: Optional[LEDHConfig] = None, *, rng_mode: str = "host", device: int = 0) -> None:
        self.tracker = tracker
        self.g = g
        self.h = h
        self.Jh = jacobian_h
        self.log_trans_pdf = log_trans_pdf
        self.log_like_pdf = log_like_pdf
        self.R = np.array(R, dtype=float)
        self.cfg = config or LEDHConfig()
        if rng_mode not in ("host", "device"):
            raise ValueError("rng_mode must be 'host' or 'device'")
        self.rng_mode = rng_mode
        self.device = int(device)
        self._dh = None
        if not isinstance(g, M.ScaleTransition):
            raise NotImplementedError("ledh_dense.LEDHFlowPF runs the sensor-network wiring (models.ScaleTransition); "
                                      "use particle_filters_amd.ledh.LEDHFlowPF for the engine's models")
        self._init_dense()
        if self.R.ndim != 2 or np.any(self.R != np.diag(np.diag(self.R))):
            raise NotImplementedError("the dense LEDH path takes a diagonal flow R")
        self._frd = np.ascontiguousarray(np.diag(self.R), dtype=float)
        if not (np.all(self._frd > 0.0) and np.all(np.isfinite(self._frd))):
            raise np.linalg.LinAlgError("Matrix is not positive definite (R)")
        self._exp = isinstance(h, M.ExpObservation)

    # ------------------------------------------------------------------ plumbing
    def close(self):
        self._dense_close()

    @property
    def shared_jacobian_path(self) -> bool:
        return not self._exp  # the identity observation: one map for all particles

    def _device_tracker(self):
        raise NotImplementedError("the device EKF tracker is not available on the dense LEDH path")

    def tracker_covariances(self, Z: Array) -> Array:
        raise NotImplementedError("tracker_covariances runs the device EKF, which is not available on the "
                                  "dense LEDH path: run the host tracker (trackers.EKFTracker / UKFTracker)")

    def _download(self, which):
        return self._dense_download(which)

    def _adopt(self, state) -> None:
        self._dense_adopt(state)

    def init_from_gaussian(self, mean0: Array, cov0: Array, *, draws=None) -> PFState:
        """ledh.py:84-91; the draw is the host's and is uploaded, or the device's own with
        ``draws=DeviceGaussianNoise`` (Philox init stream at ``draws.epoch``, which is not advanced)."""
        return self._dense_init_from_gaussian(mean0, cov0, draws)

    def process_noise_draws(self, noise, epoch=None) -> Array:
        return DensePlumbing.process_noise_draws(self, noise, epoch)

    @staticmethod
    def _sym(P, d):
        P = np.asarray(P, float).reshape(d, d)
        return np.ascontiguousarray(0.5 * (P + P.T))  # ledh.py:106

    # ------------------------------------------------------------------ one step
    def _flow_step(self, hd, P, z, u, noise, v, info):
        """The flow and the weights of one step on the device; returns the condition numbers."""
        lib = N.load()
        if not self._exp:
            Mc, cc, conds = compose_identity_map(P, z, self.R, self.L)
            N.check(lib.pf_edh_dense_step(hd, N.dptr(Mc), N.dptr(cc), N.dptr(z), N.dptr(u), noise, N.dptr(v),
                                          N.C.byref(info)), "pf_edh_dense_step")
            return conds
        trace = np.empty((self.L, self.nx))
        N.check(lib.pf_ledh_dense_step(hd, N.dptr(P), N.dptr(self._frd), N.dptr(z), N.dptr(u), self.L, noise, N.dptr(v),
                                       N.C.byref(info), N.dptr(trace)), "pf_ledh_dense_step")
        return condition_numbers(trace, P, self._frd, self.h.m1, self.h.m2)

    def _one_step(self, P, z, u, noise, v, draw_U, after_weights=None):
        """The flow, the weights (``after_weights()``: the tracker update of ledh.py:198) and the finish of
        one step on the handle's current state; ``draw_U()`` yields the resampling uniform when asked."""
        info = N.LedhInfo()
        conds = self._flow_step(self._dense_handle(), P, z, u, noise, v, info)
        if after_weights is not None:
            after_weights()
        mean, cov = self._finish_step(info, draw_U)
        return mean, cov, conds

    def step(self, state: PFState, z_k: Array, u_km1: Optional[Array] = None,
             process_noise_sampler: Optional[Callable[[int, int], Array]] = None) -> PFState:
        """One LEDH step (ledh.py:93-214).  ``LinAlgError`` when some particle's S is not positive
        definite to working precision (for instance ``exp(m2 eta)`` overflows); the state is kept."""
        self._noise_fits(process_noise_sampler, 1)
        self._adopt(state)
        _, P = self.tracker.predict()  # ledh.py:105
        P = self._sym(P, self.nx)
        noise, v, z, u = self._dense_step_inputs(z_k, u_km1, process_noise_sampler)
        mean, cov, conds = self._one_step(P, z, u, noise, v, self.cfg.rng.random,
                                          after_weights=lambda: self.tracker.update(z_k))
        self._noise_used(process_noise_sampler, 1)
        return self._new_state(mean, cov, {"condition_numbers": conds})

    # ------------------------------------------------------------------ the device loop
    def run(self, state: PFState, Z: Array, U: Optional[Array] = None, *, process_noise: str = "none",
            replay=None, tracker_seq: Optional[tuple] = None, tracker: str = "host",
            condition_numbers: bool = False) -> LEDHRunResult:
        """The driver loop ``for t: state = step(state, Z[t])`` with no host synchronisation inside T.
        The tracker object is run ahead over Z (predict / update: it never sees the particles) unless
        ``tracker_seq = (Ps [T][nx][nx],)`` gives its predicted covariances; a
        ``trackers.DeviceUKFTracker`` is run ahead on the device by one ``tracker.sequence(Z)`` call.
        Process noise is zero
        (``"none"``), replayed (``"host"`` with ``replay=(V [T][N][nx], U [T])``) or a
        ``noise.DeviceGaussianNoise`` (drawn on the device at ``epoch + t`` ahead of step t; the object moves
        on by T when the run succeeds, and ``replay`` is ``(None, U)`` or ``None``); the resampling
        uniforms are ``replay[1]`` or T draws of ``config.rng``, and U[t] is read only on steps that
        resample.  ``condition_numbers=True`` also fills ``diagnostics["condition_numbers"]`` of the
        final state (L SVDs of d x d per step on the host; the steps are then enqueued one by one).
        A step whose S is not positive definite raises ``LinAlgError`` and leaves the filter
        uninitialised, as a step without a live weight does (``FloatingPointError``)."""
        if tracker == "device":
            raise NotImplementedError("tracker='device' is not available on the dense LEDH path")
        if tracker != "host":
            raise ValueError("tracker must be 'host' or 'device'")
        Z, T, Uc, V, noise = self._run_inputs(Z, U, process_noise, replay)
        Ur = self._run_uniforms(T, replay)
        self._adopt(state)
        hd = self._dense_handle()
        lib = N.load()
        if tracker_seq is None and isinstance(self.tracker, DeviceUKFTracker):
            tracker_seq = self.tracker.sequence(Z)[:2]  # the device tracker, run ahead over Z in one call
        Ps = np.empty((T, self.nx, self.nx))
        for t in range(T):
            if tracker_seq is None:
                _, P = self.tracker.predict()
                self.tracker.update(Z[t])
            else:
                P = np.asarray(tracker_seq[0], float).reshape(T, self.nx, self.nx)[t]
            Ps[t] = self._sym(P, self.nx)
        means, covs, ess, flags, fl = self._run_outputs(T)
        conds = None
        if condition_numbers:
            for t in range(T):
                if noise == N.PF_NOISE_DEVICE:
                    self._arm_noise(process_noise, t)
                means[t], covs[t], conds = self._one_step(
                    Ps[t], Z[t], None if Uc is None else Uc[t], noise, None if V is None else V[t],
                    lambda t=t: Ur[t])
                ess[t], flags[t] = self.last_ess, self.last_resampled
        elif not self._exp:  # the identity observation: every step's map is known up front
            Ms = np.empty((T, self.nx, self.nx))
            cs = np.empty((T, self.nx))
            for t in range(T):
                Ms[t], cs[t], _ = compose_identity_map(Ps[t], Z[t], self.R, self.L)
            N.check(lib.pf_edh_dense_set_run_replay(hd, N.dptr(V), N.dptr(Ur), T), "pf_edh_dense_set_run_replay")
            if noise == N.PF_NOISE_DEVICE:
                self._arm_noise(process_noise)
            N.check(lib.pf_edh_dense_run(hd, N.dptr(Ms), N.dptr(cs), N.dptr(Z), N.dptr(Uc), T, noise, N.dptr(means),
                                         N.dptr(covs), N.dptr(ess), fl), "pf_edh_dense_run")
        else:
            N.check(lib.pf_edh_dense_set_run_replay(hd, N.dptr(V), N.dptr(Ur), T), "pf_edh_dense_set_run_replay")
            if noise == N.PF_NOISE_DEVICE:
                self._arm_noise(process_noise)
            N.check(lib.pf_ledh_dense_run(hd, N.dptr(Ps), N.dptr(self._frd), N.dptr(Z), N.dptr(Uc), T, self.L, noise,
                                          N.dptr(means), N.dptr(covs), N.dptr(ess), fl), "pf_ledh_dense_run")
        self._noise_used(process_noise, T)
        return self._run_result(means, covs, ess, flags, {"condition_numbers": conds} if condition_numbers else {})
