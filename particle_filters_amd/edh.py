"""Drop-in ``EDHFlowPF`` backed by the MI355X EDH flow kernels.

Mirrors ``/root/reference/models/EDH_particle_filter.py`` (cited ``edh.py:LINE``):
``rk4_step`` (27-33), ``systematic_resample`` / ``effective_sample_size`` (35-52),
``EDHConfig`` (58-64), ``PFState`` (67-74), ``EKFTracker`` / ``UKFTracker`` with
``get_past_mean`` (77-132), and ``EDHFlowPF`` with the same constructor (138-171),
``init_from_gaussian`` (173-180) and ``step(state, z_k, u_km1=None,
process_noise_sampler=None)`` (182-317).

The exact Daum-Huang flow linearises h once per pseudo-time step at the shared mean
trajectory etabar (edh.py:213-280), so the whole lambda integration of every particle
is one affine map of eta0.  The GPU builds that map per step in one workgroup and
applies it with the weights of edh.py:287-297 in one particle kernel
(``csrc/pf_edh_kernels.h``); resampling and the weighted statistics are the LEDH
engine's (identical code in both reference modules).  The tracker stays on the host,
called exactly as the reference calls it: ``predict()`` before the flow, then
``get_past_mean()`` for etabar, ``update(z)`` after the weights.

What a user of the reference changes is what :mod:`particle_filters_amd.ledh` lists:
device models for ``g`` / ``h``, ``h.jacobian`` for ``jacobian_h``, the Gaussian
density objects, and optionally ``rng_mode="device"``.  There is no CPU fallback.

The sensor-network models (``models.ScaleTransition`` with ``IdentityObservation`` or
``ExpObservation``, d up to 1024, Gaussian or Poisson elementwise likelihood) take the *dense*
path: the flow matrices of edh.py:229-264 are d x d, so the host composes the affine map
``eta_L = M eta_0 + c`` of each step in the reference's NumPy expressions
(:func:`compose_flow_map`) and the device applies it to the particles, evaluates the weights,
resamples and takes the moments on the fp64 matrix cores (``csrc/pf_edh_dense_kernels.h``).
With ``flow_map="device"`` (diagonal flow ``R``) the map itself is composed on the device from the
tracker's ``P`` and past mean (``csrc/pf_edh_flowmap_kernels.h``): a Cholesky factorisation of S, d
triangular solves and the d x d products of the integrator per lambda step, none of them on the host.
Given a ``trackers.DeviceUKFTracker`` as its tracker, ``run`` chains the tracker's predict and update
into the same stream of launches (``pf_edh_dense_flow_run_tracked``), so a step has no host work at all.
Process noise on these routes is the host sampler's, uploaded, or a ``noise.DeviceGaussianNoise`` given in
the sampler's place: Philox normals times chol(Q), drawn by the device ahead of each step
(``csrc/pf_noise_dense_kernels.h``).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from . import _native as N
from . import models as M
from . import ledh_dense as _ledh_dense
from ._dense import DensePlumbing
from .ledh import LEDHFlowPF, LEDHRunResult, PFState, effective_sample_size, systematic_resample
from .noise import DeviceGaussianNoise
from .trackers import DeviceUKFTracker, EKFTracker, UKFTracker

Array = np.ndarray

__all__ = ["EDHConfig", "EDHFlowPF", "PFState", "EKFTracker", "UKFTracker", "DeviceUKFTracker", "rk4_step",
           "systematic_resample", "effective_sample_size", "compose_flow_map", "DeviceGaussianNoise"]


def rk4_step(x: Array, f: Callable[[Array], Array], dt: float) -> Array:
    """edh.py:27-33 (host helper kept for API parity)."""
    k1 = f(x)
    k2 = f(x + 0.5 * dt * k1)
    k3 = f(x + 0.5 * dt * k2)
    k4 = f(x + dt * k3)
    return x + (dt / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)


def compose_flow_map(P: Array, etabar: Array, z_k: Array, h, jacobian_h, R: Array, n_steps: int,
                     integrator: str = "rk4"):
    """The whole lambda integration of edh.py:216-280 as one affine map ``eta_L = M eta_0 + c``.

    Per step, H, e, S, cond(S), A and b are the reference's expressions (edh.py:230-264) at the
    mean trajectory ``etabar``, which is advanced by the reference's own integrator step.  One
    integrator step of the affine field ``A eta + b`` is ``eta -> Phi eta + psi`` with, for
    ``E = eps A``: Euler ``Phi = I + E``, ``psi = eps b``; RK4 ``Phi = I + E + E^2/2 + E^3/6 +
    E^4/24``, ``psi = eps (I + E/2 + E^2/6 + E^3/24) b`` (``csrc/pf_edh_kernels.h``).  Returns
    ``(M, c, condition_numbers, etabar_L)``."""
    nx = etabar.size
    n_steps = max(1, int(n_steps))
    dlam = 1.0 / float(n_steps)
    lam = 0.0
    I = np.eye(nx)
    Mc, cc = np.eye(nx), np.zeros(nx)
    conds = []
    for _ in range(n_steps):
        lam = min(1.0, lam + dlam)
        H = jacobian_h(etabar)
        h_bar = h(etabar)
        e = h_bar - H @ etabar
        S = lam * H @ P @ H.T + R
        try:
            conds.append(float(np.linalg.cond(S)))
        except Exception:
            conds.append(np.nan)
        try:
            S_inv_H = np.linalg.solve(S, H)
        except np.linalg.LinAlgError:
            S = S + 1e-8 * np.eye(S.shape[0])
            S_inv_H = np.linalg.solve(S, H)
        A = -0.5 * P @ H.T @ S_inv_H
        try:
            R_inv_innov = np.linalg.solve(R, (z_k - e))
        except np.linalg.LinAlgError:
            R_inv_innov = np.linalg.inv(R + 1e-8 * np.eye(R.shape[0])) @ (z_k - e)
        PHt_Rinv_innov = P @ H.T @ R_inv_innov
        b = (I + 2.0 * lam * A) @ ((I + lam * A) @ PHt_Rinv_innov + A @ etabar)

        def field(vec):
            return A @ vec + b

        if integrator == "euler":
            Phi = I + dlam * A
            psi = dlam * b
            etabar = etabar + dlam * field(etabar)
        else:
            E = dlam * A
            G = I + (E / 2.0) @ (I + (E / 3.0) @ (I + E / 4.0))  # I + E/2 + E^2/6 + E^3/24
            Phi = I + E @ G
            psi = dlam * (G @ b)
            etabar = rk4_step(etabar, field, dlam)
        Mc = Phi @ Mc
        cc = Phi @ cc + psi
    return Mc, cc, conds, etabar


@dataclass
class EDHConfig:
    """edh.py:58-64 (including the shared default rng of the reference)."""

    n_particles: int = 512
    n_lambda_steps: int = 8
    resample_ess_ratio: float = 0.5
    flow_integrator: str = "rk4"
    rng: np.random.Generator = np.random.default_rng(0)


class EDHFlowPF(LEDHFlowPF, DensePlumbing):
    """EKF/UKF-assisted EDH particle-flow PF on an MI355X (drop-in for edh.py:135-329)."""

    def __init__(self, tracker, g, h, jacobian_h, log_trans_pdf, log_like_pdf, R,
                 config: Optional[EDHConfig] = None, *, rng_mode: str = "host", device: int = 0,
                 flow_map: str = "host") -> None:
        self.tracker = tracker
        self.g = g
        self.h = h
        self.Jh = jacobian_h
        self.log_trans_pdf = log_trans_pdf
        self.log_like_pdf = log_like_pdf
        self.R = np.array(R, dtype=float)
        self.cfg = config or EDHConfig()
        if rng_mode not in ("host", "device"):
            raise ValueError("rng_mode must be 'host' or 'device'")
        self.rng_mode = rng_mode
        if flow_map not in ("host", "device"):
            raise ValueError("flow_map must be 'host' or 'device'")
        self.flow_map = flow_map  # read on the dense path only: the engine's path builds its map on the device
        self.device = int(device)
        integ = str(self.cfg.flow_integrator).lower()
        # edh.py:271: anything but "euler" integrates with RK4
        self.integrator = "euler" if integ == "euler" else "rk4"
        self._dense = isinstance(g, M.ScaleTransition)
        if self._dense:
            self._init_dense()
            if flow_map == "device":
                if np.any(self.R[~np.eye(self.nx, dtype=bool)] != 0.0):
                    raise NotImplementedError("flow_map='device' takes a diagonal flow R")
                self._frd = np.ascontiguousarray(np.diag(self.R), dtype=float)
                if not (np.all(self._frd > 0.0) and np.all(np.isfinite(self._frd))):
                    raise np.linalg.LinAlgError("Matrix is not positive definite (R)")
            return
        self._check_engine_models("EDH")
        self.Q = log_trans_pdf.Q
        self.nx, self.nz = self.Q.shape[0], self.R.shape[0]
        self._desc, self._keep = M.describe(g, h, self.Q, self.R)
        self.n = int(self.cfg.n_particles)
        self.L = max(1, int(self.cfg.n_lambda_steps))  # edh.py:216
        seed = int(self.cfg.rng.integers(0, 2 ** 63 - 1)) if rng_mode == "device" else 0
        opts = N.EdhOpts(self.n, self.L, float(self.cfg.resample_ess_ratio), seed, self.device,
                         N.PF_EDH_EULER if self.integrator == "euler" else N.PF_EDH_RK4)
        self._h = N.C.c_void_p()
        N.check(N.load().pf_edh_create(N.C.byref(self._desc), N.C.byref(opts), N.C.byref(self._h)), "pf_edh_create")
        self._version = 0
        self._state = None
        self.last_ess = float("nan")
        self.last_resampled = False

    # ------------------------------------------------------------------ dense path
    # validation, handle and state transfers: _dense.DensePlumbing (shared with ledh_dense.LEDHFlowPF)
    def close(self):
        if not getattr(self, "_dense", False):
            return super().close()
        self._dense_close()

    # the LEDH engine's members that hand self._h to pf_ledh_* entries do not exist on the dense path
    @property
    def shared_jacobian_path(self) -> bool:
        if not self._dense:
            return LEDHFlowPF.shared_jacobian_path.fget(self)
        return False  # the dense path has no LEDH shared-Jacobian table

    def _device_tracker(self):
        if not self._dense:
            return super()._device_tracker()
        raise NotImplementedError("the device EKF tracker is not available on the dense EDH path")

    def tracker_covariances(self, Z: Array) -> Array:
        if not self._dense:
            return super().tracker_covariances(Z)
        raise NotImplementedError("tracker_covariances runs the device EKF, which is not available on the "
                                  "dense EDH path: run the host tracker (trackers.EKFTracker / UKFTracker)")

    def _download(self, which):
        if not self._dense:
            return super()._download(which)
        return self._dense_download(which)

    def _adopt(self, state) -> None:
        if not self._dense:
            return super()._adopt(state)
        self._dense_adopt(state)

    def init_from_gaussian(self, mean0: Array, cov0: Array, *, draws=None) -> PFState:
        """edh.py:173-180; on the dense path the draw is the host's and is uploaded, or the device's own with
        ``draws=DeviceGaussianNoise`` (Philox init stream at ``draws.epoch``, which is not advanced)."""
        if not self._dense:
            if draws is not None:
                raise NotImplementedError("draws is read on the dense path only: the engine path draws on the "
                                          "device with rng_mode='device'")
            return super().init_from_gaussian(mean0, cov0)
        return self._dense_init_from_gaussian(mean0, cov0, draws)

    def process_noise_draws(self, noise, epoch=None) -> Array:
        if not self._dense:
            raise NotImplementedError("process_noise_draws is of the dense path: the engine path draws inside its "
                                      "kernels with process_noise='device'")
        return DensePlumbing.process_noise_draws(self, noise, epoch)

    def _dense_map(self, P, past_mean, z, u):
        """(M, c, condition numbers) of one step from the tracker's P and past mean (edh.py:197, 213)."""
        P = np.asarray(P, float).reshape(self.nx, self.nx)
        P = 0.5 * (P + P.T)
        etabar = self.g(np.asarray(past_mean, float).reshape(self.nx), u, np.zeros(self.nx))
        Mc, cc, conds, _ = compose_flow_map(P, etabar, z, self.h, self.Jh, self.R, self.L, self.integrator)
        return np.ascontiguousarray(Mc), np.ascontiguousarray(cc), conds

    def _flow_inputs(self, P, past_mean, u):
        """(P symmetrised, etabar_0) of one device-composed step (edh.py:197, 213)."""
        P = np.asarray(P, float).reshape(self.nx, self.nx)
        P = np.ascontiguousarray(0.5 * (P + P.T))
        etabar = self.g(np.asarray(past_mean, float).reshape(self.nx), u, np.zeros(self.nx))
        return P, np.ascontiguousarray(np.asarray(etabar, float).reshape(self.nx))

    def _trace_conds(self, trace, P):
        """cond(S) per lambda step (edh.py:238-243) from etabar before each step: L SVDs on the host."""
        if isinstance(self.h, M.ExpObservation):
            return _ledh_dense.condition_numbers(trace, P, self._frd, self.h.m1, self.h.m2)
        dlam = 1.0 / float(self.L)
        lam, out = 0.0, []
        for _ in range(self.L):
            lam = min(1.0, lam + dlam)
            try:
                out.append(float(np.linalg.cond(lam * P + np.diag(self._frd))))
            except Exception:
                out.append(np.nan)
        return out

    def _step_dense(self, state, z_k, u_km1, process_noise_sampler) -> PFState:
        lib = N.load()
        self._noise_fits(process_noise_sampler, 1)
        self._adopt(state)
        hd = self._dense_handle()
        tracked = self.flow_map == "device" and isinstance(self.tracker, DeviceUKFTracker)
        if not tracked:
            _, P = self.tracker.predict()  # edh.py:195
        noise, v, z, u = self._dense_step_inputs(z_k, u_km1, process_noise_sampler)
        info = N.LedhInfo()
        if tracked:  # predict, the map, the weights and update(z_k) chained on the device
            trace = np.empty((self.L, self.nx))
            P = np.empty((self.nx, self.nx))
            N.check(lib.pf_edh_dense_flow_step_tracked(hd, self.tracker._handle(), N.dptr(self._frd), N.dptr(z),
                                                       N.dptr(u), self.L, self._integ_code(), noise, N.dptr(v),
                                                       N.C.byref(info), N.dptr(trace), N.dptr(P)),
                    "pf_edh_dense_flow_step_tracked")
            self.tracker._t += 1
            conds = self._trace_conds(trace, P)
        elif self.flow_map == "device":
            P, etabar = self._flow_inputs(P, self.tracker.get_past_mean(), u)
            trace = np.empty((self.L, self.nx))
            N.check(lib.pf_edh_dense_flow_step(hd, N.dptr(P), N.dptr(etabar), N.dptr(self._frd), N.dptr(z), N.dptr(u),
                                               self.L, self._integ_code(), noise, N.dptr(v), N.C.byref(info),
                                               N.dptr(trace)), "pf_edh_dense_flow_step")
            conds = self._trace_conds(trace, P)
        else:
            Mc, cc, conds = self._dense_map(P, self.tracker.get_past_mean(), z, u)
            N.check(lib.pf_edh_dense_step(hd, N.dptr(Mc), N.dptr(cc), N.dptr(z), N.dptr(u), noise, N.dptr(v),
                                          N.C.byref(info)), "pf_edh_dense_step")
        if not tracked:
            self.tracker.update(z_k)  # edh.py:301
        mean, cov = self._finish_step(info, self.cfg.rng.random)
        self._noise_used(process_noise_sampler, 1)
        return self._new_state(mean, cov, {"condition_numbers": conds})

    def _integ_code(self) -> int:
        return N.PF_EDH_EULER if self.integrator == "euler" else N.PF_EDH_RK4

    def _run_dense(self, state, Z, U, process_noise, tracker_seq, tracker, replay, want_conds=False) -> LEDHRunResult:
        if tracker == "device":
            raise NotImplementedError("tracker='device' is not available on the dense EDH path")
        Z, T, Uc, V, noise = self._run_inputs(Z, U, process_noise, replay)
        self._adopt(state)
        hd = self._dense_handle()
        lib = N.load()
        dev = self.flow_map == "device"
        tracked = False
        if tracker_seq is None and isinstance(self.tracker, DeviceUKFTracker):
            # the tracker runs on the device: chained into the run (flow_map="device"), or ahead over Z in one
            # call; the condition numbers need the last predicted covariance on the host
            tracked = dev and not want_conds
            if not tracked:
                tracker_seq = self.tracker.sequence(Z)[:2]
        Ms = np.empty((T, self.nx, self.nx))  # the maps, or the tracker's covariances (flow_map="device")
        cs = np.empty((T, self.nx))           # the maps' offsets, or etabar_0
        conds = []
        for t in range(0 if tracked else T):  # the tracker never sees the particles: every map is known up front
            if tracker_seq is None:
                _, P = self.tracker.predict()
                xbar = self.tracker.get_past_mean()
                self.tracker.update(Z[t])
            else:
                P = np.asarray(tracker_seq[0], float).reshape(T, self.nx, self.nx)[t]
                xbar = np.asarray(tracker_seq[1], float).reshape(T, self.nx)[t]
            if dev:
                Ms[t], cs[t] = self._flow_inputs(P, xbar, None if Uc is None else Uc[t])
                continue
            Ms[t], cs[t], cd = self._dense_map(P, xbar, Z[t], None if Uc is None else Uc[t])
            conds.append(cd)
        Ur = self._run_uniforms(T, replay)  # after the tracker's calls, which may draw from the same generator
        N.check(lib.pf_edh_dense_set_run_replay(hd, N.dptr(V), N.dptr(Ur), T), "pf_edh_dense_set_run_replay")
        if noise == N.PF_NOISE_DEVICE:
            self._arm_noise(process_noise)
        means, covs, ess, flags, fl = self._run_outputs(T)
        if tracked:
            N.check(lib.pf_edh_dense_flow_run_tracked(hd, self.tracker._handle(), N.dptr(self._frd), N.dptr(Z),
                                                      N.dptr(Uc), T, self.L, self._integ_code(), noise, N.dptr(means),
                                                      N.dptr(covs), N.dptr(ess), fl, None),
                    "pf_edh_dense_flow_run_tracked")
            self.tracker._t += T
            diag = {}
        elif dev:
            trace = np.empty((self.L, self.nx)) if want_conds else None
            N.check(lib.pf_edh_dense_flow_run(hd, N.dptr(Ms), N.dptr(cs), N.dptr(self._frd), N.dptr(Z), N.dptr(Uc), T,
                                              self.L, self._integ_code(), noise, N.dptr(means), N.dptr(covs),
                                              N.dptr(ess), fl, N.dptr(trace)), "pf_edh_dense_flow_run")
            diag = {"condition_numbers": self._trace_conds(trace, Ms[-1])} if want_conds else {}
        else:
            N.check(lib.pf_edh_dense_run(hd, N.dptr(Ms), N.dptr(cs), N.dptr(Z), N.dptr(Uc), T, noise, N.dptr(means),
                                         N.dptr(covs), N.dptr(ess), fl), "pf_edh_dense_run")
            diag = {"condition_numbers": conds[-1]}
        self._noise_used(process_noise, T)
        return self._run_result(means, covs, ess, flags, diag)

    def step(self, state: PFState, z_k: Array, u_km1: Optional[Array] = None,
             process_noise_sampler: Optional[Callable[[int, int], Array]] = None) -> PFState:
        """One EDH step (edh.py:182-317)."""
        if self._dense:
            return self._step_dense(state, z_k, u_km1, process_noise_sampler)
        lib = N.load()
        self._adopt(state)
        _, P = self.tracker.predict()  # edh.py:195
        P = np.ascontiguousarray(np.asarray(P, float).reshape(self.nx, self.nx))
        noise, v, z, u = self._step_inputs(z_k, u_km1, process_noise_sampler)  # edh.py:200-202
        xbar = np.ascontiguousarray(np.asarray(self.tracker.get_past_mean(), float).reshape(self.nx))  # edh.py:213
        info = N.LedhInfo()
        S = np.empty((self.L, self.nz, self.nz))
        N.check(lib.pf_edh_step(self._h, N.dptr(P), N.dptr(xbar), N.dptr(z), N.dptr(u), noise, N.dptr(v),
                                N.C.byref(info), N.dptr(S)), "pf_edh_step")
        self.tracker.update(z_k)  # edh.py:301
        return self._finish_engine_step(info, S)

    def run(self, state: PFState, Z: Array, U: Optional[Array] = None, *, process_noise: str = "device",
            tracker_seq: Optional[tuple] = None, tracker: str = "host", replay=None,
            condition_numbers: bool = False) -> LEDHRunResult:
        """The driver loop ``for t: state = step(state, Z[t])`` on the device with no host
        synchronisation inside T.  ``tracker="host"``: the tracker object is run ahead over Z
        (predict / get_past_mean / update, the same call sequence as the loop — it never sees
        the particles) unless ``tracker_seq = (Ps [T][nx][nx], Xbars [T][nx])`` is given.
        ``tracker="device"``: an EKFTracker over this filter's models runs on the GPU and
        also yields the past means.  Process noise is Philox times chol(Q) (``"device"``,
        resampling uniforms from Philox), zero (``"none"``) or replayed (``"host"`` with
        ``replay=(V, U)``, the contract of ``LEDHFlowPF.run``: U[t] is read only on steps that
        resample).

        On the dense path (sensor-network models) every step's map (M_t, c_t) is composed up
        front on the host; ``process_noise`` is ``"none"``, ``"host"`` or a ``noise.DeviceGaussianNoise``
        (the device draws step t's noise at ``epoch + t`` ahead of the step, and the object moves on by T
        when the run succeeds; ``replay`` is then ``(None, U)`` or ``None``) and the resampling
        uniforms are ``replay[1]`` (or T draws of ``config.rng``); ``tracker="device"`` and
        ``process_noise="device"`` raise ``NotImplementedError``.  With ``flow_map="device"`` the maps
        are composed inside the run from the tracker's covariances and past means (with a
        ``trackers.DeviceUKFTracker`` as the constructor's tracker its predict and update are chained
        into the same run, so nothing of a step is host work; with ``flow_map="host"`` it is run ahead
        by one ``tracker.sequence(Z)`` call), and
        ``condition_numbers=True`` fills the final state's ``diagnostics["condition_numbers"]`` from
        the last step's etabar trace (L SVDs of d x d on the host); the keyword is read only there.  A
        step whose S is not positive definite raises ``LinAlgError`` and leaves the filter
        uninitialised."""
        if tracker not in ("host", "device"):
            raise ValueError("tracker must be 'host' or 'device'")
        if self._dense:
            return self._run_dense(state, Z, U, process_noise, tracker_seq, tracker, replay, bool(condition_numbers))
        if tracker == "device":
            return super().run(state, Z, U, process_noise=process_noise, tracker="device", replay=replay)
        self._adopt(state)
        Z = np.ascontiguousarray(np.asarray(Z, float).reshape(-1, self.nz))
        T = Z.shape[0]
        noise = self._noise_mode(process_noise, replay, T)
        if tracker_seq is None:
            Ps, Xb = self._tracker_ahead(Z, past_means=True)
        else:
            Ps = np.ascontiguousarray(np.asarray(tracker_seq[0], float).reshape(T, self.nx, self.nx))
            Xb = np.ascontiguousarray(np.asarray(tracker_seq[1], float).reshape(T, self.nx))
        Uc = None if U is None else np.ascontiguousarray(np.asarray(U, float).reshape(T, self.nx))
        means, covs, ess, flags, fl = self._run_outputs(T)
        N.check(N.load().pf_edh_run(self._h, N.dptr(Ps), N.dptr(Xb), N.dptr(Z), N.dptr(Uc), T, noise, N.dptr(means),
                                    N.dptr(covs), N.dptr(ess), fl), "pf_edh_run")
        return self._run_result(means, covs, ess, flags, {}, record_last=False)
