"""Plumbing shared by the two filters of the sensor-network models, ``edh.EDHFlowPF`` (dense path) and
``ledh_dense.LEDHFlowPF``: the validation of the wiring, the ``pf_edh_dense_handle``, the state
transfers, the finish of a step and the validated inputs of a run.  Both classes run on the same
handle type (``include/pf_edh.h``); only the flow differs.
"""

from __future__ import annotations

import numpy as np

from . import _native as N
from . import models as M
from .noise import DeviceGaussianNoise


class DensePlumbing:
    """Mixin over ``ledh.LEDHFlowPF``, which provides what does not depend on the path: ``_new_state``,
    ``_weighted_stats``, ``_step_inputs``, ``_run_outputs`` and ``_run_result``.  ``_path`` names the
    path in the messages."""

    _path = "dense EDH path"

    def _init_dense(self) -> None:
        """Validation of the sensor-network wiring; touches no device (the handle is made at the
        first upload)."""
        g, h = self.g, self.h
        if not isinstance(h, (M.IdentityObservation, M.ExpObservation)):
            raise NotImplementedError(f"ScaleTransition runs on the {self._path}: h must be "
                                      "models.IdentityObservation or models.ExpObservation")
        if self.Jh is not None and getattr(self.Jh, "__self__", None) is not h:
            raise NotImplementedError("jacobian_h must be None or h.jacobian (the model's analytic Jacobian)")
        if self.Jh is None:
            self.Jh = h.jacobian
        lt, ll = self.log_trans_pdf, self.log_like_pdf
        if not isinstance(lt, M.GaussianTransitionDensity) or lt.g is not g:
            raise NotImplementedError("log_trans_pdf must be models.GaussianTransitionDensity(g, Q)")
        if isinstance(ll, M.PoissonLikelihood) and ll.h is h:
            self._like, self._rdiag = N.PF_EDH_LIKE_POISSON, None
        elif isinstance(ll, M.GaussianLikelihood) and ll.h is h:
            if np.any(ll.R != np.diag(np.diag(ll.R))):
                raise NotImplementedError(f"the {self._path} takes GaussianLikelihood(h, R) with diagonal R")
            self._like, self._rdiag = N.PF_EDH_LIKE_GAUSSIAN, np.ascontiguousarray(np.diag(ll.R), dtype=float)
        else:
            raise NotImplementedError("log_like_pdf must be models.PoissonLikelihood(h) or "
                                      "models.GaussianLikelihood(h, R)")
        if self.rng_mode == "device":
            raise NotImplementedError(f"rng_mode='device' is not available on the {self._path} "
                                      "(process noise and initial draws come from the host)")
        self.Q = np.ascontiguousarray(lt.Q, dtype=float)
        self.nx = self.nz = int(g.nx)
        if h.nx != self.nx or self.Q.shape != (self.nx, self.nx) or self.R.shape != (self.nx, self.nx):
            raise ValueError(f"g, h, Q and R must share the state dimension {self.nx}")
        if not 1 <= self.nx <= 1024:
            raise ValueError(f"the {self._path} takes 1 <= d <= 1024")
        self.n = int(self.cfg.n_particles)
        if self.n < 1:
            raise ValueError("n_particles must be positive")
        self.L = max(1, int(self.cfg.n_lambda_steps))  # edh.py:216, ledh.py:132
        np.linalg.cholesky(self.Q)  # LinAlgError for a Q that is not positive definite
        if self._rdiag is not None and not np.all(self._rdiag > 0.0):
            raise np.linalg.LinAlgError("Matrix is not positive definite (R)")
        self._h = None   # no pf_ledh_handle exists on this path: no pf_ledh_* / pf_edh_* entry is ever called
        self._dh = None  # the pf_edh_dense_handle, made at the first upload
        self._version = 0
        self._state = None
        self.last_ess = float("nan")
        self.last_resampled = False

    def _dense_handle(self):
        if self._dh is None:
            h = self.h
            exp = isinstance(h, M.ExpObservation)
            model = N.EdhDenseModel(self.nx, N.PF_EDH_OBS_EXP if exp else N.PF_EDH_OBS_IDENTITY, self._like, 0,
                                    self.g.alpha, h.m1 if exp else 1.0, h.m2 if exp else 0.0, N.dptr(self._rdiag),
                                    N.dptr(self.Q))
            opts = N.EdhDenseOpts(self.n, float(self.cfg.resample_ess_ratio), self.device, 0)
            hd = N.C.c_void_p()
            N.check(N.load().pf_edh_dense_create(N.C.byref(model), N.C.byref(opts), N.C.byref(hd)),
                    "pf_edh_dense_create")
            self._dh = hd
        return self._dh

    def _dense_close(self):
        if N._lib is not None and getattr(self, "_dh", None) is not None and self._dh.value:
            N._lib.pf_edh_dense_destroy(self._dh)
        self._dh = None

    def _dense_download(self, which):
        lib = N.load()
        if which == "particles":
            out = np.empty((self.n, self.nx))
            N.check(lib.pf_edh_dense_get_particles(self._dense_handle(), N.dptr(out)), "pf_edh_dense_get_particles")
        else:
            out = np.empty(self.n)
            N.check(lib.pf_edh_dense_get_weights(self._dense_handle(), N.dptr(out)), "pf_edh_dense_get_weights")
        return out

    def _dense_adopt(self, state) -> None:
        if state is self._state and self._state is not None:
            return
        p = np.ascontiguousarray(np.asarray(state.particles, float).reshape(self.n, self.nx))
        w = np.ascontiguousarray(np.asarray(state.weights, float).reshape(self.n))
        N.check(N.load().pf_edh_dense_set_state(self._dense_handle(), N.dptr(p), N.dptr(w)), "pf_edh_dense_set_state")

    def _dense_init_from_gaussian(self, mean0, cov0, draws=None):
        """edh.py:173-180 / ledh.py:84-91; the draw is the host's and is uploaded, or with
        ``draws=DeviceGaussianNoise`` the device's own on the Philox init stream (the state is then lazy, as
        after a step, and ``draws.epoch`` is not advanced)."""
        mean0 = np.asarray(mean0, float).reshape(self.nx)
        if draws is not None:
            if not isinstance(draws, DeviceGaussianNoise):
                raise TypeError("draws must be None or a noise.DeviceGaussianNoise")
            mean0 = np.ascontiguousarray(mean0)
            cov0 = np.ascontiguousarray(np.asarray(cov0, float).reshape(self.nx, self.nx))
            mean, cov = np.empty(self.nx), np.empty((self.nx, self.nx))
            N.check(N.load().pf_edh_dense_init_gaussian(self._dense_handle(), N.dptr(mean0), N.dptr(cov0), draws.seed,
                                                        draws.epoch, N.dptr(mean), N.dptr(cov)),
                    "pf_edh_dense_init_gaussian")
            return self._new_state(mean, cov, {})
        eps = self.cfg.rng.multivariate_normal(np.zeros(self.nx), cov0, size=self.n)
        particles = np.ascontiguousarray(mean0[None, :] + eps)
        weights = np.full(self.n, 1.0 / self.n)
        N.check(N.load().pf_edh_dense_set_state(self._dense_handle(), N.dptr(particles), N.dptr(weights)),
                "pf_edh_dense_set_state")
        mean, cov = self._weighted_stats(particles, weights)
        st = self._new_state(mean, cov, {})
        st.particles, st.weights = particles, weights
        return st

    # ------------------------------------------------------------------ device process noise
    def process_noise_draws(self, noise, epoch=None):
        """The process noise [N][d] a step given ``noise`` (a ``DeviceGaussianNoise``) uses at ``epoch``
        (default: its next one).  Neither the filter nor ``noise`` changes."""
        if not isinstance(noise, DeviceGaussianNoise):
            raise TypeError("process_noise_draws takes a noise.DeviceGaussianNoise")
        e = DeviceGaussianNoise(noise.seed, noise.epoch if epoch is None else epoch).epoch
        out = np.empty((self.n, self.nx))
        N.check(N.load().pf_edh_dense_noise_draws(self._dense_handle(), noise.seed, e, N.dptr(out)),
                "pf_edh_dense_noise_draws")
        return out

    def _arm_noise(self, noise, offset=0):
        """PF_NOISE_DEVICE for the handle's next step or run, from ``noise.epoch + offset``."""
        N.check(N.load().pf_edh_dense_set_noise(self._dense_handle(), noise.seed, noise.epoch + offset),
                "pf_edh_dense_set_noise")

    def _dense_step_inputs(self, z_k, u_km1, process_noise_sampler):
        """``_step_inputs`` where the sampler may be a ``DeviceGaussianNoise``: the draw is armed, not made."""
        if not isinstance(process_noise_sampler, DeviceGaussianNoise):
            return self._step_inputs(z_k, u_km1, process_noise_sampler)
        _, _, z, u = self._step_inputs(z_k, u_km1, None)
        self._arm_noise(process_noise_sampler)
        return N.PF_NOISE_DEVICE, None, z, u

    @staticmethod
    def _noise_fits(noise, T) -> None:
        """Before anything is touched: the T epochs of a ``DeviceGaussianNoise`` and the one after them exist."""
        if isinstance(noise, DeviceGaussianNoise) and noise.epoch + T > 0xFFFFFFFF:
            raise ValueError(f"the noise epoch overflows 32 bits within {T} step(s) from {noise.epoch}")

    @staticmethod
    def _noise_used(noise, T) -> None:
        """After a call that succeeded: a ``DeviceGaussianNoise`` moves on by the T epochs drawn."""
        if isinstance(noise, DeviceGaussianNoise):
            noise.epoch += T

    # ------------------------------------------------------------------ one step
    def _finish_step(self, info, draw_U):
        """The resample and the moments of the pending step; ``draw_U()`` yields the resampling uniform
        and is called only when the step resamples (edh.py:41, ledh.py:28).  Returns (mean, cov)."""
        self.last_ess = float(info.ess)
        self.last_resampled = bool(info.resample)
        U = np.array([float(draw_U())]) if info.resample else None
        mean = np.empty(self.nx)
        cov = np.empty((self.nx, self.nx))
        N.check(N.load().pf_edh_dense_finish(self._dense_handle(), N.dptr(U), N.dptr(mean), N.dptr(cov)),
                "pf_edh_dense_finish")
        return mean, cov

    # ------------------------------------------------------------------ a run
    def _run_inputs(self, Z, U, process_noise, replay):
        """(Z, T, Uc, V, noise): validated arrays and the replayed noise.  Draws nothing."""
        if process_noise == "device":
            raise NotImplementedError(f"process_noise='device' is not available on the {self._path}: "
                                      "use 'none' or 'host' with replay=(V, U)")
        device = isinstance(process_noise, DeviceGaussianNoise)
        if not device and process_noise not in ("none", "host"):
            raise ValueError("process_noise must be 'none', 'host' or a noise.DeviceGaussianNoise")
        Z = np.ascontiguousarray(np.asarray(Z, float).reshape(-1, self.nz))
        T = Z.shape[0]
        Uc = None if U is None else np.ascontiguousarray(np.asarray(U, float).reshape(T, self.nx))
        if device:  # the caller arms it (_arm_noise) once the handle holds the state
            if replay is not None and replay[0] is not None:
                raise ValueError("a DeviceGaussianNoise draws the process noise itself: replay must be (None, U) or None")
            self._noise_fits(process_noise, T)
            V, noise = None, N.PF_NOISE_DEVICE
        elif process_noise == "host":
            if replay is None or replay[0] is None:
                raise ValueError("process_noise='host' needs replay=(V [T][N][nx], U [T])")
            V = np.ascontiguousarray(np.asarray(replay[0], float).reshape(T, self.n, self.nx))
            noise = N.PF_NOISE_HOST
        else:
            V, noise = None, N.PF_NOISE_NONE
        return Z, T, Uc, V, noise

    def _run_uniforms(self, T, replay):
        """The resampling uniforms of a run: replayed, or T draws of the configured generator.  Apart from
        ``_run_inputs`` because a user's tracker may share the generator: each class draws where it always did
        relative to its tracker calls."""
        Ur = self.cfg.rng.random(T) if replay is None or replay[1] is None else replay[1]
        return np.ascontiguousarray(np.asarray(Ur, float).reshape(T))
