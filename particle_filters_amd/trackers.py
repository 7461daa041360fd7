"""Gaussian trackers that feed the LEDH flow its prior covariance P_k.

The reference's LEDHFlowPF takes any object with ``predict() -> (m, P)``,
``update(z)`` and ``get_past_mean()`` (``models/LEDH_particle_filter.py:13-16``,
the ``GaussianTracker`` protocol); its tests wrap the EKF
(``models/extended_kalman_filter.py``) in a small adaptor
(``tests/unit_tests/models/test_ledh_flow_pf.py:12-33``).  This module provides the
same pieces for this package:

* :class:`ExtendedKalmanFilter` / :class:`EKFState` — the additive-noise EKF of
  ``extended_kalman_filter.py:110-256`` (analytic or finite-difference Jacobians,
  Joseph form, innovation jitter), host NumPy: nx x nx algebra per step, no particles.
* :class:`EKFTracker` — the GaussianTracker adaptor.
* :class:`UnscentedKalmanFilter` / :class:`UKFState` / :class:`UKFTracker` — the additive-noise UKF
  of ``unscented_kalman_filter.py:68-196`` and its adaptor (``EDH_particle_filter.py:106-132``), in
  the reference's operation order (sigma-point loop, outer-product accumulation loops), so the
  covariances it hands the flow are the reference's.
* :class:`DeviceUKFTracker` — the same adaptor with its state on the GPU for the sensor-network models
  (``csrc/pf_ukf_dense_kernels.h``): the filters' ``run`` drives it without host work.

The tracker never sees the particles, so :meth:`particle_filters_amd.ledh.LEDHFlowPF.run`
can run it ahead over the whole observation sequence and hand the device the
stack of covariances in one upload.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np

Array = np.ndarray


def numerical_jacobian_g(g: Callable, x: Array, u: Optional[Array], eps: float = 1e-6) -> Array:
    """Forward-difference Jacobian of g(x, u) (extended_kalman_filter.py:43-75)."""
    x = np.asarray(x, dtype=float)
    y0 = np.asarray(g(x, u), dtype=float)
    J = np.zeros((y0.size, x.size))
    for j in range(x.size):
        dx = np.zeros(x.size)
        dx[j] = eps
        J[:, j] = (g(x + dx, u) - y0) / eps
    return J


def numerical_jacobian_h(h: Callable, x: Array, eps: float = 1e-6) -> Array:
    """Forward-difference Jacobian of h(x) (extended_kalman_filter.py:78-107)."""
    x = np.asarray(x, dtype=float)
    z0 = np.asarray(h(x), dtype=float)
    J = np.zeros((z0.size, x.size))
    for j in range(x.size):
        dx = np.zeros(x.size)
        dx[j] = eps
        J[:, j] = (h(x + dx) - z0) / eps
    return J


@dataclass
class EKFState:
    mean: Array
    cov: Array
    t: int


class ExtendedKalmanFilter:
    """x_k = g(x_{k-1}, u) + w, z_k = h(x_k) + v (extended_kalman_filter.py:110-160)."""

    def __init__(self, g, h, Q, R, jac_g=None, jac_h=None, *, joseph: bool = False, jitter: float = 0.0):
        self.g, self.h = g, h
        self.Q = np.asarray(Q, dtype=float)
        self.R = np.asarray(R, dtype=float)
        self.jac_g, self.jac_h = jac_g, jac_h
        self.joseph = bool(joseph)
        self.jitter = float(jitter)
        nx, nz = self.Q.shape[0], self.R.shape[0]
        assert self.Q.shape == (nx, nx), "Q must be square."
        assert self.R.shape == (nz, nz), "R must be square."

    def predict(self, state: EKFState, u: Optional[Array] = None) -> EKFState:
        """extended_kalman_filter.py:164-194."""
        x = np.asarray(state.mean, dtype=float)
        P = np.asarray(state.cov, dtype=float)
        x_pred = np.asarray(self.g(x, u), dtype=float)
        G = self.jac_g(x, u) if self.jac_g is not None else numerical_jacobian_g(self.g, x, u)
        if G.shape != (x.size, x.size):
            raise ValueError("jac_g must return shape (nx, nx).")
        return EKFState(mean=x_pred, cov=G @ P @ G.T + self.Q, t=state.t + 1)

    def update(self, pred: EKFState, z: Array) -> EKFState:
        """extended_kalman_filter.py:196-241."""
        x_pred = np.asarray(pred.mean, dtype=float)
        P_pred = np.asarray(pred.cov, dtype=float)
        z = np.asarray(z, dtype=float)
        H = self.jac_h(x_pred) if self.jac_h is not None else numerical_jacobian_h(self.h, x_pred)
        if H.shape[0] != z.size or H.shape[1] != x_pred.size:
            raise ValueError("jac_h must return shape (nz, nx).")
        y = z - np.asarray(self.h(x_pred), dtype=float)
        S = H @ P_pred @ H.T + self.R
        if self.jitter > 0.0:
            S = S + self.jitter * np.eye(z.size)
        K = P_pred @ H.T @ np.linalg.inv(S)
        x_post = x_pred + K @ y
        I = np.eye(P_pred.shape[0])
        if self.joseph:
            A = I - K @ H
            P_post = A @ P_pred @ A.T + K @ self.R @ K.T
        else:
            P_post = (I - K @ H) @ P_pred
        return EKFState(mean=x_post, cov=P_post, t=pred.t)

    def step(self, state: EKFState, z: Array, u: Optional[Array] = None) -> EKFState:
        return self.update(self.predict(state, u=u), z)


class EKFTracker:
    """GaussianTracker adaptor (LEDH_particle_filter.py:13-16) around an EKF."""

    def __init__(self, ekf: ExtendedKalmanFilter, initial_state: EKFState):
        self.ekf = ekf
        self.state = initial_state
        self.past_mean = np.asarray(initial_state.mean, float).copy()

    def predict(self) -> Tuple[Array, Array]:
        self.past_mean = self.state.mean.copy()
        self.state = self.ekf.predict(self.state, u=None)
        return self.state.mean, self.state.cov

    def update(self, z_k: Array) -> Tuple[Array, Array]:
        self.state = self.ekf.update(self.state, z_k)
        return self.state.mean, self.state.cov

    def get_past_mean(self) -> Array:
        return self.past_mean


@dataclass
class UKFState:
    mean: Array
    cov: Array
    t: int


class UnscentedKalmanFilter:
    """x_k = g(x_{k-1}, u) + w, z_k = h(x_k) + v with 2 nx + 1 sigma points
    (unscented_kalman_filter.py:68-196)."""

    def __init__(self, g, h, Q, R, *, alpha: float = 1e-3, beta: float = 2.0, kappa: float = 0.0,
                 jitter: float = 0.0):
        self.g, self.h = g, h
        self.Q = np.asarray(Q, dtype=float)
        self.R = np.asarray(R, dtype=float)
        self.alpha, self.beta, self.kappa, self.jitter = float(alpha), float(beta), float(kappa), float(jitter)
        self.nx, self.nz = int(self.Q.shape[0]), int(self.R.shape[0])
        assert self.Q.shape == (self.nx, self.nx), "Q must be (nx, nx)."
        assert self.R.shape == (self.nz, self.nz), "R must be (nz, nz)."
        # unscented-transform weights (:95-104)
        self._lambda = self.alpha ** 2 * (self.nx + self.kappa) - self.nx
        self._gamma = np.sqrt(self.nx + self._lambda)
        self.Wm = np.full(2 * self.nx + 1, 1.0 / (2.0 * (self.nx + self._lambda)))
        self.Wc = self.Wm.copy()
        self.Wm[0] = self._lambda / (self.nx + self._lambda)
        self.Wc[0] = self.Wm[0] + (1.0 - self.alpha ** 2 + self.beta)

    def _sigma_points(self, mean: Array, cov: Array) -> Array:
        """:107-126: mean, mean +- gamma * column i of chol(cov)."""
        mean = np.asarray(mean, float)
        cov = np.asarray(cov, float)
        cov = 0.5 * (cov + cov.T)
        try:
            L = np.linalg.cholesky(cov + self.jitter * np.eye(self.nx))
        except np.linalg.LinAlgError:
            L = np.linalg.cholesky(cov + max(self.jitter, 1e-12) * np.eye(self.nx))
        X = np.empty((2 * self.nx + 1, self.nx))
        X[0] = mean
        for i in range(self.nx):
            col = self._gamma * L[:, i]
            X[i + 1] = mean + col
            X[i + 1 + self.nx] = mean - col
        return X

    def predict(self, state: UKFState, u: Optional[Array] = None) -> UKFState:
        """:129-152."""
        X = self._sigma_points(state.mean, state.cov)
        Xp = np.array([self.g(xi, u) for xi in X])
        x_pred = np.sum(self.Wm[:, None] * Xp, axis=0)
        P_pred = self.Q.copy()
        DX = Xp - x_pred
        for i in range(Xp.shape[0]):
            P_pred += self.Wc[i] * np.outer(DX[i], DX[i])
        return UKFState(mean=x_pred, cov=P_pred, t=state.t + 1)

    def update(self, pred: UKFState, z: Array) -> UKFState:
        """:154-192."""
        X = self._sigma_points(pred.mean, pred.cov)
        Z = np.array([self.h(xi) for xi in X])
        z_pred = np.sum(self.Wm[:, None] * Z, axis=0)
        S = self.R.copy()
        DZ = Z - z_pred
        for i in range(Z.shape[0]):
            S += self.Wc[i] * np.outer(DZ[i], DZ[i])
        DX = X - pred.mean
        Pxz = np.zeros((self.nx, self.nz))
        for i in range(Z.shape[0]):
            Pxz += self.Wc[i] * np.outer(DX[i], DZ[i])
        S = 0.5 * (S + S.T)
        L = np.linalg.cholesky(S + self.jitter * np.eye(self.nz))
        K = np.linalg.solve(L.T, np.linalg.solve(L, Pxz.T)).T  # Pxz S^-1 by two triangular solves
        x_post = pred.mean + K @ (np.asarray(z, float) - z_pred)
        P_post = pred.cov - K @ S @ K.T
        P_post = 0.5 * (P_post + P_post.T)
        return UKFState(mean=x_post, cov=P_post, t=pred.t)

    def step(self, state: UKFState, z: Array, u: Optional[Array] = None) -> UKFState:
        return self.update(self.predict(state, u=u), z=z)


class UKFTracker:
    """GaussianTracker adaptor around a UKF (EDH_particle_filter.py:106-132)."""

    def __init__(self, ukf: UnscentedKalmanFilter, initial_state: UKFState):
        self.ukf = ukf
        self.state = initial_state
        self.past_mean = initial_state.mean.copy()

    def predict(self) -> Tuple[Array, Array]:
        self.past_mean = self.state.mean.copy()
        self.state = self.ukf.predict(self.state, u=None)
        return self.state.mean, self.state.cov

    def update(self, z_k: Array) -> Tuple[Array, Array]:
        self.state = self.ukf.update(self.state, z_k)
        return self.state.mean, self.state.cov

    def get_past_mean(self) -> Array:
        return self.past_mean


class DeviceUKFTracker:
    """:class:`UKFTracker` with its state on the GPU (``csrc/pf_ukf_dense_kernels.h``), for the
    sensor-network models: ``ukf`` is an :class:`UnscentedKalmanFilter` over ``models.ScaleTransition``
    and ``models.IdentityObservation`` or ``models.ExpObservation`` (1 <= d <= 1024, nz = nx); anything
    else raises ``NotImplementedError`` here, before the library is loaded.

    ``predict``, ``update``, ``get_past_mean`` and ``state`` mean what they mean on :class:`UKFTracker`
    and download on access.  The weighted sums are centred on sigma point 0, which removes the six-digit
    cancellation of the unscented weights at ``alpha = 1e-3``: the results are closer to exact arithmetic
    than the host tracker's, not bitwise its own.  ``sequence(Z)`` runs T predict / update pairs with one
    synchronisation.  Given to ``edh.EDHFlowPF`` / ``ledh_dense.LEDHFlowPF`` as their ``tracker``, ``run``
    drives it on the device.  ``LinAlgError`` where the host tracker raises it; the state from before the
    failing call is kept."""

    def __init__(self, ukf: UnscentedKalmanFilter, initial_state: UKFState, *, device: int = 0):
        from . import models as M

        if not isinstance(ukf, UnscentedKalmanFilter):
            raise NotImplementedError("DeviceUKFTracker takes a trackers.UnscentedKalmanFilter")
        if not isinstance(ukf.g, M.ScaleTransition):
            raise NotImplementedError("DeviceUKFTracker: g must be models.ScaleTransition")
        if not isinstance(ukf.h, (M.IdentityObservation, M.ExpObservation)):
            raise NotImplementedError("DeviceUKFTracker: h must be models.IdentityObservation or "
                                      "models.ExpObservation")
        d = int(ukf.nx)
        if ukf.nz != d or ukf.g.nx != d or ukf.h.nx != d:
            raise NotImplementedError(f"DeviceUKFTracker: g, h, Q and R must share the state dimension {d} (nz = nx)")
        if not 1 <= d <= 1024:
            raise NotImplementedError("DeviceUKFTracker takes 1 <= d <= 1024")
        mean = np.asarray(initial_state.mean, float)
        cov = np.asarray(initial_state.cov, float)
        if mean.shape != (d,) or cov.shape != (d, d):
            raise ValueError(f"the initial state must have mean ({d},) and cov ({d}, {d})")
        self.ukf = ukf
        self.nx = d
        self.device = int(device)
        self._t = int(initial_state.t)
        self._initial = (np.ascontiguousarray(mean), np.ascontiguousarray(cov))
        self._h = None  # the pf_ukf_dense_handle, made at the first use

    # ------------------------------------------------------------------ plumbing
    def _handle(self):
        from . import _native as N
        from . import models as M

        if self._h is None:
            u, exp = self.ukf, isinstance(self.ukf.h, M.ExpObservation)
            Q, R = np.ascontiguousarray(u.Q, dtype=float), np.ascontiguousarray(u.R, dtype=float)
            model = N.UkfDenseModel(self.nx, N.PF_EDH_OBS_EXP if exp else N.PF_EDH_OBS_IDENTITY, u.g.alpha,
                                    u.h.m1 if exp else 1.0, u.h.m2 if exp else 0.0, u.alpha, u.beta, u.kappa,
                                    u.jitter, N.dptr(Q), N.dptr(R))
            h = N.C.c_void_p()
            N.check(N.load().pf_ukf_dense_create(N.C.byref(model), self.device, N.C.byref(h)), "pf_ukf_dense_create")
            self._h = h
            N.check(N.load().pf_ukf_dense_set_state(h, N.dptr(self._initial[0]), N.dptr(self._initial[1])),
                    "pf_ukf_dense_set_state")
        return self._h

    def close(self) -> None:
        from . import _native as N

        if N._lib is not None and getattr(self, "_h", None) is not None and self._h.value:
            N._lib.pf_ukf_dense_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _get(self) -> Tuple[Array, Array]:
        from . import _native as N

        mean, cov = np.empty(self.nx), np.empty((self.nx, self.nx))
        N.check(N.load().pf_ukf_dense_get_state(self._handle(), N.dptr(mean), N.dptr(cov)), "pf_ukf_dense_get_state")
        return mean, cov

    @property
    def state(self) -> UKFState:
        mean, cov = self._get()
        return UKFState(mean=mean, cov=cov, t=self._t)

    @state.setter
    def state(self, st: UKFState) -> None:
        from . import _native as N

        mean = np.ascontiguousarray(np.asarray(st.mean, float).reshape(self.nx))
        cov = np.ascontiguousarray(np.asarray(st.cov, float).reshape(self.nx, self.nx))
        N.check(N.load().pf_ukf_dense_set_state(self._handle(), N.dptr(mean), N.dptr(cov)), "pf_ukf_dense_set_state")
        self._t = int(st.t)

    # ------------------------------------------------------------------ the GaussianTracker protocol
    def predict(self) -> Tuple[Array, Array]:
        from . import _native as N

        N.check(N.load().pf_ukf_dense_predict(self._handle(), None), "pf_ukf_dense_predict")
        self._t += 1
        return self._get()

    def update(self, z_k: Array) -> Tuple[Array, Array]:
        from . import _native as N

        z = np.ascontiguousarray(np.asarray(z_k, float).reshape(self.nx))
        N.check(N.load().pf_ukf_dense_update(self._handle(), N.dptr(z)), "pf_ukf_dense_update")
        return self._get()

    def get_past_mean(self) -> Array:
        from . import _native as N

        out = np.empty(self.nx)
        N.check(N.load().pf_ukf_dense_get_past_mean(self._handle(), N.dptr(out)), "pf_ukf_dense_get_past_mean")
        return out

    def sequence(self, Z: Array, U: Optional[Array] = None):
        """T predict / update pairs over ``Z [T][nx]`` (controls ``U [T][nx]`` or none) with one
        synchronisation: ``(Ps, Xbars, means, covs)``, the predicted covariances, the past means and the
        posteriors.  ``(Ps, Xbars)`` is a filter's ``tracker_seq``."""
        from . import _native as N

        Z = np.ascontiguousarray(np.asarray(Z, float).reshape(-1, self.nx))
        T = Z.shape[0]
        Uc = None if U is None else np.ascontiguousarray(np.asarray(U, float).reshape(T, self.nx))
        Ps, covs = np.empty((T, self.nx, self.nx)), np.empty((T, self.nx, self.nx))
        Xb, means = np.empty((T, self.nx)), np.empty((T, self.nx))
        N.check(N.load().pf_ukf_dense_sequence(self._handle(), N.dptr(Z), N.dptr(Uc), T, N.dptr(Ps), N.dptr(Xb),
                                               N.dptr(means), N.dptr(covs)), "pf_ukf_dense_sequence")
        self._t += T
        return Ps, Xb, means, covs
