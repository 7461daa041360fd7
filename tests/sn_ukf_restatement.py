"""The UKF of ``trackers.UnscentedKalmanFilter`` (the reference's models/unscented_kalman_filter.py:
95-192) restated in its plain expressions with a ``dtype`` argument, for the sensor-network models:
``g(x) = g_alpha x (+ u)``, ``h`` the identity or ``m1 exp(m2 x)``, dense Q and R.

``dtype=np.longdouble`` evaluates the same filter in 80-bit extended precision (its own Cholesky and
triangular solves; the weights and gamma recomputed in that type): the yardstick of the device tracker,
whose weighted sums differ in form from the host tracker's and are not bitwise its own.  ``dtype=float``
is the matrix form in NumPy's own routines, for the sizes at which the extended form and the host
tracker's loops are too slow.

``free_run`` runs a filter over the observations of a stored case (``sn_edh_restatement.Case``) from the
notebooks' initial state; ``host_run`` does the same with ``trackers.UKFTracker``.
"""

from __future__ import annotations

import numpy as np

from particle_filters_amd import models as M
from particle_filters_amd import trackers as TR

QUANTITIES = ("Ps", "xbars", "means", "covs")  # predicted covariances, past means, posteriors


def rel(a, b):
    """max|a - b| / max(1, max|b|), in b's precision."""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a.astype(b.dtype) - b).max() / max(1.0, float(np.abs(b).max())))


def _need_extended():
    assert np.finfo(np.longdouble).nmant >= 63, (
        "np.longdouble has %d mantissa bits on this platform: the extended-precision yardstick of the UKF needs the "
        "80-bit x87 format (nmant >= 63)" % np.finfo(np.longdouble).nmant)


def cholesky(A, dtype):
    """Lower factor; LinAlgError on a pivot that is not finite and positive."""
    if dtype is float:
        return np.linalg.cholesky(A)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=dtype)
    for j in range(n):
        p = A[j, j] - L[j, :j] @ L[j, :j]
        if not (p > 0 and np.isfinite(p)):
            raise np.linalg.LinAlgError("Matrix is not positive definite")
        L[j, j] = np.sqrt(p)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_spd(L, B, dtype):
    """(L L^T)^-1 B by two triangular solves."""
    if dtype is float:
        return np.linalg.solve(L.T, np.linalg.solve(L, B))
    n = L.shape[0]
    Y = np.zeros(B.shape, dtype=dtype)
    for i in range(n):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    X = np.zeros(B.shape, dtype=dtype)
    for i in range(n - 1, -1, -1):
        X[i] = (Y[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


class UKF:
    """predict / update on (mean, cov) pairs in ``dtype``; ``model`` has g_alpha, obs ('identity' / 'exp'),
    m1, m2, Q, R."""

    def __init__(self, model, *, alpha=1e-3, beta=2.0, kappa=0.0, jitter=0.0, dtype=np.longdouble):
        if dtype is not float:
            _need_extended()
        self.dtype = dtype
        t = dtype
        self.n = n = int(np.asarray(model["Q"]).shape[0])
        self.g_alpha, self.m1, self.m2 = t(model["g_alpha"]), t(model.get("m1", 1.0)), t(model.get("m2", 0.0))
        self.exp = model["obs"] == "exp"
        self.Q = np.asarray(model["Q"], float).astype(t)
        self.R = np.asarray(model["R"], float).astype(t)
        self.jitter = t(jitter)
        a, b, k = t(alpha), t(beta), t(kappa)
        lam = a * a * (t(n) + k) - t(n)
        self.gamma = np.sqrt(t(n) + lam)
        self.Wm = np.full(2 * n + 1, t(1) / (t(2) * (t(n) + lam)), dtype=t)
        self.Wc = self.Wm.copy()
        self.Wm[0] = lam / (t(n) + lam)
        self.Wc[0] = self.Wm[0] + (t(1) - a * a + b)

    def g(self, X, u=None):
        Y = self.g_alpha * X
        return Y if u is None else Y + np.asarray(u, float).astype(self.dtype)

    def h(self, X):
        return self.m1 * np.exp(self.m2 * X) if self.exp else X

    def sigma_points(self, mean, cov):
        t, n = self.dtype, self.n
        cov = t(0.5) * (cov + cov.T)
        I = np.eye(n, dtype=t)
        try:
            L = cholesky(cov + self.jitter * I, t)
        except np.linalg.LinAlgError:
            L = cholesky(cov + max(self.jitter, t(1e-12)) * I, t)
        X = np.empty((2 * n + 1, n), dtype=t)
        X[0] = mean
        X[1:n + 1] = mean + (self.gamma * L).T
        X[n + 1:] = mean - (self.gamma * L).T
        return X

    def predict(self, mean, cov, u=None):
        X = self.sigma_points(mean, cov)
        Xp = self.g(X, u)
        x_pred = np.sum(self.Wm[:, None] * Xp, axis=0)
        DX = Xp - x_pred
        return x_pred, self.Q + (self.Wc[:, None] * DX).T @ DX

    def update(self, mean, cov, z):
        t = self.dtype
        X = self.sigma_points(mean, cov)
        Z = self.h(X)
        z_pred = np.sum(self.Wm[:, None] * Z, axis=0)
        DZ = Z - z_pred
        S = self.R + (self.Wc[:, None] * DZ).T @ DZ
        Pxz = (self.Wc[:, None] * (X - mean)).T @ DZ
        S = t(0.5) * (S + S.T)
        L = cholesky(S + self.jitter * np.eye(self.n, dtype=t), t)
        K = solve_spd(L, Pxz.T, t).T
        x_post = mean + K @ (np.asarray(z, float).astype(t) - z_pred)
        P_post = cov - K @ S @ K.T
        return x_post, t(0.5) * (P_post + P_post.T)

    def sequence(self, mean, cov, Z, U=None):
        """T predict / update pairs: dict of Ps, xbars, means, covs in ``dtype``."""
        t = self.dtype
        m, P = np.asarray(mean, float).astype(t), np.asarray(cov, float).astype(t)
        out = {q: [] for q in QUANTITIES}
        for k in range(len(Z)):
            out["xbars"].append(m.copy())
            m, P = self.predict(m, P, None if U is None else U[k])
            out["Ps"].append(P.copy())
            m, P = self.update(m, P, Z[k])
            out["means"].append(m.copy())
            out["covs"].append(P.copy())
        return {q: np.array(v) for q, v in out.items()}


def model_of(g, h, Q, R):
    exp = isinstance(h, M.ExpObservation)
    return dict(g_alpha=g.alpha, obs="exp" if exp else "identity", m1=h.m1 if exp else 1.0, m2=h.m2 if exp else 0.0,
                Q=Q, R=R)


def case_model(c):
    g, h, _, _, R = c.objects()
    return model_of(g, h, c.Q, R)


def free_run(c, dtype=np.longdouble):
    """The notebooks' UKF (alpha = 1e-3, beta = 2, kappa = 0, x0 = 0, P0 = Sigma) free-running over the T
    observations of a stored case."""
    return UKF(case_model(c), dtype=dtype).sequence(np.zeros(c.d), c.Q, c.Z)


def tracker_run(tracker, Z):
    """The same quantities from an object with UKFTracker's interface."""
    out = {q: [] for q in QUANTITIES}
    for z in Z:
        _, P = tracker.predict()
        out["Ps"].append(np.array(P, float))
        out["xbars"].append(np.array(tracker.get_past_mean(), float))
        m, P = tracker.update(z)
        out["means"].append(np.array(m, float))
        out["covs"].append(np.array(P, float))
    return {q: np.array(v) for q, v in out.items()}


def host_run(c):
    g, h, _, _, R = c.objects()
    return tracker_run(c.tracker(g, h, R), c.Z)


def host_ukf(model, *, alpha=1e-3, beta=2.0, kappa=0.0, jitter=0.0):
    """trackers.UnscentedKalmanFilter over the model objects of a restatement model dict."""
    d = int(np.asarray(model["Q"]).shape[0])
    g = M.ScaleTransition(model["g_alpha"], d)
    h = M.ExpObservation(model["m1"], model["m2"], d) if model["obs"] == "exp" else M.IdentityObservation(d)
    return TR.UnscentedKalmanFilter(g, h, model["Q"], model["R"], alpha=alpha, beta=beta, kappa=kappa, jitter=jitter)
