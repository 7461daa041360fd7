"""Vectorised NumPy restatement of the dense LEDH step for the sensor-network models, and the
fixture helpers of tests/golden/sn_ledh_runs.npz.

``flow`` restates the lambda loop of the reference's ``LEDHFlowPF.step``
(models/LEDH_particle_filter.py:136-179, cited "ledh.py:LINE") for a diagonal Jacobian
``H_i = diag(D_i)`` in the Cholesky-pair form, for all particles at once:

    S_i  = lam (D_i D_i^T o P) + R,      S'_i = (lam - dlam/2)(D_i D_i^T o P) + R
    A_i v = -1/2 P (D_i o S_i^-1 (D_i o v))                      (A_i is never formed)
    y = P (D o R^-1 (z - e)),  t1 = y + lam A y + A eta_0,  b = t1 + 2 lam A t1
    eta += dlam (A eta + b)
    theta += log det(I + dlam A_i) = 2 (sum log diag chol S'_i - sum log diag chol S_i)

(Sylvester's identity).  ``literal_flow`` is the per-particle transcription of the reference's own
formulas (explicit A_i, slogdet) that tests/test_sn_ledh_host.py holds ``flow`` against;
``ledh_step`` adds the weights of ledh.py:186-195, the resampling and the weighted statistics.
tests/golden/make_golden_sn_ledh.py checks it against the reference itself for every stored step.
"""

from __future__ import annotations

import os

import numpy as np

from particle_filters_amd import ledh_dense as LD
from particle_filters_amd import trackers as TR
from tests import sn_edh_restatement as RS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sn_ledh_runs.npz")

# case -> (d, N, L, T, process noise, wiring)
CASES = {
    "skewt16": (16, 100, 8, 6, False, "skewt"),
    "skewt25_noise": (25, 65, 3, 4, True, "skewt"),
    "skewt144": (144, 200, 8, 2, False, "skewt"),
    "snlg64": (64, 100, 4, 4, True, "snlg"),
}
RATIO = RS.RATIO
TOL_X, TOL_COV, RTOL_W, RTOL_COND = RS.TOL_X, RS.TOL_COV, RS.RTOL_W, RS.RTOL_COND


def flow(eta0, P, z, model, rdiag, L):
    """(eta_L [N][d], theta [N], condition numbers of particle 0 [L]) from eta_0 [N][d]."""
    N, d = eta0.shape
    L = max(1, int(L))
    dlam = 1.0 / float(L)
    lam = 0.0
    eta, theta, conds = eta0.copy(), np.zeros(N), []

    def chol_logdet(C):
        return 2.0 * np.sum(np.log(np.diagonal(C, axis1=1, axis2=2)), axis=1)

    for _ in range(L):
        lam = min(1.0, lam + dlam)
        D = RS.jac_diag(model, eta)                    # [N][d]
        e = RS.h_all(model, eta) - D * eta
        DPD = D[:, :, None] * P[None] * D[:, None, :]  # [N][d][d]
        S = lam * DPD + np.diag(rdiag)[None]
        S2 = (lam - 0.5 * dlam) * DPD + np.diag(rdiag)[None]
        conds.append(float(np.linalg.cond(S[0])))
        C, C2 = np.linalg.cholesky(S), np.linalg.cholesky(S2)
        Ct = np.swapaxes(C, 1, 2)

        def A(v):  # v [N][d]
            t = np.linalg.solve(C, (D * v)[:, :, None])
            t = np.linalg.solve(Ct, t)[:, :, 0]
            return -0.5 * (D * t) @ P.T

        y = (D * ((z - e) / rdiag)) @ P.T
        t1 = y + lam * A(y) + A(eta0)
        b = t1 + 2.0 * lam * A(t1)
        eta = eta + dlam * (A(eta) + b)
        theta = theta + (chol_logdet(C2) - chol_logdet(C))
    return eta, theta, conds


def literal_flow(eta0, P, z, h, jac, R, L):
    """ledh.py:136-179 particle by particle, with the reference's expressions."""
    N, d = eta0.shape
    I = np.eye(d)
    eta, theta, conds = eta0.copy(), np.zeros(N), []
    n_steps = max(1, int(L))
    dlam = 1.0 / float(n_steps)
    lam = 0.0
    for _ in range(n_steps):
        lam = min(1.0, lam + dlam)
        for i in range(N):
            Hi = jac(eta[i])
            ei = h(eta[i]) - Hi @ eta[i]
            Si = lam * Hi @ P @ Hi.T + R
            if i == 0:
                conds.append(float(np.linalg.cond(Si)))
            Ai = -0.5 * P @ Hi.T @ np.linalg.solve(Si, Hi)
            PHtRi = P @ Hi.T @ np.linalg.solve(R, z - ei)
            bi = (I + 2.0 * lam * Ai) @ ((I + lam * Ai) @ PHtRi + Ai @ eta0[i])
            eta[i] = eta[i] + dlam * (Ai @ eta[i] + bi)
            sign, logdet = np.linalg.slogdet(I + dlam * Ai)
            assert sign > 0
            theta[i] += logdet
    return eta, theta, conds


def ledh_step(X, w, P, z, model, rdiag, L, *, v=None, u=None, ratio=RATIO, U=None):
    """One step.  Returns a dict: particles, weights, ess, flag, mean, cov, conds, and eta0 / flowed /
    theta / weights_pre (before resampling)."""
    N = X.shape[0]
    gx = model["alpha"] * X
    eta0 = gx.copy()
    if u is not None:
        eta0 = eta0 + u
    if v is not None:
        eta0 = eta0 + v
    xk, theta, conds = flow(eta0, P, z, model, rdiag, L)
    Lc = np.linalg.cholesky(model["Q"])
    q_x = np.sum(np.linalg.solve(Lc, (xk - gx).T) ** 2, axis=0)
    q_v = np.sum(np.linalg.solve(Lc, (eta0 - gx).T) ** 2, axis=0)
    logw = np.log(w + 1e-300) + theta + (-0.5 * q_x + RS.log_like_all(model, z, xk) + 0.5 * q_v)
    logw = logw - np.max(logw)
    wn = np.exp(logw)
    wn = wn / np.sum(wn)
    wnn = wn / np.sum(wn)
    ess = 1.0 / float(np.sum(wnn * wnn))
    flag = bool(ratio > 0.0 and ess < ratio * N)
    out = dict(eta0=eta0, flowed=xk, theta=theta, weights_pre=wn, ess=ess, flag=flag, conds=conds)
    if flag:
        cdf = np.cumsum(wn / np.sum(wn))
        idx = np.minimum(np.searchsorted(cdf, (U + np.arange(N)) / N, side="right"), N - 1)
        xk, wn = xk[idx], np.full(N, 1.0 / N)
    out["particles"], out["weights"] = xk, wn
    out["mean"], out["cov"] = RS.weighted_stats(xk, wn)
    return out


# ---------------------------------------------------------------- fixture helpers
class Case:
    """One stored case with its inputs rebuilt."""

    def __init__(self, G, name):
        self.name = name
        self.d, self.N, self.L, self.T, self.noise, self.wiring = CASES[name]
        k = lambda f: G[f"{name}__{f}"]  # noqa: E731
        self.has = lambda f: f"{name}__{f}" in G  # noqa: E731
        self.k = k
        d = self.d
        self.Q = RS.sym_unpack(k("Sigma"), d)
        self.Z = np.asarray(k("Z"), float)
        self.alpha, self.m1, self.m2, self.sigma_z = (float(x) for x in k("params"))
        self.Lc = np.linalg.cholesky(self.Q)
        self.init = (np.asarray(k("init_particles"), float) if self.has("init_particles")
                     else RS.seeded_normals(k("init_seed"), (self.N, d), self.Lc))
        if self.noise:
            self.V = (np.asarray(k("V"), float) if self.has("V")
                      else RS.seeded_normals(k("noise_seed"), (self.T, self.N, d), self.Lc))
        else:
            self.V = None
        self.U = np.asarray(k("U"), float)  # [T], nan where the step did not resample
        self.model = RS.model_dict(self.wiring, d, self.alpha, self.m1, self.m2, self.sigma_z, self.Q)

    def objects(self):
        return RS.model_objects(self.wiring, self.d, self.alpha, self.m1, self.m2, self.sigma_z, self.Q)

    def tracker(self, g, h, R):
        """The notebooks' trackers from x0 = 0, P0 = Sigma: the UKF (alpha = 1e-3, beta = 2, kappa = 0)
        of the skewed-t notebook, the EKF of the SNLG notebook."""
        if self.wiring == "skewt":
            ukf = TR.UnscentedKalmanFilter(g, h, self.Q, R, alpha=1e-3, beta=2.0, kappa=0.0)
            return TR.UKFTracker(ukf, TR.UKFState(mean=np.zeros(self.d), cov=self.Q.copy(), t=0))
        ekf = TR.ExtendedKalmanFilter(g, h, self.Q, R, jac_g=g.jacobian, jac_h=h.jacobian)
        return TR.EKFTracker(ekf, TR.EKFState(mean=np.zeros(self.d), cov=self.Q.copy(), t=0))

    def config(self, rng):
        return LD.LEDHConfig(n_particles=self.N, n_lambda_steps=self.L, resample_ess_ratio=RATIO, rng=rng)

    def stored_P(self):
        """[T] symmetrised predicted covariances."""
        return [RS.sym_unpack(p, self.d) for p in self.k("P")]

    def stored(self, field):
        """{t: array} of a per-step field stored for the steps listed in <field>_steps."""
        steps = [int(t) for t in self.k(field + "_steps")]
        vals = self.k(field)
        if field == "covs":
            vals = [RS.sym_unpack(c, self.d) for c in vals]
        return dict(zip(steps, vals))


ReplayUniforms = RS.ReplayUniforms


def load():
    return np.load(GOLDEN)
