"""Drop-in ``run_generalized_spf`` backed by the MI355X stochastic particle flow kernel.

Mirrors the reference's ``models/Stochastic_particle_filter.py`` (cited ``spf.py:LINE``):
``LinearGaussianBayes`` (12-118), ``kappa2_and_derivative`` (123-167),
``solve_beta_star_bisection`` (171-296) and ``run_generalized_spf`` (300-408) with the same names,
signatures, defaults and return values.

What runs where.  The schedule (``linspace``, or the shooting / bisection solver on ``eigh``) and
the step matrices ``S, Sinv, Q, LQ, K1, K2`` (spf.py:366-391) are O(n_steps n^3), independent of
the particles, and stay on the host in the reference's own NumPy expressions and order, so
``info`` is bitwise the reference's.  For the linear-Gaussian model every particle then sees the
same affine map plus Gaussian noise per step; :func:`fold_steps` folds the model and the step
matrices into ``x <- A_k x + c_k + G_k zeta`` and ``pf_spf_advance`` (``include/pf_spf.h``,
``csrc/pf_spf_kernels.h``) runs all the steps of the homotopy in one launch, in fp64.  There is no
CPU fallback.

What a user of the reference changes: nothing but the import.  Three keyword-only arguments are
new.  ``draws="philox"`` (the default) draws the prior and the step noise on the device
(Philox4x32-10 keyed by ``seed``); ``draws="numpy"`` reproduces the reference's stream from
``np.random.default_rng(seed)`` in the reference's call order and returns the reference's
particles up to rounding.  ``schedule=(lam, beta, betadot)`` skips the solver: the optimal
schedule costs seconds (about 60 shooting integrations of ``4 n_steps`` ``eigh`` calls) and
depends on ``(M0, Mh, mu, n_steps)`` only, so a sequential filtering loop reuses it.  ``device``
selects the GPU.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Literal, Optional, Tuple

import numpy as np

from . import _native as NV

Array = np.ndarray

__all__ = ["LinearGaussianBayes", "kappa2_and_derivative", "solve_beta_star_bisection", "run_generalized_spf",
           "step_matrices", "fold_steps", "SpfEngine"]

NUMPY_CHUNK_BYTES = 256 * 2**20  # draws="numpy": host normals uploaded per call of pf_spf_advance


@dataclass
class LinearGaussianBayes:
    """spf.py:12-118.  Prior ``x ~ N(m0, P0)``, likelihood ``z | x ~ N(H x, R)``."""

    m0: Array
    P0: Array
    H: Array
    R: Array
    z: Array

    def __post_init__(self):
        self.m0 = np.asarray(self.m0).reshape(-1)
        self.z = np.asarray(self.z).reshape(-1)
        self.P0 = np.asarray(self.P0)
        self.H = np.asarray(self.H)
        self.R = np.asarray(self.R)
        self.n = self.m0.size
        self.d = self.z.size
        assert self.P0.shape == (self.n, self.n)
        assert self.H.shape == (self.d, self.n)
        assert self.R.shape == (self.d, self.d)
        self.P0_inv = np.linalg.solve(self.P0, np.eye(self.n))
        self.R_inv = np.linalg.solve(self.R, np.eye(self.d))
        # Hessians of log p0 and log h, and M = M0 + beta Mh = -Hess log p, all symmetrised
        self.Hess_log_p0 = -self.P0_inv
        self.Hess_log_h = -(self.H.T @ self.R_inv @ self.H)
        self.M0 = -self.Hess_log_p0
        self.Mh = -self.Hess_log_h
        self.Hess_log_p0 = 0.5 * (self.Hess_log_p0 + self.Hess_log_p0.T)
        self.Hess_log_h = 0.5 * (self.Hess_log_h + self.Hess_log_h.T)
        self.M0 = 0.5 * (self.M0 + self.M0.T)
        self.Mh = 0.5 * (self.Mh + self.Mh.T)

    def grad_log_p0(self, x: Array) -> Array:
        return -self.P0_inv @ (x - self.m0)

    def grad_log_h(self, x: Array) -> Array:
        return self.H.T @ (self.R_inv @ (self.z - self.H @ x))

    def kalman_posterior(self) -> Tuple[Array, Array]:
        """Analytic posterior mean and covariance (spf.py:106-118)."""
        S = self.H @ self.P0 @ self.H.T + self.R
        K = self.P0 @ self.H.T @ np.linalg.solve(S, np.eye(self.d))
        m_post = self.m0 + K @ (self.z - self.H @ self.m0)
        P_post = (np.eye(self.n) - K @ self.H) @ self.P0
        P_post = 0.5 * (P_post + P_post.T)
        return m_post, P_post


def kappa2_and_derivative(M: Array, dM_dbeta: Array, eps: float = 1e-12) -> Tuple[float, float]:
    """Spectral condition number of ``M`` and its derivative along ``dM_dbeta`` (spf.py:123-167)."""
    M = 0.5 * (M + M.T)
    dM_dbeta = 0.5 * (dM_dbeta + dM_dbeta.T)
    n = M.shape[0]
    M_reg = M + eps * np.eye(n)
    try:
        w, V = np.linalg.eigh(M_reg)
    except np.linalg.LinAlgError:
        return 1e10, 0.0
    lam_min = float(max(np.abs(w[0]), eps))
    lam_max = float(max(np.abs(w[-1]), eps))
    vmin = V[:, 0]
    vmax = V[:, -1]
    dlam_min = float(vmin.T @ dM_dbeta @ vmin)
    dlam_max = float(vmax.T @ dM_dbeta @ vmax)
    kappa = lam_max / lam_min
    dkappa = (dlam_max / lam_min) - (lam_max * dlam_min) / (lam_min ** 2)
    return kappa, dkappa


def solve_beta_star_bisection(M0: Array, Mh: Array, mu: float, n_grid: int = 501, s_lo: float = -5.0,
                              s_hi: float = 5.0, max_bracket_expand: int = 30,
                              max_bisect_iter: int = 60) -> Tuple[Array, Array, Array]:
    """The optimal schedule ``beta'' = mu dkappa/dbeta``, ``beta(0) = 0``, ``beta(1) = 1`` by RK4
    shooting on the initial slope and bisection (spf.py:171-296).  Returns ``(lam, beta, betadot)``."""
    M0 = 0.5 * (M0 + M0.T)
    Mh = 0.5 * (Mh + Mh.T)
    lam = np.linspace(0.0, 1.0, n_grid)
    h = lam[1] - lam[0]

    def rhs(b):
        b = np.clip(b, -0.5, 1.5)
        return mu * kappa2_and_derivative(M0 + b * Mh, Mh)[1]

    def integrate(s0):
        beta = np.zeros(n_grid)
        betadot = np.zeros(n_grid)
        betadot[0] = s0
        for k in range(n_grid - 1):
            y1, y2 = beta[k], betadot[k]
            k11, k12 = y2, rhs(y1)
            k21, k22 = y2 + 0.5 * h * k12, rhs(y1 + 0.5 * h * k11)
            k31, k32 = y2 + 0.5 * h * k22, rhs(y1 + 0.5 * h * k21)
            k41, k42 = y2 + h * k32, rhs(y1 + h * k31)
            beta[k + 1] = y1 + (h / 6.0) * (k11 + 2 * k21 + 2 * k31 + k41)
            betadot[k + 1] = y2 + (h / 6.0) * (k12 + 2 * k22 + 2 * k32 + k42)
        return beta, betadot

    def miss(s0):
        return float(integrate(s0)[0][-1] - 1.0)

    f_lo, f_hi = miss(s_lo), miss(s_hi)
    grown = 0
    while np.sign(f_lo) == np.sign(f_hi) and grown < max_bracket_expand:
        s_lo *= 2.0
        s_hi *= 2.0
        f_lo, f_hi = miss(s_lo), miss(s_hi)
        grown += 1
    if np.sign(f_lo) == np.sign(f_hi):
        raise RuntimeError("Failed to bracket beta(1)=1 shooting root. Try wider initial s_lo/s_hi.")
    for _ in range(max_bisect_iter):
        s_mid = 0.5 * (s_lo + s_hi)
        f_mid = miss(s_mid)
        if abs(f_mid) < 1e-10:
            s_lo, s_hi = s_mid, s_mid
            break
        if np.sign(f_mid) == np.sign(f_lo):
            s_lo, f_lo = s_mid, f_mid
        else:
            s_hi, f_hi = s_mid, f_mid
    beta, betadot = integrate(0.5 * (s_lo + s_hi))
    beta[0] = 0.0
    beta[-1] = 1.0
    beta = np.clip(beta, 0.0, 1.0)
    return lam, beta, betadot


def step_matrices(model: LinearGaussianBayes, beta: float, beta_p: float, Q_mode: str, q_scale: float):
    """``(S, Sinv, Q, LQ, K1, K2)`` of one homotopy step (spf.py:366-391)."""
    n = model.n
    Hh = model.Hess_log_h
    S = model.Hess_log_p0 + beta * Hh
    S = 0.5 * (S + S.T)
    Sinv = np.linalg.solve(S, np.eye(n))
    if Q_mode == "scaled_identity":
        Q = (q_scale ** 2) * np.eye(n)
    elif Q_mode == "inv_M":
        Q = np.linalg.solve(-S, np.eye(n))
    else:
        raise ValueError("Q_mode must be 'scaled_identity' or 'inv_M'.")
    Q = 0.5 * (Q + Q.T)
    LQ = np.linalg.cholesky(Q + 1e-12 * np.eye(n))
    K2 = -beta_p * Sinv
    K1 = 0.5 * Q + 0.5 * beta_p * (Sinv @ Hh @ Sinv)
    return S, Sinv, Q, LQ, K1, K2


def fold_steps(model: LinearGaussianBayes, lam: Array, beta: Array, betadot: Array, Q_mode: str = "inv_M",
               q_scale: float = 1e-2) -> Array:
    """The affine form of every step, packed for ``pf_spf_advance``: ``(n_steps, 2 n^2 + n)`` rows
    ``[A_k | c_k | G_k]``.  With ``g_h(x) = b_h - Mh x`` and ``g_p(x) = (P0_inv m0 + beta b_h) +
    S_raw x`` (spf.py:399-400) the drift ``K1 g_p + K2 g_h`` (spf.py:402) is affine in ``x``:

        A_k = I + dlam (K1 S_raw - K2 Mh),          S_raw = -(P0_inv + beta_k Mh)
        c_k = dlam (K1 (P0_inv m0 + beta_k b_h) + K2 b_h),   b_h = H^T R_inv z
        G_k = sqrt(dlam) LQ_k
    """
    n = model.n
    n_steps = len(lam) - 1
    dlam = float(lam[1] - lam[0])
    b_h = model.H.T @ (model.R_inv @ model.z)
    p_m = model.P0_inv @ model.m0
    out = np.empty((n_steps, 2 * n * n + n))
    for k in range(n_steps):
        b, bp = float(beta[k]), float(betadot[k])
        _, _, _, LQ, K1, K2 = step_matrices(model, b, bp, Q_mode, q_scale)
        S_raw = -(model.P0_inv + b * model.Mh)
        A = np.eye(n) + dlam * (K1 @ S_raw - K2 @ model.Mh)
        c = dlam * (K1 @ (p_m + b * b_h) + K2 @ b_h)
        out[k, :n * n] = A.ravel()
        out[k, n * n:n * n + n] = c
        out[k, n * n + n:] = (np.sqrt(dlam) * LQ).ravel()
    return out


class SpfEngine:
    """One ``pf_spf`` handle: ``N`` particles of dimension ``n`` resident on one device."""

    def __init__(self, n_particles: int, n: int, device: int = 0):
        self.N, self.n = int(n_particles), int(n)
        self._lib = NV.load()
        hd = NV.C.c_void_p()
        opts = NV.SpfOpts(self.N, self.n, int(device))
        NV.check(self._lib.pf_spf_create(NV.C.byref(opts), NV.C.byref(hd)), "pf_spf_create")
        self._h = hd

    def set_particles(self, X: Array) -> None:
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.shape != (self.N, self.n):
            raise ValueError(f"X must be ({self.N}, {self.n}), got {X.shape}")
        NV.check(self._lib.pf_spf_set_particles(self._h, NV.dptr(X)), "pf_spf_set_particles")

    def draw_prior(self, m0: Array, L0: Array, seed: int) -> None:
        m0 = np.ascontiguousarray(m0, dtype=np.float64)
        L0 = np.ascontiguousarray(L0, dtype=np.float64)
        if m0.shape != (self.n,) or L0.shape != (self.n, self.n):
            raise ValueError(f"m0 must be ({self.n},) and L0 ({self.n}, {self.n})")
        NV.check(self._lib.pf_spf_draw_prior(self._h, NV.dptr(m0), NV.dptr(L0), int(seed) & (2**64 - 1)),
                "pf_spf_draw_prior")

    def advance(self, params: Array, k0: int = 0, seed: int = 0, Z: Optional[Array] = None) -> None:
        """Steps ``k0 .. k0 + len(params) - 1`` in one launch; ``Z`` (steps, N, n) replaces the
        device draws."""
        params = np.ascontiguousarray(params, dtype=np.float64)
        if params.ndim != 2 or params.shape[1] != 2 * self.n * self.n + self.n:
            raise ValueError(f"params must be (n_steps, {2 * self.n * self.n + self.n}), got {params.shape}")
        if Z is not None:
            Z = np.ascontiguousarray(Z, dtype=np.float64)
            if Z.shape != (params.shape[0], self.N, self.n):
                raise ValueError(f"Z must be ({params.shape[0]}, {self.N}, {self.n}), got {Z.shape}")
        NV.check(self._lib.pf_spf_advance(self._h, NV.dptr(params), int(k0), params.shape[0],
                                         int(seed) & (2**64 - 1), NV.dptr(Z)), "pf_spf_advance")

    def particles(self) -> Array:
        out = np.empty((self.N, self.n))
        NV.check(self._lib.pf_spf_get_particles(self._h, NV.dptr(out)), "pf_spf_get_particles")
        return out

    @property
    def workgroup(self) -> int:
        """Lanes per workgroup of the step launch (256, 128 or 64); it cannot change a result."""
        return int(self._lib.pf_spf_workgroup(self._h))

    @property
    def stream(self):
        return self._lib.pf_spf_stream(self._h)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            self._lib.pf_spf_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _schedule(model, n_steps, beta_mode, mu, schedule):
    if beta_mode not in ("linear", "optimal"):
        raise ValueError("beta_mode must be 'linear' or 'optimal'.")
    if schedule is not None:
        lam, beta, betadot = (np.asarray(a, dtype=np.float64) for a in schedule)
        if not (lam.shape == beta.shape == betadot.shape == (n_steps + 1,)):
            raise ValueError(f"schedule must be (lam, beta, betadot) with n_steps + 1 = {n_steps + 1} entries each")
        return lam, beta, betadot
    if beta_mode == "linear":
        lam = np.linspace(0.0, 1.0, n_steps + 1)
        return lam, lam.copy(), np.ones_like(lam)
    return solve_beta_star_bisection(model.M0, model.Mh, mu=mu, n_grid=n_steps + 1)


def run_generalized_spf(
    model: LinearGaussianBayes,
    N: int = 2000,
    n_steps: int = 300,
    beta_mode: Literal["linear", "optimal"] = "optimal",
    mu: float = 1e-2,
    Q_mode: Literal["scaled_identity", "inv_M"] = "inv_M",
    q_scale: float = 1e-2,
    seed: int = 0,
    *,
    draws: Literal["philox", "numpy"] = "philox",
    schedule: Optional[Tuple[Array, Array, Array]] = None,
    device: int = 0,
) -> Tuple[Array, Array, dict]:
    """Generalised stochastic particle flow with the normalised homotopy (spf.py:300-408) on the
    GPU.  Returns ``(X, x_hat, info)``: the final particles (N, n), their mean and
    ``info = {"lam", "beta", "betadot"}``.  Explicit Euler on a stiff prior diverges as it does in
    the reference; non-finite particles are returned as they are."""
    if draws not in ("philox", "numpy"):
        raise ValueError("draws must be 'philox' or 'numpy'.")
    n = model.n
    lam, beta, betadot = _schedule(model, n_steps, beta_mode, mu, schedule)  # a bad beta_mode raises first,
    if Q_mode not in ("scaled_identity", "inv_M"):                          # as in the reference
        raise ValueError("Q_mode must be 'scaled_identity' or 'inv_M'.")
    info = {"lam": lam, "beta": beta, "betadot": betadot}
    params = fold_steps(model, lam, beta, betadot, Q_mode, q_scale)
    L0 = np.linalg.cholesky(model.P0)
    with SpfEngine(N, n, device) as eng:
        if draws == "numpy":
            rng = np.random.default_rng(seed)
            eng.set_particles(model.m0[None, :] + rng.standard_normal((N, n)) @ L0.T)
            chunk = max(1, NUMPY_CHUNK_BYTES // (8 * N * n))
            for k0 in range(0, n_steps, chunk):
                steps = min(chunk, n_steps - k0)
                Z = np.empty((steps, N, n))
                for s in range(steps):  # the reference's call order: one (N, n) draw per step
                    rng.standard_normal(out=Z[s])
                eng.advance(params[k0:k0 + steps], k0, 0, Z)
        else:
            eng.draw_prior(model.m0.astype(np.float64), L0, seed)
            eng.advance(params, 0, seed)
        X = eng.particles()
    return X, X.mean(axis=0), info
