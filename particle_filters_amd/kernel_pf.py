"""Drop-in ``KernelParticleFilter`` backed by the MI355X kernel particle flow kernels.

Mirrors the reference's ``models/kernel_particle_filter.py`` (cited ``kpf.py:LINE``):
``gaspari_cohn`` (10-49), ``build_localization_matrix`` (52-80), ``Model`` (210-226),
``KPFConfig`` (229-242), ``KPFState`` (245-252) and ``KernelParticleFilter`` with the same
constructor (268-270) and ``analyze(X, y, lengthscales=None, rng=None)`` (324-447).

What runs where.  The prior statistics - mean, localised covariance ``B``, ``B_inv`` and the
lengthscales (kpf.py:288-302, 352-370) - are O(Np nx^2) once per call and stay on the host, in the
reference's own NumPy expressions, so ``B_inv`` is bitwise the reference's.  The pseudo-time
schedule (kpf.py:390-445) depends on the configuration only and is computed up front
(:func:`pseudo_time_schedule`).  Everything per particle and per pair - the scores, the all-pairs
RBF velocity and the clipped update of every step - is one stream-ordered sequence of HIP launches
(``pf_kpf_analyze``, ``csrc/pf_kpf_kernels.h``).  There is no CPU fallback.

What a user of the reference changes: ``Model.H`` is one of this package's observation objects
(:class:`models.LinearObservation` and its subclasses, :class:`models.ExpHalfObservation`,
:class:`models.AcousticObservation`) and ``Model.JH`` its ``jacobian`` (or ``None``): the device
evaluates the analytic Jacobian.  ``KPFState`` has one more field, ``n_clipped``: per pseudo-time
step, the number of particles whose move was scaled down to ``c_move_max``.

The velocities of a step are all formed from the old ensemble, so ``random_order`` cannot change
the result; a caller's ``rng`` is advanced exactly as the reference advances it (one
``shuffle(arange(Np))`` per step) so that code after ``analyze`` sees the same stream.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import numpy as np

from . import _native as N
from . import models as M

Array = np.ndarray

__all__ = ["KernelParticleFilter", "Model", "KPFConfig", "KPFState", "gaspari_cohn", "build_localization_matrix",
           "pseudo_time_schedule"]

_SUPPORTED = "models.LinearObservation (and its subclasses), models.ExpHalfObservation, models.AcousticObservation"


def gaspari_cohn(r: Array) -> Array:
    """Gaspari-Cohn compactly supported correlation of the scaled distance ``r`` (cut-off at 2)."""
    r = np.asarray(r, dtype=float)
    out = np.zeros_like(r)
    near = (r >= 0) & (r <= 1)
    q = r[near]
    out[near] = 1 - 5 * q**2 / 3 + 5 * q**3 / 8 + q**4 / 2 - q**5 / 4
    far = (r > 1) & (r <= 2)
    q = r[far]
    out[far] = 4 - 5 * q + 5 * q**2 / 3 + 5 * q**3 / 8 - q**4 / 2 + q**5 / 12 - 2 / (3 * q)
    return out


def build_localization_matrix(n: int, radius: float, metric: Optional[Array] = None) -> Array:
    """Gaspari-Cohn localisation matrix (n, n): ``metric`` holds the pairwise distances (default
    the 1-D chain ``|i - j|``), ``radius`` scales them; ``np.inf`` disables localisation."""
    if np.isinf(radius):
        return np.ones((n, n))
    if metric is None:
        idx = np.arange(n)
        D = np.abs(idx[:, None] - idx[None, :])
    else:
        D = np.asarray(metric, dtype=float)
        if D.shape != (n, n):
            raise ValueError("metric must be (n, n).")
    return gaspari_cohn(D / float(radius))


@dataclass
class Model:
    """kpf.py:210-226.  ``H``: a device observation object; ``JH``: ``H.jacobian`` or None; ``R``
    the observation noise covariance (nz, nz)."""

    H: Callable[[Array], Array]
    JH: Optional[Callable[[Array], Array]]
    R: Array


@dataclass
class KPFConfig:
    """kpf.py:229-242."""

    ds_init: float = 0.2
    ds_min: float = 1e-3
    c_move_max: float = 2.0
    min_steps: int = 5
    max_steps: int = 100
    kernel_type: str = "diagonal"
    lengthscale_mode: str = "std"
    fixed_lengthscale: float = 1.0
    reg: float = 1e-6
    localization_radius: float = np.inf
    random_order: bool = True


@dataclass
class KPFState:
    """kpf.py:245-252, plus ``n_clipped`` (per step: particles scaled down to ``c_move_max``)."""

    particles: Array
    weights: Array
    s: float
    steps: int
    ds_history: list = None
    n_clipped: list = None


def pseudo_time_schedule(cfg: KPFConfig) -> Tuple[List[float], float, int]:
    """The pseudo-time loop of kpf.py:390-445 without the particles: ``(ds_history, s, steps)``.
    The step sizes depend on the configuration only (the per-particle clip leaves ``ds`` alone)."""
    s, steps, ds = 0.0, 0, cfg.ds_init
    hist: List[float] = []
    while (s < 1.0 and steps < cfg.max_steps) or (steps < cfg.min_steps):
        steps += 1
        if s + ds > 1.0:
            ds = 1.0 - s
        hist.append(float(ds))
        s += ds
        if ds <= cfg.ds_min and (1.0 - s) < 1e-6:
            break
    return hist, s, steps


class KernelParticleFilter:
    """Kernel particle flow filter on an MI355X (drop-in for kpf.py:256-447)."""

    def __init__(self, model: Model, config: Optional[KPFConfig] = None, *, device: int = 0):
        self.model = model
        self.cfg = config or KPFConfig()
        self.device = int(device)
        h = model.H
        if not (isinstance(h, M.Observation)
                and h.kind in (N.PF_OBS_LINEAR, N.PF_OBS_EXP_HALF, N.PF_OBS_ACOUSTIC)):
            raise NotImplementedError(f"the HIP kernel particle flow needs Model.H to be one of {_SUPPORTED}; "
                                      f"got {type(h).__name__}")
        if model.JH is not None and getattr(model.JH, "__self__", None) is not h:
            raise NotImplementedError("Model.JH must be None or Model.H.jacobian (the model's analytic Jacobian)")
        self._R = np.ascontiguousarray(np.atleast_2d(np.asarray(model.R, dtype=float)))
        if self._R.shape != (h.nz, h.nz):
            raise ValueError(f"R must be ({h.nz}, {h.nz}) for this observation, got {self._R.shape}")
        if not N.load().pf_kpf_model_supported(h.nx, h.nz, h.kind):
            raise NotImplementedError(f"observation shape (nx={h.nx}, nz={h.nz}) is not supported by the HIP "
                                      f"kernel particle flow ({_SUPPORTED})")
        self._h = None
        self._h_np = -1

    # ------------------------------------------------------------------ host-side statistics
    @staticmethod
    def mean_and_cov(X: Array, reg: float = 0.0) -> Tuple[Array, Array]:
        """kpf.py:273-281."""
        mu = X.mean(axis=0)
        A = X - mu
        B = (A.T @ A) / max(1, X.shape[0] - 1)
        if reg > 0:
            B = B + reg * np.eye(B.shape[0])
        return mu, B

    def _prior_stats(self, X: Array) -> Tuple[Array, Array]:
        """kpf.py:288-294."""
        x0, B = self.mean_and_cov(X, reg=self.cfg.reg)
        L = build_localization_matrix(B.shape[0], self.cfg.localization_radius)
        return x0, np.multiply(B, L)

    def _lengthscales(self, X: Array, mode: str) -> Array:
        """kpf.py:296-302."""
        if mode == "fixed":
            return np.full(X.shape[1], self.cfg.fixed_lengthscale, dtype=float)
        return X.std(axis=0) + 1e-12

    def prior(self, X: Array, lengthscales=None):
        """``(x0, B, B_inv, ell)`` of one analysis (kpf.py:352-370); ``ell`` has nx entries (the
        scalar kernel's single lengthscale repeated)."""
        cfg = self.cfg
        n = X.shape[1]
        x0, B = self._prior_stats(X)
        B_inv = np.linalg.inv(B + cfg.reg * np.eye(n))
        if cfg.kernel_type == "scalar":
            if lengthscales is not None:
                ell = float(lengthscales) if np.isscalar(lengthscales) else float(lengthscales[0])
            elif cfg.lengthscale_mode == "fixed":
                ell = cfg.fixed_lengthscale
            else:
                ell = float(X.std(axis=0).mean())
            ell = np.full(n, ell, dtype=float)
        else:
            ell = lengthscales if lengthscales is not None else self._lengthscales(X, cfg.lengthscale_mode)
            ell = np.asarray(ell, dtype=float)
            if ell.shape != (n,):
                raise ValueError("lengthscales must be shape (n,)")
        return x0, B, B_inv, ell

    # ------------------------------------------------------------------ device handle
    def _handle(self, Np: int):
        if self._h is not None and self._h_np == Np:
            return self._h
        self.close()
        h = self.model.H
        op = np.ascontiguousarray(h.params(), dtype=float)
        desc = N.ModelDesc(h.nx, h.nz, N.PF_TRANS_LINEAR, h.kind, None, 0, N.dptr(op), op.size, None,
                           N.dptr(self._R))
        kt = N.PF_KPF_SCALAR if self.cfg.kernel_type == "scalar" else N.PF_KPF_DIAGONAL
        opts = N.KpfOpts(Np, kt, self.device)
        hd = N.C.c_void_p()
        N.check(N.load().pf_kpf_create(N.C.byref(desc), N.C.byref(opts), N.C.byref(hd)), "pf_kpf_create")
        self._h, self._h_np, self._h_kt = hd, Np, kt
        return hd

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            N.load().pf_kpf_destroy(self._h)
            self._h = None
            self._h_np = -1

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ analysis
    def analyze(self, X: Array, y: Array, lengthscales: Optional[Array] = None,
                rng: Optional[np.random.Generator] = None) -> KPFState:
        """Move the prior ensemble ``X`` (Np, n) to the posterior given ``y`` (kpf.py:324-447)."""
        X = np.ascontiguousarray(np.asarray(X, dtype=float))
        y = np.ascontiguousarray(np.asarray(y, dtype=float))
        Np, n = X.shape  # a ValueError for anything but a 2-D ensemble, as in the reference
        h = self.model.H
        if n != h.nx:
            raise ValueError(f"X must be (Np, {h.nx}) for this observation, got {X.shape}")
        if y.shape != (h.nz,):
            raise ValueError(f"y must be ({h.nz},), got {y.shape}")
        cfg = self.cfg
        x0, B, B_inv, ell = self.prior(X, lengthscales)
        ds_hist, s, steps = pseudo_time_schedule(cfg)
        if self._h is not None and self._h_kt != (N.PF_KPF_SCALAR if cfg.kernel_type == "scalar"
                                                  else N.PF_KPF_DIAGONAL):
            self.close()
        hd = self._handle(Np)
        ds = np.ascontiguousarray(ds_hist, dtype=float)
        out = np.empty_like(X)
        clip = np.zeros(max(1, steps), dtype=np.int32)
        N.check(N.load().pf_kpf_analyze(
            hd, N.dptr(X), N.dptr(y), N.dptr(np.ascontiguousarray(x0, dtype=float)),
            N.dptr(np.ascontiguousarray(B, dtype=float)), N.dptr(np.ascontiguousarray(B_inv, dtype=float)),
            N.dptr(np.ascontiguousarray(ell, dtype=float)), N.dptr(ds), steps, float(cfg.c_move_max), N.dptr(out),
            clip.ctypes.data_as(N.C.POINTER(N.C.c_int32))), "pf_kpf_analyze")
        if cfg.random_order and rng is not None:
            for _ in range(steps):  # kpf.py:399-401: the draws the reference consumes, and nothing else
                rng.shuffle(np.arange(Np))
        return KPFState(particles=out, weights=np.full(Np, 1.0 / Np), s=s, steps=steps, ds_history=ds_hist,
                        n_clipped=[int(c) for c in clip[:steps]])
