#!/usr/bin/env python
"""Generate tests/golden/spf_runs.npz by running the REFERENCE stochastic particle flow filter.

Build container only:  PF_REFERENCE=<reference checkout> python tests/golden/make_golden_spf.py

Imports the reference's ``models.Stochastic_particle_filter`` and runs ``run_generalized_spf`` on
fixed seeds (no GPU is touched).  Only numbers are stored: the model, the arguments, the seed, the
reference's final particles, ``x_hat`` and ``lam`` / ``beta`` / ``betadot``; the first and the
last four normals of the reference's stream (replayed from the seed in its call order), so that a
change of NumPy's stream shows as such and not as a parity failure; and reference values of
``LinearGaussianBayes``, ``kalman_posterior`` and ``kappa2_and_derivative``.  No draws are stored:
the tests regenerate them from the seed.

The inputs are well conditioned (cond(P0) <= 10, R >= 0.1 I); explicit Euler on a stiff prior
diverges in the reference itself.  For every case this script asserts that
  * max|X| <= 100;
  * the faithful restatement (tests/spf_restatement.py) equals the reference to
    1e-12 x max(1, max|X|) and the folded one to 1e-11 x max(1, max|X|);
  * this package's host mirror returns lam / beta / betadot bitwise equal to the reference's.
"""

from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
REF = os.environ["PF_REFERENCE"]  # a checkout of the reference project
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from models import Stochastic_particle_filter as RS  # noqa: E402  (reference)

from particle_filters_amd import stochastic_pf as SP  # noqa: E402
from tests import spf_restatement as SR  # noqa: E402

# name: (model seed, n, d, cond(P0), N, n_steps, beta_mode, mu, Q_mode, q_scale, seed)
CASES = {
    "a_default": (11, 4, 2, 4.0, 200, 100, "optimal", 1e-2, "inv_M", 1e-2, 0),
    "b_linear": (12, 4, 2, 10.0, 257, 50, "linear", 1e-2, "inv_M", 1e-2, 1),
    "c_scaled_d1": (13, 3, 1, 4.0, 64, 40, "optimal", 1e-2, "scaled_identity", 1e-2, 2),
    "d_scaled_linear_full": (14, 5, 5, 6.0, 65, 30, "linear", 1e-2, "scaled_identity", 0.2, 3),
    "e_n9": (15, 9, 4, 8.0, 100, 100, "optimal", 1e-2, "inv_M", 1e-2, 4),
    "f_n9_full": (16, 9, 9, 10.0, 63, 20, "linear", 1e-2, "inv_M", 1e-2, 5),
    "g_scalar": (17, 1, 1, 1.0, 50, 25, "optimal", 1e-2, "inv_M", 1e-2, 6),
    "h_one_step": (18, 2, 1, 2.0, 10, 1, "optimal", 1e-2, "inv_M", 1e-2, 7),
    "i_two_steps": (19, 2, 2, 2.0, 33, 2, "linear", 1e-2, "scaled_identity", 0.05, 8),
    "j_mu": (20, 8, 3, 5.0, 33, 60, "optimal", 1e-1, "scaled_identity", 0.05, 9),
    "k_one_particle": (21, 6, 2, 3.0, 1, 10, "linear", 1e-2, "inv_M", 1e-2, 10),
    "l_n7_full": (22, 7, 7, 9.0, 129, 80, "optimal", 1e-3, "inv_M", 1e-2, 2**40 + 3),
}


def main():
    out = {"names": np.array(list(CASES))}
    for name, (ms, n, d, cond, N, n_steps, beta_mode, mu, Q_mode, q_scale, seed) in CASES.items():
        m = SR.random_model(ms, n, d, cond)
        assert np.linalg.cond(m.P0) <= 10.0 * (1 + 1e-12) and np.linalg.eigvalsh(m.R)[0] >= 0.1
        ref = RS.LinearGaussianBayes(m0=m.m0, P0=m.P0, H=m.H, R=m.R, z=m.z)
        X, x_hat, info = RS.run_generalized_spf(ref, N=N, n_steps=n_steps, beta_mode=beta_mode, mu=mu, Q_mode=Q_mode,
                                                q_scale=q_scale, seed=seed)
        scale = max(1.0, float(np.max(np.abs(X))))
        assert np.all(np.isfinite(X)) and scale <= 100.0, (name, scale)
        lam, beta, betadot = info["lam"], info["beta"], info["betadot"]
        mine = SP._schedule(m, n_steps, beta_mode, mu, None)
        assert all(np.array_equal(a, b) for a, b in zip(mine, (lam, beta, betadot))), name
        draw = SR.numpy_draws(seed, N, n)
        Xf = SR.faithful(m, SR.prior(m, draw), draw, lam, beta, betadot, Q_mode, q_scale)
        draw = SR.numpy_draws(seed, N, n)
        params = SP.fold_steps(m, lam, beta, betadot, Q_mode, q_scale)
        Xa = SR.folded(params, SR.prior(m, draw), draw, n)
        e_f, e_a = float(np.max(np.abs(Xf - X))), float(np.max(np.abs(Xa - X)))
        assert e_f <= 1e-12 * scale, (name, e_f)
        assert e_a <= 1e-11 * scale, (name, e_a)
        draw = SR.numpy_draws(seed, N, n)
        first = draw(0).ravel()[:4].copy()
        for k in range(n_steps):
            last = draw(k + 1).ravel()[-4:].copy()
        print(f"{name:>22s}: max|X|={scale:.3g} faithful err={e_f:.2e} folded err={e_a:.2e}")
        rec = dict(m0=m.m0, P0=m.P0, H=m.H, R=m.R, z=m.z, N=N, n_steps=n_steps, beta_mode=SR.BETA_MODES.index(beta_mode),
                   mu=mu, Q_mode=SR.Q_MODES.index(Q_mode), q_scale=q_scale, seed=seed, X=X, x_hat=x_hat, lam=lam,
                   beta=beta, betadot=betadot, first_normals=first, last_normals=last)
        mp, Pp = ref.kalman_posterior()
        kap = np.array([RS.kappa2_and_derivative(ref.M0 + b * ref.Mh, ref.Mh) for b in (0.0, 0.3, 1.0)])
        rec.update(P0_inv=ref.P0_inv, R_inv=ref.R_inv, Hess_log_p0=ref.Hess_log_p0, Hess_log_h=ref.Hess_log_h, M0=ref.M0,
                   Mh=ref.Mh, m_post=mp, P_post=Pp, kappa=kap, grad_p0=ref.grad_log_p0(m.m0 + 1.0),
                   grad_h=ref.grad_log_h(m.m0 + 1.0))
        for k, v in rec.items():
            out[f"{name}__{k}"] = np.asarray(v)
    path = os.path.join(HERE, "spf_runs.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
