"""NumPy restatement of the device composition of the dense EDH flow map
(csrc/pf_edh_flowmap_kernels.h): the lambda loop of edh.py:216-280 for ``H = diag(D)`` and a diagonal
flow ``R = diag(r)`` in its Cholesky form.

Per lambda step: ``S = lam (D D^T o P) + diag(r) = L L^T``, ``K = S^-1 diag(D)`` through the two
triangular solves, ``A = -1/2 (P diag(D)) K``, ``y = P (D o (z - e) / r)``,
``b = (I + 2 lam A)((I + lam A) y + A etabar)``, then ``Phi`` / ``psi`` as ``edh.compose_flow_map``
and ``etabar <- Phi etabar + psi``.  tests/test_sn_edh_flowmap_host.py checks it against
``edh.compose_flow_map`` on the stored cases.
"""

from __future__ import annotations

import numpy as np


def jac_and_h(obs, m1, m2, x):
    """(D, h(x)) of the elementwise observation: identity, or m1 exp(m2 x)."""
    if obs == "exp":
        hx = m1 * np.exp(m2 * x)
        return m2 * hx, hx
    return np.ones_like(x), x.copy()


def compose(P, etabar, z, obs, m1, m2, r, n_steps, integrator):
    """(M, c, trace): the composed map and etabar before each lambda step.  Raises ``LinAlgError``
    when S is not positive definite."""
    d = etabar.size
    I = np.eye(d)
    n_steps = max(1, int(n_steps))
    dlam = 1.0 / float(n_steps)
    lam = 0.0
    Mc, cc = np.eye(d), np.zeros(d)
    etabar = np.array(etabar, dtype=float)
    trace = np.empty((n_steps, d))
    for j in range(n_steps):
        lam = min(1.0, lam + dlam)
        trace[j] = etabar
        D, hx = jac_and_h(obs, m1, m2, etabar)
        e = hx - D * etabar
        S = lam * (D[:, None] * P * D[None, :]) + np.diag(r)
        Lc = np.linalg.cholesky(S)
        K = np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.diag(D)))
        A = -0.5 * (P * D[None, :]) @ K
        y = P @ (D * (z - e) / r)
        b = (I + 2.0 * lam * A) @ ((I + lam * A) @ y + A @ etabar)
        E = dlam * A
        if integrator == "euler":
            Phi, psi = I + E, dlam * b
        else:
            G = I + (E / 2.0) @ (I + (E / 3.0) @ (I + E / 4.0))
            Phi, psi = I + E @ G, dlam * (G @ b)
        etabar = Phi @ etabar + psi
        Mc, cc = Phi @ Mc, Phi @ cc + psi
    return Mc, cc, trace
