#!/usr/bin/env python
"""Generate tests/golden/sn_ledh_runs.npz by running the REFERENCE LEDH filter on the sensor-network
models (PF_PF_results_reproduction_sn_skew.ipynb / _snlg.ipynb).

Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sn_ledh.py

Imports the reference's ``models.LEDH_particle_filter.LEDHFlowPF`` with its own trackers (the UKF of
the skewed-t notebook, the EKF of the SNLG notebook) and drives them with this package's model
objects (particle_filters_amd.models: the reference's call signatures) on data of the reference's
simulators, with a recording ``config.rng``.  Only numbers are stored: the inputs (Sigma, Z,
parameters, initial particles or their seed), the random stream consumed (process noise or its
seed, the resampling uniforms), the tracker's symmetrised predicted covariances and the per-step
outputs (the large case skewt144: particles and covariance at the last step only).  To keep the
file below 1 MB, symmetric matrices are stored as upper triangles, the two large cases store their
initial particles by seed, and snlg64 stores its process noise by seed.

Every stored step satisfies |ESS - ratio N| / N >= 1e-3, so no resample decision hinges on rounding,
and each small case (skewt16, skewt25_noise) holds both resampling and non-resampling steps; with host
process noise most seeds resample at every step, and the seeds of skewt25_noise below are chosen so
that its third step does not.  snlg64 is the exception: with the notebook's wiring its ESS / N stayed
at or below 0.1 at every step for every seed tried, so it resamples at every step, its stored weights
are uniform, and its weights before resampling are held through the stored ESS.  The reference does not return
its ESS: the stored ``ess`` is the restatement's, of the weights before resampling, on the
reference's own inputs of that step.  The vectorised restatement (tests/sn_ledh_restatement.py) is
checked against the reference here, at the bounds of tests/sn_edh_restatement.py.
"""

from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get("PF_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from models.LEDH_particle_filter import LEDHFlowPF, LEDHConfig, PFState  # noqa: E402  (reference)
from models.EDH_particle_filter import EKFTracker, UKFTracker  # noqa: E402  (reference)
from models.extended_kalman_filter import ExtendedKalmanFilter, EKFState  # noqa: E402  (reference)
from models.unscented_kalman_filter import UnscentedKalmanFilter, UKFState  # noqa: E402  (reference)
from simulator import simulator_sensor_network_skewt_dynamic as SK  # noqa: E402  (reference)
from simulator import simulator_sensor_network_linear_gaussian as LG  # noqa: E402  (reference)

from tests import sn_edh_restatement as RS  # noqa: E402
from tests import sn_ledh_restatement as LR  # noqa: E402

# seeds of (data, initial particles, filter rng / noise)
SEEDS = {"skewt16": (42, 1, 11), "skewt25_noise": (101, 201, 301), "skewt144": (42, 4, 14), "snlg64": (123, 5, 15)}
BIG = ("skewt144", "snlg64")  # initial particles by seed
NOISE_BY_SEED = ("snlg64",)
LAST_ONLY = ("skewt144",)     # particles and covariance at the last step only
BOTH_KINDS = ("skewt16", "skewt25_noise")  # the small cases: a resampling and a non-resampling step each


class Rec:
    """config.rng of the reference filter: logs the uniforms systematic_resample draws."""

    def __init__(self, gen):
        self.gen, self.uniforms = gen, []

    def random(self, size=None):
        u = self.gen.random(size)
        self.uniforms.append(float(u))
        return u

    def multivariate_normal(self, mean, cov, size=None):
        return self.gen.multivariate_normal(mean, cov, size=size)


def data_of(name):
    d, N, L, T, noise, wiring = LR.CASES[name]
    seed = SEEDS[name][0]
    if wiring == "skewt":
        grid = SK.GridConfig(d=d, alpha0=1.0, alpha1=1e-3, beta=8.0)
        dyn = SK.DynConfig(alpha=0.9, nu=8.0, gamma_scale=0.1, gamma_vec=None, clip_x=(-10.0, 10.0), seed=seed)
        meas = SK.MeasConfig(m1=1.0, m2=1.0 / 3.0)
        data = SK.simulate_many(grid, dyn, meas, SK.SimConfig(T=T, n_trials=1, save_lambda=True))
        return data["Sigma_list"][0], np.asarray(data["Z"][0], float), (0.9, 1.0, 1.0 / 3.0, 0.0)
    cfg = LG.SimConfig(d=d, T=T, trials=1, sigmas=(1.0,), seed=seed)
    _, Z, _, Sigma = LG.simulate_dataset(cfg)
    return Sigma, np.asarray(Z[0, 0], float), (cfg.alpha, 1.0, 0.0, 1.0)


def ref_tracker(wiring, g, h, Sigma, R, d):
    if wiring == "skewt":
        ukf = UnscentedKalmanFilter(g, h, Sigma, R, alpha=1e-3, beta=2.0, kappa=0.0)
        return UKFTracker(ukf, UKFState(mean=np.zeros(d), cov=Sigma.copy(), t=0))
    ekf = ExtendedKalmanFilter(g=g, h=h, jac_g=g.jacobian, jac_h=h.jacobian, Q=Sigma, R=R)
    return EKFTracker(ekf, EKFState(mean=np.zeros(d), cov=Sigma.copy(), t=0))


def run_case(name):
    d, N, L, T, noise, wiring = LR.CASES[name]
    Sigma, Z, params = data_of(name)
    Sigma = 0.5 * (Sigma + Sigma.T)
    alpha, m1, m2, sigma_z = params
    Lc = np.linalg.cholesky(Sigma)
    g, h, ltp, llp, R = RS.model_objects(wiring, d, alpha, m1, m2, sigma_z, Sigma)
    _, init_seed, run_seed = SEEDS[name]
    init = RS.seeded_normals(init_seed, (N, d), Lc)
    rec = Rec(np.random.default_rng(run_seed))
    Vlog = []
    if noise and name in NOISE_BY_SEED:
        Vall = RS.seeded_normals(run_seed + 1000, (T, N, d), Lc)

        def sampler(n, nx):
            Vlog.append(Vall[len(Vlog)])
            return Vlog[-1]
    elif noise:
        def sampler(n, nx):
            Vlog.append(rec.multivariate_normal(np.zeros(nx), Sigma, size=n))
            return Vlog[-1]
    else:
        sampler = None
    cfg = LEDHConfig(n_particles=N, n_lambda_steps=L, resample_ess_ratio=LR.RATIO, rng=rec)
    pf = LEDHFlowPF(ref_tracker(wiring, g, h, Sigma, R, d), g, h, h.jacobian, ltp, llp, R, cfg)
    st = PFState(particles=init.copy(), weights=np.full(N, 1.0 / N), mean=np.zeros(d), cov=Sigma.copy())
    model = RS.model_dict(wiring, d, alpha, m1, m2, sigma_z, Sigma)
    rdiag = np.diag(R).copy()

    big = name in BIG
    out = {"Sigma": RS.sym_pack(Sigma), "Z": Z, "params": np.array(params), "init_seed": np.array(init_seed)}
    if not big:
        out["init_particles"] = init
    means, covs, weights, ess, flags, conds, U, Ps, parts = [], [], [], [], [], [], [], [], []
    for t in range(T):
        n_u = len(rec.uniforms)
        st = pf.step(st, Z[t], process_noise_sampler=sampler)
        assert np.all(np.isfinite(st.weights)) and np.all(np.isfinite(st.particles)), (name, t)
        flag = len(rec.uniforms) > n_u
        U.append(rec.uniforms[-1] if flag else np.nan)
        means.append(st.mean); covs.append(st.cov); weights.append(st.weights); parts.append(st.particles)
        conds.append(st.diagnostics["condition_numbers"]); flags.append(flag)
    # second, identical tracker (it never sees the particles): P_t
    tr2 = ref_tracker(wiring, g, h, Sigma, R, d)
    for t in range(T):
        _, P = tr2.predict()
        Ps.append(0.5 * (np.array(P) + np.array(P).T))
        tr2.update(Z[t])
    # the restatement against the reference, step by step on the reference's own inputs
    err = dict(x=0.0, w=0.0, cov=0.0, cond=0.0)
    scale = max(1.0, float(np.max(np.abs(np.array(parts)))))
    X, w = init.copy(), np.full(N, 1.0 / N)
    for t in range(T):
        r = LR.ledh_step(X, w, Ps[t], Z[t], model, rdiag, L, v=Vlog[t] if noise else None, U=U[t])
        ess.append(r["ess"])
        assert r["flag"] == flags[t], (name, t)
        margin = abs(r["ess"] - LR.RATIO * N) / N
        assert margin >= 1e-3, f"{name} step {t}: ESS margin {margin:.2e} (change the seed)"
        err["x"] = max(err["x"], np.max(np.abs(r["particles"] - parts[t])) / scale,
                       np.max(np.abs(r["mean"] - means[t])) / scale)
        err["w"] = max(err["w"], np.max(np.abs(r["weights"] - weights[t]) / weights[t]))
        err["cov"] = max(err["cov"], np.max(np.abs(r["cov"] - covs[t])))
        err["cond"] = max(err["cond"], np.max(np.abs(np.array(r["conds"]) - conds[t]) / np.array(conds[t])))
        X, w = parts[t], weights[t]  # continue from the reference's state
    print(f"{name}: flags {np.array(flags).astype(int)} ess/N {np.round(np.array(ess) / N, 3)} "
          f"restatement vs reference: x {err['x']:.2e} w(rel) {err['w']:.2e} cov {err['cov']:.2e} "
          f"cond(rel) {err['cond']:.2e}", flush=True)
    assert err["x"] < LR.TOL_X and err["w"] < LR.RTOL_W and err["cov"] < LR.TOL_COV and err["cond"] < LR.RTOL_COND
    if name in BOTH_KINDS:
        assert any(flags) and not all(flags), f"{name}: needs a resampling and a non-resampling step"

    steps = [T - 1] if name in LAST_ONLY else list(range(T))
    out.update(means=np.array(means), weights=np.array(weights), ess=np.array(ess), flags=np.array(flags),
               conds=np.array(conds), U=np.array(U), P=np.array([RS.sym_pack(P) for P in Ps]),
               covs_steps=np.array(steps), covs=np.array([RS.sym_pack(covs[t]) for t in steps]),
               particles_steps=np.array(steps), particles=np.array([parts[t] for t in steps]))
    if noise and name in NOISE_BY_SEED:
        out["noise_seed"] = np.array(run_seed + 1000)
    elif noise:
        out["V"] = np.array(Vlog)
    return out


def main():
    store = {}
    for name in LR.CASES:
        for k, v in run_case(name).items():
            store[f"{name}__{k}"] = v
    np.savez_compressed(LR.GOLDEN, **store)
    size = os.path.getsize(LR.GOLDEN)
    print(f"wrote {LR.GOLDEN}: {size} bytes")
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()
