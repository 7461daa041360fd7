#!/usr/bin/env python
"""Generate tests/golden/sn_edh_runs.npz by running the REFERENCE EDH filter on the sensor-network
models (PF_PF_results_reproduction_sn_skew.ipynb / _snlg.ipynb).

Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_skewt.py

Imports /root/reference's ``models.EDH_particle_filter.EDHFlowPF`` with its own
``UnscentedKalmanFilter`` / ``UKFTracker`` and drives them with this package's model objects
(particle_filters_amd.models: the reference's call signatures) on data of the reference's
simulators.  Only numbers are stored: the inputs (Sigma, Z, parameters, initial particles or their
seed), the random stream consumed (process noise or its seed, the resampling uniforms) and the
per-step outputs (the large case skewt144: particles at the last step only).  To keep the file below
1 MB, symmetric matrices are stored as upper triangles, the two large cases store their initial
particles by seed, and snlg64 stores its process noise by seed (standard_normal @ chol(Sigma)^T).

Every stored step satisfies |ESS - ratio N| / N >= 1e-3, so no resample decision hinges on rounding.
The reference does not return its ESS: the stored ``ess`` is the restatement's, of the weights before
resampling, on the reference's own inputs of that step.
The vectorised restatement (tests/sn_edh_restatement.py) is checked against the reference here.
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
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

from models.EDH_particle_filter import EDHFlowPF, EDHConfig, UKFTracker, PFState  # noqa: E402  (reference)
from models.unscented_kalman_filter import UnscentedKalmanFilter, UKFState  # noqa: E402  (reference)
from simulator import simulator_sensor_network_skewt_dynamic as SK  # noqa: E402  (reference)
from simulator import simulator_sensor_network_linear_gaussian as LG  # noqa: E402  (reference)

import sn_edh_restatement as RS  # noqa: E402

# seeds of (data, initial particles, filter rng / noise)
SEEDS = {"skewt16_rk4": (42, 1, 11), "skewt16_euler_noise": (43, 2, 12), "skewt25_odd": (44, 3, 13),
         "skewt144": (42, 4, 14), "snlg64": (123, 5, 15)}
BIG = ("skewt144", "snlg64")  # initial particles by seed
NOISE_BY_SEED = ("snlg64",)


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
    d, N, L, T, integ, noise, wiring = RS.CASES[name]
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


def run_case(name):
    d, N, L, T, integ, noise, wiring = RS.CASES[name]
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
    ukf = UnscentedKalmanFilter(g, h, Sigma, R, alpha=1e-3, beta=2.0, kappa=0.0)
    tracker = UKFTracker(ukf, UKFState(mean=np.zeros(d), cov=Sigma.copy(), t=0))
    cfg = EDHConfig(n_particles=N, n_lambda_steps=L, resample_ess_ratio=RS.RATIO, flow_integrator=integ, rng=rec)
    pf = EDHFlowPF(tracker, g, h, h.jacobian, ltp, llp, R, cfg)
    st = PFState(particles=init.copy(), weights=np.full(N, 1.0 / N), mean=np.zeros(d), cov=Sigma.copy())
    model = RS.model_dict(wiring, d, alpha, m1, m2, sigma_z, Sigma)

    big = name in BIG
    out = {"Sigma": RS.sym_pack(Sigma), "Z": Z, "params": np.array(params), "init_seed": np.array(init_seed)}
    if not big:
        out["init_particles"] = init
    means, covs, weights, ess, flags, conds, U, Ps, pasts, parts = [], [], [], [], [], [], [], [], [], []
    err = dict(x=0.0, w=0.0, cov=0.0, cond=0.0)
    X, w = init.copy(), np.full(N, 1.0 / N)
    for t in range(T):
        n_u = len(rec.uniforms)
        st = pf.step(st, Z[t], process_noise_sampler=sampler)
        assert np.all(np.isfinite(st.weights)) and np.all(np.isfinite(st.particles)), (name, t)
        flag = len(rec.uniforms) > n_u
        U.append(rec.uniforms[-1] if flag else np.nan)
        means.append(st.mean); covs.append(st.cov); weights.append(st.weights); parts.append(st.particles)
        conds.append(st.diagnostics["condition_numbers"]); flags.append(flag)
    # second, identical tracker (it never sees the particles): P_t and the past means
    tr2 = UKFTracker(UnscentedKalmanFilter(g, h, Sigma, R, alpha=1e-3, beta=2.0, kappa=0.0),
                     UKFState(mean=np.zeros(d), cov=Sigma.copy(), t=0))
    for t in range(T):
        _, P = tr2.predict()
        Ps.append(np.array(P)); pasts.append(np.array(tr2.get_past_mean()))
        tr2.update(Z[t])
    # the restatement against the reference, step by step on the reference's own inputs
    scale = max(1.0, float(np.max(np.abs(np.array(parts)))))
    for t in range(T):
        P = 0.5 * (Ps[t] + Ps[t].T)
        Mc, cc, cd = RS.compose(P, alpha * pasts[t], Z[t], model, R, L, integ)
        v = Vlog[t] if noise else None
        r = RS.dense_step(X, w, Mc, cc, Z[t], model, v=v, U=U[t])
        ess.append(r["ess"])
        assert r["flag"] == flags[t], (name, t)
        margin = abs(r["ess"] - RS.RATIO * N) / N
        assert margin >= 1e-3, f"{name} step {t}: ESS margin {margin:.2e} (change the seed)"
        err["x"] = max(err["x"], np.max(np.abs(r["particles"] - parts[t])) / scale,
                       np.max(np.abs(r["mean"] - means[t])) / scale)
        err["w"] = max(err["w"], np.max(np.abs(r["weights"] - weights[t]) / weights[t]))
        err["cov"] = max(err["cov"], np.max(np.abs(r["cov"] - covs[t])))
        err["cond"] = max(err["cond"], np.max(np.abs(np.array(cd) - conds[t]) / np.array(conds[t])))
        X, w = parts[t], weights[t]  # continue from the reference's state
    print(f"{name}: flags {np.array(flags).astype(int)} ess/N {np.round(np.array(ess) / N, 3)} "
          f"restatement vs reference: x {err['x']:.2e} w(rel) {err['w']:.2e} cov {err['cov']:.2e} "
          f"cond(rel) {err['cond']:.2e}")
    assert err["x"] < RS.TOL_X and err["w"] < RS.RTOL_W and err["cov"] < RS.TOL_COV and err["cond"] < RS.RTOL_COND

    steps = list(range(T))  # posterior covariances
    psteps_P = list(range(T))
    out.update(means=np.array(means), weights=np.array(weights), ess=np.array(ess), flags=np.array(flags),
               conds=np.array(conds), U=np.array(U), past_means=np.array(pasts),
               P_steps=np.array(psteps_P), P=np.array([RS.sym_pack(0.5 * (Ps[t] + Ps[t].T)) for t in psteps_P]),
               P_asym=np.array([float(np.max(np.abs(Ps[t] - Ps[t].T))) for t in range(T)]),
               covs_steps=np.array(steps), covs=np.array([RS.sym_pack(covs[t]) for t in steps]))
    psteps = [T - 1] if name == "skewt144" else list(range(T))  # the large case: particles at the end only
    out.update(particles_steps=np.array(psteps), particles=np.array([parts[t] for t in psteps]))
    if noise and name in NOISE_BY_SEED:
        out["noise_seed"] = np.array(run_seed + 1000)
    elif noise:
        out["V"] = np.array(Vlog)
    return out


def main():
    store = {}
    for name in RS.CASES:
        for k, v in run_case(name).items():
            store[f"{name}__{k}"] = v
    np.savez_compressed(RS.GOLDEN, **store)
    size = os.path.getsize(RS.GOLDEN)
    print(f"wrote {RS.GOLDEN}: {size} bytes")
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()
