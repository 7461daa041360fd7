"""Measure the dense EDH path on the skewed-t sensor network: d = 144, 400 with N = 200, 10 000.

    python tools/bench_edh_dense.py [--reps 7] [--flow-map host|device] [--tracker host|device] [--wall]
                                    [--noise none|host|device[,...]] [--rounds 1]
                                    [--shapes 144x10000,400x10000] [--out FILE.json]

HIP events on the handle's stream around ``pf_edh_dense_run`` (uploads, T steps with no host
synchronisation inside, downloads) after a warm-up call, the median of ``--reps``; the device time
per step is the difference between a run of 10 steps and a run of 2 over the 8 steps between them.
That time includes each step's share of the run's transfers (M_t up, cov_t down: 2 d^2 doubles).
Reports, per (d, N): ms per step, its share of the fp64 matrix peak counted as the dense products
the step runs (2 N d^2 flops each: the map, |W(x_k - alpha x)|^2 and the covariance; the fourth,
|W(eta_0 - alpha x)|^2, is skipped without process noise and control, as here) against 78.6 TF,
the host time of composing one step's flow map
(``edh.compose_flow_map``, NumPy), and the time of the same step of the vectorised NumPy restatement
(tests/sn_edh_restatement.py) on this machine's CPU.  The wiring is the notebook's
(PF_PF_results_reproduction_sn_skew.ipynb: alpha = 0.9, m1 = 1, m2 = 1/3, 8 lambda steps, RK4, no
process noise, ratio 0.5), whose own table gives 31.7 s (d = 144) and 168.9 s (d = 400) for one
10-step run of the reference EDH with 10 000 particles.  ``--flow-map host`` (the default) times
``pf_edh_dense_run`` on maps composed beforehand and adds ``host_path_step_ms``, the step with its
host composition; ``--flow-map device`` times ``pf_edh_dense_flow_run``, which composes every step's
map inside the run (csrc/pf_edh_flowmap_kernels.h), so its ``step_ms`` is the whole step but for the
tracker.  ``--tracker device`` (with ``--flow-map device``) times ``pf_edh_dense_flow_run_tracked``, the
same run with the UKF tracker's predict and update chained in (csrc/pf_ukf_dense_kernels.h).

``--wall`` measures what a user of ``EDHFlowPF.run`` waits for instead: the wall clock around the whole
call, tracker included (``trackers.UKFTracker`` on the host, or ``trackers.DeviceUKFTracker``), from a
fresh tracker and state per repetition after one warm-up run; ``wall_step_ms`` is the median run over
its 10 steps.  ``--noise`` (with ``--wall``) adds the model's process noise N(0, Q) to every step: ``host`` is
the notebooks' way, ``rng.multivariate_normal(0, Q, (T, N))`` drawn up front (``host_draw_ms``, timed apart)
and uploaded by the run (``process_noise="host"``), ``device`` a ``noise.DeviceGaussianNoise``, drawn by
``k_dense_noise`` ahead of each step.  Several modes separated by commas are measured alternately, ``--rounds``
times over, in this one process, so that their difference can be read against the spread between rounds.
Prints one JSON line.  Needs an MI355X: no device, no number.
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from particle_filters_amd import _native as NV  # noqa: E402
from particle_filters_amd import edh as E  # noqa: E402
from particle_filters_amd import models as M  # noqa: E402
from particle_filters_amd import trackers as TR  # noqa: E402
from particle_filters_amd.noise import DeviceGaussianNoise  # noqa: E402
from tests import sn_edh_restatement as RS  # noqa: E402

PEAK_FP64_MATRIX = 78.6e12
ALPHA, M1, M2, L = 0.9, 1.0, 1.0 / 3.0, 8
T_LONG, T_SHORT = 10, 2
NOTEBOOK_S_PER_10_STEPS = {144: 31.735920, 400: 168.876814}  # reference EDH, N = 10 000


def sigma(d):
    """Squared-exponential covariance on the sqrt(d) x sqrt(d) lattice with a nugget (the notebook's
    alpha0 = 1, alpha1 = 1e-3, beta = 8)."""
    n = int(round(np.sqrt(d)))
    xs, ys = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    r = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(float)
    d2 = np.sum((r[:, None, :] - r[None, :, :]) ** 2, axis=-1)
    return np.exp(-d2 / 8.0) + 1e-3 * np.eye(d)


class Events:
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def time_ms(self, stream, fn):
        s = C.c_void_p(stream)
        assert self.hip.hipEventRecord(self.a, s) == 0
        fn()
        assert self.hip.hipEventRecord(self.b, s) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return float(ms.value)


def make_tracker(kind, g, h, Q, R):
    """The notebook's UKF (alpha = 1e-3, beta = 2, kappa = 0) from x0 = 0, P0 = Sigma."""
    ukf = TR.UnscentedKalmanFilter(g, h, Q, R, alpha=1e-3, beta=2.0, kappa=0.0)
    st = TR.UKFState(mean=np.zeros(Q.shape[0]), cov=Q.copy(), t=0)
    return TR.DeviceUKFTracker(ukf, st) if kind == "device" else TR.UKFTracker(ukf, st)


def measure_wall(d, N, reps, flow_map, tracker, noise="none"):
    """Wall clock of the whole EDHFlowPF.run call over T_LONG steps, tracker included; with noise="host" the
    draw of V [T][N][d] is timed apart from the run that uploads it."""
    rng = np.random.default_rng(d + N)
    Q = sigma(d)
    Lc = np.linalg.cholesky(Q)
    g, h = M.ScaleTransition(ALPHA, d), M.ExpObservation(M1, M2, d)
    R = np.eye(d) * M1
    X0 = np.ascontiguousarray(rng.standard_normal((N, d)) @ Lc.T)
    Z = rng.poisson(1.2, size=(T_LONG, d)).astype(float)
    U = rng.random(T_LONG)
    cfg = E.EDHConfig(n_particles=N, n_lambda_steps=L, resample_ess_ratio=0.5, flow_integrator="rk4")
    trk = make_tracker(tracker, g, h, Q, R)
    pf = E.EDHFlowPF(trk, g, h, h.jacobian, M.GaussianTransitionDensity(g, Q), M.PoissonLikelihood(h), R, cfg,
                     flow_map=flow_map)
    first = TR.UKFState(mean=np.zeros(d), cov=Q.copy(), t=0)
    noise_rng = np.random.default_rng(d * N)

    def run():
        trk.state = TR.UKFState(mean=first.mean.copy(), cov=first.cov.copy(), t=0)
        trk.past_mean = first.mean.copy()
        st = E.PFState(particles=X0.copy(), weights=np.full(N, 1.0 / N), mean=np.zeros(d), cov=Q.copy())
        draw = 0.0
        if noise == "host":
            t0 = time.perf_counter()
            V = noise_rng.multivariate_normal(np.zeros(d), Q, size=(T_LONG, N))
            draw = time.perf_counter() - t0
            kw = dict(process_noise="host", replay=(V, U))
        elif noise == "device":
            kw = dict(process_noise=DeviceGaussianNoise(d + N, 0), replay=(None, U))
        else:
            kw = dict(process_noise="none", replay=(None, U))
        t0 = time.perf_counter()
        res = pf.run(st, Z, **kw)
        dt = time.perf_counter() - t0
        assert np.all(np.isfinite(res.means))
        return 1e3 * dt, int(res.flags.sum()), 1e3 * draw

    run()  # warm-up: the handles, code objects, first touch of every buffer
    out = [run() for _ in range(reps)]
    ms = [o[0] for o in out]
    pf.close()
    if tracker == "device":
        trk.close()
    row = dict(d=d, N=N, flow_map=flow_map, tracker=tracker, noise=noise, steps=T_LONG,
               wall_run_ms=float(np.median(ms)), wall_run_ms_min=min(ms), wall_run_ms_max=max(ms),
               wall_step_ms=float(np.median(ms)) / T_LONG, resampled_steps=out[-1][1])
    if noise == "host":
        row["host_draw_ms"] = float(np.median([o[2] for o in out]))
        row["host_draw_step_ms"] = row["host_draw_ms"] / T_LONG
        row["wall_step_ms_with_draw"] = row["wall_step_ms"] + row["host_draw_step_ms"]
    return row


def measure(d, N, reps, ev, flow_map="host", tracker="host"):
    lib = NV.load()
    rng = np.random.default_rng(d + N)
    Q = sigma(d)
    Lc = np.linalg.cholesky(Q)
    h = M.ExpObservation(M1, M2, d)
    R = np.eye(d) * M1
    X0 = np.ascontiguousarray(rng.standard_normal((N, d)) @ Lc.T)
    w0 = np.full(N, 1.0 / N)
    Z = rng.poisson(1.2, size=(T_LONG, d)).astype(float)

    # host composition of one step's map
    P = ALPHA * ALPHA * Q + Q
    t0 = time.perf_counter()
    Mc, cc, _, _ = E.compose_flow_map(P, np.zeros(d), Z[0], h, h.jacobian, R, L, "rk4")
    compose_s = time.perf_counter() - t0
    Ms = np.ascontiguousarray(np.broadcast_to(Mc, (T_LONG, d, d)))
    cs = np.ascontiguousarray(np.broadcast_to(cc, (T_LONG, d)))
    U = rng.random(T_LONG)

    model = NV.EdhDenseModel(d, NV.PF_EDH_OBS_EXP, NV.PF_EDH_LIKE_POISSON, 0, ALPHA, M1, M2, None, NV.dptr(Q))
    opts = NV.EdhDenseOpts(N, 0.5, 0, 0)
    hd = C.c_void_p()
    NV.check(lib.pf_edh_dense_create(C.byref(model), C.byref(opts), C.byref(hd)), "pf_edh_dense_create")
    means, covs = np.empty((T_LONG, d)), np.empty((T_LONG, d, d))
    ess, flags = np.empty(T_LONG), np.zeros(T_LONG, dtype=np.uint8)

    Ps = np.ascontiguousarray(np.broadcast_to(P, (T_LONG, d, d)))
    E0 = np.zeros((T_LONG, d))
    rd = np.ascontiguousarray(np.diag(R))
    fl = flags.ctypes.data_as(C.POINTER(C.c_uint8))

    trk = make_tracker("device", M.ScaleTransition(ALPHA, d), h, Q, R) if tracker == "device" else None

    def call(T):
        NV.check(lib.pf_edh_dense_set_state(hd, NV.dptr(X0), NV.dptr(w0)), "set_state")
        NV.check(lib.pf_edh_dense_set_run_replay(hd, None, NV.dptr(U), T), "set_run_replay")
        if trk is not None:  # the tracker's predict and update inside the run, from x0 = 0, P0 = Sigma
            trk.state = TR.UKFState(mean=np.zeros(d), cov=Q.copy(), t=0)
            return lambda: NV.check(
                lib.pf_edh_dense_flow_run_tracked(hd, trk._handle(), NV.dptr(rd), NV.dptr(Z), None, T, L,
                                                  NV.PF_EDH_RK4, NV.PF_NOISE_NONE, NV.dptr(means), NV.dptr(covs),
                                                  NV.dptr(ess), fl, None), "flow_run_tracked")
        if flow_map == "device":
            return lambda: NV.check(
                lib.pf_edh_dense_flow_run(hd, NV.dptr(Ps), NV.dptr(E0), NV.dptr(rd), NV.dptr(Z), None, T, L,
                                          NV.PF_EDH_RK4, NV.PF_NOISE_NONE, NV.dptr(means), NV.dptr(covs), NV.dptr(ess),
                                          fl, None), "flow_run")
        return lambda: NV.check(
            lib.pf_edh_dense_run(hd, NV.dptr(Ms), NV.dptr(cs), NV.dptr(Z), None, T, NV.PF_NOISE_NONE, NV.dptr(means),
                                 NV.dptr(covs), NV.dptr(ess), fl), "run")

    stream = lib.pf_edh_dense_stream(hd)
    call(T_LONG)()  # warm-up: code objects, first touch of every buffer
    call(T_SHORT)()
    long_ms = [ev.time_ms(stream, call(T_LONG)) for _ in range(reps)]
    short_ms = [ev.time_ms(stream, call(T_SHORT)) for _ in range(reps)]
    assert np.all(np.isfinite(means))
    lib.pf_edh_dense_destroy(hd)
    if trk is not None:
        trk.close()
    step_ms = (float(np.median(long_ms)) - float(np.median(short_ms))) / (T_LONG - T_SHORT)

    # the same step in NumPy
    mdl = dict(alpha=ALPHA, obs="exp", m1=M1, m2=M2, like="poisson", rdiag=None, Q=Q)
    t0 = time.perf_counter()
    RS.dense_step(X0, w0, Mc, cc, Z[0], mdl, U=float(U[0]))
    numpy_s = time.perf_counter() - t0
    products = 3  # no process noise, no control: enqueue_step skips G_QV
    flops = products * 2.0 * N * d * d
    row = dict(d=d, N=N, flow_map=flow_map, tracker="device" if trk is not None else "none",
               run10_ms=float(np.median(long_ms)), run10_ms_min=min(long_ms), run10_ms_max=max(long_ms), run2_ms=float(np.median(short_ms)), step_ms=step_ms,
               dense_products_per_step=products, product_flops_per_step=flops,
               share_of_fp64_matrix_peak=flops / (step_ms * 1e-3) / PEAK_FP64_MATRIX,
               host_compose_ms_per_step=1e3 * compose_s, numpy_restatement_step_ms=1e3 * numpy_s,
               resampled_steps=int(flags.sum()))
    if flow_map == "host":
        row["host_path_step_ms"] = step_ms + 1e3 * compose_s  # the step as EDHFlowPF.run pays for it
    if N == 10000 and d in NOTEBOOK_S_PER_10_STEPS:
        row["reference_notebook_s_per_10_steps"] = NOTEBOOK_S_PER_10_STEPS[d]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--flow-map", choices=("host", "device"), default="host")
    ap.add_argument("--tracker", choices=("host", "device"), default="host",
                    help="device: the UKF tracker runs inside the run (needs --flow-map device for the event timing)")
    ap.add_argument("--wall", action="store_true", help="wall clock of the whole EDHFlowPF.run call, tracker included")
    ap.add_argument("--noise", default="none", help="with --wall: none, host or device process noise; several "
                    "separated by commas are measured alternately")
    ap.add_argument("--rounds", type=int, default=1, help="with --wall: repeat the whole alternation this often")
    ap.add_argument("--shapes", default="144x200,144x10000,400x200,400x10000", help="comma-separated dxN")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    modes = a.noise.split(",")
    if any(m not in ("none", "host", "device") for m in modes):
        ap.error("--noise takes none, host or device")
    if not a.wall and modes != ["none"]:
        ap.error("--noise is measured with --wall")
    assert NV.device_count() > 0, "bench_edh_dense needs a HIP device"
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    if a.wall:
        rows = []
        for rnd in range(a.rounds):
            for d, N in shapes:
                for m in modes:
                    rows.append(dict(measure_wall(d, N, a.reps, a.flow_map, a.tracker, m), round=rnd))
    else:
        if a.tracker == "device" and a.flow_map != "device":
            ap.error("--tracker device is timed by events only with --flow-map device (or use --wall)")
        ev = Events()
        rows = [measure(d, N, a.reps, ev, a.flow_map, a.tracker) for d, N in shapes]
    line = json.dumps({"bench": "edh_dense_skewt", "rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
