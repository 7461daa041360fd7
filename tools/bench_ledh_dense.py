"""Measure the dense LEDH path on the skewed-t sensor network: (d, N, L) = (144, 200, 8), (400, 200, 8)
and (144, 10 000, 8).

    python tools/bench_ledh_dense.py [--reps 7] [--out FILE.json]

HIP events on the handle's stream around ``pf_ledh_dense_run`` (uploads, T steps with no host
synchronisation inside, downloads) after a warm-up call, the median of ``--reps``; the device time
per step is the difference between a run of 10 steps and a run of 2 over the 8 steps between them.
That time includes each step's share of the run's transfers (P_t up, cov_t down: 2 d^2 doubles).
Reports, per (d, N, L): ms per step; the share of the fp64 matrix peak (78.6 TF) that the count
N L 2 d^3 / 3 represents (the two Cholesky factorisations per particle and lambda step, the part
that runs on the matrix cores); the time of the same step of the vectorised NumPy restatement
(tests/sn_ledh_restatement.py) on this machine's CPU, measured on at most 50 particles and scaled
to N (the restatement is linear in N and its batch of 50 d x d factors is what fits comfortably);
and the reference notebook's published time per step (PF_PF_results_reproduction_sn_skew.ipynb,
LEDH with 200 particles: 13.2 s and 96.1 s per 10-step run).  The wiring is the notebook's
(alpha = 0.9, m1 = 1, m2 = 1/3, R = I, 8 lambda steps, no process noise, ratio 0.5).  Prints one
JSON line.  Needs an MI355X: no device, no number.
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
from tests import sn_ledh_restatement as LR  # noqa: E402
from tools.bench_edh_dense import ALPHA, M1, M2, PEAK_FP64_MATRIX, T_LONG, T_SHORT, Events, sigma  # noqa: E402

NOTEBOOK_S_PER_STEP = {144: 1.32, 400: 9.61}  # reference LEDH, N = 200
NUMPY_PARTICLES = 50


def measure(d, N, L, reps, ev):
    lib = NV.load()
    rng = np.random.default_rng(d + N)
    Q = sigma(d)
    Lc = np.linalg.cholesky(Q)
    rdiag = np.ones(d)  # the notebook's flow R = I
    X0 = np.ascontiguousarray(rng.standard_normal((N, d)) @ Lc.T)
    w0 = np.full(N, 1.0 / N)
    Z = rng.poisson(1.2, size=(T_LONG, d)).astype(float)
    P = ALPHA * ALPHA * Q + Q
    Ps = np.ascontiguousarray(np.broadcast_to(P, (T_LONG, d, d)))
    U = rng.random(T_LONG)

    model = NV.EdhDenseModel(d, NV.PF_EDH_OBS_EXP, NV.PF_EDH_LIKE_POISSON, 0, ALPHA, M1, M2, None, NV.dptr(Q))
    opts = NV.EdhDenseOpts(N, 0.5, 0, 0)
    hd = C.c_void_p()
    NV.check(lib.pf_edh_dense_create(C.byref(model), C.byref(opts), C.byref(hd)), "pf_edh_dense_create")
    means, covs = np.empty((T_LONG, d)), np.empty((T_LONG, d, d))
    ess, flags = np.empty(T_LONG), np.zeros(T_LONG, dtype=np.uint8)

    def call(T):
        NV.check(lib.pf_edh_dense_set_state(hd, NV.dptr(X0), NV.dptr(w0)), "set_state")
        NV.check(lib.pf_edh_dense_set_run_replay(hd, None, NV.dptr(U), T), "set_run_replay")
        return lambda: NV.check(
            lib.pf_ledh_dense_run(hd, NV.dptr(Ps), NV.dptr(rdiag), NV.dptr(Z), None, T, L, NV.PF_NOISE_NONE,
                                  NV.dptr(means), NV.dptr(covs), NV.dptr(ess),
                                  flags.ctypes.data_as(C.POINTER(C.c_uint8))), "run")

    stream = lib.pf_edh_dense_stream(hd)
    call(T_LONG)()  # warm-up: code objects, first touch of every buffer
    call(T_SHORT)()
    long_ms = [ev.time_ms(stream, call(T_LONG)) for _ in range(reps)]
    short_ms = [ev.time_ms(stream, call(T_SHORT)) for _ in range(reps)]
    assert np.all(np.isfinite(means))
    lib.pf_edh_dense_destroy(hd)
    step_ms = (float(np.median(long_ms)) - float(np.median(short_ms))) / (T_LONG - T_SHORT)

    # the same step in NumPy, on a subset of the particles
    n_np = min(N, NUMPY_PARTICLES)
    mdl = dict(alpha=ALPHA, obs="exp", m1=M1, m2=M2, like="poisson", rdiag=None, Q=Q)
    t0 = time.perf_counter()
    LR.ledh_step(X0[:n_np], np.full(n_np, 1.0 / n_np), P, Z[0], mdl, rdiag, L, U=float(U[0]))
    numpy_s = (time.perf_counter() - t0) * N / n_np
    flops = N * L * 2.0 * d ** 3 / 3.0
    row = dict(d=d, N=N, L=L, run10_ms=float(np.median(long_ms)), run10_ms_min=min(long_ms), run10_ms_max=max(long_ms),
               run2_ms=float(np.median(short_ms)), step_ms=step_ms, cholesky_flops_per_step=flops,
               share_of_fp64_matrix_peak=flops / (step_ms * 1e-3) / PEAK_FP64_MATRIX,
               numpy_restatement_step_ms=1e3 * numpy_s, numpy_restatement_particles_timed=n_np,
               resampled_steps=int(flags.sum()))
    if N == 200:
        row["reference_notebook_s_per_step"] = NOTEBOOK_S_PER_STEP[d]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert NV.device_count() > 0, "bench_ledh_dense needs a HIP device"
    ev = Events()
    rows = [measure(d, N, L, a.reps, ev) for d, N, L in ((144, 200, 8), (400, 200, 8), (144, 10000, 8))]
    line = json.dumps({"bench": "ledh_dense_skewt", "rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
