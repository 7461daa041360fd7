"""Measure the stochastic particle flow filter: N = 2000, 1e4, 1e6 at n = 4, 9, 40, 300 steps.

    python tools/bench_spf.py [--reps 7] [--out FILE.json]

HIP events on the handle's stream around ``pf_spf_advance`` (repacking and upload of the 300
parameter blocks, then the one launch with device draws) after a warm-up call; a second series
around a one-step call gives the fixed share, and the time per step is the difference over 299.
Reports particle-steps per second from that, the wall-clock ms of the whole
``run_generalized_spf`` call given the schedule (fold, create, prior, advance, download), and
beside them the vectorised folded NumPy restatement (tests/spf_restatement.py, NumPy's own
draws) timed on this machine's CPU on 3 to 30 steps and scaled to 300.  Prints one JSON line.
Needs an MI355X: no device, no number.
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
from particle_filters_amd import stochastic_pf as SP  # noqa: E402
from tests import spf_restatement as SR  # noqa: E402

STEPS = 300


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


def problem(n):
    model = SR.random_model(500 + n, n, (n + 1) // 2)
    lam = np.linspace(0.0, 1.0, STEPS + 1)
    sched = (lam, lam.copy(), np.ones_like(lam))
    return model, sched, SP.fold_steps(model, *sched, "inv_M", 1e-2)


def gpu_times(N, n, reps, ev):
    model, sched, params = problem(n)
    L0 = np.linalg.cholesky(model.P0)
    with SP.SpfEngine(N, n) as eng:
        def call(steps):
            eng.draw_prior(model.m0, L0, 1)
            return ev.time_ms(eng.stream, lambda: eng.advance(params[:steps], 0, 1))

        call(STEPS)  # warm-up: code object, first touch of every buffer
        call(1)
        full = [call(STEPS) for _ in range(reps)]
        one = [call(1) for _ in range(reps)]
        assert np.all(np.isfinite(eng.particles()))
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        X, _, _ = SP.run_generalized_spf(model, N=N, n_steps=STEPS, beta_mode="linear", seed=1, schedule=sched)
        wall.append(1e3 * (time.perf_counter() - t0))
    step_ms = (float(np.median(full)) - float(np.median(one))) / (STEPS - 1)
    return dict(N=N, n=n, steps=STEPS, advance_ms=float(np.median(full)), advance_ms_min=min(full),
                advance_ms_max=max(full), one_step_call_ms=float(np.median(one)), step_ms=step_ms,
                particle_steps_per_s=N / (step_ms * 1e-3), whole_call_ms=float(np.median(wall)))


def numpy_ms(N, n):
    """The folded restatement with NumPy draws, ms for 300 steps (3 to 30 timed, scaled)."""
    model, _, params = problem(n)
    steps = int(max(3, min(30, 3e7 // (N * n))))
    draw = SR.numpy_draws(1, N, n)
    X0 = SR.prior(model, draw)
    t0 = time.perf_counter()
    SR.folded(params[:steps], X0, draw, n)
    return 1e3 * (time.perf_counter() - t0) * STEPS / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert NV.device_count() > 0, "bench_spf needs a HIP device"
    ev = Events()
    rows = []
    for n in (4, 9, 40):
        for N in (2000, 10_000, 1_000_000):
            r = gpu_times(N, n, a.reps, ev)
            r["numpy_restatement_ms"] = numpy_ms(N, n)
            rows.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps({"bench": "spf", "rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
