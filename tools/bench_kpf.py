"""Measure the kernel particle flow filter: diagonal kernel, nx = 40, Np = 200, 4096, 16384.

    python tools/bench_kpf.py [--reps 5] [--out FILE.json]

HIP events on the handle's stream around ``pf_kpf_analyze`` (upload, every pseudo-time step,
download) after a warm-up call; a call with zero steps measures the upload / download share, and
the time per pseudo-step is the difference over the number of steps.  Reports ms per step and
pair-dimension evaluations per second (Np^2 nx / step time), and beside them the time of one step
of the vectorised NumPy restatement (tests/kpf_restatement.py) on this machine's CPU at Np = 200
and 4096.  Prints one JSON line.  Needs an MI355X: no device, no number.
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
from particle_filters_amd import kernel_pf as KP  # noqa: E402
from particle_filters_amd import models as M  # noqa: E402
from tests import kpf_restatement as KR  # noqa: E402

NX, NZ = 40, 10


def problem(Np):
    rng = np.random.default_rng(Np)
    h = M.SelectObservation(np.arange(0, NX, 4), NX)
    X = rng.normal(size=(Np, NX)) + 1.0
    y = h(rng.normal(size=NX) + 1.0) + np.sqrt(0.5) * rng.normal(size=NZ)
    return h, 0.5 * np.eye(NZ), X, y


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


def gpu_times(Np, reps, ev):
    lib = NV.load()
    h, R, X, y = problem(Np)
    kf = KP.KernelParticleFilter(KP.Model(h, h.jacobian, R), KP.KPFConfig())
    x0, B, B_inv, ell = kf.prior(X)
    hist, _, steps = KP.pseudo_time_schedule(kf.cfg)
    ds = np.ascontiguousarray(hist, dtype=float)
    hd = kf._handle(Np)
    out = np.empty_like(X)
    clip = np.zeros(steps, dtype=np.int32)

    def call(n):
        NV.check(lib.pf_kpf_analyze(hd, NV.dptr(X), NV.dptr(y), NV.dptr(x0), NV.dptr(np.ascontiguousarray(B)),
                                    NV.dptr(np.ascontiguousarray(B_inv)), NV.dptr(ell), NV.dptr(ds), n, 2.0,
                                    NV.dptr(out), clip.ctypes.data_as(C.POINTER(C.c_int32))), "pf_kpf_analyze")

    stream = lib.pf_kpf_stream(hd)
    call(steps)  # warm-up: code objects, first-touch of every buffer
    call(0)
    full = [ev.time_ms(stream, lambda: call(steps)) for _ in range(reps)]
    empty = [ev.time_ms(stream, lambda: call(0)) for _ in range(reps)]
    assert np.all(np.isfinite(out))
    kf.close()
    step_ms = (float(np.median(full)) - float(np.median(empty))) / steps
    return dict(Np=Np, nx=NX, steps=steps, analyze_ms=float(np.median(full)), analyze_ms_min=min(full),
                analyze_ms_max=max(full), copies_only_ms=float(np.median(empty)), step_ms=step_ms,
                pair_dim_evals_per_s=Np * Np * NX / (step_ms * 1e-3))


def numpy_step_s(Np):
    h, R, X, y = problem(Np)
    cfg = KP.KPFConfig(max_steps=1, min_steps=1)
    t0 = time.perf_counter()
    KR.analyze(h, R, cfg, X, y)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert NV.device_count() > 0, "bench_kpf needs a HIP device"
    ev = Events()
    rows = [gpu_times(Np, a.reps, ev) for Np in (200, 4096, 16384)]
    for r in rows:
        if r["Np"] in (200, 4096):
            r["numpy_restatement_step_ms"] = 1e3 * numpy_step_s(r["Np"])
    line = json.dumps({"bench": "kpf_diagonal", "rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
