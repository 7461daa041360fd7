"""Measure the soft (Gumbel-Softmax) resampler: N = 100, 1000, 4096, 10000 at d = 2 and 40, B = 1,
and B = 64 at N = 100.

    python tools/bench_soft.py [--reps 7] [--no-numpy] [--backward] [--out FILE.json]

HIP events on the handle's stream around ``pf_soft_resample`` (upload, the all-pairs pass over every
component chunk and split, the merge, download) after a warm-up call, median of --reps; once
without and once with the row entropies (a second all-pairs pass).  Reports ms per call, pair
evaluations per second (B N^2 per call: one softmax entry applied to all d components) and
draw evaluations per second (B N^2 ceil(d / 16): the Gumbel draws and exponentials actually
computed, since every chunk of 16 components regenerates them).  Beside them the vectorised NumPy
restatement (tests/dpf_soft_restatement.py) on this machine's CPU, one problem timed once and
multiplied by B; above N = 4096 it is not timed (its temporaries are 800 MB each at N = 10000).
With --backward each row also times ``pf_soft_backward`` the same way (upload, r, the transposed
all-pairs pass, the merge, download), with the forward pass's saved results and without them (the call
then runs the forward launches first), beside the forward call of the same session, and reports the
ratio backward / forward.
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
from particle_filters_amd import dpf_soft as SO  # noqa: E402
from tests import dpf_soft_restatement as R  # noqa: E402

SIZES = [(100, 2, 1), (100, 40, 1), (100, 2, 64), (100, 40, 64), (1000, 2, 1), (1000, 40, 1), (4096, 2, 1),
         (4096, 40, 1), (10000, 2, 1), (10000, 40, 1)]
ALPHA, TEMP = 0.1, 0.2


def problem(N, d, B):
    cases = [R.make_case(N, d, seed=b) for b in range(B)]
    X = np.ascontiguousarray(np.stack([x for x, _ in cases]))
    lw = np.stack([w for _, w in cases])
    return X, lw, np.ascontiguousarray(SO._log_probs(SO._log_normalize(lw)[0], ALPHA))


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


def gpu_times(N, d, B, reps, ev, backward=False):
    lib = NV.load()
    X, lw, lp = problem(N, d, B)
    h = SO._Handle(N, d, B)
    out = np.empty_like(X)
    H = np.zeros((B, N))

    def call(entropy, epoch):
        NV.check(lib.pf_soft_resample(h.h, NV.dptr(X), NV.dptr(lp), TEMP, 1, epoch, 0, NV.dptr(out),
                                      NV.dptr(H) if entropy else None), "pf_soft_resample")

    stream = lib.pf_soft_stream(h.h)
    call(True, 0)  # warm-up: code objects, first touch of every buffer
    call(False, 0)
    plain = [ev.time_ms(stream, lambda: call(False, 1 + k)) for k in range(reps)]
    assert np.all(np.isfinite(out))
    ent = [ev.time_ms(stream, lambda: call(True, 1 + k)) for k in range(reps)]
    assert np.all(np.isfinite(H))
    bwd = {}
    if backward:
        g = np.random.default_rng([N, d, B, 99]).standard_normal(X.shape)
        gX, glp = np.empty_like(X), np.zeros((B, N))

        def back(epoch, saved):
            sv = (NV.dptr(out), NV.dptr(M), NV.dptr(L)) if saved else (None, None, None)
            NV.check(lib.pf_soft_backward(h.h, NV.dptr(X), NV.dptr(lp), TEMP, 1, epoch, 0, *sv, NV.dptr(g),
                                          NV.dptr(gX), NV.dptr(glp)), "pf_soft_backward")

        call(False, 1)
        M, L = h.row_stats()
        back(1, True)  # warm-up: code objects, the backward's buffers
        back(1, False)
        with_saved = [ev.time_ms(stream, lambda: back(1, True)) for k in range(reps)]
        without = [ev.time_ms(stream, lambda: back(1, False)) for k in range(reps)]
        assert np.all(np.isfinite(gX)) and np.all(np.isfinite(glp))
        bms = float(np.median(with_saved))
        bwd = dict(backward_ms=bms, backward_ms_min=min(with_saved), backward_ms_max=max(with_saved),
                   backward_recompute_ms=float(np.median(without)), backward_over_forward=bms / float(np.median(plain)))
    h.close()
    ms = float(np.median(plain))
    chunks = (d + 15) // 16
    return dict(bwd, N=N, d=d, B=B, call_ms=ms, call_ms_min=min(plain), call_ms_max=max(plain),
                call_with_entropy_ms=float(np.median(ent)), pair_evals_per_s=B * N * N / (ms * 1e-3),
                draw_evals_per_s=B * N * N * chunks / (ms * 1e-3), component_chunks=chunks)


def numpy_call_ms(N, d, B):
    X, lw, _ = problem(N, d, 1)
    t0 = time.perf_counter()
    R.soft_resample(X[0], lw[0], ALPHA, TEMP, 1, 1, 0)
    t = time.perf_counter() - t0
    return dict(numpy_restatement_call_ms=1e3 * t * B, numpy_problems_timed=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-numpy", action="store_true", help="skip the CPU restatement timings")
    ap.add_argument("--backward", action="store_true", help="time pf_soft_backward beside the forward call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert NV.device_count() > 0, "bench_soft needs a HIP device"
    ev = Events()
    rows = []
    for N, d, B in SIZES:
        r = gpu_times(N, d, B, a.reps, ev, a.backward)
        if not a.no_numpy and N <= 4096:
            r.update(numpy_call_ms(N, d, B))
        rows.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps({"bench": "soft_resample", "soft_alpha": ALPHA, "gumbel_temperature": TEMP, "rows": rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
