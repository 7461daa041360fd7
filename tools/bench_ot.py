"""Measure the Sinkhorn OT resampler: (N, d, B) = (100, 1, 1), (100, 1, 64), (1000, 3, 1),
(4096, 16, 1), (10000, 3, 1) and, with --large, (10000, 40, 1).

    python tools/bench_ot.py [--reps 7] [--large] [--no-numpy] [--backward] [--out FILE.json]

HIP events on the handle's stream around ``pf_ot_resample`` (upload, prepare, cost, n_iters = 50
iterations, projection, download) after a warm-up call, median of --reps; ``tol = 0`` so that every
iteration runs.  A call with ``n_iters = 0`` measures everything but the iterations, and the time
per half-iteration is the difference over 2 n_iters.  Reports ms per call, microseconds per
half-iteration, pair evaluations per second (B N^2 per half-iteration) and the bytes of C one pass
reads (B N^2 8) per second.  Beside them the vectorised NumPy restatement
(tests/dpf_ot_restatement.py) on this machine's CPU, one problem timed once and multiplied by B;
at N = 4096 it is timed on 2 iterations and scaled to 50 (``numpy_scaled`` says so), and above
that not at all (its temporaries are 800 MB each at N = 10000).  Prints one JSON line.

``--backward`` measures ``pf_ot_backward`` instead, at (N, B) = (100, 1), (100, 64), (1000, 1),
(4096, 1), (10000, 1) with d = 2 and d = 40: in every repetition one forward call, one backward call
with the saved dual history and one without (which replays the iterations first), alternating, on
one handle; medians, the two backward calls as multiples of the forward, and the bytes the handle
adds for the gradient with respect to the cost matrix (B N Npad 8).  ``PF_LIB`` names another
library for the forward-only run that compares two builds.

``--dev`` measures the device-pointer entries on device buffers (torch CUDA tensors), HIP events on
torch's current stream, at (N, d, B) = (50, 1, 1), (100, 1, 1), (100, 1, 64), (128, 40, 64) and, for the
launch sequence alone, (1000, 3, 1): ``pf_ot_resample_dev`` with the dual history recorded, by the
launch sequence and by the one-launch solver (``PF_OT_RESIDENT``), and ``pf_ot_backward_dev`` on the
recorded history; beside them what the host path of the torch binding runs for the same work, a
``pf_ot_resample`` and a ``pf_ot_replay``, and a ``pf_ot_backward`` with the saved history, timed by the
wall clock (they synchronise).  Under ``PF_LIB`` naming a library without the device entries only the
host figures are taken: the same-session comparison with an older build.

``--torch`` times one training iteration of ``dpf_ot_torch.DPF_OT`` on CUDA tensors at N = 100:
``run_filter`` over 10 steps, the loss, ``backward()``, with the host path, the device path, and the
device path with the one-launch solver (the last two only when the library has the entries); wall
clock around a synchronised iteration, median of --reps.
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
from particle_filters_amd import dpf_ot as OT  # noqa: E402
from tests import dpf_ot_restatement as R  # noqa: E402

SIZES = [(100, 1, 1), (100, 1, 64), (1000, 3, 1), (4096, 16, 1), (10000, 3, 1)]
LARGE = [(10000, 40, 1)]
N_ITERS = 50
EPS = 0.5


def problem(N, d, B):
    cases = [R.make_case(N, d, seed=b) for b in range(B)]
    return (np.ascontiguousarray(np.stack([x for x, _ in cases])),
            np.ascontiguousarray(np.stack([w for _, w in cases])))


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


def gpu_times(N, d, B, reps, ev):
    lib = NV.load()
    X, w = problem(N, d, B)
    h = OT._Handle(N, d, B)
    out = np.empty_like(X)
    its = np.zeros(B, dtype=np.int32)

    def call(n):
        NV.check(lib.pf_ot_resample(h.h, NV.dptr(X), NV.dptr(w), EPS, n, 1e-12, 0.0, NV.dptr(out),
                                    its.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None),
                 "pf_ot_resample")

    stream = lib.pf_ot_stream(h.h)
    call(N_ITERS)  # warm-up: code objects, first touch of every buffer
    call(0)
    full = [ev.time_ms(stream, lambda: call(N_ITERS)) for _ in range(reps)]
    assert np.all(its == N_ITERS) and np.all(np.isfinite(out))
    empty = [ev.time_ms(stream, lambda: call(0)) for _ in range(reps)]
    h.close()
    half_us = 1e3 * (float(np.median(full)) - float(np.median(empty))) / (2 * N_ITERS)
    return dict(N=N, d=d, B=B, n_iters=N_ITERS, call_ms=float(np.median(full)), call_ms_min=min(full),
                call_ms_max=max(full), no_iterations_ms=float(np.median(empty)), half_iteration_us=half_us,
                pair_evals_per_s=B * N * N / (half_us * 1e-6), cost_bytes_per_s=8.0 * B * N * N / (half_us * 1e-6))


BACKWARD_SIZES = [(100, d, 1) for d in (2, 40)] + [(100, d, 64) for d in (2, 40)] + \
    [(N, d, 1) for N in (1000, 4096, 10000) for d in (2, 40)]


def backward_times(N, d, B, reps, ev):
    lib = NV.load()
    X, w = problem(N, d, B)
    g = np.random.default_rng([N, d, B]).standard_normal((B, N, d))
    h = OT._Handle(N, d, B)
    out = np.empty_like(X)
    its = np.zeros(B, dtype=np.int32)

    def fwd():
        NV.check(lib.pf_ot_resample(h.h, NV.dptr(X), NV.dptr(w), EPS, N_ITERS, 1e-12, 0.0, NV.dptr(out),
                                    its.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None),
                 "pf_ot_resample")

    stream = lib.pf_ot_stream(h.h)
    fwd()  # warm-up: code objects, first touch of every buffer
    saved = h.replay(X, w, EPS, 1e-12, its)
    gX, _ = h.backward(X, w, g, EPS, 1e-12, its, saved.hist, saved.hist_argmax)
    h.backward(X, w, g, EPS, 1e-12, its)
    assert np.all(its == N_ITERS) and np.all(np.isfinite(gX))
    t = {"forward": [], "backward_saved": [], "backward": []}
    for _ in range(reps):
        t["forward"].append(ev.time_ms(stream, fwd))
        t["backward_saved"].append(ev.time_ms(
            stream, lambda: h.backward(X, w, g, EPS, 1e-12, its, saved.hist, saved.hist_argmax)))
        t["backward"].append(ev.time_ms(stream, lambda: h.backward(X, w, g, EPS, 1e-12, its)))
    h.close()
    med = {k: float(np.median(v)) for k, v in t.items()}
    r = dict(N=N, d=d, B=B, n_iters=N_ITERS, cost_gradient_bytes=8 * B * N * ((N + 63) // 64 * 64))
    for k, v in t.items():
        r.update({f"{k}_ms": med[k], f"{k}_ms_min": min(v), f"{k}_ms_max": max(v)})
    r["backward_saved_over_forward"] = med["backward_saved"] / med["forward"]
    r["backward_over_forward"] = med["backward"] / med["forward"]
    return r


DEV_SIZES = [(50, 1, 1), (100, 1, 1), (100, 1, 64), (128, 40, 64), (1000, 3, 1)]


def _spread(name, v):
    return {f"{name}_ms": float(np.median(v)), f"{name}_ms_min": min(v), f"{name}_ms_max": max(v)}


def dev_times(N, d, B, reps, ev):
    import torch

    lib = NV.load()
    X, w = problem(N, d, B)
    g = np.random.default_rng([N, d, B]).standard_normal((B, N, d))
    h = OT._Handle(N, d, B)
    r = dict(N=N, d=d, B=B, n_iters=N_ITERS)

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    # the host path of the torch binding: forward = resample + replay, backward with the saved history
    its = h.resample(X, w, EPS, N_ITERS, 1e-12, 0.0, False)[1]
    saved = h.replay(X, w, EPS, 1e-12, its)
    h.backward(X, w, g, EPS, 1e-12, its, saved.hist, saved.hist_argmax)

    def host_forward():
        k = h.resample(X, w, EPS, N_ITERS, 1e-12, 0.0, False)[1]
        h.replay(X, w, EPS, 1e-12, k)

    t = {"host_forward": [], "host_backward": []}
    for _ in range(reps):
        t["host_forward"].append(wall(host_forward))
        t["host_backward"].append(wall(lambda: h.backward(X, w, g, EPS, 1e-12, its, saved.hist, saved.hist_argmax)))
    for k, v in t.items():
        r.update(_spread(k, v))
    if hasattr(lib, "pf_ot_resample_dev"):
        side = torch.cuda.Stream()  # a caller's stream: the null stream would mean the handle's own
        stream = side.cuda_stream
        Xd, wd, gd = (torch.tensor(a, device="cuda") for a in (X, w, g))
        out, gX, gw = torch.empty_like(Xd), torch.empty_like(Xd), torch.empty_like(wd)
        k = torch.empty(B, dtype=torch.int32, device="cuda")
        hv = torch.empty((B, 4, N_ITERS + 1, N), dtype=torch.float64, device="cuda")
        am = torch.empty((B, N_ITERS, N), dtype=torch.int32, device="cuda")

        def fwd(flags):
            h.resample_dev(stream, Xd.data_ptr(), wd.data_ptr(), EPS, N_ITERS, 1e-12, 0.0, out.data_ptr(), k.data_ptr(),
                           hist=hv.data_ptr(), hist_argmax=am.data_ptr(), flags=flags)

        def bwd():
            h.backward_dev(stream, Xd.data_ptr(), wd.data_ptr(), EPS, 1e-12, k.data_ptr(), N_ITERS, N_ITERS,
                           hv.data_ptr(), am.data_ptr(), gd.data_ptr(), gX.data_ptr(), gw.data_ptr())

        modes = {"dev_forward": lambda: fwd(0), "dev_backward": bwd}
        if h.resident_supported():
            modes["resident_forward"] = lambda: fwd(NV.PF_OT_RESIDENT)
        torch.cuda.synchronize()
        for fn in modes.values():  # warm-up: code objects, the backward workspace
            fn()
        torch.cuda.synchronize()
        t = {m: [] for m in modes}
        for _ in range(reps):
            for m, fn in modes.items():
                t[m].append(ev.time_ms(stream, fn))
        assert bool((k == N_ITERS).all()) and bool(torch.isfinite(gX).all())
        for m, v in t.items():
            r.update(_spread(m, v))
    h.close()
    return r


def torch_times(reps):
    import torch

    from particle_filters_amd import dpf_ot_torch as TT
    from tests import dpf_ot_grad_restatement as GR

    N, d, T = 100, 2, 10
    rng = np.random.default_rng([N, d, T])
    cuda = dict(dtype=torch.float64, device="cuda")
    eps_t = torch.tensor(rng.standard_normal((T, N, d)), **cuda)
    obs = torch.tensor(rng.standard_normal((T, d)), **cuda)
    targets = torch.tensor(0.5 * rng.standard_normal((T, d)), **cuda)
    modes = {"host": dict()}
    if hasattr(NV.load(), "pf_ot_resample_dev"):
        modes["device"] = dict(device_path=True)
        modes["device_unchecked"] = dict(device_path=True, check_values=False)
        modes["device_resident"] = dict(device_path=True, solver="resident")
        modes["device_resident_unchecked"] = dict(device_path=True, solver="resident", check_values=False)
    r = dict(N=N, d=d, steps=T, n_iters=N_ITERS, epsilon=0.1)
    flts, params = {}, {}
    for m, kw in modes.items():
        a = torch.tensor(0.9, requires_grad=True, **cuda)
        sigma = torch.tensor(0.3, requires_grad=True, **cuda)
        mean = torch.zeros(d, requires_grad=True, **cuda)
        tf_, lf_ = GR.model(a, sigma, eps_t, 0.5)
        flts[m] = TT.DPF_OT(N, d, tf_, lf_, 0.1, N_ITERS, rng=np.random.default_rng(41), **kw)
        params[m] = (a, sigma, mean)

    def iteration(m):
        a, sigma, mean = params[m]
        for p in (a, sigma, mean):
            p.grad = None
        flts[m].rng = np.random.default_rng(41)
        ps, ws = flts[m].run_filter(obs, mean, torch.eye(d, **cuda))
        GR.loss_of(ps, ws, targets).backward()
        torch.cuda.synchronize()

    t = {m: [] for m in modes}
    for m in modes:
        iteration(m)  # warm-up
    for _ in range(reps):
        for m in modes:  # alternating
            t0 = time.perf_counter()
            iteration(m)
            t[m].append(1e3 * (time.perf_counter() - t0))
    for m, v in t.items():
        r.update(_spread(m, v))
        flts[m].close()
    return r


def numpy_call_ms(N, d, B):
    X, w = problem(N, d, 1)
    iters = N_ITERS if N < 4096 else 2
    t0 = time.perf_counter()
    R.sinkhorn_resample(X[0], w[0], EPS, iters, tol=0.0)
    t = time.perf_counter() - t0
    return dict(numpy_restatement_call_ms=1e3 * t * B * (N_ITERS / iters), numpy_scaled=iters != N_ITERS,
                numpy_timed_iterations=iters, numpy_problems_timed=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--large", action="store_true", help="also (10000, 40, 1)")
    ap.add_argument("--no-numpy", action="store_true", help="skip the CPU restatement timings")
    ap.add_argument("--backward", action="store_true", help="pf_ot_backward against the forward call")
    ap.add_argument("--dev", action="store_true", help="the device-pointer entries, both solvers, and the host path")
    ap.add_argument("--torch", action="store_true", help="one training iteration of dpf_ot_torch.DPF_OT per path")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert NV.device_count() > 0, "bench_ot needs a HIP device"
    ev = Events()
    rows = []
    if a.dev or a.torch:
        if a.dev:
            for N, d, B in DEV_SIZES:
                rows.append(dev_times(N, d, B, a.reps, ev))
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        else:
            rows.append(torch_times(a.reps))
        line = json.dumps({"bench": "ot_dev" if a.dev else "ot_torch", "epsilon": EPS, "library": NV.LIB_PATH,
                           "rows": rows})
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if a.backward:
        for N, d, B in BACKWARD_SIZES:
            rows.append(backward_times(N, d, B, a.reps, ev))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        line = json.dumps({"bench": "ot_backward", "epsilon": EPS, "rows": rows})
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    for N, d, B in SIZES + (LARGE if a.large else []):
        r = gpu_times(N, d, B, a.reps, ev)
        if not a.no_numpy and N <= 4096:
            r.update(numpy_call_ms(N, d, B))
        rows.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps({"bench": "ot_resample", "epsilon": EPS, "rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
