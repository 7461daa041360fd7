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

    python tools/bench_soft.py --torch {cpu,cuda} [--no-check-values] [--label NAME] [--out FILE]

times one training iteration of ``dpf_soft_torch``'s filter instead (``torch_training_ms``) at (N, d, B)
= (100, 2, 64) and (1000, 2, 1): the filter is made with ``device_path=True``, so CUDA tensors take the
device path and CPU tensors the host path.  --out
appends, so that arrangements alternated in one session end up in one file.
"""

import argparse
import ctypes as C
import inspect
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


# --torch: (N, d, B) of one training iteration of dpf_soft_torch's filter
TORCH_SHAPES = [(100, 2, 64), (1000, 2, 1)]
TORCH_STEPS = 10


def torch_training_ms(N, d, B, device, reps, check_values=True):
    """One training iteration of ``dpf_soft_torch.DifferentiableParticleFilter`` on tensors of ``device``
    ("cpu" or "cuda"): ``filter`` over T = 10 steps of the 2-D LGSSM of
    tests/dpf_rnn_grad_restatement.py, a scalar loss, ``backward()`` and the gradient to the parameter
    ``a`` the transition closes over, with ``torch.cuda.synchronize()`` at both ends; median, min and
    max of ``reps`` after a warm-up.  Works on a tree without the device path too."""
    import torch

    from particle_filters_amd import dpf_soft_torch as ST
    from tests import dpf_rnn_grad_restatement as G

    rng = np.random.default_rng([N, d, B, 7])
    obs = torch.tensor(rng.standard_normal((B, TORCH_STEPS, d)), device=device)
    noise = [torch.tensor(rng.standard_normal((B, N, d)), device=device) for _ in range(TORCH_STEPS)]
    a = torch.tensor(0.9, dtype=torch.float64, device=device, requires_grad=True)
    calls = {"k": 0}

    def transition_fn(x, params):  # G.lgssm with the noise on the tensors' device
        eps = noise[calls["k"] % len(noise)]
        calls["k"] += 1
        return a * x + 0.5 * eps

    _, log_likelihood_fn = G.lgssm([], a)
    kw = {} if check_values else {"check_values": False}
    if "device_path" in inspect.signature(ST.DifferentiableParticleFilter.__init__).parameters:
        kw["device_path"] = True  # a tree that has the device path: CUDA tensors take it
    flt = ST.DifferentiableParticleFilter(N, d, transition_fn, log_likelihood_fn, ALPHA, TEMP, seed=5,
                                          rng=np.random.default_rng(3), **kw)
    mean = torch.zeros(d, dtype=torch.float64, device=device)
    chol = torch.eye(d, dtype=torch.float64, device=device)

    def iteration():
        a.grad = None
        flt.epoch = 0
        ps, _ = flt.filter(obs, mean, chol)
        loss = ((ps[:, 1:].mean(dim=2) - obs) ** 2).sum()
        loss.backward()
        assert a.grad is not None

    times = []
    try:
        for k in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            iteration()
            torch.cuda.synchronize()
            if k:  # the first is the warm-up
                times.append(1e3 * (time.perf_counter() - t0))
    finally:
        flt.close()
    return {"N": N, "d": d, "B": B, "steps": TORCH_STEPS, "ms": float(np.median(times)), "min_ms": min(times),
            "max_ms": max(times)}


def main_torch(a):
    rows = []
    for N, d, B in TORCH_SHAPES:
        r = torch_training_ms(N, d, B, a.torch, a.reps, not a.no_check_values)
        rows.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps({"bench": "soft_torch_training", "tensors": a.torch, "check_values": not a.no_check_values,
                       "label": a.label, "rows": rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-numpy", action="store_true", help="skip the CPU restatement timings")
    ap.add_argument("--backward", action="store_true", help="time pf_soft_backward beside the forward call")
    ap.add_argument("--torch", choices=["cpu", "cuda"], default=None,
                    help="time one training iteration of dpf_soft_torch's filter on tensors of this device instead")
    ap.add_argument("--no-check-values", action="store_true", help="--torch: check_values=False")
    ap.add_argument("--label", default="", help="--torch: a name for the arrangement, copied to the result")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert NV.device_count() > 0, "bench_soft needs a HIP device"
    if a.torch:
        return main_torch(a)
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
