"""Measure the RNN resampler: N = 50 and 100 with H = 32, L = 1 at B = 1 and B = 64, N = 100 with
H = 64, N = 1000 with H = 32, LSTM and GRU, d = 1, and the resident against the streaming variant of
the recurrence at one shape.

    python tools/bench_rnn.py [--reps 7] [--no-numpy] [--backward] [--out FILE.json]

HIP events on the handle's stream around ``pf_rnn_resample`` (upload, the input projection, the
recurrence, the assignment, download of X' and of the B N N assignment matrices) after a warm-up
call, median of --reps.  Reports ms per resampling and that time divided by N, the latency of one
timestep of the recurrence with everything else charged to it.  Beside them the vectorised NumPy
restatement (tests/dpf_rnn_restatement.py) on this machine's CPU, one problem timed once and
multiplied by B.  With --backward each row also has the time of one ``pf_rnn_backward`` call (upload,
the recording forward launches, the backward chain, download of every gradient), measured the same
way on the same handle, its ratio to the forward call, and ``pf_rnn_backward_bytes``, the workspace
the first backward call allocates.  The streaming variant is forced through the test hook PF_TEST_RNN_STREAM, which is
read when the handle is made.  Prints one JSON line.  Needs an MI355X: no device, no number.

    python tools/bench_rnn.py --torch {cpu,cuda} [--no-check-values] [--label NAME] [--out FILE]

times one training iteration of ``dpf_rnn_torch``'s filter instead (``torch_training_ms``) at (N, H, B)
= (50, 32, 1) and (100, 32, 64), LSTM and GRU: CUDA tensors take the device path, CPU tensors the host
path.  --out appends, so that arrangements alternated in one session end up in one file.
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
from particle_filters_amd import dpf_rnn as RN  # noqa: E402
from tests import dpf_rnn_restatement as R  # noqa: E402

# (N, H, L, B, forced streaming)
SHAPES = [(50, 32, 1, 1, False), (50, 32, 1, 64, False), (100, 32, 1, 1, False), (100, 32, 1, 64, False),
          (100, 64, 1, 1, False), (1000, 32, 1, 1, False), (100, 32, 1, 64, True)]
D, TEMP = 1, 1.0


def problem(N, H, L, cell, B):
    rng = np.random.default_rng([N, H, L, B])
    X = np.ascontiguousarray(rng.standard_normal((B, N, D)))
    lw = R.log_normalize(1.5 * rng.standard_normal((B, N)))
    return X, lw, R.make_weights(rng, N, D, H, L, cell)


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


def gpu_times(N, H, L, cell, B, stream, reps, ev, backward=False):
    lib = NV.load()
    X, lw, W = problem(N, H, L, cell, B)
    w = np.ascontiguousarray(np.exp(lw))
    saved = {k: os.environ.get(k) for k in ("PF_TEST_HOOKS", "PF_TEST_RNN_STREAM")}
    if stream:
        os.environ.update(PF_TEST_HOOKS="1", PF_TEST_RNN_STREAM="1")
    try:
        h = RN._Handle(N, D, B, H, L, cell)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert h.resident == (not stream)
    h.set_weights(W)
    out, A = np.empty_like(X), np.empty((B, N, N))

    def call():
        NV.check(lib.pf_rnn_resample(h.h, NV.dptr(X), NV.dptr(w), TEMP, NV.dptr(out), NV.dptr(A), None),
                 "pf_rnn_resample")

    s = lib.pf_rnn_stream(h.h)
    call()  # warm-up: code objects, first touch of every buffer
    call()
    ms = [ev.time_ms(s, call) for _ in range(reps)]
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(A))
    extra = {}
    if backward:
        rng = np.random.default_rng([N, H, L, B, 1])
        gXo, gA = rng.standard_normal(X.shape), rng.standard_normal(A.shape)
        shapes = [a.shape for a in W]

        def back():
            return h.backward(X, w, TEMP, gXo, gA, shapes)

        back()  # warm-up: the workspace, the transposed fragments, code objects
        back()
        bms = [ev.time_ms(s, back) for _ in range(reps)]
        assert all(np.all(np.isfinite(g)) for g in back()[2])
        bmed = float(np.median(bms))
        extra = dict(backward_call_ms=bmed, backward_call_ms_min=min(bms), backward_call_ms_max=max(bms),
                     backward_over_forward=bmed / float(np.median(ms)), backward_bytes=h.backward_bytes)
    h.close()
    med = float(np.median(ms))
    return dict(extra, N=N, d=D, H=H, L=L, cell=cell, B=B, weights="streamed" if stream else "resident", call_ms=med,
                call_ms_min=min(ms), call_ms_max=max(ms), per_timestep_us=1e3 * med / N,
                cell_updates_per_s=B * N * N * L / (med * 1e-3))


def numpy_call_ms(N, H, L, cell, B):
    X, lw, W = problem(N, H, L, cell, 1)
    t0 = time.perf_counter()
    R.resample(X[0], lw[0], W, cell, TEMP)
    t = time.perf_counter() - t0
    return dict(numpy_restatement_call_ms=1e3 * t * B, numpy_problems_timed=1)


# --torch: (N, H, B) of one training iteration of dpf_rnn_torch's filter
TORCH_SHAPES = [(50, 32, 1), (100, 32, 64)]
TORCH_STEPS = 10


def torch_training_ms(N, H, B, cell, device, reps, check_values=True):
    """One training iteration of ``dpf_rnn_torch.DifferentiableParticleFilterRNN`` on tensors of
    ``device`` ("cpu" or "cuda"): ``filter`` over T = 10 steps of the 2-D LGSSM of
    tests/dpf_rnn_grad_restatement.py, a scalar loss on both results, ``backward()`` and an SGD step,
    with ``torch.cuda.synchronize()`` at both ends; median, min and max of ``reps`` after a warm-up.
    Works on a tree without the device path too (the parameters are then moved by hand)."""
    import torch

    from particle_filters_amd import dpf_rnn_torch as RT
    from tests import dpf_rnn_grad_restatement as G

    d = 2
    rng = np.random.default_rng([N, H, B, 7])
    obs = torch.tensor(rng.standard_normal((B, TORCH_STEPS, d)), device=device)
    noise = [torch.tensor(rng.standard_normal((B, N, d)), device=device) for _ in range(TORCH_STEPS)]
    a = torch.tensor(0.9, dtype=torch.float64, device=device)
    calls = {"k": 0}

    def transition_fn(x, params):  # G.lgssm with the noise on the tensors' device
        eps = noise[calls["k"] % len(noise)]
        calls["k"] += 1
        return a * x + 0.5 * eps

    _, log_likelihood_fn = G.lgssm([], a)
    kw = {} if check_values else {"check_values": False}
    dpf = RT.DifferentiableParticleFilterRNN(N, d, transition_fn, log_likelihood_fn, rnn_type=cell, rnn_hidden_dim=H,
                                             rng=np.random.default_rng(3), **kw)
    if hasattr(dpf, "to"):
        dpf.to(device)
    else:
        for p in dpf.parameters():
            p.data = p.data.to(device)
    opt = torch.optim.SGD(dpf.parameters(), lr=1e-3)
    mean = torch.zeros(d, dtype=torch.float64, device=device)
    chol = torch.eye(d, dtype=torch.float64, device=device)

    def iteration():
        opt.zero_grad()
        ps, _, As = dpf.filter(obs, mean, chol)
        loss = G.filter_loss(ps, As, obs)
        loss.backward()
        opt.step()

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
        dpf.close()
    return {"N": N, "H": H, "B": B, "cell": cell, "steps": TORCH_STEPS, "ms": float(np.median(times)),
            "min_ms": min(times), "max_ms": max(times)}


def main_torch(a):
    rows = []
    for N, H, B in TORCH_SHAPES:
        for cell in ("lstm", "gru"):
            r = torch_training_ms(N, H, B, cell, a.torch, a.reps, not a.no_check_values)
            rows.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps({"bench": "rnn_torch_training", "tensors": a.torch, "check_values": not a.no_check_values,
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
    ap.add_argument("--backward", action="store_true", help="also time pf_rnn_backward on every shape")
    ap.add_argument("--torch", choices=["cpu", "cuda"], default=None,
                    help="time one training iteration of dpf_rnn_torch's filter on tensors of this device instead")
    ap.add_argument("--no-check-values", action="store_true", help="--torch: check_values=False")
    ap.add_argument("--label", default="", help="--torch: a name for the arrangement, copied to the result")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert NV.device_count() > 0, "bench_rnn needs a HIP device"
    if a.torch:
        return main_torch(a)
    ev = Events()
    rows = []
    for N, H, L, B, stream in SHAPES:
        for cell in ("lstm", "gru"):
            r = gpu_times(N, H, L, cell, B, stream, a.reps, ev, a.backward)
            if not a.no_numpy and not stream:
                r.update(numpy_call_ms(N, H, L, cell, B))
            rows.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps({"bench": "rnn_resample", "temperature": TEMP, "rows": rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
