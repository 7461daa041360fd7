"""The device-pointer entries of the Sinkhorn OT resampler at the C-ABI level (-m gpu, MI355X):
pf_ot_resample_dev / pf_ot_backward_dev against pf_ot_resample / pf_ot_replay / pf_ot_backward.

The device buffers are torch CUDA tensors; the inputs are the cases of tests/dpf_ot_restatement.py.
The host entries are pinned to the restatements by the existing tests; here every comparison is on
the same input bits and is bitwise: the two kinds of entry enqueue the same kernels on the same
values, and the history the forward pass records itself (the third mode of the tau kernels, gated by
the done flag) holds the iterates of the replay (gated by the iteration counts).  Every output buffer
is filled with NaN (-7 for the int32 ones) before the call: the entries write every element.

1. forward: outputs all given and all null; N = 1; 65 (unsplit column tiles of 64 + 1, S = 3); 130
   (S = 5) with three problems that stop at different iterations, and with three component chunks;
   no and one iteration; the unsplit order;
2. the recorded history against pf_ot_replay, rows past each stop included, and the floor case whose
   argmax rows hold indices;
3. backward: with the recorded history, with a null one (the replay), k_sweep = max K_b against k_cap,
   a count above k_cap;
4. the stream contract; 5. the arguments; 6. the LDS-poison hook.
"""

import numpy as np
import pytest
import torch

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_ot as OT
from tests import dpf_ot_restatement as R

pytestmark = pytest.mark.gpu

MIN_VAL, TOL_STOP = 1e-12, 1e-6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert NV.device_count() > 0, "no HIP device visible: -m gpu tests must run on an MI355X"
    assert torch.cuda.is_available()


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device="cuda")


def ptr(t):
    return 0 if t is None else t.data_ptr()


def host(t):
    return None if t is None else t.cpu().numpy()


def nan(*shape):
    return torch.full(shape, np.nan, dtype=torch.float64, device="cuda")


def junk32(*shape):
    return torch.full(shape, -7, dtype=torch.int32, device="cuda")


_side = []


def side_stream():
    """A caller's stream (torch's current stream is the null stream, which the entries take as "the
    handle's own"); the callers below synchronise the device before and after their call on it."""
    if not _side:
        _side.append(torch.cuda.Stream())
    return _side[0].cuda_stream


def same_bits(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), k
        if x is not None:
            assert x.shape == y.shape and np.array_equal(x, y), f"array {k} differs in {int(np.sum(x != y))} elements"
    return True


# ---------------------------------------------------------------------- the cases: (X [B,N,d], w [B,N], eps, n_iters)
def batch_case():
    c = R.BATCH
    cases = [R.make_case(c["N"], c["d"], c["scale"], c["conc"], s) for s, _ in c["seeds"]]
    return np.stack([x for x, _ in cases]), np.stack([w for _, w in cases]), c["eps"], R.EARLY_ITERS


def chunk_case():
    c = R.CHUNK_BATCH
    cases = [R.solved_chunk_batch(b)[:2] for b in range(3)]
    return np.stack([x for x, _ in cases]), np.stack([w for _, w in cases]), c["eps"], c["n_iters"]


def single(N, d, eps=0.1, n_iters=50, seed=0):
    X, w = R.make_case(N, d, seed=seed)
    return X[None], w[None], eps, n_iters


def floor_case():
    X, w, eps, n_iters = R.edge_case("floor eps=0.1")
    return X[None], w[None], eps, n_iters


CASES = {"N1-d2": lambda: single(1, 2), "N65-d1": lambda: single(65, 1), "N130-d3-B3-early": batch_case,
         "N130-d40-B3": chunk_case, "no-iteration": lambda: single(65, 1, n_iters=0),
         "one-iteration": lambda: single(65, 1, n_iters=1)}
BATCH_STOPS = [k for _, k in R.BATCH["seeds"]]


def grad_of(X):
    return np.random.default_rng([X.shape[1], X.shape[2], 99]).standard_normal(X.shape)


# ---------------------------------------------------------------------- the two kinds of entry
def fwd_host(h, X, w, eps, n_iters, outs=True):
    """[X_out, iterations, change history, f, g, plan statistics] of pf_ot_resample."""
    out, its, hist, f, g, stats = h.resample(X, w, eps, n_iters, MIN_VAL, TOL_STOP, outs)
    if outs:
        hist = hist[:, :n_iters]
    return [out, its if outs else None, hist, f, g, stats]


def fwd_dev(h, X, w, eps, n_iters, outs=True, record=False, stream=0, bufs=None):
    """The same of pf_ot_resample_dev, and with ``record`` the history (hist, hist_argmax) behind them."""
    B, N, d = X.shape
    Xd, wd = dev(X), dev(w)
    out = nan(B, N, d)
    its = junk32(B) if outs else None
    ch = nan(B, n_iters, 2) if outs else None
    f, g, st = (nan(B, N), nan(B, N), nan(B, 2)) if outs else (None, None, None)
    hv = nan(B, 4, n_iters + 1, N) if record else None
    am = junk32(B, n_iters, N) if record else None
    torch.cuda.synchronize()  # the fills, which ran on torch's stream
    h.resample_dev(stream, Xd.data_ptr(), wd.data_ptr(), eps, n_iters, MIN_VAL, TOL_STOP, out.data_ptr(), ptr(its),
                   ptr(ch), ptr(f), ptr(g), ptr(st), ptr(hv), ptr(am) if n_iters else 0)
    torch.cuda.synchronize()
    if bufs is not None:
        bufs.update(X=Xd, w=wd, its=its, hist=hv, am=am)
    res = [host(t) for t in (out, its, ch, f, g, st)]
    return res + [host(hv), host(am)] if record else res


def bwd_host(h, X, w, G, eps, its, hist=None, am=None):
    """[grad_X, grad_w] of pf_ot_backward with k_cap = max(its), the replay's layout."""
    return list(h.backward(X, w, G, eps, MIN_VAL, its, hist, am))


def bwd_dev(h, bufs, G, eps, k_cap, k_sweep, with_hist=True, its=None, stream=0):
    """[grad_X, grad_w] of pf_ot_backward_dev on the buffers a recording fwd_dev left in ``bufs``."""
    Gd = dev(G)
    gX, gw = torch.full_like(bufs["X"], np.nan), torch.full_like(bufs["w"], np.nan)
    K = bufs["its"] if its is None else its
    torch.cuda.synchronize()
    h.backward_dev(stream, bufs["X"].data_ptr(), bufs["w"].data_ptr(), eps, MIN_VAL, K.data_ptr(), k_cap, k_sweep,
                   ptr(bufs["hist"]) if with_hist else 0, ptr(bufs["am"]) if with_hist and k_cap else 0, Gd.data_ptr(),
                   gX.data_ptr(), gw.data_ptr())
    torch.cuda.synchronize()
    return [host(gX), host(gw)]


def handle(X):
    return OT._Handle(X.shape[1], X.shape[2], X.shape[0])


# ====================================================================== 1. forward
@pytest.mark.parametrize("outs", [True, False], ids=["all-outputs", "null-outputs"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_gives_the_host_entrys_bits(name, outs, monkeypatch):
    monkeypatch.delenv("PF_TEST_OT_SPLITS", raising=False)
    X, w, eps, n_iters = CASES[name]()
    hh, hd = handle(X), handle(X)
    try:
        ref = fwd_host(hh, X, w, eps, n_iters, outs)
        got = fwd_dev(hd, X, w, eps, n_iters, outs)
        on_stream = fwd_dev(hd, X, w, eps, n_iters, outs, stream=side_stream())
    finally:
        hh.close()
        hd.close()
    assert np.all(np.isfinite(ref[0]))
    if name == "N130-d3-B3-early" and outs:
        assert list(ref[1]) == BATCH_STOPS
    assert same_bits(got, ref)
    assert same_bits(on_stream, ref)  # nothing polled: all n_iters iterations enqueued


def test_forward_with_the_unsplit_order(monkeypatch):
    X, w, eps, n_iters = chunk_case()
    monkeypatch.delenv("PF_TEST_OT_SPLITS", raising=False)
    h = handle(X)
    try:
        plain = fwd_dev(h, X, w, eps, n_iters)
    finally:
        h.close()
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_OT_SPLITS", "1")
    hh, hd = handle(X), handle(X)
    try:
        ref = fwd_host(hh, X, w, eps, n_iters)
        got = fwd_dev(hd, X, w, eps, n_iters, record=True)
        rep = hh.replay(X, w, eps, MIN_VAL, ref[1])
    finally:
        hh.close()
        hd.close()
    assert same_bits(got[:6], ref)
    assert same_bits(got[6:], [rep.hist, rep.hist_argmax])  # the unsplit pass records without the merge
    assert not np.array_equal(got[0], plain[0])  # the hook took effect: another summation order


# ====================================================================== 2. the recorded history
def padded_replay(h, X, w, eps, its, n_iters):
    """pf_ot_replay's history with k_cap = n_iters, the layout the forward pass records in."""
    B, N, _ = X.shape
    i32 = NV.C.POINTER(NV.C.c_int32)
    hist = np.full((B, 4, n_iters + 1, N), np.nan)
    am = np.full((B, n_iters, N), -7, dtype=np.int32)
    its = np.ascontiguousarray(its, dtype=np.int32)
    NV.check(NV.load().pf_ot_replay(h.h, NV.dptr(X), NV.dptr(w), float(eps), MIN_VAL, its.ctypes.data_as(i32), n_iters,
                                    NV.dptr(hist), am.ctypes.data_as(i32) if n_iters else None), "pf_ot_replay")
    return hist, am


@pytest.mark.parametrize("name", ["N130-d3-B3-early", "N130-d40-B3", "N65-d1", "no-iteration", "one-iteration", "floor"])
def test_the_recorded_history_is_the_replays(name, monkeypatch):
    monkeypatch.delenv("PF_TEST_OT_SPLITS", raising=False)
    X, w, eps, n_iters = floor_case() if name == "floor" else CASES[name]()
    hh, hd = handle(X), handle(X)
    try:
        ref = fwd_host(hh, X, w, eps, n_iters)
        hist, am = padded_replay(hh, X, w, eps, ref[1], n_iters)
        got = fwd_dev(hd, X, w, eps, n_iters, record=True)
        on_stream = fwd_dev(hd, X, w, eps, n_iters, record=True, stream=side_stream())
    finally:
        hh.close()
        hd.close()
    assert same_bits(got[:6], ref)  # recording changes no result
    assert same_bits(got[6:], [hist, am])
    assert same_bits(on_stream, got)
    for b, K in enumerate(ref[1]):  # the rows past each stop, written by the entry over the NaN fill
        assert not got[6][b, :, K + 1:].any() and np.all(got[7][b, K:] == -1)
        assert np.array_equal(got[6][b, 0, K], ref[3][b]) and np.array_equal(got[6][b, 1, K], ref[4][b])
    if name == "floor":
        assert np.any(got[7] >= 0)  # the argmax path was taken
    if name == "N130-d3-B3-early":
        assert list(ref[1]) == BATCH_STOPS


# ====================================================================== 3. backward
@pytest.mark.parametrize("name", ["N130-d3-B3-early", "N130-d40-B3", "N1-d2", "no-iteration", "floor"])
def test_backward_gives_the_host_entrys_bits(name, monkeypatch):
    monkeypatch.delenv("PF_TEST_OT_SPLITS", raising=False)
    X, w, eps, n_iters = floor_case() if name == "floor" else CASES[name]()
    G = grad_of(X)
    hh, hd = handle(X), handle(X)
    try:
        its = fwd_host(hh, X, w, eps, n_iters)[1]
        ref = bwd_host(hh, X, w, G, eps, its)
        rep = hh.replay(X, w, eps, MIN_VAL, its)
        assert same_bits(bwd_host(hh, X, w, G, eps, its, rep.hist, rep.hist_argmax), ref)
        bufs = {}
        fwd_dev(hd, X, w, eps, n_iters, record=True, bufs=bufs)
        kmax = int(its.max())
        sweep = max(kmax, 1) if n_iters else 0
        recorded = bwd_dev(hd, bufs, G, eps, n_iters, sweep)
        replayed = bwd_dev(hd, bufs, G, eps, n_iters, sweep, with_hist=False)
        full_sweep = bwd_dev(hd, bufs, G, eps, n_iters, n_iters)
        full_replay = bwd_dev(hd, bufs, G, eps, n_iters, n_iters, with_hist=False)
        on_stream = bwd_dev(hd, bufs, G, eps, n_iters, sweep, stream=side_stream())
    finally:
        hh.close()
        hd.close()
    assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1]))
    for tag, got in (("recorded", recorded), ("replayed", replayed), ("k_sweep = k_cap", full_sweep),
                     ("k_sweep = k_cap, replayed", full_replay), ("caller's stream", on_stream)):
        assert same_bits(got, ref), tag


def test_a_count_outside_the_sweep_is_clamped():
    X, w, eps, n_iters = chunk_case()  # full length: every problem's history holds k_cap iterations
    G = grad_of(X)
    h = handle(X)
    try:
        bufs = {}
        its = fwd_dev(h, X, w, eps, n_iters, record=True, bufs=bufs)[1]
        assert list(its) == [n_iters] * 3
        ref = bwd_dev(h, bufs, G, eps, n_iters, n_iters)
        above = torch.tensor([n_iters + 5, n_iters, 1 << 30], dtype=torch.int32, device="cuda")
        assert same_bits(bwd_dev(h, bufs, G, eps, n_iters, n_iters, its=above), ref)
        assert same_bits(bwd_dev(h, bufs, G, eps, n_iters, n_iters, its=above, with_hist=False), ref)
        # below: a negative count is no iteration, the count of a problem that never ran
        none = torch.tensor([-3, n_iters, n_iters], dtype=torch.int32, device="cuda")
        zero = torch.tensor([0, n_iters, n_iters], dtype=torch.int32, device="cuda")
        assert same_bits(bwd_dev(h, bufs, G, eps, n_iters, n_iters, its=none, with_hist=False),
                         bwd_dev(h, bufs, G, eps, n_iters, n_iters, its=zero, with_hist=False))
        # a sweep shorter than the counts: as if every problem had stopped there
        short = bwd_dev(h, bufs, G, eps, n_iters, 7, with_hist=False)
        seven = torch.full((3,), 7, dtype=torch.int32, device="cuda")
        assert same_bits(short, bwd_dev(h, bufs, G, eps, n_iters, n_iters, its=seven, with_hist=False))
    finally:
        h.close()


# ====================================================================== 4. the stream contract
def test_a_callers_stream_without_synchronisation_and_a_host_entry_straight_after():
    X, w, eps, n_iters = batch_case()
    G = grad_of(X)
    B, N, d = X.shape
    h = handle(X)
    try:
        # the synchronised run, on the bits the stream run will see: 0.5 X is exact
        bufs = {}
        ref = fwd_dev(h, 0.5 * X, w, eps, n_iters, record=True, bufs=bufs)
        ref_g = bwd_dev(h, bufs, G, eps, n_iters, n_iters)
        half, wd, Gd = dev(X), dev(w), dev(G)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            Xd = half * 0.5  # the input is produced on the stream, by the op in front of the entry
            out, its = torch.empty_like(Xd), torch.empty(B, dtype=torch.int32, device="cuda")
            hv = torch.empty((B, 4, n_iters + 1, N), dtype=torch.float64, device="cuda")
            am = torch.empty((B, n_iters, N), dtype=torch.int32, device="cuda")
            h.resample_dev(s.cuda_stream, Xd.data_ptr(), wd.data_ptr(), eps, n_iters, MIN_VAL, TOL_STOP, out.data_ptr(),
                           its.data_ptr(), hist=hv.data_ptr(), hist_argmax=am.data_ptr())
            twice = out + out  # and the output consumed by the op behind it
            gX, gw = torch.empty_like(Xd), torch.empty_like(wd)
            h.backward_dev(s.cuda_stream, Xd.data_ptr(), wd.data_ptr(), eps, MIN_VAL, its.data_ptr(), n_iters, n_iters,
                           hv.data_ptr(), am.data_ptr(), Gd.data_ptr(), gX.data_ptr(), gw.data_ptr())
        # a host entry on the same handle straight after, other input: the fence orders it behind the stream's work
        other = fwd_host(h, X, w, eps, n_iters)
        s.synchronize()
        assert same_bits([host(out), host(its), host(hv), host(am)], [ref[0], ref[1], ref[6], ref[7]])
        assert np.array_equal(host(twice), ref[0] + ref[0])
        assert same_bits([host(gX), host(gw)], ref_g)
        fresh = handle(X)
        try:
            assert same_bits(other, fwd_host(fresh, X, w, eps, n_iters))
        finally:
            fresh.close()
    finally:
        h.close()


def test_a_null_stream_returns_with_the_result_complete():
    X, w, eps, n_iters = single(65, 1)
    h = handle(X)
    try:
        ref = fwd_host(h, X, w, eps, n_iters)[0]
        Xd, wd = dev(X), dev(w)
        out = torch.full_like(Xd, np.nan)
        torch.cuda.synchronize()
        h.resample_dev(0, Xd.data_ptr(), wd.data_ptr(), eps, n_iters, MIN_VAL, TOL_STOP, out.data_ptr())
        # the handle's stream does not block torch's: the copy below waits for nothing of the entry's
        assert np.array_equal(host(out), ref)
    finally:
        h.close()


def test_close_straight_after_an_asynchronous_call():
    X, w, eps, n_iters = chunk_case()
    G = grad_of(X)
    B, N, d = X.shape
    h = handle(X)
    try:
        its_ref = fwd_host(h, X, w, eps, n_iters)
        ref = its_ref[0]
        ref_g = bwd_host(h, X, w, G, eps, its_ref[1])
    finally:
        h.close()
    h = handle(X)
    Xd, wd, Gd = dev(X), dev(w), dev(G)
    out, its = torch.full_like(Xd, np.nan), junk32(B)
    gX, gw = torch.full_like(Xd, np.nan), torch.full_like(wd, np.nan)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        h.resample_dev(s.cuda_stream, Xd.data_ptr(), wd.data_ptr(), eps, n_iters, MIN_VAL, TOL_STOP, out.data_ptr(),
                       its.data_ptr())
        h.backward_dev(s.cuda_stream, Xd.data_ptr(), wd.data_ptr(), eps, MIN_VAL, its.data_ptr(), n_iters, n_iters, 0, 0,
                       Gd.data_ptr(), gX.data_ptr(), gw.data_ptr())
    finally:
        h.close()
    s.synchronize()
    assert np.array_equal(host(out), ref)
    assert same_bits([host(gX), host(gw)], ref_g)


# ====================================================================== 5. the arguments
def test_the_entries_reject_bad_arguments():
    X, w, eps, n_iters = single(65, 3, n_iters=4)
    B, N, d = X.shape
    h = handle(X)
    try:
        Xd, wd, Gd = dev(X), dev(w), dev(grad_of(X))
        out, its = torch.empty_like(Xd), torch.empty(B, dtype=torch.int32, device="cuda")
        hv, am = nan(B, 4, n_iters + 1, N), junk32(B, n_iters, N)
        f = nan(B, N)
        a = (0, Xd.data_ptr(), wd.data_ptr(), eps, n_iters, MIN_VAL, TOL_STOP)
        with pytest.raises(ValueError, match="aliases an input"):
            h.resample_dev(*a, Xd.data_ptr())
        with pytest.raises(ValueError, match="aliases an input"):  # an overlap, not the same pointer
            h.resample_dev(*a, Xd.data_ptr() + 8)
        with pytest.raises(ValueError, match="aliases an input"):
            h.resample_dev(*a, out.data_ptr(), f=wd.data_ptr())
        with pytest.raises(ValueError, match="aliases an input"):
            h.resample_dev(*a, out.data_ptr(), iterations=wd.data_ptr())
        with pytest.raises(ValueError, match="aliases an input"):
            h.resample_dev(*a, out.data_ptr(), hist=hv.data_ptr(), hist_argmax=Xd.data_ptr())
        with pytest.raises(ValueError, match="come together or not at all"):
            h.resample_dev(*a, out.data_ptr(), hist=hv.data_ptr())
        with pytest.raises(ValueError, match="come together or not at all"):
            h.resample_dev(*a, out.data_ptr(), hist_argmax=am.data_ptr())
        with pytest.raises(ValueError, match="flags must be 0 or PF_OT_RESIDENT"):
            h.resample_dev(*a, out.data_ptr(), flags=2)
        # the host entry's messages
        with pytest.raises(ValueError, match="epsilon must be positive"):
            h.resample_dev(0, Xd.data_ptr(), wd.data_ptr(), 0.0, n_iters, MIN_VAL, TOL_STOP, out.data_ptr())
        with pytest.raises(ValueError, match="n_iters out of range"):
            h.resample_dev(0, Xd.data_ptr(), wd.data_ptr(), eps, -1, MIN_VAL, TOL_STOP, out.data_ptr())
        with pytest.raises(ValueError, match="null argument"):
            h.resample_dev(*a, 0)
        with pytest.raises(ValueError, match="null argument"):
            h.resample_dev(0, 0, wd.data_ptr(), eps, n_iters, MIN_VAL, TOL_STOP, out.data_ptr())

        h.resample_dev(*a, out.data_ptr(), its.data_ptr(), hist=hv.data_ptr(), hist_argmax=am.data_ptr())
        gX, gw = torch.empty_like(Xd), torch.empty_like(wd)
        b = (0, Xd.data_ptr(), wd.data_ptr(), eps, MIN_VAL, its.data_ptr())
        hp, ap, o = hv.data_ptr(), am.data_ptr(), (Gd.data_ptr(), gX.data_ptr(), gw.data_ptr())
        h.backward_dev(*b, n_iters, n_iters, hp, ap, *o)
        with pytest.raises(ValueError, match="aliases an input"):
            h.backward_dev(*b, n_iters, n_iters, hp, ap, Gd.data_ptr(), Gd.data_ptr(), gw.data_ptr())
        with pytest.raises(ValueError, match="aliases an input"):
            h.backward_dev(*b, n_iters, n_iters, hp, ap, Gd.data_ptr(), gX.data_ptr(), wd.data_ptr())
        with pytest.raises(ValueError, match="aliases an input"):
            h.backward_dev(*b, n_iters, n_iters, hp, ap, Gd.data_ptr(), hv.data_ptr() + 16, gw.data_ptr())
        with pytest.raises(ValueError, match="come together or not at all"):
            h.backward_dev(*b, n_iters, n_iters, hp, 0, *o)
        with pytest.raises(ValueError, match="come together or not at all"):
            h.backward_dev(*b, n_iters, n_iters, 0, ap, *o)
        for k_sweep in (0, n_iters + 1, -1):
            with pytest.raises(ValueError, match="k_sweep must be in 1 .. k_cap"):
                h.backward_dev(*b, n_iters, k_sweep, hp, ap, *o)
        with pytest.raises(ValueError, match="k_sweep must be in 1 .. k_cap"):
            h.backward_dev(*b, 0, 1, 0, 0, *o)
        with pytest.raises(ValueError, match="k_cap out of range"):
            h.backward_dev(*b, -1, -1, 0, 0, *o)
        with pytest.raises(ValueError, match="epsilon must be positive"):
            h.backward_dev(0, Xd.data_ptr(), wd.data_ptr(), -1.0, MIN_VAL, its.data_ptr(), n_iters, n_iters, hp, ap, *o)
        with pytest.raises(ValueError, match="null argument"):
            h.backward_dev(0, Xd.data_ptr(), wd.data_ptr(), eps, MIN_VAL, 0, n_iters, n_iters, hp, ap, *o)
        with pytest.raises(ValueError, match="null argument"):
            h.backward_dev(*b, n_iters, n_iters, hp, ap, 0, gX.data_ptr(), gw.data_ptr())
    finally:
        h.close()


# ====================================================================== 6. the LDS-poison hook
def test_the_new_paths_are_poisoned_and_do_not_read_uninitialised_lds(monkeypatch):
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    monkeypatch.delenv("PF_TEST_OT_SPLITS", raising=False)
    X, w, eps, n_iters = chunk_case()
    G = grad_of(X)

    def run():
        h = handle(X)
        try:
            bufs = {}
            fwd = fwd_dev(h, X, w, eps, n_iters, record=True, bufs=bufs)
            return fwd + bwd_dev(h, bufs, G, eps, n_iters, n_iters) + bwd_dev(h, bufs, G, eps, n_iters, n_iters, False)
        finally:
            h.close()

    clean = run()
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_LDS_POISON", "1")
    count = NV.load().pf_test_lds_poison_count
    before = int(count())
    got = run()
    # forward: prepare, cost, two per iteration, project, stats; each backward: prepare, cost, q, one per
    # iteration, cost, weights; the replay one more per iteration
    assert int(count()) >= before + (4 + 2 * n_iters) + 2 * (5 + n_iters) + n_iters
    assert all(np.all(np.isfinite(a)) for a in got if a.dtype == np.float64)
    assert same_bits(got, clean)
