"""The device-pointer entries of the soft and the RNN resampler at the C-ABI level (-m gpu, MI355X):
pf_soft_resample_dev / pf_soft_backward_dev / pf_rnn_set_weights_dev / pf_rnn_resample_dev /
pf_rnn_backward_dev against the host entries of the same names.

The device buffers are torch CUDA tensors; the inputs are those of the case generators of
tests/dpf_rnn_restatement.py, tests/dpf_rnn_grad_restatement.py and tests/dpf_soft_restatement.py.
The host entries are pinned to the restatements by the existing tests; here every comparison is on
the same input bits and is bitwise: the two kinds of entry run the same kernels on the same values,
and the device packing of the weights (k_rnn_pack, k_rnn_pack_T) is data movement plus one IEEE
addition.

1. packing: pf_rnn_set_weights against pf_rnn_set_weights_dev on two fresh handles, then resample
   and backward; a small network after a large one, and small after small, leave no old value in the
   padding;
2. the RNN entries, 3. the soft entries, at the sizes where a tiling changes;
4. the stream contract: a caller's stream with no synchronisation around the entry, a host entry
   straight after an asynchronous one, a null stream, close() straight after an asynchronous call;
5. the arguments; 6. the LDS-poison hook on the new paths.
"""

import numpy as np
import pytest
import torch

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_rnn as RN
from particle_filters_amd import dpf_soft as SO
from tests import dpf_rnn_grad_restatement as G
from tests import dpf_rnn_restatement as R
from tests import dpf_soft_restatement as S

pytestmark = pytest.mark.gpu


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


def same_bits(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), k
        if x is not None:
            assert x.shape == y.shape and np.array_equal(x, y), f"array {k} differs in {int(np.sum(x != y))} elements"
    return True


# ====================================================================== the RNN unit
def rnn_handle(c):
    return RN._Handle(c["N"], c["d"], c["B"], c["H"], c["L"], c["cell"], c["uw"], c["up"])


def rnn_inputs(c):
    X, lw, W = R.case_inputs(c)
    gXo, gA = G.cotangents(c)
    return X, np.ascontiguousarray(np.exp(lw)), W, gXo, gA


def rnn_host(h, c, X, w, W, gXo, gA, set_weights=True):
    """(X_out, A, hid, gX, gw, gW...) through the host entries."""
    if set_weights:
        h.set_weights(W)
    out, A, hid = h.resample(X, w, c["T"], want_hidden=True)
    gX, gw, gW = h.backward(X, w, c["T"], gXo, gA, [a.shape for a in W])
    return [out, A, hid, gX, gw] + gW


def rnn_set_weights_dev(h, W, stream=0):
    Wd = [dev(a) for a in W]
    h.set_weights_dev(stream, [a.data_ptr() for a in Wd], [a.numel() for a in Wd])
    return Wd  # kept alive by the caller until the stream has read them


def rnn_dev(h, c, X, w, W, gXo, gA, stream=0, set_weights=True, want_A=True, want_hid=True):
    """The same through the device entries; a null stream synchronises."""
    B, N, d, H = c["B"], c["N"], c["d"], c["H"]
    keep = rnn_set_weights_dev(h, W, stream) if set_weights else None
    Xd, wd, gd, gAd = dev(X), dev(w), dev(gXo), dev(gA)
    out = torch.full((B, N, d), np.nan, dtype=torch.float64, device="cuda")
    A = torch.full((B, N, N), np.nan, dtype=torch.float64, device="cuda") if want_A else None
    hid = torch.full((B, N, H), np.nan, dtype=torch.float64, device="cuda") if want_hid else None
    h.resample_dev(stream, Xd.data_ptr(), wd.data_ptr(), c["T"], out.data_ptr(), ptr(A), ptr(hid))
    gX, gw = torch.full_like(Xd, np.nan), torch.full_like(wd, np.nan)
    gW = [torch.full(a.shape, np.nan, dtype=torch.float64, device="cuda") for a in W]
    h.backward_dev(stream, Xd.data_ptr(), wd.data_ptr(), c["T"], gd.data_ptr(), ptr(gAd), gX.data_ptr(), gw.data_ptr(),
                   [a.data_ptr() for a in gW], [a.numel() for a in gW])
    torch.cuda.synchronize()
    del keep
    return [host(t) for t in [out, A, hid, gX, gw] + gW]


# ---------------------------------------------------------------------- 1. packing
# (H, L, cell, use_weight, use_particle): a partial k-step (1, 3), an exact tile (16), HT = 2 with RS = 2 (17),
# HT = 3 with RS = 1 (33), the maximum (128); the inner layers' input kernels (L = 3); every feature setting
PACK = [(1, 1, "lstm", True, True), (1, 3, "gru", True, False), (3, 3, "lstm", False, True), (3, 1, "gru", True, True),
        (16, 1, "gru", False, True), (16, 3, "lstm", True, False), (17, 3, "gru", True, True),
        (17, 1, "lstm", True, False), (33, 1, "gru", True, True), (33, 3, "lstm", False, True),
        (128, 1, "lstm", True, True), (128, 3, "gru", True, False)]


def pack_case(H, L, cell, uw, up, seed=60):
    return R.case(5, 2, H, L, cell, uw=uw, up=up, B=2, seed=seed)


@pytest.mark.parametrize("net", PACK, ids=lambda n: f"H{n[0]}-L{n[1]}-{n[2]}-w{int(n[3])}p{int(n[4])}")
def test_device_packing_gives_the_host_packers_bits(net):
    c = pack_case(*net)
    X, w, W, gXo, gA = rnn_inputs(c)
    hh, hd = rnn_handle(c), rnn_handle(c)
    try:
        ref = rnn_host(hh, c, X, w, W, gXo, gA)
        got = rnn_dev(hd, c, X, w, W, gXo, gA)
        assert hd.packs == 1
    finally:
        hh.close()
        hd.close()
    assert all(np.all(np.isfinite(a)) for a in ref)
    assert same_bits(got, ref)


def test_a_smaller_or_another_network_leaves_nothing_in_the_padding():
    big, small = pack_case(33, 3, "gru", True, True), pack_case(3, 1, "gru", True, True)
    other = pack_case(3, 1, "gru", True, True, seed=61)  # the small shape with other values
    Xb, wb, Wb, gb, gAb = rnn_inputs(big)
    h = rnn_handle(big)
    try:
        rnn_dev(h, big, Xb, wb, Wb, gb, gAb)
    finally:
        h.close()  # its buffers go back to the allocator: the next handle's are likely the same addresses
    X, w, W, gXo, gA = rnn_inputs(small)
    _, _, W2, _, _ = rnn_inputs(other)
    assert not np.array_equal(W[0], W2[0])
    h = rnn_handle(small)
    try:
        got = rnn_dev(h, small, X, w, W, gXo, gA)
        got2 = rnn_dev(h, small, X, w, W2, gXo, gA)  # small after small, the transposed set with it
        assert h.packs == 2
    finally:
        h.close()
    for Wk, g in ((W, got), (W2, got2)):
        fresh = rnn_handle(small)
        try:
            assert same_bits(g, rnn_host(fresh, small, X, w, Wk, gXo, gA))
        finally:
            fresh.close()
    assert not np.array_equal(got[0], got2[0])


# ---------------------------------------------------------------------- 2. the RNN entries
# N = 1: one timestep; 17: two 16-sequence tiles with padded rows; 50.  (N, d, B, H, L, cell, grad_A, A and hid)
ENTRIES = [(1, 1, 1, 5, 1, "lstm", False, False), (17, 3, 3, 5, 2, "gru", True, True),
           (50, 1, 3, 8, 1, "lstm", True, False), (50, 3, 1, 8, 1, "gru", False, True),
           (17, 1, 1, 16, 1, "lstm", True, True)]


def entry_case(N, d, B, H, L, cell):
    return R.case(N, d, H, L, cell, B=B, seed=70)


def rnn_entry_pair(e):
    N, d, B, H, L, cell, with_gA, with_outs = e
    c = entry_case(N, d, B, H, L, cell)
    X, w, W, gXo, gA = rnn_inputs(c)
    gA = gA if with_gA else None
    hh, hd = rnn_handle(c), rnn_handle(c)
    try:
        ref = rnn_host(hh, c, X, w, W, gXo, gA)
        hd.set_weights(W)  # the host packer on both: this test is about the entries
        got = rnn_dev(hd, c, X, w, W, gXo, gA, set_weights=False, want_A=with_outs, want_hid=with_outs)
        resident = hd.resident
    finally:
        hh.close()
        hd.close()
    if not with_outs:
        ref[1] = ref[2] = None
    return got, ref, resident


@pytest.mark.parametrize("e", ENTRIES, ids=lambda e: f"N{e[0]}-d{e[1]}-B{e[2]}-{e[5]}-gA{int(e[6])}-outs{int(e[7])}")
def test_rnn_entries_give_the_host_entries_bits(e, monkeypatch):
    monkeypatch.delenv("PF_TEST_RNN_STREAM", raising=False)
    got, ref, resident = rnn_entry_pair(e)
    assert resident and same_bits(got, ref)


def test_rnn_entries_under_forced_streaming(monkeypatch):
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_RNN_STREAM", "1")
    got, ref, resident = rnn_entry_pair(ENTRIES[1])
    assert not resident and same_bits(got, ref)


# ====================================================================== the soft unit
def soft_inputs(N, d, B, seed):
    X = np.stack([S.make_case(N, d, seed=seed + b)[0] for b in range(B)])
    lw = np.stack([S.make_case(N, d, seed=seed + b)[1] for b in range(B)])
    lp = np.ascontiguousarray(S.log_probs(lw, 0.1))
    g = np.random.default_rng([N, d, B, seed, 99]).standard_normal((B, N, d))
    return X, lp, g


def soft_host(h, X, lp, g, T, seed, epoch, base, entropy, saved):
    out, H = h.resample(X, lp, T, seed, epoch, base, entropy)
    M, L = h.row_stats()
    gX, glp = h.backward(X, lp, T, g, seed, epoch, base, (out, M, L) if saved else None)
    return [out, H, M, L, gX, glp]


def soft_dev(h, X, lp, g, T, seed, epoch, base, entropy, saved, stream=0):
    Xd, lpd, gd = dev(X), dev(lp), dev(g)
    out = torch.full_like(Xd, np.nan)
    H = torch.full_like(lpd, np.nan) if entropy else None
    M, L = torch.full_like(lpd, np.nan), torch.full_like(lpd, np.nan)
    h.resample_dev(stream, Xd.data_ptr(), lpd.data_ptr(), T, seed, epoch, base, out.data_ptr(), ptr(H), M.data_ptr(),
                   L.data_ptr())
    gX, glp = torch.full_like(Xd, np.nan), torch.full_like(lpd, np.nan)
    sv = (out, M, L) if saved else (None, None, None)
    h.backward_dev(stream, Xd.data_ptr(), lpd.data_ptr(), T, seed, epoch, base, ptr(sv[0]), ptr(sv[1]), ptr(sv[2]),
                   gd.data_ptr(), gX.data_ptr(), glp.data_ptr())
    torch.cuda.synchronize()
    return [host(t) for t in [out, H, M, L, gX, glp]]


# N = 1; 65 and 130: two and three 64-row tiles; d = 17: two component chunks.  (N, d, B, entropy, saved)
SOFT = [(1, 1, 1, True, True), (65, 17, 3, False, True), (65, 1, 1, True, False), (130, 17, 1, True, True),
        (130, 1, 3, False, False)]


def soft_pair(s):
    N, d, B, entropy, saved = s
    X, lp, g = soft_inputs(N, d, B, seed=80)
    args = (0.2, 2024, 3, 5, entropy, saved)  # T, seed, a non-zero epoch and batch_base
    hh, hd = SO._Handle(N, d, B), SO._Handle(N, d, B)
    try:
        ref = soft_host(hh, X, lp, g, *args)
        got = soft_dev(hd, X, lp, g, *args)
    finally:
        hh.close()
        hd.close()
    return got, ref


@pytest.mark.parametrize("s", SOFT, ids=lambda s: f"N{s[0]}-d{s[1]}-B{s[2]}-H{int(s[3])}-saved{int(s[4])}")
def test_soft_entries_give_the_host_entries_bits(s, monkeypatch):
    monkeypatch.delenv("PF_TEST_SOFT_SPLITS", raising=False)
    got, ref = soft_pair(s)
    assert all(np.all(np.isfinite(a)) for a in ref if a is not None)
    assert same_bits(got, ref)


def test_soft_entries_with_the_unsplit_order(monkeypatch):
    monkeypatch.delenv("PF_TEST_SOFT_SPLITS", raising=False)
    plain, _ = soft_pair(SOFT[3])
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_SOFT_SPLITS", "1")
    got, ref = soft_pair(SOFT[3])
    assert same_bits(got, ref)
    assert not np.array_equal(got[0], plain[0])  # the hook took effect: another summation order


# ====================================================================== 4. the stream contract
def test_rnn_on_a_callers_stream_without_synchronisation():
    c = entry_case(17, 3, 3, 5, 2, "gru")
    X, w, W, gXo, gA = rnn_inputs(c)
    B, N, d = c["B"], c["N"], c["d"]
    h = rnn_handle(c)
    try:
        # the synchronised run, on the bits the stream run will see: 0.5 X is exact
        ref = rnn_dev(h, c, 0.5 * X, w, W, gXo, gA)
        half, wd = dev(X), dev(w)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            keep = rnn_set_weights_dev(h, W, s.cuda_stream)
            Xd = half * 0.5  # the input is produced on the stream, by the op in front of the entry
            out = torch.empty((B, N, d), dtype=torch.float64, device="cuda")
            A = torch.empty((B, N, N), dtype=torch.float64, device="cuda")
            h.resample_dev(s.cuda_stream, Xd.data_ptr(), wd.data_ptr(), c["T"], out.data_ptr(), A.data_ptr(), 0)
            twice = out + out  # and the output consumed by the op behind it
        # a host entry on the same handle straight after: the fence orders it behind the stream's work
        again = h.resample(0.5 * X, w, c["T"])
        s.synchronize()
        del keep
        assert np.array_equal(host(out), ref[0]) and np.array_equal(host(A), ref[1])
        assert np.array_equal(host(twice), ref[0] + ref[0])
        assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])
    finally:
        h.close()


def test_soft_on_a_callers_stream_and_a_host_entry_straight_after():
    N, d, B = 130, 17, 3
    X, lp, g = soft_inputs(N, d, B, seed=81)
    h = SO._Handle(N, d, B)
    try:
        ref = soft_dev(h, 0.5 * X, lp, g, 0.2, 7, 1, 0, False, True)
        half, lpd = dev(X), dev(lp)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            Xd = half * 0.5
            out, M, L = torch.empty_like(Xd), torch.empty_like(lpd), torch.empty_like(lpd)
            h.resample_dev(s.cuda_stream, Xd.data_ptr(), lpd.data_ptr(), 0.2, 7, 1, 0, out.data_ptr(), 0, M.data_ptr(),
                           L.data_ptr())
            twice = out + out
        other = h.resample(X, lp, 0.2, 7, 1, 0)[0]  # a host entry, other input, no synchronisation in between
        rows = h.row_stats()
        s.synchronize()
        assert np.array_equal(host(out), ref[0]) and np.array_equal(host(M), ref[2]) and np.array_equal(host(L), ref[3])
        assert np.array_equal(host(twice), ref[0] + ref[0])
        fresh = SO._Handle(N, d, B)
        try:
            assert np.array_equal(other, fresh.resample(X, lp, 0.2, 7, 1, 0)[0])
            assert same_bits(list(rows), list(fresh.row_stats()))
        finally:
            fresh.close()
    finally:
        h.close()


def test_a_null_stream_returns_with_the_result_complete():
    N, d, B = 65, 1, 1
    X, lp, g = soft_inputs(N, d, B, seed=82)
    h = SO._Handle(N, d, B)
    try:
        ref = h.resample(X, lp, 0.2, 7, 0, 0)[0]
        Xd, lpd = dev(X), dev(lp)
        out = torch.full_like(Xd, np.nan)
        torch.cuda.synchronize()
        h.resample_dev(0, Xd.data_ptr(), lpd.data_ptr(), 0.2, 7, 0, 0, out.data_ptr())
        # the handle's stream does not block torch's: the copy below waits for nothing of the entry's
        assert np.array_equal(host(out), ref)
    finally:
        h.close()


def test_close_straight_after_an_asynchronous_call():
    c = entry_case(50, 3, 1, 8, 1, "gru")
    X, w, W, gXo, gA = rnn_inputs(c)
    h = rnn_handle(c)
    try:
        ref = rnn_dev(h, c, X, w, W, gXo, gA)
    finally:
        h.close()
    h = rnn_handle(c)
    Xd, wd, gd = dev(X), dev(w), dev(gXo)
    out, gX, gw = torch.full_like(Xd, np.nan), torch.full_like(Xd, np.nan), torch.full_like(wd, np.nan)
    gW = [torch.full(a.shape, np.nan, dtype=torch.float64, device="cuda") for a in W]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        keep = rnn_set_weights_dev(h, W, s.cuda_stream)
        h.resample_dev(s.cuda_stream, Xd.data_ptr(), wd.data_ptr(), c["T"], out.data_ptr())
        h.backward_dev(s.cuda_stream, Xd.data_ptr(), wd.data_ptr(), c["T"], gd.data_ptr(), 0, gX.data_ptr(),
                       gw.data_ptr(), [a.data_ptr() for a in gW], [a.numel() for a in gW])
    finally:
        h.close()
    s.synchronize()
    del keep
    none = rnn_handle(c)
    try:
        want = rnn_host(none, c, X, w, W, gXo, None)
    finally:
        none.close()
    assert np.array_equal(host(out), ref[0])
    assert same_bits([host(gX), host(gw)] + [host(a) for a in gW], want[3:])


# ====================================================================== 5. the arguments
def test_an_output_that_aliases_an_input_is_refused():
    c = entry_case(17, 3, 3, 5, 2, "gru")
    X, w, W, gXo, gA = rnn_inputs(c)
    h = rnn_handle(c)
    try:
        Xd, wd, gd = dev(X), dev(w), dev(gXo)
        out = torch.empty_like(Xd)
        with pytest.raises(ValueError, match="pf_rnn_set_weights has not been called"):
            h.resample_dev(0, Xd.data_ptr(), wd.data_ptr(), 1.0, out.data_ptr())
        keep = rnn_set_weights_dev(h, W)
        with pytest.raises(ValueError, match="aliases an input"):
            h.resample_dev(0, Xd.data_ptr(), wd.data_ptr(), 1.0, Xd.data_ptr())
        with pytest.raises(ValueError, match="aliases an input"):  # an overlap, not the same pointer
            h.resample_dev(0, Xd.data_ptr(), wd.data_ptr(), 1.0, Xd.data_ptr() + 8)
        gW = [torch.empty(a.shape, dtype=torch.float64, device="cuda") for a in W]
        gX, gw = torch.empty_like(Xd), torch.empty_like(wd)
        ptrs, sizes = [a.data_ptr() for a in gW], [a.numel() for a in gW]
        with pytest.raises(ValueError, match="aliases an input"):
            h.backward_dev(0, Xd.data_ptr(), wd.data_ptr(), 1.0, gd.data_ptr(), 0, gd.data_ptr(), gw.data_ptr(), ptrs,
                           sizes)
        with pytest.raises(ValueError, match="aliases an input"):
            h.backward_dev(0, Xd.data_ptr(), wd.data_ptr(), 1.0, gd.data_ptr(), 0, gX.data_ptr(), gw.data_ptr(),
                           [wd.data_ptr()] + ptrs[1:], sizes)
        # the host entries' messages
        with pytest.raises(ValueError, match=r"expected 8 gradient arrays \(3 per layer and 2 of the output layer\)"):
            h.backward_dev(0, Xd.data_ptr(), wd.data_ptr(), 1.0, gd.data_ptr(), 0, gX.data_ptr(), gw.data_ptr(),
                           ptrs[:-1], sizes[:-1])
        with pytest.raises(ValueError, match=f"gradient array 1 has {sizes[1] + 1} elements, expected {sizes[1]}"):
            h.backward_dev(0, Xd.data_ptr(), wd.data_ptr(), 1.0, gd.data_ptr(), 0, gX.data_ptr(), gw.data_ptr(), ptrs,
                           [sizes[0], sizes[1] + 1] + sizes[2:])
        Wp = [a.data_ptr() for a in keep]
        with pytest.raises(ValueError, match=r"expected 8 weight arrays \(3 per layer and 2 of the output layer\)"):
            h.set_weights_dev(0, Wp[:-1], sizes[:-1])
        with pytest.raises(ValueError, match=f"weight array 0 has {sizes[0] - 1} elements, expected {sizes[0]}"):
            h.set_weights_dev(0, Wp, [sizes[0] - 1] + sizes[1:])
        with pytest.raises(ValueError, match="weight array 2 is null"):
            h.set_weights_dev(0, Wp[:2] + [0] + Wp[3:], sizes)
        with pytest.raises(ValueError, match="temperature must be positive"):
            h.resample_dev(0, Xd.data_ptr(), wd.data_ptr(), 0.0, out.data_ptr())
        with pytest.raises(ValueError, match="null argument"):
            h.resample_dev(0, Xd.data_ptr(), wd.data_ptr(), 1.0, 0)
    finally:
        h.close()


def test_soft_arguments():
    N, d, B = 65, 1, 1
    X, lp, g = soft_inputs(N, d, B, seed=83)
    h = SO._Handle(N, d, B)
    try:
        Xd, lpd, gd = dev(X), dev(lp), dev(g)
        out, M, L = torch.empty_like(Xd), torch.empty_like(lpd), torch.empty_like(lpd)
        with pytest.raises(ValueError, match="aliases an input"):
            h.resample_dev(0, Xd.data_ptr(), lpd.data_ptr(), 0.2, 0, 0, 0, Xd.data_ptr())
        with pytest.raises(ValueError, match="aliases an input"):
            h.resample_dev(0, Xd.data_ptr(), lpd.data_ptr(), 0.2, 0, 0, 0, out.data_ptr(), 0, lpd.data_ptr(),
                           L.data_ptr())
        with pytest.raises(ValueError, match="given together"):
            h.resample_dev(0, Xd.data_ptr(), lpd.data_ptr(), 0.2, 0, 0, 0, out.data_ptr(), 0, M.data_ptr(), 0)
        with pytest.raises(ValueError, match="temperature must be positive"):
            h.resample_dev(0, Xd.data_ptr(), lpd.data_ptr(), -1.0, 0, 0, 0, out.data_ptr())
        with pytest.raises(ValueError, match="batch_base \\+ batch must be at most 16777216"):
            h.resample_dev(0, Xd.data_ptr(), lpd.data_ptr(), 0.2, 0, 0, 1 << 24, out.data_ptr())
        gX, glp = torch.empty_like(Xd), torch.empty_like(lpd)
        with pytest.raises(ValueError, match="X_out, row_max and row_sum must be given together or all be null"):
            h.backward_dev(0, Xd.data_ptr(), lpd.data_ptr(), 0.2, 0, 0, 0, out.data_ptr(), 0, 0, gd.data_ptr(),
                           gX.data_ptr(), glp.data_ptr())
        with pytest.raises(ValueError, match="aliases an input"):
            h.backward_dev(0, Xd.data_ptr(), lpd.data_ptr(), 0.2, 0, 0, 0, 0, 0, 0, gd.data_ptr(), gd.data_ptr(),
                           glp.data_ptr())
    finally:
        h.close()


# ====================================================================== 6. the LDS-poison hook
def test_the_new_paths_are_poisoned_and_do_not_read_uninitialised_lds(monkeypatch):
    monkeypatch.delenv("PF_TEST_LDS_POISON", raising=False)
    monkeypatch.delenv("PF_TEST_RNN_STREAM", raising=False)
    monkeypatch.delenv("PF_TEST_SOFT_SPLITS", raising=False)
    rnn_clean, _, _ = rnn_entry_pair(ENTRIES[1])
    soft_clean, _ = soft_pair(SOFT[3])
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_LDS_POISON", "1")
    count = NV.load().pf_test_lds_poison_count
    before = int(count())
    e = ENTRIES[1]
    c = entry_case(*e[:6])
    X, w, W, gXo, gA = rnn_inputs(c)
    h = rnn_handle(c)
    try:
        got = rnn_dev(h, c, X, w, W, gXo, gA)
    finally:
        h.close()
    mid = int(count())
    assert mid >= before + 2 + 4  # resample: recurrence and assignment; backward: those, bwd_assign, bwd_recur
    assert same_bits(got, rnn_clean)
    N, d, B, entropy, saved = SOFT[3]
    Xs, lp, g = soft_inputs(N, d, B, seed=80)
    h = SO._Handle(N, d, B)
    try:
        got = soft_dev(h, Xs, lp, g, 0.2, 2024, 3, 5, entropy, saved)
    finally:
        h.close()
    assert int(count()) >= mid + 2 + 1  # the pass and the entropy; the backward pass
    assert same_bits(got, soft_clean)
