"""RNN resampler and DifferentiableParticleFilterRNN on the device vs the NumPy restatement
(-m gpu, MI355X).

TensorFlow is not available, so there is no fixture of reference outputs: the device is compared
with tests/dpf_rnn_restatement.py, the reference's formulas and Keras' cell conventions in fp64,
which tests/test_dpf_rnn_host.py checks against the literal loop, against hand-evaluated scalar cases
and for conditioning (fp64 against long double: at most 3e-15 on these cases).

The recurrence kernel gives a workgroup 16 new particles, a wave 16 hidden units and an MFMA k-step
4 hidden units; R.PARITY lists what each size exercises and, as "res", whether the plan keeps the
weights in LDS or streams them on its own.  On the cases that are resident the streaming variant is
forced with PF_TEST_HOOKS=1 PF_TEST_RNN_STREAM=1, read when the handle is made.

Bounds (fp64 engine, the 1e-9 bound of the other fp64 filters): last hidden states and assignment
matrices within 1e-9, particles within 1e-9 max(1, max|X'_ref|), rows of A summing to 1 within
1e-12.  The device accumulates h W on the matrix cores in another order, folds the biases into the
initial accumulator, multiplies by 1 / T where NumPy divides, and uses the device library's exp and
tanh.

Largest errors measured on an MI355X: DESIGN.md section 4, "RNN resampling and
DifferentiableParticleFilterRNN".
"""

import ctypes as C
import os

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_rnn as RN
from tests import dpf_rnn_restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-9
ROWSUM = 1e-12


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert NV.device_count() > 0, "no HIP device visible: -m gpu tests must run on an MI355X"


def handle(c, B=None):
    return RN._Handle(c["N"], c["d"], c["B"] if B is None else B, c["H"], c["L"], c["cell"], c["uw"], c["up"])


def run(h, X, lw, T):
    X = np.ascontiguousarray(X, dtype=float)
    return h.resample(X, np.ascontiguousarray(np.exp(lw)), T, want_hidden=True)


def forced():
    """Is the streaming hook set (PF_TEST_HOOKS=1 PF_TEST_RNN_STREAM=1, read when a handle is made)?"""
    return os.environ.get("PF_TEST_HOOKS") == "1" and os.environ.get("PF_TEST_RNN_STREAM") == "1"


def device(c, X, lw, W):
    """(X_out, A, hid), batched, of one pf_rnn_resample call on a fresh handle, which must have the
    residency the case names unless the hook forces streaming."""
    h = handle(c, np.shape(X)[0])
    try:
        assert h.resident == (c["res"] and not forced())
        h.set_weights(W)
        return run(h, X, lw, c["T"])
    finally:
        h.close()


def compare(tag, out, A, hid, ref):
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(A)) and np.all(np.isfinite(hid))
    sx = max(1.0, float(np.max(np.abs(ref["particles"]))))
    ex = float(np.max(np.abs(out - ref["particles"])))
    ea = float(np.max(np.abs(A - ref["A"])))
    eh = float(np.max(np.abs(hid - ref["hid"])))
    es = float(np.max(np.abs(np.sum(A, axis=-1) - 1.0)))
    print(f"rnn {tag}: hid error {eh:.3e}, A error {ea:.3e}, particle error {ex:.3e} (scale {sx:.3g}), "
          f"row sums off by {es:.3e}")
    assert eh <= TOL and ea <= TOL
    assert ex <= TOL * sx
    assert es <= ROWSUM


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("c", R.PARITY, ids=lambda c: R.case_id(c))
def test_parity(c):
    X, lw, W, ref = R.solved(c)
    kw = dict(use_weight_features=c["uw"], use_particle_features=c["up"], return_hidden=True)
    if c["B"] == 1:  # the unbatched form of the module function
        out, A, hid = RN.rnn_resample(X[0], lw[0], W, c["cell"], c["T"], **kw)
        assert out.shape == (c["N"], c["d"]) and A.shape == (c["N"], c["N"]) and hid.shape == (c["N"], c["H"])
        out, A, hid = out[None], A[None], hid[None]
    else:
        out, A, hid = RN.rnn_resample(X, lw, W, c["cell"], c["T"], **kw)
    assert out.dtype == np.float64 and out.shape == X.shape
    for b in range(c["B"]):
        compare(f"{R.case_id(c)} problem {b}", out[b], A[b], hid[b], ref[b])
    two = RN.rnn_resample(X, lw, W, c["cell"], c["T"], use_weight_features=c["uw"], use_particle_features=c["up"])
    assert len(two) == 2 and np.array_equal(two[0], out) and np.array_equal(two[1], A)


@pytest.mark.parametrize("c", R.PARITY, ids=lambda c: R.case_id(c))
def test_the_handle_has_the_residency_the_case_names(c, monkeypatch):
    """rnn_resample does not show which variant ran: with no hook set the library's plan must be the one
    tests/test_dpf_rnn_host.py reads from make_plan."""
    monkeypatch.delenv("PF_TEST_HOOKS", raising=False)
    monkeypatch.delenv("PF_TEST_RNN_STREAM", raising=False)
    h = handle(c)
    try:
        assert h.resident == c["res"]
    finally:
        h.close()


# ------------------------------------------------------------------ 2. forced streaming
# the resident cases with two layers or more, four unit tiles (H = 64) and three (H = 48, 192 lanes); a case
# that streams anyway is not forced
STREAMED = [c for c in R.PARITY if c["res"] and c["L"] >= 2] + \
    [next(c for c in R.PARITY if c["H"] == H and c["L"] == 1) for H in (64, 48)]


@pytest.mark.parametrize("c", STREAMED, ids=lambda c: R.case_id(c))
def test_forced_streaming(c, monkeypatch):
    X, lw, W, ref = R.solved(c)
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_RNN_STREAM", "1")
    out, A, hid = device(c, X, lw, W)
    for b in range(c["B"]):
        compare(f"{R.case_id(c)} streamed problem {b}", out[b], A[b], hid[b], ref[b])


def test_the_stream_hook_needs_the_master_switch(monkeypatch):
    monkeypatch.delenv("PF_TEST_HOOKS", raising=False)
    monkeypatch.setenv("PF_TEST_RNN_STREAM", "1")
    h = handle(R.PARITY[1])
    try:
        assert h.resident
    finally:
        h.close()


# ------------------------------------------------------------------ 3. bitwise properties
BATCH = next(c for c in R.PARITY if c["B"] == 3)
BATCH_STREAMED = next(c for c in R.PARITY if c["B"] == 2 and not c["res"])  # H = 64, two layers: streams on its own


@pytest.mark.parametrize("c", [BATCH, BATCH_STREAMED], ids=lambda c: R.case_id(c))
def test_repeated_calls_are_bitwise_equal_and_a_batch_is_the_problems_alone(c):
    X, lw, W, ref = R.solved(c)
    first = device(c, X, lw, W)
    again = device(c, X, lw, W)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    for b in range(c["B"]):
        alone = device(c, X[b:b + 1], lw[b:b + 1], W)
        assert all(np.array_equal(a[0], f[b]) for a, f in zip(alone, first)), f"problem {b}"
    assert not np.array_equal(first[1][0], first[1][1])


REUSED = [next(c for c in R.PARITY if c["N"] == 35),  # two layers, three tiles of rows
          next(c for c in R.PARITY if c["H"] == 100)]  # seven unit tiles: a fragment buffer rewritten in full


@pytest.mark.parametrize("c", REUSED, ids=lambda c: R.case_id(c))
def test_a_handle_reused_after_other_weights_gives_the_same_bits(c):
    X, lw, W, ref = R.solved(c)
    W2 = R.make_weights(np.random.default_rng(99), c["N"], c["d"], c["H"], c["L"], c["cell"], c["uw"], c["up"])
    h = handle(c)
    try:
        h.set_weights(W)
        a = run(h, X, lw, c["T"])
        a2 = run(h, X, lw, c["T"])
        h.set_weights(W2)
        other = run(h, X, lw, c["T"])
        h.set_weights(W)
        back = run(h, X, lw, c["T"])
    finally:
        h.close()
    assert all(np.array_equal(x, y) for x, y in zip(a, a2)) and all(np.array_equal(x, y) for x, y in zip(a, back))
    assert not np.array_equal(a[1], other[1])
    ref2 = R.resample(X[0], lw[0], W2, c["cell"], c["T"], c["uw"], c["up"])
    compare(f"{R.case_id(c)} second weights", other[0][0], other[1][0], other[2][0], ref2)
    fresh = device(c, X, lw, W)
    assert all(np.array_equal(x, y) for x, y in zip(a, fresh))


# ------------------------------------------------------------------ 4. the baseline resampler
# N = 300: two trips of the 256 lanes over j, five waves' worth of j in A X, and with d = 5 two trips over c
@pytest.mark.parametrize("N,d,T", [(3, 2, 1.0), (65, 3, 0.5), (300, 5, 0.5)])
def test_baseline_matches_the_restatement_on_the_soft_resamplers_draws(N, d, T):
    B, seed, epoch, base = 2, 0x1234567890ABCDEF, 3, 7
    rng = np.random.default_rng([N, d])
    X = rng.standard_normal((B, N, d))
    lw = R.log_normalize(1.5 * rng.standard_normal((B, N)))
    h = RN._Handle(N, d, B, 4, 1, "lstm")
    try:
        out, A = h.baseline(np.ascontiguousarray(X), RN._baseline_log_probs(lw, T), seed, epoch, base)
        out2, A2 = h.baseline(np.ascontiguousarray(X), RN._baseline_log_probs(lw, T), seed, epoch, base)
        other, _ = h.baseline(np.ascontiguousarray(X), RN._baseline_log_probs(lw, T), seed, epoch + 1, base)
    finally:
        h.close()
    assert np.array_equal(out, out2) and np.array_equal(A, A2) and not np.array_equal(out, other)
    for b in range(B):
        ref = R.baseline(X[b], lw[b], T, seed, epoch, base + b)
        sx = max(1.0, float(np.max(np.abs(ref["particles"]))))
        ea = float(np.max(np.abs(A[b] - ref["A"])))
        ex = float(np.max(np.abs(out[b] - ref["particles"])))
        es = float(np.max(np.abs(np.sum(A[b], axis=-1) - 1.0)))
        print(f"rnn baseline N={N} problem {b}: A error {ea:.3e}, particle error {ex:.3e} (scale {sx:.3g}), "
              f"row sums off by {es:.3e}")
        assert ea <= TOL and ex <= TOL * sx and es <= ROWSUM
    # the draws are the ones pf_soft_draws reports
    from particle_filters_amd import dpf_soft as SO
    hs = SO._Handle(N, 1, 1)
    try:
        _, G = hs.draws(seed, epoch, base)
    finally:
        hs.close()
    lp = R.baseline(X[0], lw[0], T, seed, epoch, base)["lp"]
    z = lp[None, :] + 0.1 * G[0]
    e = np.exp(z - z.max(-1, keepdims=True))
    assert np.max(np.abs(A[0] - e / e.sum(-1, keepdims=True))) <= TOL


def test_baseline_filter_advances_the_epoch_and_needs_no_network():
    N, d, B = 20, 1, 2
    f = RN.DifferentiableParticleFilterRNN(N, d, *R.lgssm(3), temperature=0.5, use_baseline_resampling=True, seed=11,
                                           rng=np.random.default_rng(1))
    try:
        p0, lw0 = f.init_particles(B, np.zeros(d), np.eye(d))
        y = np.array([[0.3], [-0.2]])
        tr, ll = R.lgssm(3)
        pred = tr(p0, {})
        lw = R.log_normalize(lw0 + ll(pred, y, {}))
        new, nlw, A = f.step(p0, lw0, y)
        assert f.epoch == 1 and A.shape == (B, N, N) and np.array_equal(nlw, np.log(np.full((B, N), 1.0 / N)))
        for b in range(B):
            ref = R.baseline(pred[b], lw[b], 0.5, 11, 0, b)
            assert np.max(np.abs(A[b] - ref["A"])) <= TOL
            assert np.max(np.abs(new[b] - ref["particles"])) <= TOL * max(1.0, float(np.max(np.abs(ref["particles"]))))
        f.step(new, nlw, y)
        assert f.epoch == 2
        with pytest.raises(ValueError):
            f.step(np.full((B, N, d), np.nan), nlw, y)
        assert f.epoch == 2
    finally:
        f.close()


# ------------------------------------------------------------------ 5. the class, end to end
def test_filter_matches_the_restatements_filter_and_has_the_reference_tests_properties():
    B, T, N, d, H = 2, 5, 20, 1, 8
    W = R.make_weights(np.random.default_rng(5), N, d, H, 1, "lstm")
    obs = np.random.default_rng(4).standard_normal((B, T, d))
    f = RN.DifferentiableParticleFilterRNN(N, d, *R.lgssm(8), rnn_type="lstm", rnn_hidden_dim=H, weights=W,
                                           rng=np.random.default_rng(2))
    try:
        ps, lws, As, st = f.filter(obs, np.zeros(d), np.eye(d), return_ess=True)
        first = f._h
        assert first is not None and first.key()[:3] == (N, d, B)
        f.rng = np.random.default_rng(3)
        other, _, _ = f.filter(obs, np.zeros(d), np.eye(d))
        assert f._h is first
    finally:
        f.close()
    pr, lwr, Ar = R.filter(obs, np.zeros(d), np.eye(d), *R.lgssm(8), N, d, W, "lstm", np.random.default_rng(2))
    assert ps.shape == (B, T + 1, N, d) and lws.shape == (B, T + 1, N) and As.shape == (B, T, N, N)
    assert ps.dtype == np.float64 and np.all(np.isfinite(ps)) and np.all(np.isfinite(As))
    assert np.array_equal(ps[:, 0], pr[:, 0]) and np.array_equal(lws, lwr)
    for t in range(T):
        scale = max(1.0, float(np.max(np.abs(pr[:, t + 1]))))
        ex = float(np.max(np.abs(ps[:, t + 1] - pr[:, t + 1])))
        ea = float(np.max(np.abs(As[:, t] - Ar[:, t])))
        print(f"rnn filter step {t + 1}: particle error {ex:.3e} (scale {scale:.3g}), A error {ea:.3e}")
        assert ex <= TOL * scale and ea <= TOL
    assert np.max(np.abs(st["ess_after_resampling"] - N)) <= 1e-9 * N
    assert np.all(st["ess_before_resampling"] <= N * (1 + 1e-12)) and np.all(st["ess_before_resampling"] >= 1 - 1e-12)
    assert not np.array_equal(other[:, 0], ps[:, 0])  # another seed, another prior draw
    assert f.epoch == 0


def test_default_initialised_filter_runs_and_its_rows_are_nearly_uniform():
    N, d = 30, 1
    f = RN.DifferentiableParticleFilterRNN(N, d, *R.lgssm(8), rnn_hidden_dim=32, rng=np.random.default_rng(0))
    try:
        p0, lw0 = f.init_particles(1, np.zeros(d), np.eye(d))
        new, nlw, A = f.step(p0, lw0, np.zeros((1, d)))
    finally:
        f.close()
    assert np.all(np.isfinite(new)) and np.max(np.abs(A - 1.0 / N)) < 1e-3  # rnn.py:155-162: a 0.001 output kernel


# ------------------------------------------------------------------ 6. ABI errors
def _create(**kw):
    o = dict(n_particles=10, dim=2, batch=1, hidden=8, layers=1, cell=0, use_weight=1, use_particle=1, device=0)
    o.update(kw)
    h = C.c_void_p()
    return NV.load().pf_rnn_create(C.byref(NV.RnnOpts(**o)), C.byref(h)), h


def test_create_limits():
    lib = NV.load()
    for kw in (dict(n_particles=0), dict(dim=0), dict(dim=1025), dict(hidden=0), dict(hidden=129), dict(layers=0),
               dict(layers=5), dict(batch=0), dict(batch=65536), dict(cell=2), dict(use_weight=0, use_particle=0),
               dict(n_particles=16385), dict(n_particles=8192, batch=5)):
        st, h = _create(**kw)
        assert st == NV.PF_E_ARG and not h.value, kw
    for kw in (dict(hidden=128, layers=4, cell=1), dict(dim=1024, use_weight=0), dict(n_particles=1, hidden=1)):
        st, h = _create(**kw)
        assert st == NV.PF_OK and h.value, kw
        lib.pf_rnn_destroy(h)


def test_argument_errors_that_need_a_handle():
    lib = NV.load()
    c = R.PARITY[1]
    X, lw, W, ref = R.solved(c)
    h = handle(c)
    try:
        N, d = c["N"], c["d"]
        x, w, out = np.ascontiguousarray(X), np.ascontiguousarray(np.exp(lw)), np.zeros((1, N, d))
        assert lib.pf_rnn_resample(h.h, NV.dptr(x), NV.dptr(w), 1.0, NV.dptr(out), None, None) == NV.PF_E_ARG
        assert b"set_weights" in lib.pf_last_error()
        with pytest.raises(ValueError):
            h.set_weights(W[:-1])
        bad = list(W)
        bad[0] = np.zeros((W[0].shape[0] + 1, W[0].shape[1]))
        with pytest.raises(ValueError):
            h.set_weights(bad)
        assert lib.pf_rnn_set_weights(h.h, None, None, 3 * c["L"] + 2) == NV.PF_E_ARG
        h.set_weights(W)
        for T in (0.0, -1.0, float("inf"), float("nan")):
            assert lib.pf_rnn_resample(h.h, NV.dptr(x), NV.dptr(w), T, NV.dptr(out), None, None) == NV.PF_E_ARG
        assert lib.pf_rnn_resample(h.h, None, NV.dptr(w), 1.0, NV.dptr(out), None, None) == NV.PF_E_ARG
        assert lib.pf_rnn_resample(h.h, NV.dptr(x), None, 1.0, NV.dptr(out), None, None) == NV.PF_E_ARG
        assert lib.pf_rnn_resample(h.h, NV.dptr(x), NV.dptr(w), 1.0, None, None, None) == NV.PF_E_ARG
        assert lib.pf_rnn_resample(h.h, NV.dptr(x), NV.dptr(w), 1.0, NV.dptr(out), None, None) == NV.PF_OK
        assert np.max(np.abs(out[0] - ref[0]["particles"])) <= TOL * max(1.0, float(np.max(np.abs(ref[0]["particles"]))))
        assert lib.pf_rnn_baseline(h.h, None, NV.dptr(w), 0, 0, 0, NV.dptr(out), None) == NV.PF_E_ARG
        assert lib.pf_rnn_baseline(h.h, NV.dptr(x), None, 0, 0, 0, NV.dptr(out), None) == NV.PF_E_ARG
        assert lib.pf_rnn_baseline(h.h, NV.dptr(x), NV.dptr(w), 0, 0, 0, None, None) == NV.PF_E_ARG
        assert lib.pf_rnn_baseline(h.h, NV.dptr(x), NV.dptr(w), 0, 0, 1 << 24, NV.dptr(out), None) == NV.PF_E_ARG
        assert lib.pf_rnn_baseline(h.h, NV.dptr(x), NV.dptr(np.log(w)), 0, 0, 0, NV.dptr(out), None) == NV.PF_OK
        assert lib.pf_rnn_stream(h.h) and lib.pf_rnn_synchronize(h.h) == NV.PF_OK
    finally:
        h.close()
