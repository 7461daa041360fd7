"""CPU checks of the RNN resampler: the restatement against itself, the conditioning of the parity
cases, the Python class, and the shape plan (no GPU).

tests/dpf_rnn_restatement.py is what tests/test_gpu_dpf_rnn.py compares the device with.  Here

* its vectorised form is checked against the literal transliteration of rnn.py:289-347;
* the Keras cell conventions are pinned by scalar cases (H = 1, N = 2) evaluated with ``math`` from
  the formulas, every gate with its own weight so that a swapped gate order cannot pass;
* every parity case is shown to be well conditioned (fp64 against ``np.longdouble``) and sensitive:
  to the one-hot rows of layer 0's kernel, to the first old particle (the earliest timestep), and
  with rows of A that differ - so a kernel that drops any of these cannot pass parity;
* the class ``DifferentiableParticleFilterRNN`` is exercised with the device resampler swapped for
  the restatement.
"""

import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_rnn as RN
from tests import dpf_rnn_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [R.case_id(c) for c in R.PARITY]


def _scaled(a, ref):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(ref, dtype=np.float64)))) / \
        max(1.0, float(np.max(np.abs(np.asarray(ref, dtype=np.float64)))))


# ------------------------------------------------------------------ 1. vectorised vs literal
@pytest.mark.parametrize("c", R.PARITY, ids=IDS)  # the longest, N = 260, is 67600 cell calls: under a second
def test_vectorised_restatement_equals_the_literal_loop(c):
    X, lw, W, ref = R.solved(c)
    for b in range(c["B"]):
        lit = R.literal_resample(X[b], lw[b], W, c["cell"], c["T"], c["uw"], c["up"])
        ea = float(np.max(np.abs(ref[b]["A"] - lit["A"])))
        eh = float(np.max(np.abs(ref[b]["hid"] - lit["hid"])))
        ex = _scaled(ref[b]["particles"], lit["particles"])
        print(f"rnn {R.case_id(c)} problem {b}: vectorised - literal A {ea:.3e} hid {eh:.3e} X' {ex:.3e}")
        assert ea <= 1e-13 and eh <= 1e-13 and ex <= 1e-13


# ------------------------------------------------------------------ 2. cell conventions by hand
def _sig(x):
    return 1.0 / (1.0 + math.exp(-x))


def test_lstm_gate_order_and_update_against_scalar_arithmetic():
    # H = 1, N = 2, d = 1: inputs [w_j, x_j, onehot(i)]; kernel (4, 4), columns i, f, c, o
    K = np.array([[0.3, -0.5, 0.7, 0.2], [-0.4, 0.6, 0.1, -0.8], [0.9, -0.2, 0.5, 0.3], [-0.6, 0.4, -0.7, 0.1]])
    Rk = np.array([[0.25, -0.35, 0.45, 0.55]])
    b = np.array([0.05, 1.0, -0.1, 0.15])
    Kd, bd = np.array([[1.5, -0.5]]), np.array([0.1, -0.2])
    X, w = np.array([[0.8], [-1.2]]), np.array([0.3, 0.7])
    hid = np.zeros((2, 1))
    for i in range(2):
        h = c = 0.0
        for t in range(2):
            x = [w[t], X[t, 0], 1.0 if i == 0 else 0.0, 1.0 if i == 1 else 0.0]
            z = [sum(x[k] * K[k, g] for k in range(4)) + h * Rk[0, g] + b[g] for g in range(4)]
            c = _sig(z[1]) * c + _sig(z[0]) * math.tanh(z[2])
            h = _sig(z[3]) * math.tanh(c)
        hid[i, 0] = h
    got = R.resample(X, np.log(w), [K, Rk, b, Kd, bd], "lstm", T=0.5)
    assert np.max(np.abs(got["hid"] - hid)) <= 1e-15
    logits = (hid @ Kd + bd) / 0.5
    A = np.exp(logits) / np.sum(np.exp(logits), axis=-1, keepdims=True)
    assert np.max(np.abs(got["A"] - A)) <= 1e-15 and np.max(np.abs(got["particles"] - A @ X)) <= 1e-15
    # a swapped pair of gates is another function
    Ks = K[:, [1, 0, 2, 3]]
    assert np.max(np.abs(R.resample(X, np.log(w), [Ks, Rk, b, Kd, bd], "lstm", T=0.5)["hid"] - hid)) > 1e-3


def test_gru_reset_after_with_both_biases_against_scalar_arithmetic():
    # H = 1, N = 2, d = 1: kernel (4, 3), columns z, r, h; bias (2, 3): input bias and recurrent bias
    K = np.array([[0.3, -0.5, 0.7], [-0.4, 0.6, 0.1], [0.9, -0.2, 0.5], [-0.6, 0.4, -0.7]])
    Rk = np.array([[0.25, -0.35, 0.45]])
    b = np.array([[0.05, -0.3, 0.2], [0.4, 0.1, -0.6]])
    Kd, bd = np.array([[1.5, -0.5]]), np.array([0.1, -0.2])
    X, w = np.array([[0.8], [-1.2]]), np.array([0.3, 0.7])
    hid = np.zeros((2, 1))
    for i in range(2):
        h = 0.0
        for t in range(2):
            x = [w[t], X[t, 0], 1.0 if i == 0 else 0.0, 1.0 if i == 1 else 0.0]
            xm = [sum(x[k] * K[k, g] for k in range(4)) + b[0, g] for g in range(3)]
            hm = [h * Rk[0, g] + b[1, g] for g in range(3)]
            z, r = _sig(xm[0] + hm[0]), _sig(xm[1] + hm[1])
            hh = math.tanh(xm[2] + r * hm[2])  # reset_after: r multiplies the recurrent half, bias included
            h = z * h + (1.0 - z) * hh
        hid[i, 0] = h
    got = R.resample(X, np.log(w), [K, Rk, b, Kd, bd], "gru")
    assert np.max(np.abs(got["hid"] - hid)) <= 1e-15
    # the recurrent bias of the h gate is inside the reset product: moving it to the input bias differs
    b2 = b.copy()
    b2[0, 2] += b2[1, 2]
    b2[1, 2] = 0.0
    assert np.max(np.abs(R.resample(X, np.log(w), [K, Rk, b2, Kd, bd], "gru")["hid"] - hid)) > 1e-3


# ------------------------------------------------------------------ 3. conditioning of the parity cases
@pytest.mark.parametrize("c", R.PARITY, ids=IDS)
def test_parity_case_is_well_conditioned(c):
    X, lw, W, ref = R.solved(c)
    for b in range(c["B"]):
        hi = R.resample(X[b], lw[b], W, c["cell"], c["T"], c["uw"], c["up"], dtype=np.longdouble)
        ea = float(np.max(np.abs(ref[b]["A"] - hi["A"])))
        eh = float(np.max(np.abs(ref[b]["hid"] - hi["hid"])))
        ex = _scaled(ref[b]["particles"], hi["particles"])
        print(f"rnn {R.case_id(c)} problem {b}: fp64 - longdouble A {ea:.3e} hid {eh:.3e} X' {ex:.3e}")
        assert np.all(np.isfinite(ref[b]["A"])) and np.all(np.isfinite(ref[b]["hid"]))
        assert np.all(np.isfinite(ref[b]["particles"]))
        assert ea <= 1e-12 and eh <= 1e-12 and ex <= 1e-12
        assert np.max(np.abs(np.sum(ref[b]["A"], axis=-1) - 1.0)) <= 1e-12


@pytest.mark.parametrize("c", [c for c in R.PARITY if c["N"] >= 2], ids=lambda c: R.case_id(c))
def test_parity_case_is_sensitive_to_what_a_kernel_could_drop(c):
    """N = 1 has A = [[1]] whatever the network computes and is left out."""
    X, lw, W, ref = R.solved(c)
    N, F0 = c["N"], R.feature_dim(c["d"], c["uw"], c["up"])
    args = (c["cell"], c["T"], c["uw"], c["up"])
    for b in range(c["B"]):
        A = ref[b]["A"]
        # the one-hot rows of layer 0's kernel
        W0 = [a.copy() for a in W]
        W0[0][F0:] = 0.0
        d_onehot = float(np.max(np.abs(R.resample(X[b], lw[b], W0, *args)["A"] - A)))
        # the first old particle: the earliest timestep of every sequence
        Xm, lwm = X[b].copy(), lw[b].copy()
        Xm[0] += 1.0
        lwm[0] = np.log(np.exp(lwm[0]) + 0.25)
        d_first = float(np.max(np.abs(R.resample(Xm, lwm, W, *args)["A"] - A)))
        # a particle in the middle of every sequence, moved by 1 (its weight where the weight is the only
        # feature; in the saturated case that particle is one of the two of magnitude 1e6, which a step of 1
        # cannot move out of saturation: there its sign is flipped)
        Xm, lwm = X[b].copy(), lw[b].copy()
        if c["kind"] == "big":
            Xm[N // 2] = -Xm[N // 2]
        else:
            Xm[N // 2] += 1.0
        if not c["up"]:
            lwm[N // 2] = np.log(np.exp(lwm[N // 2]) + 0.25)
        d_mid = float(np.max(np.abs(R.resample(Xm, lwm, W, *args)["A"] - A)))
        gaps = [float(np.max(np.abs(A[i] - A[j]))) for i in range(N) for j in range(i)]
        print(f"rnn {R.case_id(c)} problem {b}: one-hot rows zeroed {d_onehot:.3e}, particle 0 moved {d_first:.3e}, "
              f"particle {N // 2} moved {d_mid:.3e}, smallest row gap {min(gaps):.3e}")
        assert d_onehot > 1e-3
        assert d_first > 1e-7  # also over the 260 steps of the longest case: a GRU chosen for that
        assert d_mid > 1e-7
        assert min(gaps) > 1e-4


def _plan_program(*args):
    """Run tests/host/pf_rnn_plan_host_check.cpp (built with ASan + UBSan) and return the finished process."""
    exe = os.path.join(REPO, "build", "pf_rnn_plan_host_check")
    if not os.path.exists(exe):  # built by __graft_entry__.build(); here if the test runs first
        subprocess.run(["make", "-C", os.path.join(REPO, "particle_filters_amd", "csrc"), "hostcheck"],
                       check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return r


PLAN_FIELDS = ("HT", "KS", "RS", "threads", "tiles", "resident", "lds_bytes", "frag_doubles")


def plan_of(c):
    """make_plan's answer for a case, from the stand-alone program."""
    words = _plan_program(c["N"], c["d"], c["H"], c["L"], c["cell"]).stdout.split()
    assert len(words) == len(PLAN_FIELDS), words
    return dict(zip(PLAN_FIELDS, (int(w) for w in words)))


def test_parity_cases_cover_what_the_kernels_branch_on():
    """What a size exercises is asked of make_plan, not read off a list of sizes: 24, 28 and 32 hidden
    units are all two unit tiles."""
    plans = [(c, plan_of(c)) for c in R.PARITY]
    for c, p in plans:
        assert p["HT"] == -(-c["H"] // 16) and p["threads"] == 64 * p["HT"] * p["RS"] and p["tiles"] == -(-c["N"] // 16)
        assert bool(p["resident"]) == c["res"], R.case_id(c)
    # the unit tiles: every workgroup shape there is, with the weights in LDS where a plan can have them
    # there (from five tiles on every plan streams) and streamed because the plan says so
    assert {p["HT"] for _, p in plans} == set(range(1, 9))
    assert {p["HT"] for _, p in plans if p["resident"]} == {1, 2, 3, 4}
    unforced = {p["HT"] for _, p in plans if not p["resident"]}
    assert {3, 4, 5, 7, 8} <= unforced and unforced & {1, 2}
    assert {c["cell"] for c, p in plans if p["HT"] == 8} == {"lstm", "gru"}  # 512 lanes in both cells' instances
    assert {c["L"] for c, _ in plans} == {1, 2, 3, 4}
    assert {bool(p["resident"]) for c, p in plans if c["L"] == 4} == {True, False}
    assert {p["KS"] % 4 for _, p in plans} == {0, 1, 2, 3} and any(c["H"] % 16 == 1 for c, _ in plans)
    # the constants mirror the kernels' (pf_rnn_kernels.h, pf_rnn_plan.h): PB = 256 lanes of k_rnn_project and
    # k_rnn_assign, PB / 64 = 4 waves sharing the coordinates of A X, RT = 16 rows of a workgroup of k_rnn_recur
    PB, WAVES, RT = 256, 4, 16
    blocks = {(-(-4 * 16 * p["HT"] // PB), 4 * 16 * p["HT"] % PB == 0) for _, p in plans}  # of 4 Hp columns
    assert any(n == 1 for n, _ in blocks) and (2, False) in blocks and (2, True) in blocks
    assert any(-(-c["N"] // PB) >= 2 for c, _ in plans) and any(p["tiles"] >= 17 for _, p in plans)
    assert any(-(-c["N"] // RT) == p["tiles"] and c["N"] % RT for c, p in plans)
    assert any(-(-c["d"] // WAVES) >= 3 and c["d"] % WAVES for c, _ in plans)

    Ns, Hs, Ls = {c["N"] for c in R.PARITY}, {c["H"] for c in R.PARITY}, {c["L"] for c in R.PARITY}
    assert {1, 3, 16, 17, 33, 30, 35} <= Ns and {1, 5, 16, 24, 64} <= Hs and {1, 2, 3} <= Ls
    assert {c["d"] for c in R.PARITY} >= {1, 2, 5} and {c["cell"] for c in R.PARITY} == {"lstm", "gru"}
    assert any(c["N"] == 30 and c["H"] == 32 and c["L"] == 1 and c["cell"] == "lstm" for c in R.PARITY)
    assert any(c["N"] == 35 and c["H"] == 28 and c["L"] == 2 and c["cell"] == "gru" for c in R.PARITY)
    assert any(not c["uw"] for c in R.PARITY) and any(not c["up"] for c in R.PARITY)
    assert any(c["B"] == 3 for c in R.PARITY) and any(c["T"] == 0.1 for c in R.PARITY)
    assert any(c["H"] % 4 for c in R.PARITY)
    X, lw, _, _ = R.solved(next(c for c in R.PARITY if c["kind"] == "neginf"))
    assert np.any(np.isneginf(lw))
    X, lw, _, _ = R.solved(next(c for c in R.PARITY if c["kind"] == "big"))
    assert np.max(np.abs(X)) > 1e5


# ------------------------------------------------------------------ 4. the class and the module
def _model():
    return R.lgssm(3)


def test_importing_the_module_does_not_load_the_library():
    code = ("import particle_filters_amd.dpf_rnn as m, particle_filters_amd._native as nv; "
            "assert nv._lib is None; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_constructor_errors():
    tr, ll = _model()
    with pytest.raises(ValueError, match="Unknown RNN type"):
        RN.DifferentiableParticleFilterRNN(5, 1, tr, ll, rnn_type="rnn")
    with pytest.raises(ValueError, match="at least one"):
        RN.DifferentiableParticleFilterRNN(5, 1, tr, ll, use_weight_features=False, use_particle_features=False)
    with pytest.raises(ValueError):
        RN.DifferentiableParticleFilterRNN(5, 1, tr, ll, rnn_hidden_dim=129)
    with pytest.raises(ValueError):
        RN.DifferentiableParticleFilterRNN(5, 1, tr, ll, rnn_num_layers=5)
    with pytest.raises(ValueError):
        RN.DifferentiableParticleFilterRNN(0, 1, tr, ll)
    with pytest.raises(ValueError):
        RN.rnn_resample(np.zeros((3, 1)), np.zeros(3), [np.zeros((5, 4))] * 5, rnn_type="elman")
    f = RN.DifferentiableParticleFilterRNN(5, 1, tr, ll, rnn_type="GRU", name="x")
    assert f.rnn_type == "gru" and f.name == "x" and f.temperature == 1.0 and f.rnn_hidden_dim == 64
    assert f.rnn_num_layers == 1 and f.use_weight_features and f.use_particle_features
    assert not f.use_baseline_resampling and f.epoch == 0 and f._h is None
    base = RN.DifferentiableParticleFilterRNN(5, 1, tr, ll, use_baseline_resampling=True)
    assert base.get_weights() == []
    with pytest.raises(ValueError):
        base.set_weights([])


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("uw,up", [(True, True), (True, False), (False, True)])
def test_get_weights_shapes_and_default_initialisation(cell, L, uw, up):
    tr, ll = _model()
    N, d, H = 7, 3, 6
    f = RN.DifferentiableParticleFilterRNN(N, d, tr, ll, rnn_type=cell, rnn_hidden_dim=H, rnn_num_layers=L,
                                           use_weight_features=uw, use_particle_features=up,
                                           rng=np.random.default_rng(1))
    W = f.get_weights()
    G, F0 = R.GATES[cell], R.feature_dim(d, uw, up)
    assert len(W) == 3 * L + 2
    for l in range(L):
        K, Rk, b = W[3 * l:3 * l + 3]
        assert K.shape == ((F0 + N) if l == 0 else H, G * H) and Rk.shape == (H, G * H)
        lim = np.sqrt(6.0 / (K.shape[0] + K.shape[1]))
        assert np.max(np.abs(K)) <= lim and np.std(K) > 0.3 * lim
        assert np.max(np.abs(Rk @ Rk.T - np.eye(H))) <= 1e-12  # orthogonal: (H, G H) with orthonormal rows
        if cell == "lstm":
            assert b.shape == (4 * H,) and np.array_equal(b, np.r_[np.zeros(H), np.ones(H), np.zeros(2 * H)])
        else:
            assert b.shape == (2, 3 * H) and not np.any(b)
    assert W[-2].shape == (H, N) and W[-1].shape == (N,) and not np.any(W[-1])
    assert 0.0 < np.max(np.abs(W[-2])) < 0.01
    # set_weights: a round trip, and wrong shapes
    f.set_weights(W)
    assert all(np.array_equal(a, b) for a, b in zip(f.get_weights(), W))
    W[0][0, 0] = 5.0
    assert f.get_weights()[0][0, 0] != 5.0  # copies
    with pytest.raises(ValueError):
        f.set_weights(W[:-1])
    for k in range(len(W)):
        bad = [a.copy() for a in W]
        bad[k] = np.zeros(tuple(s + 1 for s in bad[k].shape))
        with pytest.raises(ValueError):
            f.set_weights(bad)
    bad = [a.copy() for a in W]
    bad[1][0, 0] = np.nan
    with pytest.raises(ValueError):
        f.set_weights(bad)
    assert f._h is None  # nothing above touched the device


def test_compute_rnn_features_and_utilities():
    tr, ll = _model()
    N, d, B = 4, 2, 3
    rng = np.random.default_rng(0)
    P, lw = rng.standard_normal((B, N, d)), np.log(np.full((B, N), 0.25))
    for uw, up in ((True, True), (True, False), (False, True)):
        f = RN.DifferentiableParticleFilterRNN(N, d, tr, ll, rnn_hidden_dim=4, use_weight_features=uw,
                                               use_particle_features=up, rng=rng)
        F0 = R.feature_dim(d, uw, up)
        feat = f._compute_rnn_features(P, lw, target_particle_idx=2)
        assert feat.shape == (B, N, F0 + N) and f._compute_rnn_features(P, lw).shape == (B, N, F0)
        assert np.array_equal(feat[..., F0:], np.broadcast_to(np.eye(N)[2], (B, N, N)))
        if uw:
            assert np.allclose(feat[..., 0], 0.25)
        if up:
            assert np.array_equal(feat[..., F0 - d:F0], P)
    cls = RN.DifferentiableParticleFilterRNN
    w = np.array([[0.5, 0.5, 0.0, 0.0]])
    with np.errstate(divide="ignore"):
        assert abs(cls.compute_ess(np.log(w))[0] - 2.0) <= 1e-15
        # clipped to [1e-10, 1]: the zero weights contribute -1e-10 log 1e-10 each (rnn.py:419)
        want = -(2 * 0.5 * math.log(0.5) + 2 * 1e-10 * math.log(1e-10))
        assert abs(cls.compute_weight_entropy(np.log(w))[0] - want) <= 1e-15
    n, z = cls._log_normalize(np.array([[0.0, 0.0]]))
    assert np.allclose(n, math.log(0.5)) and np.allclose(z, math.log(2.0))


@pytest.mark.parametrize("T", [0, 4])
def test_filter_shapes_and_keys_with_the_restatement_as_resampler(T):
    B, N, d, H = 2, 6, 1, 3
    W = R.make_weights(np.random.default_rng(5), N, d, H, 1, "gru")
    f = RN.DifferentiableParticleFilterRNN(N, d, *R.lgssm(3), rnn_type="gru", rnn_hidden_dim=H, weights=W,
                                           temperature=0.5, rng=np.random.default_rng(7))
    f._resample = R.resample_fn(W, "gru")
    obs = np.random.default_rng(1).standard_normal((B, T, d))
    ps, lws, As = f.filter(obs, np.zeros(d), np.eye(d))
    assert ps.shape == (B, T + 1, N, d) and lws.shape == (B, T + 1, N) and As.shape == (B, T, N, N)
    assert ps.dtype == np.float64 and np.all(np.isfinite(ps))
    f.rng = np.random.default_rng(7)
    f.transition_fn, f.log_likelihood_fn = R.lgssm(3)
    ps2, lws2, As2, st = f.filter(obs, np.zeros(d), np.eye(d), return_ess=True)
    assert np.array_equal(ps2, ps) and np.array_equal(As2, As)
    assert set(st) == {"ess_before_resampling", "ess_after_resampling", "entropy_before_resampling",
                       "entropy_after_resampling", "mean_ess_before", "mean_ess_after", "mean_entropy_before",
                       "mean_entropy_after", "min_ess_before", "min_ess_after"}
    assert st["ess_before_resampling"].shape == (B, T) and st["entropy_after_resampling"].shape == (B, T)
    if T:
        assert np.allclose(st["ess_after_resampling"], N) and np.allclose(As.sum(-1), 1.0)
        ref = R.filter(obs, np.zeros(d), np.eye(d), *R.lgssm(3), N, d, W, "gru", np.random.default_rng(7), T=0.5)
        assert np.array_equal(ref[0], ps) and np.array_equal(ref[2], As)
        # step: the tuple and the dictionary of rnn.py:531-537
        out = f.step(ps[:, 0], lws[:, 0], obs[:, 0], return_ess=True)
        assert len(out) == 4 and set(out[3]) == {"ess_before", "ess_after", "entropy_before", "entropy_after"}
        assert out[0].shape == (B, N, d) and out[2].shape == (B, N, N) and len(f.step(ps[:, 0], lws[:, 0], obs[:, 0])) == 3
    assert f.epoch == 0 and f._h is None


def test_python_validation_raises_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(NV, "load", no_load)
    W = R.make_weights(np.random.default_rng(0), 2, 1, 3, 1, "lstm")
    for P, lw, kw in [(np.zeros(4), np.zeros(4), {}), (np.zeros((2, 1)), np.zeros(3), {}),
                      (np.array([[0.0], [np.nan]]), np.zeros(2), {}), (np.zeros((2, 1)), np.array([0.0, np.nan]), {}),
                      (np.zeros((2, 1)), np.array([-np.inf, -np.inf]), {}), (np.zeros((2, 1)), np.zeros(2), {"temperature": 0.0}),
                      (np.zeros((2, 1)), np.zeros(2), {"use_weight_features": False, "use_particle_features": False}),
                      (np.zeros((2, 2)), np.zeros(2), {})]:  # d = 2 against weights made for d = 1
        with pytest.raises(ValueError):
            RN.rnn_resample(P, lw, W, **kw)


# ------------------------------------------------------------------ 5. the C entries without a device
def _create(**kw):
    o = dict(n_particles=10, dim=2, batch=1, hidden=8, layers=1, cell=0, use_weight=1, use_particle=1, device=0)
    o.update(kw)
    h = C.c_void_p()
    st = NV.load().pf_rnn_create(C.byref(NV.RnnOpts(**o)), C.byref(h))
    return st, h


@pytest.mark.parametrize("kw,word", [
    (dict(n_particles=0), "n_particles"), (dict(dim=0), "dim"), (dict(dim=1025), "dim"),
    (dict(hidden=0), "hidden"), (dict(hidden=129), "hidden"), (dict(layers=0), "layers"), (dict(layers=5), "layers"),
    (dict(batch=0), "batch"), (dict(batch=65536), "batch"), (dict(cell=2), "cell"),
    (dict(use_weight=0, use_particle=0), "use_weight"), (dict(n_particles=16385), "2^28"),
    (dict(n_particles=8192, batch=5), "2^28"), (dict(n_particles=1 << 40), "2^28"),
])
def test_create_rejects_each_limit_before_touching_a_device(kw, word):
    st, h = _create(**kw)
    assert st == NV.PF_E_ARG and not h.value
    assert word in NV.load().pf_last_error().decode()


def test_entries_reject_null_arguments():
    lib = NV.load()
    h = C.c_void_p()
    x = np.zeros(4)
    assert lib.pf_rnn_create(None, C.byref(h)) == NV.PF_E_ARG
    assert lib.pf_rnn_create(C.byref(NV.RnnOpts(10, 2, 1, 8, 1, 0, 1, 1, 0)), None) == NV.PF_E_ARG
    assert lib.pf_rnn_set_weights(None, None, None, 0) == NV.PF_E_ARG
    assert lib.pf_rnn_resample(None, NV.dptr(x), NV.dptr(x), 1.0, NV.dptr(x), None, None) == NV.PF_E_ARG
    assert lib.pf_rnn_baseline(None, NV.dptr(x), NV.dptr(x), 0, 0, 0, NV.dptr(x), None) == NV.PF_E_ARG
    assert lib.pf_rnn_synchronize(None) == NV.PF_E_ARG
    assert not lib.pf_rnn_stream(None) and lib.pf_rnn_resident(None) == 0
    lib.pf_rnn_destroy(None)


# ------------------------------------------------------------------ 6. the shape plan
def test_recurrence_plan_under_sanitizers():
    """pf::rnn::make_plan (csrc/pf_rnn_plan.h) in a stand-alone program under AddressSanitizer +
    UndefinedBehaviorSanitizer (tests/host/pf_rnn_plan_host_check.cpp)."""
    r = _plan_program()
    assert r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    # the second mode, one shape: H = 40 with two layers is three unit tiles whose fragments do not fit
    assert _plan_program(17, 2, 40, 2, "gru").stdout.split() == ["3", "10", "1", "192", "2", "0", "27648", "23040"]
