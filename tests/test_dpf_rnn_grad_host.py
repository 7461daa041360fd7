"""The reference of the RNN resampler's backward pass, checked on the CPU, and the host side of the
new entries (no GPU).

tests/dpf_rnn_grad_restatement.py restates tests/dpf_rnn_restatement.resample in torch so that CPU
fp64 autograd gives the gradients tests/test_gpu_dpf_rnn_grad.py compares the device with.  Here:

1. the torch forward equals the NumPy restatement (measured: at most 1.2e-15 on A over the cases);
2. autograd agrees with fp64 central differences on a tiny LSTM and a tiny GRU;
3. no gradient vanishes: for every case with N >= 2 each of gX, gw (with use_weight), every gK_l,
   gR_l, gb_l, gKd and gbd has max |g_ref| > 1e-3 max(1, scale), scale being the size of the
   cotangent-weighted outputs (1 for these cases: the cotangents are standard normals and A <= 1), so
   a backward pass that returns zeros cannot pass (smallest maximum measured: 4.4e-2, gR0 at N = 3,
   H = 5, L = 3); at N = 1 every gradient but gX = gXo is exactly 0, asserted instead;
4. conditioning: the same network with the hidden units of every layer renumbered - the same
   function in another summation order - moves every gradient by at most 1e-12 relative to
   max(1, max |g|) on every case the GPU tests use, H = 128 / L = 4 included (measured: at most
   3.5e-14, gX, gw and gbd at T = 0.1; elsewhere at most 3e-15);
5. the plan of the backward pass (csrc/pf_rnn_bwd_plan.h) in a stand-alone program under
   AddressSanitizer + UndefinedBehaviorSanitizer;
6. argument errors of rnn_resample_vjp and the torch wrapper are raised before the library loads, and
   the CPU training trajectory the GPU test follows ends below its start.
"""

import os
import subprocess

import numpy as np
import pytest
import torch

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_rnn as RN
from particle_filters_amd import dpf_rnn_torch as RT
from tests import dpf_rnn_grad_restatement as G
from tests import dpf_rnn_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every case a GPU test of the backward pass runs
EXTRA = [R.case(17, 2, 16, 1, "lstm", seed=51), R.case(16, 2, 16, 1, "lstm", seed=51),
         R.case(17, 2, 5, 2, "gru", seed=21), R.case(33, 1, 24, 1, "lstm", seed=22),
         R.case(16, 1, 128, 1, "gru", seed=23, res=False), R.case(17, 1, 8, 4, "gru", seed=24)]
CASES = R.PARITY + EXTRA


def _id(c):
    return R.case_id(c) + f"-s{c['seed']}"


# ------------------------------------------------------------------ 1. the torch forward
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_torch_forward_is_the_numpy_restatement(c):
    X, lw, W, ref = R.solved(c)
    _, _, _, _, _, g = G.solved(c)
    for b in range(c["B"]):
        ea = float(np.max(np.abs(g[1][b] - ref[b]["A"])))
        ex = float(np.max(np.abs(g[0][b] - ref[b]["particles"])))
        assert ea <= 1e-13, ea
        assert ex <= 1e-13 * max(1.0, float(np.max(np.abs(ref[b]["particles"])))), ex


# ------------------------------------------------------------------ 2. central differences
@pytest.mark.parametrize("c", [R.case(3, 2, 3, 2, "lstm", seed=61), R.case(3, 2, 3, 2, "gru", seed=62)], ids=_id)
def test_autograd_agrees_with_central_differences(c):
    X, lw, W = R.case_inputs(c)
    gXo, gA = G.cotangents(c)
    _, _, gX, glw, gW = G.gradients(X, lw, W, gXo, gA, c["cell"], c["T"], True, True)

    def loss(X, lw, W):
        r = R.resample(X[0], lw[0], W, c["cell"], c["T"])
        return float(np.sum(gXo[0] * r["particles"]) + np.sum(gA[0] * r["A"]))

    eps = 1e-6
    arrays = [X, lw] + W
    for k, (a, g) in enumerate(zip(arrays, [gX, glw] + list(gW))):
        fd = np.zeros_like(a)
        for idx in np.ndindex(a.shape):
            hi, lo = [x.copy() for x in arrays], [x.copy() for x in arrays]
            hi[k][idx] += eps
            lo[k][idx] -= eps
            fd[idx] = (loss(hi[0], hi[1], hi[2:]) - loss(lo[0], lo[1], lo[2:])) / (2 * eps)
        # central differences in fp64: truncation eps^2 |f'''| and round-off 1e-16 |f| / eps, both below 1e-7
        assert np.max(np.abs(fd - g)) <= 1e-7 * max(1.0, float(np.max(np.abs(g)))), k


# ------------------------------------------------------------------ 3. no gradient vanishes
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_no_reference_gradient_vanishes(c):
    X, lw, W, gXo, gA, ref = G.solved(c)
    named = dict(zip(["gX", "glw"] + G.names(c["L"]), [ref[2], ref[3]] + list(ref[4])))
    if c["N"] == 1:
        assert np.array_equal(named.pop("gX"), gXo)
        for name, g in named.items():
            assert np.all(g == 0.0), name
        return
    if not c["uw"]:
        assert np.all(named.pop("glw") == 0.0)
    for name, g in named.items():
        assert float(np.max(np.abs(g))) > 1e-3, name


# ------------------------------------------------------------------ 4. conditioning
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_gradients_are_well_conditioned(c):
    X, lw, W, gXo, gA, ref = G.solved(c)
    Wp, back = G.permuted(W, c["cell"], np.random.default_rng(c["seed"]))
    other = G.gradients(X, lw, Wp, gXo, gA, c["cell"], c["T"], c["uw"], c["up"])
    for name, g, o in zip(["gX", "glw"] + G.names(c["L"]), [ref[2], ref[3]] + list(ref[4]),
                          [other[2], other[3]] + back(list(other[4]))):
        rel = float(np.max(np.abs(g - o))) / max(1.0, float(np.max(np.abs(g))))
        assert rel <= 1e-12, (name, rel)


def test_permutation_is_the_same_function():
    c = R.PARITY[4]
    X, lw, W, ref = R.solved(c)
    Wp, _ = G.permuted(W, c["cell"], np.random.default_rng(1))
    assert any(not np.array_equal(a, b) for a, b in zip(W, Wp))
    got = R.resample(X[0], lw[0], Wp, c["cell"], c["T"])
    assert np.max(np.abs(got["A"] - ref[0]["A"])) <= 1e-13


# ------------------------------------------------------------------ 5. the plan of the backward pass
def _plan_program(*args):
    exe = os.path.join(REPO, "build", "pf_rnn_bwd_plan_host_check")
    if not os.path.exists(exe):  # built by __graft_entry__.build(); here if the test runs first
        subprocess.run(["make", "-C", os.path.join(REPO, "particle_filters_amd", "csrc"), "hostcheck"],
                       check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_backward_plan_under_sanitizers():
    assert _plan_program().stdout.strip().endswith("ok")
    # one shape: N = 100, d = 1, B = 64, H = 32, L = 1, LSTM keeps both sets of fragments on chip
    res, lds, tc, chunks, ws = (int(v) for v in _plan_program(100, 1, 64, 32, 1, "lstm").stdout.split())
    assert (res, lds, tc, chunks) == (1, 8 * (6 * 32 * 18 + 2 * 4096), 8, 13)
    hist = 64 * 7 * 100 * 16 * 32  # B tiles N L 16 Hp
    assert ws > 8 * 6 * hist and ws < 8 * 6 * hist * 1.1  # h, c and the four slot deltas dominate


# ------------------------------------------------------------------ 6. arguments, no library
def _no_load(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(NV, "load", no_load)


def test_vjp_validation_raises_before_the_library_is_loaded(monkeypatch):
    _no_load(monkeypatch)
    rng = np.random.default_rng(0)
    W = R.make_weights(rng, 4, 2, 3, 1, "gru")
    X, lw, g = np.zeros((4, 2)), np.full(4, np.log(0.25)), np.zeros((4, 2))
    bad = [
        dict(grad_new_particles=np.zeros((4, 3))),
        dict(grad_new_particles=np.full((4, 2), np.nan)),
        dict(grad_assignment=np.zeros((4, 5))),
        dict(grad_assignment=np.full((4, 4), np.inf)),
        dict(temperature=0.0),
        dict(rnn_type="rnn"),
        dict(weights=W[:-1]),
        dict(weights=W[:1] + [W[1][:, :-1]] + W[2:]),
        dict(use_weight_features=False, use_particle_features=False),
        dict(log_weights=np.full(4, np.nan)),
    ]
    for kw in bad:
        args = dict(particles=X, log_weights=lw, weights=W, grad_new_particles=g, rnn_type="gru")
        args.update(kw)
        with pytest.raises(ValueError):
            RN.rnn_resample_vjp(**args)


def test_torch_wrapper_argument_errors_before_the_library_is_loaded(monkeypatch):
    _no_load(monkeypatch)
    W = [torch.from_numpy(a) for a in R.make_weights(np.random.default_rng(0), 4, 2, 3, 1, "gru")]
    x, w = torch.zeros((4, 2), dtype=torch.float64), torch.full((4,), float(np.log(0.25)), dtype=torch.float64)
    for bad_x, bad_w, bad_W in ((x.float(), w, W), (x, w.float(), W), (x, w, [a.float() for a in W]), (x.numpy(), w, W)):
        with pytest.raises(TypeError):
            RT.rnn_resample(bad_x, bad_w, bad_W, "gru")
    with pytest.raises(TypeError, match="temperature"):
        RT.rnn_resample(x, w, W, "gru", torch.tensor(1.0))
    with pytest.raises(ValueError):
        RT.rnn_resample(x, w, W[:-1], "gru")
    with pytest.raises(ValueError, match="baseline"):
        RT.DifferentiableParticleFilterRNN(4, 2, None, None, use_baseline_resampling=True)
    dpf = RT.DifferentiableParticleFilterRNN(4, 2, None, None, rnn_type="gru", rnn_hidden_dim=3,
                                             rng=np.random.default_rng(1))
    params = dpf.parameters()
    assert [tuple(p.shape) for p in params] == RN.weight_shapes(4, 2, "gru", 3, 1)
    assert all(isinstance(p, torch.nn.Parameter) and p.dtype == torch.float64 for p in params)
    dpf.set_weights([a.numpy() for a in W])
    assert all(p is q for p, q in zip(params, dpf.parameters()))  # an optimizer keeps its parameters
    assert all(np.array_equal(a, b.numpy()) for a, b in zip(dpf.get_weights(), W))
    with pytest.raises(ValueError):
        dpf.set_weights([a.numpy() for a in W[:-1]])


def test_new_entries_are_declared():
    assert {"pf_rnn_backward", "pf_rnn_backward_bytes"} <= set(NV.SIGNATURES)
    assert len(NV.SIGNATURES["pf_rnn_backward"][1]) == 11


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_cpu_training_trajectory_descends(cell):
    losses = G.cpu_training(cell)
    assert len(losses) == G.TRAIN_STEPS and losses[-1] < losses[0]
    assert all(b < a for a, b in zip(losses, losses[1:]))
