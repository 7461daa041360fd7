"""CPU checks of the soft (Gumbel-Softmax) resampler's host side (no GPU).

* the vectorised restatement (tests/dpf_soft_restatement.py), which the GPU tests compare the device
  with, equals the literal loop over rows and sources;
* the draw definition: the uniforms are odd multiples of 2^-53 strictly inside (0, 1), a draw at
  (i, j) does not depend on N or on the batch, and with T -> 0 the ancestors argmax_j(log q_j + G_ij)
  are distributed as q (a chi-square test over 8 groups at N = 1024: a failure would be a finding
  about the counter layout);
* pf_soft_create's argument checks and the null-pointer checks of the other entries, which answer
  before a device is touched, and the Python validation, which answers before the library is loaded;
* the members of DifferentiableParticleFilter against hand values, and ``filter`` with the
  restatement injected as resampler;
* the condition the hard-limit GPU test rests on.
"""

import ctypes as C

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_soft as SO
from tests import dpf_soft_restatement as R

CHI2_7_999 = 24.3219  # the 99.9 % quantile of chi-square with 7 degrees of freedom


@pytest.mark.parametrize("N,d,alpha,T,seed,epoch,problem", [(1, 2, 0.1, 0.2, 0, 0, 0), (2, 1, 0.0, 1.0, 1, 0, 3),
                                                            (7, 3, 0.1, 0.2, 2, 5, 0), (24, 2, 1.0, 0.2, 3, 0, 1),
                                                            (17, 5, 0.1, 1.0, 1 << 40, 2, 0)])
def test_vectorised_restatement_equals_the_loop(N, d, alpha, T, seed, epoch, problem):
    X, lw = R.make_case(N, d, seed=seed % 1000)
    v = R.soft_resample(X, lw, alpha, T, seed, epoch, problem)
    l = R.loop_resample(X, lw, alpha, T, seed, epoch, problem)
    for key in ("particles", "entropy", "log_probs"):
        scale = max(1.0, float(np.max(np.abs(l[key]))))
        err = float(np.max(np.abs(v[key] - l[key])))
        print(f"restatement vs loop N={N} d={d} {key}: {err:.3e} (scale {scale:.3g})")
        assert err <= 1e-13 * scale
    assert np.allclose(v["A"].sum(axis=-1), 1.0, rtol=0, atol=1e-14)


def test_uniforms_are_odd_multiples_of_2_to_minus_53_inside_the_open_interval():
    m = R.mantissas(np.arange(40), np.arange(41), seed=3, epoch=1, problem=2)
    assert m.dtype == np.uint64 and int(m.max()) < 1 << 52
    U = R.uniforms(np.arange(40), np.arange(41), seed=3, epoch=1, problem=2)
    assert np.all(U > 0.0) and np.all(U < 1.0)
    k = U * 9007199254740992.0  # exact: a power of two
    assert np.array_equal(k, np.floor(k)) and np.all(k.astype(np.uint64) % 2 == 1)
    assert np.array_equal(k.astype(np.uint64), 2 * m + 1)
    # the extremes of m give the extremes of u, both inside (0, 1) and finite under -log(-log(u))
    for mm in (0, (1 << 52) - 1):
        u = (2 * mm + 1) * R.TWO_M53
        assert 0.0 < u < 1.0 and np.isfinite(-np.log(-np.log(u)))
    assert len(np.unique(U)) == U.size  # 52 bits: no repeats among 1640 draws


def test_draws_do_not_depend_on_n_or_on_the_batch():
    U5, G5 = R.draws(5, seed=9, epoch=2, problem=1)
    U9, G9 = R.draws(9, seed=9, epoch=2, problem=1)
    assert np.array_equal(U5, U9[:5, :5]) and np.array_equal(G5, G9[:5, :5])
    # the two halves of a Philox call go to the sources (2k, 2k + 1) of one row
    k0, k1 = 9, 0
    x, y, z, w = (int(v) for v in R.philox4x32_10(1, 4, 2, 5 + 256, k0, k1))
    assert U9[4, 2] == (2 * (((x >> 6) << 26) | (y >> 6)) + 1) * R.TWO_M53
    assert U9[4, 3] == (2 * (((z >> 6) << 26) | (w >> 6)) + 1) * R.TWO_M53
    # other problems, epochs and seeds are other streams
    for kw in (dict(problem=0), dict(epoch=3), dict(seed=10)):
        args = dict(seed=9, epoch=2, problem=1)
        args.update(kw)
        assert not np.any(R.draws(9, **args)[0] == U9)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ancestors_follow_q(seed):
    """T -> 0: row i picks argmax_j(log q_j + G_ij), a draw from q (the Gumbel-max trick).  Weights on 8
    groups of 128 particles; the group counts of the N = 1024 rows against N q."""
    N, groups = 1024, 8
    share = np.array([0.30, 0.22, 0.16, 0.12, 0.08, 0.06, 0.04, 0.02])
    lw = np.log(np.repeat(share / (N // groups), N // groups))
    lp = R.log_probs(lw, 0.1)
    q = np.exp(lp)
    assert abs(q.sum() - 1.0) <= 1e-12
    _, G = R.draws(N, seed=seed, epoch=0, problem=0)
    anc = np.argmax(lp[None, :] + G, axis=-1)
    counts = np.bincount(anc // (N // groups), minlength=groups)
    expect = N * q.reshape(groups, -1).sum(axis=1)
    chi2 = float(np.sum((counts - expect) ** 2 / expect))
    print(f"ancestors seed={seed}: counts {counts.tolist()}, expected {np.round(expect, 1).tolist()}, chi2 {chi2:.2f}")
    assert chi2 <= CHI2_7_999
    # and inside a group the ancestors spread over its particles
    assert len(np.unique(anc)) > N // 4


# ------------------------------------------------------------------ C ABI, no device
def _create(n, d, b, dev=0):
    h = C.c_void_p()
    st = NV.load().pf_soft_create(C.byref(NV.SoftOpts(n, d, b, dev)), C.byref(h))
    return st, h


def test_entries_reject_bad_arguments_before_touching_a_device():
    lib = NV.load()
    for n, d, b in ((0, 2, 1), (-5, 2, 1), ((1 << 24) + 1, 2, 1), (10, 0, 1), (10, 1025, 1), (10, 2, 0), (10, 2, -1),
                    (10, 2, 65536)):
        st, h = _create(n, d, b)
        assert st == NV.PF_E_ARG and not h.value, (n, d, b)
        assert lib.pf_last_error()
    h = C.c_void_p()
    assert lib.pf_soft_create(None, C.byref(h)) == NV.PF_E_ARG
    assert lib.pf_soft_create(C.byref(NV.SoftOpts(10, 2, 1, 0)), None) == NV.PF_E_ARG
    x = np.zeros(4)
    assert lib.pf_soft_resample(None, NV.dptr(x), NV.dptr(x), 0.2, 0, 0, 0, NV.dptr(x), None) == NV.PF_E_ARG
    assert lib.pf_soft_draws(None, 0, 0, 0, NV.dptr(x), NV.dptr(x)) == NV.PF_E_ARG
    assert lib.pf_soft_synchronize(None) == NV.PF_E_ARG
    assert not lib.pf_soft_stream(None)
    lib.pf_soft_destroy(None)
    with pytest.raises(ValueError):
        NV.check(NV.PF_E_ARG)


@pytest.mark.parametrize("particles,log_weights,kw", [
    (np.zeros(4), np.zeros(4), {}),                        # rank
    (np.zeros((2, 3, 4, 5)), np.zeros((2, 3)), {}),        # rank
    (np.zeros((4, 2)), np.zeros((4, 1)), {}),              # log_weights rank
    (np.zeros((4, 2)), np.zeros(5), {}),                   # N mismatch
    (np.zeros((3, 4, 2)), np.zeros((2, 4)), {}),           # batch mismatch
    (np.zeros((0, 2)), np.zeros(0), {}),                   # N < 1
    (np.zeros((4, 0)), np.zeros(4), {}),                   # d < 1
    (np.zeros((2, 1025)), np.zeros(2), {}),                # d above the device limit
    (np.array([[0.0], [np.nan]]), np.zeros(2), {}),        # non-finite particles
    (np.array([[0.0], [np.inf]]), np.zeros(2), {}),
    (np.zeros((2, 1)), np.array([0.0, np.nan]), {}),       # NaN log-weight
    (np.zeros((2, 1)), np.array([0.0, np.inf]), {}),       # +inf log-weight
    (np.zeros((2, 1)), np.array([-np.inf, -np.inf]), {}),  # no finite log-weight
    (np.zeros((2, 1)), np.zeros(2), {"soft_alpha": -0.1}),
    (np.zeros((2, 1)), np.zeros(2), {"soft_alpha": 1.5}),
    (np.zeros((2, 1)), np.zeros(2), {"soft_alpha": np.nan}),
    (np.zeros((2, 1)), np.zeros(2), {"gumbel_temperature": 0.0}),
    (np.zeros((2, 1)), np.zeros(2), {"gumbel_temperature": -1.0}),
    (np.zeros((2, 1)), np.zeros(2), {"gumbel_temperature": np.inf}),
    (np.zeros((2, 1)), np.zeros(2), {"seed": -1}),
    (np.zeros((2, 1)), np.zeros(2), {"seed": 1 << 64}),
    (np.zeros((2, 1)), np.zeros(2), {"epoch": 1 << 32}),
    (np.zeros((2, 1)), np.zeros(2), {"epoch": 0.5}),
])
def test_python_validation_raises_before_the_library_is_loaded(monkeypatch, particles, log_weights, kw):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(NV, "load", no_load)
    with pytest.raises(ValueError):
        SO.soft_resample(particles, log_weights, **kw)


def test_log_probs_of_the_module_are_the_restatements():
    X, lw = R.make_case(30, 2, seed=5)
    for alpha in (0.0, 0.1, 1.0):
        norm, log_z = SO.DifferentiableParticleFilter._log_normalize(lw)
        assert np.max(np.abs(SO._log_probs(norm, alpha) - R.log_probs(lw, alpha))) <= 1e-14
    # a zero weight: log(0 + 1e-20) with alpha = 0, the uniform share otherwise
    lw0 = np.array([0.0, -np.inf, 0.0])
    norm, _ = SO._log_normalize(lw0)
    assert SO._log_probs(norm, 0.0)[1] == np.log(1e-20)
    assert SO._log_probs(norm, 0.3)[1] == pytest.approx(np.log(0.1), rel=1e-15)


# ------------------------------------------------------------------ the class on the host
def _filter(N=12, d=2, **kw):
    tf_, lf_ = R.linear_model(8)
    flt = SO.DifferentiableParticleFilter(N, d, tf_, lf_, **kw)
    flt._resample = R.resample_fn
    return flt


def test_static_members_against_hand_values():
    F = SO.DifferentiableParticleFilter
    N = 20
    uni = np.log(np.full((3, N), 1.0 / N))
    assert np.allclose(F.compute_ess(uni), N, rtol=1e-14, atol=0)
    assert np.allclose(F.compute_ess(uni + 4.0), N, rtol=1e-14, atol=0)  # unnormalised log-weights
    assert np.allclose(F.compute_weight_entropy(uni), np.log(N), rtol=0, atol=1e-8)  # the 1e-10 inside the log
    one = np.full((1, N), -np.inf)
    one[0, 3] = 0.0
    assert F.compute_ess(one)[0] == 1.0 and abs(F.compute_weight_entropy(one)[0]) <= 1e-9
    lw = np.random.default_rng(1).standard_normal((2, 7)) * 5.0
    norm, log_z = F._log_normalize(lw)
    assert norm.shape == (2, 7) and log_z.shape == (2,)
    assert np.allclose(np.sum(np.exp(norm), axis=-1), 1.0, rtol=0, atol=1e-14)
    assert np.allclose(log_z, np.log(np.sum(np.exp(lw), axis=-1)), rtol=1e-14, atol=0)
    assert F._log_normalize(lw, keepdims=True)[1].shape == (2, 1)


def test_particle_diversity_is_the_references_formulas():
    rng = np.random.default_rng(6)
    P = rng.standard_normal((2, 30, 3))
    dv = SO.DifferentiableParticleFilter.compute_particle_diversity(P, block=7)  # blocks with a tail
    for b in range(2):
        full = np.linalg.norm(P[b, :, None, :] - P[b, None, :, :], axis=-1)
        full[np.arange(30), np.arange(30)] = 0.0
        assert dv["mean_pairwise_dist"][b] == pytest.approx(full.sum() / (30 * 29), rel=1e-13)
        assert dv["std_pairwise_dist"][b] == pytest.approx(np.std(full.reshape(-1)), rel=1e-13)  # zeros included
        assert dv["particle_spread"][b] == pytest.approx(np.trace(np.cov(P[b].T, bias=True)), rel=1e-13)
    assert set(dv) == {"mean_pairwise_dist", "std_pairwise_dist", "particle_spread"}
    # two points at distance 5: masked array (0, 5, 5, 0), mean over the 2 ordered pairs
    dv2 = SO.DifferentiableParticleFilter.compute_particle_diversity(np.array([[[0.0, 0.0], [3.0, 4.0]]]))
    assert dv2["mean_pairwise_dist"][0] == 5.0 and dv2["std_pairwise_dist"][0] == 2.5
    assert dv2["particle_spread"][0] == pytest.approx(6.25)


def test_init_particles_shapes_and_the_eps_times_l_orientation():
    N, d, B = 6, 2, 3
    flt = _filter(N, d, rng=np.random.default_rng(4))
    L = np.array([[1.0, 0.0], [2.0, 0.5]])  # not symmetric: eps @ L and eps @ L.T differ
    mean = np.array([10.0, -10.0])
    particles, logw = flt.init_particles(B, mean, L)
    assert particles.shape == (B, N, d) and particles.dtype == np.float64
    assert np.array_equal(logw, np.log(np.full((B, N), 1.0 / N)))
    eps = np.random.default_rng(4).standard_normal((B, N, d))
    assert np.allclose(particles, mean + eps @ L, rtol=0, atol=1e-14)
    assert not np.allclose(particles, mean + eps @ L.T, rtol=0, atol=1e-3)
    # batched mean and factor
    flt.rng = np.random.default_rng(4)
    Lb = np.stack([L, 2 * L, 3 * L])
    mb = np.stack([mean, mean + 1, mean + 2])
    pb, _ = flt.init_particles(B, mb, Lb)
    assert np.allclose(pb[2], mb[2] + eps[2] @ Lb[2], rtol=0, atol=1e-13)


def test_gumbel_utilities_draw_from_the_filters_rng():
    flt = _filter(rng=np.random.default_rng(11))
    g = flt._sample_gumbel((4, 5))
    u = np.random.default_rng(11).uniform(1e-20, 1.0 - 1e-20, size=(4, 5))
    assert np.array_equal(g, -np.log(-np.log(u)))
    y = flt._gumbel_softmax(np.log(np.full((3, 8), 0.125)), 0.5)
    assert y.shape == (3, 8) and np.allclose(y.sum(axis=-1), 1.0, rtol=0, atol=1e-14) and np.all(y > 0.0)


def test_step_hands_the_normalised_log_weights_to_the_resampler_and_advances_the_epoch():
    N, d, B = 12, 2, 2
    tf_, lf_ = R.linear_model(8)
    flt = SO.DifferentiableParticleFilter(N, d, tf_, lf_, soft_alpha=0.3, gumbel_temperature=0.7, seed=5,
                                          rng=np.random.default_rng(3))
    seen = {}

    def stub(particles, log_weights, soft_alpha, gumbel_temperature, seed, epoch, want_entropy):
        seen.update(particles=particles.copy(), log_weights=log_weights.copy(), alpha=soft_alpha,
                    T=gumbel_temperature, seed=seed, epoch=epoch, want=want_entropy)
        return particles + 1.0, None
    flt._resample = stub
    particles, logw = flt.init_particles(B, np.zeros(d), np.eye(d))
    lw_in = np.random.default_rng(1).standard_normal((B, N))
    y = np.array([[0.4, -0.2], [0.1, 0.3]])
    out, lw_out = flt.step(particles, lw_in, y)
    pred = 0.9 * particles + 0.1 * np.random.default_rng(8).standard_normal(particles.shape)
    lw = lw_in + lf_(pred, y, {})
    lw = lw - np.log(np.sum(np.exp(lw), axis=-1, keepdims=True))
    assert np.array_equal(seen["particles"], pred)
    assert np.allclose(seen["log_weights"], lw, rtol=0, atol=1e-13)
    assert (seen["alpha"], seen["T"], seen["seed"], seen["epoch"], seen["want"]) == (0.3, 0.7, 5, 0, False)
    assert np.array_equal(out, pred + 1.0) and np.array_equal(lw_out, np.log(np.full((B, N), 1.0 / N)))
    assert flt.epoch == 1

    def failing(*a):
        raise RuntimeError("resampler failed")
    flt._resample = failing
    with pytest.raises(RuntimeError):
        flt.step(particles, lw_in, y)
    assert flt.epoch == 1  # a failed call does not advance the epoch


@pytest.mark.parametrize("T", [0, 5])
def test_filter_shapes_with_the_restatement_as_resampler(T):
    N, d, B = 12, 2, 2
    flt = _filter(N, d, rng=np.random.default_rng(2), seed=3)
    obs = np.random.default_rng(4).standard_normal((B, T, d))
    ps, lws = flt.filter(obs, np.zeros(d), np.eye(d))
    assert ps.shape == (B, T + 1, N, d) and lws.shape == (B, T + 1, N)
    assert ps.dtype == np.float64 and np.all(np.isfinite(ps)) and flt.epoch == T
    assert np.array_equal(lws, np.log(np.full((B, T + 1, N), 1.0 / N)))
    truth = np.zeros((B, T + 1, d))
    flt2 = _filter(N, d, rng=np.random.default_rng(2), seed=3)
    ps2, lws2, diag = flt2.filter(obs, np.zeros(d), np.eye(d), return_diagnostics=True, ground_truth=truth)
    assert np.array_equal(ps2, ps)  # the diagnostics change no result
    assert diag["rmse_sequence"].shape == (T + 1,) and diag["total_time"] >= 0.0
    if T == 0:
        assert set(diag) == {"total_time", "mean_step_time", "rmse_sequence", "mean_rmse", "final_rmse"}
        return
    for key in ("ess_before", "ess_after", "entropy_before", "entropy_after", "assignment_entropy_mean",
                "assignment_entropy_std", "max_weight_before"):
        for s in ("_mean", "_std", "_min", "_max"):
            assert key + s in diag, key + s
    for key in ("soft_alpha", "gumbel_temperature", "step_time"):
        assert key + "_mean" in diag and key + "_std" in diag and key + "_min" not in diag
    assert set(diag["diversity_before"]) == {k + s for k in ("mean_pairwise_dist", "std_pairwise_dist",
                                                              "particle_spread")
                                             for s in ("_mean", "_std", "_min", "_max")}
    assert abs(diag["ess_after_mean"] - N) <= 1e-9 and diag["soft_alpha_mean"] == pytest.approx(0.1)
    assert 0.0 < diag["assignment_entropy_mean_mean"] < np.log(N)


def test_rmse_sequence_is_the_batch_root_mean_square():
    flt = _filter(3, 1)
    ps = np.array([[[[1.0], [2.0], [3.0]]], [[[0.0], [0.0], [6.0]]]])  # (B = 2, T + 1 = 1, N = 3, d = 1)
    lw = np.log(np.full((2, 1, 3), 1.0 / 3.0))
    truth = np.zeros((2, 1, 1))
    assert flt._compute_rmse_sequence(ps, lw, truth) == pytest.approx([np.sqrt((4.0 + 4.0) / 2.0)])


# ------------------------------------------------------------------ what the GPU tests assume
def test_hard_limit_rows_have_a_clear_winner():
    """tests/test_gpu_dpf_soft.py compares row i at T = 1e-3 with X[argmax_j(log q_j + G_ij)] on every
    row whose top-two gap exceeds 0.04: there the leading weight is at least 1 - N e^-40.  At least
    90 % of the rows must qualify."""
    c = R.HARD
    X, lw, anc, gap = R.hard_case()
    ok = gap > c["gap"]
    print(f"hard limit: {int(ok.sum())} of {c['N']} rows have a top-two gap above {c['gap']}, smallest {gap.min():.3e}")
    assert ok.mean() >= c["share"]
    r = R.soft_resample(X, lw, c["alpha"], c["T"], c["seed"], c["epoch"])
    lead = np.max(r["A"], axis=-1)
    assert np.all(lead[ok] >= 1.0 - c["N"] * np.exp(-40.0))
    assert np.array_equal(np.argmax(r["A"], axis=-1), anc)
    scale = max(1.0, float(np.max(np.abs(X))))
    assert np.max(np.abs(r["particles"][ok] - X[anc[ok]])) <= 1e-9 * scale


def test_parity_cases_are_finite_and_cover_what_they_claim():
    Ns = {c[0] for c in R.PARITY}
    ds = {c[1] for c in R.PARITY}
    assert {1, 2, 3, 63, 64, 65, 130, 300} <= Ns and {1, 2, 5, 16, 17, 40} <= ds
    assert {c[2] for c in R.PARITY} == {0.0, 0.1, 1.0} and {c[3] for c in R.PARITY} == {0.2, 1.0}
    assert {c[4] for c in R.PARITY} == {"uniform", "normal", "dominant"}
    X, lw = R.dominant_case(65, 1, 5)
    assert np.max(lw) - np.min(lw) == 30.0
    for case in R.PARITY[:6]:
        X, lw, ref = R.solved(*case)
        assert np.all(np.isfinite(ref["particles"])) and np.all(np.isfinite(ref["entropy"]))
