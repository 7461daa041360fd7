"""The argument errors of the three DPF resampler modules, character for character (no GPU).

``dpf_ot``, ``dpf_soft`` and ``dpf_rnn`` share their checks (``particle_filters_amd/_dpf_common.py``)
but not every wording: the tables below hold, for each module's ``_validate`` and for each
constructor, bad inputs and the exact text of the ``ValueError`` each must raise - recorded from
the modules as they were when each still spelled its checks out.  Where an input is wrong in two
ways the message is that of the check that comes first in the module's order.  Every check answers
before the library is loaded.
"""

import numpy as np
import pytest

from particle_filters_amd import _dpf_common as DC
from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_ot as OT
from particle_filters_amd import dpf_rnn as RN
from particle_filters_amd import dpf_soft as SO

INF = np.inf
Z = np.zeros


@pytest.fixture(autouse=True)
def _no_library(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(NV, "load", no_load)


def _raises(message, fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == message


# what all three say alike, with the module's name for its weights: (particles, weights, message)
def _shared(name):
    return [
        (Z(4), np.ones(4), "particles must be (N, d) or (B, N, d), got shape (4,)"),
        (Z((2, 3, 4, 5)), Z((2, 3)), "particles must be (N, d) or (B, N, d), got shape (2, 3, 4, 5)"),
        (Z((4, 2)), Z((4, 1)), f"{name} must be (N,) for particles of shape (4, 2), got shape (4, 1)"),
        (Z((2, 4, 2)), Z(4), f"{name} must be (B, N) for particles of shape (2, 4, 2), got shape (4,)"),
        (Z((4, 2)), Z(5), f"particles (4, 2) and {name} (5,) disagree on N (or on the batch)"),
        (Z((3, 4, 2)), Z((2, 4)), f"particles (4, 2) and {name} (4,) disagree on N (or on the batch)"),
        (Z((0, 2)), Z(0), "need N >= 1 and d >= 1, got N = 0, d = 2"),
        (Z((4, 0)), Z(4), "need N >= 1 and d >= 1, got N = 4, d = 0"),
        (Z((2, 1025)), Z(2), "d = 1025 is above the device limit of 1024"),
        (np.array([[0.0], [np.nan]]), Z(2), "particles must be finite"),
        (np.array([[[0.0], [INF]]]), Z((1, 2)), "particles must be finite"),
    ]


LOG_WEIGHTS = [
    (Z((2, 1)), np.array([0.0, INF]), "log_weights must not hold NaN or +inf"),
    (Z((2, 1)), np.array([0.0, np.nan]), "log_weights must not hold NaN or +inf"),
    (Z((2, 1)), np.array([-INF, -INF]), "every problem needs at least one finite log-weight"),
    (Z((2, 2, 1)), np.array([[0.0, -INF], [-INF, -INF]]), "every problem needs at least one finite log-weight"),
]


# ------------------------------------------------------------------ dpf_ot
@pytest.mark.parametrize("X,w,message", _shared("weights") + [
    (Z((0, 4, 2)), Z((0, 4)), "the batch must hold at least one problem"),
    (Z((0, 0, 2)), Z((0, 0)), "the batch must hold at least one problem"),
    (Z((2, 1)), np.array([1.0, INF]), "weights must be finite"),
    (Z((2, 1)), np.array([1.0, np.nan]), "weights must be finite"),
    (np.array([[np.nan], [0.0]]), np.array([1.0, INF]), "particles must be finite"),
])
def test_ot_validate_shapes_and_values(X, w, message):
    _raises(message, OT._validate, X, w, 0.1, 50)
    _raises(message, OT.sinkhorn_ot_resample, X, w)


@pytest.mark.parametrize("kw,message", [
    (dict(epsilon=0.0), "epsilon must be positive, got 0.0"),
    (dict(epsilon=-1), "epsilon must be positive, got -1"),
    (dict(epsilon=INF), "epsilon must be positive, got inf"),
    (dict(epsilon=np.nan), "epsilon must be positive, got nan"),
    (dict(n_iters=-1), "n_iters must be a non-negative integer, got -1"),
    (dict(n_iters=2.5), "n_iters must be a non-negative integer, got 2.5"),
    (dict(epsilon=0.0, n_iters=-1), "epsilon must be positive, got 0.0"),
])
def test_ot_validate_parameters(kw, message):
    _raises(message, OT.sinkhorn_ot_resample, Z((2, 1)), np.ones(2) / 2, **kw)
    _raises(message, OT._validate, Z((2, 1)), np.ones(2) / 2, kw.get("epsilon", 0.1), kw.get("n_iters", 50))


def test_ot_validate_returns_the_batched_arrays():
    X, w, batched = OT._validate(np.arange(6).reshape(3, 2), [1, 2, 3], 0.1, 5)
    assert X.shape == (1, 3, 2) and w.shape == (1, 3) and not batched
    assert X.dtype == w.dtype == np.float64 and X.flags.c_contiguous and w.flags.c_contiguous
    X, w, batched = OT._validate(Z((2, 3, 2)), Z((2, 3)), 0.1, 0)
    assert X.shape == (2, 3, 2) and w.shape == (2, 3) and batched


def test_ot_constructor():
    _raises("need N_particles >= 1 and state_dim >= 1, got 0, 2", OT.DPF_OT, 0, 2, None, None)
    _raises("need N_particles >= 1 and state_dim >= 1, got 3, 0", OT.DPF_OT, 3, 0, None, None)
    f = OT.DPF_OT(3, 2, None, None)
    assert f._h is None and f._resample == f._device_resample
    f.close()


# ------------------------------------------------------------------ dpf_soft
@pytest.mark.parametrize("X,lw,message", _shared("log_weights") + LOG_WEIGHTS + [
    (Z((0, 4, 2)), Z((0, 4)), "the batch must hold at least one problem"),
    (Z((65536, 1, 1)), Z((65536, 1)), "B = 65536 is above the device limit of 65535"),
    (Z((65536, 0, 1)), Z((65536, 0)), "B = 65536 is above the device limit of 65535"),
    (np.array([[np.nan], [0.0]]), np.array([0.0, INF]), "particles must be finite"),
])
def test_soft_validate_shapes_and_values(X, lw, message):
    _raises(message, SO._validate, X, lw, 0.1, 0.2)
    _raises(message, SO.soft_resample, X, lw)
    _raises(message, SO.soft_resample_vjp, X, lw, X)


@pytest.mark.parametrize("kw,message", [
    (dict(soft_alpha=1.5), "soft_alpha must be in [0, 1], got 1.5"),
    (dict(soft_alpha=-0.1), "soft_alpha must be in [0, 1], got -0.1"),
    (dict(soft_alpha=np.nan), "soft_alpha must be in [0, 1], got nan"),
    (dict(gumbel_temperature=0.0), "gumbel_temperature must be positive, got 0.0"),
    (dict(gumbel_temperature=-2), "gumbel_temperature must be positive, got -2"),
    (dict(gumbel_temperature=INF), "gumbel_temperature must be positive, got inf"),
    (dict(seed=-1), "seed must be an integer in [0, 2^64), got -1"),
    (dict(seed=1.5), "seed must be an integer in [0, 2^64), got 1.5"),
    (dict(seed=1 << 64), "seed must be an integer in [0, 2^64), got 18446744073709551616"),
    (dict(epoch=-1), "epoch must be an integer in [0, 2^32), got -1"),
    (dict(epoch=0.5), "epoch must be an integer in [0, 2^32), got 0.5"),
    (dict(epoch=1 << 32), "epoch must be an integer in [0, 2^32), got 4294967296"),
    (dict(soft_alpha=2, gumbel_temperature=0, seed=-1, epoch=-1), "soft_alpha must be in [0, 1], got 2"),
    (dict(gumbel_temperature=0, seed=-1, epoch=-1), "gumbel_temperature must be positive, got 0"),
    (dict(seed=-1, epoch=-1), "seed must be an integer in [0, 2^64), got -1"),
])
def test_soft_validate_parameters(kw, message):
    X, lw = Z((2, 1)), Z(2)
    _raises(message, SO.soft_resample, X, lw, **kw)
    _raises(message, SO.soft_resample_vjp, X, lw, X, **kw)
    _raises(message, SO._validate, X, lw, kw.get("soft_alpha", 0.1), kw.get("gumbel_temperature", 0.2),
            kw.get("seed", 0), kw.get("epoch", 0))


def test_soft_validate_accepts_the_edges_and_returns_the_batched_arrays():
    X, lw, batched = SO._validate(Z((3, 2)), [0.0, -INF, -3.0], 0.0, 1e-300, (1 << 64) - 1, (1 << 32) - 1)
    assert X.shape == (1, 3, 2) and lw.shape == (1, 3) and not batched
    assert X.dtype == lw.dtype == np.float64 and X.flags.c_contiguous and lw.flags.c_contiguous
    assert SO._validate(Z((2, 3, 2)), Z((2, 3)), 1.0, 5.0)[2]


def test_soft_constructor():
    _raises("need n_particles >= 1 and state_dim >= 1, got 0, 2", SO.DifferentiableParticleFilter, 0, 2, None, None)
    _raises("need n_particles >= 1 and state_dim >= 1, got 3, 0", SO.DifferentiableParticleFilter, 3, 0, None, None)
    _raises("seed must be an integer in [0, 2^64), got -1", SO.DifferentiableParticleFilter, 3, 2, None, None, seed=-1)
    _raises("seed must be an integer in [0, 2^64), got 0.5", SO.DifferentiableParticleFilter, 3, 2, None, None,
            seed=0.5)
    f = SO.DifferentiableParticleFilter(3, 2, None, None, seed=(1 << 64) - 1)
    assert f._h is None and f.epoch == 0 and f._resample == f._device_resample
    f.close()


# ------------------------------------------------------------------ dpf_rnn
@pytest.mark.parametrize("X,lw,message", _shared("log_weights") + LOG_WEIGHTS + [
    (Z((0, 4, 2)), Z((0, 4)), "the batch must hold 1 .. 65535 problems, got 0"),
    (Z((65536, 1, 1)), Z((65536, 1)), "the batch must hold 1 .. 65535 problems, got 65536"),
    (Z((1, 16385, 1)), Z((1, 16385)), "B N^2 = 268468225 is above the device limit of 268435456"),
    (Z((4097, 256, 1)), Z((4097, 256)), "B N^2 = 268500992 is above the device limit of 268435456"),
    (np.full((1, 16385, 1), np.nan), Z((1, 16385)), "B N^2 = 268468225 is above the device limit of 268435456"),
    (np.broadcast_to(0.0, (1, 16385, 1025)), Z((1, 16385)), "d = 1025 is above the device limit of 1024"),
])
def test_rnn_validate_shapes_and_values(X, lw, message):
    _raises(message, RN._validate, X, lw, 1.0)
    _raises(message, RN.rnn_resample, X, lw, [])


@pytest.mark.parametrize("T,message", [
    (0.0, "temperature must be positive, got 0.0"),
    (-1, "temperature must be positive, got -1"),
    (INF, "temperature must be positive, got inf"),
    (np.nan, "temperature must be positive, got nan"),
])
def test_rnn_validate_parameters(T, message):
    _raises(message, RN._validate, Z((2, 1)), Z(2), T)
    _raises(message, RN.rnn_resample, Z((2, 1)), Z(2), [], temperature=T)


def test_rnn_validate_returns_the_batched_arrays():
    X, lw, batched = RN._validate(Z((3, 2)), [0.0, -INF, -3.0], 1e-300)
    assert X.shape == (1, 3, 2) and lw.shape == (1, 3) and not batched
    assert X.dtype == lw.dtype == np.float64 and X.flags.c_contiguous and lw.flags.c_contiguous
    assert RN._validate(Z((1, 16384, 1)), Z((1, 16384)), 1.0)[2]  # B N^2 = 2^28 exactly


def test_rnn_constructor_and_function_arguments():
    F = RN.DifferentiableParticleFilterRNN
    _raises("need n_particles >= 1 and state_dim >= 1, got 0, 2", F, 0, 2, None, None)
    _raises("seed must be an integer in [0, 2^64), got 18446744073709551616", F, 3, 2, None, None, seed=1 << 64)
    _raises("Must use at least one of weight_features or particle_features", F, 3, 2, None, None,
            use_weight_features=False, use_particle_features=False)
    _raises("Unknown RNN type: rnn. Use 'lstm' or 'gru'", F, 3, 2, None, None, rnn_type="RNN")
    _raises("rnn_hidden_dim must be in 1 .. 128, got 129", F, 3, 2, None, None, rnn_hidden_dim=129)
    _raises("rnn_num_layers must be in 1 .. 4, got 0", F, 3, 2, None, None, rnn_num_layers=0)
    _raises("expected 5 weight arrays (kernel, recurrent_kernel, bias per layer, then the output kernel and bias), "
            "got 1", F, 3, 2, None, None, rnn_hidden_dim=4, weights=[Z(3)])
    _raises("Unknown RNN type: rnn. Use 'lstm' or 'gru'", RN.rnn_resample, Z((2, 1)), Z(2), [], rnn_type="rnn")
    _raises("weights must be kernel, recurrent_kernel, bias per layer, then the output kernel and bias",
            RN.rnn_resample, Z((2, 1)), Z(2), [])
    f = F(3, 2, None, None, use_baseline_resampling=True)
    _raises("the baseline resampler has no network", f.set_weights, [])
    _raises("particles must be (B, 3, 2), got (1, 4, 2)", f._baseline_resample, Z((1, 4, 2)), Z((1, 4)))
    assert f._h is None and f.epoch == 0 and f._resample == f._device_resample
    f.close()


# ------------------------------------------------------------------ one definition each
def test_the_shared_pieces_are_shared():
    assert SO._log_normalize is RN._log_normalize is DC.log_normalize
    assert SO.DifferentiableParticleFilter._log_normalize is DC.log_normalize
    assert RN.DifferentiableParticleFilterRNN._log_normalize is DC.log_normalize
    assert SO.MAX_DIM == RN.MAX_DIM == OT.MAX_DIM == 1024 and SO.MAX_BATCH == RN.MAX_BATCH == 65535
    for M in (OT, SO, RN):
        assert issubclass(M._Handle, DC.NativeHandle) and M._Handle.close is DC.NativeHandle.close
    for cls in (OT.DPF_OT, SO.DifferentiableParticleFilter, RN.DifferentiableParticleFilterRNN):
        assert cls.close is DC.HandleCache.close
