"""CPU checks of the soft resampler's backward pass (no GPU).

* the closed-form backward the device implements (tests/dpf_soft_grad_restatement.py, both forms of
  glp) against PyTorch's CPU fp64 autograd of the literal forward on the same draws, on every PARITY
  case and on one case offset by 30.  Bounds: 1e-12 sc for g log_weights, sc being the size of the
  summed terms (the rounding of any summation order is about N 2^-53 sc, 3e-14 sc at N = 300), and
  1e-12 max(1, max|gX|) for gX;
* the host chain of the module (``dpf_soft._log_weights_grad``) against the same reference, and its
  exact zeros: ``soft_alpha = 1``, a log-weight of -inf;
* the argument errors of ``soft_resample_vjp`` and of the torch wrapper, which answer before the
  library is loaded;
* ``import particle_filters_amd`` does not import torch.
"""

import subprocess
import sys

import numpy as np
import pytest
import torch

from particle_filters_amd import _native as NV
from particle_filters_amd import dpf_soft as SO
from particle_filters_amd import dpf_soft_torch as ST
from tests import dpf_soft_grad_restatement as GR
from tests import dpf_soft_restatement as R
from tests.conftest import REPO

CASES = [c + (0.0,) for c in R.PARITY] + [GR.OFFSET_CASE + (30.0,)]
IDS = [f"N{c[0]}-d{c[1]}-a{c[2]}-T{c[3]}-{c[4]}-off{c[7]:g}" for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_closed_form_equals_autograd(case):
    N, d, alpha, T = case[:4]
    ref = GR.autograd(*case)
    cf = GR.closed_form(ref["X"], ref["lw"], ref["gXo"], alpha, T, ref["A"])
    sc, sx = ref["sc"], max(1.0, float(np.max(np.abs(ref["gX"]))))
    ex = float(np.max(np.abs(cf["gX"] - ref["gX"])))
    ea = float(np.max(np.abs(cf["glw_pairs"] - ref["glw"])))
    eb = float(np.max(np.abs(cf["glw_sums"] - ref["glw"])))
    # the module's own host chain on the closed form's glp
    em = float(np.max(np.abs(SO._log_weights_grad(ref["lw"][None], alpha, cf["glp_sums"][None])[0] - ref["glw"])))
    print(f"soft grad host N={N} d={d} alpha={alpha} T={T} {case[4]} offset={case[7]:g}: gX error {ex:.3e} "
          f"(scale {sx:.3g}), g log_weights error pairs {ea:.3e} sums {eb:.3e} module chain {em:.3e} "
          f"(sc {sc:.3g}, max|g log_weights| {np.max(np.abs(ref['glw'])):.3e})")
    assert ex <= 1e-12 * sx
    assert ea <= 1e-12 * sc and eb <= 1e-12 * sc and em <= 1e-12 * sc


def test_alpha_one_gives_exactly_zero():
    X, lw = R.make_case(24, 3, seed=1)
    glp = np.random.default_rng(5).standard_normal((2, 24))
    g = SO._log_weights_grad(np.stack([lw, lw + 3.0]), 1.0, glp)
    assert g.shape == (2, 24) and np.all(g == 0.0)
    assert np.all(GR.chain(lw, 1.0, glp[0]) == 0.0)
    # and autograd agrees: with alpha = 1 the log-weights do not enter
    for case in R.PARITY:
        if case[2] == 1.0:
            assert np.all(GR.autograd(*case)["glw"] == 0.0)


def test_minus_inf_log_weight_gets_exactly_zero_and_the_rest_is_finite():
    N, d, alpha, T = 17, 3, 0.1, 0.2
    X, lw = R.make_case(N, d, seed=2)
    lw = lw.copy()
    lw[[3, 11]] = -np.inf
    res = R.soft_resample(X, lw, alpha, T, 4, 1, 0)
    gXo = GR.grad_out(N, d)
    cf = GR.closed_form(X, lw, gXo, alpha, T, res["A"])
    g = SO._log_weights_grad(lw[None], alpha, cf["glp_sums"][None])[0]
    assert g[3] == 0.0 and g[11] == 0.0
    assert np.all(np.isfinite(g)) and np.max(np.abs(g)) > 0.0
    assert np.array_equal(g == 0.0, np.isinf(lw))
    # autograd of the literal forward on the finite slots
    Xt = torch.tensor(X, requires_grad=True)
    lwt = torch.tensor(lw, requires_grad=True)
    GR.torch_forward(Xt, lwt, alpha, T, torch.from_numpy(res["G"])).backward(torch.from_numpy(gXo))
    ref = lwt.grad.numpy()
    fin = np.isfinite(lw)
    sc = GR.scale(X, gXo, T, res["A"])
    assert np.max(np.abs(g[fin] - ref[fin])) <= 1e-12 * sc


# ------------------------------------------------------------------ argument errors, no library
def _no_load(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(NV, "load", no_load)


_SAVED = SO.SoftSaved(np.zeros((1, 4, 2)), np.zeros((1, 4)), np.ones((1, 4)), 0, 0)


@pytest.mark.parametrize("particles,log_weights,grad,kw", [
    (np.zeros((4, 2)), np.zeros(5), np.zeros((4, 2)), {}),                       # _validate's checks still apply
    (np.zeros((4, 2)), np.zeros(4), np.zeros((4, 2)), {"soft_alpha": 1.5}),
    (np.zeros((4, 2)), np.zeros(4), np.zeros((4, 2)), {"gumbel_temperature": 0.0}),
    (np.zeros((4, 2)), np.zeros(4), np.zeros((4, 2)), {"epoch": 1 << 32}),
    (np.zeros((4, 2)), np.zeros(4), np.zeros((4, 3)), {}),                       # the gradient's shape
    (np.zeros((4, 2)), np.zeros(4), np.zeros((1, 4, 2)), {}),
    (np.zeros((1, 4, 2)), np.zeros((1, 4)), np.zeros((4, 2)), {}),
    (np.zeros((4, 2)), np.zeros(4), np.full((4, 2), np.nan), {}),                # and its finiteness
    (np.zeros((4, 2)), np.zeros(4), np.full((4, 2), np.inf), {}),
    (np.zeros((4, 2)), np.zeros(4), np.zeros((4, 2)), {"saved": (1, 2, 3)}),     # not a SoftSaved
    (np.zeros((5, 2)), np.zeros(5), np.zeros((5, 2)), {"saved": _SAVED}),        # saved of another shape
    (np.zeros((4, 2)), np.zeros(4), np.zeros((4, 2)), {"saved": _SAVED, "seed": 1}),   # of other draws
    (np.zeros((4, 2)), np.zeros(4), np.zeros((4, 2)), {"saved": _SAVED, "epoch": 2}),
    (np.zeros((4, 2)), np.zeros(4), np.zeros((4, 2)), {"saved": _SAVED._replace(row_sum=np.zeros((1, 4)))}),
    (np.zeros((4, 2)), np.zeros(4), np.zeros((4, 2)), {"saved": _SAVED._replace(row_max=np.full((1, 4), np.nan))}),
])
def test_vjp_validation_raises_before_the_library_is_loaded(monkeypatch, particles, log_weights, grad, kw):
    _no_load(monkeypatch)
    with pytest.raises(ValueError):
        SO.soft_resample_vjp(particles, log_weights, grad, **kw)


def test_torch_wrapper_argument_errors_before_the_library_is_loaded(monkeypatch):
    _no_load(monkeypatch)
    x, w = torch.zeros((4, 2), dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    for bad_x, bad_w in ((x.float(), w), (x, w.float()), (x.half(), w), (x.to(torch.int64), w), (x.numpy(), w)):
        with pytest.raises(TypeError):
            ST.soft_resample(bad_x, bad_w)
    with pytest.raises(TypeError):
        ST.soft_resample(x, w, torch.tensor(0.1, dtype=torch.float64), 0.2)
    with pytest.raises(TypeError):
        ST.soft_resample(x, w, 0.1, torch.tensor(0.2, dtype=torch.float64))
    for kw in ({"soft_alpha": -0.1}, {"gumbel_temperature": 0.0}, {"seed": -1}, {"epoch": 0.5}):
        with pytest.raises(ValueError):
            ST.soft_resample(x, w, **kw)
    with pytest.raises(ValueError):
        ST.soft_resample(x, torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError):
        ST.soft_resample(torch.full((4, 2), float("nan"), dtype=torch.float64), w)
    flt = ST.DifferentiableParticleFilter(4, 2, lambda p, params: p, lambda p, y, params: p.sum(-1), seed=3,
                                          rng=np.random.default_rng(0))
    p0, lw0 = flt.init_particles(2, np.zeros(2), np.eye(2))
    assert p0.shape == (2, 4, 2) and p0.dtype == torch.float64 and lw0.shape == (2, 4)
    with pytest.raises(TypeError):
        flt.step(p0.float(), lw0, torch.zeros(2, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        flt.step(torch.full((2, 4, 2), float("inf"), dtype=torch.float64), lw0, torch.zeros(2, 2, dtype=torch.float64))
    assert flt.epoch == 0  # a failed step does not advance the epoch
    with pytest.raises(ValueError):
        ST.DifferentiableParticleFilter(0, 2, None, None)


def test_default_arguments_leave_soft_resample_as_it_was():
    """``return_saved`` is keyword-only and off by default: two or three return values, as before."""
    import inspect
    sig = inspect.signature(SO.soft_resample)
    assert sig.parameters["return_saved"].default is False
    assert sig.parameters["return_saved"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig.parameters)[:4] == ["particles", "log_weights", "soft_alpha", "gumbel_temperature"]
    vjp = inspect.signature(SO.soft_resample_vjp)
    assert list(vjp.parameters)[:5] == ["particles", "log_weights", "grad_new_particles", "soft_alpha",
                                        "gumbel_temperature"]
    assert (vjp.parameters["soft_alpha"].default, vjp.parameters["gumbel_temperature"].default) == (0.1, 0.2)
    assert all(vjp.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("seed", "epoch", "saved", "device"))
    assert {"pf_soft_row_stats", "pf_soft_backward"} <= set(NV.SIGNATURES)


def test_the_package_imports_without_torch():
    code = ("import sys; import particle_filters_amd; from particle_filters_amd import dpf_soft; "
            "assert 'torch' not in sys.modules, 'torch was imported'; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
