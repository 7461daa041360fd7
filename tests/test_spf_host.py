"""CPU checks of the stochastic particle flow filter (no GPU).

* the two NumPy restatements (tests/spf_restatement.py) on the reference's draws against the
  reference's own runs (tests/golden/spf_runs.npz, tests/golden/make_golden_spf.py): the faithful
  one at 1e-12 x max(1, max|X|), the folded one - the affine form the device runs, through
  ``stochastic_pf.fold_steps`` - at 1e-11 x max(1, max|X|), the bounds the generator asserted
  (it measured at most 1.4e-14 and 7.1e-15);
* the schedule (lam, beta, betadot) bitwise equal to the reference's, and the ``schedule=`` checks;
* ``LinearGaussianBayes`` / ``kalman_posterior`` / ``kappa2_and_derivative`` against stored
  reference values (the same expressions in the same order: equal);
* the exact moments of the folded chain: first-order convergence to the Kalman posterior;
* the ValueError paths that need no device;
* the C ABI of include/pf_spf.h: the header parses to exactly the ``pf_spf_`` names of
  ``_native.SIGNATURES``, the library exports every name, and ``pf_spf_create``
  rejects bad arguments before it touches a device.
"""

import ctypes as C
import os
import re

import numpy as np
import pytest

from particle_filters_amd import _native as NV
from particle_filters_amd import stochastic_pf as SP
from tests import spf_restatement as SR

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "spf_runs.npz"))
NAMES = [str(n) for n in GOLD["names"]]


def test_golden_covers_the_cases():
    seen = set()
    for name in NAMES:
        model, kw, g = SR.golden_case(GOLD, name)
        d = "d1" if model.d == 1 else "full" if model.d == model.n else "partial"
        seen |= {kw["beta_mode"], kw["Q_mode"], d, f"steps{kw['n_steps']}" if kw["n_steps"] <= 2 else "steps"}
        assert kw["N"] <= 257 and model.n <= 9 and kw["n_steps"] <= 100
        assert np.linalg.cond(model.P0) <= 10.0 * (1 + 1e-12) and np.linalg.eigvalsh(model.R)[0] >= 0.1
        assert float(np.max(np.abs(g["X"]))) <= 100.0
    assert seen >= {"linear", "optimal", "scaled_identity", "inv_M", "d1", "partial", "full", "steps1", "steps2"}


@pytest.mark.parametrize("name", NAMES)
def test_numpy_stream_is_the_generators(name):
    """A failure here is a change of NumPy's stream, not of the filter."""
    model, kw, g = SR.golden_case(GOLD, name)
    draw = SR.numpy_draws(kw["seed"], kw["N"], model.n)
    assert np.array_equal(draw(0).ravel()[:4], g["first_normals"])
    for k in range(kw["n_steps"]):
        last = draw(k + 1).ravel()[-4:]
    assert np.array_equal(last, g["last_normals"])


@pytest.mark.parametrize("name", NAMES)
def test_restatements_match_reference(name):
    model, kw, g = SR.golden_case(GOLD, name)
    lam, beta, betadot = g["lam"], g["beta"], g["betadot"]
    scale = max(1.0, float(np.max(np.abs(g["X"]))))
    draw = SR.numpy_draws(kw["seed"], kw["N"], model.n)
    Xf = SR.faithful(model, SR.prior(model, draw), draw, lam, beta, betadot, kw["Q_mode"], kw["q_scale"])
    draw = SR.numpy_draws(kw["seed"], kw["N"], model.n)
    params = SP.fold_steps(model, lam, beta, betadot, kw["Q_mode"], kw["q_scale"])
    Xa = SR.folded(params, SR.prior(model, draw), draw, model.n)
    e_f, e_a = float(np.max(np.abs(Xf - g["X"]))), float(np.max(np.abs(Xa - g["X"])))
    print(f"{name}: faithful {e_f:.3e}, folded {e_a:.3e} (scale {scale:.3g})")
    assert params.shape == (kw["n_steps"], 2 * model.n ** 2 + model.n)
    assert e_f <= 1e-12 * scale
    assert e_a <= 1e-11 * scale
    assert np.max(np.abs(Xf.mean(axis=0) - g["x_hat"])) <= 1e-12 * scale


@pytest.mark.parametrize("name", NAMES)
def test_schedule_bitwise(name):
    model, kw, g = SR.golden_case(GOLD, name)
    lam, beta, betadot = SP._schedule(model, kw["n_steps"], kw["beta_mode"], kw["mu"], None)
    assert np.array_equal(lam, g["lam"]) and np.array_equal(beta, g["beta"]) and np.array_equal(betadot, g["betadot"])
    assert lam.dtype == beta.dtype == betadot.dtype == np.float64


def test_solver_signature_and_direct_call():
    model, kw, g = SR.golden_case(GOLD, "c_scaled_d1")
    lam, beta, betadot = SP.solve_beta_star_bisection(model.M0, model.Mh, kw["mu"], kw["n_steps"] + 1)
    assert np.array_equal(beta, g["beta"]) and np.array_equal(betadot, g["betadot"]) and np.array_equal(lam, g["lam"])
    assert beta[0] == 0.0 and beta[-1] == 1.0
    import inspect
    sig = inspect.signature(SP.solve_beta_star_bisection)
    assert list(sig.parameters) == ["M0", "Mh", "mu", "n_grid", "s_lo", "s_hi", "max_bracket_expand", "max_bisect_iter"]
    assert [p.default for p in sig.parameters.values()][3:] == [501, -5.0, 5.0, 30, 60]
    sig = inspect.signature(SP.run_generalized_spf)
    assert list(sig.parameters) == ["model", "N", "n_steps", "beta_mode", "mu", "Q_mode", "q_scale", "seed", "draws",
                                    "schedule", "device"]
    assert [p.default for p in sig.parameters.values()][1:] == [2000, 300, "optimal", 1e-2, "inv_M", 1e-2, 0, "philox",
                                                                None, 0]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("draws", "schedule", "device"))
    assert inspect.signature(SP.kappa2_and_derivative).parameters["eps"].default == 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_model_helpers_match_reference_values(name):
    model, _, g = SR.golden_case(GOLD, name)
    for k in ("P0_inv", "R_inv", "Hess_log_p0", "Hess_log_h", "M0", "Mh"):
        assert np.array_equal(getattr(model, k), g[k]), k
    mp, Pp = model.kalman_posterior()
    assert np.array_equal(mp, g["m_post"]) and np.array_equal(Pp, g["P_post"])
    kap = np.array([SP.kappa2_and_derivative(model.M0 + b * model.Mh, model.Mh) for b in (0.0, 0.3, 1.0)])
    assert np.array_equal(kap, g["kappa"])
    assert np.array_equal(model.grad_log_p0(model.m0 + 1.0), g["grad_p0"])
    assert np.array_equal(model.grad_log_h(model.m0 + 1.0), g["grad_h"])
    assert (model.n, model.d) == (g["m0"].size, g["z"].size)


def test_moments_of_the_folded_chain():
    """The continuous flow carries N(m0, P0) to the Kalman posterior and Euler-Maruyama is first
    order in the moments, so four times the steps must cut the distance of ``moments`` to the
    posterior by about four: the assertion allows a factor between 2 (order 1/2) and 8 (order
    3/2).  And ``moments`` equals the composition of the steps written out."""
    model = SR.random_model(5, 4, 2, 4.0)
    mp, Pp = model.kalman_posterior()
    err = []
    for steps in (100, 400):
        lam = np.linspace(0.0, 1.0, steps + 1)
        params = SP.fold_steps(model, lam, lam.copy(), np.ones_like(lam), "inv_M", 1e-2)
        m, P = SR.moments(params, model.m0, model.P0, 4)
        err.append((np.max(np.abs(m - mp)), np.max(np.abs(P - Pp))))
    print("distance to the Kalman posterior at 100 / 400 steps:", err)
    assert 2.0 < err[0][0] / err[1][0] < 8.0 and 2.0 < err[0][1] / err[1][1] < 8.0
    # the same recursion as one composed map on two steps
    A, c, G = SR.unpack(params[:2], 4)
    m2, P2 = SR.moments(params[:2], model.m0, model.P0, 4)
    assert np.allclose(m2, A[1] @ (A[0] @ model.m0 + c[0]) + c[1], rtol=0, atol=1e-14)
    assert np.allclose(P2, A[1] @ (A[0] @ model.P0 @ A[0].T + G[0] @ G[0].T) @ A[1].T + G[1] @ G[1].T, rtol=0,
                       atol=1e-14)
    assert np.all(np.triu(G[0], 1) == 0.0)


def test_sliced_philox_draws_are_the_oracles():
    """``philox_draws(rows=...)`` (the tail slices of tests/test_gpu_spf.py) against the full draw."""
    for n in (3, 8, 61):
        full, part = SR.philox_draws(9, 300, n), SR.philox_draws(9, 300, n, rows=(257, 300))
        head = SR.philox_draws(9, 300, n, rows=(0, 40))
        for k in (0, 1, 5):
            f = full(k)
            assert np.array_equal(part(k), f[257:300]) and np.array_equal(head(k), f[:40])


def test_value_errors_without_a_device():
    model = SR.random_model(1, 3, 2)
    with pytest.raises(ValueError, match="beta_mode must be 'linear' or 'optimal'"):
        SP.run_generalized_spf(model, N=4, n_steps=2, beta_mode="cubic")
    with pytest.raises(ValueError, match="Q_mode must be 'scaled_identity' or 'inv_M'"):
        SP.run_generalized_spf(model, N=4, n_steps=2, beta_mode="linear", Q_mode="full")
    with pytest.raises(ValueError, match="beta_mode"):  # both bad: the reference raises beta_mode first
        SP.run_generalized_spf(model, N=4, n_steps=2, beta_mode="cubic", Q_mode="full")
    with pytest.raises(ValueError, match="draws"):
        SP.run_generalized_spf(model, N=4, n_steps=2, beta_mode="linear", draws="pcg")
    lam = np.linspace(0.0, 1.0, 3)
    with pytest.raises(ValueError, match="n_steps \\+ 1"):
        SP.run_generalized_spf(model, N=4, n_steps=3, schedule=(lam, lam, np.ones(3)))
    with pytest.raises(ValueError, match="n_steps \\+ 1"):
        SP.run_generalized_spf(model, N=4, n_steps=2, schedule=(lam, lam, np.ones(4)))
    with pytest.raises(ValueError, match="Q_mode"):
        SP.step_matrices(model, 0.5, 1.0, "full", 1e-2)


# ----------------------------------------------------------------------------- C ABI
def header_functions():
    src = open(os.path.join(REPO, "include", "pf_spf.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_][A-Za-z0-9_]*\s*\*?\s*(pf_[a-z_0-9]+)\s*\(", src,
                                 flags=re.M)))


def test_spf_binding_covers_header_exactly():
    names = header_functions()
    spf = {n: v for n, v in NV.SIGNATURES.items() if n.startswith("pf_spf_")}
    assert names == sorted(spf)
    for must in ("pf_spf_create", "pf_spf_destroy", "pf_spf_supported", "pf_spf_set_particles", "pf_spf_draw_prior",
                 "pf_spf_advance", "pf_spf_get_particles", "pf_spf_workgroup", "pf_spf_stream", "pf_spf_synchronize"):
        assert must in names
    raw = C.CDLL(NV.LIB_PATH)
    assert not [n for n in names if not hasattr(raw, n)]
    lib = NV.load()
    for n, (res, args) in spf.items():
        assert getattr(lib, n).argtypes == args and getattr(lib, n).restype == res


def test_spf_supported_shapes():
    lib = NV.load()
    assert [n for n in range(-1, 70) if lib.pf_spf_supported(n)] == list(range(1, 65))


def _create(n_particles=10, n=3, null=None):
    o = NV.SpfOpts(n_particles, n, 0)
    hd = C.c_void_p()
    st = NV.load().pf_spf_create(None if null == "opts" else C.byref(o), None if null == "out" else C.byref(hd))
    return st, hd


def test_spf_create_rejects_bad_arguments_before_touching_a_device():
    lib = NV.load()
    for bad in (0, -5):
        st, hd = _create(n_particles=bad)
        assert st == NV.PF_E_ARG and not hd.value
        assert "n_particles" in lib.pf_last_error().decode()
    for bad in (0, 65, -1):
        st, hd = _create(n=bad)
        assert st == NV.PF_E_UNSUPPORTED and not hd.value
        with pytest.raises(NotImplementedError, match="1 <= n <= 64"):
            NV.check(st)
    st, hd = _create(n_particles=2**32, n=1)  # the Philox group index is 32 bits
    assert st == NV.PF_E_ARG and not hd.value
    st, hd = _create(n_particles=2**28, n=64)
    assert st == NV.PF_E_ARG and not hd.value
    for null in ("opts", "out"):
        assert _create(null=null)[0] == NV.PF_E_ARG
    assert lib.pf_spf_advance(None, None, 0, 1, 0, None) == NV.PF_E_ARG
    assert lib.pf_spf_set_particles(None, None) == NV.PF_E_ARG
    assert lib.pf_spf_get_particles(None, None) == NV.PF_E_ARG
    assert lib.pf_spf_draw_prior(None, None, None, 0) == NV.PF_E_ARG
    assert lib.pf_spf_synchronize(None) == NV.PF_E_ARG
    assert lib.pf_spf_stream(None) is None
    assert lib.pf_spf_workgroup(None) == 0
    lib.pf_spf_destroy(None)
