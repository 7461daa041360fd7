"""What the GPU tests of the OT device entries and of the one-launch solver rest on, on the CPU.

tests/test_gpu_dpf_ot_resident.py compares the one-launch solver (PF_OT_RESIDENT, N <= 128) with the
NumPy restatement under "iteration counts equal, results within 1e-9 of the scales".  Here the
restatement (tests/dpf_ot_restatement.py, imported) is asked what makes that well defined for each of
its cases: the full-length cases run all their iterations with every convergence check far from tol;
the early-stop batches stop where stated, with the margin tests/test_dpf_ot_host.py asks for; the floor
case that fits the solver has exactly one floored column in every g pass, and no column sum near
min_val; the plan statistics' count is compared only where no plan entry is within 1e-12 of the
sparsity threshold.  Also the argument errors of the torch binding that need no GPU, and the
stand-alone sanitizer check of the solver's LDS plan (tests/host/pf_ot_resident_plan_check.cpp).
"""

import os
import subprocess

import numpy as np
import pytest

from tests import dpf_ot_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-6

# the cases of tests/test_gpu_dpf_ot_resident.py
FULL = [(3, 1, 0.1, 50, 0), (33, 1, 0.1, 50, 0), (64, 2, 0.1, 50, 0), (100, 2, 0.1, 50, 0), (128, 3, 0.1, 50, 0),
        (128, 17, 1.0, 50, 0), (63, 40, 2.0, 50, 0), (100, 65, 4.0, 50, 0)]
EARLY_BATCHES = [(128, 3, ((1, 33), (4, 34), (13, 38))), (100, 2, ((4, 32), (7, 36), (10, 33)))]


def _margin(hist):
    return min(min(abs(e["f_change"] - TOL), abs(e["g_change"] - TOL)) for e in hist)


@pytest.mark.parametrize("case", FULL, ids=lambda c: f"N{c[0]}-d{c[1]}")
def test_full_length_cases_run_every_iteration_far_from_tol(case):
    N, d, eps, n_iters, seed = case
    X, w, r = R.solved(N, d, eps, n_iters, 1.0, 1.0, seed)
    hist = r["diagnostics"]["convergence_history"]
    m = _margin(hist)
    print(f"full N={N} d={d}: {r['iterations']} iterations, smallest |change - tol| = {m / TOL:.3g} tol")
    assert r["iterations"] == n_iters and len(hist) == n_iters - 1
    assert m >= 2e3 * TOL
    assert np.all(np.isfinite(r["particles"]))


@pytest.mark.parametrize("batch", EARLY_BATCHES, ids=lambda b: f"N{b[0]}-d{b[1]}")
def test_early_stop_batches_stop_where_stated_with_a_margin(batch):
    N, d, seeds = batch
    for seed, stop in seeds:
        X, w, r = R.solved(N, d, 0.1, R.EARLY_ITERS, 0.2, 1.0, seed)
        m = _margin(r["diagnostics"]["convergence_history"])
        print(f"early N={N} d={d} seed {seed}: stops at {r['iterations']}, smallest |change - tol| = {m / TOL:.3g} tol")
        assert r["iterations"] == stop
        assert m >= 1e-3 * TOL
    assert len({s for _, s in seeds}) == 3  # a batch whose problems stop at different iterations


def floor_case():
    X, w = R.weight_case("zeros", N=100, d=3, seed=7)
    X, w = X.copy(), 37.5 * w
    X[99] = (-25.0, 10.0, 5.0)
    w[99] = 0.0
    return X, w, 0.1, 50


def test_the_floor_case_has_one_floored_column_with_room():
    X, w, eps, n_iters = floor_case()
    sums = []
    r = R.sinkhorn_resample(X, w, eps, n_iters, col_sums=sums)
    S = np.array(sums)
    assert S.shape == (n_iters, 100) and r["iterations"] == n_iters
    below = S < 1e-12
    near = float(np.min(np.abs(S / 1e-12 - 1.0)))
    print(f"floor N=100: columns below min_val per iteration {below.sum(axis=1).min()}..{below.sum(axis=1).max()}, "
          f"nearest relative distance to the floor {near:.3g}")
    assert np.all(below.sum(axis=1) == 1) and np.all(below[:, 99])
    assert near >= 0.5
    assert _margin(r["diagnostics"]["convergence_history"]) >= 1e-3 * TOL


def test_some_cases_pass_the_sparsity_gap_and_the_others_are_skipped_by_it():
    """The count of P > 1e-6 is compared on the device only where the restatement has no plan entry
    within 1e-12 of the threshold; the GPU test applies this condition per case."""
    gaps = {}
    for N, d, eps, n_iters, seed in FULL:
        r = R.solved(N, d, eps, n_iters, 1.0, 1.0, seed)[2]
        gaps[(N, d)] = float(np.min(np.abs(r["P"] - 1e-6)))
    print("sparsity gaps:", {k: f"{v:.2e}" for k, v in gaps.items()})
    assert sum(g > 1e-12 for g in gaps.values()) >= 3


def test_argument_errors_of_the_torch_binding_that_need_no_gpu():
    torch = pytest.importorskip("torch")
    from particle_filters_amd import dpf_ot_torch as TT

    x, w = torch.zeros(129, 2, dtype=torch.float64), torch.full((129,), 1.0 / 129, dtype=torch.float64)
    with pytest.raises(ValueError, match=r'solver="resident" needs N <= 128, got N = 129'):
        TT.sinkhorn_ot_resample(x, w, solver="resident", device_path=True)
    with pytest.raises(ValueError, match=r'solver="resident" needs device_path=True'):
        TT.sinkhorn_ot_resample(x[:100], w[:100], solver="resident")
    with pytest.raises(ValueError, match="needs every tensor on the device that computes"):
        TT.sinkhorn_ot_resample(x[:100], w[:100], solver="resident", device_path=True)
    with pytest.raises(ValueError, match="solver must be one of"):
        TT.sinkhorn_ot_resample(x[:100], w[:100], solver="auto")
    with pytest.raises(ValueError, match=r'solver="resident" needs N <= 128'):
        TT.DPF_OT(129, 2, None, None, solver="resident", device_path=True)
    with pytest.raises(ValueError, match=r'solver="resident" needs device_path=True'):
        TT.DPF_OT(100, 2, None, None, solver="resident")


def test_the_lds_plan_of_the_one_launch_solver_under_sanitizers():
    exe = os.path.join(REPO, "build", "pf_ot_resident_plan_check")
    if not os.path.exists(exe):  # built by __graft_entry__.build(); here if the test runs first
        subprocess.run(["make", "-C", os.path.join(REPO, "particle_filters_amd", "csrc"), "hostcheck"],
                       check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"{128 + 5} cases ok", r.stdout + r.stderr  # N = 1 .. 128 and five refused sizes


def test_the_plan_is_shared_by_the_kernel_the_host_and_the_check():
    csrc = os.path.join(REPO, "particle_filters_amd", "csrc")
    for path in (os.path.join(csrc, "pf_ot_resident.h"), os.path.join(csrc, "pf_ot.hip"),
                 os.path.join(REPO, "tests", "host", "pf_ot_resident_plan_check.cpp")):
        assert "resident_plan(" in open(path).read(), path
