"""The host support header (particle_filters_amd/csrc/pf_host.h) and the LEDH layout, on the CPU.

`make -C particle_filters_amd/csrc hostcheck` builds tests/host/pf_host_check.cpp, a stand-alone
program with its own main, under AddressSanitizer + UndefinedBehaviorSanitizer.  It asserts the
exception boundary of the C ABI (an entry that throws returns PF_E_HIP and names itself), the shared
Cholesky / SPD inverse / is_diag on exact dyadic cases, the owning device pointer without a device,
and (at compile time) that LedhLay(nx, nz) is Lay<NX, NZ> / TLay<NX, NZ> for every compiled shape.
"""

import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "build", "pf_host_check")
# leak checking off as in test_host_asan.py (the HIP runtime keeps process-lifetime allocations)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def _run_check(exe):
    if not os.path.exists(exe):  # built by __graft_entry__.build(); here if the test runs first
        subprocess.run(["make", "-C", os.path.join(REPO, "particle_filters_amd", "csrc"), "hostcheck"],
                       check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_host_support_cpu():
    _run_check(EXE)


def test_ledh_run_plan_under_sanitizers():
    """The run bookkeeping of the LEDH / EDH engine flows (csrc/pf_ledh_run_plan.h) in a stand-alone program
    under the same sanitizers (tests/host/pf_ledh_run_plan_host_check.cpp): the mean ring of the fused run
    for every T from 1 to 40 against a brute-force model, the tracker-ahead chunk starts for every T from 1
    to 100, the arena layout at hand-computed shapes and past 2^32 bytes, and the EKF slots."""
    _run_check(os.path.join(REPO, "build", "pf_ledh_run_plan_host_check"))
