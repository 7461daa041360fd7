"""The index maps of the RNN resampler's weight packing, on the CPU.

``csrc/pf_rnn_plan.h`` states once, as ``__host__ __device__`` functions, where every element of the
packed buffers (W0x, W0i, binit, the MFMA fragments and their transposed set) comes from in the
Keras arrays; ``k_rnn_pack`` and ``k_rnn_pack_T`` evaluate those maps on the device
(``pf_rnn_set_weights_dev``).  ``tests/host/pf_rnn_pack_check.cpp`` is a stand-alone program (its own
``main``, plain C++ for the host, AddressSanitizer and UndefinedBehaviorSanitizer, no device and no
preloaded library) that evaluates them against the packing loops of ``pf_rnn_set_weights``, kept
there as the fixed statement of the layout: every H in 1 .. 128, L in 1 .. 4, both cells, the three
feature settings and N in {1, 5, 17}; byte equality, no map pointing outside its array, and every
destination element zero or from exactly one source element (two for the GRU's summed biases).

On the device the same maps are checked end to end by tests/test_gpu_dpf_dev_entries.py.
"""

import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _program():
    exe = os.path.join(REPO, "build", "pf_rnn_pack_check")
    if not os.path.exists(exe):  # built by __graft_entry__.build(); here if the test runs first
        subprocess.run(["make", "-C", os.path.join(REPO, "particle_filters_amd", "csrc"), "hostcheck"],
                       check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:quarantine_size_mb=8",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)


def test_the_index_maps_are_the_packing_loops_under_sanitizers():
    r = _program()
    assert r.returncode == 0, r.stdout + r.stderr
    # 128 hidden sizes x 4 layer counts x 2 cells x 3 feature settings x 3 particle counts
    assert r.stdout.strip() == f"{128 * 4 * 2 * 3 * 3} cases ok", r.stdout + r.stderr


def test_the_maps_are_shared_by_the_kernels_and_the_host_check():
    """One statement of the layout: the kernels call the maps of pf_rnn_plan.h, and so does the check."""
    csrc = os.path.join(REPO, "particle_filters_amd", "csrc")
    kernels = open(os.path.join(csrc, "pf_rnn_kernels.h")).read()
    check = open(os.path.join(REPO, "tests", "host", "pf_rnn_pack_check.cpp")).read()
    for name in ("pack_src_W0x", "pack_src_W0i", "pack_src_binit", "pack_src_frag", "pack_fragT_from_frag"):
        assert name + "(" in kernels, name
        assert name in check, name
    assert "k_rnn_pack_T" in open(os.path.join(csrc, "pf_rnn.hip")).read()
