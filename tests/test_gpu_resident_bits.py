"""The resident SV kernel keeps its bits (-m gpu).

tests/golden/resident_sv_bits.npz holds what the commit named in it computed for the runs of
tests/resident_bits_cases.py (made by tests/golden/make_golden_resident_bits.py on an MI355X).
The build in the tree must give the same bits: every step's mean, Neff, log normaliser and
resample flag, and the final particles, weights and log-weights (compared through SHA-256
digests of their bytes, and element by element for the first run).

The cases aim at the per-thread sums and the wave reductions of the step: a last tile with a
thread of one live and seven dead (l = -inf) slots and threads with none, several resamples, two
replicates, the regularisation jitter, a control input, first_update_only (no transition in step 0),
a step whose outlier observation makes most exp(l - max l) underflow, five particles, and both forms
of the kernel (PF_RES_REDUCER=0 and 1).
"""

import numpy as np
import pytest

from tests import resident_bits_cases as RB
from tests.conftest import load_golden
from particle_filters_amd import _native as NV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    assert NV.device_count() > 0, "no HIP device visible: -m gpu tests must run on an MI355X"
    g = load_golden("resident_sv_bits")
    assert len(str(g["commit"])) >= 7
    return g


@pytest.mark.parametrize("case", list(RB.CASES))
def test_resident_run_has_the_stored_bits(golden, monkeypatch, case):
    out = RB.run_case(case, monkeypatch.setenv)
    assert bool(out["resident"]) == bool(golden[f"{case}/resident"])
    assert out["flags"].any(), "no resample in the run"
    for f in RB.FIELDS:
        want = golden[f"{case}/{f}"]
        assert out[f].dtype == want.dtype and out[f].shape == want.shape, f
        steps = np.flatnonzero((out[f].view(np.uint8) != want.view(np.uint8)).reshape(RB.T, -1).any(axis=1))
        assert steps.size == 0, f"{f}: {steps.size} steps differ, the first is step {steps[0]}"
    if case == "base":
        for f in ("x", "w", "lw"):
            assert np.array_equal(out[f].view(np.uint64), golden[f"base/{f}"].view(np.uint64)), f
    for f in ("x", "w", "lw"):
        assert RB.digest(out[f]) == str(golden[f"{case}/{f}_sha256"]), f"final {f}"
