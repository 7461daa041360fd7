"""The runs of tests/test_gpu_resident_bits.py and of its fixture's generator
(tests/golden/make_golden_resident_bits.py): SV log-squared filters in fp32 on the resident kernel.

Np = 3 * 4096 + 17: the last tile has two full threads, one thread with a single live slot and
seven slots at l = -inf, and threads with no live slot at all (their maximum is -inf), so the
per-thread sums see every kind of slot.  Np = 5 is less than one thread's worth.
"""

import hashlib

import numpy as np

from particle_filters_amd import _native as NV, models as M, simulators as S
from particle_filters_amd.batch import ParticleFilterBatch

T = 48
NP = 3 * 4096 + 17
FIELDS = ("means", "neff", "log_norm", "flags")

# name -> (Np, replicates, regularize, controls, first_update_only, outlier, PF_RES_REDUCER)
CASES = {
    "base": (NP, 1, False, False, False, False, "1"),
    "base-all-verify": (NP, 1, False, False, False, False, "0"),
    "two-replicates": (NP, 2, False, False, False, False, "1"),
    "regularize": (NP, 1, True, False, False, False, "1"),
    "controls": (NP, 1, False, True, False, False, "1"),
    "first-update-only": (NP, 1, False, False, True, False, "1"),
    "outlier": (NP, 1, False, False, False, True, "1"),
    "five-particles": (5, 1, False, False, False, False, "1"),
}


def observations(outlier=False):
    d = S.simulate_sv_1d(T + 1, 0.95, 0.2, 1.0, seed=7)
    Z = np.log(d.Y[1:] ** 2)[:, None]
    if outlier:  # one observation far from every particle's: most l - max(l) underflow in that step
        Z = Z.copy()
        Z[20, 0] = 600.0
    return d.X[0], Z


def run_case(name, setenv):
    """One run on whichever library is loaded; `setenv(name, value)` sets an environment variable
    for the run (monkeypatch.setenv in the test).  Returns the per-step outputs, the final particles,
    weights and log-weights, and whether the resident kernel ran."""
    N, R, reg, controls, fo, outlier, reducer = CASES[name]
    setenv("PF_RES_REDUCER", reducer)
    x0, Z = observations(outlier)
    U = 0.01 * np.sin(np.arange(T))[:, None] if controls else None
    pf = ParticleFilterBatch(M.SVTransition(0.95), M.SVLogSqObservation(1.0), [[0.04]], [[M.LOGCHI2_VAR]], Np=N,
                             n_replicates=R, seed=42, regularize_after_resample=reg, resample_thresh=0.7)
    pf.initialize([x0], [[0.5]])
    res = pf.run(Z, U, first_update_only=fo)
    out = {f: np.asarray(getattr(res, f)) for f in FIELDS}
    out["resident"] = np.array(bool(pf.last_run_resident))
    w, lw = np.empty((R, N)), np.empty((R, N))
    NV.check(NV.load().pf_get_weights(pf.handle, NV.dptr(w), NV.dptr(lw)), "pf_get_weights")
    out["x"], out["w"], out["lw"] = pf.particles(), w, lw
    pf.close()
    return out


def digest(a):
    """The bytes of an array as a SHA-256: equal digests are equal bits."""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
