"""The reducer form of k_resident (pf_resident.h, RED) against the all-verify form (-m gpu).

In the reducer form one workgroup more per replicate reduces each step's records once - with the
code every workgroup of the all-verify form runs - and the compute workgroups verify from its
summary.  Nothing about the arithmetic changes, so the two forms must agree BITWISE: moments,
Neff, decisions, log normaliser, the final particles and the final log-weights.
PF_RES_REDUCER=0 forces the all-verify form; pf_last_run_reducer tells which form ran.

* the forms agree at one workgroup, a partial and a full last tile, many workgroups (with and
  without the regularisation jitter), two replicates, a run cut in two (exit header -> entry
  header) and the notebook driver with controls;
* a configuration whose G R workgroups fit the device but whose (G + 1) R do not stays on the
  resident path in the all-verify form, bitwise its single-replicate runs;
* a forced co-residency abort (the existing PF_TEST_ABORT hook) of the reducer form is repeated
  by pf_run, bitwise the undisturbed run.
"""

import numpy as np
import pytest

from particle_filters_amd import _native as NV, models as M, simulators as S
from particle_filters_amd.batch import ParticleFilterBatch

pytestmark = pytest.mark.gpu

T = 60


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert NV.device_count() > 0, "no HIP device visible: -m gpu tests must run on an MI355X"


@pytest.fixture(scope="module")
def data():
    d = S.simulate_sv_1d(T + 1, 0.95, 0.2, 1.0, seed=7)
    return d.X[0], np.log(d.Y[1:] ** 2)[:, None]


def make(N, R=1, reg=False, base=0):
    return ParticleFilterBatch(M.SVTransition(0.95), M.SVLogSqObservation(1.0), [[0.04]], [[M.LOGCHI2_VAR]], Np=N,
                               n_replicates=R, replicate_base=base, seed=42, regularize_after_resample=reg,
                               resample_thresh=0.7)


def state(pf):
    w, lw = np.empty((pf.n_replicates, pf.Np)), np.empty((pf.n_replicates, pf.Np))
    NV.check(NV.load().pf_get_weights(pf.handle, NV.dptr(w), NV.dptr(lw)), "pf_get_weights")
    return pf.particles(), lw


def run(monkeypatch, x0, Z, N, reducer, cuts=(), U=None, fo=False, expect=None, **kw):
    """One filter run (cut into consecutive pf.run calls at `cuts`) in the given form: the
    concatenated outputs and the final state."""
    monkeypatch.setenv("PF_RES_REDUCER", "1" if reducer else "0")
    pf = make(N, **kw)
    pf.initialize([x0], [[0.5]])
    parts = []
    edges = [0, *cuts, Z.shape[0]]
    for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        parts.append(pf.run(Z[lo:hi], None if U is None else U[lo:hi], first_update_only=fo and k == 0))
        assert pf.last_run_resident
        assert bool(NV.load().pf_last_run_reducer(pf.handle)) == (reducer if expect is None else expect)
    out = {f: np.concatenate([np.asarray(getattr(p, f)) for p in parts]) for f in ("means", "covs", "neff", "flags", "log_norm")}
    out["x"], out["lw"] = state(pf)
    pf.close()
    return out


def same(a, b):
    for f in a:
        assert np.array_equal(a[f], b[f]), f


CASES = {
    "one-workgroup": dict(N=1000),
    "partial-last-tile": dict(N=4096 * 3 + 5),
    "full-last-tile": dict(N=4096 * 4),
    "many-workgroups": dict(N=200_003),
    "many-workgroups-regularize": dict(N=200_003, reg=True),
    "two-replicates": dict(N=200_003, R=2),
    "cut-23-37": dict(N=200_003, cuts=(23,)),
    "first-update-only-controls": dict(N=100_000, fo=True, controls=True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_reducer_form_is_bitwise_the_all_verify_form(data, monkeypatch, case):
    x0, Z = data
    kw = dict(CASES[case])
    if kw.pop("controls", False):
        kw["U"] = 0.01 * np.sin(np.arange(T))[:, None]
    red = run(monkeypatch, x0, Z, reducer=True, **kw)
    old = run(monkeypatch, x0, Z, reducer=False, **kw)
    assert red["flags"].any(), "no resample in the run"
    assert np.all(np.isfinite(red["means"]))
    same(red, old)
    if kw.get("R", 1) > 1:
        assert not np.array_equal(red["means"][:, 0], red["means"][:, 1])


def test_grid_without_room_for_the_reducer_stays_resident(data, monkeypatch):
    """N = 4096 x 128, two replicates: 256 workgroups fill a 256-CU device, 258 do not fit.  The
    run keeps its one resident launch in the all-verify form and equals its single-replicate runs."""
    x0, Z = data
    N = 4096 * 128
    both = run(monkeypatch, x0, Z, N, reducer=True, expect=False, R=2)
    assert both["flags"].any()
    for r in range(2):
        one = run(monkeypatch, x0, Z, N, reducer=True, base=r)  # 129 workgroups: the reducer form
        for f in ("means", "covs", "neff", "flags", "log_norm"):
            assert np.array_equal(one[f][:, 0], both[f][:, r]), (f, r)
        assert np.array_equal(one["x"][0], both["x"][r]) and np.array_equal(one["lw"][0], both["lw"][r])


def test_forced_abort_of_the_reducer_form_repeats_bitwise(data, monkeypatch):
    """The existing hook: one workgroup arrives only after the others gave up, the launch aborts
    with the state untouched and pf_run repeats it (cooperatively)."""
    x0, Z = data
    ref = run(monkeypatch, x0, Z, 200_003, reducer=True)
    monkeypatch.setenv("PF_TEST_HOOKS", "1")
    monkeypatch.setenv("PF_TEST_ABORT", "1")
    got = run(monkeypatch, x0, Z, 200_003, reducer=True)
    assert ref["flags"].any()
    same(ref, got)
