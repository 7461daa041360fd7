"""bench.py --dump-outputs (bench.dump_outputs): float64 files, the byte budget, and the same
trailing steps / seeded sample on every call."""

import os

import numpy as np

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole(tmp_path):
    means = np.arange(5 * 2 * 3, dtype=np.float32).reshape(5, 2, 3)
    flags = np.array([[1, 0]] * 5, dtype=np.int32)
    bench.dump_outputs(str(tmp_path), {"means": means, "flags": flags, "covs": None, "ess": np.arange(5.0)})
    out = _load(tmp_path)
    assert sorted(out) == ["ess", "flags", "means"]
    assert all(v.dtype == np.float64 for v in out.values())
    assert np.array_equal(out["means"], means) and np.array_equal(out["flags"], flags)
    assert out["ess"].shape == (5,)


def test_budget_keeps_trailing_steps_then_a_fixed_sample(tmp_path, monkeypatch):
    rng = np.random.default_rng(1)
    arrays = {"means": rng.normal(size=(50, 2, 3)), "covs": rng.normal(size=(50, 1000))}
    # 20 steps of 1006 doubles fit: the last 20 steps, whole
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 20 * 1006 * 8 + 100)
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    a = _load(tmp_path / "a")
    assert np.array_equal(a["covs"], arrays["covs"][30:]) and np.array_equal(a["means"], arrays["means"][30:])
    # one step alone does not fit: the last step, the wide array sampled at fixed indices
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    for sub in ("b", "c"):
        bench.dump_outputs(str(tmp_path / sub), arrays)
    b, c = _load(tmp_path / "b"), _load(tmp_path / "c")
    assert sorted(b) == ["covs", "covs_index", "means"]
    assert all(np.array_equal(b[k], c[k]) for k in b)
    idx = b["covs_index"].astype(int)
    assert np.all(np.diff(idx) > 0) and np.array_equal(b["covs"], arrays["covs"][49:, idx])
    assert np.array_equal(b["means"], arrays["means"][49:])
    assert sum(v.nbytes for v in b.values()) <= 4000
