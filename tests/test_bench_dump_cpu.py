"""bench.py --dump-outputs on host tensors: float32 files, one row per env, and above the byte budget the same seeded sample of
envs from every array (its indices in env_index.npy)."""
import numpy as np
import torch

import bench


def _arrays(n):
    g = torch.Generator().manual_seed(0)
    return {"obs": torch.rand(n, 14, generator=g), "reward": torch.rand(n, generator=g),
            "terminated": (torch.rand(n, generator=g) < 0.1).to(torch.uint8)}


def test_under_the_budget_every_env_is_written(tmp_path):
    a = _arrays(100)
    bench.dump_outputs(str(tmp_path), a, budget=1 << 20)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["obs.npy", "reward.npy", "terminated.npy"]
    for k, t in a.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, t.float().numpy()), k


def test_over_the_budget_a_fixed_sample_of_envs_is_written(tmp_path):
    n, budget = 5000, 40000
    a = _arrays(n)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), a, "_rank1", budget=budget)
    idx = np.load(tmp_path / "x" / "env_index_rank1.npy")
    assert idx.dtype == np.float64 and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < n
    total = 0
    for k, t in a.items():
        got = np.load(tmp_path / "x" / f"{k}_rank1.npy")
        assert got.dtype == np.float32 and np.array_equal(got, t.float().numpy()[idx.astype(np.int64)]), k
        assert np.array_equal(got, np.load(tmp_path / "y" / f"{k}_rank1.npy")), k
        total += got.nbytes
    assert total + idx.nbytes <= budget and len(idx) == budget // (4 * 16 + 8)
