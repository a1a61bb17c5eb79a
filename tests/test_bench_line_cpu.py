"""bench.py's plain-run line, built from a known wall time on the host: the contract keys, the roofline fraction that follows from
its own clock, and nothing measured beside the timed block (no side file unless one is asked for)."""
import argparse
import json

import torch

import bench


def test_plain_line_is_the_headline_and_its_clock(capsys, monkeypatch, tmp_path):
    monkeypatch.delenv("WL_BENCH_DETAIL", raising=False)
    args = argparse.Namespace(steps=20, warmup=5, full=False, detail_out=None, print_detail=False)
    metrics = torch.zeros(16)
    metrics[8], metrics[9], metrics[10] = 7, 3, 4
    wall = 20 * 7.0e-6
    bench.emit(bench.headline_record(args, 4096, 1, 128, wall, 0, None, metrics), args)
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and len(out[0]) < bench.MAX_LINE_BYTES
    line = json.loads(out[0])
    assert set(line) == {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                         "vs_baseline", "dtype", "data", "config", "roofline", "rccl", "episode_metrics", "detail"}
    assert line["value"] == 4096 * 20 / wall and line["ms_per_step"] == wall * 1e3 / 20 and line["unit"] == "env-steps/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["detail"] is None and line["rccl"] is None
    r = line["roofline"]
    assert r["frac"] == r["achieved"] / 8000.0 and abs(r["achieved"] - 334 * 4096 / (wall / 20) / 1e9) < 1e-9 * r["achieved"]
    assert r["regime"] == "latency" and r["bytes_per_env_step"] == 334 and r["envs_per_launch"] == 4096
    assert not {"launch_us", "frac_launch", "frac_profile", "frac_counters", "traffic"} & set(r)
    assert line["episode_metrics"] == {"resets": 7.0, "timeouts": 3.0, "out_of_bounds": 4.0, "nonfinite": 0.0}
    # asked for a side file, a plain run writes one and names it
    args.detail_out = str(tmp_path / "d.json")
    bench.emit(bench.headline_record(args, 4096, 1, 128, wall, 0, None, metrics), args)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert json.load(open(tmp_path / "d.json"))["value"] == line["value"] and line["detail"].endswith("d.json")
