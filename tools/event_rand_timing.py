"""What the per-episode domain randomisation costs on the stepwise path: the time of env.step() per env step,
with and without one reset-mode friction term, device events around blocks of back-to-back steps, median over the blocks.

    python tools/event_rand_timing.py --task elevation --layer on      # one JSON line
    python tools/event_rand_timing.py --task drift --layer off --root /path/to/another/tree

--root puts another checkout (built) in front of this one on sys.path: the same measurement of the same config on, say, the parent
commit, whose tree knows nothing of the layer (--layer off only).  Warm-up: the timed shape itself, `--warmup` steps, before the
first block (code objects load on first launch; every env has reset at least once by then at the default episode length)."""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", choices=("drift", "elevation"), required=True)
    ap.add_argument("--layer", choices=("on", "off"), default="off")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--root", default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.root or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path.insert(0, root)
    import torch

    import wheeledlab_amd.tasks  # noqa: F401
    from wheeledlab_amd import registry
    assert os.path.abspath(os.path.dirname(os.path.dirname(registry.__file__))) == root, "another tree was imported"
    assert torch.cuda.is_available(), "needs a GPU"
    task = {"drift": "Isaac-MushrDriftRL-v0", "elevation": "Isaac-MushrElevationRL-v0"}[a.task]
    cfg = registry.parse_env_cfg(task, device="cuda:0", num_envs=a.envs)
    cfg.seed = 7
    if a.layer == "on":
        cfg.events.change_wheel_friction.mode = "reset"
    env = registry.make(task, cfg=cfg)
    assert (getattr(env, "_event_rand", None) is not None) == (a.layer == "on")
    env.reset()
    g = torch.Generator(device="cuda:0").manual_seed(1)
    actions = torch.rand(a.steps, a.envs, 2, device="cuda:0", generator=g) * 2 - 1
    for k in range(a.warmup):
        env.step(actions[k % a.steps])
    torch.cuda.synchronize()
    times = []
    for _ in range(a.blocks):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for k in range(a.steps):
            env.step(actions[k])
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / a.steps)
    print(json.dumps(dict(task=a.task, layer=a.layer, envs=a.envs, tree=root, steps_per_block=a.steps, us_per_step=[round(t, 2) for t in times],
                          median_us=round(statistics.median(times), 2), min_us=round(min(times), 2), max_us=round(max(times), 2))), flush=True)


if __name__ == "__main__":
    main()
