#!/usr/bin/env python3
"""How long a terrain change takes on the device, beside one PPO iteration (procedural terrains):

  regenerate   DeviceHeightField.regenerate(seed) of the default 800 x 800 TerrainGeneratorCfg with one DepthCamera on the field: tile
               table on the host, descriptor upload, wl_terrain_generate, wl_heightfield_pairs, the decoded heights, the pyramid
  parent path  what changing the terrain took before the generator: terrain.synthetic_heightfield(seed) on the host, a new
               DeviceHeightField (quantise, upload, pairs) and a new DepthCamera (pyramid)
  iteration    one elevation PPO iteration (collection + update) at 4096 envs, as scripts/train_rl.py -r RSS_ELEV_CONFIG runs it

Wall clock around work that ends in a device synchronise; prints one JSON line.

    python tools/terrain_regen_timing.py [--reps 200] [--iterations 8]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, sync):
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--parent-reps", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--num-envs", type=int, default=4096)
    args = ap.parse_args()

    import torch

    from wheeledlab_amd.core import DepthCamera, DeviceHeightField, _launch_terrain_generator, generate_heightfield
    from wheeledlab_amd.envs.terrain_gen_cfg import TerrainGeneratorCfg
    from wheeledlab_amd.terrain import synthetic_heightfield

    dev = "cuda:0"
    sync = torch.cuda.synchronize
    cfg = TerrainGeneratorCfg(seed=0)
    hf = generate_heightfield(cfg, dev)
    cam = DepthCamera(hf, dev)
    seeds = iter(range(1, 10 ** 9))
    for _ in range(10):
        hf.regenerate(next(seeds))
    regen = timed(lambda: hf.regenerate(next(seeds)), args.reps, sync)
    launch = timed(lambda: _launch_terrain_generator(cfg, hf.codes), args.reps, sync)            # table + upload + the generator alone
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sync()
    e0.record()
    for _ in range(args.reps):
        hf.regenerate(next(seeds))
    e1.record()
    sync()
    back_to_back = e0.elapsed_time(e1) * 1e-3 / args.reps

    def parent(seed):
        field = DeviceHeightField(synthetic_heightfield(seed=seed), dev)
        return DepthCamera(field, dev)
    parent(1)
    old = timed(lambda: parent(next(seeds) % 1000), args.parent_reps, sync)
    host_only = timed(lambda: synthetic_heightfield(seed=next(seeds) % 1000), args.parent_reps, lambda: None)
    del cam

    from wheeledlab_amd import registry
    from wheeledlab_amd.configs.runs import resolve_run
    from wheeledlab_amd.rl import ClipAction, RslRlVecEnvWrapper
    from wheeledlab_amd.rl.ppo import OnPolicyRunner
    run = resolve_run("RSS_ELEV_CONFIG", [f"env_setup.num_envs={args.num_envs}", "train.log.no_log=true", "train.log.no_checkpoints=true"])
    torch.manual_seed(run.train.seed)
    env = registry.make(run.env_setup.task_name, cfg=run.env)
    env.action_space.low, env.action_space.high = -1.0, 1.0
    env = RslRlVecEnvWrapper(ClipAction(env))
    runner = OnPolicyRunner(env, run.agent, log_dir=None, device=run.train.device)
    env.seed(run.agent.seed)
    hist = runner.learn(args.iterations, verbose=False)
    its = [h["collection_time"] + h["learn_time"] for h in hist[2:]]                              # the first two warm up

    ms = lambda v: round(1e3 * v, 4)
    print(json.dumps({"field": "800x800", "reps": args.reps,
                      "regenerate_ms_median": ms(statistics.median(regen)), "regenerate_ms_mean": ms(statistics.mean(regen)),
                      "regenerate_ms_min": ms(min(regen)), "regenerate_back_to_back_ms": ms(back_to_back),
                      "generate_only_ms_median": ms(statistics.median(launch)),
                      "parent_path_ms_median": ms(statistics.median(old)), "parent_path_ms_min": ms(min(old)),
                      "parent_host_synthetic_ms_median": ms(statistics.median(host_only)),
                      "elev_iteration_ms_median": ms(statistics.median(its)), "elev_iteration_ms_all": [ms(v) for v in its],
                      "elev_num_envs": args.num_envs, "steps_per_env": runner.num_steps_per_env}))


if __name__ == "__main__":
    main()
