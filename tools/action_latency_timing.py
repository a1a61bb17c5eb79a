"""What action latency costs.  Two measurements, device events around blocks of back-to-back work after a
warm-up of the same shape, median (min - max) over the blocks:

    python tools/action_latency_timing.py --task elevation --layer on      # env.step() per env step, the layer at (1, 3); one JSON line
    python tools/action_latency_timing.py --task drift --layer off --root /path/to/another/tree
    python tools/action_latency_timing.py --task drift --launches          # the two launches alone against the same operation from torch ops

--root puts another checkout (built) in front of this one on sys.path: the same measurement of the same config on, say, the parent
commit, whose tree knows nothing of the layer (--layer off only).  --launches times, on one set of buffers of the task's shape,
(a) wl_action_latency_push + wl_action_latency_finish and (b) the composition a user has without them: a `gather` over the ring, `where`
on the flags, `clamp`, and slice writes into the row and the state (the lag redraw of reset envs is left out of the composition, which
flatters it)."""
import argparse
import json
import os
import statistics
import sys


def _blocks(torch, fn, blocks, steps, warmup):
    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    times = []
    for _ in range(blocks):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for k in range(steps):
            fn(k)
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / steps)
    return dict(us=[round(t, 2) for t in times], median_us=round(statistics.median(times), 2), min_us=round(min(times), 2), max_us=round(max(times), 2))


def _launches(torch, a, env):
    """the two launches and their torch composition on the env's own buffers (the env is not stepped: flags and actions are made up)"""
    from wheeledlab_amd import _abi as A
    from wheeledlab_amd.envs.latency import ActionLatency, LatencySpec
    b, n, dev = env._batch, env.num_envs, "cuda:0"
    L = ActionLatency(LatencySpec(1, 3, False, "throttle_steer"), b, task=env._task)
    L.reset_all()
    g = torch.Generator(device=dev).manual_seed(1)
    actions = torch.randn(a.steps, n, 2, device=dev, generator=g)
    term = torch.rand(a.steps, n, device=dev, generator=g) < 0.01
    trunc = torch.rand(a.steps, n, device=dev, generator=g) < 0.01
    row = b.obs

    def kernel(k):
        L.push(actions[k])
        L.finish(actions[k], row, term[k], trunc[k])

    slots, col = 4, L.col
    ring = torch.zeros(slots, n, 2, device=dev)
    lag = torch.randint(1, 4, (n, 2), device=dev, generator=g)
    head = torch.zeros((), dtype=torch.long, device=dev)
    applied = torch.zeros(n, 2, device=dev)
    zero = torch.zeros((), device=dev)

    def composed(k):
        act = actions[k]
        head.add_(1).remainder_(slots)
        ring[head] = act
        idx = (head - lag).remainder(slots)                                     # [n, 2]
        applied.copy_(ring.gather(0, idx.unsqueeze(0)).squeeze(0))
        reset = (term[k] | trunc[k]).unsqueeze(-1)
        b.state[A.S_ACT0:A.S_ACT0 + 2, :n] = torch.where(reset, zero, act).T
        row[:, col:col + 2] = torch.where(reset, zero, act.clamp(-1.0, 1.0))

    return dict(launches=_blocks(torch, kernel, a.blocks, a.steps, a.warmup), composition=_blocks(torch, composed, a.blocks, a.steps, a.warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", choices=("drift", "elevation"), required=True)
    ap.add_argument("--layer", choices=("on", "off"), default="off")
    ap.add_argument("--launches", action="store_true")
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
        cfg.actions.throttle_steer.latency = {"min_delay": 1, "max_delay": 3}
    env = registry.make(task, cfg=cfg)
    assert (getattr(env, "action_latency", None) is not None) == (a.layer == "on")
    env.reset()
    out = dict(task=a.task, envs=a.envs, tree=root, steps_per_block=a.steps)
    if a.launches:
        out.update(_launches(torch, a, env))
    else:
        g = torch.Generator(device="cuda:0").manual_seed(1)
        actions = torch.rand(a.steps, a.envs, 2, device="cuda:0", generator=g) * 2 - 1
        out.update(layer=a.layer, **_blocks(torch, lambda k: env.step(actions[k % a.steps]), a.blocks, a.steps, a.warmup))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
