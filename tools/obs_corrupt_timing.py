#!/usr/bin/env python3
"""What the observation-corruption launch costs on the device:

  launch       wl_obs_corrupt_apply alone at 4096 envs on the drift layout (14: Gaussian, Gaussian, uniform, Gaussian + a per-episode
               uniform bias, last_action clipped from the state), the elevation layout (689: a Gaussian on every term, the shipped
               clips) and the visual layout (3208: the declared Unoise on the three proprioceptive terms, the image untouched): time per
               launch, bytes moved (every row word read once and written once, the flags, the action rows, the bias block) over that
               time, and that rate as a share of the HBM rate the chip sustains (6.3 TB/s)
  composition  the same operation composed from torch ops on the same buffers -- per noisy term rand_like / randn_like, a multiply-add,
               the add onto the slice, clamp, mul, for the bias a where on the flags, and a cat into the output: what a user has without
               the launch (torch's generator: other numbers, the same work)

Device events around windows of back-to-back launches that alternate between two output buffers, after a warm-up; median and spread
over the windows.  Prints one JSON line.

    python tools/obs_corrupt_timing.py [--windows 30] [--launches 50] [--num-envs 4096]"""
import argparse
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE = 6.3e12      # bytes / s


def windows(fn, n_windows, launches):
    """seconds per call of fn(i) over n_windows event-timed windows of `launches` calls"""
    import torch
    for i in range(2 * launches):
        fn(i)
    out = []
    for _ in range(n_windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(launches):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3 / launches)
    return out


def summary(ts, nbytes):
    med = statistics.median(ts)
    return {"us_median": round(med * 1e6, 3), "us_min": round(min(ts) * 1e6, 3), "us_max": round(max(ts) * 1e6, 3),
            "TB_per_s": round(nbytes / med * 1e-12, 3), "share_of_6.3_TB_per_s": round(nbytes / med / HBM_ACHIEVABLE, 3)}


def layouts():
    """name -> [(width, noise, bias, clip, from_state)]: noise / bias ("g", mean, std) | ("u", lo, hi) | None"""
    g, u = (lambda m, s: ("g", m, s)), (lambda a, b: ("u", a, b))
    return {
        "drift": [(3, g(0.0, 0.1), None, None, False), (3, g(0.0, 0.1), None, None, False), (3, u(-0.1, 0.1), None, None, False),
                  (3, g(0.0, 0.4), u(-0.05, 0.05), None, False), (2, None, None, (-1.0, 1.0), True)],
        "elevation": [(2, g(0.0, 0.05), None, None, False), (3, g(0.0, 0.02), None, None, False), (3, g(0.0, 0.1), None, (-10.0, 10.0), False),
                      (3, g(0.0, 0.1), None, (-10.0, 10.0), False), (2, g(0.0, 0.05), None, (-1.0, 1.0), True),
                      (676, g(0.0, 0.02), None, (-10.0, 10.0), False)],
        "visual": [(3200, None, None, None, False), (3, u(-0.1, 0.1), None, None, False), (3, u(-0.1, 0.1), None, None, False),
                   (2, u(-0.1, 0.1), None, (-1.0, 1.0), True)],
    }


def table(spec):
    """-> CorruptionLayout of a spec"""
    import numpy as np

    from wheeledlab_amd import _abi as A
    from wheeledlab_amd.envs.corruption import CorruptionLayout

    def kind(v):
        if v is None:
            return A.OC_NONE, 0.0, 0.0
        if v[0] == "g":
            return A.OC_GAUSSIAN, float(np.float32(v[1])), float(np.float32(v[2]))
        return A.OC_UNIFORM, float(np.float32(v[1])), float(np.float32(v[2]) - np.float32(v[1]))
    rows, off, boff = [], 0, 0
    for w, noise, bias, clip, from_state in spec:
        nk, na, nb = kind(noise)
        bk, ba, bb = kind(bias)
        lo, hi = clip or (-float("inf"), float("inf"))
        rows.append((off, w, nk, A.OC_ADD, na, nb, bk, 1, ba, bb, boff, 0, lo, hi, 1.0, A.S_ACT0 if from_state else -1))
        off += w
        boff += w if bias is not None else 0
    return CorruptionLayout(tuple(rows), tuple(str(i) for i in range(len(rows))), off, boff, True)


def composition(spec, obs, state, bias, reset, out):
    """the same work from torch ops: draw, combine, clamp, where on the flags for the bias, cat into `out`"""
    import torch
    from wheeledlab_amd import _abi as A

    def draw(v, like):
        if v[0] == "g":
            return torch.randn_like(like) * v[2] + v[1]
        return torch.rand_like(like) * (v[2] - v[1]) + v[1]
    parts, off, boff = [], 0, 0
    for w, noise, b, clip, from_state in spec:
        x = state[A.S_ACT0:A.S_ACT0 + w, :obs.shape[0]].T if from_state else obs[:, off:off + w]
        if noise is not None:
            x = x + draw(noise, x)
            if b is not None:
                held = bias[:, boff:boff + w]
                held.copy_(torch.where(reset.unsqueeze(-1), draw(b, held), held))
                x = x + held
                boff += w
        if clip is not None:
            x = x.clamp(clip[0], clip[1])
        parts.append(x)
        off += w
    return torch.cat(parts, dim=-1, out=out)


def case(name, spec, n, args):
    import torch

    from wheeledlab_amd import _abi as A
    from wheeledlab_amd.envs.corruption import ObsCorruption
    dev = torch.device("cuda:0")
    layout = table(spec)
    g = torch.Generator(device=dev).manual_seed(0)
    state = torch.randn(A.S_COUNT, n, device=dev, generator=g)
    batch = types.SimpleNamespace(n=n, state=state, stride=n, seed=42, step_count=0, env_offset=0)
    layer = ObsCorruption(layout, batch)
    obs = torch.randn(n, layout.D, device=dev, generator=g)
    outs = [torch.empty(n, layout.D, device=dev) for _ in range(2)]
    reset = torch.rand(n, device=dev, generator=g) < 0.05
    trunc = torch.zeros(n, dtype=torch.bool, device=dev)
    bias = torch.zeros(n, max(layout.Db, 1), device=dev)
    # the two agree where nothing is drawn, and everywhere in shape
    layer.apply(obs, outs[0], reset, trunc, step=1)
    want = composition(spec, obs, state, bias, reset, torch.empty_like(outs[1]))
    torch.cuda.synchronize()
    off = 0
    for w, noise, b, clip, from_state in spec:
        if noise is None:
            assert torch.equal(outs[0][:, off:off + w].view(torch.int32), want[:, off:off + w].view(torch.int32)), (name, off)
        off += w
    state_rows = sum(w for w, *_, fs in spec if fs)
    nbytes = 2 * n * layout.D * 4 + 2 * n + state_rows * n * 4 + n * layout.Db * 4
    res = {"D": layout.D, "Db": layout.Db, "n": n, "bytes": nbytes}

    def launch(i):
        batch.step_count = i
        layer.apply(obs, outs[i & 1], reset, trunc)
    res["launch"] = summary(windows(launch, args.windows, args.launches), nbytes)
    res["composition"] = summary(windows(lambda i: composition(spec, obs, state, bias, reset, outs[i & 1]), args.windows, args.launches), nbytes)
    res["composition_over_launch"] = round(res["composition"]["us_median"] / res["launch"]["us_median"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--num-envs", type=int, default=4096)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "a timing needs the GPU"
    out = {"num_envs": args.num_envs, "windows": args.windows, "launches_per_window": args.launches}
    for name, spec in layouts().items():
        out[name] = case(name, spec, args.num_envs, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
