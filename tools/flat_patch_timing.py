#!/usr/bin/env python3
"""What finding the flat patches again adds to a terrain redraw (flat patches), by the method of
tools/terrain_regen_timing.py: DeviceHeightField.regenerate(seed) of the default 800 x 800 TerrainGeneratorCfg with one DepthCamera
on the field (tile table on the host, descriptor upload, wl_terrain_generate, wl_heightfield_pairs, the decoded heights, the
pyramid) -- on a field WITH "init_pos" patches on every tile (8 per tile, radius 0.15 m, 0.02 m, 4096 tries: + wl_flat_patches) and on
one WITHOUT, in alternating blocks of one process so that clocks and neighbours are the same for both.  Wall clock around work that
ends in a device synchronise; prints one JSON line with the medians and the spread over the blocks.

`--root DIR` measures another checkout of the package (the parent commit's, built there: patches off only -- it has none), so that a
driver can alternate the two processes:

    python tools/flat_patch_timing.py [--reps 200] [--blocks 6]
    python tools/flat_patch_timing.py --root ../parent --patches off"""
import argparse
import json
import os
import statistics
import sys
import time


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
    ap.add_argument("--reps", type=int, default=200, help="redraws per block")
    ap.add_argument("--blocks", type=int, default=6, help="blocks per configuration, alternating")
    ap.add_argument("--patches", choices=("both", "on", "off"), default="both")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package is measured")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    import torch

    from wheeledlab_amd.core import DepthCamera, generate_heightfield
    from wheeledlab_amd.envs.terrain_gen_cfg import TerrainGeneratorCfg

    dev = "cuda:0"
    sync = torch.cuda.synchronize
    fields, keep = {}, []
    for which in (("off", "on") if args.patches == "both" else (args.patches,)):
        hf = generate_heightfield(TerrainGeneratorCfg(seed=0), dev)
        keep.append(DepthCamera(hf, dev))                       # the pyramid is part of every redraw, as in a task that ray-casts
        if which == "on":
            from wheeledlab_amd.core import find_flat_patches
            from wheeledlab_amd.envs.terrain_gen_cfg import FlatPatchSamplingCfg
            cfg = TerrainGeneratorCfg(seed=0, flat_patch_sampling={"init_pos": FlatPatchSamplingCfg(
                num_patches=8, patch_radius=0.15, max_height_diff=0.02, max_tries=4096)})
            keep.append(find_flat_patches(hf, cfg, seed=5))
        fields[which] = hf
    seeds = iter(range(1, 10 ** 9))
    for hf in fields.values():
        for _ in range(10):
            hf.regenerate(next(seeds))
    blocks = {which: [] for which in fields}
    for _ in range(args.blocks):
        for which, hf in fields.items():
            blocks[which].append(timed(lambda: hf.regenerate(next(seeds)), args.reps, sync))
    ms = lambda v: round(1e3 * v, 4)      # noqa: E731
    out = {"label": args.label, "root": os.path.abspath(args.root), "field": "800x800", "reps": args.reps, "blocks": args.blocks}
    for which, runs in blocks.items():
        every = sorted(t for r in runs for t in r)
        out[f"regenerate_{which}_ms"] = {"median": ms(statistics.median(every)), "min": ms(every[0]), "p10": ms(every[len(every) // 10]),
                                        "p90": ms(every[9 * len(every) // 10]), "block_medians": [ms(statistics.median(r)) for r in runs]}
    if "on" in fields:
        fp = keep[-1]
        out["patches"] = {"tiles": fp.n_tiles, "per_tile": fp.n_patches, "failed_last_draw": fp.failed,
                          "largest_accepted_attempt_last_draw": int(fp.tries.max())}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        e0.record()
        for _ in range(args.reps):
            fp.find()
        e1.record()
        sync()
        out["find_only_back_to_back_ms"] = ms(e0.elapsed_time(e1) * 1e-3 / args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
