#!/usr/bin/env python3
"""What the ray caster's two kernel forms cost beside the kernels they generalise, by the method of
tools/flat_patch_timing.py: one process, alternating blocks so that clocks and neighbours are the same for every configuration, a
device synchronise around each timed call, medians and spread over the blocks as one JSON line (plus each configuration's
back-to-back time per call between two events, which leaves the launch's host cost out).

Workload: the bench field, 4096 envs of an ElevBatch after a reset and a few steps.
  column        the elevation scanner's 26 x 26 grid, 20 m above the car, yaw-aligned: the column form (one bilinear sample per ray)
  walk          the same rays through the general form (the bound-pyramid walk)
  observe       ElevBatch.observe() of the same batch: the task's own fused scan -- exists in a parent checkout too
  rc_camera     a 60 x 80 ray-caster camera with the visual camera's intrinsics and mount, 20 m
  depth_camera  DepthCamera.render at 20 m (the tiled kernel) -- exists in a parent checkout too
  lidar         a default LidarCfg (1 x 360 beams, 10 m) through LidarScanner.render -- exists in a parent checkout too
  lidar_plane   the same over the z = 0 plane of a DriftBatch (launch- and store-bound) -- exists in a parent checkout too

`--root DIR` measures another checkout of the package (the parent commit's, built there): the configurations it has.

    python tools/raycaster_timing.py [--reps 200] [--blocks 6]
    python tools/raycaster_timing.py --root ../parent"""
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
    ap.add_argument("--reps", type=int, default=200, help="calls per block")
    ap.add_argument("--blocks", type=int, default=6, help="blocks per configuration, alternating")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package is measured")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    import torch

    from wheeledlab_amd import core
    from wheeledlab_amd.params import visual_params

    dev = "cuda:0"
    sync = torch.cuda.synchronize
    n = args.envs
    batch = core.ElevBatch(n, device=dev, seed=3)
    batch.reset()
    batch.rollout(torch.rand(4, n, 2, device=dev) * 2 - 1)
    cam = core.DepthCamera(batch.hf, dev)
    scratch = torch.empty_like(batch.obs)
    image = torch.empty(n, cam.IMG_H, cam.IMG_W, dtype=torch.float32, device=dev)
    runs = {"observe": lambda: batch.observe(scratch), "depth_camera": lambda: cam.render(batch, 20.0, out=image)}
    if hasattr(core, "RayCaster"):
        from wheeledlab_amd.envs.sensors_cfg import GridPatternCfg, PinholeCameraPatternCfg, RayCasterCameraCfg, RayCasterCfg
        scanner = RayCasterCfg(offset_pos=(0.0, 0.0, 20.0), attach_yaw_only=True, pattern_cfg=GridPatternCfg(size=(2.5, 2.5), resolution=0.1),
                               max_distance=100.0)
        column, walk = core.RayCaster(scanner, dev), core.RayCaster(scanner, dev, vertical=False)
        assert column.vertical and not walk.vertical and column.n_rays == 676
        p = visual_params()
        pin = PinholeCameraPatternCfg(width=80, height=60, focal_length=p.fx, horizontal_aperture=80.0, vertical_aperture=60 * p.fx / p.fy)
        rc_cam = core.RayCaster(RayCasterCameraCfg(pattern_cfg=pin, offset_pos=tuple(p.cam_pos), offset_rot=(0.5, -0.5, 0.5, -0.5),
                                                   max_distance=20.0), dev)
        grid_out = torch.empty(n, 676, dtype=torch.float32, device=dev)
        flat_image = image.view(n, -1)
        runs.update(column=lambda: column.render(batch, cam, out=grid_out), walk=lambda: walk.render(batch, cam, out=grid_out),
                    rc_camera=lambda: rc_cam.render(batch, cam, out=flat_image))
    if hasattr(core, "LidarScanner"):
        lidar = core.LidarScanner(device=dev)
        drift = core.DriftBatch(n, device=dev, seed=3)
        drift.reset()
        ranges = torch.empty(n, lidar.n_beams, dtype=torch.float32, device=dev)
        runs.update(lidar=lambda: lidar.render(batch, out=ranges, camera=cam), lidar_plane=lambda: lidar.render(drift, out=ranges))
    for fn in runs.values():
        for _ in range(10):
            fn()
    blocks = {name: [] for name in runs}
    for _ in range(args.blocks):
        for name, fn in runs.items():
            blocks[name].append(timed(fn, args.reps, sync))
    us = lambda v: round(1e6 * v, 2)      # noqa: E731
    out = {"label": args.label, "root": os.path.abspath(args.root), "field": "bench 800x800", "envs": n, "reps": args.reps, "blocks": args.blocks}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, per_block in blocks.items():
        every = sorted(t for r in per_block for t in r)
        sync()
        e0.record()
        for _ in range(args.reps):
            runs[name]()
        e1.record()
        sync()
        out[f"{name}_us"] = {"median": us(statistics.median(every)), "min": us(every[0]), "p10": us(every[len(every) // 10]),
                             "p90": us(every[9 * len(every) // 10]), "block_medians": [us(statistics.median(r)) for r in per_block],
                             "back_to_back": us(e0.elapsed_time(e1) * 1e-3 / args.reps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
