#!/usr/bin/env python3
"""Time per call of the observation normaliser's entry points (csrc/wl_obs_norm.hip) at the rollout shapes of the agents at 4096
envs (observation normalisation):

  accumulate   wl_obsnorm_accumulate, both launches (the pass + the fixed-order sum of the partials), in place (out = x) and
               without an output; bytes per second from the bytes the pass must move: rows x D x 4, read once (+ written once in place)
  update       wl_obsnorm_update (one workgroup)
  fold         wl_obsnorm_fold of one [64, D] first layer

Device events around `--windows` windows of `--reps` back-to-back calls each, after `--warmup` calls of the same shape; every figure
is the median window's time per call with the fastest window's beside it (`*_min_us`), so the spread is on the line.  update and fold
are a few microseconds of work: their figures are launch latency.  Needs a GPU (there is no fallback).  Prints one JSON line per shape.

    python tools/obsnorm_probe.py [--reps 100] [--windows 5] [--warmup 5] [--shapes 524288x14,524288x689,131072x3208]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="524288x14,524288x689,131072x3208")
    args = ap.parse_args()

    import torch

    from wheeledlab_amd import _abi as A
    from wheeledlab_amd.rl.normalizer import EmpiricalNormalization

    if not torch.cuda.is_available():
        raise SystemExit("obsnorm_probe needs a GPU")
    dev, lib = "cuda:0", A.load()
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        per_call = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            per_call.append(e0.elapsed_time(e1) * 1e-3 / args.reps)
        return statistics.median(per_call), min(per_call)

    for shape in args.shapes.split(","):
        rows, D = (int(v) for v in shape.split("x"))
        nz = EmpiricalNormalization(D).to(dev)
        x = torch.randn(rows, D, device=dev) * 3.0 + 1.0
        sums = nz._accumulate(x, None)
        t_read = timed(lambda: nz._accumulate(x, None))
        t_inplace = timed(lambda: nz._accumulate(x, x))           # x / 1.01 each time: the values shrink (by 1.01^600 < 400 in all), the traffic does not
        t_update = timed(lambda: A.check(lib.wl_obsnorm_update(D, sums.data_ptr(), rows, 2 ** 62, 1e-2, nz._mean.data_ptr(), nz._var.data_ptr(),
                                                               nz._std.data_ptr(), nz._inv_std.data_ptr(), nz.count.data_ptr(), stream()), "update"))
        w, b = torch.randn(64, D, device=dev), torch.randn(64, device=dev)
        wo, bo = torch.empty_like(w), torch.empty_like(b)
        t_fold = timed(lambda: A.check(lib.wl_obsnorm_fold(D, 64, w.data_ptr(), b.data_ptr(), nz._mean.data_ptr(), nz._inv_std.data_ptr(),
                                                           wo.data_ptr(), bo.data_ptr(), stream()), "fold"))
        nbytes = rows * D * 4
        us = lambda t: round(t * 1e6, 2)
        print(json.dumps({"rows": rows, "D": D, "scratch_bytes": int(lib.wl_obsnorm_scratch_bytes(rows, D, D)),
                          "accumulate_read_only_us": us(t_read[0]), "accumulate_read_only_min_us": us(t_read[1]),
                          "read_only_GBps": round(nbytes / t_read[0] * 1e-9, 1),
                          "accumulate_in_place_us": us(t_inplace[0]), "accumulate_in_place_min_us": us(t_inplace[1]),
                          "in_place_GBps": round(2 * nbytes / t_inplace[0] * 1e-9, 1),
                          "update_us": us(t_update[0]), "update_min_us": us(t_update[1]), "fold_us": us(t_fold[0]), "fold_min_us": us(t_fold[1]),
                          "reps": args.reps, "windows": args.windows}), flush=True)


if __name__ == "__main__":
    main()
