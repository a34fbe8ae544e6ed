#!/usr/bin/env python3
"""Time of the device photometric augmentation (pp_photo_augment_u8) at the training batch shape, B = 8, 640 x 480:
  per op:      every image of the batch runs the same single op;
  worst chain: two 7 x 7 neighbourhood ops (median, bilateral) each followed by a run of per-pixel ops;
  mean chain:  the mean over --chains batches of sampled chains (utils/photometric.sample_programs), and the host time to
               sample, build and pack one batch's programs.
Each figure is the median of --runs timed windows of --iters calls between device events; beside them the affine warp
(pp_warp_affine_u8) of the same batch, and for each op the bytes it has to move (one pass: batch in + batch out) over its
time.  Writes the figures to --out (JSON).
Usage: python3 tools/bench_photo.py [--runs 20] [--iters 10] [--chains 1000] [--out profiles/bench_photo.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrapose_amd import ops  # noqa: E402
from pyrapose_amd.runtime import default_context  # noqa: E402
from pyrapose_amd.utils import photometric as PH  # noqa: E402


def median_us(fn, runs, iters):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / iters)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chains", type=int, default=1000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = default_context()
    B, H, W = 8, 480, 640
    rng = np.random.default_rng(0)
    img = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)).cuda()
    out = torch.empty_like(img)
    pass_bytes = 2 * img.numel()
    result = dict(device=torch.cuda.get_device_name(0), batch=B, height=H, width=W, runs=args.runs, iters=args.iters, pass_bytes=pass_bytes,
                  per_op={})
    mats = [np.array([[1.05, 0.02, 3.0], [-0.02, 0.97, -5.0]]) for _ in range(B)]
    med, lo, hi = median_us(lambda: ops.warp_affine_u8(ctx, img, mats, out=out), args.runs, args.iters)
    result["warp_affine_us"] = dict(median=med, min=lo, max=hi)
    print("warp_affine: %.1f us (min %.1f, max %.1f)" % (med, lo, hi))
    mask = PH.frequency_noise_mask(rng, -2.0, 16)
    lut = PH.op_lut(PH.lut_gamma([0.8, 1.0, 1.2]))
    blend = PH.op_blend(PH.lut_multiply(1.2), PH.lut_linear_contrast(0.8), mask)
    single = [("copy (empty program)", []), ("lut", [lut]), ("gray", [PH.op_gray(0.15)]), ("huesat", [PH.op_huesat(6, -9)]), ("blend", [blend]),
              ("conv 3x3", [PH.op_conv(PH.average_taps(3))]), ("conv 5x5", [PH.op_conv(PH.gaussian_taps(1.2))]),
              ("conv 7x7", [PH.op_conv(PH.gaussian_taps(2.0))]), ("median 3x3", [PH.op_median(3)]), ("median 5x5", [PH.op_median(5)]),
              ("median 7x7", [PH.op_median(7)]), ("bilateral 3x3", [PH.op_bilateral(*PH.bilateral_tables(3, 50.0, 50.0))]),
              ("bilateral 5x5", [PH.op_bilateral(*PH.bilateral_tables(5, 50.0, 50.0))]),
              ("bilateral 7x7", [PH.op_bilateral(*PH.bilateral_tables(7, 50.0, 50.0))])]
    for name, chain in single:
        progs = PH.compile_chain([chain] * B)
        med, lo, hi = median_us(lambda: ops.photo_augment_u8(ctx, img, progs, out=out), args.runs, args.iters)
        result["per_op"][name] = dict(median_us=med, min_us=lo, max_us=hi, gb_per_s_of_one_pass=pass_bytes / med / 1e3)
        print("%-22s %8.1f us (min %.1f, max %.1f)  one pass of %.1f MB over it: %.0f GB/s" % (name, med, lo, hi, pass_bytes / 1e6, pass_bytes / med / 1e3))
    worst = [PH.op_median(7), lut, PH.op_gray(0.15), PH.op_huesat(6, -9), PH.op_bilateral(*PH.bilateral_tables(7, 50.0, 50.0)), blend, lut,
             PH.op_huesat(-4, 3)]
    progs = PH.compile_chain([worst] * B, fuse=False)
    med, lo, hi = median_us(lambda: ops.photo_augment_u8(ctx, img, progs, out=out), args.runs, args.iters)
    result["worst_chain_us"] = dict(median=med, min=lo, max=hi, ops=[op["kind"] for op in worst])
    print("worst chain (median 7x7 + 3 per-pixel, bilateral 7x7 + 3 per-pixel): %.1f us (min %.1f, max %.1f)" % (med, lo, hi))
    # sampled chains: each batch once per window, windows of all the batches
    t0 = time.perf_counter()
    batches = [PH.sample_programs(rng, B) for _ in range(args.chains)]
    for p in batches:
        p.pinned_pool()
    host_ms = (time.perf_counter() - t0) / args.chains * 1e3
    for p in batches[:3]:
        ops.photo_augment_u8(ctx, img, p, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for p in batches:
            ops.photo_augment_u8(ctx, img, p, out=out)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / len(batches))
    n_ops = float(np.mean([p.n_ops().mean() for p in batches]))
    result["sampled_chain_us"] = dict(mean_of_chains_median_of_runs=float(np.median(times)), min=float(np.min(times)), max=float(np.max(times)),
                                      batches=len(batches), mean_ops_per_image_after_lut_fusion=n_ops, host_sample_build_pack_ms_per_batch=host_ms)
    print("mean over %d sampled batches: %.1f us per batch (min %.1f, max %.1f over %d runs); %.2f ops per image; host sampling + tables + "
          "packing %.2f ms per batch" % (len(batches), float(np.median(times)), float(np.min(times)), float(np.max(times)), args.runs, n_ops, host_ms))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
