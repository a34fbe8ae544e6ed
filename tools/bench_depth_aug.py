#!/usr/bin/env python3
"""Time of the depth-sensor simulation (pp_depth_augment, csrc/depth_aug.hip) on device tensors: 64 images at 640 x 480 and at
720 x 540, for the reference's three methods (0 both stages, 1 sensor only, 2 simplex only) and 4 and 8 octaves of simplex
noise (method 1 has none: one row), with the float32 depth as the only output -- what utils.depth_image.augment_depth_batch
returns.  Synthetic depth of a tilted plane with noise on a background at 0 (millimetres), parameter rows from
sample_depth_programs with the octaves set; each figure is the median of 9 windows of 20 calls (a window ends in a
synchronise), the spread is (slowest - fastest window) / median.  The share of launch C (up-sampling and simplex warp) is
1 - t(the launches before it) / t(all): the launches before it are timed by asking for the half-size image alone (methods 0
and 1: launches A and B) or the mask alone (method 2: launch A), which skips launch C and the full-size float32 image launch A
writes for it -- so the share is an upper bound by that write.  Beside it the time of the numpy restatement
(tests/depth_aug_np.py) on ONE image of each shape on the benchmark host: an observation, one run, one thread, not a tuned
baseline.
Usage: python3 tools/bench_depth_aug.py [--windows 9] [--iters 20] [--out profiles/bench_depth_aug.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyrapose_amd import ops  # noqa: E402
from pyrapose_amd.runtime import default_context  # noqa: E402
from pyrapose_amd.utils.depth_image import sample_depth_programs  # noqa: E402
from tests import depth_aug_np as A  # noqa: E402

LEGS = ((0, 4), (0, 8), (1, None), (2, 4), (2, 8))  # (method, octaves)


def windows(fn, n_windows, iters):
    """seconds per call: (median over the windows, (max - min) / median); one warm-up call first"""
    fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(n_windows):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        per_call.append((time.perf_counter() - t0) / iters)
    med = float(np.median(per_call))
    return med, (max(per_call) - min(per_call)) / med


def scenes(rng, n, H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    depth = np.stack([np.rint(500.0 + 40.0 * i + 1.1 * x + 1.7 * y + rng.integers(-3, 4, size=(H, W))) for i in range(n)]).astype(np.float32)
    depth[:, : H // 5] = 0.0
    depth[:, :, W - W // 6:] = 0.0
    depth[:, H // 3:H // 3 + 40, W // 2:W // 2 + 60] = 0.0
    return depth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default="profiles/bench_depth_aug.json")
    args = ap.parse_args()
    ctx = default_context()
    rng = np.random.default_rng(0)
    rows = []

    def report(row):
        rows.append(row)
        print(" ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in row.items()), flush=True)

    for W, H in ((640, 480), (720, 540)):
        host = scenes(rng, args.images, H, W)
        depth = torch.from_numpy(host).cuda()
        mask = (depth > 0).to(torch.uint8)
        h2, w2 = ops.depth_aug_half_size(H), ops.depth_aug_half_size(W)
        z = torch.randn((args.images, h2, w2), dtype=torch.float32, device="cuda")
        for method, octaves in LEGS:
            programs = sample_depth_programs(np.random.default_rng(1), args.images, method)
            if octaves is not None:
                programs[:, ops.DEPTH_AUG_PARAMS["octaves"][0]] = octaves
            before = "mask_u8" if method == 2 else "half_f64"
            dt, spread = windows(lambda: ops.depth_augment(ctx, depth, mask, programs, z, ("depth_f32",)), args.windows, args.iters)
            dt_ab, spread_ab = windows(lambda: ops.depth_augment(ctx, depth, mask, programs, z, (before,)), args.windows, args.iters)
            report(dict(leg="method_%d" % method, octaves=octaves, images=args.images, width=W, height=H, calls_per_window=args.iters,
                        ms=dt * 1e3, spread=spread, images_per_s=args.images / dt, ms_before_launch_c=dt_ab * 1e3,
                        spread_before_launch_c=spread_ab, launch_c_share=1.0 - dt_ab / dt))
            t0 = time.perf_counter()
            A.depth_augment(host[0], mask[0].cpu().numpy(), programs[0], z[0].cpu().numpy())
            report(dict(leg="numpy_restatement_one_image", method=method, octaves=octaves, width=W, height=H, runs=1,
                        seconds=time.perf_counter() - t0))
    result = dict(device=torch.cuda.get_device_name(0), windows=args.windows, iters=args.iters, window_rule="median of the windows' seconds per call; "
                  "spread = (slowest - fastest window) / median", launch_c_share="1 - ms_before_launch_c / ms: an upper bound, see the tool's docstring",
                  host_rows="numpy restatement, one image, one run: an observation", rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
