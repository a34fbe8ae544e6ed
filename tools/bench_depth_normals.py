#!/usr/bin/env python3
"""Time of the depth normal images (pp_depth_normals_f64, csrc/depth_image.hip) on device tensors: 64 images at 640 x 480 and at
720 x 540, in two modes -- for_vis=True with the float64 normals only, and for_vis=False with the uint8 image only -- in images
per second and in bytes moved per second (the bytes the launches must move at least: 4 read per pixel, the smoothed depth
written once and read once per later launch, and the requested output written; halo and neighbour re-reads, which the caches
serve, are not counted).  Synthetic depth of a tilted plane with noise and holes (millimetres); each figure is the median of 9
windows of 20 calls (a window ends in a synchronise), the spread is (slowest - fastest window) / median.  Beside it the time of
the numpy restatement (tests/depth_normals_np.py) on ONE image of each shape on the benchmark host: an observation, one run, one
thread, not a tuned baseline.
Usage: python3 tools/bench_depth_normals.py [--windows 9] [--iters 20] [--out profiles/bench_depth_normals.json]"""
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
from tests import depth_normals_np as DN  # noqa: E402

# (for_vis, wanted output, minimal bytes per pixel: read f32 4; write d 8; d read once per later launch 8; the output)
MODES = {"for_vis_normals_f64": (True, "normals", 4 + 8 + 8 + 24), "image_u8": (False, "normals_u8", 4 + 8 + 8 + 8 + 3)}


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
    depth[:, H // 3:H // 3 + 40, W // 2:W // 2 + 60] = 0.0
    return depth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default="profiles/bench_depth_normals.json")
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
        intr = torch.from_numpy(np.tile([572.4114 * W / 640.0, 325.2611 * W / 640.0, 242.04899 * H / 480.0], (args.images, 1))).cuda()
        for name, (for_vis, want, bytes_px) in MODES.items():
            dt, spread = windows(lambda: ops.depth_normals(ctx, depth, intr, for_vis, (want,)), args.windows, args.iters)
            report(dict(leg=name, images=args.images, width=W, height=H, calls_per_window=args.iters, ms=dt * 1e3, spread=spread,
                        images_per_s=args.images / dt, min_bytes_per_pixel=bytes_px, min_gbytes_per_s=bytes_px * args.images * H * W / dt / 1e9))
        for for_vis in (True, False):
            t0 = time.perf_counter()
            DN.depth_normals(host[0], *[float(v) for v in intr[0].cpu()], for_vis=for_vis)
            report(dict(leg="numpy_restatement_one_image", for_vis=for_vis, width=W, height=H, runs=1, seconds=time.perf_counter() - t0))
    result = dict(device=torch.cuda.get_device_name(0), windows=args.windows, iters=args.iters, window_rule="median of the windows' seconds per call; "
                  "spread = (slowest - fastest window) / median", host_rows="numpy restatement, one image, one run: an observation", rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
