#!/usr/bin/env python3
"""Time of the layered depth-hole filling (pp_depth_inpaint, csrc/depth_inpaint.hip) on device tensors: 64 images at 640 x 480
and at 720 x 540 with the float32 filled depth as the only output -- what utils.depth_image.inpaint_depth_batch returns.  The
object is a box with thin bars (4 to 10 mm wide) rendered at 64 poses by render_depth_batch; augment_depth_batch cuts its shadow
holes (the bars narrower than the opening's box go, the silhouette is eaten into).
  leg a  the augmented object over a non-zero background plane: the holes are the shadow holes alone; radius 5, no limit.
  leg b  the same renders over the empty (zero) background, max_dist = 16: the background is a hole whose rim is filled 16 deep.
  leg c  leg a's images through inpaint + normals (normals_from_depth_batch(inpaint=...), for_vis=False) against normals alone.
Each figure is the median of 9 windows of 20 calls (a window ends in a synchronise), the spread is (slowest - fastest window) /
median.  Every row carries the holes, the pixels filled and the deepest layer per image (mean and maximum over the batch), which
set the work: the number of fill launches is the batch's deepest layer.  Beside them the time of the numpy restatement
(tests/depth_inpaint_np.py) on ONE image of leg a on the benchmark host: an observation, one run, one thread, not a baseline.
Usage: python3 tools/bench_depth_inpaint.py [--windows 9] [--iters 20] [--out profiles/bench_depth_inpaint.json]"""
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
from pyrapose_amd.utils.depth_image import augment_depth_batch, normals_from_depth_batch, sample_depth_programs  # noqa: E402
from pyrapose_amd.utils.renderer import render_depth_batch  # noqa: E402
from tests import depth_inpaint_np as I  # noqa: E402


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


def box(centre, size):
    c, s = np.asarray(centre, np.float64), np.asarray(size, np.float64) / 2
    pts = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * s + c
    faces = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                      [1, 5, 7], [1, 7, 3]])
    return pts, faces


def barred_box():
    """a 120 x 80 x 40 mm body with bars of 4, 6, 8 and 10 mm sticking out of it (millimetres)"""
    parts = [box((0, 0, 0), (120, 80, 40))]
    for i, w in enumerate((4, 6, 8, 10)):
        parts.append(box((-45 + 30 * i, 75, 0), (w, 70, w)))
        parts.append(box((95, -30 + 20 * i, 0), (70, w, w)))
    pts, faces, at = [], [], 0
    for p, f in parts:
        pts.append(p)
        faces.append(f + at)
        at += len(p)
    return {"pts": np.concatenate(pts), "faces": np.concatenate(faces)}


def poses(rng, n):
    R = []
    for _ in range(n):
        a, b = rng.uniform(-0.5, 0.5), rng.uniform(0, 2 * np.pi)
        ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
        R.append(np.array([[cb, -sb, 0], [sb, cb, 0], [0, 0, 1.0]]) @ np.array([[1.0, 0, 0], [0, ca, -sa], [0, sa, ca]]))
    t = np.stack([rng.uniform(-60, 60, n), rng.uniform(-40, 40, n), rng.uniform(450, 700, n)], axis=1)
    return np.stack(R), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default="profiles/bench_depth_inpaint.json")
    args = ap.parse_args()
    ctx = default_context()
    rng = np.random.default_rng(0)
    rows = []

    def report(row):
        rows.append(row)
        print(" ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in row.items()), flush=True)

    def work(depth, max_dist):
        c = ops.depth_inpaint(ctx, depth, None, 5, max_dist, False, ("counts",))["counts"].cpu().numpy()
        return dict(holes_mean=float(c[:, 0].mean()), holes_max=int(c[:, 0].max()), filled_mean=float(c[:, 1].mean()),
                    filled_max=int(c[:, 1].max()), deepest_layer_mean=float(c[:, 2].mean()), deepest_layer_max=int(c[:, 2].max()))

    model = barred_box()
    for W, H in ((640, 480), (720, 540)):
        K = np.array([[572.4 * W / 640, 0, W / 2 + 0.37], [0, 573.6 * W / 640, H / 2 - 0.21], [0, 0, 1]])
        R, t = poses(rng, args.images)
        rendered = render_depth_batch(model, (W, H), K, R, t)
        programs = sample_depth_programs(np.random.default_rng(1), args.images)
        empty = augment_depth_batch(rendered, None, programs, generator=torch.Generator(device="cuda").manual_seed(2))
        y, x = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
        plane = torch.round(1500.0 + 0.4 * x + 0.7 * y).to(torch.float32)
        over_plane = torch.where(rendered > 0, empty, plane.expand_as(empty)).contiguous()
        shape = dict(images=args.images, width=W, height=H, calls_per_window=args.iters)
        for leg, depth, max_dist in (("a_background_plane", over_plane, 0), ("b_empty_background_max_dist_16", empty, 16)):
            dt, spread = windows(lambda: ops.depth_inpaint(ctx, depth, None, 5, max_dist, False, ("filled_f32",)), args.windows, args.iters)
            report(dict(leg=leg, radius=5, max_dist=max_dist, ms=dt * 1e3, spread=spread, images_per_s=args.images / dt, **shape,
                        **work(depth, max_dist)))
        dt_n, spread_n = windows(lambda: normals_from_depth_batch(over_plane, K, for_vis=False, ctx=ctx), args.windows, args.iters)
        dt_c, spread_c = windows(lambda: normals_from_depth_batch(over_plane, K, for_vis=False, ctx=ctx, inpaint=dict(radius=5)),
                                 args.windows, args.iters)
        report(dict(leg="c_fill_and_normals", radius=5, max_dist=0, ms=dt_c * 1e3, spread=spread_c, ms_normals_alone=dt_n * 1e3,
                    spread_normals_alone=spread_n, ratio=dt_c / dt_n, **shape))
        host = over_plane[0].cpu().numpy()
        t0 = time.perf_counter()
        I.depth_inpaint(host, None, 5, 0, False)
        report(dict(leg="numpy_restatement_one_image_of_leg_a", width=W, height=H, runs=1, seconds=time.perf_counter() - t0))
    result = dict(device=torch.cuda.get_device_name(0), windows=args.windows, iters=args.iters, window_rule="median of the windows' seconds "
                  "per call; spread = (slowest - fastest window) / median", host_rows="numpy restatement, one image, one run: an observation",
                  rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
