#!/usr/bin/env python3
"""Time of the evaluation overlays (pp_draw_overlay_u8, csrc/overlay.hip) on device tensors: 64 images at 640 x 480 and at
720 x 540, the list and the id image already on the device (what ops.draw_overlay takes), a separate output tensor.
  leg a  10 detections per image: a box (4 segments) and a caption with its rim (2 glyph records per character) each.
  leg b  8 ground-truth and 8 estimated cuboid wireframes (12 segments each) and 64 discs of diameter 7 per image.
  leg c  the id layer alone: 8 label blobs per image, fill and outline of width 2, no records.
  leg d  a, b and c together.
  leg e  stress: 4096 segments per image, 20 to 120 pixels long, thickness 2 -- every tile walks 16 chunks of 256 records.
Each figure is the median of 9 windows of 20 calls (a window ends in a synchronise), the spread is (slowest - fastest window) /
median.  In the same process, on the same tensors, out.copy_(images) is timed the same way: a pass that reads and writes every
byte once cannot be faster, and every leg is also given as a multiple of it.  Beside them the time of the numpy restatement
(tests/overlay_np.py) on ONE image of leg d on the benchmark host: an observation, one run, one thread, not a baseline.
Usage: python3 tools/bench_overlay.py [--windows 9] [--iters 20] [--out profiles/bench_overlay.json]"""
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
from pyrapose_amd.utils import visualization as V  # noqa: E402
from pyrapose_amd.utils.colors import label_color  # noqa: E402
from tests import overlay_np as O  # noqa: E402


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


def cuboid(rng, W, H):
    """16 pixel coordinates of a cuboid seen from the front: two rectangles, the back one shifted and shrunk"""
    cx, cy = rng.uniform(80, W - 80), rng.uniform(80, H - 80)
    w, h, dx, dy = rng.uniform(30, 90), rng.uniform(30, 90), rng.uniform(-25, 25), rng.uniform(-25, 25)
    front = [(cx - w, cy - h), (cx + w, cy - h), (cx + w, cy + h), (cx - w, cy + h)]
    back = [(x * 0.8 + 0.2 * cx + dx, y * 0.8 + 0.2 * cy + dy) for x, y in front]
    return np.array(front + back)


def detections(ov, i, rng, W, H):
    for k in range(10):
        x1, y1 = rng.uniform(0, W - 120), rng.uniform(20, H - 120)
        box = (x1, y1, x1 + rng.uniform(40, 200), y1 + rng.uniform(40, 200))
        ov.box(i, box, label_color(k))
        ov.caption(i, box, "object_%02d: %.2f" % (k, rng.uniform(0.5, 1.0)))


def wireframes(ov, i, rng, W, H):
    for k in range(8):
        c = cuboid(rng, W, H)
        ov.box3d(i, c, (255, 0, 0))
        ov.box3d(i, c + rng.normal(scale=3.0, size=c.shape), (0, 204, 0))
    for k in range(64):
        ov.disc(i, (rng.uniform(0, W), rng.uniform(0, H)), label_color(k % 8))


def stress(ov, i, rng, W, H):
    for k in range(4096):
        x, y, a, n = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0, 2 * np.pi), rng.uniform(20, 120)
        ov.segment(i, (x, y), (x + n * np.cos(a), y + n * np.sin(a)), label_color(k), 2)


def blobs(rng, B, H, W):
    ids = np.zeros((B, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        for k in range(8):
            cx, cy, rx, ry = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(30, 90), rng.uniform(30, 90)
            ids[b][((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0] = k + 1
    return ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default="profiles/bench_overlay.json")
    args = ap.parse_args()
    ctx = default_context()
    B = args.images
    rows = []

    def report(row):
        rows.append(row)
        print(" ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in row.items()), flush=True)

    for W, H in ((640, 480), (720, 540)):
        rng = np.random.default_rng(W)
        images_host = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
        images = torch.from_numpy(images_host).cuda()
        out = torch.empty_like(images)
        ids_host = blobs(rng, B, H, W)
        ids = torch.from_numpy(ids_host).cuda()
        palette_host = V.pack_palette(None, 96)
        palette = torch.from_numpy(palette_host).cuda()
        lists = {}
        for name, parts in (("a", (detections,)), ("b", (wireframes,)), ("d", (detections, wireframes)), ("e", (stress,))):
            ov = V.OverlayList(B)
            part_rng = np.random.default_rng(W + 1)  # leg d draws leg a's and leg b's kinds of records
            for i in range(B):
                for part in parts:
                    part(ov, i, part_rng, W, H)
            prims, off = ov.pack()
            lists[name] = (torch.from_numpy(prims).cuda(), torch.from_numpy(off).cuda(), prims, off, ov.dropped)
        none = (torch.zeros((0, 8), dtype=torch.int32, device="cuda"), torch.zeros((B + 1,), dtype=torch.int32, device="cuda"))
        shape = dict(images=B, width=W, height=H, calls_per_window=args.iters)
        copy_s, copy_spread = windows(lambda: out.copy_(images), args.windows, args.iters)
        report(dict(leg="copy_floor", ms=copy_s * 1e3, spread=copy_spread, gb_per_s=2 * images.numel() / copy_s / 1e9, **shape))
        legs = (("a_detections_with_captions", lists["a"], False), ("b_wireframes_and_discs", lists["b"], False),
                ("c_id_layer_fill_outline_2", none, True), ("d_all_together", lists["d"], True), ("e_stress_4096_segments", lists["e"], False))
        for leg, lst, layer in legs:
            kw = dict(ids=ids, palette=palette, fill=True, outline=2) if layer else {}
            dt, spread = windows(lambda: ops.draw_overlay(ctx, images, lst[0], lst[1], out=out, **kw), args.windows, args.iters)
            report(dict(leg=leg, ms=dt * 1e3, spread=spread, times_copy=dt / copy_s, images_per_s=B / dt,
                        records_per_image=int(lst[0].shape[0]) // B, dropped=lst[4] if len(lst) > 4 else 0, id_layer=layer, **shape))
        prims, off = lists["d"][2], lists["d"][3]
        t0 = time.perf_counter()
        want = O.draw_image(images_host[0], prims[off[0]:off[1]], ids_host[0], palette_host.view(np.uint32).astype(np.int64), True, 2)
        seconds = time.perf_counter() - t0
        got = ops.draw_overlay(ctx, images, lists["d"][0], lists["d"][1], ids, palette, True, 2)[0].cpu().numpy()
        report(dict(leg="numpy_restatement_one_image_of_leg_d", width=W, height=H, runs=1, seconds=seconds,
                    device_matches=bool(np.array_equal(got, want))))
    result = dict(device=torch.cuda.get_device_name(0), windows=args.windows, iters=args.iters, window_rule="median of the windows' seconds "
                  "per call; spread = (slowest - fastest window) / median", copy_floor="out.copy_(images) on the same tensors, same process, "
                  "timed the same way; times_copy = a leg's median / the floor's", host_rows="numpy restatement, one image, one run: an observation",
                  rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
