#!/usr/bin/env python3
"""Time of connected-component labelling (pp_cc_label / pp_cc_select, csrc/cc.hip) on device tensors, 8-connectivity, binary
mode, max_components 256, outputs and workspace allocated per call as ops.cc_label does.
  leg a  104 planes of 60 x 80: the mask head at B = 8, C = 13 -- seeded blobs and 2 % salt noise.
  leg b  64 planes of 480 x 640 with 8 filled ellipses each.
  leg c  the same 64 planes at density 0.6 random fill.
  leg d  64 planes of 480 x 640, each the one-pixel serpentine: one component, the longest merge chain.
  leg e  pp_cc_select of 512 slots from leg b's labels.
  leg f  utils.components.instances_from_mask_output end to end on a [8, 60 * 80, 13] prediction.
Each figure is the median of 9 windows of 20 calls (a window ends in a synchronise), the spread is (slowest - fastest window) /
median.  Beside each labelling leg, in the same process, a copy_ of the label tensor is timed the same way: a pass that reads
and writes every label once, the traffic yardstick; every leg is also given as a multiple of it.  The error word is read after
each leg.  scipy.ndimage.label on ONE plane of each leg on the benchmark host: an observation, one run, not a baseline.
Usage: python3 tools/bench_cc.py [--windows 9] [--iters 20] [--out profiles/bench_cc.json]"""
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
from pyrapose_amd.utils import components  # noqa: E402


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


def ellipses(rng, N, H, W, n, r_lo, r_hi):
    planes = np.zeros((N, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(N):
        for _ in range(n):
            cx, cy, rx, ry = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(r_lo, r_hi), rng.uniform(r_lo, r_hi)
            planes[i][((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0] = 1
    return planes


def serpentine(H, W):
    p = np.zeros((H, W), np.uint8)
    p[0::2, :] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        p[y, W - 1 if k % 2 == 0 else 0] = 1
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="profiles/bench_cc.json")
    args = ap.parse_args()
    from scipy import ndimage
    ctx = default_context()
    rows = []

    def report(row):
        rows.append(row)
        print(" ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in row.items()), flush=True)

    rng = np.random.default_rng(0)
    head = ellipses(rng, 104, 60, 80, 2, 4, 14) | (rng.random((104, 60, 80)) < 0.02).astype(np.uint8)
    big = ellipses(rng, 64, 480, 640, 8, 30, 90)
    legs = (("a_mask_head_104x60x80_blobs_salt", head), ("b_64x480x640_8_ellipses", big),
            ("c_64x480x640_density_0.6", (rng.random((64, 480, 640)) < 0.6).astype(np.uint8)),
            ("d_64x480x640_serpentine", np.broadcast_to(serpentine(480, 640), (64, 480, 640)).copy()))
    eight = ndimage.generate_binary_structure(2, 2)
    labels_b = None
    for leg, host in legs:
        planes = torch.from_numpy(host).cuda()
        N, H, W = host.shape
        res = ops.cc_label(ctx, planes)
        labels, twin = res["labels"], torch.empty_like(res["labels"])
        copy_s, copy_spread = windows(lambda: twin.copy_(labels), args.windows, args.iters)
        dt, spread = windows(lambda: ops.cc_label(ctx, planes), args.windows, args.iters)
        t0 = time.perf_counter()
        want, n = ndimage.label(host[0], structure=eight)
        scipy_s = time.perf_counter() - t0
        report(dict(leg=leg, planes=N, height=H, width=W, ms=dt * 1e3, spread=spread, copy_ms=copy_s * 1e3, copy_spread=copy_spread,
                    times_copy=dt / copy_s, mpixels_per_s=N * H * W / dt / 1e6, components_plane0=int(res["counts"][0]),
                    components_max=int(res["counts"].max()), error_word=int(res["error"].item()), scipy_one_plane_ms=scipy_s * 1e3,
                    scipy_runs=1, device_matches_scipy=bool(n == int(res["counts"][0]) and np.array_equal(labels[0].cpu().numpy(), want)),
                    calls_per_window=args.iters))
        if leg.startswith("b_"):
            labels_b = labels
    S = 512
    slot_plane = torch.from_numpy((np.arange(S) % 64).astype(np.int32)).cuda()
    slot_label = torch.from_numpy((np.arange(S) // 64 + 1).astype(np.int32)).cuda()
    dt, spread = windows(lambda: ops.cc_select(ctx, labels_b, slot_plane, slot_label), args.windows, args.iters)
    masks = ops.cc_select(ctx, labels_b, slot_plane, slot_label)
    twin = torch.empty_like(masks)
    copy_s, copy_spread = windows(lambda: twin.copy_(masks), args.windows, args.iters)
    report(dict(leg="e_cc_select_512_slots_480x640", slots=S, ms=dt * 1e3, spread=spread, mask_copy_ms=copy_s * 1e3, mask_copy_spread=copy_spread,
                times_mask_copy=dt / copy_s, calls_per_window=args.iters))
    pred_host = (rng.random((8, 60, 80, 13)) * 0.4).astype(np.float32)
    pred_host[head.reshape(8, 13, 60, 80).transpose(0, 2, 3, 1) != 0] += 0.5
    pred = torch.from_numpy(pred_host.reshape(8, 60 * 80, 13)).cuda()
    dt, spread = windows(lambda: components.instances_from_mask_output(pred, (60, 80)), args.windows, args.iters)
    inst = components.instances_from_mask_output(pred, (60, 80))
    report(dict(leg="f_instances_from_mask_output_8x60x80x13", ms=dt * 1e3, spread=spread, instances=int((inst["det_labels"] >= 0).sum()),
                error_word=int(inst["error"].item()), calls_per_window=args.iters))
    result = dict(device=torch.cuda.get_device_name(0), windows=args.windows, iters=args.iters, window_rule="median of the windows' seconds "
                  "per call; spread = (slowest - fastest window) / median", copy_yardstick="copy_ of the int32 label tensor (of the uint8 "
                  "masks for leg e), same process, timed the same way; times_copy = a leg's median / the yardstick's",
                  host_rows="scipy.ndimage.label on plane 0 of the leg, one run on the benchmark host: an observation", rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
