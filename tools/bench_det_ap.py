#!/usr/bin/env python3
"""Time of the detection-metric chain (ops.det_match -> det_order -> det_pr_curve -> det_ap, csrc/det_eval.hip) on synthetic
detections: `--images` images x `--dets` detections x `--classes` classes, about `--gts` ground truths per image.
Leg 1: one IoU threshold, the reference rule with the area integration (what utils.eval.evaluate runs).
Leg 2: COCO's ten thresholds in one launch, beside ten one-threshold launches on the same inputs.
Each figure is the median of `--windows` windows of `--calls` calls, with the spread (min .. max of the windows) beside it.
The host restatement (tests/det_eval_np.py, plain numpy loops) is timed once on a slice of the images, as an observation.
There is no bar to pass.  Usage: python3 tools/bench_det_ap.py [--out profiles/bench_det_ap.json]"""
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
from tests import det_eval_np as DN  # noqa: E402


def windows(fn, n_windows, calls):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n_windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / calls * 1e3)
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def make_inputs(B, D, C, n_gt, seed=0):
    rng = np.random.default_rng(seed)
    counts = rng.integers(max(n_gt // 2, 1), n_gt + n_gt // 2 + 1, size=B)
    offs = np.zeros(B + 1, np.int32)
    offs[1:] = np.cumsum(counts)
    G = int(offs[-1])
    xy = rng.uniform(0, 560, size=(G, 2))
    gt_boxes = np.concatenate([xy, xy + rng.uniform(20, 120, size=(G, 2))], axis=1)
    gt_labels = rng.integers(0, C, size=G).astype(np.int32)
    det_boxes = np.zeros((B, D, 4))
    det_labels = np.zeros((B, D), np.int32)
    for b in range(B):
        j = rng.integers(offs[b], offs[b + 1], size=D)
        hit = rng.uniform(size=D) < 0.5
        jitter = rng.normal(0, 6, size=(D, 4))
        p = rng.uniform(0, 560, size=(D, 2))
        clutter = np.concatenate([p, p + rng.uniform(20, 120, size=(D, 2))], axis=1)
        det_boxes[b] = np.where(hit[:, None], gt_boxes[j] + jitter, clutter)
        det_labels[b] = np.where(hit, gt_labels[j], rng.integers(0, C, size=D))
    det_scores = rng.permutation(B * D).reshape(B, D) / float(B * D)
    return det_boxes, det_scores, det_labels, gt_boxes, gt_labels, offs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--classes", type=int, default=15)
    ap.add_argument("--gts", type=int, default=8)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-images", type=int, default=50, help="images the numpy restatement is timed on")
    ap.add_argument("--out", default="profiles/bench_det_ap.json")
    args = ap.parse_args()
    ctx = default_context()
    B, D, C = args.images, args.dets, args.classes
    host = make_inputs(B, D, C, args.gts)
    f64, i32 = torch.float64, torch.int32
    db, ds, dl, gb, gl, go = (torch.from_numpy(a).cuda().to(t) for a, t in zip(host, (f64, f64, i32, f64, i32, i32)))
    coco = np.linspace(0.5, 0.95, 10)

    def chain(thr, rule, integration):
        match, ign, npos = ops.det_match(ctx, db, ds, dl, gb, gl, go, C, thr, rule=rule, check=False)
        order, offs = ops.det_order(ds, dl, C)
        _tp, _fp, recall, env = ops.det_pr_curve(ctx, order, offs, match, ign, npos, check=False)
        return ops.det_ap(ctx, offs, npos, recall, env, integration, check=False)

    w = (args.windows, args.calls)
    res = dict(device=torch.cuda.get_device_name(0), images=B, detections_per_image=D, classes=C, ground_truth=int(host[5][-1]),
               windows=args.windows, calls_per_window=args.calls)
    res["leg1_one_threshold_chain"] = windows(lambda: chain([0.5], "reference", "area"), *w)
    res["leg1_one_threshold_match_only"] = windows(lambda: ops.det_match(ctx, db, ds, dl, gb, gl, go, C, [0.5], rule="reference", check=False), *w)
    res["leg2_ten_thresholds_chain"] = windows(lambda: chain(coco, "coco", "101"), *w)
    res["leg2_ten_thresholds_match_only"] = windows(lambda: ops.det_match(ctx, db, ds, dl, gb, gl, go, C, coco, rule="coco", check=False), *w)
    res["leg2_ten_one_threshold_launches_match_only"] = windows(
        lambda: [ops.det_match(ctx, db, ds, dl, gb, gl, go, C, [t], rule="coco", check=False) for t in coco], *w)
    res["det_order_only"] = windows(lambda: ops.det_order(ds, dl, C), *w)
    res["ten_in_one_over_ten_launches"] = (res["leg2_ten_thresholds_match_only"]["median_ms"] /
                                           res["leg2_ten_one_threshold_launches_match_only"]["median_ms"])
    ap_dev = chain(coco, "coco", "101")[0].cpu().numpy()
    res["coco_AP_of_the_synthetic_set"] = float(ap_dev[ap_dev > -1].mean())
    # the host restatement on the first images, one threshold and ten (an observation: plain numpy loops, not a tuned baseline)
    n = min(args.host_images, B)
    g1 = int(host[5][n])
    sl = (host[0][:n], host[1][:n], host[2][:n], host[3][:g1], host[4][:g1], host[5][:n + 1])
    for name, thr, rule, integ in (("host_restatement_one_threshold", [0.5], "reference", "area"),
                                   ("host_restatement_ten_thresholds", list(coco), "coco", "101")):
        t0 = time.perf_counter()
        DN.evaluate(*sl, C, thr, rule, integ)
        res[name] = dict(images=n, ms=(time.perf_counter() - t0) * 1e3)
    print(json.dumps(res, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
