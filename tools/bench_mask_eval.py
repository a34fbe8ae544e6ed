#!/usr/bin/env python3
"""Time of the segmentation-metric chain (ops.mask_pack -> mask_iou_pairs -> det_match_iou -> det_order -> det_pr_curve ->
det_ap, csrc/mask_eval.hip) on synthetic instance masks: `--images` images x `--dets` detection slots x `--classes` classes at
`--width` x `--height`, about `--gts` ground truths per image.  The masks are filled rectangles and ellipses inscribed in the
boxes of tools/bench_det_ap.py's generator, drawn on the device `--chunk` images at a time and packed at once, so the byte
masks never exist all together (1 000 x 100 masks of 640 x 480 would be 30 GB; their packed words are 3.8 GB).
Each figure is the median of `--windows` windows of `--calls` calls, with the spread (min .. max of the windows) beside it.
pp_mask_iou_pairs also gets its achieved bytes/s against the packed words it must read at least once (every non-padding
detection's and every ground truth's non-empty word range), beside the HBM bandwidth AMD publishes for the MI355X (8 TB/s:
a published figure, not one measured here).  The box chain on the same detections runs in the same process, as an observation;
so does one run of the numpy restatement (tests/mask_eval_np.py, plain loops) on a few small images.  There is no bar to pass.
Usage: python3 tools/bench_mask_eval.py [--out profiles/bench_mask_eval.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from pyrapose_amd import ops  # noqa: E402
from pyrapose_amd.runtime import default_context  # noqa: E402
from tools.bench_det_ap import make_inputs, windows  # noqa: E402

HBM_PUBLISHED_TBS = 8.0  # AMD's data sheet for the MI355X (HBM3E peak), quoted, not measured


def draw(boxes, ellipse, H, W):
    """boxes [n,4] float64 (device), ellipse bool [n] -> uint8 [n,H,W]: the box's pixels, or the ellipse inscribed in it"""
    y = torch.arange(H, device=boxes.device, dtype=torch.float64)[None, :, None] + 0.5
    x = torch.arange(W, device=boxes.device, dtype=torch.float64)[None, None, :] + 0.5
    x1, y1, x2, y2 = (boxes[:, k][:, None, None] for k in range(4))
    inside = (x >= x1) & (x < x2) & (y >= y1) & (y < y2)
    r = ((x - (x1 + x2) / 2) / ((x2 - x1) / 2)) ** 2 + ((y - (y1 + y2) / 2) / ((y2 - y1) / 2)) ** 2
    return (inside & (~ellipse[:, None, None] | (r <= 1.0))).to(torch.uint8)


def pack_in_chunks(ctx, boxes, ellipse, H, W, chunk):
    parts = [ops.mask_pack(ctx, draw(boxes[i:i + chunk], ellipse[i:i + chunk], H, W)) for i in range(0, boxes.shape[0], chunk)]
    return tuple(torch.cat([p[k] for p in parts]) for k in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--classes", type=int, default=15)
    ap.add_argument("--gts", type=int, default=8)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--chunk", type=int, default=500, help="masks drawn and packed at a time")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-images", type=int, default=2, help="images the numpy restatement is timed on (at 1/8 of the size)")
    ap.add_argument("--out", default="profiles/bench_mask_eval.json")
    args = ap.parse_args()
    ctx = default_context()
    B, D, C, H, W = args.images, args.dets, args.classes, args.height, args.width
    host = make_inputs(B, D, C, args.gts)
    host = (np.clip(host[0] * (W / 680.0), 0, [W, H, W, H]),) + host[1:3] + (np.clip(host[3] * (W / 680.0), 0, [W, H, W, H]),) + host[4:]
    f64, i32 = torch.float64, torch.int32
    db, ds, dl, gb, gl, go = (torch.from_numpy(np.ascontiguousarray(a)).cuda().to(t) for a, t in zip(host, (f64, f64, i32, f64, i32, i32)))
    rng = np.random.default_rng(1)
    det_ell = torch.from_numpy(rng.uniform(size=B * D) < 0.5).cuda()
    gt_ell = torch.from_numpy(rng.uniform(size=gb.shape[0]) < 0.5).cuda()
    coco = np.linspace(0.5, 0.95, 10)
    w = (args.windows, args.calls)
    res = dict(device=torch.cuda.get_device_name(0), images=B, detections_per_image=D, classes=C, ground_truth=int(host[5][-1]),
               height=H, width=W, windows=args.windows, calls_per_window=args.calls, hbm_published_TBps=HBM_PUBLISHED_TBS)

    sample = draw(db.reshape(-1, 4)[:args.chunk], det_ell[:args.chunk], H, W)
    res["mask_pack_%d_masks" % sample.shape[0]] = windows(lambda: ops.mask_pack(ctx, sample), *w)
    res["mask_pack_bytes_read"] = int(sample.numel())
    res["mask_rle_row_%d_masks" % min(256, sample.shape[0])] = windows(lambda: ops.mask_rle(ctx, sample[:256], order="row"), *w)
    res["mask_rle_column_%d_masks" % min(256, sample.shape[0])] = windows(lambda: ops.mask_rle(ctx, sample[:256], order="column"), *w)
    del sample
    t0 = time.perf_counter()
    dp = pack_in_chunks(ctx, db.reshape(-1, 4), det_ell, H, W, args.chunk)
    gp = pack_in_chunks(ctx, gb, gt_ell, H, W, args.chunk)
    torch.cuda.synchronize()
    res["draw_and_pack_all_masks_once_ms"] = (time.perf_counter() - t0) * 1e3

    def pairs():
        return ops.mask_iou_pairs(ctx, dp, gp, go, (H, W), D, det_labels=dl)

    def chain():
        iou, _po = pairs()
        match, ign, npos = ops.det_match_iou(ctx, iou, ds, dl, gl, go, C, coco, rule="coco", check=False)
        order, offs = ops.det_order(ds, dl, C)
        _tp, _fp, recall, env = ops.det_pr_curve(ctx, order, offs, match, ign, npos, check=False)
        return ops.det_ap(ctx, offs, npos, recall, env, "101", check=False)

    def box_chain():
        match, ign, npos = ops.det_match(ctx, db, ds, dl, gb, gl, go, C, coco, rule="coco", check=False)
        order, offs = ops.det_order(ds, dl, C)
        _tp, _fp, recall, env = ops.det_pr_curve(ctx, order, offs, match, ign, npos, check=False)
        return ops.det_ap(ctx, offs, npos, recall, env, "101", check=False)

    iou = pairs()[0]
    res["mask_iou_pairs"] = windows(pairs, *w)
    res["det_match_iou_ten_thresholds"] = windows(lambda: ops.det_match_iou(ctx, iou, ds, dl, gl, go, C, coco, rule="coco", check=False), *w)
    res["mask_ap_chain_from_packed_masks"] = windows(chain, *w)
    res["box_ap_chain_same_detections_observation"] = windows(box_chain, *w)
    # the words pp_mask_iou_pairs has to read at least once: each mask's non-empty word range
    must = int(((dp[2][:, 1] - dp[2][:, 0]).sum() + (gp[2][:, 1] - gp[2][:, 0]).sum()).item()) * 8
    res["mask_iou_pairs_min_bytes"] = must
    res["mask_iou_pairs_achieved_TBps_of_min_bytes"] = must / (res["mask_iou_pairs"]["median_ms"] * 1e-3) / 1e12
    res["mask_iou_pairs_fraction_of_published_hbm"] = res["mask_iou_pairs_achieved_TBps_of_min_bytes"] / HBM_PUBLISHED_TBS
    ap_dev = chain()[0].cpu().numpy()
    res["coco_mask_AP_of_the_synthetic_set"] = float(ap_dev[ap_dev > -1].mean())
    ap_box = box_chain()[0].cpu().numpy()
    res["coco_box_AP_of_the_synthetic_set"] = float(ap_box[ap_box > -1].mean())
    # the numpy restatement (plain loops) on a few images at an eighth of the size: an observation, not a baseline
    import mask_eval_np as MN
    n, h8, w8 = min(args.host_images, B), max(H // 8, 1), max(W // 8, 1)
    g1 = int(host[5][n])
    dm = draw(db[:n].reshape(-1, 4) / 8.0, det_ell[:n * D], h8, w8).cpu().numpy()
    gm = draw(gb[:g1] / 8.0, gt_ell[:g1], h8, w8).cpu().numpy()
    t0 = time.perf_counter()
    MN.mask_iou_pairs(MN.mask_pack(dm), MN.mask_pack(gm), host[5][:n + 1], D, host[2][:n])
    res["host_restatement_pack_and_iou_observation"] = dict(images=n, height=h8, width=w8, ms=(time.perf_counter() - t0) * 1e3)
    print(json.dumps(res, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
