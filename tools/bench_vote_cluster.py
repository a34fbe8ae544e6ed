#!/usr/bin/env python3
"""Cost of clustering votes into object instances (pp_vote_cluster) beside the pose tail it feeds, at the T-LESS inference shape
(BASELINE configs[4]: C = 30, 720x540 -> N = 72 369 anchors) with B = 32 images.  Synthetic votes: in every image `--classes`
classes hold two instances of `--votes` votes each (make_votes of tests/test_oracle_pnp.py: 1 px noise, 20 % outlier votes,
boxes moved a box width apart), every other score stays below the threshold.
Times ops.vote_cluster alone (the memsets and the one launch) and pose_decode.poses_from_outputs with instances=None (what the
parent commit runs: one pooled problem per class) and with instances={...}; writes the figures to --out (JSON).
Usage: python3 tools/bench_vote_cluster.py [--iters 20] [--out profiles/bench_vote_cluster.json]"""
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
from pyrapose_amd.utils import pose_decode  # noqa: E402
from tests.cluster_np import BOX, K4, separated_poses  # noqa: E402


def timed(fn, iters):
    out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n-class", type=int, default=30)
    ap.add_argument("--anchors", type=int, default=72369)
    ap.add_argument("--classes", type=int, default=4, help="classes with votes per image")
    ap.add_argument("--votes", type=int, default=40, help="votes per instance")
    ap.add_argument("--out", default="profiles/bench_vote_cluster.json")
    args = ap.parse_args()
    ctx = default_context()
    B, C, N, k = args.batch, args.n_class, args.anchors, args.votes
    g = torch.Generator(device="cuda").manual_seed(0)
    boxes3d = torch.rand((B, N, 16), device="cuda", generator=g) * 600.0
    scores = torch.rand((B, N, C), device="cuda", generator=g) * 0.3
    rng = np.random.default_rng(0)
    for b in range(B):
        anchors = rng.permutation(N)[:2 * k * args.classes].reshape(args.classes, 2, k)
        for c in range(args.classes):
            for j, (_R, _t, votes, _clean) in enumerate(separated_poses(rng, 2, k, 1.0, 0.2)):
                a = torch.from_numpy(np.sort(anchors[c, j])).cuda()
                boxes3d[b, a] = torch.from_numpy(votes.astype(np.float32)).cuda()
                scores[b, a, c] = torch.from_numpy(rng.uniform(0.55, 0.99, size=k).astype(np.float32)).cuda()
    corners = np.tile(BOX[None], (C, 1, 1))
    Kmat = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])
    (idx, cnt), dt_compact = timed(lambda: ops.score_threshold_compact(ctx, scores, 0.5), args.iters)
    got, dt_cluster = timed(lambda: ops.vote_cluster(ctx, boxes3d, scores, idx, cnt, 0.5, 10, 8), args.iters)
    n_inst = int(got[3].sum())
    pooled, dt_pooled = timed(lambda: pose_decode.poses_from_outputs(boxes3d, scores, corners, Kmat, ctx=ctx), max(args.iters // 4, 2))
    per, dt_inst = timed(lambda: pose_decode.poses_from_outputs(boxes3d, scores, corners, Kmat, ctx=ctx, instances=dict(iou=0.5)),
                         max(args.iters // 4, 2))
    result = dict(device=torch.cuda.get_device_name(0), iters=args.iters, batch=B, n_class=C, anchors=N, classes_with_votes=args.classes,
                  votes_per_instance=k, instances_found=n_inst, instances_placed=2 * B * args.classes,
                  score_threshold_compact_ms=dt_compact * 1e3, vote_cluster_ms=dt_cluster * 1e3,
                  poses_from_outputs_pooled_ms=dt_pooled * 1e3, poses_from_outputs_instances_ms=dt_inst * 1e3,
                  poses_pooled=len(pooled), poses_instances=len(per))
    print("B=%d C=%d N=%d: vote_cluster %.3f ms per call (%d instances of %d placed); score_threshold_compact %.3f ms; "
          "poses_from_outputs %.2f ms pooled (%d poses), %.2f ms per instance (%d poses)" %
          (B, C, N, dt_cluster * 1e3, n_inst, 2 * B * args.classes, dt_compact * 1e3, dt_pooled * 1e3, len(pooled), dt_inst * 1e3, len(per)))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
