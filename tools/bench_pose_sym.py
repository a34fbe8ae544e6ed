#!/usr/bin/env python3
"""Throughput of BOP's symmetry-aware pose errors (pp_pose_mssd_f64 / pp_pose_mspd_f64) in poses per second, 64 pose pairs of
one model per launch, at n_pts in {2 000, 20 000} model points x n_sym in {1, 2, 630} symmetries (630: one continuous symmetry
at BOP's default step with one discrete one).  Synthetic scenes of tests/pose_sym_np.py: random points, poses 400-1200 mm in
front of a LineMOD-like camera, random rigid symmetry sets with the identity first.  Times ops.pose_mssd / ops.pose_mspd on
device tensors (workspace allocation and the two launches each); writes the figures to --out (JSON).
Usage: python3 tools/bench_pose_sym.py [--iters 20] [--out profiles/bench_pose_sym.json]"""
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
from tests import pose_sym_np as SN  # noqa: E402


def timed(fn, iters, min_seconds=0.25):
    """seconds per call: one warm-up call, then rounds of `iters` calls (each round ends in a synchronise) until the window
    is at least min_seconds long"""
    out = fn()
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while calls == 0 or time.perf_counter() - t0 < min_seconds:
        for _ in range(iters):
            out = fn()
        torch.cuda.synchronize()
        calls += iters
    return out, (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--n-pts", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--n-sym", type=int, nargs="+", default=[1, 2, 630])
    ap.add_argument("--out", default="profiles/bench_pose_sym.json")
    args = ap.parse_args()
    ctx = default_context()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rng = np.random.default_rng(0)
    rows = []
    for n_pts in args.n_pts:
        pts, R_est, t_est, R_gt, t_gt = SN.scene(rng, args.poses, n_pts)
        p, re_, te_, rg, tg = (dev(a) for a in (pts, R_est, t_est, R_gt, t_gt))
        k9 = dev(np.broadcast_to(SN.K_LINEMOD, (args.poses, 3, 3)))
        for n_sym in args.n_sym:
            sr, st = (dev(a) for a in SN.random_symmetries(rng, n_sym))
            (e3, _s3), dt3 = timed(lambda: ops.pose_mssd(ctx, p, sr, st, re_, te_, rg, tg), args.iters)
            (e2, _s2), dt2 = timed(lambda: ops.pose_mspd(ctx, p, sr, st, k9, re_, te_, rg, tg), args.iters)
            assert bool(torch.isfinite(e3).all()) and bool(torch.isfinite(e2).all())
            rows.append(dict(n_pts=n_pts, n_sym=n_sym, mssd_ms=dt3 * 1e3, mspd_ms=dt2 * 1e3, mssd_poses_per_s=args.poses / dt3,
                             mspd_poses_per_s=args.poses / dt2, point_distances_per_launch=args.poses * n_pts * n_sym))
            print("n_pts=%6d n_sym=%4d poses=%d: mssd %.3f ms (%.0f poses/s), mspd %.3f ms (%.0f poses/s)" %
                  (n_pts, n_sym, args.poses, dt3 * 1e3, args.poses / dt3, dt2 * 1e3, args.poses / dt2))
    result = dict(device=torch.cuda.get_device_name(0), iters=args.iters, poses=args.poses, rows=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
