#!/usr/bin/env python3
"""One pp_vsd_multi_f64 launch at BOP's ten misalignment tolerances against ten pp_vsd_f64 launches, on the problems of
tools/bench_vsd.py: 64 rendered pose pairs of a 60 mm mesh at 720 x 540, scene depth = the ground-truth render in front of a
plane at 1200 mm, once shared by all problems and once per problem, estimates independent of the ground truth (as there) and
near it; delta 15, taus 0.05 ... 0.5 x 60 mm, both pixel costs,
visibility rule 'bop18' on both sides so that the two must return the same values (checked before anything is timed: 'step'
exactly, 'tlinear' within 1e-12 relative; whether the bits are the same is reported).
Device time between two events around --inner back-to-back calls, --repeats windows per variant, the two variants
alternating; per leg the median, minimum and maximum of the windows' time per call.  Prints one JSON line (and writes it to
--out).  Usage: python3 tools/bench_vsd_bop.py [--poses 64] [--inner 20] [--repeats 9] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_vsd import mesh, rot  # noqa: E402
from pyrapose_amd import ops  # noqa: E402
from pyrapose_amd.runtime import default_context  # noqa: E402


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner  # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--lat", type=int, default=100)
    ap.add_argument("--lon", type=int, default=101)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = default_context()
    rng = np.random.default_rng(0)
    W, H, n = 720, 540, args.poses
    pts, faces = mesh(args.lat, args.lon, rng)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    R = dev(np.stack([rot(rng) for _ in range(2 * n)]))
    t = dev(np.stack([[rng.uniform(-80, 80), rng.uniform(-60, 60), rng.uniform(400, 900)] for _ in range(2 * n)]))
    K4 = dev(np.repeat([[1075.65091572, 1073.90347929, 360.0, 270.0]], 2 * n, 0))
    v, f = dev(pts), dev(faces)
    d_gt = ops.render_depth(ctx, v, f, R[n:], t[n:], K4[:n], W, H, 100.0, 10000.0)
    # the estimates: the independent poses tools/bench_vsd.py pairs the ground truth with (they hardly overlap it), and the
    # ground truth moved by a few millimetres (they overlap it, as a detection does: every intersection pixel is costed)
    t_near = t[n:] + dev(rng.normal(0.0, 4.0, (n, 3)))
    estimates = (("independent", ops.render_depth(ctx, v, f, R[:n], t[:n], K4[:n], W, H, 100.0, 10000.0)),
                 ("near_gt", ops.render_depth(ctx, v, f, R[n:], t_near, K4[:n], W, H, 100.0, 10000.0)))
    scenes = torch.where(d_gt > 0, torch.round(d_gt), torch.full_like(d_gt, 1200.0))
    taus = [round(0.05 * k, 2) * 60.0 for k in range(1, 11)]
    result = dict(tool="bench_vsd_bop", width=W, height=H, problems=n, taus=taus, delta=15.0, visib_mode="bop18",
                  inner_calls_per_window=args.inner, windows=args.repeats, device=torch.cuda.get_device_name(0), legs={})
    scene_sets = (("shared", scenes[0].contiguous()), ("per_problem", scenes))
    legs = [(en, d_est, sn, scene, cost) for en, d_est in estimates for sn, scene in scene_sets for cost in ("step", "tlinear")]
    for est_name, d_est, scene_name, scene, cost in legs:
        multi = lambda: ops.vsd_multi(ctx, scene, d_est, d_gt, K4[:n], 15.0, taus, cost, "bop18")
        ten = lambda: [ops.vsd(ctx, scene, d_est, d_gt, K4[:n], 15.0, tau, cost) for tau in taus]
        e_multi = multi()[0].cpu().numpy()
        e_ten = np.stack([r[0].cpu().numpy() for r in ten()], axis=1)
        same_bits = bool(np.array_equal(e_multi, e_ten))
        if not (same_bits if cost == "step" else np.allclose(e_multi, e_ten, rtol=1e-12, atol=0)):
            raise SystemExit("bench_vsd_bop: the two variants disagree (%s, %s, %s)" % (est_name, scene_name, cost))
        for _ in range(args.warmup):
            window(multi, args.inner)
            window(ten, args.inner)
        tm, tt = [], []
        for _ in range(args.repeats):
            tm.append(window(multi, args.inner))
            tt.append(window(ten, args.inner))
        stat = lambda x: dict(median=round(float(np.median(x)), 4), min=round(float(np.min(x)), 4), max=round(float(np.max(x)), 4))
        result["legs"]["%s_%s_%s" % (est_name, scene_name, cost)] = dict(
            one_multi_launch_ms=stat(tm), ten_single_launches_ms=stat(tt),
            ten_over_one=round(float(np.median(tt) / np.median(tm)), 3), same_bits=same_bits,
            mean_e_first_and_last_tau=[round(float(e_multi[:, 0].mean()), 4), round(float(e_multi[:, -1].mean()), 4)])
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
