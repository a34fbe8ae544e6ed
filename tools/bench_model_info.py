#!/usr/bin/env python3
"""Time of the model-geometry entry points (pp_pts_diameter_f64 / pp_farthest_points_f64, csrc/model_info.hip) on device
tensors: the diameter of one point set at 7 000, 20 000 and 250 000 points, of 30 sets of 20 000 points one after the other, and
farthest-point sampling (rule 'min' and the reference's rule 'sum') at k = 8 and 64 of one 20 000-point model and of 30 in one
launch.  Random points of a LineMOD-sized object (millimetres).  Each figure is the median of 9 windows of 20 calls (a window
ends in a synchronise); the spread is (slowest - fastest window) / median.  The diameter's pair rate n (n + 1) / 2 / time stands
next to the float64 vector rate of the device (78.6 TFLOP/s on an MI355X by AMD's published figure; a pair is 3 subtractions,
3 products, 2 sums and a comparison).  --cpu times the literal restatement of bop_toolkit's calc_pts_diameter
(tests/model_info_np.py) once at 7 000 points on this host, an observation beside the device figure.
Usage: python3 tools/bench_model_info.py [--windows 9] [--iters 20] [--cpu] [--out profiles/bench_model_info.json]"""
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
from tests import model_info_np as MN  # noqa: E402

FP64_VECTOR_TFLOPS = 78.6   # MI355X, AMD's published peak = half the float32 vector rate (157.3); not measured by this project
FLOP_PER_PAIR = 8           # 3 subtractions, 3 products, 2 sums (the comparison and the selects not counted)


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


def cloud(rng, n):
    return rng.normal(size=(n, 3)) * (40.0, 25.0, 60.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--n-pts", type=int, nargs="+", default=[7000, 20000, 250000])
    ap.add_argument("--models", type=int, default=30)
    ap.add_argument("--model-pts", type=int, default=20000)
    ap.add_argument("--k", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--cpu", action="store_true", help="also time the literal calc_pts_diameter restatement at 7 000 points on the host")
    ap.add_argument("--out", default="profiles/bench_model_info.json")
    args = ap.parse_args()
    ctx = default_context()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rng = np.random.default_rng(0)
    rows = []

    def report(row):
        rows.append(row)
        print(" ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in row.items()), flush=True)

    for n in args.n_pts:
        p = dev(cloud(rng, n))
        iters = args.iters
        dt, spread = windows(lambda: ops.pts_diameter(ctx, p), args.windows, iters)
        pairs = n * (n + 1) // 2
        report(dict(leg="diameter", n_pts=n, calls_per_window=iters, ms=dt * 1e3, spread=spread, pairs_per_s=pairs / dt,
                    tflops_fp64=pairs * FLOP_PER_PAIR / dt / 1e12, fraction_of_fp64_vector_peak=pairs * FLOP_PER_PAIR / dt / 1e12 / FP64_VECTOR_TFLOPS))
    models = [dev(cloud(rng, args.model_pts)) for _ in range(args.models)]
    dt, spread = windows(lambda: [ops.pts_diameter(ctx, p) for p in models], args.windows, args.iters)
    report(dict(leg="diameter_models_in_sequence", models=args.models, n_pts=args.model_pts, calls_per_window=args.iters, ms=dt * 1e3,
                spread=spread, ms_per_model=dt * 1e3 / args.models))
    flat = torch.cat(models)
    offs_all = np.arange(args.models + 1, dtype=np.int32) * args.model_pts
    md_all = dev(np.array([MN.fps_min_dist_np(p.cpu().numpy()) for p in models]))
    for rule in ("min", "sum"):
        for k in args.k:
            for m, pts, offs, md in ((1, models[0], offs_all[:2], md_all[:1]), (args.models, flat, offs_all, md_all)):
                fn = lambda: ops.farthest_points(ctx, pts, offs, k, rule, md if rule == "sum" else None)
                dt, spread = windows(fn, args.windows, args.iters)
                report(dict(leg="farthest_points", rule=rule, k=k, models=m, n_pts=args.model_pts, calls_per_window=args.iters, ms=dt * 1e3,
                            spread=spread, us_per_pick=dt * 1e6 / k))
    cpu = None
    if args.cpu:
        host = cloud(rng, 7000)
        t0 = time.perf_counter()
        d = MN.calc_pts_diameter_np(host)
        cpu = dict(leg="calc_pts_diameter_restated_on_host", n_pts=7000, seconds=time.perf_counter() - t0, diameter=d, runs=1)
        print(cpu, flush=True)
    result = dict(device=torch.cuda.get_device_name(0), windows=args.windows, iters=args.iters, window_rule="median of the windows' seconds per call; "
                  "spread = (slowest - fastest window) / median", fp64_vector_peak_tflops=FP64_VECTOR_TFLOPS, flop_per_pair=FLOP_PER_PAIR, rows=rows,
                  host_observation=cpu)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
