#!/usr/bin/env python3
"""Time of the symmetry score (pp_sym_hausdorff_f64, csrc/model_info.hip) on device tensors: 2 000 x 20 000 and 20 000 x 20 000
points (source x target) with 64 and 512 candidate transformations, in point pairs per second (K n m pairs per call).  Beside
it, in the same process, pp_pose_adi_f64 on the target's 20 000 points with the same transformations as its estimates (identity
ground truth): K n n pairs of the same arithmetic with a sum in place of the maximum, one candidate per workgroup -- its pair
rate is the yardstick (it has no 2 000 x 20 000 form: one point set).  Then one whole utils.model_info.find_symmetries on a
20 000-vertex mesh (a lathe surface with one continuous axis; sample = 0.01, tol = 0.03), median of 3 runs.  Random points of a LineMOD-sized
object (millimetres); each kernel figure is the median of 9 windows of 20 calls (a window ends in a synchronise), the spread is
(slowest - fastest window) / median.  The float64 vector peak beside the rates is AMD's published figure, not measured by this
project.
Usage: python3 tools/bench_model_sym.py [--windows 9] [--iters 20] [--out profiles/bench_model_sym.json]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrapose_amd import ops  # noqa: E402
from pyrapose_amd.runtime import default_context  # noqa: E402
from pyrapose_amd.utils.model_info import find_symmetries  # noqa: E402
from pyrapose_amd.utils.symmetry import _rotation  # noqa: E402

FP64_VECTOR_TFLOPS = 78.6   # MI355X, AMD's published peak; not measured by this project
FLOP_PER_PAIR = 8           # 3 subtractions, 3 products, 2 sums (the comparison and the select not counted)


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


def lathe_mesh(n_z=100, n_theta=200):
    """a surface of revolution about z, n_z x n_theta vertices, two triangles per grid cell"""
    z = np.linspace(-60.0, 60.0, n_z)
    r = 30.0 + 10.0 * np.sin(z / 25.0) + 0.05 * z
    th = 2.0 * math.pi * np.arange(n_theta) / n_theta
    pts = np.stack([np.outer(r, np.cos(th)), np.outer(r, np.sin(th)), np.repeat(z[:, None], n_theta, axis=1)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n_z - 1), np.arange(n_theta), indexing="ij")
    a, b = i * n_theta + j, i * n_theta + (j + 1) % n_theta
    faces = np.concatenate([np.stack([a, b, a + n_theta], -1).reshape(-1, 3), np.stack([b, b + n_theta, a + n_theta], -1).reshape(-1, 3)])
    return {"pts": pts, "faces": faces}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--n-src", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--n-tgt", type=int, default=20000)
    ap.add_argument("--cands", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--out", default="profiles/bench_model_sym.json")
    args = ap.parse_args()
    ctx = default_context()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rng = np.random.default_rng(0)
    rows = []

    def report(row):
        rows.append(row)
        print(" ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in row.items()), flush=True)

    tgt_host = rng.normal(size=(args.n_tgt, 3)) * (40.0, 25.0, 60.0)
    tgt = dev(tgt_host)
    for K in args.cands:
        S_R = np.stack([_rotation(rng.uniform(0.0, math.pi), rng.normal(size=3)) for _ in range(K)])
        S_t = rng.normal(size=(K, 3))
        dS_R, dS_t = dev(S_R), dev(S_t)
        eye_R, eye_t = dev(np.tile(np.eye(3), (K, 1, 1))), dev(np.zeros((K, 3)))
        for n in args.n_src:
            src = tgt[:n].contiguous()
            dt, spread = windows(lambda: ops.sym_hausdorff(ctx, src, tgt, dS_R, dS_t), args.windows, args.iters)
            pairs = K * n * args.n_tgt
            report(dict(leg="sym_hausdorff", n_src=n, n_tgt=args.n_tgt, candidates=K, calls_per_window=args.iters, ms=dt * 1e3, spread=spread,
                        pairs_per_s=pairs / dt, fraction_of_fp64_vector_peak=pairs * FLOP_PER_PAIR / dt / 1e12 / FP64_VECTOR_TFLOPS))
        dt, spread = windows(lambda: ops.pose_errors(ctx, tgt, dS_R, dS_t, eye_R, eye_t, symmetric=True), args.windows, args.iters)
        pairs = K * args.n_tgt * args.n_tgt
        report(dict(leg="pose_adi", n_pts=args.n_tgt, poses=K, calls_per_window=args.iters, ms=dt * 1e3, spread=spread, pairs_per_s=pairs / dt,
                    fraction_of_fp64_vector_peak=pairs * FLOP_PER_PAIR / dt / 1e12 / FP64_VECTOR_TFLOPS))
    mesh = lathe_mesh()
    kw = dict(sample=0.01, tol=0.03)   # a sampled cloud's own residual stays below (1 + sqrt 3) * sample
    found = find_symmetries(mesh, **kw)   # warm-up
    torch.cuda.synchronize()
    secs = []
    for _ in range(3):
        t0 = time.perf_counter()
        found = find_symmetries(mesh, **kw)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    report(dict(leg="find_symmetries", vertices=int(mesh["pts"].shape[0]), faces=int(mesh["faces"].shape[0]), runs=3, sample=kw["sample"], tol=kw["tol"],
                seconds=float(np.median(secs)), spread=(max(secs) - min(secs)) / float(np.median(secs)),
                discrete=len(found.get("symmetries_discrete", [])), continuous=len(found.get("symmetries_continuous", []))))
    result = dict(device=torch.cuda.get_device_name(0), windows=args.windows, iters=args.iters, window_rule="median of the windows' seconds per call; "
                  "spread = (slowest - fastest window) / median", fp64_vector_peak_tflops=FP64_VECTOR_TFLOPS, flop_per_pair=FLOP_PER_PAIR, rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
