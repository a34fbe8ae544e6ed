#!/usr/bin/env python3
"""Throughput of batched ICP (pp_icp_f64): P problems of --src source points (an ellipsoid surface, 60 mm across, millimetres)
against --tgt target points (another sampling of it at a random pose 500-900 mm away, with 0.2 mm noise), starting 0.5-1
degree / 1-3 mm off (larger starts send some point-to-plane problems on this closed surface off to no correspondences,
which ends them early and would shorten the timed work; the cost of a pass does not depend on the pose),
--iters ICP iterations with the convergence test switched off (relative thresholds 0) and a 100 mm correspondence
distance, so every problem runs all of them,
both estimation modes.  Timed with device events around the whole launch sequence after --warmup runs; medians of --runs.
Prints one JSON line and writes it to profiles/ (--out).  The FLOP count assumed for the correspondence pass is
P x src x tgt x (iters + 1) float64 distance evaluations of 8 flops (3 sub, 3 mul, 2 add); the solves are not counted.
Usage: python3 tools/bench_icp.py [--problems 8 32 104] [--src 2048] [--tgt 8192] [--iters 30] [--runs 10] [--warmup 2]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyrapose_amd import ops  # noqa: E402
from pyrapose_amd._lib import check, lib  # noqa: E402
from pyrapose_amd.runtime import default_context  # noqa: E402

DIST = 100.0  # correspondence distance (mm): every source point keeps a partner, so no problem stops early


def surface(n, rng):
    """n random points of an ellipsoid with semi-axes 30 / 21 / 15 mm and their exact normals"""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    ax = np.array([30.0, 21.0, 15.0])
    p = u * ax
    nrm = p / ax ** 2
    return p, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def rot(axis, deg):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.radians(deg)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def problems(P, ns, nt, rng):
    src, tgt, tn, init = [], [], [], []
    for _ in range(P):
        s, _ = surface(ns, rng)
        q, n = surface(nt, rng)
        R, t = rot(rng.normal(size=3), rng.uniform(0, 180)), np.array([rng.uniform(-80, 80), rng.uniform(-60, 60), rng.uniform(500, 900)])
        tgt.append(q @ R.T + t + rng.normal(scale=0.2, size=q.shape))
        tn.append(n @ R.T)
        dt = rng.normal(size=3)
        T0 = np.eye(4)
        T0[:3, :3] = rot(rng.normal(size=3), rng.uniform(0.5, 1.0)) @ R
        T0[:3, 3] = t + dt * rng.uniform(1, 3) / np.linalg.norm(dt)
        src.append(s)
        init.append(T0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    so = dev(np.arange(P + 1, dtype=np.int32) * ns)
    to = dev(np.arange(P + 1, dtype=np.int32) * nt)
    return so, to, dev(np.concatenate(src)), dev(np.concatenate(tgt)), dev(np.concatenate(tn)), dev(np.stack(init))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, nargs="+", default=[8, 32, 104])
    ap.add_argument("--src", type=int, default=2048)
    ap.add_argument("--tgt", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_icp.json"))
    args = ap.parse_args()
    ctx = default_context()
    rng = np.random.default_rng(0)
    flop_per_eval = 8
    rows = []
    for P in args.problems:
        so, to, src, tgt, tn, init = problems(P, args.src, args.tgt, rng)
        for mode in ("point_to_plane", "point_to_point"):
            out = ops.icp(ctx, so, to, src, tgt, init, DIST, args.iters, 0.0, 0.0, mode, tn if mode == "point_to_plane" else None)
            assert int(out[4].min()) == args.iters and int(out[5].max()) == 0, (
                "every problem must run all iterations: iterations %s, status %s" % (out[4].tolist(), out[5].tolist()))
            # the timed call is the C entry point itself on preallocated buffers (ops.icp adds a host check of the offsets)
            nbytes = lib.pp_icp_workspace_bytes(P, args.src)
            ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
            bufs = [torch.empty_like(o) for o in out]
            ptr = lambda t: ops._ptr(t)
            nrm = tn if mode == "point_to_plane" else None

            def run():
                check(lib.pp_icp_f64(ctx.handle, P, ptr(so), ptr(to), args.src, ptr(src), ptr(tgt), ptr(nrm), ptr(init), DIST, args.iters,
                                     0.0, 0.0, ops.ICP_MODES[mode], ptr(ws), nbytes, *[ptr(b) for b in bufs]), ctx.handle, "pp_icp_f64")

            for _ in range(args.warmup):
                run()
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(out, bufs)), "the C call must reproduce ops.icp"
            ts = []
            for _ in range(args.runs):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e-3)
            med = float(np.median(ts))
            passes = args.iters + 1
            flops = float(P) * args.src * args.tgt * passes * flop_per_eval
            rows.append(dict(problems=P, mode=mode, src_points=args.src, tgt_points=args.tgt, iterations=args.iters,
                             seconds_median=med, seconds_min=float(np.min(ts)), problems_per_s=P / med,
                             ms_per_iteration=1e3 * med / passes, corr_flops_assumed=flops, corr_tflops=flops / med * 1e-12))
    res = dict(tool="bench_icp", device=torch.cuda.get_device_name(0), flop_per_distance_eval=flop_per_eval,
               note="one pp_icp_f64 call: 2 x (iterations + 1) + 2 launches, preallocated buffers", rows=rows)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
