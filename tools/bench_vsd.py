#!/usr/bin/env python3
"""Throughput of the depth renderer (pp_render_depth_f32) and of VSD (pp_vsd_f64) at 720 x 540, the T-LESS image size
(BASELINE configs[4]): a synthetic closed mesh of about 20 k triangles (a bumpy ellipsoid, 60 mm across, millimetres) at
n poses between 400 and 900 mm, K of the T-LESS Primesense camera.  Prints one JSON line: renders/s, VSD problems/s (on
depth images already rendered) and VSD problems/s end to end (two renders per problem + VSD), medians of --iters timed runs
after --warmup.  There is no fused render + VSD path, so nothing is compared against one.
Usage: python3 tools/bench_vsd.py [--poses 64] [--lat 100] [--lon 101] [--iters 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrapose_amd import ops  # noqa: E402
from pyrapose_amd.runtime import default_context  # noqa: E402


def mesh(n_lat, n_lon, rng):
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = 30.0 * (1.0 + 0.05 * np.sin(5 * T) * np.cos(7 * P))
    ring = np.stack([r * np.sin(T) * np.cos(P), 0.7 * r * np.sin(T) * np.sin(P), 0.5 * r * np.cos(T)], -1).reshape(-1, 3)
    pts = np.concatenate([[[0, 0, 15.0]], ring, [[0, 0, -15.0]]])
    faces = [[0, 1 + j, 1 + (j + 1) % n_lon] for j in range(n_lon)]
    for i in range(n_lat - 2):
        for j in range(n_lon):
            a, b = 1 + i * n_lon + j, 1 + i * n_lon + (j + 1) % n_lon
            faces += [[a, a + n_lon, b], [b, a + n_lon, b + n_lon]]
    last, base = len(pts) - 1, 1 + (n_lat - 2) * n_lon
    faces += [[base + j, last, base + (j + 1) % n_lon] for j in range(n_lon)]
    return pts, np.array(faces, np.int32)


def rot(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--lat", type=int, default=100)
    ap.add_argument("--lon", type=int, default=101)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
    render = lambda k: ops.render_depth(ctx, v, f, R[:k], t[:k], K4[:k], W, H, 100.0, 10000.0)
    depth = render(2 * n)
    scene = depth[n].clone()
    vsd = lambda: ops.vsd(ctx, scene, depth[:n], depth[n:], K4[:n], 0.3, 20.0, "step")

    def end_to_end():
        d = render(2 * n)
        return ops.vsd(ctx, scene, d[:n], d[n:], K4[:n], 0.3, 20.0, "step")

    t_r, t_r_min = timed(lambda: render(n), args.iters, args.warmup)
    t_v, t_v_min = timed(vsd, args.iters, args.warmup)
    t_e, t_e_min = timed(end_to_end, args.iters, args.warmup)
    covered = float((depth[:n] > 0).float().mean().item())
    print(json.dumps(dict(tool="bench_vsd", width=W, height=H, poses=n, vertices=int(len(pts)), triangles=int(len(faces)),
                          covered_fraction=round(covered, 4), render_ms=round(t_r * 1e3, 4), render_ms_min=round(t_r_min * 1e3, 4),
                          renders_per_s=round(n / t_r, 1), vsd_ms=round(t_v * 1e3, 4), vsd_ms_min=round(t_v_min * 1e3, 4),
                          vsd_problems_per_s=round(n / t_v, 1), end_to_end_ms=round(t_e * 1e3, 4),
                          end_to_end_problems_per_s=round(n / t_e, 1), fused="none", device=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
