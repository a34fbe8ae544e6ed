#!/usr/bin/env python3
"""Time of the mesh-geometry entry points (pp_mesh_face_geometry_f64 / pp_mesh_vertex_normals_f64 / pp_mesh_sample_surface_f64,
csrc/mesh.hip) on device tensors: face geometry and face geometry + vertex normals of a 7 k- and a 20 k-triangle sphere
(tests/mesh_np.sphere, millimetres of a LineMOD-sized object), and 2^16 and 2^20 surface samples of the 20 k mesh in both modes
(points, faces, barycentrics and normals written).  Beside each stands a copy_ of the leg's output tensor into a buffer of the
same size: what moving the bytes alone costs.  Each figure is the median of 9 windows of 20 calls (a window ends in a
synchronise); the spread is (slowest - fastest window) / median.  --host runs the host sampler utils.icp._mesh_samples once at a
spacing that gives a comparable count: an observation only -- it places a grid per triangle and computes something else.
Usage: python3 tools/bench_mesh.py [--windows 9] [--iters 20] [--host] [--out profiles/bench_mesh.json]"""
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
from tests import mesh_np as MN  # noqa: E402

MESHES = {"7k": (60, 59), "20k": (101, 100)}   # (n_lat, n_lon) -> 2 n_lon (n_lat - 1) triangles: 6 962 and 20 000


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--samples", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--host", action="store_true", help="also run the host sampler utils.icp._mesh_samples once (an observation)")
    ap.add_argument("--out", default="profiles/bench_mesh.json")
    args = ap.parse_args()
    ctx = default_context()
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    rows = []

    def report(row):
        rows.append(row)
        print(" ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in row.items()), flush=True)

    def leg(name, fn, out_of, **extra):
        dt, spread = windows(fn, args.windows, args.iters)
        src = out_of(fn())
        dst = torch.empty_like(src)
        ct, cspread = windows(lambda: dst.copy_(src), args.windows, args.iters)
        report(dict(leg=name, calls_per_window=args.iters, us=dt * 1e6, spread=spread, copy_of_output_us=ct * 1e6, copy_spread=cspread,
                    output_bytes=src.numel() * src.element_size(), **extra))

    meshes = {}
    for tag, (n_lat, n_lon) in MESHES.items():
        p, f = MN.sphere(n_lat, n_lon, radius=80.0)
        P, F = dev(p, np.float64), dev(f, np.int32)
        meshes[tag] = (p, f, P, F)
        size = dict(mesh=tag, n_v=len(p), n_f=len(f))
        leg("face_geometry", lambda: ops.mesh_face_geometry(ctx, P, F), lambda g: g["normal"], **size)
        leg("face_geometry_and_vertex_normals", lambda: ops.mesh_vertex_normals(ctx, len(p), F, ops.mesh_face_geometry(ctx, P, F)),
            lambda o: o[0], **size)
    p, f, P, F = meshes["20k"]
    geom = ops.mesh_face_geometry(ctx, P, F)
    for n in args.samples:
        for mode in ("random", "weyl"):
            leg("sample_surface", lambda: ops.mesh_sample_surface(ctx, P, F, geom, n, 0, mode), lambda o: o["points"], mesh="20k", n_f=len(f),
                n_samples=n, mode=mode)
    host = None
    if args.host:
        from pyrapose_amd.utils.icp import _mesh_samples
        t0 = time.perf_counter()
        S, _ = _mesh_samples(p, f.astype(np.int64), 0.55)
        host = dict(leg="host_mesh_samples_observation", mesh="20k", spacing=0.55, n_points=int(len(S)), seconds=time.perf_counter() - t0, runs=1,
                    note="a barycentric grid per triangle for a voxel filter: not the same computation, not a baseline")
        print(host, flush=True)
    result = dict(device=torch.cuda.get_device_name(0), windows=args.windows, iters=args.iters,
                  window_rule="median of the windows' seconds per call; spread = (slowest - fastest window) / median", rows=rows,
                  host_observation=host)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
