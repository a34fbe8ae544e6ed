#!/usr/bin/env python3
"""The textured colour pass (ops.render_rgbd_tex -> pp_render_rgbd_tex) beside the vertex-colour pass (ops.render_rgbd ->
pp_render_rgbd) on the same poses in the same process: 64 poses of each of the two meshes of tools/bench_render_rgb.py (random
vertex colours, the smooth surface's normals, UVs from the mesh's own latitude / longitude grid stretched over [-0.25, 1.25] so
that wrapping is exercised) at 640 x 480 and 720 x 540, phong shaded, outputs rgb (uint8) and depth, tensors resident on the
device.  Per leg (mesh, size):
  vertex_alone_ms     pp_render_rgbd, vertex colours, in windows of its own (what --untextured-only measures)
  vertex_ms           the same, its windows alternating with those of the textured variants
  tex_nearest_ms      pp_render_rgbd_tex, nearest, clamp, a 512 x 512 texture
  tex_bilinear_512_ms pp_render_rgbd_tex, bilinear, repeat, 512 x 512 (1 MiB: stays in the caches)
  tex_bilinear_2048_ms the same with a 2048 x 2048 texture (16 MiB)
and each ratio to vertex_ms; depth and triangle ids of the textured call are checked to be the vertex-colour call's before
anything is timed.  Device time between two events around --inner back-to-back calls, --repeats windows per variant, the
variants alternating; per variant the median, minimum and maximum of the windows' time per call.
--untextured-only times vertex_alone_ms only: with PP_LIB naming a build of the parent commit this is the same tool's untextured time
there, and --parent FILE (that run's output) records it beside this tree's vertex_alone_ms with the verdict
untextured_within_spread: the two medians differ by no more than the wider of the two window spreads (max - min).
Prints one JSON line (and writes it to --out).
Usage: python3 tools/bench_render_tex.py [--poses 64] [--inner 20] [--repeats 9] [--warmup 2] [--untextured-only]
       [--parent FILE] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_vsd import mesh, rot  # noqa: E402
from bench_vsd_bop import window  # noqa: E402
from pyrapose_amd import _lib, ops  # noqa: E402
from pyrapose_amd.runtime import default_context  # noqa: E402
from pyrapose_amd.utils._host import k4, to_device  # noqa: E402


def grid_uv(lat, lon):
    """(u, v) of bench_vsd.mesh's vertices: longitude and latitude of its grid, the poles at u = 0.5"""
    T, P = np.meshgrid(np.arange(1, lat) / lat, np.arange(lon) / lon, indexing="ij")
    ring = np.stack([P, T], -1).reshape(-1, 2)
    return -0.25 + 1.5 * np.concatenate([[[0.5, 0.0]], ring, [[0.5, 1.0]]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--untextured-only", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = default_context()
    rng = np.random.default_rng(0)
    models = {}
    for obj_id, (lat, lon) in ((1, (100, 101)), (2, (60, 61))):
        pts, faces = mesh(lat, lon, rng)
        normals = pts / np.array([1.0, 0.49, 0.25])  # the gradient of the ellipsoid the mesh ripples about; the kernel normalises
        models[obj_id] = {"pts": pts, "faces": faces, "colors": rng.uniform(size=pts.shape), "normals": normals, "uv": grid_uv(lat, lon)}
    textures = {s: torch.from_numpy(rng.integers(0, 256, size=(s, s, 4)).astype(np.uint8)).cuda() for s in (512, 2048)}
    n = args.poses
    R = np.stack([rot(rng) for _ in range(n)])
    t = np.stack([[rng.uniform(-80, 80), rng.uniform(-60, 60), rng.uniform(400, 900)] for _ in range(n)])
    result = dict(tool="bench_render_tex", poses=n, shading="phong", outputs=["rgb", "depth"], untextured_only=args.untextured_only,
                  library=os.path.basename(_lib.LIB_PATH),
                  triangles={k: int(len(m["faces"])) for k, m in models.items()}, inner_calls_per_window=args.inner, windows=args.repeats,
                  device=torch.cuda.get_device_name(0), legs={})
    stat = lambda x: dict(median=round(float(np.median(x)), 4), min=round(float(np.min(x)), 4), max=round(float(np.max(x)), 4))

    def run(variants):
        times = {k: [] for k, _ in variants}
        for _ in range(args.warmup):
            for _k, fn in variants:
                window(fn, args.inner)
        for _ in range(args.repeats):
            for k, fn in variants:
                times[k].append(window(fn, args.inner))
        return {k: stat(v) for k, v in times.items()}

    for W, H in ((640, 480), (720, 540)):
        K = np.array([[1075.65091572 * W / 720.0, 0.0, W / 2.0], [0.0, 1073.90347929 * H / 540.0, H / 2.0], [0.0, 0.0, 1.0]])
        Rd, td, K4 = to_device(R), to_device(t), to_device(k4(K, n))
        for obj_id, m in models.items():
            mesh_args = (to_device(m["pts"]), to_device(m["faces"], torch.int32), Rd, td, K4, W, H)
            normals, colors, uv = to_device(m["normals"]), to_device(m["colors"]), to_device(m["uv"])
            vertex = lambda: ops.render_rgbd(ctx, *mesh_args, colors=colors, normals=normals, shading="phong", outputs=("rgb", "depth"))
            variants = [("vertex_ms", vertex)]
            if not args.untextured_only:
                tex = lambda size, filter, wrap: (lambda: ops.render_rgbd_tex(ctx, *mesh_args, uv=uv, tex=textures[size], filter=filter, wrap=wrap,
                                                                              normals=normals, shading="phong", outputs=("rgb", "depth")))
                variants += [("tex_nearest_ms", tex(512, "nearest", "clamp")), ("tex_bilinear_512_ms", tex(512, "bilinear", "repeat")),
                             ("tex_bilinear_2048_ms", tex(2048, "bilinear", "repeat"))]
                want = ops.render_rgbd(ctx, *mesh_args, outputs=("depth", "tri_id"))
                got = ops.render_rgbd_tex(ctx, *mesh_args, uv=uv, tex=textures[512], filter="bilinear", wrap="repeat", normals=normals,
                                          outputs=("rgb", "depth", "tri_id"))
                if not (torch.equal(got["depth"], want["depth"]) and torch.equal(got["tri_id"], want["tri_id"])):
                    raise SystemExit("bench_render_tex: depth or ids of pp_render_rgbd_tex are not pp_render_rgbd's (%d x %d, mesh %d)" % (W, H, obj_id))
            alone = run(variants[:1])["vertex_ms"]  # as --untextured-only times it: no textured call between its windows
            leg = run(variants) if len(variants) > 1 else {"vertex_ms": alone}
            leg["vertex_alone_ms"] = alone
            for k, _ in variants[1:]:
                leg[k[:-3] + "_over_vertex"] = round(leg[k]["median"] / leg["vertex_ms"]["median"], 3)
            leg["covered_fraction"] = round(float((vertex()["depth"] > 0).float().mean().item()), 4)
            result["legs"]["%dx%d_mesh%d" % (W, H, obj_id)] = leg
    if args.parent:
        with open(args.parent) as f:
            parent = json.loads(f.readline())
        result["parent_library"] = parent.get("library")
        ok = True
        for name, leg in result["legs"].items():
            a, b = leg["vertex_alone_ms"], parent["legs"][name]["vertex_alone_ms"]
            leg["parent_vertex_ms"] = b
            leg["vertex_over_parent"] = round(a["median"] / b["median"], 4)
            leg["within_spread"] = bool(abs(a["median"] - b["median"]) <= max(a["max"] - a["min"], b["max"] - b["min"]))
            ok = ok and leg["within_spread"]
        result["untextured_within_spread"] = ok
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
