#!/usr/bin/env python3
"""The colour renderer on the device (ops.render_rgbd -> pp_render_rgbd) beside the depth pass (ops.render_depth ->
pp_render_depth_f32) on the same poses in the same process: 64 poses of each of the two meshes of tools/bench_scene_gt.py (the
mesh of tools/bench_vsd.py at two resolutions, random vertex colours, the smooth surface's normals) at 640 x 480 and 720 x 540,
phong shaded, tensors resident on the device.  Per leg (mesh, size):
  rgbd_all_ms     pp_render_rgbd with depth, tri_id, rgb_f32 and rgb_u8
  rgb_u8_ms       pp_render_rgbd with rgb_u8 alone
  depth_ms        pp_render_depth_f32
and their ratios to depth_ms; the depth output of the first is checked to be the depth pass's bits before anything is timed.
Per size also the scene path end to end, scene_ms: utils.scene_gt.render_scenes on 64 scenes of 8 instances of the two meshes
(both meshes rendered in colour and depth, the ground-truth pass, the composed uint8 images left on the device, the counts and
boxes copied to the host).  Device time between two events around --inner back-to-back calls, --repeats windows per variant,
the variants alternating; per variant the median, minimum and maximum of the windows' time per call.  Prints one JSON line
(and writes it to --out).
Usage: python3 tools/bench_render_rgb.py [--poses 64] [--inner 20] [--repeats 9] [--warmup 2] [--out FILE]"""
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
from pyrapose_amd import ops  # noqa: E402
from pyrapose_amd.runtime import default_context  # noqa: E402
from pyrapose_amd.utils import scene_gt as SG  # noqa: E402
from pyrapose_amd.utils._host import k4, to_device  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--per-scene", type=int, default=8)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = default_context()
    rng = np.random.default_rng(0)
    models = {}
    for obj_id, (lat, lon) in ((1, (100, 101)), (2, (60, 61))):
        pts, faces = mesh(lat, lon, rng)
        normals = pts / np.array([1.0, 0.49, 0.25])  # the gradient of the ellipsoid the mesh ripples about; the kernel normalises
        models[obj_id] = {"pts": pts, "faces": faces, "colors": rng.uniform(size=pts.shape), "normals": normals}
    n = args.poses
    R = np.stack([rot(rng) for _ in range(n)])
    t = np.stack([[rng.uniform(-80, 80), rng.uniform(-60, 60), rng.uniform(400, 900)] for _ in range(n)])
    scenes = [[{"obj_id": 1 + (i + s) % 2, "R": rot(rng), "t": [rng.uniform(-80, 80), rng.uniform(-60, 60), rng.uniform(400, 900)]}
               for i in range(args.per_scene)] for s in range(n)]
    result = dict(tool="bench_render_rgb", poses=n, scenes=n, instances_per_scene=args.per_scene, shading="phong",
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
            shade = dict(colors=to_device(m["colors"]), normals=to_device(m["normals"]), shading="phong")
            rgbd_all = lambda: ops.render_rgbd(ctx, *mesh_args, outputs=("rgb", "rgb_f32", "depth", "tri_id"), **shade)
            rgb_u8 = lambda: ops.render_rgbd(ctx, *mesh_args, outputs=("rgb",), **shade)
            depth = lambda: ops.render_depth(ctx, *mesh_args)
            first = rgbd_all()
            if not torch.equal(first["depth"], depth()):
                raise SystemExit("bench_render_rgb: the depth of pp_render_rgbd is not the depth pass's (%d x %d, mesh %d)" % (W, H, obj_id))
            leg = run([("rgbd_all_ms", rgbd_all), ("rgb_u8_ms", rgb_u8), ("depth_ms", depth)])
            leg["rgbd_all_over_depth"] = round(leg["rgbd_all_ms"]["median"] / leg["depth_ms"]["median"], 3)
            leg["rgb_u8_over_depth"] = round(leg["rgb_u8_ms"]["median"] / leg["depth_ms"]["median"], 3)
            leg["covered_fraction"] = round(float((first["tri_id"] >= 0).float().mean().item()), 4)
            result["legs"]["%dx%d_mesh%d" % (W, H, obj_id)] = leg
        scene = lambda: SG.render_scenes(scenes, models, K, (W, H))
        images, _info = scene()
        leg = run([("scene_ms", scene)])
        leg["nonblack_fraction"] = round(float((images.amax(dim=-1) > 0).float().mean().item()), 4)
        result["legs"]["%dx%d_scenes" % (W, H)] = leg
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
