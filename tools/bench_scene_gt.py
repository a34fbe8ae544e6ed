#!/usr/bin/env python3
"""Scene ground truth on the device (utils.scene_gt.scene_gt_info -> pp_scene_gt_info) on 64 scenes of 8 instances of two
meshes (the mesh of tools/bench_vsd.py at two resolutions, interleaved within every scene) at 640 x 480 and 720 x 540, with
sensor depth (the rounded scene in front of a plane at 1200 mm, resident on the device) and without (the scene depth is composed
from the instances).  Per leg three timings:
  from_poses_ms        utils.scene_gt.scene_gt_info: one render launch per mesh, the gather into scene order, the pass, the
                       results copied to the host (counts, boxes, id images; no masks)
  device_pass_ms       ops.scene_gt_info alone on the stack already rendered (its three kernels)
  visib_fract_batch_ms the only route that overlapped before: utils.pose_error.visib_fract_batch on the same instances, one call
                       per mesh with each instance's scene depth -- it renders too, but returns one ratio per instance and no
                       mask, box or id image, and needs sensor depth (null in the legs without)
The two routes compute different amounts, so the numbers are an observation, not a comparison of like with like; the visible
fractions of both are checked to be equal before anything is timed.  Device time between two events around --inner back-to-back
calls (each call ends in a copy to the host), --repeats windows per variant, the variants alternating; per leg the median,
minimum and maximum of the windows' time per call.  Prints one JSON line (and writes it to --out).
Usage: python3 tools/bench_scene_gt.py [--scenes 64] [--per-scene 8] [--inner 20] [--repeats 9] [--warmup 2] [--out FILE]"""
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
from pyrapose_amd.utils import pose_error as PE  # noqa: E402
from pyrapose_amd.utils import scene_gt as SG  # noqa: E402
from pyrapose_amd.utils._host import k4, to_device  # noqa: E402
from pyrapose_amd.utils.renderer import render_depth_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=64)
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
        models[obj_id] = {"pts": pts, "faces": faces}
    scenes = [[{"obj_id": 1 + (i + s) % 2, "R": rot(rng), "t": [rng.uniform(-80, 80), rng.uniform(-60, 60), rng.uniform(400, 900)]}
               for i in range(args.per_scene)] for s in range(args.scenes)]
    plan = SG.plan_instances(scenes)
    n = len(plan.obj_ids)
    result = dict(tool="bench_scene_gt", scenes=args.scenes, instances=n, triangles={k: int(len(m["faces"])) for k, m in models.items()},
                  delta=15.0, inner_calls_per_window=args.inner, windows=args.repeats, device=torch.cuda.get_device_name(0), legs={})
    stat = lambda x: dict(median=round(float(np.median(x)), 4), min=round(float(np.min(x)), 4), max=round(float(np.max(x)), 4))
    for W, H in ((640, 480), (720, 540)):
        K = np.array([[1075.65091572 * W / 720.0, 0.0, W / 2.0], [0.0, 1073.90347929 * H / 540.0, H / 2.0], [0.0, 0.0, 1.0]])
        renders = [render_depth_batch(models[o], (W, H), K, plan.R[idx], plan.t[idx], ctx=ctx) for o, idx in plan.groups.items()]
        stack = torch.cat(renders)[torch.from_numpy(plan.order).cuda()]
        K4 = to_device(k4(K, n))
        composed = ops.scene_gt_info(ctx, stack, plan.scene_offsets, K4).scene_depth
        sensor = torch.where(composed > 0, torch.round(composed), torch.full_like(composed, 1200.0))
        per_mesh = [(o, np.asarray(idx), sensor[torch.from_numpy(plan.scene_of[idx]).cuda()].contiguous()) for o, idx in plan.groups.items()]
        for name, depth in (("sensor", sensor), ("composed", None)):
            from_poses = lambda: SG.scene_gt_info(scenes, models, K, depth, (W, H))
            device_pass = lambda: ops.scene_gt_info(ctx, stack, plan.scene_offsets, K4, depth)
            before = lambda: [PE.visib_fract_batch(plan.R[idx], plan.t[idx], models[o], d, K) for o, idx, d in per_mesh]
            variants = [("from_poses_ms", from_poses), ("device_pass_ms", device_pass)] + ([("visib_fract_batch_ms", before)] if depth is not None else [])
            got = from_poses()
            fract = np.array([row["visib_fract"] for rows in got.info for row in rows])
            if depth is not None:
                old = np.empty(n)
                for (_o, idx, _d), f in zip(per_mesh, before()):
                    old[idx] = f
                if not np.array_equal(old, fract):
                    raise SystemExit("bench_scene_gt: the visible fractions of the two routes differ (%d x %d)" % (W, H))
            times = {k: [] for k, _ in variants}
            for _ in range(args.warmup):
                for _k, fn in variants:
                    window(fn, args.inner)
            for _ in range(args.repeats):
                for k, fn in variants:
                    times[k].append(window(fn, args.inner))
            leg = {k: stat(v) for k, v in times.items()}
            leg.setdefault("visib_fract_batch_ms", None)
            leg["mean_visib_fract"] = round(float(fract.mean()), 4)
            leg["id_pixels"] = int((got.id_images > 0).sum())
            result["legs"]["%dx%d_%s" % (W, H, name)] = leg
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
