#!/usr/bin/env python3
"""Throughput of the device weighted-PnP refinement (pp_pnp_refine_weighted_f64) beside the RANSAC launch
(pp_pnp_ransac_f64) on the same problems, for the two shapes it is used in:
  corners: 2048 problems x 8 correspondences (per-corner mean + weight from pp_vote_stats_f64): the one-wave-per-problem path;
  votes:   256 problems x 320 correspondences (40 votes x 8 corners, every vote a correspondence): the workgroup path.
Prints problems/s of each launch and the ratio; writes the figures to --out (JSON).
Usage: python3 tools/bench_wpnp.py [--iters 20] [--out profiles/bench_wpnp.json]"""
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
from tests.wpnp_scenes import BOX, K4A, rot_err_deg, scene  # noqa: E402


def timed(fn, iters):
    out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--votes", type=int, default=40)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = default_context()
    dev = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    result = dict(device=torch.cuda.get_device_name(0), iters=args.iters, shapes={})
    for name, P in (("corners", 2048), ("votes", 256)):
        k = args.votes
        scs = [scene(s, k) for s in range(P)]
        offs = dev(8 * k * np.arange(P + 1, dtype=np.int32), torch.int32)
        obj, img = dev(np.concatenate([s["obj"] for s in scs])), dev(np.concatenate([s["img"] for s in scs]))
        K = dev(np.tile(K4A, (P, 1)))
        (R, t, n_in, mask, ok), dt_ransac = timed(lambda: ops.pnp_ransac(ctx, offs, obj, img, K, 300, 5.0, 1, 8), max(args.iters // 4, 2))
        st, dt_stats = timed(lambda: ops.vote_stats(ctx, offs, img, 8, None, mask, "full", 0.5, check_offsets=False), args.iters)
        if name == "corners":
            o8 = dev(8 * np.arange(P + 1, dtype=np.int32), torch.int32)
            a = (o8, dev(np.tile(BOX, (P, 1))), st["mu"].reshape(-1, 2), st["wgt"].reshape(-1, 3))
        else:
            w = st["wgt"][:, None].expand(P, k, 8, 3).reshape(-1, 3) * mask.double()[:, None]
            a = (offs, obj, img, w.contiguous())
        ref, dt = timed(lambda: ops.pnp_refine_weighted(ctx, *a, K, R, t, check_offsets=False), args.iters)
        Rr, Rn = ref["R"].cpu().numpy(), R.cpu().numpy()
        e_ref = float(np.median([rot_err_deg(Rr[p], scs[p]["R"]) for p in range(P)]))
        e_ran = float(np.median([rot_err_deg(Rn[p], scs[p]["R"]) for p in range(P)]))
        n = int(a[1].shape[0]) // P
        result["shapes"][name] = dict(problems=P, correspondences=n, path="one wave per problem" if n <= 64 else "one workgroup per problem",
                                      refine_ms=dt * 1e3, refine_problems_per_s=P / dt, vote_stats_ms=dt_stats * 1e3, ransac_ms=dt_ransac * 1e3,
                                      ransac_problems_per_s=P / dt_ransac, refine_over_ransac_time=dt / dt_ransac,
                                      passes_mean=float(ref["iterations"].double().mean()), converged=int((ref["status"] == 0).sum()),
                                      median_rot_err_deg_refined=e_ref, median_rot_err_deg_ransac=e_ran)
        print("%s: %d problems x %d correspondences (%s): refine %.3f ms = %.0f problems/s (%.1f passes); vote_stats %.3f ms; RANSAC %.2f ms = "
              "%.0f problems/s; refine / RANSAC time %.4f; median rotation error %.3f deg refined, %.3f deg RANSAC" %
              (name, P, n, result["shapes"][name]["path"], dt * 1e3, P / dt, result["shapes"][name]["passes_mean"], dt_stats * 1e3,
               dt_ransac * 1e3, P / dt_ransac, dt / dt_ransac, e_ref, e_ran))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
