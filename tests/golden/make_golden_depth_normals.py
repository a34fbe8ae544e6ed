#!/usr/bin/env python3
"""Golden vectors for the depth normal images (test infrastructure, runs ONLY where the reference checkout is at hand).

Loads the reference's unmodified ``annotation_scripts/Augmentations.py`` by path from make_golden.REF (nothing copied into this
repository), with stub modules for ``cv2``, ``pyfastnoisesimd`` and ``imgaug`` / ``imgaug.augmenters``, which the module imports
at its top and ``get_normal`` never uses; scipy and numpy are the real ones.  Calls ``get_normal`` on seeded synthetic depth
maps and writes tests/golden/depth_normals.npz: the inputs and both return values, for both modes where both are pinned.

  A  48x64, depth positive everywhere: a tilted plane plus a smooth bump plus integer-rounded noise, a block beyond 2000 so
     that the far cut fires; non-integer intrinsics inside the image, so the int16 truncation acts on both sides of the
     principal point.  Both modes.
  B  37x53, the same recipe with a few zero-depth holes, each smaller than the 17x17 filter support, so the smoothed depth is
     never exactly 0.  Both modes.
  C  66x80 (the smallest at which a hole wider than the 17 taps stays within 1/16 of the image), case A's recipe with one
     18x18 zero hole: its 2x2 core smooths to exactly 0, and there the reference's cross product of two parallel tangents is
     rounding noise.
     for_vis=True only: under for_vis=False such a pixel carries the largest factor and can set the image's maximum.
  D  5x7, shorter than the filter radius on both axes.  for_vis=True only.

The depths are whole numbers, so float32 (what the device takes) holds them exactly.  Also prints the largest difference between
the reference and the restatement tests/depth_normals_np.py, from which tests/test_depth_normals_cpu.py takes its bounds.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import depth_normals_np as DN  # noqa: E402

REF = make_golden.REF


def load_reference():
    for name in ("cv2", "pyfastnoisesimd", "imgaug", "imgaug.augmenters"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["imgaug"].augmenters = sys.modules["imgaug.augmenters"]
    spec = importlib.util.spec_from_file_location("ref_augmentations", os.path.join(REF, "annotation_scripts/Augmentations.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scene(rng, H, W, far_block=True):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    plane = 700.0 + 6.0 * x + 9.0 * y
    bump = 180.0 * np.exp(-(((x - 0.6 * W) / (0.2 * W)) ** 2 + ((y - 0.4 * H) / (0.25 * H)) ** 2))
    depth = np.rint(plane - bump + rng.integers(-3, 4, size=(H, W)))
    if far_block:
        depth[H // 8:H // 8 + H // 3, W // 10:W // 10 + W // 3] += 1900.0
    assert depth.min() > 0 and np.array_equal(depth, depth.astype(np.float32))
    return depth


def intrinsics(H, W):
    """the LineMOD camera scaled to the image: non-integer, the principal point inside"""
    s = W / 640.0
    return 572.4114 * s, 573.57043 * s, 325.2611 * s, 242.04899 * H / 480.0


def main():
    ref = load_reference()
    rng = np.random.default_rng(20261020)
    cases = {}
    A = scene(rng, 48, 64)
    cases["A"] = (A, intrinsics(48, 64), (True, False))
    B = scene(rng, 37, 53)
    for (r, c, h, w) in ((3, 5, 6, 9), (20, 30, 11, 4), (30, 2, 5, 14), (0, 40, 7, 7)):
        B[r:r + h, c:c + w] = 0.0
    cases["B"] = (B, intrinsics(37, 53), (True, False))
    C = scene(rng, 66, 80)
    C[30:48, 50:68] = 0.0  # 18 x 18 = 324 pixels <= 66 * 80 / 16 = 330: a 2 x 2 core whose whole 17 x 17 window is zero
    cases["C"] = (C, intrinsics(66, 80), (True,))
    D = scene(rng, 5, 7, far_block=False)
    cases["D"] = (D, intrinsics(5, 7), (True,))
    out = {}
    worst_n = worst_d = 0.0
    for name, (depth, (fx, fy, cx, cy), modes) in cases.items():
        out[name + "_depth"] = depth
        out[name + "_intr"] = np.array([fx, fy, cx, cy], np.float64)
        for for_vis in modes:
            with np.errstate(all="ignore"):
                n, d = ref.get_normal(depth.copy(), fx=fx, fy=fy, cx=cx, cy=cy, for_vis=for_vis)
            tag = "%s_vis%d" % (name, int(for_vis))
            out[tag + "_normals"], out[tag + "_smoothed"] = n, d
            mine = DN.depth_normals(depth, fx, cx, cy, for_vis=for_vis)
            keep = d != 0
            excluded = 1.0 - keep.mean()
            dd = np.abs(mine["depth"] - d)[keep]
            rel = (dd / np.abs(d[keep])).max()
            if for_vis:
                dn = np.abs(mine["normals"] - n)[keep].max()
                worst_n, worst_d = max(worst_n, dn), max(worst_d, rel)
                print("%s: excluded %.4f, normals max abs diff %.3e, depth max rel diff %.3e" % (tag, excluded, dn, rel))
            else:
                du = np.abs(mine["normals_u8"].astype(np.int32) - n.astype(np.int32))
                worst_d = max(worst_d, rel)
                print("%s: excluded %.4f, uint8 values that differ %d (max %d), depth max rel diff %.3e" %
                      (tag, excluded, int((du != 0).sum()), int(du.max()), rel))
    print("worst over the fixture: normals %.3e abs, depth %.3e rel" % (worst_n, worst_d))
    path = os.path.join(HERE, "depth_normals.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
