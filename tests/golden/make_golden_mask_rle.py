#!/usr/bin/env python3
"""Golden vectors for the run-length encoding (test infrastructure, runs ONLY where the reference checkout is at hand).

Loads the reference's unmodified ``annotation_scripts/misc.py`` by path from make_golden.REF (nothing copied into this
repository), with stub modules for ``yaml``, ``cv2``, ``transforms3d``, ``OpenEXR`` and ``Imath``, which the module imports at
its top and ``rle_encode`` never uses; numpy is the real one.  Calls ``rle_encode`` on seeded 0 / 1 masks and writes
tests/golden/mask_rle.npz: `masks` uint8 [n,H,W] and `strings`, the returned string of each.

The masks (13 x 17, not square, H W = 221 is no multiple of 64): all zero; all one; first pixel set; last pixel set; first and
last; a checkerboard (the most runs a mask can have); its complement; single pixels; a filled rectangle; a rectangle touching
the right edge, so that runs join across rows; three random masks of density 0.1, 0.5 and 0.9.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

REF = make_golden.REF
H, W = 13, 17


def load_reference():
    for name in ("yaml", "cv2", "transforms3d", "OpenEXR", "Imath"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    spec = importlib.util.spec_from_file_location("ref_misc", os.path.join(REF, "annotation_scripts/misc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def masks():
    rng = np.random.default_rng(20261020)
    out = [np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)]
    for pixels in ([(0, 0)], [(H - 1, W - 1)], [(0, 0), (H - 1, W - 1)]):
        m = np.zeros((H, W), np.uint8)
        for y, x in pixels:
            m[y, x] = 1
        out.append(m)
    board = ((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2).astype(np.uint8)
    out += [board, 1 - board]
    single = np.zeros((H, W), np.uint8)
    single[[1, 4, 4, 9], [3, 0, 16, 8]] = 1
    out.append(single)
    rect = np.zeros((H, W), np.uint8)
    rect[3:9, 4:11] = 1
    out.append(rect)
    edge = np.zeros((H, W), np.uint8)
    edge[2:6, 12:W] = 1
    edge[3:5, 0:2] = 1
    out.append(edge)
    for p in (0.1, 0.5, 0.9):
        out.append((rng.uniform(size=(H, W)) < p).astype(np.uint8))
    return np.stack(out)


def main():
    ref = load_reference()
    m = masks()
    strings = np.array([ref.rle_encode(x) for x in m])
    path = os.path.join(HERE, "mask_rle.npz")
    np.savez_compressed(path, masks=m, strings=strings)
    print("wrote", path, os.path.getsize(path), "bytes;", len(m), "masks, longest string", max(len(s) for s in strings))


if __name__ == "__main__":
    main()
