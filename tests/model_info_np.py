"""float64 numpy restatement of the model-geometry entry points (csrc/model_info.hip, utils/model_info.py), loops made explicit:
the diameter of a point set (bop_toolkit_lib.misc.calc_pts_diameter, restated -- no bop_toolkit at hand), greedy farthest-point
sampling (the reference's FPS.py:37-94, restated -- it needs open3d and a stale package name -- and the standard min-distance
rule) and the 3-D box corners of annotation_scripts/annotate_BOP.py:204-219.  Every squared distance is
(dx * dx + dy * dy) + dz * dz, each product and sum rounded on its own, which is also what numpy's
(diff * diff).sum(axis=1) evaluates on rows of three."""
import math

import numpy as np


def d2_rows(p, q):
    """p [a,3] against q [b,3] -> [a,b] squared distances in the stated association"""
    dx = p[:, None, 0] - q[None, :, 0]
    dy = p[:, None, 1] - q[None, :, 1]
    dz = p[:, None, 2] - q[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def diameter_np(pts, block=512):
    """(d2 float64 [1], pair int32 [2]): max over i <= j of d2(p_i, p_j) and the pair that attains it -- the lowest i, then the
    lowest j.  Blocked over rows of i; pairs j < i are masked out, never computed as zero points."""
    pts = np.asarray(pts, np.float64)
    n = pts.shape[0]
    row_max, row_arg = np.empty(n), np.empty(n, np.int64)
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        D = d2_rows(pts[i0:i1], pts[i0:])          # columns j >= i0 only: the rest of these rows has j < i
        D[np.tril_indices(i1 - i0, -1)] = -1.0     # and j < i inside the diagonal block
        row_arg[i0:i1] = i0 + D.argmax(axis=1)     # the first maximum: the lowest j
        row_max[i0:i1] = D[np.arange(i1 - i0), row_arg[i0:i1] - i0]
    i = int(row_max.argmax())                      # the first maximum: the lowest i
    return np.array([row_max[i]], np.float64), np.array([i, row_arg[i]], np.int32)


def calc_pts_diameter_np(pts):
    """bop_toolkit_lib.misc.calc_pts_diameter restated literally: its loop over rows, the difference of the row against itself
    and everything after it, the root of each row's maximum.  O(n^2) with a Python loop: small n only."""
    pts = np.asarray(pts, np.float64)
    diameter = -1.0
    for pt_id in range(pts.shape[0]):
        pt_dup = np.tile(np.array([pts[pt_id, :]]), [pts.shape[0] - pt_id, 1])
        pts_diff = pt_dup - pts[pt_id:, :]
        max_dist = math.sqrt((pts_diff * pts_diff).sum(axis=1).max())
        if max_dist > diameter:
            diameter = max_dist
    return diameter


def fps_min_dist_np(pts):
    """FPS.py:49-59"""
    pts = np.asarray(pts, np.float64)
    x_dim = np.max(pts[:, 0]) - np.min(pts[:, 0])
    y_dim = np.max(pts[:, 1]) - np.min(pts[:, 1])
    z_dim = np.max(pts[:, 2]) - np.min(pts[:, 2])
    return (x_dim + y_dim + z_dim) / 7


def farthest_np(pts, k, rule="min", start=None, min_dist=None, round32=True):
    """k greedy picks from pts [n,3] -> int64 [k].  start None: the first maximum of (x x + y y) + z z (FPS.py:40-42, the
    norm's argmax on squares).  rule 'min': score = min over the chosen of d2, next = np.argmax(score).  rule 'sum'
    (FPS.py:62-94): the chosen point is rounded to float32 (control_points is float32; round32=False leaves that out, for the
    test that shows the rounding matters), score = the sum of the distances in the order chosen, 0.0 where any of them is
    below min_dist (None: FPS.py's own), next = np.argmax(score) -- index 0 when every score is 0."""
    pts = np.asarray(pts, np.float64)
    n = pts.shape[0]
    if start is None:
        start = int(np.argmax((pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2]))
    if rule == "sum" and min_dist is None:
        min_dist = fps_min_dist_np(pts)
    chosen = [int(start)]
    score = np.full(n, np.inf) if rule == "min" else np.zeros(n)
    skipped = np.zeros(n, bool)
    for _ in range(int(k) - 1):
        c = pts[chosen[-1]]
        if rule == "sum" and round32:
            c = c.astype(np.float32).astype(np.float64)
        q = d2_rows(pts, c[None])[:, 0]
        if rule == "min":
            score = np.minimum(score, q)
            chosen.append(int(np.argmax(score)))
        else:
            d = np.sqrt(q)
            score = score + d
            skipped |= d < min_dist
            chosen.append(int(np.argmax(np.where(skipped, 0.0, score))))
    return np.array(chosen, np.int64)


def three_boxes_np(info, n_classes, fac=1.0):
    """annotate_BOP.py:198-219 on an info dict (fac as annotate_synthetic_LineMOD_train.py:38-44 applies it): float32 [C,8,3]"""
    # the reference's corner order as (x, y, z) signs: '+' = min + size, '-' = min
    order = ("+++", "++-", "+--", "+-+", "-++", "-+-", "---", "--+")
    out = np.zeros((n_classes, 8, 3), dtype=np.float32)
    for key, value in info.items():
        for corner, signs in enumerate(order):
            for a, (axis, sign) in enumerate(zip("xyz", signs)):
                minus = value["min_" + axis] * fac
                out[int(key), corner, a] = value["size_" + axis] * fac + minus if sign == "+" else minus
    return out
