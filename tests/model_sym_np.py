"""float64 numpy restatement of the symmetry score (pp_sym_hausdorff_f64, csrc/model_info.hip): for every candidate rigid
transformation S_k the squared one-sided Hausdorff distance of the moved source to the target,
    d2[k] = max_i min_j d2(S_k src_i, tgt_j),
with the pair (i, j) that attains it: the lowest i that attains the maximum, and for that i the lowest j that attains its
minimum.  The move is written element by element in the association of pose.hip's rigid() --
R[0] * x + R[1] * y + R[2] * z + t[0], left to right -- not as a matrix product, which may fuse or reorder; the squared
distance is tests/model_info_np.d2_rows: (dx * dx + dy * dy) + dz * dz."""
import math

import numpy as np

from tests.model_info_np import d2_rows


def move_np(R, t, pts):
    """S p for the rows of pts [n,3]: every product and sum rounded on its own, left to right"""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([R[0, 0] * x + R[0, 1] * y + R[0, 2] * z + t[0],
                     R[1, 0] * x + R[1, 1] * y + R[1, 2] * z + t[1],
                     R[2, 0] * x + R[2, 1] * y + R[2, 2] * z + t[2]], axis=1)


def sym_hausdorff_np(src, tgt, S_R, S_t, block=512):
    """(d2 float64 [K], arg int32 [K,2]); tgt None = src.  Blocked over the rows of the moved source."""
    src = np.asarray(src, np.float64)
    tgt = src if tgt is None else np.asarray(tgt, np.float64)
    S_R, S_t = np.asarray(S_R, np.float64).reshape(-1, 3, 3), np.asarray(S_t, np.float64).reshape(-1, 3)
    K, n = S_R.shape[0], src.shape[0]
    d2, arg = np.empty(K, np.float64), np.empty((K, 2), np.int32)
    for k in range(K):
        moved = move_np(S_R[k], S_t[k], src)
        row_min, row_arg = np.empty(n), np.empty(n, np.int64)
        for i0 in range(0, n, block):
            D = d2_rows(moved[i0:i0 + block], tgt)
            row_arg[i0:i0 + block] = D.argmin(axis=1)      # the first minimum: the lowest j
            row_min[i0:i0 + block] = D[np.arange(D.shape[0]), row_arg[i0:i0 + block]]
        i = int(row_min.argmax())                          # the first maximum: the lowest i
        d2[k] = row_min[i]
        arg[k] = (i, row_arg[i])
    return d2, arg


def scorer(src, tgt, S_R, S_t):
    """the restatement in the form utils.model_info's host logic takes its scoring function"""
    return sym_hausdorff_np(src, tgt, S_R, S_t)


def diameter_of(pts):
    """the diameter in the form the host logic takes it (numpy; small clouds only)"""
    return math.sqrt(float(d2_rows(pts, pts).max()))


# ---- the shapes of the find_symmetries tests and their groups ------------------------------------------------------------

OFFSET = np.array([3.0, -2.0, 5.0])   # every shape is translated off the origin


def fixed_rotation():
    """one arbitrary rotation (no axis of a shape stays a coordinate axis): Rodrigues about (1, 2, 3) by 0.7 rad"""
    return rot((1.0, 2.0, 3.0), 0.7)


def rot(axis, angle):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(angle) * Kx + (1.0 - math.cos(angle)) * Kx.dot(Kx)


def box_grid(sx, sy, sz, spacing):
    """the surface points of the grid of `spacing` on the box [-sx/2, sx/2] x [-sy/2, sy/2] x [-sz/2, sz/2]"""
    ax = [np.arange(int(round(s / spacing)) + 1) * spacing - 0.5 * s for s in (sx, sy, sz)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    on = np.zeros(len(g), bool)
    for a, s in enumerate((sx, sy, sz)):
        on |= np.abs(np.abs(g[:, a]) - 0.5 * s) < 1e-9
    return g[on]


def hex_prism(per_edge, heights):
    """rings of 6 edges x per_edge points (corners at radius 1, the first on +x) at `heights`"""
    corner = np.array([[math.cos(math.pi / 3 * k), math.sin(math.pi / 3 * k)] for k in range(7)])
    ring = np.array([corner[k] + (corner[k + 1] - corner[k]) * (m / per_edge) for k in range(6) for m in range(per_edge)])
    return np.array([[x, y, z] for z in heights for x, y in ring])


def cylinder(per_ring, heights):
    ring = [(math.cos(2 * math.pi * k / per_ring), math.sin(2 * math.pi * k / per_ring)) for k in range(per_ring)]
    return np.array([[x, y, z] for z in heights for x, y in ring])


def cut_box(spacing):
    """the 2 x 3 x 4 box without the surface points of its (+, +, +) corner region, plus one point off every plane"""
    g = box_grid(2.0, 3.0, 4.0, spacing)
    cut = (g[:, 0] > 0.2) & (g[:, 1] > 0.7) & (g[:, 2] > 0.9)
    return np.concatenate([g[~cut], [[0.3, 0.2, 2.6]]])


def dihedral(n):
    """the non-identity rotations of D_n: n-fold about z, 2-fold axes in the xy plane every pi / n from +x"""
    return [rot((0, 0, 1), 2 * math.pi * k / n) for k in range(1, n)] + \
           [rot((math.cos(math.pi * k / n), math.sin(math.pi * k / n), 0.0), math.pi) for k in range(n)]


def angle_between(A, B):
    return math.acos(min(1.0, max(-1.0, (np.trace(A.T.dot(B)) - 1.0) / 2.0)))


def check_result(result, pts, expected, tol, Q=None, continuous_axis=None, count=None):
    """The asserts every find_symmetries test makes: the count, every element's residual recomputed by the restatement in both
    directions <= tol * diameter, every element within 0.03 rad of its own member of the expected group `expected` (rotations
    of the axis-aligned placement, conjugated by Q for a rotated one; count: the number of elements where it is not the whole
    group); a continuous axis is compared as a line."""
    Q = np.eye(3) if Q is None else Q
    diameter = diameter_of(pts)
    found = [np.asarray(m, np.float64).reshape(4, 4) for m in result.get("symmetries_discrete", [])]
    print("found", len(found), "discrete, expected", len(expected), "continuous", result.get("symmetries_continuous"))
    assert len(found) == (len(expected) if count is None else count)
    for key in ("symmetries_discrete", "symmetries_continuous"):
        assert key not in result or len(result[key]) > 0      # absent when empty
    matched = set()
    for M in found:
        assert np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0])
        inv_R, t = M[:3, :3].T, M[:3, 3]
        d2, _ = sym_hausdorff_np(pts, None, np.stack([M[:3, :3], inv_R]), np.stack([t, -inv_R.dot(t)]))
        angles = [angle_between(Q.dot(E).dot(Q.T), M[:3, :3]) for E in expected]
        print("  residual / diameter %.3g, nearest expected element at %.3g rad" % (math.sqrt(d2.max()) / diameter, min(angles)))
        assert math.sqrt(d2.max()) <= tol * diameter
        assert min(angles) <= 0.03
        matched.add(int(np.argmin(angles)))
    assert len(matched) == len(found)                         # no member of the group twice
    if continuous_axis is None:
        assert "symmetries_continuous" not in result
    else:
        assert len(result["symmetries_continuous"]) == 1
        entry = result["symmetries_continuous"][0]
        a = np.asarray(entry["axis"], np.float64)
        assert abs(np.linalg.norm(a) - 1.0) < 1e-12 and math.acos(min(1.0, abs(a.dot(Q.dot(continuous_axis))))) <= 0.03
        # the offset lies on the axis through the cloud's centre
        off = np.asarray(entry["offset"], np.float64) - pts.mean(axis=0)
        assert np.linalg.norm(off - a * a.dot(off)) <= tol * diameter
