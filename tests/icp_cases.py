"""The designed inputs of tests/test_gpu_icp_stages.py, built from fixed seeds, and independent float64 references of the five
stages of csrc/icp.hip.  The references share no code with tests/icp_np.py (the restatement of the kernels' own structure):
boolean indexing, a dictionary, np.lexsort, np.linalg.eigh / svd / solve.  tests/test_icp_cases_cpu.py ties the restatement to
them on every case family and asserts the preconditions of the inputs (gaps between best and second-best distances, bit-equal
ties, the eigenvalue-gap gate); the GPU file compares the kernels with the restatement and, where cheap, with these."""
import functools
import math

import numpy as np

from tests.test_icp_cpu import asymmetric_cloud, rot

INTR = (572.4114, 573.57043, 3.7, 1.9)             # fx, fy, cx, cy: cx, cy no integers, so (c - cx) and (r - cy) never vanish
INVALID = np.array([0.0, -0.0, np.nan, np.inf, -np.inf], np.float32)
CLOUD_SHAPES = {1: 3, 255: 4, 256: 5, 257: 5, 513: 4}   # width -> height; 256 columns are one chunk of cloud_scatter_kernel
COARSE_GRID = np.array([[1, 0, 1], [0, 1, 1]], np.uint8)   # 2 x 3: divides none of the images


# ---- independent references ----------------------------------------------------------------------------------------------

def dense_ref(depth, fx, fy, cx, cy, ds):
    """((c - cx) z / fx, (r - cy) z / fy, z) of every pixel, z = float64(depth) ds -> ([h,w,3], z [h,w])"""
    d = np.asarray(depth, np.float32)
    h, w = d.shape
    z = d.astype(np.float64) * ds
    c, r = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return np.stack([(c - cx) * z / fx, (r - cy) * z / fy, z], -1), z


def cloud_ref(depth, fx, fy, cx, cy, ds=1.0, pixel_mask=None):
    """boolean indexing of the dense back-projection, row-major -> (points [n,3], row offsets [h+1]); pixel_mask [h,w] bool"""
    dense, z = dense_ref(depth, fx, fy, cx, cy, ds)
    valid = np.isfinite(z) & (z != 0)
    if pixel_mask is not None:
        valid = valid & np.asarray(pixel_mask, bool)
    return dense[valid], np.concatenate([[0], np.cumsum(valid.sum(1))])


def create_ref(depth, fx, fy, cx, cy, ds):
    """the dense form [h*w,3]: a NaN row where z == 0 (either sign), everything else as the expressions give it"""
    dense, z = dense_ref(depth, fx, fy, cx, cy, ds)
    dense[z == 0] = np.nan
    return dense.reshape(-1, 3)


def voxel_ref(pts, voxel, normals=None):
    """dictionary keyed by floor((p - (min - v/2)) / v); each voxel a sequential sum in original point order; output sorted by
    (ix, iy, iz) -> (means [m,3], unit mean normals [m,3] or None, index triples [m,3], member lists)"""
    P = np.asarray(pts, np.float64)
    lo = P.min(0) - voxel / 2.0
    groups = {}
    for i in range(len(P)):
        groups.setdefault(tuple(int(math.floor((P[i, a] - lo[a]) / voxel)) for a in range(3)), []).append(i)
    keys = sorted(groups)
    means, nrm = [], []
    for k in keys:
        s, q = np.zeros(3), np.zeros(3)
        for i in groups[k]:
            s = s + P[i]
            if normals is not None:
                q = q + np.asarray(normals, np.float64)[i]
        means.append(s / float(len(groups[k])))
        ln = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
        nrm.append(q / ln if ln > 0 else np.zeros(3))
    return np.array(means), (np.array(nrm) if normals is not None else None), np.array(keys), [groups[k] for k in keys]


def neighbours_ref(pts, radius, max_nn):
    """all-pairs d2, np.lexsort((index, d2)), the entries with d2 <= r r, the first max_nn -> list of index arrays"""
    P = np.asarray(pts, np.float64)
    d = P[:, None, :] - P[None, :, :]
    d2 = (d * d).sum(-1)
    idx = np.arange(len(P))
    out = []
    for i in range(len(P)):
        o = np.lexsort((idx, d2[i]))
        out.append(o[d2[i][o] <= radius * radius][:max_nn])
    return out


def normal_ref(pts, nbrs):
    """np.linalg.eigh of the neighbours' covariance: the eigenvector of the smallest eigenvalue with n . p <= 0; zero with
    fewer than 3 neighbours -> (normals [n,3], eigenvalues ascending [n,3], NaN where there is no normal)"""
    P = np.asarray(pts, np.float64)
    N, W = np.zeros_like(P), np.full_like(P, np.nan)
    for i, js in enumerate(nbrs):
        if len(js) < 3:
            continue
        Q = P[js] - P[js].mean(0)
        w, V = np.linalg.eigh(Q.T @ Q / len(js))
        n = V[:, 0]
        N[i], W[i] = (-n if n @ P[i] > 0 else n), w
    return N, W


def gap_ok(W):
    """the gate of the eigh comparison: the two smallest eigenvalues separated by more than 1e-6 of the largest"""
    return (W[:, 1] - W[:, 0]) > 1e-6 * W[:, 2]


def angle(a, b):
    return 2.0 * np.arcsin(np.minimum(np.linalg.norm(a - b, axis=-1) / 2.0, 1.0))


def transform_ref(src, T):
    a, b, c = np.asarray(src, np.float64).T
    T = np.asarray(T, np.float64)
    return np.stack([T[k, 0] * a + T[k, 1] * b + T[k, 2] * c + T[k, 3] for k in range(3)], -1)


def corr_ref(src, tgt, T, max_d, tgt_normals=None):
    """all-pairs argmin (the lowest index of equals) of the source under T; with tgt_normals (plane mode) only targets with a
    non-zero normal; -1 where best > max_d^2 or nothing is usable
    -> dict(corr, best [ns] (inf without a usable target), second [ns], fitness, inlier_rmse, X)"""
    X = transform_ref(src, T)
    tgt = np.asarray(tgt, np.float64)
    ns = len(X)
    d = X[:, None, :] - tgt[None, :, :]
    d2 = (d * d).sum(-1)
    if tgt_normals is not None:
        d2[:, ~np.asarray(tgt_normals, np.float64).any(1)] = np.inf
    if d2.shape[1] == 0:
        d2 = np.full((ns, 1), np.inf)
    j = np.argmin(d2, 1)
    best = d2[np.arange(ns), j]
    rest = d2.copy()
    rest[np.arange(ns), j] = np.inf
    ok = np.isfinite(best) & (best <= max_d * max_d)
    corr = np.where(ok, j, -1)
    return dict(corr=corr, best=best, second=rest.min(1), fitness=ok.sum() / float(ns) if ns else 0.0,
                inlier_rmse=float(np.sqrt(np.mean(best[ok]))) if ok.any() else 0.0, X=X)


def step_point_ref(X, Q):
    """Kabsch by SVD with the determinant fix: the rigid (R, t) that takes X [k,3] onto Q [k,3] in the least-squares sense"""
    xm, qm = X.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - qm).T @ (X - xm))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, qm - R @ xm


def step_plane_ref(X, Q, N):
    """one Gauss-Newton step of sum(((R X + t - Q) . N)^2) linearised about the identity: np.linalg.solve of the 6x6 normal
    equations, R = Rz Ry Rx, t = x[3:6]"""
    J = np.concatenate([np.cross(X, N), N], 1)
    r = ((X - Q) * N).sum(1)
    x = np.linalg.solve(J.T @ J, -(J.T @ r))
    a, b, g = x[:3]
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(g), -math.sin(g), 0], [math.sin(g), math.cos(g), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx, x[3:6]


def one_update_ref(pr, max_d, mode):
    """the pose after one ICP update from pr['init'] -> (R, t)"""
    plane = mode == "point_to_plane"
    c = corr_ref(pr["source"], pr["target"], pr["init"], max_d, pr["target_normals"] if plane else None)
    ok = c["corr"] >= 0
    X, Q = c["X"][ok], np.asarray(pr["target"], np.float64)[c["corr"][ok]]
    Ru, tu = step_plane_ref(X, Q, np.asarray(pr["target_normals"], np.float64)[c["corr"][ok]]) if plane else step_point_ref(X, Q)
    T = np.asarray(pr["init"], np.float64)
    return Ru @ T[:3, :3], Ru @ T[:3, 3] + tu


# ---- cloud ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cloud_image(w):
    """float32 depth [CLOUD_SHAPES[w], w]: row 0 all valid, row 1 all invalid (every invalid value in turn), row 2 valid only
    in the last columns of its last partial chunk, further rows about half valid; one negative finite depth"""
    h = CLOUD_SHAPES[w]
    rng = np.random.default_rng(1000 + w)
    d = rng.uniform(400, 1200, (h, w)).astype(np.float32)
    bad = INVALID[(np.arange(h * w) % len(INVALID))].reshape(h, w)
    d[1] = bad[1]
    last = ((w - 1) // 256) * 256
    keep = np.arange(w) >= max(last, w - 3)
    d[2] = np.where(keep, d[2], bad[2])
    for r in range(3, h):
        d[r] = np.where(rng.uniform(size=w) < 0.5, d[r], bad[r])
    d[0, w // 2] = -650.0
    d.setflags(write=False)
    return d


def cloud_masks(w):
    """name -> (grid uint8 [mh,mw] or None): none, full resolution, coarse, all zero"""
    h = CLOUD_SHAPES[w]
    rng = np.random.default_rng(2000 + w)
    full = (rng.uniform(size=(h, w)) < 0.6).astype(np.uint8)
    full[2, w - 1] = 1
    return {"none": None, "full": full, "coarse": COARSE_GRID, "zero": np.zeros((2, 3), np.uint8)}


# ---- voxels --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def voxel_cases():
    """name -> (pts [n,3], voxel, normals [n,3])"""
    out = {}
    for n in (1, 255, 256, 257, 1000):
        rng = np.random.default_rng(3000 + n)
        p = rng.uniform(-40, 40, (n, 3))
        p[n - 1] = p.min(0) - np.array([1.3, 0.7, 2.1])                 # every axis' minimum at the last index
        out["n%d" % n] = (p, 5.0, rng.normal(size=(n, 3)))
    rng = np.random.default_rng(3100)
    g = np.stack(np.meshgrid(*[np.arange(-2.0, 2.25, 0.25)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))[:600]]
    g[-1] = [-2.0, -2.0, -2.0]
    out["dyadic_faces"] = (g, 0.5, rng.normal(size=g.shape))             # lower corner -2.25: x.25 and x.75 lie on voxel faces
    p = np.array([3.0, -2.0, 700.0]) + rng.uniform(0, 0.2, (100, 3))
    out["one_voxel"] = (p, 5.0, rng.normal(size=p.shape))
    p = np.zeros((257, 3))
    p[:, 0], p[:, 1], p[:, 2] = 10.0 * rng.permutation(257) - 900.0, -10.0 * (np.arange(257) % 3), 10.0 * (np.arange(257) % 5)
    out["own_voxels_257"] = (p, 5.0, rng.normal(size=p.shape))
    big = np.array([100.0, -200.0, 700.0]) + rng.uniform(0, 24, (300, 3)) * 10.0 ** rng.uniform(-6, 0, (300, 1))
    single = np.array([100.0, -200.0, 700.0]) + 100.0 * np.stack([np.arange(1, 21), -np.arange(1, 21), np.arange(1, 21) % 4], 1)
    p = np.concatenate([big, single])[rng.permutation(320)]
    p = np.concatenate([p, [[100.0, -2200.0, 700.0]]])                    # the lower corner, its own voxel
    out["one_big_voxel"] = (p, 50.0, rng.normal(size=p.shape))
    p = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [20.0, 0.0, 0.0], [21.0, 1.0, 0.5], [1.5, 0.5, 0.25], [0.5, 0.25, 1.0]])
    nr = np.array([[0.5, -0.25, 1.0], [-0.5, 0.25, -1.0], [0.0, 0.0, 2.0], [0.0, 3.0, 0.0], [0.25, 0.5, -0.125], [-0.25, -0.5, 0.125]])
    out["cancelling_normals"] = (p, 5.0, nr)                              # voxel 0: four normals that sum to exactly zero
    for v in out.values():
        for a in v[::2]:
            a.setflags(write=False)
    return out


# ---- normals -------------------------------------------------------------------------------------------------------------

NORMAL_SIZES = (1, 2, 63, 64, 65, 129)
LATTICE_RADII, LATTICE_MAX_NN = (1.0, 2.0), (1, 2, 3, 7, 32)


@functools.lru_cache(maxsize=None)
def surface(n):
    """the first n points of a jittered 13 x 10 grid (4 mm) on a curved surface 700 mm from the camera; radius 10, max_nn 10"""
    rng = np.random.default_rng(4000)
    u, v = np.meshgrid(np.arange(13) * 4.0 - 24.0, np.arange(10) * 4.0 - 18.0, indexing="ij")
    p = np.stack([u, v, 700.0 + 0.004 * (u * u) - 0.003 * (v * v) + 0.002 * u * v], -1).reshape(-1, 3)
    p = (p + rng.normal(scale=0.4, size=p.shape))[rng.permutation(len(p))][:n] + np.array([15.0, -10.0, 0.0])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def lattice():
    """5 x 5 x 5 integer lattice, spacing 1, shuffled: d2 is an exact integer, d2 == r r occurs at both radii, a centre point has
    33 points within radius 2 (one more than the 32 the kernel keeps)"""
    g = np.stack(np.meshgrid(np.arange(5.0) - 2.0, np.arange(5.0) - 2.0, np.arange(5.0) + 10.0, indexing="ij"), -1).reshape(-1, 3)
    g = g[np.random.default_rng(4100).permutation(len(g))]
    g.setflags(write=False)
    return g


def isolated_points():
    return np.array([[0.0, 0.0, 500.0], [100.0, 0.0, 500.0], [0.0, 100.0, 500.0], [100.0, 100.0, 600.0], [3.0, 0.0, 500.0]])


def coplanar_patches():
    """(points exactly on a plane, its unit normal toward the origin): z = 600, and z = 600 + x/2 + y/4 on dyadic coordinates"""
    x, y = (a.reshape(-1) for a in np.meshgrid(np.arange(-16.0, 17.0, 4.0), np.arange(-12.0, 13.0, 4.0), indexing="ij"))
    flat = np.stack([x, y, np.full_like(x, 600.0)], 1)
    tilt = np.stack([x, y, 600.0 + 0.5 * x + 0.25 * y], 1)
    n = np.array([0.5, 0.25, -1.0])
    return [(flat, np.array([0.0, 0.0, -1.0])), (tilt, n / np.linalg.norm(n))]


def collinear_points():
    """three points 3 apart along (1,2,2)/3, and two far from them -> (points, line direction)"""
    p = np.array([[10.0, 20.0, 500.0], [11.0, 22.0, 502.0], [12.0, 24.0, 504.0], [300.0, 0.0, 500.0], [-300.0, 0.0, 500.0]])
    return p, np.array([1.0, 2.0, 2.0]) / 3.0


# ---- correspondences -----------------------------------------------------------------------------------------------------

RAGGED_SRC, RAGGED_TGT = (1, 63, 64, 65, 127, 128, 129, 257), (1, 127, 128, 129, 300)
RAGGED_MAX_D = 12.0


def _problem(rng, ns, nt, zero_normals=0.15):
    """random source and target in one 80 x 60 x 50 mm box 700 mm away, a start 1-3 degrees / 1-3 mm off the identity"""
    c = np.array([20.0, -10.0, 700.0])
    src = c + rng.uniform(-1, 1, (ns, 3)) * [40.0, 30.0, 25.0]
    tgt = c + rng.uniform(-1, 1, (nt, 3)) * [40.0, 30.0, 25.0]
    tn = rng.normal(size=(nt, 3))
    tn /= np.linalg.norm(tn, axis=1, keepdims=True)
    tn[rng.uniform(size=nt) < zero_normals] = 0.0
    R = rot(rng.normal(size=3), rng.uniform(1, 3))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, c - R @ c + rng.normal(size=3)
    return dict(source=src, target=tgt, init=T, target_normals=tn)


@functools.lru_cache(maxsize=None)
def ragged_batch():
    """eight problems: every source count of RAGGED_SRC against the target counts of RAGGED_TGT in turn (one problem owns three
    source tiles, most own one)"""
    rng = np.random.default_rng(5000)
    return tuple(_problem(rng, ns, RAGGED_TGT[k % len(RAGGED_TGT)]) for k, ns in enumerate(RAGGED_SRC))


def explicit_problems():
    """name -> (problem, max_d, {mode: expected corr}); identity init and dyadic coordinates, so every distance is exact"""
    I4, z3, up = np.eye(4), np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]])
    out = {}
    t = np.array([[4.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 2.0, 0.0]])
    out["duplicate_targets"] = (dict(source=z3, target=t, init=I4, target_normals=np.repeat(up, 4, 0)), 10.0,
                                {"point_to_point": [1], "point_to_plane": [1]})
    t = np.array([[8.0, 0.0, 0.0], [0.0, 2.0, 0.0], [-2.0, 0.0, 0.0], [0.0, 0.0, 2.0]])
    s = np.array([[0.0, 0.0, 0.0], [-1.0, 1.0, 0.0], [0.0, 1.0, 1.0]])
    out["equidistant_targets"] = (dict(source=s, target=t, init=I4, target_normals=np.repeat(up, 4, 0)), 10.0,
                                  {"point_to_point": [1, 1, 1], "point_to_plane": [1, 1, 1]})
    t = np.array([[3.0, 4.0, 0.0]])
    out["at_max_distance"] = (dict(source=z3, target=t, init=I4, target_normals=up), 5.0,
                              {"point_to_point": [0], "point_to_plane": [0]})
    out["over_max_distance"] = (dict(source=z3, target=t, init=I4, target_normals=up), 4.999,
                                {"point_to_point": [-1], "point_to_plane": [-1]})
    t = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 3.0]])
    tn = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    s = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 2.0]])
    out["nearest_without_normal"] = (dict(source=s, target=t, init=I4, target_normals=tn), 10.0,
                                     {"point_to_point": [0, 2], "point_to_plane": [1, 2]})
    out["no_normal_at_all"] = (dict(source=s, target=t, init=I4, target_normals=np.zeros((3, 3))), 10.0,
                               {"point_to_point": [0, 2], "point_to_plane": [-1, -1]})
    return out


TINY_P, TINY_NO_SOURCE, TINY_NO_TARGET = 65, 20, 41


@functools.lru_cache(maxsize=None)
def tiny_batch():
    """65 problems of about 7 source and 9 target points (one more than the 64-thread block of the per-problem kernels), every
    source point with a partner a few millimetres away; one problem without source points and one without targets, mid-batch"""
    rng = np.random.default_rng(5100)
    out = []
    for p in range(TINY_P):
        pr = _problem(rng, int(rng.integers(6, 9)), 2, zero_normals=0.0)
        T = np.eye(4)                                                       # the targets: the source moved 1 degree / 2 mm, then two more
        T[:3, :3] = rot(rng.normal(size=3), 1.0)
        T[:3, 3] = pr["source"].mean(0) - T[:3, :3] @ pr["source"].mean(0) + [1.0, -1.5, 1.0]
        moved = pr["source"] @ T[:3, :3].T + T[:3, 3]
        tn = rng.normal(size=moved.shape)
        pr["target"] = np.concatenate([moved, pr["target"]])
        pr["target_normals"] = np.concatenate([tn / np.linalg.norm(tn, axis=1, keepdims=True), pr["target_normals"]])
        pr["init"] = np.eye(4)
        if p == TINY_NO_SOURCE:
            pr["source"] = np.zeros((0, 3))
        if p == TINY_NO_TARGET:
            pr["target"], pr["target_normals"] = np.zeros((0, 3)), np.zeros((0, 3))
        out.append(pr)
    return tuple(out)


# ---- solvers -------------------------------------------------------------------------------------------------------------

STEP_MAX_D = 15.0


@functools.lru_cache(maxsize=None)
def step_problems():
    """four problems for one update: an ellipsoid with a bump (129-260 source points), its moved, thinned and noisy copy as the
    target with exact normals, a start 2-4 degrees and 4-8 mm off"""
    rng = np.random.default_rng(6000)
    out = []
    for k, n in enumerate((97, 150, 192, 200)):
        src, nrm = asymmetric_cloud(n, 60 + k)
        R, t = rot(rng.normal(size=3), rng.uniform(0, 180)), np.array([rng.uniform(-50, 50), rng.uniform(-40, 40), rng.uniform(600, 900)])
        keep = rng.uniform(size=len(src)) < 0.85
        tgt = (src @ R.T + t)[keep] + rng.normal(scale=0.2, size=(keep.sum(), 3))
        dt = rng.normal(size=3)
        dt *= rng.uniform(4, 8) / np.linalg.norm(dt)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = rot(rng.normal(size=3), rng.uniform(2, 4)) @ R, t + dt
        out.append(dict(source=src, target=tgt, init=T, target_normals=(nrm @ R.T)[keep]))
    return tuple(out)


def exact_problems():
    """name -> (problem, R, t): the target is the moved source, the points 30 mm or more apart and the motion small, so every
    point's nearest target is its partner from the start; 'coplanar' has a rank-2 cross-covariance"""
    rng = np.random.default_rng(6100)
    g = np.stack(np.meshgrid(np.arange(3) * 40.0, np.arange(3) * 35.0, np.arange(2) * 30.0, indexing="ij"), -1).reshape(-1, 3)
    g = g + rng.uniform(-4, 4, g.shape) + np.array([-40.0, -30.0, 650.0])
    flat = np.stack(np.meshgrid(np.arange(4) * 40.0, np.arange(3) * 35.0, indexing="ij"), -1).reshape(-1, 2)
    flat = np.concatenate([flat + rng.uniform(-4, 4, flat.shape), np.zeros((len(flat), 1))], 1) + np.array([-60.0, -35.0, 700.0])
    out = {}
    for name, s in (("general", g), ("coplanar", flat)):
        c = s.mean(0)
        R = rot(rng.normal(size=3), 2.0)
        t = c - R @ c + np.array([2.0, -1.5, 1.0])
        out[name] = (dict(source=s, target=s @ R.T + t, init=np.eye(4), target_normals=None), R, t)
    return out


def singular_plane_problem():
    """every target normal (0,0,1): J^T J has three zero rows -> singular"""
    rng = np.random.default_rng(6200)
    s = np.array([20.0, -10.0, 700.0]) + rng.uniform(-30, 30, (40, 3))
    T = np.eye(4)
    T[:3, 3] = [0.5, -0.25, 0.125]
    return dict(source=s, target=s + rng.normal(scale=0.1, size=s.shape), init=T, target_normals=np.tile([0.0, 0.0, 1.0], (40, 1)))


def threshold_problem(k, n_src=10):
    """n_src source points 100 mm apart; exactly k of them have a target (1 mm away, random unit normals), max_d 5"""
    rng = np.random.default_rng(6300)
    s = np.array([0.0, 0.0, 600.0]) + 100.0 * np.stack(np.unravel_index(rng.permutation(27)[:n_src], (3, 3, 3)), 1)
    d = rng.normal(size=(n_src, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n = rng.normal(size=(n_src, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    far = np.array([[5000.0, 0.0, 600.0]])                                # a target nothing reaches
    return dict(source=s, target=np.concatenate([far, (s + d)[:k]]), init=np.eye(4), target_normals=np.concatenate([[[0.0, 1.0, 0.0]], n[:k]]))
