"""float64 numpy restatement of BOP's symmetry-aware pose errors as csrc/pose.hip evaluates them (pp_pose_mssd_f64 /
pp_pose_mspd_f64), operation by operation, plus the scenes the tests and tools/bench_pose_sym.py share.

Every product-sum is written elementwise and evaluated left to right -- no `@` / dot on the point arrays, BLAS may fuse or
reorder -- so that the device, compiled without FMA contraction, performs the same IEEE operations in the same order; maxima
and minima are exact in any order.  With G_s = (R_gt S_R[s], R_gt S_t[s] + t_gt):
  MSSD = min_s max_i || (R_est p_i + t_est) - (G_s.R p_i + G_s.t) ||
  MSPD = min_s max_i || proj(K, R_est, t_est, p_i) - proj(K, G_s.R, G_s.t, p_i) ||      u = a / w, v = b / w
bop_blas_mssd / bop_blas_mspd state the same two formulas the way bop_toolkit writes them (matrix products): agreement to
rounding, not bit for bit."""
import numpy as np

K_LINEMOD = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def compose(R_gt, t_gt, S_R, S_t):
    """G_s of one ground-truth pose for every symmetry: ([n_sym,3,3], [n_sym,3])"""
    R, t = np.asarray(R_gt, np.float64).reshape(3, 3), np.asarray(t_gt, np.float64).reshape(3)
    S_R, S_t = np.asarray(S_R, np.float64).reshape(-1, 3, 3), np.asarray(S_t, np.float64).reshape(-1, 3)
    G_R = np.empty_like(S_R)
    G_t = np.empty_like(S_t)
    for r in range(3):
        for c in range(3):
            G_R[:, r, c] = R[r, 0] * S_R[:, 0, c] + R[r, 1] * S_R[:, 1, c] + R[r, 2] * S_R[:, 2, c]
        G_t[:, r] = (R[r, 0] * S_t[:, 0] + R[r, 1] * S_t[:, 1] + R[r, 2] * S_t[:, 2]) + t[r]
    return G_R, G_t


def rigid(R, t, pts):
    """R p + t as the kernels' rigid(): R [...,3,3], t [...,3], pts [n,3] -> three arrays [..., n]"""
    R, t = np.asarray(R, np.float64)[..., None], np.asarray(t, np.float64)[..., None]
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return tuple(R[..., r, 0, :] * x + R[..., r, 1, :] * y + R[..., r, 2, :] * z + t[..., r, :] for r in range(3))


def pixel(K, X, Y, Z):
    a = K[0, 0] * X + K[0, 1] * Y + K[0, 2] * Z
    b = K[1, 0] * X + K[1, 1] * Y + K[1, 2] * Z
    w = K[2, 0] * X + K[2, 1] * Y + K[2, 2] * Z
    return a / w, b / w


def per_symmetry(pts, S_R, S_t, R_est, t_est, R_gt, t_gt, K=None):
    """max over the points of the distance, per symmetry, of ONE pose pair: [n_sym] (surface distance, or pixels with K)"""
    pts = np.asarray(pts, np.float64)
    G_R, G_t = compose(R_gt, t_gt, S_R, S_t)
    ax, ay, az = rigid(np.asarray(R_est, np.float64).reshape(3, 3), np.asarray(t_est, np.float64).reshape(3), pts)
    bx, by, bz = rigid(G_R, G_t, pts)
    if K is None:
        dx, dy, dz = ax - bx, ay - by, az - bz
        sq = dx * dx + dy * dy + dz * dz
    else:
        K = np.asarray(K, np.float64).reshape(3, 3)
        au, av = pixel(K, ax, ay, az)
        bu, bv = pixel(K, bx, by, bz)
        du, dv = au - bu, av - bv
        sq = du * du + dv * dv
    return np.sqrt(np.max(sq, axis=1))


def mssd_np(pts, S_R, S_t, R_est, t_est, R_gt, t_gt, K=None):
    """n pose pairs -> (err float64 [n], best_sym int32 [n]); with K [3,3] or [n,3,3]: mspd_np"""
    n = len(R_est)
    K = None if K is None else np.broadcast_to(np.asarray(K, np.float64), (n, 3, 3))
    e = [per_symmetry(pts, S_R, S_t, R_est[i], t_est[i], R_gt[i], t_gt[i], None if K is None else K[i]) for i in range(n)]
    return np.array([np.min(v) for v in e], np.float64), np.array([np.argmin(v) for v in e], np.int32)


def mspd_np(pts, S_R, S_t, K, R_est, t_est, R_gt, t_gt):
    return mssd_np(pts, S_R, S_t, R_est, t_est, R_gt, t_gt, K)


def bop_blas_mssd(R_est, t_est, R_gt, t_gt, pts, syms):
    """pose_error.mssd as bop_toolkit writes it: syms a list of {'R', 't'}"""
    tr = lambda R, t: (np.asarray(R).dot(pts.T) + np.asarray(t).reshape(3, 1)).T
    pts_est = tr(R_est, t_est)
    es = []
    for sym in syms:
        R_gt_sym = np.asarray(R_gt).dot(sym["R"])
        t_gt_sym = np.asarray(R_gt).dot(sym["t"].reshape(3, 1)) + np.asarray(t_gt).reshape(3, 1)
        es.append(np.linalg.norm(pts_est - tr(R_gt_sym, t_gt_sym), axis=1).max())
    return min(es)


def bop_blas_mspd(R_est, t_est, R_gt, t_gt, K, pts, syms):
    """pose_error.mspd as bop_toolkit writes it (misc.project_pts: K (R p + t), divided by its third row)"""
    def proj(R, t):
        im = np.asarray(K).dot(np.asarray(R).dot(pts.T) + np.asarray(t).reshape(3, 1))
        return (im[:2] / im[2]).T
    proj_est = proj(R_est, t_est)
    es = []
    for sym in syms:
        R_gt_sym = np.asarray(R_gt).dot(sym["R"])
        t_gt_sym = np.asarray(R_gt).dot(sym["t"].reshape(3, 1)) + np.asarray(t_gt).reshape(3, 1)
        es.append(np.linalg.norm(proj_est - proj(R_gt_sym, t_gt_sym), axis=1).max())
    return min(es)


def axis_angle(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def random_symmetries(rng, n_sym, shift=20.0):
    """a random rigid set, the identity first: (S_R [n_sym,3,3], S_t [n_sym,3])"""
    S_R = np.stack([np.eye(3)] + [random_rotation(rng) for _ in range(n_sym - 1)])
    S_t = np.concatenate([np.zeros((1, 3)), rng.uniform(-shift, shift, size=(n_sym - 1, 3))])
    return np.ascontiguousarray(S_R), np.ascontiguousarray(S_t)


def scene(rng, n_pose, n_pts, extent=(60.0, 45.0, 80.0)):
    """model points in a box of +-extent mm, ground-truth poses 400-1200 mm in front of a LineMOD-like camera, estimates a few
    degrees and millimetres off: (pts, R_est, t_est, R_gt, t_gt)"""
    pts = rng.uniform(-1.0, 1.0, size=(n_pts, 3)) * np.asarray(extent)
    R_gt = np.stack([random_rotation(rng) for _ in range(n_pose)])
    t_gt = np.stack([rng.uniform(-150, 150, n_pose), rng.uniform(-100, 100, n_pose), rng.uniform(400, 1200, n_pose)], axis=1)
    R_est = np.stack([axis_angle(rng.normal(scale=0.08, size=3)) @ R for R in R_gt])
    t_est = t_gt + rng.normal(scale=6.0, size=(n_pose, 3))
    return pts, R_est, t_est, R_gt, t_gt
