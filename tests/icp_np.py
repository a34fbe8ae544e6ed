"""Numpy restatement of csrc/icp.hip (test infrastructure): back-projection, voxel down-sampling, normals and batched ICP with
the same expressions in the same order -- the per-tile wave trees of the ICP partial sums included -- so the device results
can be compared with tight tolerances.  Only sin / cos may differ from the device's by an ulp."""
import math

import numpy as np

ICP_TILE = 128
NRM_SWEEPS = 6
ICP_SWEEPS = 10
OK, TOO_FEW, SINGULAR = 0, 1, 2


def back_project(r, c, z, fx, fy, cx, cy):
    return np.stack([((c - cx) * z) / fx, ((r - cy) * z) / fy, z], -1)


def create_point_cloud(depth, fx, fy, cx, cy, ds):
    """dense [h*w,3] float64, all-NaN rows where z == 0 (pyrapose_node.py:170-189)"""
    d = np.asarray(depth, np.float32).astype(np.float64)
    h, w = d.shape
    r, c = np.mgrid[0:h, 0:w]
    z = d * ds
    out = back_project(r.astype(np.float64), c.astype(np.float64), z, fx, fy, cx, cy).reshape(-1, 3)
    out[z.reshape(-1) == 0] = np.nan
    return out


def cloud_from_depth(depth, fx, fy, cx, cy, ds=1.0, mask=None, row_idx=None, col_idx=None):
    """the valid (finite, non-zero z, mask cell set) pixels in row-major order"""
    d = np.asarray(depth, np.float32).astype(np.float64)
    h, w = d.shape
    r, c = np.mgrid[0:h, 0:w]
    z = d * ds
    valid = np.isfinite(z) & (z != 0)
    if mask is not None:
        valid &= np.asarray(mask)[np.asarray(row_idx)[:, None], np.asarray(col_idx)[None, :]] != 0
    return back_project(r[valid].astype(np.float64), c[valid].astype(np.float64), z[valid], fx, fy, cx, cy)


def voxel_down_sample(pts, voxel, normals=None):
    P = np.asarray(pts, np.float64)
    lo = P.min(0)
    idx = np.floor((P - (lo - voxel * 0.5)) / voxel).astype(np.int64)
    keys = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    perm = np.argsort(keys, kind="stable")
    sk = keys[perm]
    starts = np.concatenate([[0], np.nonzero(np.diff(sk))[0] + 1, [len(sk)]])
    cnt = np.diff(starts)
    m = len(cnt)
    sp = np.zeros((m, 3))
    sn = np.zeros((m, 3))
    for k in range(int(cnt.max())):  # the k-th member of every voxel: sequential sums in original point order
        live = cnt > k
        i = perm[starts[:-1][live] + k]
        sp[live] = sp[live] + P[i]
        if normals is not None:
            sn[live] = sn[live] + np.asarray(normals, np.float64)[i]
    out = sp / cnt[:, None].astype(np.float64)
    if normals is None:
        return out, None, sk[starts[:-1]]
    ln = np.sqrt((sn[:, 0] * sn[:, 0] + sn[:, 1] * sn[:, 1]) + sn[:, 2] * sn[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        on = np.where(ln[:, None] > 0, sn / ln[:, None], 0.0)
    return out, on, sk[starts[:-1]]


def _jacobi_rot(a, v, p, q):
    apq = a[p][q]
    if apq == 0.0:
        return
    theta = (a[q][q] - a[p][p]) / (2.0 * apq)
    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    a[p][p] = a[p][p] - t * apq
    a[q][q] = a[q][q] + t * apq
    a[p][q] = a[q][p] = 0.0
    n = len(a)
    for r in range(n):
        if r == p or r == q:
            continue
        arp, arq = a[r][p], a[r][q]
        a[r][p] = c * arp - s * arq
        a[p][r] = a[r][p]
        a[r][q] = s * arp + c * arq
        a[q][r] = a[r][q]
    for r in range(n):
        vp, vq = v[r][p], v[r][q]
        v[r][p] = c * vp - s * vq
        v[r][q] = s * vp + c * vq


def jacobi(a, sweeps):
    """cyclic Jacobi on a symmetric list-of-lists matrix (in place) -> eigenvector matrix (columns)"""
    n = len(a)
    v = [[1.0 if r == c else 0.0 for c in range(n)] for r in range(n)]
    pairs = [(p, q) for p in range(n) for q in range(p + 1, n)]
    with np.errstate(over="ignore"):  # theta overflows to inf for a negligible a[p][q], as on the device (t = 0 then)
        for _ in range(sweeps):
            for p, q in pairs:
                _jacobi_rot(a, v, p, q)
    return v


def neighbors(pts, radius, max_nn):
    P = np.asarray(pts, np.float64)
    out = []
    r2 = radius * radius
    for i in range(len(P)):
        d = P[i] - P
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        j = np.nonzero(d2 <= r2)[0]
        o = np.lexsort((j, d2[j]))
        out.append(j[o][:max_nn])
    return out


def estimate_normals(pts, radius, max_nn):
    P = np.asarray(pts, np.float64)
    nb = neighbors(P, radius, max_nn)
    N = np.zeros_like(P)
    for i, js in enumerate(nb):
        if len(js) < 3:
            continue
        m = [0.0, 0.0, 0.0]
        for j in js:
            for a in range(3):
                m[a] += P[j, a]
        inv = 1.0 / float(len(js))
        m = [x * inv for x in m]
        A = [[0.0] * 3 for _ in range(3)]
        for j in js:
            d = [P[j, 0] - m[0], P[j, 1] - m[1], P[j, 2] - m[2]]
            for r in range(3):
                for c in range(r, 3):
                    A[r][c] += d[r] * d[c]
        for r in range(3):
            for c in range(r, 3):
                A[r][c] *= inv
                A[c][r] = A[r][c]
        V = jacobi(A, NRM_SWEEPS)
        k = (2 if A[2][2] < A[1][1] else 1) if A[1][1] < A[0][0] else (2 if A[2][2] < A[0][0] else 0)
        n = [V[0][k], V[1][k], V[2][k]]
        ln = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        n = [x / ln for x in n]
        if (n[0] * P[i, 0] + n[1] * P[i, 1]) + n[2] * P[i, 2] > 0.0:
            n = [-x for x in n]
        N[i] = n
    return N, nb


def euler_update(x):
    ca, sa, cb, sb, cg, sg = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
    return np.array([[cg * cb, (cg * sb) * sa - sg * ca, (cg * sb) * ca + sg * sa],
                     [sg * cb, (sg * sb) * sa + cg * ca, (sg * sb) * ca - cg * sa],
                     [-sb, cb * sa, cb * ca]])


def _solve_plane(S):
    A = [[0.0] * 6 for _ in range(6)]
    k = 0
    for r in range(6):
        for c in range(r, 6):
            A[r][c] = A[c][r] = S[k]
            k += 1
    b = [-S[21 + r] for r in range(6)]
    dmax = 0.0
    for r in range(6):
        dmax = max(dmax, A[r][r])
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    ok = dmax > 0.0
    for j in range(6):
        s = A[j][j]
        for q in range(j):
            s -= (L[j][q] * L[j][q]) * d[q]
        d[j] = s
        ok = ok and s > 1e-12 * dmax
        for i in range(j + 1, 6):
            u = A[i][j]
            for q in range(j):
                u -= (L[i][q] * L[j][q]) * d[q]
            L[i][j] = u / s if s != 0.0 else 0.0
    if not ok:
        return None
    x = [0.0] * 6
    for i in range(6):
        s = b[i]
        for q in range(i):
            s -= L[i][q] * x[q]
        x[i] = s
    x = [x[i] / d[i] for i in range(6)]
    for i in range(5, -1, -1):
        s = x[i]
        for q in range(i + 1, 6):
            s -= L[q][i] * x[q]
        x[i] = s
    return euler_update(x), np.array(x[3:])


def _solve_point(S, n):
    ms = [S[0] / n, S[1] / n, S[2] / n]
    mq = [S[3] / n, S[4] / n, S[5] / n]
    C = [[S[6 + 3 * a + b] / n - ms[a] * mq[b] for b in range(3)] for a in range(3)]
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = C
    N = [[(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
         [Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz],
         [Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy],
         [Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy]]
    V = jacobi(N, ICP_SWEEPS)
    k, best = 0, N[0][0]
    for i in (1, 2, 3):
        if N[i][i] > best:
            k, best = i, N[i][i]
    qw, qx, qy, qz = V[0][k], V[1][k], V[2][k], V[3][k]
    ln = math.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
    if not ln > 0.0:
        return None
    qw, qx, qy, qz = qw / ln, qx / ln, qy / ln, qz / ln
    R = np.array([[((qw * qw + qx * qx) - qy * qy) - qz * qz, 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)],
                  [2.0 * (qx * qy + qw * qz), ((qw * qw - qx * qx) + qy * qy) - qz * qz, 2.0 * (qy * qz - qw * qx)],
                  [2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), ((qw * qw - qx * qx) - qy * qy) + qz * qz]])
    t = np.array([mq[a] - ((R[a, 0] * ms[0] + R[a, 1] * ms[1]) + R[a, 2] * ms[2]) for a in range(3)])
    return R, t


def _partials(src, tgt, tgt_n, R, T, max_d2, plane):
    """-> (S [29] summed like the device: wave trees per tile, the two waves, then the tiles), corr [ns]"""
    a, b, c = src[:, 0], src[:, 1], src[:, 2]
    x = ((R[0, 0] * a + R[0, 1] * b) + R[0, 2] * c) + T[0]
    y = ((R[1, 0] * a + R[1, 1] * b) + R[1, 2] * c) + T[1]
    z = ((R[2, 0] * a + R[2, 1] * b) + R[2, 2] * c) + T[2]
    tx, ty, tz = tgt[:, 0].copy(), tgt[:, 1].copy(), tgt[:, 2].copy()
    if plane:
        skip = (tgt_n[:, 0] == 0) & (tgt_n[:, 1] == 0) & (tgt_n[:, 2] == 0)
        tx[skip] = ty[skip] = tz[skip] = np.inf
    ns = len(src)
    corr = np.full(ns, -1, np.int64)
    v = np.zeros((ns, 29))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(ns):
            dx, dy, dz = x[i] - tx, y[i] - ty, z[i] - tz
            d2 = (dx * dx + dy * dy) + dz * dz
            j = int(np.argmin(d2))
            best = d2[j]
            if not (best < np.finfo(np.float64).max and best <= max_d2):
                continue
            corr[i] = j
            qx, qy, qz = tgt[j]
            X, Y, Z = x[i], y[i], z[i]
            if plane:
                nx, ny, nz = tgt_n[j]
                j0, j1, j2 = Y * nz - Z * ny, Z * nx - X * nz, X * ny - Y * nx
                r = ((X - qx) * nx + (Y - qy) * ny) + (Z - qz) * nz
                J = [j0, j1, j2, nx, ny, nz]
                k = 0
                for p in range(6):
                    for q in range(p, 6):
                        v[i, k] = J[p] * J[q]
                        k += 1
                for p in range(6):
                    v[i, 21 + p] = J[p] * r
            else:
                v[i, 0:6] = [X, Y, Z, qx, qy, qz]
                s, q = [X, Y, Z], [qx, qy, qz]
                for p in range(3):
                    for o in range(3):
                        v[i, 6 + 3 * p + o] = s[p] * q[o]
            v[i, 27] = 1.0
            v[i, 28] = best
    tiles = (ns + ICP_TILE - 1) // ICP_TILE
    pad = np.zeros((tiles * ICP_TILE, 29))
    pad[:ns] = v
    w = pad.reshape(tiles, ICP_TILE // 64, 64, 29).copy()
    off = 32
    while off > 0:
        w[:, :, :off] = w[:, :, :off] + w[:, :, off:2 * off]
        off //= 2
    tile_sum = w[:, 0, 0]
    for k in range(1, ICP_TILE // 64):
        tile_sum = tile_sum + w[:, k, 0]
    S = np.zeros(29)
    for tl in range(tiles):
        S = S + tile_sum[tl]
    return S, corr


def registration_icp(src, tgt, init, max_correspondence_distance, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
                     estimation="point_to_plane", tgt_normals=None):
    """-> dict(R, t, fitness, inlier_rmse, iterations, status, corr)"""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    plane = estimation == "point_to_plane"
    T = np.asarray(init, np.float64)
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    out = dict(fitness=0.0, inlier_rmse=0.0, iterations=0, status=OK, corr=np.full(len(src), -1, np.int64))
    if len(src) == 0 or len(tgt) == 0:
        out.update(R=R, t=t, status=TOO_FEW)
        return out
    max_d2 = max_correspondence_distance * max_correspondence_distance
    fit_prev = rmse_prev = 0.0
    for p in range(max_iteration + 1):
        S, corr = _partials(src, tgt, tgt_normals, R, t, max_d2, plane)
        out["corr"] = corr
        n = S[27]
        fitness = n / float(len(src))
        rmse = math.sqrt(S[28] / n) if n > 0 else 0.0
        converged = p > 0 and abs(fit_prev - fitness) < relative_fitness and abs(rmse_prev - rmse) < relative_rmse
        fit_prev, rmse_prev = fitness, rmse
        out.update(fitness=fitness, inlier_rmse=rmse)
        if converged or p >= max_iteration:
            break
        if n < (6.0 if plane else 3.0):
            out["status"] = TOO_FEW
            break
        upd = _solve_plane(S) if plane else _solve_point(S, n)
        if upd is None:
            out["status"] = SINGULAR
            break
        Ru, tu = upd
        R2 = np.empty((3, 3))
        t2 = np.empty(3)
        for r in range(3):
            for c in range(3):
                R2[r, c] = (Ru[r, 0] * R[0, c] + Ru[r, 1] * R[1, c]) + Ru[r, 2] * R[2, c]
            t2[r] = ((Ru[r, 0] * t[0] + Ru[r, 1] * t[1]) + Ru[r, 2] * t[2]) + tu[r]
        R, t = R2, t2
        out["iterations"] += 1
    out.update(R=R, t=t)
    return out
