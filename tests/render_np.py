"""Numpy restatement of the depth renderer of csrc/render.hip (test infrastructure): the same expressions in the same order
in float64 from float32 screen positions, one triangle at a time, so coverage and depth can be compared with the device.
Pixel (r, c) samples (c + 0.5, r + 0.5); a pixel centre on an edge belongs to the triangle when the edge is a top or left
edge; triangles with a vertex at Z <= 0 are skipped; depths outside [clip_near, clip_far] are dropped; 0 = empty."""
import numpy as np


def project(pts, K, R, t):
    """-> screen x, y (float32) and 1/Z (float64, 0 for Z <= 0 or a non-finite projection)"""
    P = np.asarray(pts, np.float64)
    R = np.asarray(R, np.float64)
    t = np.asarray(t, np.float64).reshape(3)
    X = R[0, 0] * P[:, 0] + R[0, 1] * P[:, 1] + R[0, 2] * P[:, 2] + t[0]
    Y = R[1, 0] * P[:, 0] + R[1, 1] * P[:, 1] + R[1, 2] * P[:, 2] + t[1]
    Z = R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1] + R[2, 2] * P[:, 2] + t[2]
    ok = Z > 0
    Zs = np.where(ok, Z, 1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        x = (K[0, 0] * X / Zs + K[0, 2]).astype(np.float32)
        y = (K[1, 1] * Y / Zs + K[1, 2]).astype(np.float32)
    ok &= np.isfinite(x) & np.isfinite(y)
    iz = np.where(ok, 1.0 / Zs, 0.0)
    return np.where(ok, x, 0).astype(np.float32), np.where(ok, y, 0).astype(np.float32), iz


def edge_fn(ax, ay, bx, by, px, py):
    """edge function of a -> b at p, evaluated in the canonical direction of the edge"""
    ax, ay, bx, by = float(ax), float(ay), float(bx), float(by)
    sw = ax > bx or (ax == bx and ay > by)
    if sw:
        ax, ay, bx, by = bx, by, ax, ay
    e = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    return -e if sw else e


def top_left(ax, ay, bx, by, s):
    A = -s * (float(by) - float(ay))
    B = s * (float(bx) - float(ax))
    return A > 0.0 or (A == 0.0 and B > 0.0)


def render_depth(pts, faces, K, R, t, w, h, clip_near=100.0, clip_far=10000.0):
    """-> depth float32 [h, w], 0 = empty.  Coverage and depth are the device's at every pixel, pixels on or next to an edge
    included: both sides decide them with the same float64 expressions on the same float32 screen positions."""
    K = np.asarray(K, np.float64)
    x, y, iz = project(pts, K, R, t)
    zb = np.full((h, w), np.inf)
    for f in np.asarray(faces, np.int64):
        i0, i1, i2 = (int(v) for v in f)
        if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= len(x) or not (iz[i0] > 0 and iz[i1] > 0 and iz[i2] > 0):
            continue
        V = [(x[i0], y[i0], iz[i0]), (x[i1], y[i1], iz[i1]), (x[i2], y[i2], iz[i2])]
        area2 = edge_fn(V[1][0], V[1][1], V[2][0], V[2][1], float(V[0][0]), float(V[0][1]))
        if area2 == 0.0:
            continue
        s = 1.0 if area2 > 0 else -1.0
        edges = [(V[1], V[2]), (V[2], V[0]), (V[0], V[1])]
        tl = [top_left(a[0], a[1], b[0], b[1], s) for a, b in edges]
        xs = [float(v[0]) for v in V]
        ys = [float(v[1]) for v in V]
        c0 = max(int(np.ceil(min(max(min(xs) - 0.5, -1.0), float(w)))), 0)
        c1 = min(int(np.floor(min(max(max(xs) - 0.5, -1.0), float(w)))), w - 1)
        r0 = max(int(np.ceil(min(max(min(ys) - 0.5, -1.0), float(h)))), 0)
        r1 = min(int(np.floor(min(max(max(ys) - 0.5, -1.0), float(h)))), h - 1)
        if r0 > r1 or c0 > c1:
            continue
        rr, cc = np.mgrid[r0:r1 + 1, c0:c1 + 1]
        px, py = cc + 0.5, rr + 0.5
        ws = [s * edge_fn(a[0], a[1], b[0], b[1], px, py) for a, b in edges]
        inside = np.ones(px.shape, bool)
        for k in range(3):
            inside &= (ws[k] > 0.0) | ((ws[k] == 0.0) & tl[k])
        den = (ws[0] + ws[1]) + ws[2]
        num = (ws[0] * V[0][2] + ws[1] * V[1][2]) + ws[2] * V[2][2]
        with np.errstate(divide="ignore", invalid="ignore"):
            Z = den / num
        keep = inside & (Z >= clip_near) & (Z <= clip_far)
        z32 = Z.astype(np.float32).astype(np.float64)
        reg = zb[r0:r1 + 1, c0:c1 + 1]
        zb[r0:r1 + 1, c0:c1 + 1] = np.where(keep, np.minimum(reg, z32), reg)
    return np.where(np.isfinite(zb), zb, 0.0).astype(np.float32)


def box_mesh(sx, sy, sz):
    """axis-aligned box centred at the origin: 8 vertices, 12 triangles"""
    v = np.array([[x, y, z] for x in (-sx, sx) for y in (-sy, sy) for z in (-sz, sz)], np.float64) / 2
    f = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]]
    return {"pts": v, "faces": np.array(f, np.int64)}


def sphere_mesh(radius, n_lat, n_lon, scale=(1.0, 1.0, 1.0)):
    """UV sphere (optionally an ellipsoid): 2 + (n_lat - 1) n_lon vertices, 2 n_lon (n_lat - 1) triangles"""
    pts = [[0, 0, radius]]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            pts.append([radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)])
    pts.append([0, 0, -radius])
    pts = np.array(pts) * np.asarray(scale)
    faces = []
    for j in range(n_lon):
        faces.append([0, 1 + j, 1 + (j + 1) % n_lon])
    for i in range(n_lat - 2):
        for j in range(n_lon):
            a = 1 + i * n_lon + j
            b = 1 + i * n_lon + (j + 1) % n_lon
            faces.append([a, a + n_lon, b])
            faces.append([b, a + n_lon, b + n_lon])
    last = len(pts) - 1
    base = 1 + (n_lat - 2) * n_lon
    for j in range(n_lon):
        faces.append([base + j, last, base + (j + 1) % n_lon])
    return {"pts": pts, "faces": np.array(faces, np.int64)}
