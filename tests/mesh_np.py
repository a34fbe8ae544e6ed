"""numpy restatement of csrc/mesh.hip (pp_mesh_face_geometry_f64, pp_mesh_vertex_normals_f64, pp_mesh_sample_surface_f64), the
loops made explicit; the kernels are bit-identical to it (tests/test_gpu_mesh.py).  The rules are this project's own: nothing in
the reference computes them and no mesh library was at hand to pin them against (tests/test_mesh_cpu.py holds closed forms).
Every numpy operation below is one rounding, in the association the header states."""
import math

import numpy as np

THREADS = 256        # MESH_THREADS: faces per chunk of the float sums
SCAN_CHUNK = 1024    # MESH_SCAN_CHUNK (the integer scan's shape does not show in its result; kept for the tests' shapes)
Q_BITS = 39
MAX_ELEMS = 1 << 22
MAX_SAMPLES = 1 << 24
MAX_ATTR = 8
WEYL = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
MODES = {"random": 0, "weyl": 1}


def splitmix64(x):
    """the published mixer on Python integers (csrc/splitmix.h)"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def tree_sum(v):
    """the sum of v in the kernels' order: chunks of THREADS in order, each by the halving tree, a tail padded with +0.0"""
    v = np.asarray(v, np.float64)
    chunks = (len(v) + THREADS - 1) // THREADS
    red = np.zeros((chunks, THREADS))
    red.reshape(-1)[:len(v)] = v
    s = THREADS // 2
    while s > 0:
        red[:, :s] = red[:, :s] + red[:, s:2 * s]
        s >>= 1
    total = np.float64(0.0)
    for c in range(chunks):
        total = total + red[c, 0]
    return total


def faces_ok(faces, n_v):
    faces = np.asarray(faces, np.int64)
    return ((faces >= 0) & (faces < n_v)).all(axis=1)


def face_geometry(pts, faces):
    """-> dict(normal [n_f,3], area2 [n_f], totals [8], status int)"""
    pts = np.asarray(pts, np.float64)
    faces = np.asarray(faces, np.int64)
    ok = faces_ok(faces, len(pts))
    P = np.zeros((len(faces), 3, 3))
    P[ok] = pts[faces[ok]]
    p0, p1, p2 = P[:, 0], P[:, 1], P[:, 2]
    u, v = p1 - p0, p2 - p0
    n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    area2 = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    vol = (p0[:, 0] * n[:, 0] + p0[:, 1] * n[:, 1]) + p0[:, 2] * n[:, 2]
    cen = area2[:, None] * ((p0 + p1) + p2)
    totals = np.zeros(8)
    totals[0] = tree_sum(area2)
    totals[1] = tree_sum(vol)
    for a in range(3):
        totals[2 + a] = tree_sum(cen[:, a])
    totals[5] = area2.max()
    status = (0 if ok.all() else 1) | (0 if totals[5] > 0.0 else 2)
    return dict(normal=n, area2=area2, totals=totals, status=status)


def adjacency(faces, n_v):
    """-> (adj_offsets int32 [n_v+1], adj_faces int32 [3 n_f]): per vertex its faces ascending, a face once per listing; the
    faces with an index out of range are listed nowhere and the tail is -1"""
    faces = np.asarray(faces, np.int64)
    ok = faces_ok(faces, n_v)
    lists = [[] for _ in range(n_v)]
    for f in range(len(faces)):
        if ok[f]:
            for k in range(3):
                lists[faces[f, k]].append(f)
    offsets = np.zeros(n_v + 1, np.int32)
    adj = np.full(3 * len(faces), -1, np.int32)
    at = 0
    for v in range(n_v):
        offsets[v] = at
        for f in lists[v]:
            adj[at] = f
            at += 1
    offsets[n_v] = at
    return offsets, adj


def vertex_normals(faces, n_v, normal, totals, outward=True):
    """-> (vnormal [n_v,3], adj_offsets, adj_faces)"""
    offsets, adj = adjacency(faces, n_v)
    flip = bool(outward) and totals[1] < 0.0
    out = np.zeros((n_v, 3))
    for v in range(n_v):
        s = np.zeros(3)
        for j in range(offsets[v], offsets[v + 1]):
            s = s + normal[adj[j]]
        l = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        if l > 0.0:
            out[v] = -(s / l) if flip else s / l
    return out, offsets, adj


def quantise(faces, n_v, area2, largest):
    """q [n_f] uint64"""
    q = np.zeros(len(area2), np.uint64)
    if not largest > 0.0:
        return q
    shift = Q_BITS - (math.frexp(float(largest))[1] - 1)  # ilogb
    ok = faces_ok(faces, n_v) & (area2 > 0.0) & (area2 <= largest)
    q[ok] = np.floor(np.ldexp(area2[ok], shift)).astype(np.uint64)
    return q


def sample_surface(pts, faces, geom, n, seed=0, mode="random", outward=True, attr=None):
    """-> dict(points [n,3], face int32 [n], bary [n,3], normals [n,3], attr_out [n,n_attr] or None)"""
    pts = np.asarray(pts, np.float64)
    faces = np.asarray(faces, np.int64)
    normal, area2, totals = geom["normal"], geom["area2"], geom["totals"]
    cum = np.cumsum(quantise(faces, len(pts), area2, totals[5]), dtype=np.uint64)
    total = int(cum[-1])
    n_attr = 0 if attr is None else np.asarray(attr).shape[1]
    out = dict(points=np.zeros((n, 3)), face=np.full(n, -1, np.int32), bary=np.zeros((n, 3)), normals=np.zeros((n, 3)),
               attr_out=None if attr is None else np.zeros((n, n_attr)))
    if total == 0:
        return out
    seed = int(seed) & M64
    s = [splitmix64((4 * seed + j) & M64) for j in range(4)]
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        u = _mix(np.uint64(s[0]) + i) if MODES[mode] == 0 else np.uint64(s[3]) + i * np.uint64(WEYL)
        w1, w2 = _mix(np.uint64(s[1]) + i), _mix(np.uint64(s[2]) + i)
    t = np.array([(int(x) * total) >> 64 for x in u], np.uint64)   # Python integers for the high multiply
    f = np.searchsorted(cum, t, side="right")                       # the first f with cum[f] > t
    r1 = (w1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    r2 = (w2 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    sq = np.sqrt(r1)
    a, b, c = 1.0 - sq, sq * (1.0 - r2), sq * r2
    tri = faces[f]
    blend = lambda tab: (a[:, None] * tab[tri[:, 0]] + b[:, None] * tab[tri[:, 1]]) + c[:, None] * tab[tri[:, 2]]
    out["face"] = f.astype(np.int32)
    out["bary"] = np.stack([a, b, c], axis=1)
    out["points"] = blend(pts)
    nrm = normal[f] / area2[f][:, None]
    out["normals"] = -nrm if (outward and totals[1] < 0.0) else nrm
    if attr is not None:
        out["attr_out"] = blend(np.asarray(attr, np.float64))
    return out


def _mix(x):
    """splitmix64 on a uint64 array (wrapping arithmetic)"""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        z = x
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


# ---- meshes the tests share -------------------------------------------------------------------------------------------------

def cube(side=1.0, origin=(0.0, 0.0, 0.0), inward=False):
    """12 triangles, outward winding (inward: every face reversed)"""
    p = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64) * side + np.asarray(origin, np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = []
    for a, b, c, d in quads:
        f += [(a, b, c), (a, c, d)]
    f = np.array(f, np.int32)
    return p, (f[:, ::-1].copy() if inward else f)


def octahedron():
    p = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return p, f


def tetrahedron():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    return p, f


def fan(valence, offset=(0.0, 0.0, 0.0), lift=0.25):
    """a hub (vertex 0) with `valence` triangles around it, the rim rising with the angle so that no two normals agree"""
    k = valence
    ang = 2.0 * np.pi * np.arange(k + 1) / (k + 1)
    rim = np.stack([np.cos(ang), np.sin(ang), lift * np.arange(k + 1) / (k + 1)], axis=1)
    p = np.concatenate([np.zeros((1, 3)), rim]) + np.asarray(offset, np.float64)
    f = np.array([[0, 1 + j, 2 + j] for j in range(k)], np.int32)
    return p, f


def strip(n_f, rng, offset=(1000.0, 1000.0, 1000.0)):
    """n_f triangles of a jittered strip, every face of another size, points far from the origin"""
    n_v = n_f + 2
    p = np.stack([np.arange(n_v) * 0.5, (np.arange(n_v) % 2) * 1.0, np.zeros(n_v)], axis=1) + rng.uniform(-0.2, 0.2, (n_v, 3))
    f = np.stack([np.arange(n_f), np.arange(n_f) + 1, np.arange(n_f) + 2], axis=1).astype(np.int32)
    f[1::2] = f[1::2, ::-1]
    return p + np.asarray(offset, np.float64), f


def soup(n_f, rng, offset=(1000.0, 1000.0, 1000.0), scale=None):
    """n_f separate random triangles (3 n_f vertices) near `offset`, triangle k scaled about its first corner by scale[k]"""
    tri = rng.uniform(-1.0, 1.0, (n_f, 3, 3))
    if scale is not None:
        tri[:, 1:] = tri[:, :1] + (tri[:, 1:] - tri[:, :1]) * np.asarray(scale, np.float64)[:, None, None]
    return tri.reshape(-1, 3) + np.asarray(offset, np.float64), np.arange(3 * n_f, dtype=np.int32).reshape(n_f, 3)


def join(meshes):
    """several (pts, faces) as one mesh"""
    pts, faces, at = [], [], 0
    for p, f in meshes:
        pts.append(p)
        faces.append(np.asarray(f, np.int32) + at)
        at += len(p)
    return np.concatenate(pts), np.concatenate(faces).astype(np.int32)


def ratio_mesh():
    """four separate right triangles in the plane z = 0.5 whose areas are in the ratios 1 : 2 : 5 : 50"""
    p, f = [], []
    for k, area in enumerate((1.0, 2.0, 5.0, 50.0)):
        x0 = 20.0 * k
        p += [[x0, 0.0, 0.5], [x0 + 2.0 * area, 0.0, 0.5], [x0, 1.0, 0.5]]
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    return np.array(p, np.float64), np.array(f, np.int32)


def sphere(n_lat, n_lon, radius=1.0):
    """a closed latitude-longitude sphere, outward winding: 2 n_lon (n_lat - 1) triangles"""
    p = [[0.0, 0.0, radius]]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2.0 * np.pi * j / n_lon
            p.append([radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)])
    p.append([0.0, 0.0, -radius])
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    f = [[0, ring(1, j), ring(1, j + 1)] for j in range(n_lon)]
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f += [[ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)], [ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)]]
    last = len(p) - 1
    f += [[last, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)] for j in range(n_lon)]
    return np.array(p, np.float64), np.array(f, np.int32)
