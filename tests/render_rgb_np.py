"""Numpy restatement of the colour renderer of csrc/render.hip (pp_render_rgbd) and of the scene image (pp_scene_compose_u8);
test infrastructure.  The same expressions in the same order in float64 from float32 screen positions, on top of
tests/render_np.py's project / edge_fn, so that colour can be compared with the device bit for bit:
  fragments   per triangle the pixels it covers with their float32 depth (the depth pass's rule, tests/render_np.py)
  render_ids  depth and triangle id: the nearest fragment, among equal float32 depths the smallest triangle index
  shade_rgb   float32 and uint8 colour of a triangle-id image (flat or phong, the rule in csrc/render.hip's header comment)
  compose     a scene's image from an id image and its instances' colour images"""
import numpy as np

from tests.render_np import edge_fn, project, top_left


def _setup(x, y, iz, f):
    """the triangle's vertices ((x, y, iz) with x, y float32), orientation sign and top-left flags, or None when it draws nothing"""
    i0, i1, i2 = (int(v) for v in f)
    if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= len(x) or not (iz[i0] > 0 and iz[i1] > 0 and iz[i2] > 0):
        return None
    V = [(x[i0], y[i0], iz[i0]), (x[i1], y[i1], iz[i1]), (x[i2], y[i2], iz[i2])]
    area2 = edge_fn(V[1][0], V[1][1], V[2][0], V[2][1], float(V[0][0]), float(V[0][1]))
    if area2 == 0.0:
        return None
    s = 1.0 if area2 > 0 else -1.0
    edges = [(V[1], V[2]), (V[2], V[0]), (V[0], V[1])]
    tl = [top_left(a[0], a[1], b[0], b[1], s) for a, b in edges]
    return V, s, edges, tl


def _weights(s, edges, rr, cc):
    """w0, w1, w2 at the pixel centres of rows rr and columns cc, as shade() of csrc/render.hip computes them"""
    px, py = cc + 0.5, rr + 0.5
    return [s * edge_fn(a[0], a[1], b[0], b[1], px, py) for a, b in edges]


def fragments(pts, faces, K, R, t, w, h, clip_near=100.0, clip_far=10000.0):
    """yields (triangle index, rows slice, columns slice, keep bool [rows, cols], float32 depth [rows, cols]) per drawn triangle"""
    K = np.asarray(K, np.float64)
    x, y, iz = project(pts, K, R, t)
    for tri, f in enumerate(np.asarray(faces, np.int64)):
        T = _setup(x, y, iz, f)
        if T is None:
            continue
        V, s, edges, tl = T
        xs, ys = [float(v[0]) for v in V], [float(v[1]) for v in V]
        c0 = max(int(np.ceil(min(max(min(xs) - 0.5, -1.0), float(w)))), 0)
        c1 = min(int(np.floor(min(max(max(xs) - 0.5, -1.0), float(w)))), w - 1)
        r0 = max(int(np.ceil(min(max(min(ys) - 0.5, -1.0), float(h)))), 0)
        r1 = min(int(np.floor(min(max(max(ys) - 0.5, -1.0), float(h)))), h - 1)
        if r0 > r1 or c0 > c1:
            continue
        rr, cc = np.mgrid[r0:r1 + 1, c0:c1 + 1]
        ws = _weights(s, edges, rr, cc)
        inside = np.ones(rr.shape, bool)
        for k in range(3):
            inside &= (ws[k] > 0.0) | ((ws[k] == 0.0) & tl[k])
        den = (ws[0] + ws[1]) + ws[2]
        num = (ws[0] * V[0][2] + ws[1] * V[1][2]) + ws[2] * V[2][2]
        with np.errstate(divide="ignore", invalid="ignore"):
            Z = den / num
            keep = inside & (Z >= clip_near) & (Z <= clip_far)
            z32 = Z.astype(np.float32)
        yield tri, slice(r0, r1 + 1), slice(c0, c1 + 1), keep & np.isfinite(z32) & (z32 > 0), z32


def render_ids(pts, faces, K, R, t, w, h, clip_near=100.0, clip_far=10000.0):
    """-> (depth float32 [h,w], 0 = empty; triangle id int32 [h,w], -1 = none): per pixel the minimum of the key
    (float32 depth, triangle index)"""
    zb = np.full((h, w), np.inf, np.float32)
    ids = np.full((h, w), -1, np.int32)
    for tri, rs, cs, keep, z32 in fragments(pts, faces, K, R, t, w, h, clip_near, clip_far):
        take = keep & (z32 < zb[rs, cs])  # triangles come in index order: a later one of equal depth does not replace
        zb[rs, cs] = np.where(take, z32, zb[rs, cs])
        ids[rs, cs] = np.where(take, tri, ids[rs, cs])
    return np.where(ids >= 0, zb, np.float32(0.0)).astype(np.float32), ids


def smallest_id_at_depth(pts, faces, K, R, t, w, h, depth, clip_near=100.0, clip_far=10000.0):
    """per pixel the smallest index among the triangles whose float32 fragment depth there equals depth [h,w]; -1 = none"""
    ids = np.full((h, w), -1, np.int32)
    depth = np.asarray(depth, np.float32)
    for tri, rs, cs, keep, z32 in fragments(pts, faces, K, R, t, w, h, clip_near, clip_far):
        take = keep & (z32 == depth[rs, cs]) & (ids[rs, cs] < 0)
        ids[rs, cs] = np.where(take, tri, ids[rs, cs])
    return ids


def _normalize(v):
    """rows of v [..., 3] divided by their length, 0 where the length is 0"""
    length = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    ok = length > 0.0
    safe = np.where(ok, length, 1.0)
    return np.where(ok[..., None], v / safe[..., None], 0.0)


def vertex_attributes(pts, normals, R, t, light):
    """per vertex: eye position P = R p + t, N = normalize(R n) (zeros without normals), L = normalize(light - P)"""
    p = np.asarray(pts, np.float64)
    R = np.asarray(R, np.float64)
    t = np.asarray(t, np.float64).reshape(3)
    rot = lambda v: np.stack([R[k, 0] * v[:, 0] + R[k, 1] * v[:, 1] + R[k, 2] * v[:, 2] for k in range(3)], axis=1)
    P = rot(p) + t[None, :]
    N = _normalize(rot(np.asarray(normals, np.float64))) if normals is not None else np.zeros_like(P)
    L = _normalize(np.asarray(light, np.float64).reshape(1, 3) - P)
    return P, N, L


def _interp(q, a):
    """(q0 a0 + q1 a1) + q2 a2 for q three [m] arrays and a three [3] vertex attributes -> [m, 3]"""
    return (q[0][:, None] * a[0][None, :] + q[1][:, None] * a[1][None, :]) + q[2][:, None] * a[2][None, :]


def shade_rgb(pts, faces, colors, normals, K, R, t, tri_id, shading="phong", ambient_weight=0.5, light=(0.0, 0.0, 0.0),
              bg_color=(0.0, 0.0, 0.0), screen=None, dtype=np.float32):
    """tri_id int32 [h,w] (-1 = background) -> (float32 [h,w,3], uint8 [h,w,3]).  screen: (x, y, iz) in place of project()'s;
    dtype=np.float64: the colour before it is rounded to float32 (for the closed-form tests), no uint8."""
    K = np.asarray(K, np.float64)
    faces = np.asarray(faces, np.int64)
    colors = np.asarray(colors, np.float64)
    x, y, iz = project(pts, K, R, t) if screen is None else screen
    P, N, L = vertex_attributes(pts, normals if shading == "phong" else None, R, t, light)
    tri_id = np.asarray(tri_id)
    out = np.empty(tri_id.shape + (3,), dtype)
    out[:] = np.asarray(bg_color, np.float64).astype(np.float32)
    for tri in np.unique(tri_id[tri_id >= 0]):
        V, s, edges, _ = _setup(x, y, iz, faces[tri])
        i = faces[tri]
        rr, cc = np.nonzero(tri_id == tri)
        w = _weights(s, edges, rr, cc)
        b = [w[k] * V[k][2] for k in range(3)]
        den = (b[0] + b[1]) + b[2]
        q = [b[k] / den for k in range(3)]
        c = _interp(q, colors[i])
        l = _normalize(_interp(q, L[i]))
        if shading == "phong":
            n = _normalize(_interp(q, N[i]))
        else:
            u, v = P[i[1]] - P[i[0]], P[i[2]] - P[i[0]]
            n = _normalize(np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]))
            if (n[0] * P[i[0]][0] + n[1] * P[i[0]][1]) + n[2] * P[i[0]][2] > 0.0:
                n = -n
            n = np.broadcast_to(n, l.shape)
        dot = (l[:, 0] * n[:, 0] + l[:, 1] * n[:, 1]) + l[:, 2] * n[:, 2]
        d = np.where(dot > 0.0, dot, 0.0)
        total = ambient_weight + d
        light_w = np.where(total > 1.0, 1.0, total)
        out[rr, cc] = (light_w[:, None] * c).astype(dtype)
    return out, (to_u8(out) if dtype == np.float32 else None)


def to_u8(rgb_f32):
    """np.round(rgb * 255).astype(np.uint8) of hodan_renderer.py:516, in float32 (round half to even, as rintf)"""
    return np.round(np.asarray(rgb_f32, np.float32) * np.float32(255)).astype(np.uint8)


def compose(id_image, colors, scene_offsets, background=(0, 0, 0), channel_order="bgr"):
    """id_image uint8 [S,h,w], colors uint8 [n,h,w,3] (RGB), background uint8 [S,h,w,3] or three values (RGB) ->
    uint8 [S,h,w,3]: id k > 0 selects instance scene_offsets[s] + k - 1, anything else the background"""
    id_image, colors = np.asarray(id_image, np.uint8), np.asarray(colors, np.uint8)
    S, h, w = id_image.shape
    background = np.asarray(background, np.uint8)
    out = np.empty((S, h, w, 3), np.uint8)
    for s in range(S):
        out[s] = background[s] if background.ndim == 4 else background.reshape(1, 1, 3)
        for k in range(1, scene_offsets[s + 1] - scene_offsets[s] + 1):
            out[s] = np.where((id_image[s] == k)[..., None], colors[scene_offsets[s] + k - 1], out[s])
    return out[..., ::-1].copy() if channel_order == "bgr" else out


def quad(corners):
    """two triangles over four camera-frame corners given in order round the quad"""
    return {"pts": np.asarray(corners, np.float64), "faces": np.array([[0, 1, 2], [0, 2, 3]])}


def unproject(u, v, Z, K):
    return [(u - K[0, 2]) * Z / K[0, 0], (v - K[1, 2]) * Z / K[1, 1], Z]
