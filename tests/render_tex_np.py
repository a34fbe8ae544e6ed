"""Numpy restatement of the textured colour pass of csrc/render.hip (pp_render_rgbd_tex); test infrastructure.  The sampling
rule of include/pyrapose_hip.h, the same expressions in the same order in float64, on top of tests/render_rgb_np.py's
weights and lighting, so that colour can be compared with the device bit for bit:
  sample         the texture at (u, v): nearest or bilinear, clamp to edge or repeat, three channels in [0, 1]
  shade_rgb_tex  float32 and uint8 colour of a triangle-id image of a UV-mapped mesh (flat or phong)
  interp_uv      the perspective-correct (u, v) at the pixels of a triangle-id image"""
import numpy as np

from tests import render_rgb_np as RR
from tests.render_np import project

INDEX_MAX = 2.0 ** 30
FILTERS, WRAPS = ("nearest", "bilinear"), ("clamp", "repeat")


def _wrap(i, n, wrap):
    """texel indices i (int64, any value) -> [0, n)"""
    if wrap == "repeat":
        return i - n * np.floor_divide(i, n)
    return np.minimum(np.maximum(i, 0), n - 1)


def _to_int(f):
    return np.clip(f, -INDEX_MAX, INDEX_MAX).astype(np.int64)


def _channels(tex, i, j):
    """GL texel (i, j), both in range -> float64 [m, 3]: row tex_h - 1 - j of the image as stored (top row first)"""
    return tex[tex.shape[0] - 1 - j, i, :3].astype(np.float64) / 255.0


def sample(tex, u, v, filter="nearest", wrap="clamp"):
    """tex uint8 [tex_h,tex_w,3 or 4] in file order, u and v float64 [m] -> float64 [m, 3]"""
    assert filter in FILTERS and wrap in WRAPS
    tex = np.asarray(tex, np.uint8)
    th, tw = tex.shape[:2]
    u, v = np.atleast_1d(np.asarray(u, np.float64)), np.atleast_1d(np.asarray(v, np.float64))
    with np.errstate(over="ignore", invalid="ignore"):
        x, y = u * tw, v * th
    bad = ~(np.isfinite(x) & np.isfinite(y))
    x, y = np.where(bad, 0.5, x), np.where(bad, 0.5, y)
    if filter == "nearest":
        return _channels(tex, _wrap(_to_int(np.floor(x)), tw, wrap), _wrap(_to_int(np.floor(y)), th, wrap))
    xs, ys = x - 0.5, y - 0.5
    fi, fj = np.floor(xs), np.floor(ys)
    fx, fy = (xs - fi)[:, None], (ys - fj)[:, None]
    i, j = _to_int(fi), _to_int(fj)
    i0, i1, j0, j1 = _wrap(i, tw, wrap), _wrap(i + 1, tw, wrap), _wrap(j, th, wrap), _wrap(j + 1, th, wrap)
    c00, c10, c01, c11 = _channels(tex, i0, j0), _channels(tex, i1, j0), _channels(tex, i0, j1), _channels(tex, i1, j1)
    return ((1.0 - fx) * c00 + fx * c10) * (1.0 - fy) + ((1.0 - fx) * c01 + fx * c11) * fy


def _per_triangle(pts, faces, K, R, t, tri_id, screen=None):
    """yields (vertex indices, rows, columns, [q0, q1, q2]) per triangle shown in tri_id: the weights of RR.shade_rgb"""
    x, y, iz = project(pts, np.asarray(K, np.float64), R, t) if screen is None else screen
    faces = np.asarray(faces, np.int64)
    for tri in np.unique(tri_id[tri_id >= 0]):
        V, s, edges, _ = RR._setup(x, y, iz, faces[tri])
        rr, cc = np.nonzero(tri_id == tri)
        w = RR._weights(s, edges, rr, cc)
        b = [w[k] * V[k][2] for k in range(3)]
        den = (b[0] + b[1]) + b[2]
        yield faces[tri], rr, cc, [b[k] / den for k in range(3)]


def interp_uv(pts, faces, uv, K, R, t, tri_id, screen=None):
    """-> float64 [h,w,2]: (u, v) = (q0 a0 + q1 a1) + q2 a2 where tri_id >= 0, NaN elsewhere"""
    tri_id, uv = np.asarray(tri_id), np.asarray(uv, np.float64)
    out = np.full(tri_id.shape + (2,), np.nan)
    for i, rr, cc, q in _per_triangle(pts, faces, K, R, t, tri_id, screen):
        for k in range(2):
            out[rr, cc, k] = (q[0] * uv[i[0], k] + q[1] * uv[i[1], k]) + q[2] * uv[i[2], k]
    return out


def _light_w(i, q, P, N, L, shading, ambient_weight):
    """min(ambient + max(l . n, 0), 1) at the pixels with weights q of the triangle with vertices i: RR.shade_rgb's lines"""
    l = RR._normalize(RR._interp(q, L[i]))
    if shading == "phong":
        n = RR._normalize(RR._interp(q, N[i]))
    else:
        a, b = P[i[1]] - P[i[0]], P[i[2]] - P[i[0]]
        n = RR._normalize(np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]))
        if (n[0] * P[i[0]][0] + n[1] * P[i[0]][1]) + n[2] * P[i[0]][2] > 0.0:
            n = -n
        n = np.broadcast_to(n, l.shape)
    dot = (l[:, 0] * n[:, 0] + l[:, 1] * n[:, 1]) + l[:, 2] * n[:, 2]
    total = ambient_weight + np.where(dot > 0.0, dot, 0.0)
    return np.where(total > 1.0, 1.0, total)


def shade_rgb_tex(pts, faces, uv, tex, normals, K, R, t, tri_id, filter="nearest", wrap="clamp", shading="phong", ambient_weight=0.5,
                  light=(0.0, 0.0, 0.0), bg_color=(0.0, 0.0, 0.0), screen=None, dtype=np.float32):
    """tri_id int32 [h,w] (-1 = background) -> (float32 [h,w,3], uint8 [h,w,3]): (float)(light_w * texture(u, v)); dtype=np.float64:
    the colour before it is rounded to float32, no uint8"""
    tri_id, uv = np.asarray(tri_id), np.asarray(uv, np.float64)
    P, N, L = RR.vertex_attributes(pts, normals if shading == "phong" else None, R, t, light)
    out = np.empty(tri_id.shape + (3,), dtype)
    out[:] = np.asarray(bg_color, np.float64).astype(np.float32)
    for i, rr, cc, q in _per_triangle(pts, faces, K, R, t, tri_id, screen):
        u = (q[0] * uv[i[0], 0] + q[1] * uv[i[1], 0]) + q[2] * uv[i[2], 0]
        v = (q[0] * uv[i[0], 1] + q[1] * uv[i[1], 1]) + q[2] * uv[i[2], 1]
        light_w = _light_w(i, q, P, N, L, shading, ambient_weight)
        out[rr, cc] = (light_w[:, None] * sample(tex, u, v, filter, wrap)).astype(dtype)
    return out, (RR.to_u8(out) if dtype == np.float32 else None)
