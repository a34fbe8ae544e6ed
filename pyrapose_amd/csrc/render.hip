// Depth and colour renderer of the evaluation tail: the images the VSD pose error (vsd.hip; tless_eval.py:470-471, 651-662 and the
// same calls in occlusion_eval.py / ycbv_eval.py / homebrewed_eval.py / linemod_eval.py) and scene ground truth (scene_gt.hip) read.
//
// Renderer: the depth pass of utils/hodan_renderer.py (mode='depth'), which the reference's vsd() (utils/pose_error.py:105-176)
// calls twice per detection.  Per pixel the value is the eye depth Z (camera-frame z of the nearest surface point,
// hodan_renderer.py:121-143), interpolated perspective-correctly (Z = 1 / sum_i b_i / Z_i, b_i screen-space barycentrics),
// 0 where nothing is drawn.  With the projection of _calc_calib_proj(..., 'y_down') (:185-225) window x = fx X/Z + cx and
// window y = h - (fy Y/Z + cy); GL samples pixel centres at window (j + 0.5) and _draw_depth flips the rows (:548-553), so
// image pixel (row r, column c) samples (u, v) = (c + 0.5, r + 0.5) in OpenCV pixel coordinates.  Fragments with Z outside
// [clip_near, clip_far] are dropped.  Skew is ignored (the reference's K has none).
// Deviations: a triangle with a vertex at Z <= 0 (or projecting to a non-finite point) is skipped, not clipped; a pixel centre
// exactly on an edge belongs to the triangle only if the edge is a top or left edge (edge functions are evaluated in one
// canonical direction per edge, so a shared edge gives exactly opposite values and is drawn exactly once).
//
// Passes, one set of launches for n poses of one mesh:
//   1. vertex:  R p + t in float64 per (pose, vertex) -> float32 screen x / y and float64 1/Z
//   2. count:   per (pose, triangle) the 32x32-pixel screen tiles its pixel bounding box touches; a triangle on at most 4 tiles
//               adds one entry per tile to that (pose, tile)'s list, a larger one goes to the pose's list of big triangles
//   3. scan:    exclusive prefix sum of the per-(pose, tile) counts
//   4. scatter: fill the lists (arrival order -- the result does not depend on it, see below)
//   5. raster:  one workgroup per (pose, tile): the tile's z-buffer in LDS, min with LDS integer atomics on the bits of positive
//               float32 depths (which order like the floats), one vectorised store of the tile.  A triangle whose box covers
//               more than RASTER_SMALL_PX pixels of the tile, and every big triangle, is spread over the whole workgroup.
// Every fragment's depth is a pure function of (triangle, pixel) and the z-buffer keeps the minimum, so the image is the same
// bits whatever order the lists and the atomics run in.
//
// Colour renderer (after the depth pass): shaded RGB, depth and triangle ids on the same passes 1-4 and the same raster phase.
// Compiled with -ffp-contract=off: the host restatements (tests/render_np.py, tests/render_rgb_np.py, tests/render_tex_np.py)
// evaluate the same expressions in the same order.
#include <math.h>
#include <stdint.h>
#include "pose_common.h"

#define RT 32                  // screen tile edge (pixels)
#define RASTER_THREADS 256
#define RASTER_SMALL_PX 64     // larger per-tile boxes are rasterised by the whole workgroup
#define BIN_MAX_TILES 4        // triangles on more tiles go to the pose's big list

struct __align__(16) rvtx {
  float x, y;   // screen position (OpenCV pixel coordinates)
  double iz;    // 1 / Z, 0 when Z <= 0 or the projection is not finite
};

__global__ void render_vertex_kernel(int n_vert, const double* __restrict__ verts, const double* __restrict__ R,
                                     const double* __restrict__ t, const double* __restrict__ K4, rvtx* __restrict__ vtx) {
  const int pose = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_vert) return;
  const double* r = R + 9 * pose;
  const double* tt = t + 3 * pose;
  const double* k = K4 + 4 * pose;
  const double px = verts[3 * i], py = verts[3 * i + 1], pz = verts[3 * i + 2];
  const double X = r[0] * px + r[1] * py + r[2] * pz + tt[0];
  const double Y = r[3] * px + r[4] * py + r[5] * pz + tt[1];
  const double Z = r[6] * px + r[7] * py + r[8] * pz + tt[2];
  rvtx v;
  v.x = 0.0f;
  v.y = 0.0f;
  v.iz = 0.0;
  if (Z > 0.0) {
    const float x = (float)(k[0] * X / Z + k[2]);
    const float y = (float)(k[1] * Y / Z + k[3]);
    if (isfinite(x) && isfinite(y)) {
      v.x = x;
      v.y = y;
      v.iz = 1.0 / Z;
    }
  }
  vtx[(size_t)pose * n_vert + i] = v;
}

// Edge function of the directed edge a -> b at p, evaluated in the canonical direction of the edge and negated when (a, b) is
// the other one, so that two triangles sharing an edge get exactly opposite values.
__device__ __forceinline__ double edge_fn(float ax, float ay, float bx, float by, double px, double py) {
  const bool sw = (ax > bx) || (ax == bx && ay > by);
  const double x0 = sw ? bx : ax, y0 = sw ? by : ay, x1 = sw ? ax : bx, y1 = sw ? ay : by;
  const double e = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0);
  return sw ? -e : e;
}

// top-left rule: the inward normal (A, B) of an edge with w = A x + B y + C > 0 inside (image y points down)
__device__ __forceinline__ bool top_left(float ax, float ay, float bx, float by, double s) {
  const double A = -s * ((double)by - ay), B = s * ((double)bx - ax);
  return A > 0.0 || (A == 0.0 && B > 0.0);
}

struct tri_setup {
  float x[3], y[3];
  double iz[3];
  double s;            // orientation sign (w_i = s * e_i > 0 inside)
  bool tl[3];          // top-left flag of the edge opposite vertex i
  int c0, c1, r0, r1;  // pixel box (inclusive), clamped to the image; empty when c0 > c1 or r0 > r1
};

// false: the triangle draws nothing (bad index, vertex behind the camera, zero area, off-screen)
__device__ bool setup_triangle(const rvtx* __restrict__ vtx, int n_vert, const int* __restrict__ faces, int tri, int width,
                               int height, tri_setup* T) {
  const int i0 = faces[3 * tri], i1 = faces[3 * tri + 1], i2 = faces[3 * tri + 2];
  if (i0 < 0 || i0 >= n_vert || i1 < 0 || i1 >= n_vert || i2 < 0 || i2 >= n_vert) return false;
  const rvtx a = vtx[i0], b = vtx[i1], c = vtx[i2];
  if (!(a.iz > 0.0 && b.iz > 0.0 && c.iz > 0.0)) return false;
  T->x[0] = a.x; T->y[0] = a.y; T->iz[0] = a.iz;
  T->x[1] = b.x; T->y[1] = b.y; T->iz[1] = b.iz;
  T->x[2] = c.x; T->y[2] = c.y; T->iz[2] = c.iz;
  const double area2 = edge_fn(b.x, b.y, c.x, c.y, a.x, a.y);
  if (area2 == 0.0) return false;
  T->s = area2 > 0.0 ? 1.0 : -1.0;
  T->tl[0] = top_left(b.x, b.y, c.x, c.y, T->s);
  T->tl[1] = top_left(c.x, c.y, a.x, a.y, T->s);
  T->tl[2] = top_left(a.x, a.y, b.x, b.y, T->s);
  // pixel centres c + 0.5 in [min x, max x]; clamp in float before converting (coordinates may be huge)
  const double lo_x = fmin(fmin((double)a.x, (double)b.x), (double)c.x), hi_x = fmax(fmax((double)a.x, (double)b.x), (double)c.x);
  const double lo_y = fmin(fmin((double)a.y, (double)b.y), (double)c.y), hi_y = fmax(fmax((double)a.y, (double)b.y), (double)c.y);
  const double cl = ceil(fmin(fmax(lo_x - 0.5, -1.0), (double)width)), ch = floor(fmin(fmax(hi_x - 0.5, -1.0), (double)width));
  const double rl = ceil(fmin(fmax(lo_y - 0.5, -1.0), (double)height)), rh = floor(fmin(fmax(hi_y - 0.5, -1.0), (double)height));
  T->c0 = max((int)cl, 0);
  T->c1 = min((int)ch, width - 1);
  T->r0 = max((int)rl, 0);
  T->r1 = min((int)rh, height - 1);
  return T->c0 <= T->c1 && T->r0 <= T->r1;
}

// depth of the triangle at pixel (r, c), or 0 when the pixel centre is outside it or the depth is clipped
__device__ __forceinline__ float shade(const tri_setup& T, int r, int c, double zn, double zf) {
  const double px = c + 0.5, py = r + 0.5;
  const double w0 = T.s * edge_fn(T.x[1], T.y[1], T.x[2], T.y[2], px, py);
  const double w1 = T.s * edge_fn(T.x[2], T.y[2], T.x[0], T.y[0], px, py);
  const double w2 = T.s * edge_fn(T.x[0], T.y[0], T.x[1], T.y[1], px, py);
  const bool in0 = w0 > 0.0 || (w0 == 0.0 && T.tl[0]);
  const bool in1 = w1 > 0.0 || (w1 == 0.0 && T.tl[1]);
  const bool in2 = w2 > 0.0 || (w2 == 0.0 && T.tl[2]);
  if (!(in0 && in1 && in2)) return 0.0f;
  const double den = (w0 + w1) + w2;
  const double num = (w0 * T.iz[0] + w1 * T.iz[1]) + w2 * T.iz[2];
  const double Z = den / num;
  if (!(Z >= zn && Z <= zf)) return 0.0f;
  return (float)Z;
}

__device__ __forceinline__ void tri_tiles(const tri_setup& T, int* tc0, int* tc1, int* tr0, int* tr1) {
  *tc0 = T.c0 / RT;
  *tc1 = T.c1 / RT;
  *tr0 = T.r0 / RT;
  *tr1 = T.r1 / RT;
}

// mode 0: count entries per (pose, tile); mode 1: scatter triangle ids into the lists / the pose's big list
__global__ void render_bin_kernel(int mode, int n_vert, int n_tri, const int* __restrict__ faces, const rvtx* __restrict__ vtx_all,
                                  int width, int height, int tiles_x, int n_tiles, int* __restrict__ counts, int* __restrict__ cursor,
                                  int* __restrict__ list, int* __restrict__ big_n, int* __restrict__ big) {
  const int pose = blockIdx.y, tri = blockIdx.x * blockDim.x + threadIdx.x;
  if (tri >= n_tri) return;
  tri_setup T;
  if (!setup_triangle(vtx_all + (size_t)pose * n_vert, n_vert, faces, tri, width, height, &T)) return;
  int tc0, tc1, tr0, tr1;
  tri_tiles(T, &tc0, &tc1, &tr0, &tr1);
  const int nt = (tc1 - tc0 + 1) * (tr1 - tr0 + 1);
  if (nt > BIN_MAX_TILES) {
    if (mode == 1) big[(size_t)pose * n_tri + atomicAdd(&big_n[pose], 1)] = tri;
    return;
  }
  for (int ty = tr0; ty <= tr1; ++ty)
    for (int tx = tc0; tx <= tc1; ++tx) {
      const size_t b = (size_t)pose * n_tiles + ty * tiles_x + tx;
      if (mode == 0)
        atomicAdd(&counts[b], 1);
      else
        list[atomicAdd(&cursor[b], 1)] = tri;
    }
}

// The z-buffer word Z of a fragment: unsigned, the bits of its positive float32 depth (the depth pass), or unsigned long long,
// those bits << 32 | triangle index (the colour pass).  Both order like (depth, triangle), so the integer minimum resolves them.
template <class Z>
__device__ __forceinline__ void raster_px(Z* zb, const tri_setup& T, int tri, int r, int c, int r0, int c0, double zn, double zf) {
  const float z = shade(T, r, c, zn, zf);
  if (z > 0.0f) {
    if constexpr (sizeof(Z) == 4)
      atomicMin(&zb[(r - r0) * RT + (c - c0)], __float_as_uint(z));
    else
      atomicMin(&zb[(r - r0) * RT + (c - c0)], ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)tri);
  }
}

// the queued triangles, each spread over the whole workgroup
template <class Z>
__device__ void raster_queue(Z* zb, const int* queue, int qn, const rvtx* vtx, int n_vert, const int* faces, int width, int height,
                             int r0, int c0, double zn, double zf) {
  for (int q = 0; q < qn; ++q) {
    tri_setup T;
    setup_triangle(vtx, n_vert, faces, queue[q], width, height, &T);  // queued triangles passed it already
    const int a0 = max(T.c0, c0), a1 = min(T.c1, c0 + RT - 1), b0 = max(T.r0, r0), b1 = min(T.r1, r0 + RT - 1);
    const int bw = a1 - a0 + 1, n = bw * (b1 - b0 + 1);
    for (int k = threadIdx.x; k < n; k += RASTER_THREADS) raster_px(zb, T, queue[q], b0 + k / bw, a0 + k % bw, r0, c0, zn, zf);
  }
}

__global__ void __launch_bounds__(RASTER_THREADS)
render_raster_kernel(int n_vert, const int* __restrict__ faces, const rvtx* __restrict__ vtx_all, int n_tri, int width, int height,
                     int tiles_x, int n_tiles, const int* __restrict__ offsets, const int* __restrict__ list, const int* __restrict__ big_n,
                     const int* __restrict__ big, double zn, double zf, float* __restrict__ depth) {
  __shared__ unsigned zb[RT * RT];
  __shared__ int queue[RASTER_THREADS];
  __shared__ int qn;
  const int pose = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const int r0 = (tile / tiles_x) * RT, c0 = (tile % tiles_x) * RT;
  const rvtx* vtx = vtx_all + (size_t)pose * n_vert;
#define RASTER_EMPTY 0x7F800000u  // +inf
#include "render_raster_tile.inc"
  // the tile, 4 pixels of one row per thread
  const int r = r0 + tid / (RT / 4), c = c0 + (tid % (RT / 4)) * 4;
  if (r >= height) return;
  float v[4];
  for (int k = 0; k < 4; ++k) {
    const unsigned u = zb[(tid / (RT / 4)) * RT + (tid % (RT / 4)) * 4 + k];
    v[k] = u == 0x7F800000u ? 0.0f : __uint_as_float(u);
  }
  float* row = depth + ((size_t)pose * height + r) * width;
  if ((width & 3) == 0 && c + 3 < width) {
    *(float4*)(row + c) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < 4; ++k)
      if (c + k < width) row[c + k] = v[k];
  }
}

struct render_ws {
  rvtx* vtx;
  int *counts, *offsets, *cursor, *list, *big_n, *big;
  char* end;  // the first byte behind the lists (the colour pass keeps its vertex attributes there)
};

static size_t render_layout(int n_pose, int n_vert, int n_tri, int width, int height, char* base, render_ws* w) {
  const size_t tiles = (size_t)((width + RT - 1) / RT) * ((height + RT - 1) / RT);
  const size_t nb = (size_t)n_pose * tiles;
  const size_t sizes[7] = {(size_t)n_pose * n_vert * sizeof(rvtx), nb * sizeof(int), (nb + 1) * sizeof(int), nb * sizeof(int),
                           (size_t)n_pose * n_tri * BIN_MAX_TILES * sizeof(int), (size_t)n_pose * sizeof(int),
                           (size_t)n_pose * n_tri * sizeof(int)};
  size_t off[7], total = 0;
  for (int i = 0; i < 7; ++i) {
    off[i] = total;
    total += pp_align256(sizes[i]);
  }
  if (w) {
    w->vtx = (rvtx*)(base + off[0]);
    w->counts = (int*)(base + off[1]);
    w->offsets = (int*)(base + off[2]);
    w->cursor = (int*)(base + off[3]);
    w->list = (int*)(base + off[4]);
    w->big_n = (int*)(base + off[5]);
    w->big = (int*)(base + off[6]);
    w->end = base + total;
  }
  return total;
}

// the scan takes the number of (pose, tile) bins as an int and the bin kernel indexes counts / cursor with it
static bool render_shape_ok(int n_pose, int n_vert, int n_tri, int width, int height) {
  if (!(n_pose > 0 && n_pose <= 65535 && n_vert > 0 && n_tri > 0 && width > 0 && height > 0 && width <= 16384 && height <= 16384))
    return false;
  const long long tiles = (long long)((width + RT - 1) / RT) * ((height + RT - 1) / RT);
  return (long long)n_pose * n_tri * BIN_MAX_TILES <= 0x7FFFFFFFLL && (long long)n_pose * n_vert <= 0x7FFFFFFFLL &&
         (long long)n_pose * tiles <= 0x7FFFFFFFLL;
}

extern "C" size_t pp_render_workspace_bytes(int n_pose, int n_vert, int n_tri, int width, int height) {
  if (!render_shape_ok(n_pose, n_vert, n_tri, width, height)) return 0;
  return render_layout(n_pose, n_vert, n_tri, width, height, nullptr, nullptr);
}

// ---- colour renderer: shaded RGB, depth and triangle ids ------------------------------------------------------------------
// The 'rgb' / 'rgb+depth' modes of utils/hodan_renderer.py (shaders :22-103, _draw_rgb :480-518) beside the depth pass, which
// stays as it is.  Passes 1-4 are the depth pass's.  Then:
//   4b. attributes: per (pose, vertex) the eye position P = R p + t, the normal N = R n normalised (phong) and the direction to
//                   the light L = normalize(light - P), float64 (only when a colour output is asked for)
//   5.  raster:     the tile's z-buffer holds 64-bit keys (bits of the positive float32 depth) << 32 | triangle index, resolved
//                   with the 64-bit LDS integer minimum: the nearest fragment wins and, among fragments of equal float32 depth,
//                   the smallest triangle index.  The key is a pure function of (triangle, pixel), so the image is the same bits
//                   whatever order the lists and atomics run in, and the key's high word is the depth pass's value bit for bit.
//                   The same workgroup then shades the resolved tile -- a thread owns the 4 pixels of a row it stores -- so no
//                   id image goes through memory between raster and shade.
// Shading rule (the reference's shaders restated in the OpenCV camera frame; tests/render_rgb_np.py evaluates the same
// expressions in the same order): with the winning triangle's edge weights w_i as shade() computes them, q_i = w_i iz_i /
// ((w0 iz0 + w1 iz1) + w2 iz2) and an attribute is a = (q0 a0 + q1 a1) + q2 a2.  c = interpolated vertex colour, l =
// normalize(interp L); phong: n = normalize(interp N) (back-facing normals are not flipped: ambient light only); flat: n =
// normalize((P1 - P0) x (P2 - P0)) with its sign chosen so that n . P0 < 0 (the shader's cross(dFdx, dFdy) faces the viewer
// whatever the winding).  d = max(l . n, 0), 0 for a zero-length n or l; light_w = min(ambient + d, 1); out = (float)(light_w c);
// uint8 = rintf(out * 255.0f) (np.round(rgb * 255).astype(np.uint8), :516).  No fragment: bg_color, id -1, depth 0.
// Deviations: the 3-vector normal is normalised (the reference normalises u_nm * vec4(normal, 1) over four components);
// light_cam_pos is in the OpenCV camera frame; parity with an OpenGL driver is unpinned.
// Textured variant (pp_render_rgbd_tex; the shaders' other branch, hodan_renderer.py:56-57, 72-76, 98-102): the same kernel
// text (render_rgbd_raster.inc) compiled with TEX, in which c = texture(u, v) replaces the interpolated vertex colour.  (u, v) = the vertices' UVs
// interpolated like any attribute, read straight from uv (they do not depend on the pose); tri_shading holds them where the
// untextured kernel holds the vertex colours.  With x = u tex_w and y = v tex_h in GL texel space (GL row j is row
// tex_h - 1 - j of tex, which is given top row first as on disk; non-finite x or y: x = y = 0.5, the centre of GL texel (0, 0)):
//   nearest:  texel (wrap(floor(x)), wrap(floor(y)))
//   bilinear: xs = x - 0.5, i0 = floor(xs), fx = xs - i0, i1 = i0 + 1, likewise ys, j0, fy, j1, each index wrapped on its own;
//             per channel c = ((1 - fx) c00 + fx c10) (1 - fy) + ((1 - fx) c01 + fx c11) fy, cab = texel (ia, jb)
//   wrap:     clamp min(max(i, 0), n - 1) or repeat i - n floor(i / n), on integers (floors beyond +-2^30 are taken as +-2^30)
// and a channel is (double)byte / 255.0.  tests/render_tex_np.py evaluates the same expressions in the same order.  No mip-maps.
#define ZKEY_EMPTY 0xFFFFFFFFFFFFFFFFull
#define TEX_INDEX_MAX 1073741824.0  // 2^30

struct __align__(8) rattr {
  double P[3], N[3], L[3];
};

struct rgb_params {
  double light[3], bg[3], ambient;
  int phong;
};

// v / |v|, or 0 when the length is 0 (or not a number)
__device__ __forceinline__ void normalize3(double x, double y, double z, double* o) {
  const double len = sqrt((x * x + y * y) + z * z);
  const bool ok = len > 0.0;
  o[0] = ok ? x / len : 0.0;
  o[1] = ok ? y / len : 0.0;
  o[2] = ok ? z / len : 0.0;
}

__global__ void render_attr_kernel(int n_vert, const double* __restrict__ verts, const double* __restrict__ normals,
                                   const double* __restrict__ R, const double* __restrict__ t, rgb_params prm, rattr* __restrict__ attr) {
  const int pose = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_vert) return;
  const double* r = R + 9 * pose;
  const double* tt = t + 3 * pose;
  const double px = verts[3 * i], py = verts[3 * i + 1], pz = verts[3 * i + 2];
  rattr a;
  a.P[0] = r[0] * px + r[1] * py + r[2] * pz + tt[0];
  a.P[1] = r[3] * px + r[4] * py + r[5] * pz + tt[1];
  a.P[2] = r[6] * px + r[7] * py + r[8] * pz + tt[2];
  a.N[0] = a.N[1] = a.N[2] = 0.0;
  if (prm.phong) {
    const double nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
    normalize3(r[0] * nx + r[1] * ny + r[2] * nz, r[3] * nx + r[4] * ny + r[5] * nz, r[6] * nx + r[7] * ny + r[8] * nz, a.N);
  }
  normalize3(prm.light[0] - a.P[0], prm.light[1] - a.P[1], prm.light[2] - a.P[2], a.L);
  attr[(size_t)pose * n_vert + i] = a;
}

// what shading needs of the triangle a pixel shows: kept while the thread's next pixel shows the same one
// TEX: C holds the vertices' (u, v) in place of their colours
template <bool TEX>
struct tri_shading {
  tri_setup T;
  double L[3][3], N[3][3], C[3][TEX ? 2 : 3];  // per vertex; flat shading: N[0] is the face normal
};

// the texture of the textured kernel, passed by value
struct tex_params {
  const unsigned* tex;  // [h,w] RGBX texels, one 32-bit word each (R in the low byte), top row first
  int w, h, bilinear, repeat;
};

// colors: [n_vert,3] vertex colours or, TEX, [n_vert,2] texture coordinates
template <bool TEX>
__device__ void load_tri_shading(const rvtx* __restrict__ vtx, const rattr* __restrict__ attr, const double* __restrict__ colors,
                                 int n_vert, const int* __restrict__ faces, int tri, int width, int height, int phong,
                                 tri_shading<TEX>* S) {
  setup_triangle(vtx, n_vert, faces, tri, width, height, &S->T);  // the triangle won a pixel: it passed already
  double P[3][3];
  for (int v = 0; v < 3; ++v) {
    const int i = faces[3 * tri + v];
    const rattr* a = attr + i;
    for (int k = 0; k < 3; ++k) {
      P[v][k] = a->P[k];
      S->L[v][k] = a->L[k];
      S->N[v][k] = a->N[k];
      if (!TEX) S->C[v][k] = colors[3 * (size_t)i + k];
    }
    if (TEX) {
      S->C[v][0] = colors[2 * (size_t)i];
      S->C[v][1] = colors[2 * (size_t)i + 1];
    }
  }
  if (!phong) {
    const double ux = P[1][0] - P[0][0], uy = P[1][1] - P[0][1], uz = P[1][2] - P[0][2];
    const double vx = P[2][0] - P[0][0], vy = P[2][1] - P[0][1], vz = P[2][2] - P[0][2];
    double* n = S->N[0];
    normalize3(uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx, n);
    if ((n[0] * P[0][0] + n[1] * P[0][1]) + n[2] * P[0][2] > 0.0) {
      n[0] = -n[0];
      n[1] = -n[1];
      n[2] = -n[2];
    }
  }
}

// texel index i (any integer) -> [0, n): clamp to edge, or repeat (i - n floor(i / n) on integers)
__device__ __forceinline__ int tex_wrap(int i, int n, int repeat) {
  if (repeat) {
    const int m = i % n;
    return m < 0 ? m + n : m;
  }
  return min(max(i, 0), n - 1);
}

// texel (i, j) of GL texel space, both in range: row tex_h - 1 - j of the image as given.  tex_w * tex_h <= 2^28: 32-bit offsets
__device__ __forceinline__ unsigned tex_fetch(const tex_params& tp, int i, int j) {
  return tp.tex[(unsigned)(tp.h - 1 - j) * (unsigned)tp.w + (unsigned)i];
}

// floor value f of a texel coordinate as an integer; floors beyond +-2^30 are taken as +-2^30, so no conversion overflows
__device__ __forceinline__ int tex_int(double f) { return (int)fmin(fmax(f, -TEX_INDEX_MAX), TEX_INDEX_MAX); }

// the texture at (u, v), three channels in [0, 1]; the rule is in the comment at the head of the colour renderer
__device__ __forceinline__ void sample_tex(const tex_params& tp, double u, double v, double* c) {
  double x = u * tp.w, y = v * tp.h;
  if (!(isfinite(x) && isfinite(y))) x = y = 0.5;  // no index is computed from a NaN
  if (!tp.bilinear) {
    const unsigned p = tex_fetch(tp, tex_wrap(tex_int(floor(x)), tp.w, tp.repeat), tex_wrap(tex_int(floor(y)), tp.h, tp.repeat));
    for (int k = 0; k < 3; ++k) c[k] = (double)((p >> (8 * k)) & 0xFFu) / 255.0;
    return;
  }
  const double xs = x - 0.5, ys = y - 0.5;
  const double fi = floor(xs), fj = floor(ys);
  const double fx = xs - fi, fy = ys - fj;
  const int i = tex_int(fi), j = tex_int(fj);
  const int i0 = tex_wrap(i, tp.w, tp.repeat), i1 = tex_wrap(i + 1, tp.w, tp.repeat);
  const int j0 = tex_wrap(j, tp.h, tp.repeat), j1 = tex_wrap(j + 1, tp.h, tp.repeat);
  const unsigned p00 = tex_fetch(tp, i0, j0), p10 = tex_fetch(tp, i1, j0), p01 = tex_fetch(tp, i0, j1), p11 = tex_fetch(tp, i1, j1);
  for (int k = 0; k < 3; ++k) {
    const double c00 = (double)((p00 >> (8 * k)) & 0xFFu) / 255.0, c10 = (double)((p10 >> (8 * k)) & 0xFFu) / 255.0;
    const double c01 = (double)((p01 >> (8 * k)) & 0xFFu) / 255.0, c11 = (double)((p11 >> (8 * k)) & 0xFFu) / 255.0;
    c[k] = ((1.0 - fx) * c00 + fx * c10) * (1.0 - fy) + ((1.0 - fx) * c01 + fx * c11) * fy;
  }
}

template <bool TEX>
__device__ __forceinline__ void shade_rgb_px(const tri_shading<TEX>& S, int r, int c, const rgb_params& prm, const tex_params& tp,
                                             float* out) {
  const tri_setup& T = S.T;
  const double px = c + 0.5, py = r + 0.5;
  const double w0 = T.s * edge_fn(T.x[1], T.y[1], T.x[2], T.y[2], px, py);
  const double w1 = T.s * edge_fn(T.x[2], T.y[2], T.x[0], T.y[0], px, py);
  const double w2 = T.s * edge_fn(T.x[0], T.y[0], T.x[1], T.y[1], px, py);
  const double b0 = w0 * T.iz[0], b1 = w1 * T.iz[1], b2 = w2 * T.iz[2];
  const double den = (b0 + b1) + b2;
  const double q0 = b0 / den, q1 = b1 / den, q2 = b2 / den;
  double l[3], n[3];
  normalize3((q0 * S.L[0][0] + q1 * S.L[1][0]) + q2 * S.L[2][0], (q0 * S.L[0][1] + q1 * S.L[1][1]) + q2 * S.L[2][1],
             (q0 * S.L[0][2] + q1 * S.L[1][2]) + q2 * S.L[2][2], l);
  if (prm.phong) {
    normalize3((q0 * S.N[0][0] + q1 * S.N[1][0]) + q2 * S.N[2][0], (q0 * S.N[0][1] + q1 * S.N[1][1]) + q2 * S.N[2][1],
               (q0 * S.N[0][2] + q1 * S.N[1][2]) + q2 * S.N[2][2], n);
  } else {
    n[0] = S.N[0][0];
    n[1] = S.N[0][1];
    n[2] = S.N[0][2];
  }
  const double dot = (l[0] * n[0] + l[1] * n[1]) + l[2] * n[2];
  const double d = dot > 0.0 ? dot : 0.0;
  const double sum = prm.ambient + d;
  const double light_w = sum > 1.0 ? 1.0 : sum;
  if (TEX) {
    double t[3];
    sample_tex(tp, (q0 * S.C[0][0] + q1 * S.C[1][0]) + q2 * S.C[2][0], (q0 * S.C[0][1] + q1 * S.C[1][1]) + q2 * S.C[2][1], t);
    for (int k = 0; k < 3; ++k) out[k] = (float)(light_w * t[k]);
  } else {
    for (int k = 0; k < 3; ++k) out[k] = (float)(light_w * ((q0 * S.C[0][k] + q1 * S.C[1][k]) + q2 * S.C[2][k]));
  }
}

__device__ __forceinline__ unsigned char rgb_to_u8(float v) { return (unsigned char)fminf(fmaxf(rintf(v * 255.0f), 0.0f), 255.0f); }

// the untextured kernel, then the textured one
#define RASTER_KERNEL render_rgbd_raster_kernel
#define RASTER_TEX false
#define RASTER_TP_PARAM
#define RASTER_TP tex_params()
#include "render_rgbd_raster.inc"
#define RASTER_KERNEL render_rgbd_tex_raster_kernel
#define RASTER_TEX true
#define RASTER_TP_PARAM , tex_params tp
#define RASTER_TP tp
#include "render_rgbd_raster.inc"

// ---- host paths ---------------------------------------------------------------------------------------------------------------
// the two checks every entry point words alike, under its own name
static int render_check_shape(pp_ctx* ctx, const char* what, int n_pose, int n_vert, int n_tri, int width, int height) {
  PP_CHECK_ARG(ctx, render_shape_ok(n_pose, n_vert, n_tri, width, height), PP_ERR_SHAPE,
               "%s: need 1..65535 poses, vertices, triangles, a 1..16384 image, n_pose * n_tri * 4 < 2^31 and n_pose * tiles < 2^31 (32 x 32 pixel tiles)",
               what);
  return PP_OK;
}

static int render_check_clip(pp_ctx* ctx, const char* what, double clip_near, double clip_far) {
  PP_CHECK_ARG(ctx, clip_near >= 0.0 && clip_far >= clip_near, PP_ERR_ARG, "%s: need 0 <= clip_near <= clip_far", what);
  return PP_OK;
}

// Passes 1-4 of entry point `what`: the workspace carved up into w (it must hold `extra` more bytes behind the lists), then vertex,
// count, scan and scatter; with prm, the colour pass's attributes (4b) to w->end behind the vertex kernel.  The raster kernel
// that follows reads w.
static int render_bin_passes(pp_ctx* ctx, const char* what, int n_pose, int n_vert, const double* verts, int n_tri, const int* faces,
                             const double* R, const double* t, const double* K4, int width, int height, void* workspace,
                             size_t workspace_bytes, size_t extra, const double* normals, const rgb_params* prm, render_ws* w) {
  const size_t need = render_layout(n_pose, n_vert, n_tri, width, height, (char*)workspace, w) + extra;
  PP_CHECK_ARG(ctx, workspace_bytes >= need, PP_ERR_ARG, "%s: workspace of %zu bytes, need %zu", what, workspace_bytes, need);
  const int tiles_x = (width + RT - 1) / RT, n_tiles = tiles_x * ((height + RT - 1) / RT);
  const size_t nb = (size_t)n_pose * n_tiles;
  hipMemsetAsync(w->counts, 0, nb * sizeof(int), ctx->stream);
  hipMemsetAsync(w->big_n, 0, (size_t)n_pose * sizeof(int), ctx->stream);
  const dim3 vg((n_vert + 255) / 256, n_pose);
  hipLaunchKernelGGL(render_vertex_kernel, vg, dim3(256), 0, ctx->stream, n_vert, verts, R, t, K4, w->vtx);
  if (prm) hipLaunchKernelGGL(render_attr_kernel, vg, dim3(256), 0, ctx->stream, n_vert, verts, normals, R, t, *prm, (rattr*)w->end);
  const dim3 tg((n_tri + 255) / 256, n_pose);
  hipLaunchKernelGGL(render_bin_kernel, tg, dim3(256), 0, ctx->stream, 0, n_vert, n_tri, faces, (const rvtx*)w->vtx, width, height,
                     tiles_x, n_tiles, w->counts, w->cursor, w->list, w->big_n, w->big);
  hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, (int)nb, (const int*)w->counts, w->offsets, w->cursor);
  hipLaunchKernelGGL(render_bin_kernel, tg, dim3(256), 0, ctx->stream, 1, n_vert, n_tri, faces, (const rvtx*)w->vtx, width, height,
                     tiles_x, n_tiles, w->counts, w->cursor, w->list, w->big_n, w->big);
  return PP_OK;
}

extern "C" int pp_render_depth_f32(pp_ctx* ctx, int n_pose, int n_vert, const double* verts, int n_tri, const int* faces,
                                   const double* R, const double* t, const double* K4, int width, int height, double clip_near,
                                   double clip_far, void* workspace, size_t workspace_bytes, float* depth) {
  const char* what = "pp_render_depth_f32";
  PP_REQUIRE_CTX(ctx);
  if (const int rc = render_check_shape(ctx, what, n_pose, n_vert, n_tri, width, height)) return rc;
  PP_CHECK_ARG(ctx, verts && faces && R && t && K4 && workspace && depth, PP_ERR_ARG, "%s: null argument", what);
  if (const int rc = render_check_clip(ctx, what, clip_near, clip_far)) return rc;
  render_ws w;
  if (const int rc = render_bin_passes(ctx, what, n_pose, n_vert, verts, n_tri, faces, R, t, K4, width, height, workspace, workspace_bytes,
                                       0, nullptr, nullptr, &w))
    return rc;
  const int tiles_x = (width + RT - 1) / RT, n_tiles = tiles_x * ((height + RT - 1) / RT);
  hipLaunchKernelGGL(render_raster_kernel, dim3(n_tiles, n_pose), dim3(RASTER_THREADS), 0, ctx->stream, n_vert, faces,
                     (const rvtx*)w.vtx, n_tri, width, height, tiles_x, n_tiles, (const int*)w.offsets, (const int*)w.list,
                     (const int*)w.big_n, (const int*)w.big, clip_near, clip_far, depth);
  PP_CHECK_LAUNCH(ctx, what);
  return PP_OK;
}

// the per-(pose, vertex) attributes, behind the depth pass's layout
static size_t render_attr_bytes(int n_pose, int n_vert) { return pp_align256((size_t)n_pose * n_vert * sizeof(rattr)); }

extern "C" size_t pp_render_rgbd_workspace_bytes(int n_pose, int n_vert, int n_tri, int width, int height) {
  if (!render_shape_ok(n_pose, n_vert, n_tri, width, height)) return 0;
  return render_layout(n_pose, n_vert, n_tri, width, height, nullptr, nullptr) + render_attr_bytes(n_pose, n_vert);
}

// pp_render_rgbd (tp null; colors [n_vert,3]) and pp_render_rgbd_tex (colors: the texture coordinates [n_vert,2])
static int render_rgbd_run(pp_ctx* ctx, const char* what, int n_pose, int n_vert, const double* verts, const double* colors,
                           const double* normals, int n_tri, const int* faces, const double* R, const double* t, const double* K4,
                           int width, int height, double clip_near, double clip_far, int shading, double ambient_weight,
                           const double* light_cam_pos, const double* bg_color, void* workspace, size_t workspace_bytes, float* depth,
                           int* tri_id, float* rgb_f32, unsigned char* rgb_u8, const tex_params* tp) {
  PP_REQUIRE_CTX(ctx);
  if (const int rc = render_check_shape(ctx, what, n_pose, n_vert, n_tri, width, height)) return rc;
  PP_CHECK_ARG(ctx, verts && faces && R && t && K4 && workspace && light_cam_pos && bg_color, PP_ERR_ARG, "%s: null argument", what);
  PP_CHECK_ARG(ctx, depth || tri_id || rgb_f32 || rgb_u8, PP_ERR_ARG, "%s: no output requested", what);
  const bool rgb = rgb_f32 || rgb_u8;
  PP_CHECK_ARG(ctx, shading == 0 || shading == 1, PP_ERR_ARG, "%s: shading must be 0 (flat) or 1 (phong)", what);
  if (tp) {
    PP_CHECK_ARG(ctx, !rgb || (colors && tp->tex), PP_ERR_ARG, "%s: a colour output needs uv and tex", what);
    PP_CHECK_ARG(ctx, (reinterpret_cast<uintptr_t>(tp->tex) & 3u) == 0, PP_ERR_ALIGN, "%s: tex must be aligned to 4 bytes", what);
  } else {
    PP_CHECK_ARG(ctx, !rgb || colors, PP_ERR_ARG, "%s: a colour output needs vertex colours", what);
  }
  PP_CHECK_ARG(ctx, !rgb || shading == 0 || normals, PP_ERR_ARG, "%s: phong shading needs vertex normals", what);
  if (const int rc = render_check_clip(ctx, what, clip_near, clip_far)) return rc;
  PP_CHECK_ARG(ctx, ambient_weight >= 0.0 && ambient_weight <= 1.0, PP_ERR_ARG, "%s: ambient_weight must lie in [0, 1]", what);
  rgb_params prm;
  for (int k = 0; k < 3; ++k) {
    PP_CHECK_ARG(ctx, isfinite(light_cam_pos[k]), PP_ERR_ARG, "%s: light_cam_pos must be finite", what);
    PP_CHECK_ARG(ctx, bg_color[k] >= 0.0 && bg_color[k] <= 1.0, PP_ERR_ARG, "%s: bg_color must lie in [0, 1]", what);
    prm.light[k] = light_cam_pos[k];
    prm.bg[k] = bg_color[k];
  }
  prm.ambient = ambient_weight;
  prm.phong = shading;
  render_ws w;
  if (const int rc = render_bin_passes(ctx, what, n_pose, n_vert, verts, n_tri, faces, R, t, K4, width, height, workspace, workspace_bytes,
                                       render_attr_bytes(n_pose, n_vert), normals, rgb ? &prm : nullptr, &w))
    return rc;
  const rattr* attr = (const rattr*)w.end;
  const int tiles_x = (width + RT - 1) / RT, n_tiles = tiles_x * ((height + RT - 1) / RT);
  if (tp && rgb) {
    hipLaunchKernelGGL(render_rgbd_tex_raster_kernel, dim3(n_tiles, n_pose), dim3(RASTER_THREADS), 0, ctx->stream, n_vert, faces,
                       (const rvtx*)w.vtx, n_tri, width, height, tiles_x, n_tiles, (const int*)w.offsets, (const int*)w.list,
                       (const int*)w.big_n, (const int*)w.big, clip_near, clip_far, attr, colors, prm, depth, tri_id, rgb_f32,
                       rgb_u8, *tp);
  } else {  // (without a colour output the shading tail is not reached: the untextured kernel serves both entry points)
    hipLaunchKernelGGL(render_rgbd_raster_kernel, dim3(n_tiles, n_pose), dim3(RASTER_THREADS), 0, ctx->stream, n_vert, faces,
                       (const rvtx*)w.vtx, n_tri, width, height, tiles_x, n_tiles, (const int*)w.offsets, (const int*)w.list,
                       (const int*)w.big_n, (const int*)w.big, clip_near, clip_far, attr, colors, prm, depth, tri_id, rgb_f32,
                       rgb_u8);
  }
  PP_CHECK_LAUNCH(ctx, what);
  return PP_OK;
}

extern "C" int pp_render_rgbd(pp_ctx* ctx, int n_pose, int n_vert, const double* verts, const double* colors, const double* normals,
                              int n_tri, const int* faces, const double* R, const double* t, const double* K4, int width, int height,
                              double clip_near, double clip_far, int shading, double ambient_weight, const double* light_cam_pos,
                              const double* bg_color, void* workspace, size_t workspace_bytes, float* depth, int* tri_id,
                              float* rgb_f32, unsigned char* rgb_u8) {
  return render_rgbd_run(ctx, "pp_render_rgbd", n_pose, n_vert, verts, colors, normals, n_tri, faces, R, t, K4, width, height, clip_near,
                         clip_far, shading, ambient_weight, light_cam_pos, bg_color, workspace, workspace_bytes, depth, tri_id, rgb_f32,
                         rgb_u8, nullptr);
}

#define TEX_MAX_TEXELS (1 << 28)  // texels are fetched at 32-bit offsets

static bool render_tex_ok(int tex_w, int tex_h) {
  return tex_w >= 1 && tex_w <= 16384 && tex_h >= 1 && tex_h <= 16384 && (long long)tex_w * tex_h <= TEX_MAX_TEXELS;
}

extern "C" size_t pp_render_rgbd_tex_workspace_bytes(int n_pose, int n_vert, int n_tri, int width, int height, int tex_w, int tex_h) {
  if (!render_tex_ok(tex_w, tex_h)) return 0;
  return pp_render_rgbd_workspace_bytes(n_pose, n_vert, n_tri, width, height);
}

extern "C" int pp_render_rgbd_tex(pp_ctx* ctx, int n_pose, int n_vert, const double* verts, const double* uv, const unsigned char* tex,
                                  int tex_w, int tex_h, int filter, int wrap, const double* normals, int n_tri, const int* faces,
                                  const double* R, const double* t, const double* K4, int width, int height, double clip_near,
                                  double clip_far, int shading, double ambient_weight, const double* light_cam_pos,
                                  const double* bg_color, void* workspace, size_t workspace_bytes, float* depth, int* tri_id,
                                  float* rgb_f32, unsigned char* rgb_u8) {
  PP_REQUIRE_CTX(ctx);
  if (tex || rgb_f32 || rgb_u8) {  // a call for depth / tri_id alone needs no texture
    PP_CHECK_ARG(ctx, render_tex_ok(tex_w, tex_h), PP_ERR_SHAPE,
                 "pp_render_rgbd_tex: need a texture of 1..16384 x 1..16384 and at most 2^28 texels, got %d x %d", tex_w, tex_h);
    PP_CHECK_ARG(ctx, filter == 0 || filter == 1, PP_ERR_ARG, "pp_render_rgbd_tex: filter must be 0 (nearest) or 1 (bilinear)");
    PP_CHECK_ARG(ctx, wrap == 0 || wrap == 1, PP_ERR_ARG, "pp_render_rgbd_tex: wrap must be 0 (clamp to edge) or 1 (repeat)");
  }
  tex_params tp;
  tp.tex = (const unsigned*)tex;
  tp.w = tex_w;
  tp.h = tex_h;
  tp.bilinear = filter;
  tp.repeat = wrap;
  return render_rgbd_run(ctx, "pp_render_rgbd_tex", n_pose, n_vert, verts, uv, normals, n_tri, faces, R, t, K4, width, height, clip_near,
                         clip_far, shading, ambient_weight, light_cam_pos, bg_color, workspace, workspace_bytes, depth, tri_id, rgb_f32,
                         rgb_u8, &tp);
}
