// Depth renderer and the VSD pose error of the evaluation tail (tless_eval.py:470-471, 651-662 and the
// same calls in occlusion_eval.py / ycbv_eval.py / homebrewed_eval.py / linemod_eval.py).
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
// VSD: pose_error.py:15-61 + 105-176 per problem on the rendered depth images, float64 where the reference is; per-block
// partial counts / sums, then one ordered pass per problem.
// Scene ground truth (at the end of the file): masks, boxes, pixel counts and the id image of a scene from its instances' renders.
// Colour renderer (after the depth pass): shaded RGB, depth and triangle ids; a scene's image from its instances' colour renders
// (at the end of the file).
// Compiled with -ffp-contract=off: the host restatements (tests/render_np.py, utils/pose_error.py) evaluate the same
// expressions in the same order.
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "pose_common.h"

#define RT 32                  // screen tile edge (pixels)
#define RASTER_THREADS 256
#define RASTER_SMALL_PX 64     // larger per-tile boxes are rasterised by the whole workgroup
#define BIN_MAX_TILES 4        // triangles on more tiles go to the pose's big list
#define VSD_THREADS 256
#define VSD_PER_THREAD 4
#define VSD_BLOCK (VSD_THREADS * VSD_PER_THREAD)

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

__device__ __forceinline__ void raster_px(unsigned* zb, const tri_setup& T, int r, int c, int r0, int c0, double zn, double zf) {
  const float z = shade(T, r, c, zn, zf);
  if (z > 0.0f) atomicMin(&zb[(r - r0) * RT + (c - c0)], __float_as_uint(z));
}

// the queued triangles, each spread over the whole workgroup
__device__ void raster_queue(unsigned* zb, const int* queue, int qn, const rvtx* vtx, int n_vert, const int* faces, int width,
                             int height, int r0, int c0, double zn, double zf) {
  for (int q = 0; q < qn; ++q) {
    tri_setup T;
    setup_triangle(vtx, n_vert, faces, queue[q], width, height, &T);  // queued triangles passed it already
    const int a0 = max(T.c0, c0), a1 = min(T.c1, c0 + RT - 1), b0 = max(T.r0, r0), b1 = min(T.r1, r0 + RT - 1);
    const int bw = a1 - a0 + 1, n = bw * (b1 - b0 + 1);
    for (int k = threadIdx.x; k < n; k += RASTER_THREADS) raster_px(zb, T, b0 + k / bw, a0 + k % bw, r0, c0, zn, zf);
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
  for (int k = tid; k < RT * RT; k += RASTER_THREADS) zb[k] = 0x7F800000u;  // +inf
  if (tid == 0) qn = 0;
  __syncthreads();
  const size_t b = (size_t)pose * n_tiles + tile;
  const int l0 = offsets[b], l1 = offsets[b + 1];
  for (int base = l0; base < l1; base += RASTER_THREADS) {
    if (base + tid < l1) {
      const int tri = list[base + tid];
      tri_setup T;
      if (setup_triangle(vtx, n_vert, faces, tri, width, height, &T)) {
        const int a0 = max(T.c0, c0), a1 = min(T.c1, c0 + RT - 1), b0 = max(T.r0, r0), b1 = min(T.r1, r0 + RT - 1);
        const int area = (a1 - a0 + 1) * (b1 - b0 + 1);
        if (a0 <= a1 && b0 <= b1) {
          if (area <= RASTER_SMALL_PX) {
            for (int r = b0; r <= b1; ++r)
              for (int c = a0; c <= a1; ++c) raster_px(zb, T, r, c, r0, c0, zn, zf);
          } else {
            queue[atomicAdd(&qn, 1)] = tri;
          }
        }
      }
    }
    __syncthreads();
    raster_queue(zb, queue, qn, vtx, n_vert, faces, width, height, r0, c0, zn, zf);
    __syncthreads();
    if (tid == 0) qn = 0;
    __syncthreads();
  }
  const int nb = big_n[pose];
  for (int base = 0; base < nb; base += RASTER_THREADS) {
    if (base + tid < nb) {
      const int tri = big[(size_t)pose * n_tri + base + tid];
      tri_setup T;
      if (setup_triangle(vtx, n_vert, faces, tri, width, height, &T) && T.c0 < c0 + RT && T.c1 >= c0 && T.r0 < r0 + RT && T.r1 >= r0)
        queue[atomicAdd(&qn, 1)] = tri;
    }
    __syncthreads();
    raster_queue(zb, queue, qn, vtx, n_vert, faces, width, height, r0, c0, zn, zf);
    __syncthreads();
    if (tid == 0) qn = 0;
    __syncthreads();
  }
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
  }
  return total;
}

static bool render_shape_ok(int n_pose, int n_vert, int n_tri, int width, int height) {
  return n_pose > 0 && n_pose <= 65535 && n_vert > 0 && n_tri > 0 && width > 0 && height > 0 && width <= 16384 && height <= 16384 &&
         (long long)n_pose * n_tri * BIN_MAX_TILES <= 0x7FFFFFFFLL && (long long)n_pose * n_vert <= 0x7FFFFFFFLL;
}

extern "C" size_t pp_render_workspace_bytes(int n_pose, int n_vert, int n_tri, int width, int height) {
  if (!render_shape_ok(n_pose, n_vert, n_tri, width, height)) return 0;
  return render_layout(n_pose, n_vert, n_tri, width, height, nullptr, nullptr);
}

extern "C" int pp_render_depth_f32(pp_ctx* ctx, int n_pose, int n_vert, const double* verts, int n_tri, const int* faces,
                                   const double* R, const double* t, const double* K4, int width, int height, double clip_near,
                                   double clip_far, void* workspace, size_t workspace_bytes, float* depth) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, render_shape_ok(n_pose, n_vert, n_tri, width, height), PP_ERR_SHAPE,
               "pp_render_depth_f32: need 1..65535 poses, vertices, triangles, a 1..16384 image and n_pose * n_tri * 4 < 2^31");
  PP_CHECK_ARG(ctx, verts && faces && R && t && K4 && workspace && depth, PP_ERR_ARG, "pp_render_depth_f32: null argument");
  PP_CHECK_ARG(ctx, clip_near >= 0.0 && clip_far >= clip_near, PP_ERR_ARG, "pp_render_depth_f32: need 0 <= clip_near <= clip_far");
  render_ws w;
  const size_t need = render_layout(n_pose, n_vert, n_tri, width, height, (char*)workspace, &w);
  PP_CHECK_ARG(ctx, workspace_bytes >= need, PP_ERR_ARG, "pp_render_depth_f32: workspace of %zu bytes, need %zu", workspace_bytes, need);
  const int tiles_x = (width + RT - 1) / RT, n_tiles = tiles_x * ((height + RT - 1) / RT);
  const size_t nb = (size_t)n_pose * n_tiles;
  hipMemsetAsync(w.counts, 0, nb * sizeof(int), ctx->stream);
  hipMemsetAsync(w.big_n, 0, (size_t)n_pose * sizeof(int), ctx->stream);
  hipLaunchKernelGGL(render_vertex_kernel, dim3((n_vert + 255) / 256, n_pose), dim3(256), 0, ctx->stream, n_vert, verts, R, t, K4, w.vtx);
  const dim3 tg((n_tri + 255) / 256, n_pose);
  hipLaunchKernelGGL(render_bin_kernel, tg, dim3(256), 0, ctx->stream, 0, n_vert, n_tri, faces, (const rvtx*)w.vtx, width, height,
                     tiles_x, n_tiles, w.counts, w.cursor, w.list, w.big_n, w.big);
  hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, (int)nb, (const int*)w.counts, w.offsets, w.cursor);
  hipLaunchKernelGGL(render_bin_kernel, tg, dim3(256), 0, ctx->stream, 1, n_vert, n_tri, faces, (const rvtx*)w.vtx, width, height,
                     tiles_x, n_tiles, w.counts, w.cursor, w.list, w.big_n, w.big);
  hipLaunchKernelGGL(render_raster_kernel, dim3(n_tiles, n_pose), dim3(RASTER_THREADS), 0, ctx->stream, n_vert, faces,
                     (const rvtx*)w.vtx, n_tri, width, height, tiles_x, n_tiles, (const int*)w.offsets, (const int*)w.list,
                     (const int*)w.big_n, (const int*)w.big, clip_near, clip_far, depth);
  PP_CHECK_LAUNCH(ctx, "pp_render_depth_f32");
  return PP_OK;
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

__device__ __forceinline__ void raster_px(unsigned long long* zb, const tri_setup& T, int tri, int r, int c, int r0, int c0, double zn,
                                          double zf) {
  const float z = shade(T, r, c, zn, zf);
  if (z > 0.0f) atomicMin(&zb[(r - r0) * RT + (c - c0)], ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)tri);
}

__device__ void raster_queue(unsigned long long* zb, const int* queue, int qn, const rvtx* vtx, int n_vert, const int* faces, int width,
                             int height, int r0, int c0, double zn, double zf) {
  for (int q = 0; q < qn; ++q) {
    tri_setup T;
    setup_triangle(vtx, n_vert, faces, queue[q], width, height, &T);  // queued triangles passed it already
    const int a0 = max(T.c0, c0), a1 = min(T.c1, c0 + RT - 1), b0 = max(T.r0, r0), b1 = min(T.r1, r0 + RT - 1);
    const int bw = a1 - a0 + 1, n = bw * (b1 - b0 + 1);
    for (int k = threadIdx.x; k < n; k += RASTER_THREADS) raster_px(zb, T, queue[q], b0 + k / bw, a0 + k % bw, r0, c0, zn, zf);
  }
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

// The untextured kernel, and the declaration of the textured one, which is defined at the end of the file: the code object then
// holds the kernels that were there before it at the places they had.
#define RASTER_KERNEL render_rgbd_raster_kernel
#define RASTER_TEX false
#define RASTER_TP_PARAM
#define RASTER_TP tex_params()
#include "render_rgbd_raster.inc"

__global__ void __launch_bounds__(RASTER_THREADS)
render_rgbd_tex_raster_kernel(int n_vert, const int* __restrict__ faces, const rvtx* __restrict__ vtx_all, int n_tri, int width, int height,
                              int tiles_x, int n_tiles, const int* __restrict__ offsets, const int* __restrict__ list,
                              const int* __restrict__ big_n, const int* __restrict__ big, double zn, double zf,
                              const rattr* __restrict__ attr_all, const double* __restrict__ uv, rgb_params prm, float* __restrict__ depth,
                              int* __restrict__ tri_id, float* __restrict__ rgb_f32, unsigned char* __restrict__ rgb_u8, tex_params tp);

static size_t render_rgbd_layout(int n_pose, int n_vert, int n_tri, int width, int height, char* base, render_ws* w, rattr** attr) {
  const size_t head = render_layout(n_pose, n_vert, n_tri, width, height, base, w);
  if (attr) *attr = (rattr*)(base + head);
  return head + pp_align256((size_t)n_pose * n_vert * sizeof(rattr));
}

extern "C" size_t pp_render_rgbd_workspace_bytes(int n_pose, int n_vert, int n_tri, int width, int height) {
  if (!render_shape_ok(n_pose, n_vert, n_tri, width, height)) return 0;
  return render_rgbd_layout(n_pose, n_vert, n_tri, width, height, nullptr, nullptr, nullptr);
}

// pp_render_rgbd (tp null; colors [n_vert,3]) and pp_render_rgbd_tex (colors: the texture coordinates [n_vert,2])
static int render_rgbd_run(pp_ctx* ctx, const char* what, int n_pose, int n_vert, const double* verts, const double* colors,
                           const double* normals, int n_tri, const int* faces, const double* R, const double* t, const double* K4,
                           int width, int height, double clip_near, double clip_far, int shading, double ambient_weight,
                           const double* light_cam_pos, const double* bg_color, void* workspace, size_t workspace_bytes, float* depth,
                           int* tri_id, float* rgb_f32, unsigned char* rgb_u8, const tex_params* tp) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, render_shape_ok(n_pose, n_vert, n_tri, width, height), PP_ERR_SHAPE,
               "%s: need 1..65535 poses, vertices, triangles, a 1..16384 image and n_pose * n_tri * 4 < 2^31", what);
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
  PP_CHECK_ARG(ctx, clip_near >= 0.0 && clip_far >= clip_near, PP_ERR_ARG, "%s: need 0 <= clip_near <= clip_far", what);
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
  rattr* attr = nullptr;
  const size_t need = render_rgbd_layout(n_pose, n_vert, n_tri, width, height, (char*)workspace, &w, &attr);
  PP_CHECK_ARG(ctx, workspace_bytes >= need, PP_ERR_ARG, "%s: workspace of %zu bytes, need %zu", what, workspace_bytes, need);
  const int tiles_x = (width + RT - 1) / RT, n_tiles = tiles_x * ((height + RT - 1) / RT);
  const size_t nb = (size_t)n_pose * n_tiles;
  hipMemsetAsync(w.counts, 0, nb * sizeof(int), ctx->stream);
  hipMemsetAsync(w.big_n, 0, (size_t)n_pose * sizeof(int), ctx->stream);
  const dim3 vg((n_vert + 255) / 256, n_pose);
  hipLaunchKernelGGL(render_vertex_kernel, vg, dim3(256), 0, ctx->stream, n_vert, verts, R, t, K4, w.vtx);
  if (rgb) hipLaunchKernelGGL(render_attr_kernel, vg, dim3(256), 0, ctx->stream, n_vert, verts, normals, R, t, prm, attr);
  const dim3 tg((n_tri + 255) / 256, n_pose);
  hipLaunchKernelGGL(render_bin_kernel, tg, dim3(256), 0, ctx->stream, 0, n_vert, n_tri, faces, (const rvtx*)w.vtx, width, height,
                     tiles_x, n_tiles, w.counts, w.cursor, w.list, w.big_n, w.big);
  hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, (int)nb, (const int*)w.counts, w.offsets, w.cursor);
  hipLaunchKernelGGL(render_bin_kernel, tg, dim3(256), 0, ctx->stream, 1, n_vert, n_tri, faces, (const rvtx*)w.vtx, width, height,
                     tiles_x, n_tiles, w.counts, w.cursor, w.list, w.big_n, w.big);
  if (tp && rgb) {
    hipLaunchKernelGGL(render_rgbd_tex_raster_kernel, dim3(n_tiles, n_pose), dim3(RASTER_THREADS), 0, ctx->stream, n_vert, faces,
                       (const rvtx*)w.vtx, n_tri, width, height, tiles_x, n_tiles, (const int*)w.offsets, (const int*)w.list,
                       (const int*)w.big_n, (const int*)w.big, clip_near, clip_far, (const rattr*)attr, colors, prm, depth, tri_id, rgb_f32,
                       rgb_u8, *tp);
  } else {  // (without a colour output the shading tail is not reached: the untextured kernel serves both entry points)
    hipLaunchKernelGGL(render_rgbd_raster_kernel, dim3(n_tiles, n_pose), dim3(RASTER_THREADS), 0, ctx->stream, n_vert, faces,
                       (const rvtx*)w.vtx, n_tri, width, height, tiles_x, n_tiles, (const int*)w.offsets, (const int*)w.list,
                       (const int*)w.big_n, (const int*)w.big, clip_near, clip_far, (const rattr*)attr, colors, prm, depth, tri_id, rgb_f32,
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

// ---- VSD ----------------------------------------------------------------------------------------------------------------

// depth_im_to_dist_im (pose_error.py:43-61) at one pixel: || ((c - cx) d / fx, (r - cy) d / fy, d) ||, summed x, y, z in order
__device__ __forceinline__ double dist_px(float d, int r, int c, double cx, double cy, double rfx, double rfy) {
  const double dd = (double)d;
  const double X = (((double)c - cx) * dd) * rfx;
  const double Y = (((double)r - cy) * dd) * rfy;
  return sqrt((X * X + Y * Y) + dd * dd);
}

// estimate_visib_mask (pose_error.py:15-29): both valid and float32(d_model) - float32(d_test) <= delta (in float32)
__device__ __forceinline__ bool visib(double d_test, double d_model, float delta) {
  return d_test > 0.0 && d_model > 0.0 && ((float)d_model - (float)d_test) <= delta;
}

__device__ void block_reduce3(double c, int inter, int uni, double* rd, int* ri, int* ru) {
  const int tid = threadIdx.x;
  rd[tid] = c;
  ri[tid] = inter;
  ru[tid] = uni;
  __syncthreads();
  for (int s = VSD_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      rd[tid] += rd[tid + s];
      ri[tid] += ri[tid + s];
      ru[tid] += ru[tid + s];
    }
    __syncthreads();
  }
}

// grid (blocks of VSD_BLOCK pixels, problems): per block the cost sum over the intersection, |inter| and |union|
__global__ void __launch_bounds__(VSD_THREADS)
vsd_partial_kernel(int width, int hw, const float* __restrict__ depth_test, long long test_stride, const float* __restrict__ depth_est,
                   const float* __restrict__ depth_gt, const double* __restrict__ K4, float delta, double tau, int cost_type,
                   double* __restrict__ part_cost, int* __restrict__ part_cnt) {
  __shared__ double rd[VSD_THREADS];
  __shared__ int ri[VSD_THREADS], ru[VSD_THREADS];
  const int prob = blockIdx.y;
  const double* k = K4 + 4 * prob;
  const double cx = k[2], cy = k[3], rfx = 1.0 / k[0], rfy = 1.0 / k[1], rtau = 1.0 / tau;
  const float* dt = depth_test + (size_t)prob * test_stride;
  const float* de = depth_est + (size_t)prob * hw;
  const float* dg = depth_gt + (size_t)prob * hw;
  double cost = 0.0;
  int inter = 0, uni = 0;
  for (int j = 0; j < VSD_PER_THREAD; ++j) {
    const int p = blockIdx.x * VSD_BLOCK + j * VSD_THREADS + threadIdx.x;
    if (p >= hw) break;
    const int r = p / width, c = p - r * width;
    const double t_ = dist_px(dt[p], r, c, cx, cy, rfx, rfy);
    const double e_ = dist_px(de[p], r, c, cx, cy, rfx, rfy);
    const double g_ = dist_px(dg[p], r, c, cx, cy, rfx, rfy);
    const bool vg = visib(t_, g_, delta);
    const bool ve = visib(t_, e_, delta) || (vg && e_ > 0.0);
    if (vg && ve) {
      ++inter;
      const double d = fabs(g_ - e_);
      if (cost_type == 0) {
        cost += d >= tau ? 1.0 : 0.0;
      } else {
        const double q = d * rtau;
        cost += q > 1.0 ? 1.0 : q;
      }
    }
    uni += (vg || ve) ? 1 : 0;
  }
  block_reduce3(cost, inter, uni, rd, ri, ru);
  if (threadIdx.x == 0) {
    const size_t o = (size_t)prob * gridDim.x + blockIdx.x;
    part_cost[o] = rd[0];
    part_cnt[2 * o] = ri[0];
    part_cnt[2 * o + 1] = ru[0];
  }
}

__global__ void vsd_final_kernel(int n, int nblk, const double* __restrict__ part_cost, const int* __restrict__ part_cnt,
                                 double* __restrict__ e, long long* __restrict__ inter_out, long long* __restrict__ union_out) {
  const int prob = blockIdx.x * blockDim.x + threadIdx.x;
  if (prob >= n) return;
  double cost = 0.0;
  long long inter = 0, uni = 0;
  for (int b = 0; b < nblk; ++b) {
    const size_t o = (size_t)prob * nblk + b;
    cost += part_cost[o];
    inter += part_cnt[2 * o];
    uni += part_cnt[2 * o + 1];
  }
  e[prob] = uni > 0 ? (cost + (double)(uni - inter)) / (double)uni : 1.0;
  if (inter_out) inter_out[prob] = inter;
  if (union_out) union_out[prob] = uni;
}

extern "C" size_t pp_vsd_workspace_bytes(int n, int width, int height) {
  if (n <= 0 || width <= 0 || height <= 0) return 0;
  const size_t nblk = ((size_t)width * height + VSD_BLOCK - 1) / VSD_BLOCK;
  return pp_align256((size_t)n * nblk * sizeof(double)) + (size_t)n * nblk * 2 * sizeof(int);
}

extern "C" int pp_vsd_f64(pp_ctx* ctx, int n, int width, int height, const float* depth_test, long long test_stride,
                          const float* depth_est, const float* depth_gt, const double* K4, double delta, double tau, int cost_type,
                          void* workspace, double* e, long long* inter, long long* uni) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n > 0 && n <= 65535 && width > 0 && height > 0 && (long long)width * height <= 0x7FFFFFFFLL, PP_ERR_SHAPE,
               "pp_vsd_f64: need 1..65535 problems and a non-empty image");
  PP_CHECK_ARG(ctx, depth_test && depth_est && depth_gt && K4 && workspace && e, PP_ERR_ARG, "pp_vsd_f64: null argument");
  PP_CHECK_ARG(ctx, test_stride == 0 || test_stride == (long long)width * height, PP_ERR_ARG,
               "pp_vsd_f64: test_stride must be 0 (one shared scene depth) or width * height");
  PP_CHECK_ARG(ctx, cost_type == 0 || cost_type == 1, PP_ERR_ARG, "pp_vsd_f64: cost_type must be 0 (step) or 1 (tlinear)");
  PP_CHECK_ARG(ctx, tau > 0.0, PP_ERR_ARG, "pp_vsd_f64: tau must be positive");
  const int hw = width * height, nblk = (hw + VSD_BLOCK - 1) / VSD_BLOCK;
  double* part_cost = (double*)workspace;
  int* part_cnt = (int*)((char*)workspace + pp_align256((size_t)n * nblk * sizeof(double)));
  hipLaunchKernelGGL(vsd_partial_kernel, dim3(nblk, n), dim3(VSD_THREADS), 0, ctx->stream, width, hw, depth_test, test_stride,
                     depth_est, depth_gt, K4, (float)delta, tau, cost_type, part_cost, part_cnt);
  hipLaunchKernelGGL(vsd_final_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, n, nblk, (const double*)part_cost,
                     (const int*)part_cnt, e, inter, uni);
  PP_CHECK_LAUNCH(ctx, "pp_vsd_f64");
  return PP_OK;
}

// ---- VSD over a tolerance range (BOP's AR_VSD) ----------------------------------------------------------------------------
// One pass over the pixels for up to VSD_MAX_TAU misalignment tolerances: a pixel's three distances, both visibility masks
// and |d_gt - d_est| are computed once and serve every tau.  Same blocks, per-thread order and halving tree as
// vsd_partial_kernel, so a column of e carries the bits pp_vsd_f64 gives at that tau.
#define VSD_MAX_TAU 16

struct vsd_taus {
  double tau[VSD_MAX_TAU];  // strictly increasing; entries past n_tau are not read
};

// BOP 2019 (bop_toolkit's estimate_visib_mask with visib_mode 'bop19'; parity with bop_toolkit unpinned): a rendered pixel
// without a sensor value counts as visible
__device__ __forceinline__ bool visib_bop19(double d_test, double d_model, float delta) {
  return d_model > 0.0 && (((float)d_model - (float)d_test) <= delta || d_test == 0.0);
}

struct vsd_px {
  bool vg, ve, gt;  // the two visibility masks, d_gt > 0
  double d;         // |d_gt - d_est|
};

// pixel p of one problem; depths of 0 (also what a pixel past the image is loaded as) are in no mask
__device__ __forceinline__ vsd_px vsd_pixel(float dt, float de, float dg, int p, int width, double cx, double cy, double rfx,
                                            double rfy, float delta, int visib_mode) {
  const int r = p / width, c = p - r * width;
  const double t_ = dist_px(dt, r, c, cx, cy, rfx, rfy);
  const double e_ = dist_px(de, r, c, cx, cy, rfx, rfy);
  const double g_ = dist_px(dg, r, c, cx, cy, rfx, rfy);
  vsd_px o;
  o.vg = visib_mode ? visib_bop19(t_, g_, delta) : visib(t_, g_, delta);
  o.ve = (visib_mode ? visib_bop19(t_, e_, delta) : visib(t_, e_, delta)) || (o.vg && e_ > 0.0);
  o.gt = g_ > 0.0;
  o.d = fabs(g_ - e_);
  return o;
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (blocks of VSD_BLOCK pixels, problems).  COST 0 ('step'): integer arithmetic -- taus increase, so a pixel of the
// intersection adds one to a single LDS bin (the number of taus <= its d) and cost_t is the count of the bins above t.
// COST 1 ('tlinear'): n_tau float64 sums per thread, all reduced by one halving tree (its order per tau is block_reduce3's).
// part_cost [problem][block][n_tau] (step: the exact count as a double), part_cnt [problem][block][4] = |inter|, |union|,
// |visib_gt|, |d_gt > 0|.
template <int COST>
__global__ void __launch_bounds__(VSD_THREADS)
vsd_multi_partial_kernel(int width, int hw, const float* __restrict__ depth_test, long long test_stride,
                         const float* __restrict__ depth_est, const float* __restrict__ depth_gt, const double* __restrict__ K4,
                         float delta, int n_tau, vsd_taus taus, int visib_mode, double* __restrict__ part_cost,
                         int* __restrict__ part_cnt) {
  __shared__ double red[COST == 1 ? VSD_MAX_TAU * VSD_THREADS : 1];
  __shared__ int bins[VSD_MAX_TAU + 1];
  __shared__ int cnt[4];
  const int tid = threadIdx.x, prob = blockIdx.y;
  const double* k = K4 + 4 * prob;
  const double cx = k[2], cy = k[3], rfx = 1.0 / k[0], rfy = 1.0 / k[1];
  const float* dt = depth_test + (size_t)prob * test_stride;
  const float* de = depth_est + (size_t)prob * hw;
  const float* dg = depth_gt + (size_t)prob * hw;
  if (tid <= VSD_MAX_TAU) bins[tid] = 0;
  if (tid < 4) cnt[tid] = 0;
  __syncthreads();
  const int base = blockIdx.x * VSD_BLOCK, left = hw - base;  // base < hw: base + an offset below `left` cannot overflow
  float ft[VSD_PER_THREAD], fe[VSD_PER_THREAD], fg[VSD_PER_THREAD];
#pragma unroll
  for (int j = 0; j < VSD_PER_THREAD; ++j) {
    const int off = j * VSD_THREADS + tid;
    const bool in = off < left;
    ft[j] = in ? dt[base + off] : 0.0f;
    fe[j] = in ? de[base + off] : 0.0f;
    fg[j] = in ? dg[base + off] : 0.0f;
  }
  double cost[COST == 1 ? VSD_MAX_TAU : 1];
  double rtau[COST == 1 ? VSD_MAX_TAU : 1];
  if constexpr (COST == 1) {
#pragma unroll
    for (int t = 0; t < VSD_MAX_TAU; ++t) {
      cost[t] = 0.0;
      rtau[t] = t < n_tau ? 1.0 / taus.tau[t] : 0.0;
    }
  }
  int inter = 0, uni = 0, n_vg = 0, n_gt = 0;
#pragma unroll
  for (int j = 0; j < VSD_PER_THREAD; ++j) {
    const vsd_px px = vsd_pixel(ft[j], fe[j], fg[j], base + (j * VSD_THREADS + tid < left ? j * VSD_THREADS + tid : 0), width, cx, cy,
                                rfx, rfy, delta, visib_mode);
    if (px.vg && px.ve) {
      ++inter;
      if constexpr (COST == 0) {
        int b = 0;
#pragma unroll
        for (int t = 0; t < VSD_MAX_TAU; ++t) b += (t < n_tau && px.d >= taus.tau[t]) ? 1 : 0;
        if (b > 0) atomicAdd(&bins[b], 1);
      } else {
#pragma unroll
        for (int t = 0; t < VSD_MAX_TAU; ++t) {
          const double q = px.d * rtau[t];
          cost[t] += q > 1.0 ? 1.0 : q;
        }
      }
    }
    uni += (px.vg || px.ve) ? 1 : 0;
    n_vg += px.vg ? 1 : 0;
    n_gt += px.gt ? 1 : 0;
  }
  inter = wave_sum(inter);
  uni = wave_sum(uni);
  n_vg = wave_sum(n_vg);
  n_gt = wave_sum(n_gt);
  if ((tid & 63) == 0) {
    atomicAdd(&cnt[0], inter);
    atomicAdd(&cnt[1], uni);
    atomicAdd(&cnt[2], n_vg);
    atomicAdd(&cnt[3], n_gt);
  }
  if constexpr (COST == 1) {
#pragma unroll
    for (int t = 0; t < VSD_MAX_TAU; ++t)
      if (t < n_tau) red[t * VSD_THREADS + tid] = cost[t];
  }
  __syncthreads();
  if constexpr (COST == 1) {
    for (int s = VSD_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s)
        for (int t = 0; t < n_tau; ++t) red[t * VSD_THREADS + tid] += red[t * VSD_THREADS + tid + s];
      __syncthreads();
    }
  }
  const size_t o = (size_t)prob * gridDim.x + blockIdx.x;
  if (tid < n_tau) {
    if constexpr (COST == 0) {
      int c = 0;
      for (int b = tid + 1; b <= n_tau; ++b) c += bins[b];
      part_cost[o * n_tau + tid] = (double)c;
    } else {
      part_cost[o * n_tau + tid] = red[tid * VSD_THREADS];
    }
  }
  if (tid < 4) part_cnt[4 * o + tid] = cnt[tid];
}

// one thread per (problem, tau): the blocks' partials in block order
__global__ void vsd_multi_final_kernel(int n, int nblk, int n_tau, const double* __restrict__ part_cost, const int* __restrict__ part_cnt,
                                       double* __restrict__ e, long long* __restrict__ inter_out, long long* __restrict__ union_out,
                                       long long* __restrict__ visib_gt_out, long long* __restrict__ px_gt_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * n_tau) return;
  const int prob = i / n_tau, t = i - prob * n_tau;
  double cost = 0.0;
  long long inter = 0, uni = 0, n_vg = 0, n_gt = 0;
  for (int b = 0; b < nblk; ++b) {
    const size_t o = (size_t)prob * nblk + b;
    cost += part_cost[o * n_tau + t];
    inter += part_cnt[4 * o];
    uni += part_cnt[4 * o + 1];
    n_vg += part_cnt[4 * o + 2];
    n_gt += part_cnt[4 * o + 3];
  }
  e[i] = uni > 0 ? (cost + (double)(uni - inter)) / (double)uni : 1.0;
  if (t != 0) return;
  if (inter_out) inter_out[prob] = inter;
  if (union_out) union_out[prob] = uni;
  if (visib_gt_out) visib_gt_out[prob] = n_vg;
  if (px_gt_out) px_gt_out[prob] = n_gt;
}

extern "C" size_t pp_vsd_multi_workspace_bytes(int n, int width, int height, int n_tau) {
  if (n <= 0 || width <= 0 || height <= 0 || n_tau <= 0 || n_tau > VSD_MAX_TAU) return 0;
  const size_t nblk = ((size_t)width * height + VSD_BLOCK - 1) / VSD_BLOCK;
  return pp_align256((size_t)n * nblk * n_tau * sizeof(double)) + (size_t)n * nblk * 4 * sizeof(int);
}

extern "C" int pp_vsd_multi_f64(pp_ctx* ctx, int n, int width, int height, const float* depth_test, long long test_stride,
                                const float* depth_est, const float* depth_gt, const double* K4, double delta, int n_tau,
                                const double* taus, int cost_type, int visib_mode, void* workspace, double* e, long long* inter,
                                long long* uni, long long* visib_gt, long long* px_gt) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n > 0 && n <= 65535 && width > 0 && height > 0 && (long long)width * height <= 0x7FFFFFFFLL, PP_ERR_SHAPE,
               "pp_vsd_multi_f64: need 1..65535 problems and a non-empty image");
  PP_CHECK_ARG(ctx, n_tau >= 1 && n_tau <= VSD_MAX_TAU, PP_ERR_SHAPE, "pp_vsd_multi_f64: need 1..%d taus, got %d", VSD_MAX_TAU, n_tau);
  PP_CHECK_ARG(ctx, depth_test && depth_est && depth_gt && K4 && taus && workspace && e, PP_ERR_ARG, "pp_vsd_multi_f64: null argument");
  PP_CHECK_ARG(ctx, test_stride == 0 || test_stride == (long long)width * height, PP_ERR_ARG,
               "pp_vsd_multi_f64: test_stride must be 0 (one shared scene depth) or width * height");
  PP_CHECK_ARG(ctx, cost_type == 0 || cost_type == 1, PP_ERR_ARG, "pp_vsd_multi_f64: cost_type must be 0 (step) or 1 (tlinear)");
  PP_CHECK_ARG(ctx, visib_mode == 0 || visib_mode == 1, PP_ERR_ARG, "pp_vsd_multi_f64: visib_mode must be 0 (bop18) or 1 (bop19)");
  vsd_taus tv;
  for (int t = 0; t < VSD_MAX_TAU; ++t) {
    tv.tau[t] = t < n_tau ? taus[t] : 0.0;
    // (written so that a NaN is refused too)
    PP_CHECK_ARG(ctx, t >= n_tau || (taus[t] > 0.0 && (t == 0 || taus[t] > taus[t - 1])), PP_ERR_ARG,
                 "pp_vsd_multi_f64: taus must be positive and strictly increasing (tau[%d] = %g)", t, t < n_tau ? taus[t] : 0.0);
  }
  const int hw = width * height, nblk = (hw + VSD_BLOCK - 1) / VSD_BLOCK;
  double* part_cost = (double*)workspace;
  int* part_cnt = (int*)((char*)workspace + pp_align256((size_t)n * nblk * n_tau * sizeof(double)));
  auto partial = cost_type == 0 ? vsd_multi_partial_kernel<0> : vsd_multi_partial_kernel<1>;
  hipLaunchKernelGGL(partial, dim3(nblk, n), dim3(VSD_THREADS), 0, ctx->stream, width, hw, depth_test, test_stride, depth_est,
                     depth_gt, K4, (float)delta, n_tau, tv, visib_mode, part_cost, part_cnt);
  const int total = n * n_tau;
  hipLaunchKernelGGL(vsd_multi_final_kernel, dim3((total + 63) / 64), dim3(64), 0, ctx->stream, n, nblk, n_tau,
                     (const double*)part_cost, (const int*)part_cnt, e, inter, uni, visib_gt, px_gt);
  PP_CHECK_LAUNCH(ctx, "pp_vsd_multi_f64");
  return PP_OK;
}

// ---- scene ground truth from rendered instances (masks, boxes, visibility) -------------------------------------------------
// What bop_toolkit's calc_gt_masks / calc_gt_info write beforehand and annotation_scripts/annotate_BOP.py:363-378, 420, 461-471
// reads back (mask_visib/*.png, scene_gt_info.json), computed from the depth renders of a scene's instances.  Two passes:
//   1. scene:    per (scene, image pixel) the scene depth -- the given sensor depth or, without one, the nearest positive
//                instance depth -- then the id image: the scene's instances from the last to the first, the first one whose
//                'bop19' visibility mask holds the pixel wins, which is the later instance overwriting the earlier one
//                (annotate_BOP.py:373)
//   2. instance: per (instance, canvas pixel) the three pixel counts, both boxes and the optional masks; per-workgroup partials
//                (LDS integer atomics), then one wave per instance folds them
// A thread owns four pixels of a row whose image column is a multiple of 4: depths come in as one 16-byte load and bytes go out
// as one packed 4-byte store where the address allows, element by element otherwise.  Integer counts, minima and maxima only:
// the same bits whatever order the atomics run in.
#define SGT_THREADS 256
#define SGT_PART 11  // n_all, n_valid, n_visib, then (x_min, x_max, y_min, y_max) of the object and of its visible mask

// row[c0 .. c0 + 3] of a row of w floats, 0 where the column is outside [0, w)
__device__ __forceinline__ void load4_f32(const float* __restrict__ row, int c0, int w, float (&v)[4]) {
  if (c0 >= 0 && c0 + 3 < w && (reinterpret_cast<uintptr_t>(row + c0) & 15u) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(row + c0);
    v[0] = q.x;
    v[1] = q.y;
    v[2] = q.z;
    v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (c0 + k >= 0 && c0 + k < w) ? row[c0 + k] : 0.0f;
  }
}

// the columns of v inside [0, w) to row[c0 .. c0 + 3]; c0 >= 0
__device__ __forceinline__ void store4_f32(float* __restrict__ row, int c0, int w, const float (&v)[4]) {
  if (c0 + 3 < w && (reinterpret_cast<uintptr_t>(row + c0) & 15u) == 0) {
    *reinterpret_cast<float4*>(row + c0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k < w) row[c0 + k] = v[k];
  }
}

__device__ __forceinline__ void store4_u8(unsigned char* __restrict__ row, int c0, int w, const unsigned char (&v)[4]) {
  if (c0 + 3 < w && (reinterpret_cast<uintptr_t>(row + c0) & 3u) == 0) {
    *reinterpret_cast<unsigned*>(row + c0) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k < w) row[c0 + k] = v[k];
  }
}

__device__ __forceinline__ int wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ int wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// the instances [i0, i1) of a scene; whatever the device copy of the offsets holds, the range stays inside the stack
__device__ __forceinline__ void scene_range(const int* __restrict__ scene_offsets, int scene, int n_inst, int* i0, int* i1) {
  *i0 = min(max(scene_offsets[scene], 0), n_inst);
  *i1 = min(max(scene_offsets[scene + 1], *i0), n_inst);
}

// grid (blocks of SGT_THREADS groups of 4 image pixels, scenes)
__global__ void __launch_bounds__(SGT_THREADS)
scene_gt_scene_kernel(int n_inst, int canvas_w, int canvas_h, int width, int height, int off_x, int off_y,
                      const float* __restrict__ stack, const int* __restrict__ scene_offsets, const float* __restrict__ depth_test,
                      long long test_stride, const double* __restrict__ K4, float delta, float* __restrict__ scene_depth,
                      unsigned char* __restrict__ id_image) {
  const int groups = (width + 3) / 4, gi = blockIdx.x * SGT_THREADS + threadIdx.x, scene = blockIdx.y;
  if (gi >= height * groups) return;
  const int r = gi / groups, c0 = (gi - r * groups) * 4;
  int i0, i1;
  scene_range(scene_offsets, scene, n_inst, &i0, &i1);
  const size_t cpx = (size_t)canvas_w * canvas_h, hw = (size_t)width * height;
  const float* win = stack + (size_t)(r + off_y) * canvas_w + off_x;  // row r of the window in instance 0's canvas
  float dt[4], dg[4];
  if (depth_test) {
    load4_f32(depth_test + (size_t)scene * test_stride + (size_t)r * width, c0, width, dt);
  } else {
    dt[0] = dt[1] = dt[2] = dt[3] = 0.0f;
    for (int i = i0; i < i1; ++i) {
      load4_f32(win + i * cpx, c0, width, dg);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (dg[k] > 0.0f && (dt[k] == 0.0f || dg[k] < dt[k])) dt[k] = dg[k];
    }
    store4_f32(scene_depth + scene * hw + (size_t)r * width, c0, width, dt);
  }
  unsigned char id[4] = {0, 0, 0, 0};
  int open = 0;  // bit k: pixel c0 + k is in the image and no instance has claimed it yet
#pragma unroll
  for (int k = 0; k < 4; ++k) open |= (c0 + k < width) ? 1 << k : 0;
  for (int i = i1 - 1; i >= i0 && open; --i) {
    load4_f32(win + i * cpx, c0, width, dg);
    const double* kk = K4 + 4 * (size_t)i;
    const double cx = kk[2], cy = kk[3], rfx = 1.0 / kk[0], rfy = 1.0 / kk[1];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!((open >> k) & 1) || !(dg[k] > 0.0f)) continue;
      const double t_ = dist_px(dt[k], r, c0 + k, cx, cy, rfx, rfy);
      const double g_ = dist_px(dg[k], r, c0 + k, cx, cy, rfx, rfy);
      if (visib_bop19(t_, g_, delta)) {
        id[k] = (unsigned char)(i - i0 + 1);
        open &= ~(1 << k);
      }
    }
  }
  store4_u8(id_image + scene * hw + (size_t)r * width, c0, width, id);
}

// grid (blocks of SGT_THREADS groups of 4 canvas pixels, instances).  A canvas row is cut into `groups` groups that start at
// canvas column 4 g - shift, shift = (4 - off_x % 4) % 4, so that a group's first image column is a multiple of 4.
// part [instance][block][SGT_PART]; box coordinates are image coordinates (canvas minus the window's offset).
__global__ void __launch_bounds__(SGT_THREADS)
scene_gt_inst_kernel(int n_scene, int canvas_w, int canvas_h, int width, int height, int off_x, int off_y, int shift, int groups,
                     const float* __restrict__ stack, const int* __restrict__ scene_offsets, const float* __restrict__ test,
                     long long test_stride, const double* __restrict__ K4, float delta, int* __restrict__ part,
                     unsigned char* __restrict__ mask_full, unsigned char* __restrict__ mask_visib) {
  __shared__ int acc[SGT_PART];
  const int tid = threadIdx.x, inst = blockIdx.y, gi = blockIdx.x * SGT_THREADS + tid;
  if (tid < SGT_PART) acc[tid] = tid < 3 ? 0 : (((tid - 3) & 1) ? INT_MIN : INT_MAX);
  __syncthreads();
  int n_all = 0, n_valid = 0, n_vis = 0;
  int ox0 = INT_MAX, ox1 = INT_MIN, oy0 = INT_MAX, oy1 = INT_MIN, vx0 = INT_MAX, vx1 = INT_MIN, vy0 = INT_MAX, vy1 = INT_MIN;
  if (gi < canvas_h * groups) {
    const int R = gi / groups, C0 = (gi - R * groups) * 4 - shift, r = R - off_y, c0 = C0 - off_x;  // c0 is a multiple of 4
    const bool row_in = r >= 0 && r < height;
    const size_t hw = (size_t)width * height;
    float dg[4], dt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    load4_f32(stack + (size_t)inst * canvas_w * canvas_h + (size_t)R * canvas_w, C0, canvas_w, dg);
    if (row_in) {
      int lo = 0, hi = n_scene;  // scene_offsets[lo] <= inst < scene_offsets[hi]; lo stays in [0, n_scene)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (scene_offsets[mid] <= inst) lo = mid; else hi = mid;
      }
      load4_f32(test + (size_t)lo * test_stride + (size_t)r * width, c0, width, dt);
    }
    const double* kk = K4 + 4 * (size_t)inst;
    const double cx = kk[2], cy = kk[3], rfx = 1.0 / kk[0], rfy = 1.0 / kk[1];
    unsigned char mf[4], mv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + k;
      const bool gt = dg[k] > 0.0f;
      bool vis = false;
      if (gt) {
        ++n_all;
        ox0 = min(ox0, c);
        ox1 = max(ox1, c);
        oy0 = min(oy0, r);
        oy1 = max(oy1, r);
        if (row_in && c >= 0 && c < width) {
          n_valid += dt[k] > 0.0f ? 1 : 0;
          vis = visib_bop19(dist_px(dt[k], r, c, cx, cy, rfx, rfy), dist_px(dg[k], r, c, cx, cy, rfx, rfy), delta);
        }
      }
      if (vis) {
        ++n_vis;
        vx0 = min(vx0, c);
        vx1 = max(vx1, c);
        vy0 = min(vy0, r);
        vy1 = max(vy1, r);
      }
      mf[k] = gt ? 255 : 0;
      mv[k] = vis ? 255 : 0;
    }
    if (row_in && c0 >= 0 && c0 < width) {
      if (mask_full) store4_u8(mask_full + inst * hw + (size_t)r * width, c0, width, mf);
      if (mask_visib) store4_u8(mask_visib + inst * hw + (size_t)r * width, c0, width, mv);
    }
  }
  const int sums[3] = {wave_sum(n_all), wave_sum(n_valid), wave_sum(n_vis)};
  const int mins[4] = {wave_min(ox0), wave_min(oy0), wave_min(vx0), wave_min(vy0)};
  const int maxs[4] = {wave_max(ox1), wave_max(oy1), wave_max(vx1), wave_max(vy1)};
  if ((tid & 63) == 0) {
    for (int k = 0; k < 3; ++k) atomicAdd(&acc[k], sums[k]);
    // acc: obj x_min, x_max, y_min, y_max, visible x_min, x_max, y_min, y_max
    for (int k = 0; k < 4; ++k) {
      atomicMin(&acc[3 + 2 * k], mins[k]);
      atomicMax(&acc[4 + 2 * k], maxs[k]);
    }
  }
  __syncthreads();
  if (tid < SGT_PART) part[((size_t)inst * gridDim.x + blockIdx.x) * SGT_PART + tid] = acc[tid];
}

// one wave per instance: the blocks' partials -> px_count [3], bbox_obj (x, y, w, h), bbox_visib (x, y, w, h)
__global__ void __launch_bounds__(64)
scene_gt_final_kernel(int nblk, const int* __restrict__ part, long long* __restrict__ px_count, int* __restrict__ bbox_obj,
                      int* __restrict__ bbox_visib) {
  const int inst = blockIdx.x, lane = threadIdx.x;
  int v[SGT_PART];
#pragma unroll
  for (int k = 0; k < SGT_PART; ++k) v[k] = k < 3 ? 0 : (((k - 3) & 1) ? INT_MIN : INT_MAX);
  for (int b = lane; b < nblk; b += 64) {
    const int* p = part + ((size_t)inst * nblk + b) * SGT_PART;
#pragma unroll
    for (int k = 0; k < SGT_PART; ++k) v[k] = k < 3 ? v[k] + p[k] : (((k - 3) & 1) ? max(v[k], p[k]) : min(v[k], p[k]));
  }
#pragma unroll
  for (int k = 0; k < SGT_PART; ++k) v[k] = k < 3 ? wave_sum(v[k]) : (((k - 3) & 1) ? wave_max(v[k]) : wave_min(v[k]));
  if (lane != 0) return;
  for (int k = 0; k < 3; ++k) px_count[3 * (size_t)inst + k] = v[k];
  const bool seen = v[2] > 0;  // calc_gt_info: both boxes are (-1, -1, -1, -1) when nothing is visible
  for (int b = 0; b < 2; ++b) {
    int* box = (b ? bbox_visib : bbox_obj) + 4 * (size_t)inst;
    const int* m = v + 3 + 4 * b;  // x_min, x_max, y_min, y_max
    box[0] = seen ? m[0] : -1;
    box[1] = seen ? m[2] : -1;
    box[2] = seen ? m[1] - m[0] : -1;
    box[3] = seen ? m[3] - m[2] : -1;
  }
}

#define SGT_MAX_PER_SCENE 255  // the id image is uint8 and 0 is the background

static bool scene_gt_shape_ok(int n_inst, int canvas_w, int canvas_h) {
  return n_inst > 0 && n_inst <= 65535 && canvas_w > 0 && canvas_h > 0 && canvas_w <= 16384 && canvas_h <= 16384;
}

// workgroups of scene_gt_inst_kernel per instance, at the window offset that needs the most groups per row
static size_t scene_gt_blocks(int canvas_w, int canvas_h, int shift) {
  const size_t groups = ((size_t)canvas_w + shift + 3) / 4;
  return (groups * canvas_h + SGT_THREADS - 1) / SGT_THREADS;
}

extern "C" size_t pp_scene_gt_workspace_bytes(int n_inst, int canvas_w, int canvas_h) {
  if (!scene_gt_shape_ok(n_inst, canvas_w, canvas_h)) return 0;
  return (size_t)n_inst * scene_gt_blocks(canvas_w, canvas_h, 3) * SGT_PART * sizeof(int);
}

extern "C" int pp_scene_gt_info(pp_ctx* ctx, int n_inst, int n_scene, const int* scene_offsets_host, const int* scene_offsets_dev,
                                int canvas_w, int canvas_h, int width, int height, int off_x, int off_y, const float* depth_stack,
                                const double* K4, const float* depth_test, long long test_stride, double delta, void* workspace,
                                size_t workspace_bytes, float* scene_depth, unsigned char* id_image, long long* px_count,
                                int* bbox_obj, int* bbox_visib, unsigned char* mask_full, unsigned char* mask_visib) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, scene_gt_shape_ok(n_inst, canvas_w, canvas_h) && n_scene > 0 && n_scene <= 65535, PP_ERR_SHAPE,
               "pp_scene_gt_info: need 1..65535 instances, 1..65535 scenes and a 1..16384 canvas");
  PP_CHECK_ARG(ctx, width > 0 && height > 0 && off_x >= 0 && off_y >= 0 && off_x <= canvas_w - width && off_y <= canvas_h - height,
               PP_ERR_SHAPE, "pp_scene_gt_info: the %d x %d window at (%d, %d) must lie inside the %d x %d canvas", width, height,
               off_x, off_y, canvas_w, canvas_h);
  PP_CHECK_ARG(ctx, scene_offsets_host && scene_offsets_dev && depth_stack && K4 && workspace && id_image && px_count && bbox_obj &&
                        bbox_visib, PP_ERR_ARG, "pp_scene_gt_info: null argument");
  PP_CHECK_ARG(ctx, (depth_test != nullptr) != (scene_depth != nullptr), PP_ERR_ARG,
               "pp_scene_gt_info: give depth_test, or scene_depth for the depth composed from the instances, not both");
  PP_CHECK_ARG(ctx, !depth_test || test_stride == 0 || test_stride == (long long)width * height, PP_ERR_ARG,
               "pp_scene_gt_info: test_stride must be 0 (one depth image shared by the scenes) or width * height");
  PP_CHECK_ARG(ctx, delta >= 0.0, PP_ERR_ARG, "pp_scene_gt_info: delta must not be negative");  // (a NaN is refused too)
  PP_CHECK_ARG(ctx, scene_offsets_host[0] == 0 && scene_offsets_host[n_scene] == n_inst, PP_ERR_ARG,
               "pp_scene_gt_info: scene_offsets must run from 0 to n_inst");
  for (int s = 0; s < n_scene; ++s) {
    const int m = scene_offsets_host[s + 1] - scene_offsets_host[s];
    PP_CHECK_ARG(ctx, m >= 0, PP_ERR_ARG, "pp_scene_gt_info: scene_offsets must not decrease (scene %d)", s);
    PP_CHECK_ARG(ctx, m <= SGT_MAX_PER_SCENE, PP_ERR_SHAPE, "pp_scene_gt_info: scene %d has %d instances, the uint8 id image holds %d",
                 s, m, SGT_MAX_PER_SCENE);
  }
  const int shift = (4 - off_x % 4) % 4, groups = (canvas_w + shift + 3) / 4;
  const size_t nblk = scene_gt_blocks(canvas_w, canvas_h, shift), need = (size_t)n_inst * nblk * SGT_PART * sizeof(int);
  PP_CHECK_ARG(ctx, workspace_bytes >= need, PP_ERR_ARG, "pp_scene_gt_info: workspace of %zu bytes, need %zu", workspace_bytes, need);
  const size_t hw = (size_t)width * height;
  const int scene_blocks = (int)((((size_t)width + 3) / 4 * height + SGT_THREADS - 1) / SGT_THREADS);
  hipLaunchKernelGGL(scene_gt_scene_kernel, dim3(scene_blocks, n_scene), dim3(SGT_THREADS), 0, ctx->stream, n_inst, canvas_w, canvas_h,
                     width, height, off_x, off_y, depth_stack, scene_offsets_dev, depth_test, test_stride, K4, (float)delta, scene_depth,
                     id_image);
  const float* test = depth_test ? depth_test : scene_depth;
  hipLaunchKernelGGL(scene_gt_inst_kernel, dim3((unsigned)nblk, n_inst), dim3(SGT_THREADS), 0, ctx->stream, n_scene, canvas_w, canvas_h,
                     width, height, off_x, off_y, shift, groups, depth_stack, scene_offsets_dev, test,
                     depth_test ? test_stride : (long long)hw, K4, (float)delta, (int*)workspace, mask_full, mask_visib);
  hipLaunchKernelGGL(scene_gt_final_kernel, dim3(n_inst), dim3(64), 0, ctx->stream, (int)nblk, (const int*)workspace, px_count, bbox_obj,
                     bbox_visib);
  PP_CHECK_LAUNCH(ctx, "pp_scene_gt_info");
  return PP_OK;
}

// ---- a scene's image from its instances' colour renders ---------------------------------------------------------------------
// Per (scene, pixel): id k > 0 of pp_scene_gt_info's id image selects the colour of instance scene_offsets[scene] + k - 1 of
// the uint8 stack (pp_render_rgbd outputs in scene order), anything else the background -- the scene's image or a constant.
// Inputs are RGB; the output is RGB or, reversed per pixel, BGR.  A thread owns four pixels of a row (one packed load of the
// ids, three packed stores where the addresses allow).  Bytes are selected, never computed.
__global__ void __launch_bounds__(SGT_THREADS)
scene_compose_kernel(int n_inst, int width, int height, const int* __restrict__ scene_offsets, const unsigned char* __restrict__ id_image,
                     const unsigned char* __restrict__ colors, const unsigned char* __restrict__ background, unsigned bg_const, int bgr,
                     unsigned char* __restrict__ out) {
  const int groups = (width + 3) / 4, gi = blockIdx.x * SGT_THREADS + threadIdx.x, scene = blockIdx.y;
  if (gi >= height * groups) return;
  const int r = gi / groups, c0 = (gi - r * groups) * 4;
  int i0, i1;
  scene_range(scene_offsets, scene, n_inst, &i0, &i1);
  const size_t hw = (size_t)width * height, p0 = (size_t)r * width + c0;
  const unsigned char* ids = id_image + scene * hw + p0;
  const bool whole = c0 + 3 < width;
  unsigned packed = 0;
  if (whole && (reinterpret_cast<uintptr_t>(ids) & 3u) == 0) {
    packed = *reinterpret_cast<const unsigned*>(ids);
  } else {
    for (int k = 0; k < 4; ++k)
      if (c0 + k < width) packed |= (unsigned)ids[k] << (8 * k);
  }
  unsigned char v[12];
  for (int k = 0; k < 4; ++k) {
    const int id = (int)((packed >> (8 * k)) & 255u);
    const unsigned char* src = nullptr;
    if (c0 + k < width) {
      if (id > 0 && id <= i1 - i0)
        src = colors + ((size_t)(i0 + id - 1) * hw + p0 + k) * 3;
      else if (background)
        src = background + (scene * hw + p0 + k) * 3;
    }
    for (int j = 0; j < 3; ++j) {
      const int jj = bgr ? 2 - j : j;
      v[3 * k + j] = src ? src[jj] : (unsigned char)((bg_const >> (8 * jj)) & 255u);
    }
  }
  unsigned char* o = out + (scene * hw + p0) * 3;
  if (whole && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
    for (int j = 0; j < 3; ++j)
      reinterpret_cast<unsigned*>(o)[j] = (unsigned)v[4 * j] | ((unsigned)v[4 * j + 1] << 8) | ((unsigned)v[4 * j + 2] << 16) | ((unsigned)v[4 * j + 3] << 24);
  } else {
    for (int k = 0; k < 12; ++k)
      if (c0 + k / 3 < width) o[k] = v[k];
  }
}

extern "C" int pp_scene_compose_u8(pp_ctx* ctx, int n_inst, int n_scene, const int* scene_offsets_host, const int* scene_offsets_dev,
                                   int width, int height, const unsigned char* id_image, const unsigned char* colors,
                                   const unsigned char* background, const unsigned char* bg_const, int channel_order,
                                   unsigned char* out) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, scene_gt_shape_ok(n_inst, width, height) && n_scene > 0 && n_scene <= 65535, PP_ERR_SHAPE,
               "pp_scene_compose_u8: need 1..65535 instances, 1..65535 scenes and a 1..16384 image");
  PP_CHECK_ARG(ctx, scene_offsets_host && scene_offsets_dev && id_image && colors && out && (background || bg_const), PP_ERR_ARG,
               "pp_scene_compose_u8: null argument (give a background image or a constant)");
  PP_CHECK_ARG(ctx, channel_order == 0 || channel_order == 1, PP_ERR_ARG, "pp_scene_compose_u8: channel_order must be 0 (RGB) or 1 (BGR)");
  PP_CHECK_ARG(ctx, scene_offsets_host[0] == 0 && scene_offsets_host[n_scene] == n_inst, PP_ERR_ARG,
               "pp_scene_compose_u8: scene_offsets must run from 0 to n_inst");
  for (int s = 0; s < n_scene; ++s) {
    const int m = scene_offsets_host[s + 1] - scene_offsets_host[s];
    PP_CHECK_ARG(ctx, m >= 0, PP_ERR_ARG, "pp_scene_compose_u8: scene_offsets must not decrease (scene %d)", s);
    PP_CHECK_ARG(ctx, m <= SGT_MAX_PER_SCENE, PP_ERR_SHAPE, "pp_scene_compose_u8: scene %d has %d instances, the uint8 id image holds %d",
                 s, m, SGT_MAX_PER_SCENE);
  }
  const unsigned bg = background ? 0u : (unsigned)bg_const[0] | ((unsigned)bg_const[1] << 8) | ((unsigned)bg_const[2] << 16);
  const int blocks = (int)((((size_t)width + 3) / 4 * height + SGT_THREADS - 1) / SGT_THREADS);
  hipLaunchKernelGGL(scene_compose_kernel, dim3(blocks, n_scene), dim3(SGT_THREADS), 0, ctx->stream, n_inst, width, height,
                     scene_offsets_dev, id_image, colors, background, bg, channel_order, out);
  PP_CHECK_LAUNCH(ctx, "pp_scene_compose_u8");
  return PP_OK;
}

// ---- the textured raster kernel of the colour renderer (declared there) ---------------------------------------------------------
#define RASTER_KERNEL render_rgbd_tex_raster_kernel
#define RASTER_TEX true
#define RASTER_TP_PARAM , tex_params tp
#define RASTER_TP tp
#include "render_rgbd_raster.inc"
