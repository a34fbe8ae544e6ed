// Evaluation overlays: an ordered list of primitives and an id layer painted over a batch of uint8 images in ONE launch
// (pp_draw_overlay_u8; the rule is written out in include/pyrapose_hip.h and restated in tests/overlay_np.py).  What the reference
// draws with cv2.rectangle / cv2.putText (utils/visualization.py), twelve cv2.line calls per 3-D box and cv2.circle per voted
// corner (linemod_eval.py:537-620) and draw_axis (annotation_scripts/misc.py:8).  The coverage rules are the project's own --
// exact integer distance tests, no Bresenham stepping, no anti-aliasing, no font in the kernel -- so parity with OpenCV is not
// pinned; the output is a pure function of the inputs: integers only, no atomics, no floating point.
//
//   tiles     one workgroup of 256 threads per 32 x 32 tile and image; a thread owns 4 horizontally adjacent pixels, which stay
//             in registers (packed c0 | c1 << 8 | c2 << 16) from the one read to the one write: `out` may be `images`.
//   id layer  the tile's ids with a halo of 4 pixels as bytes in LDS, the palette beside them; fill, then the inner contour by a
//             search of the (2 width + 1)^2 window, clipped to the image.
//   list      the image's records in chunks of 256: thread i loads record base + i, checks it ONCE, and tests its bounding box
//             (grown by ceil(t / 2) for a segment, by dilate for a glyph) against the tile.  The records that reach the tile
//             are compacted into LDS IN LIST ORDER: a 64-lane ballot and the popcount of the lanes below within a wave, the four
//             waves' counts through LDS.  Then every pixel walks the compacted list in order.  The list holds a chunk, so it
//             cannot overflow.  Two barriers per chunk: counts visible, list visible; the next chunk's counts are written after
//             the second, when nobody reads the old ones, and its list after its own first, when nobody walks the old one.
// Every tile reads its image's whole list (no binning pass, no workspace): profiles/bench_overlay.json, DESIGN.md 7b.
#include "pp_internal.h"

#define OV_TILE 32
#define OV_THREADS 256
#define OV_PX 4               // pixels per thread
#define OV_CHUNK 256          // records per pass = capacity of the LDS list
#define OV_HALO 4             // = the widest outline
#define OV_IDW (OV_TILE + 2 * OV_HALO)
#define OV_MAX_SIDE 8192
#define OV_MAX_COORD 8192
#define OV_MAX_THICK 64
#define OV_MAX_SCALE 4
#define OV_MAX_DILATE 2
#define OV_MAX_PRIMS (1 << 24)
#define OV_MAX_GRID_Z 65535

#define OV_SEGMENT 0
#define OV_GLYPH 1
#define OV_FILL_RECT 2

// p <- (A c + (255 - A) p + 127) / 255 per channel; the dividend is at most 255 * 255 + 127 < 2^16
__device__ __forceinline__ unsigned int ov_paint(unsigned int p, unsigned int colour) {
  const unsigned int A = colour >> 24, nA = 255u - A;
  unsigned int r = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const unsigned int c = (colour >> (8 * ch)) & 255u, v = (p >> (8 * ch)) & 255u;
    r |= ((A * c + nA * v + 127u) / 255u) << (8 * ch);
  }
  return r;
}

__device__ __forceinline__ bool ov_coord_ok(int v) { return v >= -OV_MAX_COORD && v <= OV_MAX_COORD; }

// The one check of a record: its kind and fields, and its bounding box against the tile [tx0, tx1] x [ty0, ty1] (already cut to
// the image).  -> the box inside the tile in tile coordinates, one byte each (x0 | y0 << 8 | x1 << 16 | y1 << 24), or -1.
__device__ __forceinline__ int ov_record_box(const int* r, int tx0, int ty0, int tx1, int ty1) {
  long long bx0, by0, bx1, by1;  // (a FILL_RECT's corners are any int32: 64 bits for the glyph's and segment's sums is simply safe)
  const int a0 = r[1], a1 = r[2], a2 = r[3], a3 = r[4], size = r[5];
  if (r[0] == OV_SEGMENT) {
    if (size < 1 || size > OV_MAX_THICK || !ov_coord_ok(a0) || !ov_coord_ok(a1) || !ov_coord_ok(a2) || !ov_coord_ok(a3)) return -1;
    const int g = (size + 1) / 2;
    bx0 = min(a0, a2) - g, bx1 = max(a0, a2) + g, by0 = min(a1, a3) - g, by1 = max(a1, a3) + g;
  } else if (r[0] == OV_GLYPH) {
    const int scale = size & 255, dilate = (size >> 8) & 255;
    if ((size >> 16) != 0 || scale < 1 || scale > OV_MAX_SCALE || dilate > OV_MAX_DILATE || !ov_coord_ok(a0) || !ov_coord_ok(a1)) return -1;
    bx0 = a0 - dilate, bx1 = a0 + 8 * scale - 1 + dilate, by0 = a1 - dilate, by1 = a1 + 8 * scale - 1 + dilate;
  } else if (r[0] == OV_FILL_RECT) {
    bx0 = min(a0, a2), bx1 = max(a0, a2), by0 = min(a1, a3), by1 = max(a1, a3);
  } else {
    return -1;
  }
  if (bx0 < tx0) bx0 = tx0;
  if (by0 < ty0) by0 = ty0;
  if (bx1 > tx1) bx1 = tx1;
  if (by1 > ty1) by1 = ty1;
  if (bx0 > bx1 || by0 > by1) return -1;
  return (int)(bx0 - tx0) | (int)(by0 - ty0) << 8 | (int)(bx1 - tx0) << 16 | (int)(by1 - ty0) << 24;
}

// Pixel (x, y) against the segment P0 P1 of thickness t: squared distance to the segment <= t^2 / 4, exactly.
// 0 <= x, y < 8192 and |P0|, |P1| <= 8192 per coordinate, so |d| = |P1 - P0| <= 2^14 and |w| = |P - P0| < 2^14 per coordinate:
//   s = w.d, L2 = d.d, |w|^2, |P - P1|^2  <=  2 * 2^14 * 2^14 = 2^29                        (int32)
//   |cross(d, w)| = |dx wy - dy wx|       <=  2^29,  so  4 cross^2 <= 2^60 < 2^61           (int64)
//   t^2 L2                                <=  2^12 * 2^29 = 2^41                            (int64)
__device__ __forceinline__ bool ov_on_segment(int x, int y, int x0, int y0, int x1, int y1, int t) {
  const int dx = x1 - x0, dy = y1 - y0, wx = x - x0, wy = y - y0;
  const int L2 = dx * dx + dy * dy, s = wx * dx + wy * dy, t2 = t * t;
  if (s <= 0) return wx * wx + wy * wy <= (t2 >> 2);  // 4 |w|^2 <= t^2 without the 2^31 of 4 |w|^2 (also P0 == P1: the disc of diameter t)
  if (s >= L2) {
    const int ux = x - x1, uy = y - y1;
    return ux * ux + uy * uy <= (t2 >> 2);
  }
  const long long cr = (long long)dx * wy - (long long)dy * wx;
  return 4 * cr * cr <= (long long)t2 * L2;
}

// Pixel (x, y) against the 8 x 8 bitmap at (x0, y0): some position within chessboard distance `dilate` lies in a set cell.  The
// positions x - dilate .. x + dilate fall into the columns c_lo .. c_hi (floor division by scale; a negative offset is left of
// the cell whatever its quotient), likewise the rows: covered iff the bitmap has a bit inside that block of cells.
__device__ __forceinline__ bool ov_on_glyph(int x, int y, int x0, int y0, unsigned long long bits, int scale, int dilate) {
  const int lo_x = x - dilate - x0, hi_x = x + dilate - x0, lo_y = y - dilate - y0, hi_y = y + dilate - y0;
  if (hi_x < 0 || hi_y < 0) return false;
  const int c_lo = lo_x < 0 ? 0 : lo_x / scale, c_hi = min(hi_x / scale, 7);
  const int r_lo = lo_y < 0 ? 0 : lo_y / scale, r_hi = min(hi_y / scale, 7);
  if (c_lo > c_hi || r_lo > r_hi) return false;
  const unsigned long long cols = ((1ull << (c_hi + 1)) - (1ull << c_lo)) * 0x0101010101010101ull;
  const unsigned long long upto = r_hi == 7 ? ~0ull : (1ull << (8 * (r_hi + 1))) - 1ull;
  const unsigned long long rows = upto & ~((1ull << (8 * r_lo)) - 1ull);
  return (bits & cols & rows) != 0ull;
}

__global__ void __launch_bounds__(OV_THREADS)
ov_draw_kernel(int B, int H, int W, const unsigned char* images, unsigned char* out, const int* __restrict__ prims,
               const int* __restrict__ image_offsets, int n_total, const unsigned char* __restrict__ ids, const int* __restrict__ palette,
               int id_mode, int width) {
  __shared__ int s_list[OV_CHUNK][8];
  __shared__ int s_wave[OV_THREADS / 64];
  __shared__ int s_palette[256];
  __shared__ unsigned char s_id[OV_IDW * OV_IDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx0 = blockIdx.x * OV_TILE, ty0 = blockIdx.y * OV_TILE;
  const int tx1 = min(tx0 + OV_TILE, W) - 1, ty1 = min(ty0 + OV_TILE, H) - 1;
  const int lx = (tid % (OV_TILE / OV_PX)) * OV_PX, ly = tid / (OV_TILE / OV_PX);
  const int x = tx0 + lx, y = ty0 + ly;
  const int n_px = y < H ? min(max(W - x, 0), OV_PX) : 0;  // this thread's pixels inside the image
  if (ids && id_mode) s_palette[tid] = palette[tid];
  for (int img = blockIdx.z; img < B; img += gridDim.z) {
    const size_t px0 = ((size_t)img * H + (size_t)(n_px ? y : 0)) * W + (size_t)(n_px ? x : 0);
    const unsigned char* src = images + 3 * px0;
    unsigned char* dst = out + 3 * px0;
    // four pixels are twelve bytes: three dwords where they are all there and the address allows it
    const bool wide = n_px == OV_PX && (((size_t)src | (size_t)dst) & 3) == 0;
    unsigned int p[OV_PX] = {0u, 0u, 0u, 0u};
    if (wide) {
      const unsigned int d0 = ((const unsigned int*)src)[0], d1 = ((const unsigned int*)src)[1], d2 = ((const unsigned int*)src)[2];
      p[0] = d0 & 0xffffffu;
      p[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
      p[2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
      p[3] = d2 >> 8;
    } else {
      for (int k = 0; k < n_px; ++k) p[k] = src[3 * k] | src[3 * k + 1] << 8 | src[3 * k + 2] << 16;
    }

    if (ids && id_mode) {
      const unsigned char* id_img = ids + (size_t)img * H * W;
      for (int i = tid; i < OV_IDW * OV_IDW; i += OV_THREADS) {
        const int gx = tx0 - OV_HALO + i % OV_IDW, gy = ty0 - OV_HALO + i / OV_IDW;
        s_id[i] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? id_img[(size_t)gy * W + gx] : 0;
      }
      __syncthreads();
      for (int k = 0; k < n_px; ++k) {
        const int cx = lx + k + OV_HALO, cy = ly + OV_HALO;
        const unsigned char L = s_id[cy * OV_IDW + cx];
        if (L == 0) continue;
        const unsigned int colour = (unsigned int)s_palette[L];
        if (id_mode & 1) p[k] = ov_paint(p[k], colour);
        if (id_mode & 2) {
          // neighbours outside the image are ignored: the window is cut to it (it stays inside the halo, width <= OV_HALO)
          const int dx0 = -min(width, x + k), dx1 = min(width, W - 1 - (x + k)), dy0 = -min(width, y), dy1 = min(width, H - 1 - y);
          bool edge = false;
          for (int dy = dy0; dy <= dy1 && !edge; ++dy)
            for (int dx = dx0; dx <= dx1; ++dx) edge = edge || s_id[(cy + dy) * OV_IDW + cx + dx] != L;
          if (edge) p[k] = ov_paint(p[k], colour);
        }
      }
    }

    const int begin = min(max(image_offsets[img], 0), n_total), end = min(max(image_offsets[img + 1], begin), n_total);
    for (int base = begin; base < end; base += OV_CHUNK) {
      int r[8], box = -1;
      if (base + tid < end) {
        const int* rec = prims + (size_t)(base + tid) * 8;
#pragma unroll
        for (int f = 0; f < 8; ++f) r[f] = rec[f];
        box = ov_record_box(r, tx0, ty0, tx1, ty1);
      }
      const unsigned long long hits = __ballot(box >= 0);
      if (lane == 0) s_wave[wave] = __popcll(hits);
      __syncthreads();
      int slot = __popcll(hits & ((1ull << lane) - 1ull)), n_hit = 0;
#pragma unroll
      for (int w = 0; w < OV_THREADS / 64; ++w) {
        const int c = s_wave[w];
        slot += w < wave ? c : 0;
        n_hit += c;
      }
      if (box >= 0) {
#pragma unroll
        for (int f = 0; f < 7; ++f) s_list[slot][f] = r[f];
        s_list[slot][7] = box;
      }
      __syncthreads();
      for (int j = 0; j < n_hit; ++j) {
        const int box_j = s_list[j][7];
        const int bx0 = box_j & 255, by0 = (box_j >> 8) & 255, bx1 = (box_j >> 16) & 255, by1 = (box_j >> 24) & 255;
        if (ly < by0 || ly > by1 || lx + OV_PX - 1 < bx0 || lx > bx1) continue;
        const int kind = s_list[j][0], a0 = s_list[j][1], a1 = s_list[j][2], a2 = s_list[j][3], a3 = s_list[j][4], size = s_list[j][5];
        const unsigned int colour = (unsigned int)s_list[j][6];
        const unsigned long long bits = (unsigned long long)(unsigned int)a2 | (unsigned long long)(unsigned int)a3 << 32;
#pragma unroll
        for (int k = 0; k < OV_PX; ++k) {
          if (lx + k < bx0 || lx + k > bx1) continue;  // (the box lies inside the image: so does this pixel)
          bool on = true;
          if (kind == OV_SEGMENT) on = ov_on_segment(x + k, y, a0, a1, a2, a3, size);
          else if (kind == OV_GLYPH) on = ov_on_glyph(x + k, y, a0, a1, bits, size & 255, size >> 8);
          if (on) p[k] = ov_paint(p[k], colour);
        }
      }
    }

    if (wide) {
      ((unsigned int*)dst)[0] = p[0] | p[1] << 24;
      ((unsigned int*)dst)[1] = p[1] >> 8 | p[2] << 16;
      ((unsigned int*)dst)[2] = p[2] >> 16 | p[3] << 8;
    } else {
      for (int k = 0; k < n_px; ++k) {
        dst[3 * k] = (unsigned char)p[k];
        dst[3 * k + 1] = (unsigned char)(p[k] >> 8);
        dst[3 * k + 2] = (unsigned char)(p[k] >> 16);
      }
    }
    __syncthreads();  // the next image's id tile and list go where this one's were read
  }
}

extern "C" int pp_draw_overlay_u8(pp_ctx* ctx, int B, int H, int W, const unsigned char* images, unsigned char* out, const int* prims,
                                  const int* image_offsets, int n_total, const unsigned char* ids, const int* palette, int id_mode,
                                  int outline_width) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, B >= 1 && H >= 1 && W >= 1 && H <= OV_MAX_SIDE && W <= OV_MAX_SIDE, PP_ERR_ARG,
               "pp_draw_overlay_u8: need B >= 1 images of 1..%d x 1..%d pixels, got %d of %d x %d", OV_MAX_SIDE, OV_MAX_SIDE, B, H, W);
  PP_CHECK_ARG(ctx, n_total >= 0 && n_total <= OV_MAX_PRIMS, PP_ERR_ARG, "pp_draw_overlay_u8: n_total %d, need 0..%d", n_total, OV_MAX_PRIMS);
  PP_CHECK_ARG(ctx, images && out && image_offsets && (prims || n_total == 0), PP_ERR_ARG, "pp_draw_overlay_u8: null argument");
  PP_CHECK_ARG(ctx, id_mode >= 0 && id_mode <= 3, PP_ERR_ARG, "pp_draw_overlay_u8: id_mode %d, need bit 0 (fill) | bit 1 (outline)", id_mode);
  PP_CHECK_ARG(ctx, !ids || palette, PP_ERR_ARG, "pp_draw_overlay_u8: ids without a palette");
  PP_CHECK_ARG(ctx, !(ids && (id_mode & 2)) || (outline_width >= 1 && outline_width <= OV_HALO), PP_ERR_ARG,
               "pp_draw_overlay_u8: outline_width %d, need 1..%d", outline_width, OV_HALO);
  const dim3 grid((W + OV_TILE - 1) / OV_TILE, (H + OV_TILE - 1) / OV_TILE, B < OV_MAX_GRID_Z ? B : OV_MAX_GRID_Z);
  hipLaunchKernelGGL(ov_draw_kernel, grid, dim3(OV_THREADS), 0, ctx->stream, B, H, W, images, out, prims, image_offsets, n_total, ids,
                     palette, id_mode, outline_width);
  PP_CHECK_LAUNCH(ctx, "pp_draw_overlay_u8");
  return PP_OK;
}
