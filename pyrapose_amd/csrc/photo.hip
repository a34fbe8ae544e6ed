// Photometric augmentation of uint8 BGR batches on the device: the APPLY half of the reference's imgaug chain
//   utils/image.py:154-191  apply_transform: iaa.Sequential([blur, colour, brightness, contrast], random_order=True)
// The SAMPLING half (a few random numbers per image) stays on the host: pyrapose_amd/utils/photometric.py draws one ordered op
// list per image and builds every table; this file applies the lists.  imgaug and OpenCV are not installed here and the
// reference has no fixture: parity with them is UNPINNED.  What is pinned, byte for byte, is tests/photo_np.py, a numpy
// restatement of the definitions below.  They use float32 + - * / in the stated order (compiled with -ffp-contract=off; hipcc's
// float32 divide is correctly rounded), rintf (ties to even) and a clamp to [0,255]; no transcendental function is evaluated on
// the device -- every curve arrives as a table.
//
// CONTRACT: after every op the image is rounded to uint8 and the next op reads those bytes, however the launches are fused.
// Pixels are (b, g, r) bytes; u8(f) = (unsigned char)min(max(rintf(f), 0), 255).
//
// Per-pixel ops
//   LUT      out_c = T[c][v_c]                              T: 3 x 256 bytes at off0
//   GRAY     luma = (0.299f*r + 0.587f*g) + 0.114f*b;  out_c = u8(v_c + f0 * (luma - v_c))                  f0 = alpha
//   HUESAT   dh = (int)f0, ds = (int)f1; dh == 0 && ds == 0: identity (the uint8 HSV round trip below is not).  Otherwise
//              V = max(b,g,r); m = min(b,g,r); d = V - m                       (floats holding integers)
//              S = V > 0 ? (int)rintf((255.f * d) / V) : 0
//              h = d == 0 ? 0 : V == r ? (30.f*(g - b)) / d : V == g ? 60.f + (30.f*(b - r)) / d : 120.f + (30.f*(r - g)) / d
//              if (h < 0) h = h + 180.f;  Hq = (int)rintf(h);  if (Hq >= 180) Hq -= 180         (H in [0,180): 2 degrees a unit)
//              H' = (Hq + dh) mod 180 (wraps, in [0,180));  S' = min(max(S + ds, 0), 255) (saturates);  V stays
//              s = (float)S' / 255.f;  hh = (float)H' / 30.f;  i = (int)floorf(hh);  f = hh - (float)i
//              p = V*(1.f - s);  q = V*(1.f - s*f);  t = V*(1.f - s*(1.f - f))
//              (r,g,b) = i==0 (V,t,p)  1 (q,V,p)  2 (p,V,t)  3 (p,q,V)  4 (t,p,V)  5 (V,p,q);  out = u8 of each
//   BLEND    out_c = u8(a * T1[c][v_c] + (1.f - a) * T2[c][v_c])      T1, T2: 2 x 3 x 256 bytes at off0
//            a: bilinear from the mask at off1 = {int32 mh, int32 mw, float32 m[mh][mw]}, mh, mw <= 32 (the host reads and checks
//            mh, mw and hands them to the kernel with the op record).  For pixel (x, y):
//              u = ((float)x + 0.5f) * ((float)mw / (float)W) - 0.5f, clamped to [0, mw-1]; x0 = (int)floorf(u); fx = u - (float)x0;
//              x1 = min(x0+1, mw-1); the same for v, y0, fy, y1 with mh and H;
//              a = (m[y0][x0]*(1.f-fx) + m[y0][x1]*fx)*(1.f-fy) + (m[y1][x0]*(1.f-fx) + m[y1][x1]*fx)*fy
// Neighbourhood ops (per channel, k odd <= 7, r = k/2; (dy,dx) in row-major order from (-r,-r))
//   CONV      acc = 0; acc = acc + tap[dy][dx] * v(y+dy, x+dx); out = u8(acc)        taps: k x k float32 at off0; border reflect-101
//             (correlation, like cv2.filter2D)
//   MEDIAN    the exact median of the k*k bytes, k in {3,5,7}; border replicate
//   BILATERAL w = space[dy][dx] * colour[|db|+|dg|+|dr|] against the centre pixel; num_c = num_c + w * v_c; den = den + w;
//             out_c = den > 0 ? u8(num_c / den) : centre.  space: k x k float32 at off0 (0 outside the circle), colour: 766
//             float32 at off1; border reflect-101
//   The device always walks a 7 x 7 window with the k x k table centred in zeros: a zero tap adds +0 to a sum, which changes no
//   bit of it (the one exception, a sum that is -0, rounds to the same byte).
//
// KERNEL SHAPE: one kernel, photo_stage_kernel; one workgroup of 256 lanes per (64 x 16 tile, image), 4 pixels = 12 bytes per
// lane.  A STAGE is an optional neighbourhood op followed by a run of up to 4 per-pixel ops applied in registers (the run rides
// as the epilogue of the neighbourhood launch); a run without a neighbourhood op in front reads its 12 bytes straight from
// global memory.  The stage record of the image is a kernel argument, so the op kinds are workgroup-uniform scalars.  The
// neighbourhood ops stage the tile with a 3-row / 4-pixel halo in LDS as dwords (4 pixels on the sides keep the rows
// dword-aligned in global memory: interior tiles load dwords, tiles that touch the left / right border gather bytes), rows 80
// dwords apart: a lane reads dwords 3*tx .. 3*tx+8 of its 7 rows, and with ds_read_b32 banks (a/4) mod 32 the 16 tx of one
// row fill 16 banks and the row below (80 = 16 mod 32) the other 16.  The window then lives in 63 registers and every byte is
// a shift of a compile-time position.  Tables (LUTs, blend masks, taps, the bilateral tables) are copied to LDS first.
// The batch goes through in launches indexed by stage slot: slot s applies every image's s-th stage; images ping-pong between
// dst and a scratch batch such that their last stage writes dst, and an image without a stage in the slot is skipped.
// No host synchronisation anywhere; no kernel here uses scratch (-Rpass-analysis=kernel-resource-usage).
#include <vector>

#include "pp_internal.h"

#define PH_TW 64               // tile: 64 x 16 pixels
#define PH_TH 16
#define PH_ROWS (PH_TH + 6)    // + 3 rows above and below
#define PH_ROW_DW 54           // (4 + 64 + 4) pixels * 3 bytes / 4
#define PH_ROW_STRIDE 80       // dwords between tile rows in LDS (16 mod 32: see above)
#define PH_MAX_RUN 4           // per-pixel ops per stage
#define PH_CHUNK 32            // images per launch (the stage records travel as kernel arguments: 4 KiB limit)
#define PH_MAX_IMG 64
#define PH_MAX_OPS 32          // ops per image
#define PH_MASK_MAX 32
#define PH_SLOT_BYTES (1536 + PH_MASK_MAX * PH_MASK_MAX * 4)  // LDS per per-pixel op: two LUTs + a blend mask

struct PhPx { int kind, off0, off1; float f0, f1; };
struct PhStage {
  int nb_kind;  // -1: no stage in this slot; PP_PHOTO_NONE (0): per-pixel run only; CONV / MEDIAN / BILATERAL
  int k, off0, off1;
  int n_px;
  int in_sel, out_sel;  // 0 = src, 1 = dst, 2 = scratch
  PhPx px[PH_MAX_RUN];
};
struct PhSlot { PhStage s[PH_CHUNK]; };

__device__ __forceinline__ int ph_reflect101(int i, int n) {
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}
__device__ __forceinline__ int ph_clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
__device__ __forceinline__ unsigned ph_u8(float f) {
  f = rintf(f);
  f = f < 0.f ? 0.f : (f > 255.f ? 255.f : f);
  return (unsigned)f;
}

// byte `rb` (compile-time) of a window row held as 9 dwords
#define PH_WB(row, rb) ((w[row][(rb) >> 2] >> (((rb)&3) * 8)) & 255u)

template <int NB>
__global__ __launch_bounds__(256) void photo_stage_kernel(const PhSlot slot, int img0, int H, int W, const unsigned char* __restrict__ pool,
                                                          const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                          unsigned char* __restrict__ tmp) {
  __shared__ unsigned tile[PH_ROWS * PH_ROW_STRIDE];
  __shared__ unsigned tabs[PH_MAX_RUN * PH_SLOT_BYTES / 4];
  __shared__ float taps[49];
  __shared__ float ctab[768];

  const PhStage& st = slot.s[blockIdx.z];
  if (st.nb_kind != NB) return;  // (also the images without a stage in this slot: -1)
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int x0 = blockIdx.x * PH_TW, y0 = blockIdx.y * PH_TH;
  const size_t img_off = (size_t)(img0 + blockIdx.z) * H * W * 3;
  const unsigned char* in = (st.in_sel == 0 ? src : (st.in_sel == 1 ? dst : tmp)) + img_off;
  unsigned char* out = (st.out_sel == 1 ? dst : tmp) + img_off;
  // rows are dword-aligned in global memory when W is a multiple of 4 (image strides then are too) and the bases are
  const bool aligned = (W & 3) == 0 && ((((uintptr_t)src) | ((uintptr_t)dst) | ((uintptr_t)tmp)) & 3) == 0;

  // ---- tables into LDS
  for (int o = 0; o < st.n_px; ++o) {
    const PhPx& p = st.px[o];
    unsigned* t = tabs + o * (PH_SLOT_BYTES / 4);
    if (p.kind == PP_PHOTO_LUT || p.kind == PP_PHOTO_BLEND) {
      const int nd = p.kind == PP_PHOTO_LUT ? 192 : 384;
      const unsigned* g = (const unsigned*)(pool + p.off0);
      for (int i = tid; i < nd; i += 256) t[i] = g[i];
    }
    if (p.kind == PP_PHOTO_BLEND) {
      const int nm = (int)p.f0 * (int)p.f1;  // mask rows x columns as the host validated them (<= 32 x 32)
      const unsigned* g = (const unsigned*)(pool + p.off1 + 8);
      for (int i = tid; i < nm; i += 256) t[384 + i] = g[i];
    }
  }
  if (NB == PP_PHOTO_CONV || NB == PP_PHOTO_BILATERAL) {
    const float* g = (const float*)(pool + st.off0);
    const int k = st.k, o = (7 - k) / 2;
    if (tid < 49) {
      const int r = tid / 7 - o, c = tid % 7 - o;
      taps[tid] = (r >= 0 && r < k && c >= 0 && c < k) ? g[r * k + c] : 0.f;
    }
    if (NB == PP_PHOTO_BILATERAL) {
      const float* gc = (const float*)(pool + st.off1);
      for (int i = tid; i < 766; i += 256) ctab[i] = gc[i];
    }
  }

  unsigned v[4][3];
  const int px = x0 + tx * 4, py = y0 + ty;  // this lane's first pixel
  const bool row_ok = py < H;

  if constexpr (NB == PP_PHOTO_NONE) {
    if (row_ok && px < W) {
      const unsigned char* p = in + ((size_t)py * W + px) * 3;
      if (aligned && px + 4 <= W) {
        const unsigned* q = (const unsigned*)p;
        const unsigned d0 = q[0], d1 = q[1], d2 = q[2];
        v[0][0] = d0 & 255u; v[0][1] = (d0 >> 8) & 255u; v[0][2] = (d0 >> 16) & 255u;
        v[1][0] = d0 >> 24;  v[1][1] = d1 & 255u;        v[1][2] = (d1 >> 8) & 255u;
        v[2][0] = (d1 >> 16) & 255u; v[2][1] = d1 >> 24; v[2][2] = d2 & 255u;
        v[3][0] = (d2 >> 8) & 255u; v[3][1] = (d2 >> 16) & 255u; v[3][2] = d2 >> 24;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int c = 0; c < 3; ++c) v[j][c] = (px + j < W) ? p[j * 3 + c] : 0u;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[j][c] = 0u;
    }
    __syncthreads();  // the tables
  } else {
    // ---- the tile: rows y0-3 .. y0+18, pixels x0-4 .. x0+67, as dwords
    constexpr bool replicate = NB == PP_PHOTO_MEDIAN;
    const bool fast = aligned && x0 >= 4 && x0 + PH_TW + 4 <= W;
    for (int i = tid; i < PH_ROWS * PH_ROW_DW; i += 256) {
      const int row = i / PH_ROW_DW, q = i - row * PH_ROW_DW;
      const int yy = y0 - 3 + row;
      const int gy = replicate ? ph_clampi(yy, H) : ph_reflect101(yy, H);
      unsigned d;
      if (fast) {
        d = *(const unsigned*)(in + ((size_t)gy * W + (x0 - 4)) * 3 + 4 * q);
      } else {
        d = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int bi = 4 * q + b, pxl = bi / 3, c = bi - pxl * 3;
          const int xx = x0 - 4 + pxl;
          const int gx = replicate ? ph_clampi(xx, W) : ph_reflect101(xx, W);
          d |= (unsigned)in[((size_t)gy * W + gx) * 3 + c] << (8 * b);
        }
      }
      tile[row * PH_ROW_STRIDE + q] = d;
    }
    __syncthreads();
    unsigned w[7][9];
#pragma unroll
    for (int r = 0; r < 7; ++r)
#pragma unroll
      for (int q = 0; q < 9; ++q) w[r][q] = tile[(ty + r) * PH_ROW_STRIDE + tx * 3 + q];
    // output pixel j, offset (dy, dx), channel c  ->  window row dy + 3, byte (4 + j + dx) * 3 + c

    if constexpr (NB == PP_PHOTO_CONV) {
      float acc[4][3];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[j][c] = 0.f;
#pragma unroll
      for (int r = 0; r < 7; ++r)
#pragma unroll
        for (int dx = 0; dx < 7; ++dx) {
          const float t = taps[r * 7 + dx];
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[j][c] = acc[j][c] + t * (float)PH_WB(r, (1 + j + dx) * 3 + c);
        }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[j][c] = ph_u8(acc[j][c]);
    } else {
      // MEDIAN and BILATERAL keep one pixel's working set live at a time: the pixel loop is not unrolled, every pass works on
      // "pixel 0" of the window (compile-time byte positions) and then moves the window 3 bytes on; the three result bytes are
      // shifted into a 96-bit value
      unsigned r0 = 0, r1 = 0, r2 = 0;
#pragma unroll 1
      for (int j = 0; j < 4; ++j) {
        unsigned res;
        if constexpr (NB == PP_PHOTO_MEDIAN) {
          // bisection on the value: the median is the smallest m with #(x <= m) >= (k*k + 1) / 2
          const int rad = st.k >> 1, need = (st.k * st.k + 1) >> 1;
          int lo[3] = {0, 0, 0}, hi[3] = {255, 255, 255};
#pragma unroll 1
          for (int it = 0; it < 8; ++it) {
            // (keeps the 147 byte extractions inside the loop instead of in 147 registers across it)
#pragma unroll
            for (int r = 0; r < 7; ++r)
#pragma unroll
              for (int q = 0; q < 6; ++q) asm volatile("" : "+v"(w[r][q]));
            int cnt[3] = {0, 0, 0}, mid[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) mid[c] = (lo[c] + hi[c]) >> 1;
#pragma unroll
            for (int r = 0; r < 7; ++r)
#pragma unroll
              for (int dx = 0; dx < 7; ++dx) {
                const int ar = r < 3 ? 3 - r : r - 3, ax = dx < 3 ? 3 - dx : dx - 3;
                if (ar <= rad && ax <= rad) {  // (uniform)
#pragma unroll
                  for (int c = 0; c < 3; ++c) cnt[c] += ((int)PH_WB(r, (1 + dx) * 3 + c) <= mid[c]) ? 1 : 0;
                }
              }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              if (cnt[c] >= need) hi[c] = mid[c];
              else lo[c] = mid[c] + 1;
            }
          }
          res = (unsigned)lo[0] | ((unsigned)lo[1] << 8) | ((unsigned)lo[2] << 16);
        } else {  // PP_PHOTO_BILATERAL
          const int cb = (int)PH_WB(3, 12), cg = (int)PH_WB(3, 13), cr = (int)PH_WB(3, 14);
          float nb = 0.f, ng = 0.f, nr = 0.f, den = 0.f;
#pragma unroll
          for (int r = 0; r < 7; ++r)
#pragma unroll
            for (int dx = 0; dx < 7; ++dx) {
              const int b = (int)PH_WB(r, (1 + dx) * 3 + 0), g = (int)PH_WB(r, (1 + dx) * 3 + 1), rr = (int)PH_WB(r, (1 + dx) * 3 + 2);
              const int db = b - cb, dg = g - cg, dr = rr - cr;
              const float wgt = taps[r * 7 + dx] * ctab[(db < 0 ? -db : db) + (dg < 0 ? -dg : dg) + (dr < 0 ? -dr : dr)];
              nb = nb + wgt * (float)b;
              ng = ng + wgt * (float)g;
              nr = nr + wgt * (float)rr;
              den = den + wgt;
            }
          res = den > 0.f ? (ph_u8(nb / den) | (ph_u8(ng / den) << 8) | (ph_u8(nr / den) << 16)) : ((unsigned)cb | ((unsigned)cg << 8) | ((unsigned)cr << 16));
        }
        r0 = (r0 >> 24) | (r1 << 8);
        r1 = (r1 >> 24) | (r2 << 8);
        r2 = (r2 >> 24) | (res << 8);
#pragma unroll
        for (int r = 0; r < 7; ++r) {
#pragma unroll
          for (int q = 0; q < 8; ++q) w[r][q] = (w[r][q] >> 24) | (w[r][q + 1] << 8);
          w[r][8] >>= 24;
        }
      }
      v[0][0] = r0 & 255u; v[0][1] = (r0 >> 8) & 255u; v[0][2] = (r0 >> 16) & 255u;
      v[1][0] = r0 >> 24;  v[1][1] = r1 & 255u;        v[1][2] = (r1 >> 8) & 255u;
      v[2][0] = (r1 >> 16) & 255u; v[2][1] = r1 >> 24; v[2][2] = r2 & 255u;
      v[3][0] = (r2 >> 8) & 255u; v[3][1] = (r2 >> 16) & 255u; v[3][2] = r2 >> 24;
    }
  }

  // ---- the run of per-pixel ops, bytes in registers
  for (int o = 0; o < st.n_px; ++o) {
    const PhPx& p = st.px[o];
    const unsigned char* t8 = (const unsigned char*)(tabs + o * (PH_SLOT_BYTES / 4));
    if (p.kind == PP_PHOTO_LUT) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[j][c] = t8[c * 256 + v[j][c]];
    } else if (p.kind == PP_PHOTO_GRAY) {
      const float a = p.f0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float b = (float)v[j][0], g = (float)v[j][1], r = (float)v[j][2];
        const float luma = (0.299f * r + 0.587f * g) + 0.114f * b;
        v[j][0] = ph_u8(b + a * (luma - b));
        v[j][1] = ph_u8(g + a * (luma - g));
        v[j][2] = ph_u8(r + a * (luma - r));
      }
    } else if (p.kind == PP_PHOTO_HUESAT) {
      const int dh = (int)p.f0, ds = (int)p.f1;
      if (dh != 0 || ds != 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float b = (float)v[j][0], g = (float)v[j][1], r = (float)v[j][2];
          const float V = fmaxf(fmaxf(b, g), r), m = fminf(fminf(b, g), r), d = V - m;
          const int S = V > 0.f ? (int)rintf((255.f * d) / V) : 0;
          float h = d == 0.f ? 0.f : (V == r ? (30.f * (g - b)) / d : (V == g ? 60.f + (30.f * (b - r)) / d : 120.f + (30.f * (r - g)) / d));
          if (h < 0.f) h = h + 180.f;
          int Hq = (int)rintf(h);
          if (Hq >= 180) Hq -= 180;
          int H2 = (Hq + dh) % 180;
          if (H2 < 0) H2 += 180;
          int S2 = S + ds;
          S2 = S2 < 0 ? 0 : (S2 > 255 ? 255 : S2);
          const float s = (float)S2 / 255.f, hh = (float)H2 / 30.f;
          const int i = (int)floorf(hh);
          const float f = hh - (float)i;
          const float pp = V * (1.f - s), qq = V * (1.f - s * f), tt = V * (1.f - s * (1.f - f));
          float ro, go, bo;
          if (i == 0) { ro = V; go = tt; bo = pp; }
          else if (i == 1) { ro = qq; go = V; bo = pp; }
          else if (i == 2) { ro = pp; go = V; bo = tt; }
          else if (i == 3) { ro = pp; go = qq; bo = V; }
          else if (i == 4) { ro = tt; go = pp; bo = V; }
          else { ro = V; go = pp; bo = qq; }
          v[j][0] = ph_u8(bo); v[j][1] = ph_u8(go); v[j][2] = ph_u8(ro);
        }
      }
    } else if (p.kind == PP_PHOTO_BLEND) {
      const int mh = (int)p.f0, mw = (int)p.f1;
      const float* mk = (const float*)(t8 + 1536);
      float vv = ((float)py + 0.5f) * ((float)mh / (float)H) - 0.5f;
      vv = vv < 0.f ? 0.f : (vv > (float)(mh - 1) ? (float)(mh - 1) : vv);
      const int my0 = (int)floorf(vv), my1 = my0 + 1 < mh ? my0 + 1 : mh - 1;
      const float fy = vv - (float)my0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float u = ((float)(px + j) + 0.5f) * ((float)mw / (float)W) - 0.5f;
        u = u < 0.f ? 0.f : (u > (float)(mw - 1) ? (float)(mw - 1) : u);
        const int mx0 = (int)floorf(u), mx1 = mx0 + 1 < mw ? mx0 + 1 : mw - 1;
        const float fx = u - (float)mx0;
        const float a = (mk[my0 * mw + mx0] * (1.f - fx) + mk[my0 * mw + mx1] * fx) * (1.f - fy) +
                        (mk[my1 * mw + mx0] * (1.f - fx) + mk[my1 * mw + mx1] * fx) * fy;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          v[j][c] = ph_u8(a * (float)t8[c * 256 + v[j][c]] + (1.f - a) * (float)t8[768 + c * 256 + v[j][c]]);
      }
    }
  }

  // ---- 12 bytes per lane out
  if (row_ok && px < W) {
    unsigned char* p = out + ((size_t)py * W + px) * 3;
    if (aligned && px + 4 <= W) {
      uint3 d;
      d.x = v[0][0] | (v[0][1] << 8) | (v[0][2] << 16) | (v[1][0] << 24);
      d.y = v[1][1] | (v[1][2] << 8) | (v[2][0] << 16) | (v[2][1] << 24);
      d.z = v[2][2] | (v[3][0] << 8) | (v[3][1] << 16) | (v[3][2] << 24);
      *(uint3*)p = d;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (px + j < W) {
#pragma unroll
          for (int c = 0; c < 3; ++c) p[j * 3 + c] = (unsigned char)v[j][c];
        }
    }
  }
}

extern "C" size_t pp_photo_workspace_bytes(int n_img, int H, int W) {
  if (n_img <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)n_img * H * W * 3;
}

static int ph_in_pool(long long off, long long bytes, size_t pool_bytes) {
  return off >= 0 && (off & 3) == 0 && bytes >= 0 && (unsigned long long)(off + bytes) <= (unsigned long long)pool_bytes;
}

extern "C" int pp_photo_augment_u8(pp_ctx* ctx, int n_img, int H, int W, int channels, const int* op_offsets_host, const pp_photo_op* ops_host,
                                   const unsigned char* pool_host, size_t pool_bytes, const unsigned char* pool_dev, const unsigned char* src,
                                   unsigned char* dst, void* workspace, size_t workspace_bytes) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, channels == 3, PP_ERR_ARG, "pp_photo_augment_u8: 3 channels (BGR), got %d", channels);
  PP_CHECK_ARG(ctx, n_img > 0 && n_img <= PH_MAX_IMG && H >= 2 && W >= 2 && H < 32768 && W < 32768, PP_ERR_ARG,
               "pp_photo_augment_u8: 1..%d images of at least 2 x 2", PH_MAX_IMG);
  PP_CHECK_ARG(ctx, src && dst && src != dst && op_offsets_host && (pool_bytes == 0 || (pool_host && pool_dev && pp_is_aligned16(pool_dev))), PP_ERR_ARG, "pp_photo_augment_u8: null or aliased buffers");
  PP_CHECK_ARG(ctx, pool_bytes < (1u << 30) && op_offsets_host[0] == 0, PP_ERR_ARG, "pp_photo_augment_u8: op_offsets start at 0, pool under 1 GiB");
  // ---- validate every program and group it into stages, before anything is launched
  std::vector<PhStage> stage_buf((size_t)n_img * (PH_MAX_OPS + 1));
  PhStage(*stages)[PH_MAX_OPS + 1] = reinterpret_cast<PhStage(*)[PH_MAX_OPS + 1]>(stage_buf.data());
  int n_stages[PH_MAX_IMG];
  int max_stages = 0;
  for (int n = 0; n < n_img; ++n) {
    const int o0 = op_offsets_host[n], o1 = op_offsets_host[n + 1];
    PP_CHECK_ARG(ctx, o1 >= o0 && o1 - o0 <= PH_MAX_OPS && (o1 == o0 || ops_host), PP_ERR_ARG, "pp_photo_augment_u8: image %d: 0..%d ops", n, PH_MAX_OPS);
    int ns = 0;
    PhStage* cur = nullptr;
    for (int o = o0; o < o1; ++o) {
      const pp_photo_op& op = ops_host[o];
      int blend_hdr[2] = {0, 0};
      const bool nb = op.kind == PP_PHOTO_CONV || op.kind == PP_PHOTO_MEDIAN || op.kind == PP_PHOTO_BILATERAL;
      if (nb) {
        PP_CHECK_ARG(ctx, (op.k & 1) == 1 && op.k >= 1 && op.k <= 7, PP_ERR_ARG, "pp_photo_augment_u8: image %d op %d: k must be odd and <= 7, got %d", n, o - o0, op.k);
        PP_CHECK_ARG(ctx, op.kind != PP_PHOTO_MEDIAN || op.k >= 3, PP_ERR_ARG, "pp_photo_augment_u8: image %d op %d: median k is 3, 5 or 7", n, o - o0);
        if (op.kind != PP_PHOTO_MEDIAN)
          PP_CHECK_ARG(ctx, ph_in_pool(op.off0, (long long)op.k * op.k * 4, pool_bytes), PP_ERR_ARG, "pp_photo_augment_u8: image %d op %d: k x k table outside the pool", n, o - o0);
        if (op.kind == PP_PHOTO_BILATERAL)
          PP_CHECK_ARG(ctx, ph_in_pool(op.off1, 766 * 4, pool_bytes), PP_ERR_ARG, "pp_photo_augment_u8: image %d op %d: colour table outside the pool", n, o - o0);
        cur = &stages[n][ns++];
        memset(cur, 0, sizeof(*cur));
        cur->nb_kind = op.kind; cur->k = op.k; cur->off0 = op.off0; cur->off1 = op.off1;
        continue;
      }
      switch (op.kind) {
        case PP_PHOTO_LUT:
          PP_CHECK_ARG(ctx, ph_in_pool(op.off0, 768, pool_bytes), PP_ERR_ARG, "pp_photo_augment_u8: image %d op %d: LUT outside the pool", n, o - o0);
          break;
        case PP_PHOTO_GRAY:
          PP_CHECK_ARG(ctx, op.f0 >= 0.f && op.f0 <= 1.f, PP_ERR_ARG, "pp_photo_augment_u8: image %d op %d: alpha in [0,1]", n, o - o0);
          break;
        case PP_PHOTO_HUESAT:
          PP_CHECK_ARG(ctx, op.f0 == (float)(int)op.f0 && op.f1 == (float)(int)op.f1 && op.f0 >= -180.f && op.f0 <= 180.f && op.f1 >= -255.f && op.f1 <= 255.f,
                       PP_ERR_ARG, "pp_photo_augment_u8: image %d op %d: integer dh in [-180,180], ds in [-255,255]", n, o - o0);
          break;
        case PP_PHOTO_BLEND: {
          PP_CHECK_ARG(ctx, ph_in_pool(op.off0, 1536, pool_bytes) && ph_in_pool(op.off1, 8, pool_bytes), PP_ERR_ARG,
                       "pp_photo_augment_u8: image %d op %d: blend tables outside the pool", n, o - o0);
          int* hdr = blend_hdr;
          memcpy(hdr, pool_host + op.off1, 8);
          PP_CHECK_ARG(ctx, hdr[0] >= 1 && hdr[0] <= PH_MASK_MAX && hdr[1] >= 1 && hdr[1] <= PH_MASK_MAX && ph_in_pool(op.off1, 8 + (long long)hdr[0] * hdr[1] * 4, pool_bytes),
                       PP_ERR_ARG, "pp_photo_augment_u8: image %d op %d: blend mask of 1..%d x 1..%d inside the pool", n, o - o0, PH_MASK_MAX, PH_MASK_MAX);
          break;
        }
        default:
          return pp_fail(ctx, PP_ERR_ARG, "pp_photo_augment_u8: image %d op %d: unknown op kind %d", n, o - o0, op.kind);
      }
      if (!cur || cur->n_px == PH_MAX_RUN) {
        cur = &stages[n][ns++];
        memset(cur, 0, sizeof(*cur));
        cur->nb_kind = PP_PHOTO_NONE;
      }
      PhPx& p = cur->px[cur->n_px++];
      p.kind = op.kind; p.off0 = op.off0; p.off1 = op.off1; p.f0 = op.f0; p.f1 = op.f1;
      if (op.kind == PP_PHOTO_BLEND) { p.f0 = (float)blend_hdr[0]; p.f1 = (float)blend_hdr[1]; }  // the kernel never reads the header
    }
    if (ns == 0) {  // an empty program copies through
      memset(&stages[n][0], 0, sizeof(PhStage));
      stages[n][0].nb_kind = PP_PHOTO_NONE;
      ns = 1;
    }
    // ping-pong such that the last stage writes dst
    for (int s = 0; s < ns; ++s) {
      stages[n][s].out_sel = ((ns - 1 - s) & 1) ? 2 : 1;
      stages[n][s].in_sel = s == 0 ? 0 : stages[n][s - 1].out_sel;
    }
    n_stages[n] = ns;
    if (ns > max_stages) max_stages = ns;
  }
  PP_CHECK_ARG(ctx, workspace && pp_is_aligned16(workspace) && workspace_bytes >= pp_photo_workspace_bytes(n_img, H, W), PP_ERR_ARG,
               "pp_photo_augment_u8: workspace of pp_photo_workspace_bytes, 16-byte aligned");
  unsigned char* tmp = (unsigned char*)workspace;
  const dim3 block(256);
  for (int s = 0; s < max_stages; ++s)
    for (int i0 = 0; i0 < n_img; i0 += PH_CHUNK) {
      const int cnt = n_img - i0 < PH_CHUNK ? n_img - i0 : PH_CHUNK;
      PhSlot slot;
      bool any = false;
      for (int i = 0; i < PH_CHUNK; ++i) {
        if (i < cnt && s < n_stages[i0 + i]) { slot.s[i] = stages[i0 + i][s]; any = true; }
        else { memset(&slot.s[i], 0, sizeof(PhStage)); slot.s[i].nb_kind = -1; }
      }
      if (!any) continue;
      const dim3 grid((W + PH_TW - 1) / PH_TW, (H + PH_TH - 1) / PH_TH, cnt);
      // one instantiation per neighbourhood kind (each with its own register budget); a workgroup of another kind's image exits
      unsigned kinds = 0;
      for (int i = 0; i < cnt; ++i)
        if (slot.s[i].nb_kind >= 0) kinds |= 1u << slot.s[i].nb_kind;
      if (kinds & (1u << PP_PHOTO_NONE))
        hipLaunchKernelGGL(photo_stage_kernel<PP_PHOTO_NONE>, grid, block, 0, ctx->stream, slot, i0, H, W, pool_dev, src, dst, tmp);
      if (kinds & (1u << PP_PHOTO_CONV))
        hipLaunchKernelGGL(photo_stage_kernel<PP_PHOTO_CONV>, grid, block, 0, ctx->stream, slot, i0, H, W, pool_dev, src, dst, tmp);
      if (kinds & (1u << PP_PHOTO_MEDIAN))
        hipLaunchKernelGGL(photo_stage_kernel<PP_PHOTO_MEDIAN>, grid, block, 0, ctx->stream, slot, i0, H, W, pool_dev, src, dst, tmp);
      if (kinds & (1u << PP_PHOTO_BILATERAL))
        hipLaunchKernelGGL(photo_stage_kernel<PP_PHOTO_BILATERAL>, grid, block, 0, ctx->stream, slot, i0, H, W, pool_dev, src, dst, tmp);
      PP_CHECK_LAUNCH(ctx, "pp_photo_augment_u8");
    }
  return PP_OK;
}
