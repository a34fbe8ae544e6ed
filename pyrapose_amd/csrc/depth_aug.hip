// Depth-sensor simulation: the reference's augmentDepth (annotation_scripts/Augmentations.py:10-134, augment_syn_LineMOD.py:
// 273-418, augment_syn_Tless.py:219-356) on the device.  Integer work on the mask, float64 from the first average on, every
// product, sum and quotient rounded on its own (-ffp-contract=off) in the order the numpy restatement (tests/depth_aug_np.py)
// takes them, so the outputs are its bits.  The batch rides on gridDim.z; one float64 parameter row per image
// (PP_DA_* of include/pyrapose_hip.h).  No atomics, no reduction across lanes: the only cross-lane work is the LDS tiles.
//
//   A shadow   a workgroup owns a DA_TILE x DA_TILE tile of the full-size image and keeps the mask of the tile plus a 9-pixel
//              halo (3 box filters of radius <= 3) as bytes in two LDS arrays of 50 x 50, which the separable passes ping-pong
//              between: erode (rows, columns), dilate (rows, columns), count (rows), then count (columns) and the majority
//              test on the tile alone.  Pixels outside the image are 1 for the erosion and 0 afterwards; a window is cut at
//              the edge of the LDS region, which spoils at most `radius` pixels per filter from that edge inwards -- 9 in all,
//              the halo.  Writes the mask, d1 = m ? depth : 0 as float32 (exact: it is the input or 0) for an image without
//              the sensor stage, and for one with it the half-size d2 (the tile starts at an even pixel, so a half-size pixel's
//              2 x 2 source lies in one tile).
//   B sensor   half size: a 32 x 32 tile of d2 with a 3-pixel reflect_101 halo in LDS, the k_blur taps along the rows into a
//              second LDS array, then along the columns; resolution, quantisation, noise.  An image without the sensor stage
//              gets zeros.
//   C warp     one lane per full-size pixel: D is d1, or the bilinear up-sampling of s evaluated where it is needed (at the
//              pixel and at its gather target: 8 loads from an array a quarter of the size, instead of a float64 image written
//              and gathered from); three fractal simplex values, the gather, the depth offset.
//
// Simplex noise N(x, y, z; seed), the project's own: Gustavson's 3-D simplex noise.  s = ((x + y) + z) / 3 (the constant
// 1.0 / 3.0), (i, j, k) = floor of (x + s, y + s, z + s); t = ((i + j) + k) (1.0 / 6.0); offsets d0 = p - ((i, j, k) - t).
// Corner order from the offsets: x0 >= y0: y0 >= z0 -> (1,0,0),(1,1,0); else x0 >= z0 -> (1,0,0),(1,0,1); else (0,0,1),(1,0,1);
// x0 < y0: y0 < z0 -> (0,0,1),(0,1,1); else x0 < z0 -> (0,1,0),(0,1,1); else (0,1,0),(1,1,0).  d1 = (d0 - c1) + G3, d2 = (d0 - c2) +
// 2 G3, d3 = (d0 - 1) + 3 G3.  A corner gives t^4 (g . d) where t = ((0.6 - dx dx) - dy dy) - dz dz > 0, t^4 = (t t)(t t),
// g . d = (gx dx + gy dy) + gz dz with g one of the 12 edge midpoints (the table below), chosen by
//   h = lo32(seed) ^ hi32(seed) ^ i 0x9E3779B1 ^ j 0x85EBCA77 ^ k 0xC2B2AE3D  (uint32, i j k their low 32 bits),
//   h ^= h >> 16, h *= 0x85EBCA6B, h ^= h >> 13, h *= 0xC2B2AE35, h ^= h >> 16  (murmur3's finaliser), index h mod 12.
// N = 32 (((n0 + n1) + n2) + n3): |N| < 1 (0.98 over 2 10^6 random points).
#include <cmath>

#include "pp_internal.h"
#include "splitmix.h"

#define DA_TILE 32
#define DA_HALO 9
#define DA_REG (DA_TILE + 2 * DA_HALO)  // 50
#define DA_BH 3                         // the blur's halo
#define DA_BREG (DA_TILE + 2 * DA_BH)   // 38
#define DA_THREADS 256
#define DA_CW 32                        // launch C: 32 x 8 pixels per workgroup
#define DA_CH 8
#define DA_MAX_SIDE 16384
#define DA_MIN_SIDE 8
#define DA_MAX_IMG 65535
#define DA_P PP_DA_P

static inline size_t da_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// one separable pass over the 50 x 50 region: OP 0 = min, 1 = max, 2 = sum over the 2 r + 1 window along a row (HORIZ) or a
// column, the window cut at the region's edge.  ZERO_OUTSIDE: positions outside the image become 0.
template <int OP, bool HORIZ, bool ZERO_OUTSIDE>
__device__ __forceinline__ void da_pass(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int r, int y0, int x0,
                                        int H, int W) {
  for (int i = threadIdx.x; i < DA_REG * DA_REG; i += DA_THREADS) {
    const int rr = i / DA_REG, cc = i - rr * DA_REG;
    const int at = HORIZ ? cc : rr;
    const int lo = at - r < 0 ? 0 : at - r, hi = at + r > DA_REG - 1 ? DA_REG - 1 : at + r;
    int v = OP == 0 ? 1 : 0;
    for (int k = lo; k <= hi; ++k) {
      const int s = HORIZ ? src[rr * DA_REG + k] : src[k * DA_REG + cc];
      v = OP == 0 ? (s < v ? s : v) : (OP == 1 ? (s > v ? s : v) : v + s);
    }
    if (ZERO_OUTSIDE) {
      const int y = y0 + rr - DA_HALO, x = x0 + cc - DA_HALO;
      if (y < 0 || y >= H || x < 0 || x >= W) v = 0;
    }
    dst[i] = (unsigned char)v;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(DA_THREADS)
da_shadow_kernel(int H, int W, int h2, int w2, const float* __restrict__ depth, const unsigned char* __restrict__ mask,
                 const double* __restrict__ params, unsigned char* __restrict__ mask_u8, float* __restrict__ d1, double* __restrict__ d2) {
  __shared__ unsigned char a[DA_REG * DA_REG];
  __shared__ unsigned char b[DA_REG * DA_REG];
  const int img = blockIdx.z, x0 = blockIdx.x * DA_TILE, y0 = blockIdx.y * DA_TILE, tid = threadIdx.x;
  const double* row = params + (size_t)img * DA_P;
  const int r_open = ((int)row[PP_DA_K_OPEN] - 1) / 2, k_med = (int)row[PP_DA_K_MED], r_med = (k_med - 1) / 2;
  const bool sensor = row[PP_DA_SENSOR] != 0.0;
  const unsigned char* msrc = mask + (size_t)img * H * W;
  const float* dsrc = depth + (size_t)img * H * W;
  for (int i = tid; i < DA_REG * DA_REG; i += DA_THREADS) {
    const int rr = i / DA_REG, cc = i - rr * DA_REG;
    const int y = y0 + rr - DA_HALO, x = x0 + cc - DA_HALO;
    const bool inside = y >= 0 && y < H && x >= 0 && x < W;
    a[i] = inside ? (msrc[(size_t)y * W + x] != 0 ? 1 : 0) : 1;  // outside takes no part in the erosion
  }
  __syncthreads();
  da_pass<0, true, false>(a, b, r_open, y0, x0, H, W);
  da_pass<0, false, true>(b, a, r_open, y0, x0, H, W);   // eroded; outside takes no part in the dilation
  da_pass<1, true, false>(a, b, r_open, y0, x0, H, W);
  da_pass<1, false, true>(b, a, r_open, y0, x0, H, W);   // opened; zero-padded for the count
  da_pass<2, true, false>(a, b, r_med, y0, x0, H, W);    // row counts, <= 7
  // column counts and the majority test on the tile; a's tile positions take m (a is read by nobody any more)
  for (int i = tid; i < DA_TILE * DA_TILE; i += DA_THREADS) {
    const int rr = i / DA_TILE + DA_HALO, cc = i % DA_TILE + DA_HALO;
    int cnt = 0;
    for (int k = rr - r_med; k <= rr + r_med; ++k) cnt += b[k * DA_REG + cc];
    a[rr * DA_REG + cc] = 2 * cnt > k_med * k_med ? 1 : 0;
  }
  __syncthreads();
  for (int i = tid; i < DA_TILE * DA_TILE; i += DA_THREADS) {
    const int ty = i / DA_TILE, tx = i % DA_TILE, y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) continue;
    const int m = a[(ty + DA_HALO) * DA_REG + tx + DA_HALO];
    const size_t px = ((size_t)img * H + y) * W + x;
    if (mask_u8) mask_u8[px] = m ? 255 : 0;
    if (d1 && !sensor) d1[px] = m ? dsrc[(size_t)y * W + x] : 0.0f;
  }
  if (d2 && sensor) {
    // one half-size pixel per lane: 16 x 16 of them lie in this tile
    const int hy = y0 / 2 + tid / (DA_TILE / 2), hx = x0 / 2 + tid % (DA_TILE / 2);
    if (hy < h2 && hx < w2) {
      const int r0 = min(2 * hy, H - 1), r1 = min(2 * hy + 1, H - 1), c0 = min(2 * hx, W - 1), c1 = min(2 * hx + 1, W - 1);
#define DA_D1(r, c) (a[((r) - y0 + DA_HALO) * DA_REG + (c) - x0 + DA_HALO] ? (double)dsrc[(size_t)(r) * W + (c)] : 0.0)
      const double ta = 0.5 * DA_D1(r0, c0) + 0.5 * DA_D1(r0, c1);
      const double tb = 0.5 * DA_D1(r1, c0) + 0.5 * DA_D1(r1, c1);
#undef DA_D1
      d2[((size_t)img * h2 + hy) * w2 + hx] = 0.5 * ta + 0.5 * tb;
    }
  }
}

// cv2's BORDER_REFLECT_101 (g f e d c b | a b c d e f g h): period 2 (n - 1)
__device__ __forceinline__ int da_reflect_101(int j, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  int m = j % p;
  if (m < 0) m += p;
  return m < n ? m : p - m;
}

__global__ void __launch_bounds__(DA_THREADS)
da_sensor_kernel(int h2, int w2, const double* __restrict__ d2, const float* __restrict__ z, const double* __restrict__ params,
                 double* __restrict__ s) {
  __shared__ double raw[DA_BREG * DA_BREG];
  __shared__ double mid[DA_BREG * DA_TILE];
  const int img = blockIdx.z, x0 = blockIdx.x * DA_TILE, y0 = blockIdx.y * DA_TILE, tid = threadIdx.x;
  const double* row = params + (size_t)img * DA_P;
  const size_t base = (size_t)img * h2 * w2;
  if (row[PP_DA_SENSOR] == 0.0) {  // (the whole workgroup: one image per blockIdx.z)
    for (int i = tid; i < DA_TILE * DA_TILE; i += DA_THREADS) {
      const int y = y0 + i / DA_TILE, x = x0 + i % DA_TILE;
      if (y < h2 && x < w2) s[base + (size_t)y * w2 + x] = 0.0;
    }
    return;
  }
  const int k = (int)row[PP_DA_K_BLUR], first = DA_BH - (k - 1) / 2;
  double w[7];
#pragma unroll
  for (int t = 0; t < 7; ++t) w[t] = row[PP_DA_TAPS + t];
  const double depth_noise = row[PP_DA_DEPTH_NOISE];
  const double* src = d2 + base;
  for (int i = tid; i < DA_BREG * DA_BREG; i += DA_THREADS) {
    const int rr = i / DA_BREG, cc = i - rr * DA_BREG;
    raw[i] = src[(size_t)da_reflect_101(y0 + rr - DA_BH, h2) * w2 + da_reflect_101(x0 + cc - DA_BH, w2)];
  }
  __syncthreads();
  // along the rows: mid[rr][c] of padded row rr, output column x0 + c
  for (int i = tid; i < DA_BREG * DA_TILE; i += DA_THREADS) {
    const int rr = i / DA_TILE, c = i % DA_TILE;
    const double* p = raw + rr * DA_BREG + c + first;
    double acc = w[0] * p[0];
#pragma unroll
    for (int t = 1; t < 7; ++t)
      if (t < k) acc = acc + w[t] * p[t];
    mid[i] = acc;
  }
  __syncthreads();
  for (int i = tid; i < DA_TILE * DA_TILE; i += DA_THREADS) {
    const int ry = i / DA_TILE, c = i % DA_TILE, y = y0 + ry, x = x0 + c;
    if (y >= h2 || x >= w2) continue;
    const double* p = mid + (ry + first) * DA_TILE + c;
    double acc = w[0] * p[0];
#pragma unroll
    for (int t = 1; t < 7; ++t)
      if (t < k) acc = acc + w[t] * p[t * DA_TILE];
    const double d = raw[(ry + DA_BH) * DA_BREG + c + DA_BH];
    const double tt = (d / 1000.0) * 1.41421356;
    const double res = tt * tt;
    const double q = res != 0.0 ? rint(acc / res) * res : 0.0;
    s[base + (size_t)y * w2 + x] = q + (q * depth_noise) * (double)z[base + (size_t)y * w2 + x];
  }
}

__device__ const double DA_GRAD[12][3] = {{1, 1, 0}, {-1, 1, 0}, {1, -1, 0}, {-1, -1, 0}, {1, 0, 1}, {-1, 0, 1},
                                          {1, 0, -1}, {-1, 0, -1}, {0, 1, 1}, {0, -1, 1}, {0, 1, -1}, {0, -1, -1}};
#define DA_F3 (1.0 / 3.0)
#define DA_G3 (1.0 / 6.0)
#define DA_G3_2 (2.0 * (1.0 / 6.0))
#define DA_G3_3 (3.0 * (1.0 / 6.0))
#define DA_NOISE_SCALE 32.0

__device__ __forceinline__ double da_corner(double x, double y, double z, long long i, long long j, long long k, unsigned int seed32) {
  const double t = ((0.6 - x * x) - y * y) - z * z;
  if (!(t > 0.0)) return 0.0;
  unsigned int h = seed32 ^ ((unsigned int)i * 0x9E3779B1u) ^ ((unsigned int)j * 0x85EBCA77u) ^ ((unsigned int)k * 0xC2B2AE3Du);
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  const double* g = DA_GRAD[h % 12u];
  const double dot = (g[0] * x + g[1] * y) + g[2] * z;
  const double t2 = t * t;
  return (t2 * t2) * dot;
}

__device__ double da_simplex3(double x, double y, double z, unsigned long long seed) {
  const unsigned int seed32 = (unsigned int)(seed ^ (seed >> 32));
  const double s = ((x + y) + z) * DA_F3;
  const double fi = floor(x + s), fj = floor(y + s), fk = floor(z + s);
  const long long i = (long long)fi, j = (long long)fj, k = (long long)fk;
  const double t = (double)((i + j) + k) * DA_G3;
  const double x0 = x - (fi - t), y0 = y - (fj - t), z0 = z - (fk - t);
  int i1, j1, k1, i2, j2, k2;
  if (x0 >= y0) {
    if (y0 >= z0) { i1 = 1; j1 = 0; k1 = 0; i2 = 1; j2 = 1; k2 = 0; }
    else if (x0 >= z0) { i1 = 1; j1 = 0; k1 = 0; i2 = 1; j2 = 0; k2 = 1; }
    else { i1 = 0; j1 = 0; k1 = 1; i2 = 1; j2 = 0; k2 = 1; }
  } else {
    if (y0 < z0) { i1 = 0; j1 = 0; k1 = 1; i2 = 0; j2 = 1; k2 = 1; }
    else if (x0 < z0) { i1 = 0; j1 = 1; k1 = 0; i2 = 0; j2 = 1; k2 = 1; }
    else { i1 = 0; j1 = 1; k1 = 0; i2 = 1; j2 = 1; k2 = 0; }
  }
  double n = da_corner(x0, y0, z0, i, j, k, seed32);
  n = n + da_corner((x0 - (double)i1) + DA_G3, (y0 - (double)j1) + DA_G3, (z0 - (double)k1) + DA_G3, i + i1, j + j1, k + k1, seed32);
  n = n + da_corner((x0 - (double)i2) + DA_G3_2, (y0 - (double)j2) + DA_G3_2, (z0 - (double)k2) + DA_G3_2, i + i2, j + j2, k + k2, seed32);
  n = n + da_corner((x0 - 1.0) + DA_G3_3, (y0 - 1.0) + DA_G3_3, (z0 - 1.0) + DA_G3_3, i + 1, j + 1, k + 1, seed32);
  return DA_NOISE_SCALE * n;
}

// field f of pixel (y, x): the fractal sum at (j_f, y, x) freq
__device__ double da_field(const double* __restrict__ row, int f, int y, int x, unsigned long long pixel) {
  const unsigned long long seed = (unsigned long long)row[PP_DA_SEED];
  const double u = (double)(splitmix64(splitmix64(4ull * seed + (unsigned long long)f) + pixel) >> 11) * 0x1p-53;
  const double lo = row[PP_DA_JITTER_LO + f], hi = row[PP_DA_JITTER_HI + f], freq = row[PP_DA_FREQ];
  const double jf = lo + (hi - lo) * u;
  const double px = jf * freq, py = (double)y * freq, pz = (double)x * freq;
  const int octaves = (int)row[PP_DA_OCTAVES];
  const double lacunarity = row[PP_DA_LACUNARITY], gain = row[PP_DA_GAIN];
  double total = 0.0, norm = 0.0, amp = 1.0, fo = 1.0;
  for (int o = 0; o < octaves; ++o) {
    total = total + amp * da_simplex3(px * fo, py * fo, pz * fo, seed + (unsigned long long)o);
    norm = norm + amp;
    amp = amp * gain;
    fo = fo * lacunarity;
  }
  return total / norm;
}

// cv2's INTER_LINEAR source of output index o: (s0, s1, frac)
__device__ __forceinline__ void da_up_axis(int o, double scale, int n_in, int* s0, int* s1, double* frac) {
  const double f = ((double)o + 0.5) * scale - 0.5;
  const double fl = floor(f);
  double fr = f - fl;
  int si = (int)fl;
  if (si < 0) { si = 0; fr = 0.0; }
  else if (si >= n_in - 1) { si = n_in - 1; fr = 0.0; }
  *s0 = si;
  *s1 = min(si + 1, n_in - 1);
  *frac = fr;
}

struct da_image {
  const float* d1;   // [H,W] of an image without the sensor stage
  const double* s;   // [h2,w2] of one with it
  int H, W, h2, w2;
  bool sensor;
};

__device__ __forceinline__ double da_D(const da_image& im, int y, int x) {
  if (!im.sensor) return (double)im.d1[(size_t)y * im.W + x];
  int sy0, sy1, sx0, sx1;
  double fy, fx;
  da_up_axis(y, (double)im.h2 / (double)im.H, im.h2, &sy0, &sy1, &fy);
  da_up_axis(x, (double)im.w2 / (double)im.W, im.w2, &sx0, &sx1, &fx);
  const double* r0 = im.s + (size_t)sy0 * im.w2;
  const double* r1 = im.s + (size_t)sy1 * im.w2;
  const double top = (1.0 - fx) * r0[sx0] + fx * r0[sx1];
  const double bot = (1.0 - fx) * r1[sx0] + fx * r1[sx1];
  return (1.0 - fy) * top + fy * bot;
}

__global__ void __launch_bounds__(DA_THREADS)
da_warp_kernel(int H, int W, int h2, int w2, const float* __restrict__ d1, const double* __restrict__ s, const double* __restrict__ params,
               float* __restrict__ depth_f32, double* __restrict__ depth_f64, double* __restrict__ sensor_f64) {
  const int img = blockIdx.z, x = blockIdx.x * DA_CW + threadIdx.x % DA_CW, y = blockIdx.y * DA_CH + threadIdx.x / DA_CW;
  if (x >= W || y >= H) return;
  const double* row = params + (size_t)img * DA_P;
  da_image im;
  im.sensor = row[PP_DA_SENSOR] != 0.0;
  im.d1 = d1 + (size_t)img * H * W;
  im.s = s + (size_t)img * h2 * w2;
  im.H = H; im.W = W; im.h2 = h2; im.w2 = w2;
  const size_t px = ((size_t)img * H + y) * W + x;
  const double D = da_D(im, y, x);
  if (sensor_f64) sensor_f64[px] = D;
  double out = D;
  if (row[PP_DA_SIMPLEX] != 0.0 && (depth_f32 || depth_f64)) {
    const unsigned long long pixel = (unsigned long long)y * (unsigned long long)W + (unsigned long long)x;
    const double V0 = da_field(row, 0, y, x, pixel), V1 = da_field(row, 1, y, x, pixel), V2 = da_field(row, 2, y, x, pixel);
    const double a = D * 0.001;
    const double axy = a * row[PP_DA_W_XY];
    double fx = (double)x + axy * V0, fy = (double)y + axy * V1;
    fx = fx < 0.0 ? 0.0 : (fx > (double)(W - 1) ? (double)(W - 1) : fx);
    fy = fy < 0.0 ? 0.0 : (fy > (double)(H - 1) ? (double)(H - 1) : fy);
    int gx = (int)fx, gy = (int)fy;
    gx = gx < 0 ? 0 : (gx > W - 1 ? W - 1 : gx);  // (a NaN from non-finite parameters must not leave the image)
    gy = gy < 0 ? 0 : (gy > H - 1 ? H - 1 : gy);
    out = da_D(im, gy, gx) + (a * row[PP_DA_W_Z]) * V2;
    out = out > 0.0 ? out : 0.0;
  }
  if (depth_f64) depth_f64[px] = out;
  if (depth_f32) depth_f32[px] = (float)out;
}

static inline bool da_shape_ok(int n_img, int H, int W) {
  return n_img >= 1 && n_img <= DA_MAX_IMG && H >= DA_MIN_SIDE && W >= DA_MIN_SIDE && H <= DA_MAX_SIDE && W <= DA_MAX_SIDE;
}

// cv2's cvRound(n / 2): half to even
static inline int da_half(int n) { return (n / 2) + ((n & 1) ? ((n / 2) & 1) : 0); }

// d1 float32 [n,H,W], then d2 and s float64 [n,h2,w2] each
extern "C" size_t pp_depth_augment_workspace_bytes(int n_img, int H, int W) {
  if (!da_shape_ok(n_img, H, W)) return 0;
  const size_t half = da_align256((size_t)n_img * da_half(H) * da_half(W) * sizeof(double));
  return da_align256((size_t)n_img * H * W * sizeof(float)) + 2 * half;
}

extern "C" int pp_depth_augment(pp_ctx* ctx, int n_img, int H, int W, const float* depth, const unsigned char* mask, const double* params,
                                const double* params_host, const float* z, void* workspace, size_t workspace_bytes, float* depth_f32,
                                double* depth_f64, unsigned char* mask_u8, double* half_f64, double* sensor_f64) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, da_shape_ok(n_img, H, W), PP_ERR_SHAPE, "pp_depth_augment: need 1..%d images of %d..%d x %d..%d pixels, got %d of %d x %d",
               DA_MAX_IMG, DA_MIN_SIDE, DA_MAX_SIDE, DA_MIN_SIDE, DA_MAX_SIDE, n_img, H, W);
  PP_CHECK_ARG(ctx, depth && mask && params && params_host && workspace, PP_ERR_ARG, "pp_depth_augment: null argument");
  PP_CHECK_ARG(ctx, depth_f32 || depth_f64 || mask_u8 || half_f64 || sensor_f64, PP_ERR_ARG, "pp_depth_augment: no output asked for");
  PP_CHECK_ARG(ctx, workspace_bytes >= pp_depth_augment_workspace_bytes(n_img, H, W), PP_ERR_ARG,
               "pp_depth_augment: workspace of %zu bytes, need %zu (pp_depth_augment_workspace_bytes)", workspace_bytes,
               pp_depth_augment_workspace_bytes(n_img, H, W));
  bool any_sensor = false;
  for (int i = 0; i < n_img; ++i) {
    const double* r = params_host + (size_t)i * DA_P;
    const int ks[3] = {PP_DA_K_OPEN, PP_DA_K_MED, PP_DA_K_BLUR};
    for (int c = 0; c < 3; ++c)
      PP_CHECK_ARG(ctx, r[ks[c]] == 1.0 || r[ks[c]] == 3.0 || r[ks[c]] == 5.0 || r[ks[c]] == 7.0, PP_ERR_ARG,
                   "pp_depth_augment: image %d: kernel size %d is %g, need 1, 3, 5 or 7", i, c, r[ks[c]]);
    PP_CHECK_ARG(ctx, r[PP_DA_OCTAVES] >= 1.0 && r[PP_DA_OCTAVES] <= 8.0 && r[PP_DA_OCTAVES] == floor(r[PP_DA_OCTAVES]), PP_ERR_ARG,
                 "pp_depth_augment: image %d: octaves %g, need an integer in 1..8", i, r[PP_DA_OCTAVES]);
    PP_CHECK_ARG(ctx, (r[PP_DA_SENSOR] == 0.0 || r[PP_DA_SENSOR] == 1.0) && (r[PP_DA_SIMPLEX] == 0.0 || r[PP_DA_SIMPLEX] == 1.0), PP_ERR_ARG,
                 "pp_depth_augment: image %d: sensor and simplex must be 0 or 1", i);
    PP_CHECK_ARG(ctx, r[PP_DA_SEED] >= 0.0 && r[PP_DA_SEED] < 9007199254740992.0 && r[PP_DA_SEED] == floor(r[PP_DA_SEED]), PP_ERR_ARG,
                 "pp_depth_augment: image %d: seed must be an integer in [0, 2^53)", i);
    // the noise lattice is indexed with 64-bit integers: coordinates stay far below 2^63
    PP_CHECK_ARG(ctx, r[PP_DA_FREQ] >= 0.0 && r[PP_DA_FREQ] <= 16.0 && r[PP_DA_LACUNARITY] > 0.0 && r[PP_DA_LACUNARITY] <= 4.0, PP_ERR_ARG,
                 "pp_depth_augment: image %d: need freq in [0, 16] and lacunarity in (0, 4]", i);
    for (int c = 0; c < DA_P; ++c) PP_CHECK_ARG(ctx, std::isfinite(r[c]), PP_ERR_ARG, "pp_depth_augment: image %d: parameter %d is not finite", i, c);
    for (int c = 0; c < 3; ++c)
      PP_CHECK_ARG(ctx, fabs(r[PP_DA_JITTER_LO + c]) <= 65536.0 && fabs(r[PP_DA_JITTER_HI + c]) <= 65536.0, PP_ERR_ARG,
                   "pp_depth_augment: image %d: jitter range %d beyond +-65536", i, c);
    any_sensor = any_sensor || r[PP_DA_SENSOR] == 1.0;
  }
  PP_CHECK_ARG(ctx, z || !any_sensor, PP_ERR_ARG, "pp_depth_augment: z is null while an image has sensor = 1");
  const int h2 = da_half(H), w2 = da_half(W);
  const size_t half = da_align256((size_t)n_img * h2 * w2 * sizeof(double));
  float* d1 = (float*)workspace;
  double* d2 = (double*)((char*)workspace + da_align256((size_t)n_img * H * W * sizeof(float)));
  double* s = half_f64 ? half_f64 : (double*)((char*)d2 + half);
  const bool need_c = depth_f32 || depth_f64 || sensor_f64;
  const bool need_b = (any_sensor && need_c) || half_f64;
  const dim3 block(DA_THREADS);
  const dim3 grid_a((W + DA_TILE - 1) / DA_TILE, (H + DA_TILE - 1) / DA_TILE, n_img);
  hipLaunchKernelGGL(da_shadow_kernel, grid_a, block, 0, ctx->stream, H, W, h2, w2, depth, mask, params, mask_u8, need_c ? d1 : nullptr,
                     need_b ? d2 : nullptr);
  if (need_b) {
    const dim3 grid_b((w2 + DA_TILE - 1) / DA_TILE, (h2 + DA_TILE - 1) / DA_TILE, n_img);
    hipLaunchKernelGGL(da_sensor_kernel, grid_b, block, 0, ctx->stream, h2, w2, (const double*)d2, z, params, s);
  }
  if (need_c) {
    const dim3 grid_c((W + DA_CW - 1) / DA_CW, (H + DA_CH - 1) / DA_CH, n_img);
    hipLaunchKernelGGL(da_warp_kernel, grid_c, block, 0, ctx->stream, H, W, h2, w2, (const float*)d1, (const double*)s, params, depth_f32,
                       depth_f64, sensor_f64);
  }
  PP_CHECK_LAUNCH(ctx, "pp_depth_augment");
  return PP_OK;
}
