// Normal images from depth maps: the reference's get_normal (annotation_scripts/Augmentations.py:394-467) on the device.
// float64 from the first filter tap on, every product, sum and quotient rounded on its own (-ffp-contract=off) in the order the
// numpy restatement (tests/depth_normals_np.py) takes them, so the outputs are its bits.  The batch rides on gridDim.z.
//
//   smooth    one launch, both passes of scipy.ndimage.gaussian_filter(depth, 2) (radius 8, 17 taps, border mode 'reflect').  A
//             workgroup owns a DN_TILE x DN_TILE tile: it loads the float32 tile with its 8-pixel halo into LDS through the
//             reflect index rule (period 2n, so a line shorter than the halo mirrors repeatedly), runs the vertical pass over the
//             tile plus its horizontal halo into a second LDS array, and the horizontal pass from there.  Tap order of both passes:
//             the first tap, then the others in increasing index.  for_vis = 0 folds the image's largest d in (see below).
//   normals   one launch: np.gradient(d, 2, edge_order=2), the two tangents, cross product, normalisation, the NaN rule and
//             the far cut, from d in global memory (a pixel reads its 4 neighbours; on the first / last row or column the three
//             values of the one-sided formula, which reach 2 pixels in).  Writes the unit normals and / or, with for_vis = 0,
//             folds the image's largest scaled component in.
//   encode    for_vis = 0 only, the last pass: the same device function gives the normal once more (cheaper than 24 bytes per
//             pixel through memory), scaled, truncated to uint8; it also writes the scaled depth.
// The two per-image maxima are integer atomicMax on the bits of non-negative doubles (zeroed by a memset node before): the
// maximum is exact and order-free, so the results are the same from run to run.  A workgroup first folds its lanes in LDS and
// issues one global atomic.
#include "pp_internal.h"

#define DN_TILE 32
#define DN_R 8                       // int(4 * 2 + 0.5)
#define DN_TAPS (2 * DN_R + 1)
#define DN_HALO (DN_TILE + 2 * DN_R)  // 48
#define DN_THREADS 256
#define DN_MAX_SIDE 16384
#define DN_MAX_IMG 65535

struct dn_taps { double w[DN_TAPS]; };

static inline size_t dn_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// scipy's 'reflect' (d c b a | a b c d), numpy's 'symmetric': period 2n
__device__ __forceinline__ int dn_reflect(int j, int n) {
  const int p = 2 * n;
  int m = j % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// the workgroup's largest `v` (v >= 0, not NaN: its bits order as unsigned integers) into *dst
__device__ __forceinline__ void dn_group_max(double v, unsigned long long* slot, unsigned long long* dst) {
  if (threadIdx.x == 0) *slot = 0ull;
  __syncthreads();
  atomicMax(slot, (unsigned long long)__double_as_longlong(v));
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(dst, *slot);
}

__global__ void __launch_bounds__(DN_THREADS)
dn_smooth_kernel(int H, int W, const float* __restrict__ depth, dn_taps taps, double* __restrict__ d, unsigned long long* __restrict__ dmax) {
  __shared__ float raw[DN_HALO * DN_HALO];
  __shared__ double mid[DN_TILE * DN_HALO];
  __shared__ unsigned long long slot;
  const int img = blockIdx.z, x0 = blockIdx.x * DN_TILE, y0 = blockIdx.y * DN_TILE, tid = threadIdx.x;
  const float* src = depth + (size_t)img * H * W;
  for (int i = tid; i < DN_HALO * DN_HALO; i += DN_THREADS) {
    const int r = i / DN_HALO, c = i - r * DN_HALO;
    raw[i] = src[(size_t)dn_reflect(y0 + r - DN_R, H) * W + dn_reflect(x0 + c - DN_R, W)];
  }
  __syncthreads();
  // vertical pass over the tile plus its horizontal halo: mid[r][c] of output row y0 + r, padded column x0 + c - 8
  for (int i = tid; i < DN_TILE * DN_HALO; i += DN_THREADS) {
    double acc = taps.w[0] * (double)raw[i];
#pragma unroll
    for (int k = 1; k < DN_TAPS; ++k) acc = acc + taps.w[k] * (double)raw[i + k * DN_HALO];
    mid[i] = acc;
  }
  __syncthreads();
  const int tx = tid % DN_TILE, ty = tid / DN_TILE;
  double best = 0.0;
  for (int r = ty; r < DN_TILE; r += DN_THREADS / DN_TILE) {
    const double* row = mid + r * DN_HALO + tx;
    double acc = taps.w[0] * row[0];
#pragma unroll
    for (int k = 1; k < DN_TAPS; ++k) acc = acc + taps.w[k] * row[k];
    const int x = x0 + tx, y = y0 + r;
    if (x < W && y < H) {
      d[((size_t)img * H + y) * W + x] = acc;
      if (acc > best) best = acc;
    }
  }
  if (dmax) dn_group_max(best, &slot, dmax + img);
}

// The signed unit normal of pixel (y, x) of one smoothed image, zeros where the reference gives zeros (a 0 / 0 and the far
// cut); intr = (fx, cx, cy).  u, v: numpy's assignment of a float64 into an int16 array truncates toward zero.
__device__ __forceinline__ void dn_normal_at(const double* __restrict__ d, int H, int W, int y, int x, const double* __restrict__ intr,
                                             double* n0, double* n1, double* n2, double* dc_out) {
  const double c = 1.0 / intr[0];
  const double u = (double)(int)((double)x - intr[1]), v = (double)(int)((double)y - intr[2]);
  const double* p = d + (size_t)y * W + x;
  const double dc = p[0];
  double gx, gy;
  if (x == 0) gx = (-0.75 * p[0] + 1.0 * p[1]) + -0.25 * p[2];
  else if (x == W - 1) gx = (0.25 * p[-2] + -1.0 * p[-1]) + 0.75 * p[0];
  else gx = (p[1] - p[-1]) / 4.0;
  const size_t s = (size_t)W;
  if (y == 0) gy = (-0.75 * p[0] + 1.0 * p[s]) + -0.25 * p[2 * s];
  else if (y == H - 1) gy = (0.25 * *(p - 2 * s) + -1.0 * *(p - s)) + 0.75 * p[0];
  else gy = (p[s] - *(p - s)) / 4.0;
  const double uc = u * c, vc = v * c, dz = dc * c;
  const double vx0 = dz + uc * gx, vx1 = vc * gx, vx2 = gx;
  const double vy0 = uc * gy, vy1 = dz + vc * gy, vy2 = gy;
  double c0 = vx1 * vy2 - vx2 * vy1, c1 = vx2 * vy0 - vx0 * vy2, c2 = vx0 * vy1 - vx1 * vy0;
  const double norm = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
  c0 = c0 / norm;
  c1 = c1 / norm;
  c2 = c2 / norm;
  // np.nan_to_num: NaN -> 0, +-inf -> +-the largest finite double
  const double big = 1.7976931348623157e308;
  c0 = c0 != c0 ? 0.0 : (c0 > big ? big : (c0 < -big ? -big : c0));
  c1 = c1 != c1 ? 0.0 : (c1 > big ? big : (c1 < -big ? -big : c1));
  c2 = c2 != c2 ? 0.0 : (c2 > big ? big : (c2 < -big ? -big : c2));
  if (dc > 2000.0) c0 = c1 = c2 = 0.0;
  *n0 = c0;
  *n1 = c1;
  *n2 = c2;
  *dc_out = dc;
}

// the factor of for_vis = 0 on a pixel's normal: 1 - (d s - 0.5), s = 1 / the image's largest d
__device__ __forceinline__ double dn_vis_factor(double dc, double s) { return 1.0 - (dc * s - 0.5); }

__global__ void __launch_bounds__(DN_THREADS)
dn_normals_kernel(int H, int W, const double* __restrict__ d, const double* __restrict__ intr, double* __restrict__ normals,
                  double* __restrict__ signed_n, const unsigned long long* __restrict__ dmax, unsigned long long* __restrict__ nmax) {
  __shared__ unsigned long long slot;
  const int img = blockIdx.z, x = blockIdx.x * DN_TILE + threadIdx.x % DN_TILE;
  const double* di = d + (size_t)img * H * W;
  double best = 0.0;
  const double dm = nmax ? __longlong_as_double((long long)dmax[img]) : 0.0;
  for (int r = threadIdx.x / DN_TILE; r < DN_TILE; r += DN_THREADS / DN_TILE) {
    const int y = blockIdx.y * DN_TILE + r;
    if (x >= W || y >= H) continue;
    double n0, n1, n2, dc;
    dn_normal_at(di, H, W, y, x, intr + 3 * img, &n0, &n1, &n2, &dc);
    const size_t o = (((size_t)img * H + y) * W + x) * 3;
    if (signed_n) {
      signed_n[o] = n0;
      signed_n[o + 1] = n1;
      signed_n[o + 2] = n2;
    }
    n0 = fabs(n0);
    n1 = fabs(n1);
    n2 = fabs(n2);
    if (normals) {
      normals[o] = n0;
      normals[o + 1] = n1;
      normals[o + 2] = n2;
    }
    if (nmax && dm > 0.0) {
      const double f = dn_vis_factor(dc, 1.0 / dm);
      best = fmax(best, fmax(fmax(n0 * f, n1 * f), n2 * f));
    }
  }
  if (nmax) dn_group_max(best, &slot, nmax + img);
}

// Degenerate images: a largest d of 0, or a largest scaled component of 0, makes the reference divide by zero; here the uint8
// image and the scaled depth of such an image are all zero.
__global__ void __launch_bounds__(DN_THREADS)
dn_encode_kernel(int H, int W, const double* __restrict__ d, const double* __restrict__ intr, const unsigned long long* __restrict__ dmax,
                 const unsigned long long* __restrict__ nmax, unsigned char* __restrict__ normals_u8, double* __restrict__ depth_scaled) {
  const int img = blockIdx.z, x = blockIdx.x * DN_TILE + threadIdx.x % DN_TILE;
  const double* di = d + (size_t)img * H * W;
  const double dm = __longlong_as_double((long long)dmax[img]), nm = __longlong_as_double((long long)nmax[img]);
  const bool live = dm > 0.0 && nm > 0.0;
  const double s = 1.0 / dm, sc = 255.0 / nm;
  for (int r = threadIdx.x / DN_TILE; r < DN_TILE; r += DN_THREADS / DN_TILE) {
    const int y = blockIdx.y * DN_TILE + r;
    if (x >= W || y >= H) continue;
    const size_t px = ((size_t)img * H + y) * W + x;
    if (!live) {
      if (normals_u8) normals_u8[3 * px] = normals_u8[3 * px + 1] = normals_u8[3 * px + 2] = 0;
      if (depth_scaled) depth_scaled[px] = 0.0;
      continue;
    }
    if (depth_scaled) depth_scaled[px] = di[(size_t)y * W + x] * s;
    if (normals_u8) {
      double n0, n1, n2, dc;
      dn_normal_at(di, H, W, y, x, intr + 3 * img, &n0, &n1, &n2, &dc);
      const double f = dn_vis_factor(dc, s);
      normals_u8[3 * px] = (unsigned char)(int)((fabs(n0) * f) * sc);
      normals_u8[3 * px + 1] = (unsigned char)(int)((fabs(n1) * f) * sc);
      normals_u8[3 * px + 2] = (unsigned char)(int)((fabs(n2) * f) * sc);
    }
  }
}

static inline bool dn_shape_ok(int n_img, int H, int W) {
  return n_img >= 1 && n_img <= DN_MAX_IMG && H >= 3 && W >= 3 && H <= DN_MAX_SIDE && W <= DN_MAX_SIDE &&
         (long long)n_img * H * W < (1ll << 31);
}

// [2 n_img] maxima (the bits of the largest d, then of the largest scaled component), then the unscaled d [n_img,H,W]
extern "C" size_t pp_depth_normals_workspace_bytes(int n_img, int H, int W) {
  if (!dn_shape_ok(n_img, H, W)) return 0;
  return dn_align256(2 * (size_t)n_img * sizeof(unsigned long long)) + (size_t)n_img * H * W * sizeof(double);
}

extern "C" int pp_depth_normals_f64(pp_ctx* ctx, int n_img, int H, int W, const float* depth, const double* intr, const double* taps_host,
                                    int for_vis, void* workspace, size_t workspace_bytes, double* normals_f64,
                                    unsigned char* normals_u8, double* depth_smoothed_f64, double* signed_f64) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, dn_shape_ok(n_img, H, W), PP_ERR_SHAPE,
               "pp_depth_normals_f64: need 1..%d images of 3..%d x 3..%d pixels, fewer than 2^31 in all, got %d of %d x %d", DN_MAX_IMG,
               DN_MAX_SIDE, DN_MAX_SIDE, n_img, H, W);
  PP_CHECK_ARG(ctx, depth && intr && taps_host && workspace, PP_ERR_ARG, "pp_depth_normals_f64: null argument");
  PP_CHECK_ARG(ctx, for_vis == 0 || for_vis == 1, PP_ERR_ARG, "pp_depth_normals_f64: for_vis must be 0 or 1, got %d", for_vis);
  PP_CHECK_ARG(ctx, !(for_vis && normals_u8), PP_ERR_ARG, "pp_depth_normals_f64: normals_u8 is an output of for_vis = 0 only");
  PP_CHECK_ARG(ctx, normals_f64 || normals_u8 || depth_smoothed_f64 || signed_f64, PP_ERR_ARG, "pp_depth_normals_f64: no output asked for");
  PP_CHECK_ARG(ctx, workspace_bytes >= pp_depth_normals_workspace_bytes(n_img, H, W), PP_ERR_ARG,
               "pp_depth_normals_f64: workspace of %zu bytes, need %zu (pp_depth_normals_workspace_bytes)", workspace_bytes,
               pp_depth_normals_workspace_bytes(n_img, H, W));
  dn_taps taps;
  for (int k = 0; k < DN_TAPS; ++k) {
    PP_CHECK_ARG(ctx, taps_host[k] > 0.0 && taps_host[k] < 1.0, PP_ERR_ARG, "pp_depth_normals_f64: tap %d is not a weight in (0, 1)", k);
    taps.w[k] = taps_host[k];
  }
  const size_t max_bytes = dn_align256(2 * (size_t)n_img * sizeof(unsigned long long));
  unsigned long long* dmax = (unsigned long long*)workspace;
  unsigned long long* nmax = dmax + n_img;
  double* d_ws = (double*)((char*)workspace + max_bytes);
  // for_vis = 1 returns d as it is: smooth straight into the output where one is given
  double* d = (for_vis && depth_smoothed_f64) ? depth_smoothed_f64 : d_ws;
  const dim3 grid((W + DN_TILE - 1) / DN_TILE, (H + DN_TILE - 1) / DN_TILE, n_img), block(DN_THREADS);
  if (!for_vis) PP_HIP(ctx, hipMemsetAsync(workspace, 0, max_bytes, ctx->stream));
  hipLaunchKernelGGL(dn_smooth_kernel, grid, block, 0, ctx->stream, H, W, depth, taps, d, for_vis ? nullptr : dmax);
  if (for_vis) {
    if (normals_f64 || signed_f64)
      hipLaunchKernelGGL(dn_normals_kernel, grid, block, 0, ctx->stream, H, W, (const double*)d, intr, normals_f64, signed_f64,
                         (const unsigned long long*)nullptr, (unsigned long long*)nullptr);
  } else {
    hipLaunchKernelGGL(dn_normals_kernel, grid, block, 0, ctx->stream, H, W, (const double*)d, intr, normals_f64, signed_f64,
                       (const unsigned long long*)dmax, nmax);
    if (normals_u8 || depth_smoothed_f64)
      hipLaunchKernelGGL(dn_encode_kernel, grid, block, 0, ctx->stream, H, W, (const double*)d, intr, (const unsigned long long*)dmax,
                         (const unsigned long long*)nmax, normals_u8, depth_smoothed_f64);
  }
  PP_CHECK_LAUNCH(ctx, "pp_depth_normals_f64");
  return PP_OK;
}
