// The VSD pose error of the evaluation tail (tless_eval.py:470-471, 651-662 and the same calls in occlusion_eval.py /
// ycbv_eval.py / homebrewed_eval.py / linemod_eval.py), on the depth images render.hip draws.
//
// VSD: pose_error.py:15-61 + 105-176 per problem on the rendered depth images, float64 where the reference is; per-block
// partial counts / sums, then one ordered pass per problem.
// Compiled with -ffp-contract=off: the host restatements (utils/pose_error.py, tests/vsd_bop_np.py) evaluate the same
// expressions in the same order.
#include <math.h>
#include <stdint.h>
#include "pose_common.h"
#include "visib_common.h"

#define VSD_THREADS 256
#define VSD_PER_THREAD 4
#define VSD_BLOCK (VSD_THREADS * VSD_PER_THREAD)

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
