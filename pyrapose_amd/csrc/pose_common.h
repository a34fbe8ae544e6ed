// Pieces shared by the evaluation tail (pose.hip, render.hip, vsd.hip, icp.hip): the 256-wide tile sum with its mean over tiles,
// the tile maximum, the one-workgroup exclusive scan (the renderer's bins, the ICP cloud) and the workspace alignment.  Every
// includer is compiled with -ffp-contract=off.  What VSD and scene ground truth share is in visib_common.h.
// Not here, on purpose: the small-matrix code of pnp.hip / wpnp.hip / icp.hip (solve6 vs wpnp_ldlt, so3_exp_mul vs
// wpnp_rot_and_jl, the point accumulators) -- each is pinned operation by operation to its own numpy restatement.
#pragma once
#include "pp_internal.h"

#define POSE_TILE 256
#define SCAN_THREADS 1024

static inline size_t pp_align256(size_t b) { return (b + 255) & ~(size_t)255; }

// sum of v over the workgroup's POSE_TILE threads in a fixed order (LDS halving tree), returned to every thread
__device__ __forceinline__ double tile_sum256(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = POSE_TILE / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// max of each of v[0..N) over the workgroup's POSE_TILE threads, returned to every thread.  A maximum is exact in any order:
// 64-lane butterflies, then the waves' values through red (N * POSE_TILE / 64 doubles).  NaN never wins a comparison.
template <int N>
__device__ __forceinline__ void tile_max256(double (&v)[N], double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    for (int o = 32; o > 0; o >>= 1) {
      const double u = __shfl_xor(v[k], o, 64);
      v[k] = u > v[k] ? u : v[k];
    }
    if (lane == 0) red[k * (POSE_TILE / 64) + wave] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double r = red[k * (POSE_TILE / 64)];
    for (int w = 1; w < POSE_TILE / 64; ++w) {
      const double u = red[k * (POSE_TILE / 64) + w];
      r = u > r ? u : r;
    }
    v[k] = r;
  }
  __syncthreads();
}

// out[pose] = (partial[pose][0] + partial[pose][1] + ...) / n_pts, the tiles in order
static __global__ void tile_mean_kernel(int n_pose, int n_tiles, int n_pts, const double* __restrict__ partial, double* __restrict__ out) {
  const int pose = blockIdx.x * blockDim.x + threadIdx.x;
  if (pose >= n_pose) return;
  double s = 0.0;
  for (int t = 0; t < n_tiles; ++t) s += partial[(size_t)pose * n_tiles + t];
  out[pose] = s / (double)n_pts;
}

// A per-pose mean over model points: the common argument checks, tile_kernel on grid (tiles, poses) for partial[pose][tile]
// in `workspace` (pp_pose_error_workspace_bytes), then the mean.  in: the kernel's input pointers, none may be null.
template <class... In>
static int tile_mean_launch(pp_ctx* ctx, const char* who, void (*tile_kernel)(int, In..., double*), int n_pose, int n_pts,
                            void* workspace, double* out, In... in) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n_pose > 0 && n_pose <= 65535 && n_pts > 0, PP_ERR_SHAPE, "%s: need 1..65535 poses and at least one model point", who);
  PP_CHECK_ARG(ctx, (... && in) && workspace && out, PP_ERR_ARG, "%s: null argument", who);
  const int tiles = (n_pts + POSE_TILE - 1) / POSE_TILE;
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(tile_kernel, dim3(tiles, n_pose), dim3(POSE_TILE), 0, ctx->stream, n_pts, in..., partial);
  hipLaunchKernelGGL(tile_mean_kernel, dim3((n_pose + 63) / 64), dim3(64), 0, ctx->stream, n_pose, tiles, n_pts, (const double*)partial, out);
  PP_CHECK_LAUNCH(ctx, who);
  return PP_OK;
}

// one workgroup of SCAN_THREADS: offsets[i] = sum of counts[0..i), offsets[n] = total; cursor (may be null) = offsets[0..n)
static __global__ void __launch_bounds__(SCAN_THREADS)
exclusive_scan_kernel(int n, const int* __restrict__ counts, int* __restrict__ offsets, int* __restrict__ cursor) {
  __shared__ int s[SCAN_THREADS];
  __shared__ int carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += SCAN_THREADS) {
    const int v = base + tid < n ? counts[base + tid] : 0;
    s[tid] = v;
    __syncthreads();
    for (int off = 1; off < SCAN_THREADS; off <<= 1) {
      const int u = tid >= off ? s[tid - off] : 0;
      __syncthreads();
      s[tid] += u;
      __syncthreads();
    }
    const int excl = carry + s[tid] - v;
    if (base + tid < n) {
      offsets[base + tid] = excl;
      if (cursor) cursor[base + tid] = excl;
    }
    __syncthreads();
    if (tid == SCAN_THREADS - 1) carry += s[SCAN_THREADS - 1];
    __syncthreads();
  }
  if (tid == 0) offsets[n] = carry;
}
