// Pose-error metrics of the evaluation tail: ADD and ADD-S/ADI (utils/pose_error.py:210-246, called at
// utils/linemod_eval.py:525-531 with the decision err < 0.1 * diameter) and the reprojection error (pose_error.py:179-207,
// tless_eval.py:651-662).  float64 like the reference's numpy.
//   ADD = mean_i || (R_est p_i + t_est) - (R_gt p_i + t_gt) ||
//   ADI = mean_i  min_j || (R_gt p_i + t_gt) - (R_est p_j + t_est) ||     (cKDTree(pts_est).query(pts_gt, k=1))
//   reproj = mean_i || proj(K, R_est, t_est, p_i) - proj(K, R_gt, t_gt, p_i) ||   (float32 pixels and norm)
// BOP's symmetry-aware errors (bop_toolkit pose_error.mssd / mspd; S = misc.get_symmetry_transformations, identity first):
//   G_s  = (R_gt S_R[s], R_gt S_t[s] + t_gt)                               the ground truth moved by symmetry s
//   MSSD = min_s max_i || (R_est p_i + t_est) - (G_s.R p_i + G_s.t) ||
//   MSPD = min_s max_i || proj(K, R_est, t_est, p_i) - proj(K, G_s.R, G_s.t, p_i) ||     (float64 pixels)
// Reductions are fixed-order (per-tile partial sums, then one pass over the tiles): results do not depend on timing.
// (The maxima and minima of MSSD / MSPD are exact in any order.)
// Compiled with -ffp-contract=off: x*x + y*y + z*z is evaluated as written.
#include "pose_common.h"

__device__ __forceinline__ void rigid(const double* __restrict__ R, const double* __restrict__ t, double x, double y, double z,
                                      double* ox, double* oy, double* oz) {
  *ox = R[0] * x + R[1] * y + R[2] * z + t[0];
  *oy = R[3] * x + R[4] * y + R[5] * z + t[1];
  *oz = R[6] * x + R[7] * y + R[8] * z + t[2];
}

// grid (tiles, poses): partial[pose][tile] = sum over the tile's points of the per-point distance
__global__ void pose_add_kernel(int n_pts, const double* __restrict__ pts, const double* __restrict__ R_est,
                                const double* __restrict__ t_est, const double* __restrict__ R_gt, const double* __restrict__ t_gt,
                                double* __restrict__ partial) {
  __shared__ double red[POSE_TILE];
  const int pose = blockIdx.y, i = blockIdx.x * POSE_TILE + threadIdx.x;
  double d = 0.0;
  if (i < n_pts) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    double ax, ay, az, bx, by, bz;
    rigid(R_est + 9 * pose, t_est + 3 * pose, x, y, z, &ax, &ay, &az);
    rigid(R_gt + 9 * pose, t_gt + 3 * pose, x, y, z, &bx, &by, &bz);
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    d = sqrt(dx * dx + dy * dy + dz * dz);
  }
  const double s = tile_sum256(d, red);
  if (threadIdx.x == 0) partial[(size_t)pose * gridDim.x + blockIdx.x] = s;
}

__global__ void pose_adi_kernel(int n_pts, const double* __restrict__ pts, const double* __restrict__ R_est,
                                const double* __restrict__ t_est, const double* __restrict__ R_gt, const double* __restrict__ t_gt,
                                double* __restrict__ partial) {
  __shared__ double red[POSE_TILE];
  __shared__ double ex[POSE_TILE], ey[POSE_TILE], ez[POSE_TILE];
  const int pose = blockIdx.y, i = blockIdx.x * POSE_TILE + threadIdx.x;
  double gx = 0.0, gy = 0.0, gz = 0.0;
  if (i < n_pts) rigid(R_gt + 9 * pose, t_gt + 3 * pose, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], &gx, &gy, &gz);
  double best = 1.0e300;
  for (int j0 = 0; j0 < n_pts; j0 += POSE_TILE) {
    const int j = j0 + threadIdx.x;
    __syncthreads();
    if (j < n_pts) rigid(R_est + 9 * pose, t_est + 3 * pose, pts[3 * j], pts[3 * j + 1], pts[3 * j + 2], &ex[threadIdx.x], &ey[threadIdx.x], &ez[threadIdx.x]);
    __syncthreads();
    const int lim = min(POSE_TILE, n_pts - j0);
    for (int k = 0; k < lim; ++k) {
      const double dx = gx - ex[k], dy = gy - ey[k], dz = gz - ez[k];
      const double q = dx * dx + dy * dy + dz * dz;
      best = q < best ? q : best;
    }
  }
  const double s = tile_sum256(i < n_pts ? sqrt(best) : 0.0, red);
  if (threadIdx.x == 0) partial[(size_t)pose * gridDim.x + blockIdx.x] = s;
}

// pose_error.py:179-207: both poses projected with K, pixels rounded to float32 as the reference's arrays are
__device__ __forceinline__ void project_f32(const double* __restrict__ K, const double* __restrict__ R, const double* __restrict__ t,
                                            double x, double y, double z, float* u, float* v) {
  const double X = R[0] * x + R[1] * y + R[2] * z + t[0];
  const double Y = R[3] * x + R[4] * y + R[5] * z + t[1];
  const double Z = R[6] * x + R[7] * y + R[8] * z + t[2];
  const double a = K[0] * X + K[1] * Y + K[2] * Z, b = K[3] * X + K[4] * Y + K[5] * Z, w = K[6] * X + K[7] * Y + K[8] * Z;
  *u = (float)(a / w);
  *v = (float)(b / w);
}

// grid (tiles, poses): partial[pose][tile] = sum over the tile's points of || est_px - gt_px || (float32 pixels, float32 norm)
__global__ void pose_reproj_kernel(int n_pts, const double* __restrict__ pts, const double* __restrict__ K9, const double* __restrict__ R_est,
                                   const double* __restrict__ t_est, const double* __restrict__ R_gt, const double* __restrict__ t_gt,
                                   double* __restrict__ partial) {
  __shared__ double red[POSE_TILE];
  const int pose = blockIdx.y, i = blockIdx.x * POSE_TILE + threadIdx.x;
  double d = 0.0;
  if (i < n_pts) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    float ue, ve, ug, vg;
    project_f32(K9 + 9 * pose, R_est + 9 * pose, t_est + 3 * pose, x, y, z, &ue, &ve);
    project_f32(K9 + 9 * pose, R_gt + 9 * pose, t_gt + 3 * pose, x, y, z, &ug, &vg);
    const float du = ue - ug, dv = ve - vg;
    d = (double)sqrtf(du * du + dv * dv);
  }
  const double s = tile_sum256(d, red);
  if (threadIdx.x == 0) partial[(size_t)pose * gridDim.x + blockIdx.x] = s;
}

extern "C" size_t pp_pose_error_workspace_bytes(int n_pose, int n_pts) {
  if (n_pose <= 0 || n_pts <= 0) return 0;
  return (size_t)n_pose * ((n_pts + POSE_TILE - 1) / POSE_TILE) * sizeof(double);
}

extern "C" int pp_pose_add_f64(pp_ctx* ctx, int n_pose, int n_pts, const double* pts, const double* R_est, const double* t_est,
                               const double* R_gt, const double* t_gt, void* workspace, double* out) {
  return tile_mean_launch(ctx, "pp_pose_add_f64", pose_add_kernel, n_pose, n_pts, workspace, out, pts, R_est, t_est, R_gt, t_gt);
}

extern "C" int pp_pose_adi_f64(pp_ctx* ctx, int n_pose, int n_pts, const double* pts, const double* R_est, const double* t_est,
                               const double* R_gt, const double* t_gt, void* workspace, double* out) {
  return tile_mean_launch(ctx, "pp_pose_adi_f64", pose_adi_kernel, n_pose, n_pts, workspace, out, pts, R_est, t_est, R_gt, t_gt);
}

extern "C" int pp_pose_reproj_f64(pp_ctx* ctx, int n_pose, int n_pts, const double* pts, const double* K9, const double* R_est,
                                  const double* t_est, const double* R_gt, const double* t_gt, void* workspace, double* out) {
  return tile_mean_launch(ctx, "pp_pose_reproj_f64", pose_reproj_kernel, n_pose, n_pts, workspace, out, pts, K9, R_est, t_est, R_gt, t_gt);
}

// ---- MSSD / MSPD ------------------------------------------------------------------------------------------------------
// grid (point ranges of POSE_SYM_RANGE, chunks of POSE_SYM_CHUNK symmetries, poses): a workgroup composes its chunk's G_s into
// LDS, every thread walks its range with stride POSE_TILE, transforms each point by the estimate once and keeps one running
// maximum of the SQUARED distance per symmetry of the chunk; partial[pose][range][s] = the workgroup's maximum.
#define POSE_SYM_CHUNK 8
#define POSE_SYM_RANGE 2048
#define POSE_SYM_MAX_SYM (POSE_SYM_CHUNK * 65535)

// project_f32 from the camera-frame point on, kept in float64
__device__ __forceinline__ void pixel(const double* __restrict__ K, double X, double Y, double Z, double* u, double* v) {
  const double a = K[0] * X + K[1] * Y + K[2] * Z, b = K[3] * X + K[4] * Y + K[5] * Z, w = K[6] * X + K[7] * Y + K[8] * Z;
  *u = a / w;
  *v = b / w;
}

template <bool PROJ>
__global__ void __launch_bounds__(POSE_TILE)
pose_sym_kernel(int n_pts, int n_sym, const double* __restrict__ pts, const double* __restrict__ S_R, const double* __restrict__ S_t,
                const double* __restrict__ K9, const double* __restrict__ R_est, const double* __restrict__ t_est,
                const double* __restrict__ R_gt, const double* __restrict__ t_gt, double* __restrict__ partial) {
  __shared__ double G[POSE_SYM_CHUNK][12];  // R row-major, then t
  __shared__ double red[POSE_SYM_CHUNK * (POSE_TILE / 64)];
  const int tid = threadIdx.x, range = blockIdx.x, s0 = blockIdx.y * POSE_SYM_CHUNK, pose = blockIdx.z;
  const int ns = min(POSE_SYM_CHUNK, n_sym - s0);  // >= 1: the grid has ceil(n_sym / POSE_SYM_CHUNK) chunks
  if (tid < ns) {
    const double *Rg = R_gt + 9 * pose, *tg = t_gt + 3 * pose, *Sr = S_R + 9 * (size_t)(s0 + tid), *St = S_t + 3 * (size_t)(s0 + tid);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) G[tid][3 * r + c] = Rg[3 * r] * Sr[c] + Rg[3 * r + 1] * Sr[3 + c] + Rg[3 * r + 2] * Sr[6 + c];
      G[tid][9 + r] = (Rg[3 * r] * St[0] + Rg[3 * r + 1] * St[1] + Rg[3 * r + 2] * St[2]) + tg[r];
    }
  }
  __syncthreads();
  const double* K = PROJ ? K9 + 9 * pose : nullptr;
  const int i0 = range * POSE_SYM_RANGE, cnt = min(POSE_SYM_RANGE, n_pts - i0);
  double m[POSE_SYM_CHUNK];
#pragma unroll
  for (int k = 0; k < POSE_SYM_CHUNK; ++k) m[k] = 0.0;
  for (int j = tid; j < cnt; j += POSE_TILE) {
    const size_t i = (size_t)i0 + j;
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    double ax, ay, az, au = 0.0, av = 0.0;
    rigid(R_est + 9 * pose, t_est + 3 * pose, x, y, z, &ax, &ay, &az);
    if (PROJ) pixel(K, ax, ay, az, &au, &av);
#pragma unroll
    for (int k = 0; k < POSE_SYM_CHUNK; ++k) {
      if (k < ns) {  // uniform over the workgroup
        double bx, by, bz, q;
        rigid(G[k], G[k] + 9, x, y, z, &bx, &by, &bz);
        if (PROJ) {
          double bu, bv;
          pixel(K, bx, by, bz, &bu, &bv);
          const double du = au - bu, dv = av - bv;
          q = du * du + dv * dv;
        } else {
          const double dx = ax - bx, dy = ay - by, dz = az - bz;
          q = dx * dx + dy * dy + dz * dz;
        }
        m[k] = q > m[k] ? q : m[k];
      }
    }
  }
  tile_max256(m, red);
#pragma unroll
  for (int k = 0; k < POSE_SYM_CHUNK; ++k)
    if (tid == k && k < ns) partial[((size_t)pose * gridDim.x + range) * n_sym + s0 + k] = m[k];
}

// one workgroup per pose: per symmetry the maximum over the ranges and its square root, then the smallest distance and the
// lowest index that attains it (np.argmin)
__global__ void __launch_bounds__(POSE_TILE)
pose_sym_finish_kernel(int n_ranges, int n_sym, const double* __restrict__ partial, double* __restrict__ out, int* __restrict__ best_sym) {
  __shared__ double rd[POSE_TILE];
  __shared__ int ri[POSE_TILE];
  const int tid = threadIdx.x, pose = blockIdx.x, none = 0x7fffffff;
  const double* p = partial + (size_t)pose * n_ranges * n_sym;
  double bd = __builtin_inf();
  int bi = none;
  for (int s = tid; s < n_sym; s += POSE_TILE) {
    double m = p[s];
    for (int r = 1; r < n_ranges; ++r) {
      const double u = p[(size_t)r * n_sym + s];
      m = u > m ? u : m;
    }
    const double d = sqrt(m);
    if (bi == none || d < bd) {
      bd = d;
      bi = s;
    }
  }
  rd[tid] = bd;
  ri[tid] = bi;
  __syncthreads();
  for (int st = POSE_TILE / 2; st > 0; st >>= 1) {
    if (tid < st) {
      const double od = rd[tid + st];
      const int oi = ri[tid + st];
      if (od < rd[tid] || (od == rd[tid] && oi < ri[tid])) {
        rd[tid] = od;
        ri[tid] = oi;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[pose] = rd[0];
    if (best_sym) best_sym[pose] = ri[0];
  }
}

extern "C" size_t pp_pose_sym_workspace_bytes(int n_pose, int n_pts, int n_sym) {
  if (n_pose <= 0 || n_pts <= 0 || n_sym <= 0) return 0;
  return (size_t)n_pose * ((n_pts + POSE_SYM_RANGE - 1) / POSE_SYM_RANGE) * n_sym * sizeof(double);
}

template <bool PROJ>
static int pose_sym_launch(pp_ctx* ctx, const char* who, int n_pose, int n_pts, int n_sym, const double* pts, const double* S_R,
                           const double* S_t, const double* K9, const double* R_est, const double* t_est, const double* R_gt,
                           const double* t_gt, void* workspace, double* out, int* best_sym) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n_pose > 0 && n_pose <= 65535 && n_pts > 0 && n_sym > 0 && n_sym <= POSE_SYM_MAX_SYM, PP_ERR_SHAPE,
               "%s: need 1..65535 poses, at least one model point and 1..%d symmetries", who, POSE_SYM_MAX_SYM);
  PP_CHECK_ARG(ctx, pts && S_R && S_t && (K9 || !PROJ) && R_est && t_est && R_gt && t_gt && workspace && out, PP_ERR_ARG, "%s: null argument", who);
  const int ranges = (int)(((long long)n_pts + POSE_SYM_RANGE - 1) / POSE_SYM_RANGE), chunks = (n_sym + POSE_SYM_CHUNK - 1) / POSE_SYM_CHUNK;
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(pose_sym_kernel<PROJ>, dim3(ranges, chunks, n_pose), dim3(POSE_TILE), 0, ctx->stream, n_pts, n_sym, pts, S_R, S_t, K9,
                     R_est, t_est, R_gt, t_gt, partial);
  hipLaunchKernelGGL(pose_sym_finish_kernel, dim3(n_pose), dim3(POSE_TILE), 0, ctx->stream, ranges, n_sym, (const double*)partial, out, best_sym);
  PP_CHECK_LAUNCH(ctx, who);
  return PP_OK;
}

extern "C" int pp_pose_mssd_f64(pp_ctx* ctx, int n_pose, int n_pts, int n_sym, const double* pts, const double* S_R, const double* S_t,
                                const double* R_est, const double* t_est, const double* R_gt, const double* t_gt, void* workspace,
                                double* out, int* best_sym) {
  return pose_sym_launch<false>(ctx, "pp_pose_mssd_f64", n_pose, n_pts, n_sym, pts, S_R, S_t, nullptr, R_est, t_est, R_gt, t_gt, workspace,
                                out, best_sym);
}

extern "C" int pp_pose_mspd_f64(pp_ctx* ctx, int n_pose, int n_pts, int n_sym, const double* pts, const double* S_R, const double* S_t,
                                const double* K9, const double* R_est, const double* t_est, const double* R_gt, const double* t_gt,
                                void* workspace, double* out, int* best_sym) {
  return pose_sym_launch<true>(ctx, "pp_pose_mspd_f64", n_pose, n_pts, n_sym, pts, S_R, S_t, K9, R_est, t_est, R_gt, t_gt, workspace, out,
                               best_sym);
}
