// Pose-error metrics of the evaluation tail: ADD and ADD-S/ADI (utils/pose_error.py:210-246, called at
// utils/linemod_eval.py:525-531 with the decision err < 0.1 * diameter) and the reprojection error (pose_error.py:179-207,
// tless_eval.py:651-662).  float64 like the reference's numpy.
//   ADD = mean_i || (R_est p_i + t_est) - (R_gt p_i + t_gt) ||
//   ADI = mean_i  min_j || (R_gt p_i + t_gt) - (R_est p_j + t_est) ||     (cKDTree(pts_est).query(pts_gt, k=1))
//   reproj = mean_i || proj(K, R_est, t_est, p_i) - proj(K, R_gt, t_gt, p_i) ||   (float32 pixels and norm)
// Reductions are fixed-order (per-tile partial sums, then one pass over the tiles): results do not depend on timing.
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
