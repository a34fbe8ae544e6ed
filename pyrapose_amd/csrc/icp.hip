// ICP refinement of estimated poses against scene depth: the block of PyraPose_ROS_wrapper/scripts/pyrapose_node.py:run_estimation
// (:662-756, same block at utils/ycbv_eval.py:424-526, 812-896 and the get_evaluation* helpers of tless_eval.py:23-65).
//
//   cloud:   create_point_cloud (pyrapose_node.py:170-189) with the class mask applied (PIL-nearest upsampled through index
//            maps, :602-604) and invalid depth dropped: count per row, exclusive scan over the rows, scatter in row-major order.
//   voxel:   Open3D voxel_down_sample: key of floor((p - (min_bound - v/2)) / v); the caller sorts the keys stably (plumbing),
//            then one thread per voxel sums its points (and normals) in original point order and divides.
//   normals: Open3D estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)): brute-force neighbours through LDS tiles, the
//            max_nn nearest within radius (ties to the lower index), float64 covariance, eigenvector of its smallest
//            eigenvalue by cyclic Jacobi sweeps, oriented toward the camera (n . p < 0); fewer than 3 neighbours: zero normal.
//   icp:     Open3D registration_icp for a batch of problems: per pass one launch over (source tile, problem) finds the nearest
//            target of every transformed source point and writes per-tile partial sums (wave shuffles, then the waves in
//            order), one launch per problem sums the tiles in order, evaluates fitness / inlier_rmse, tests convergence and
//            solves the update.  The host issues max_iteration + 1 pairs without synchronising; a finished problem's blocks
//            exit at once.  No grid barrier and no inter-workgroup flags.
// Compiled with -ffp-contract=off: tests/icp_np.py evaluates the same expressions in the same order.
#include <float.h>
#include <math.h>
#include "pose_common.h"

#define CLOUD_THREADS 256
#define VOX_THREADS 256
#define NRM_THREADS 64       // one wave; per-thread neighbour lists live in LDS
#define NRM_MAXNN 32
#define NRM_SWEEPS 6
#define ICP_TILE 128         // source points per workgroup (two waves)
#define ICP_NV 29            // partial sums per tile: plane 21 JTJ + 6 JTr + count + SSE; point 3 + 3 + 9 (+ 12 unused) + count + SSE
#define ICP_STRIDE 32
#define ICP_SWEEPS 10

// ---- point cloud from depth ----------------------------------------------------------------------------------------------

__device__ __forceinline__ bool cloud_pixel(const float* __restrict__ depth, const unsigned char* __restrict__ mask, int mask_w,
                                            const int* __restrict__ row_idx, const int* __restrict__ col_idx, int width, int r, int c,
                                            double ds, double* z) {
  *z = (double)depth[(size_t)r * width + c] * ds;
  if (mask && mask[(size_t)row_idx[r] * mask_w + col_idx[c]] == 0) return false;
  return isfinite(*z) && *z != 0.0;
}

__global__ void __launch_bounds__(CLOUD_THREADS)
cloud_count_kernel(int width, const float* __restrict__ depth, const unsigned char* __restrict__ mask, int mask_w,
                   const int* __restrict__ row_idx, const int* __restrict__ col_idx, double ds, int* __restrict__ row_cnt) {
  __shared__ int red[CLOUD_THREADS];
  const int r = blockIdx.x, tid = threadIdx.x;
  int n = 0;
  for (int c = tid; c < width; c += CLOUD_THREADS) {
    double z;
    n += cloud_pixel(depth, mask, mask_w, row_idx, col_idx, width, r, c, ds, &z) ? 1 : 0;
  }
  red[tid] = n;
  __syncthreads();
  for (int s = CLOUD_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) row_cnt[r] = red[0];
}

// create_point_cloud's expressions: x = ((c - cx) z) / fx, y = ((r - cy) z) / fy
__device__ __forceinline__ void back_project(int r, int c, double z, double fx, double fy, double cx, double cy, double* out) {
  out[0] = (((double)c - cx) * z) / fx;
  out[1] = (((double)r - cy) * z) / fy;
  out[2] = z;
}

// compact: the valid pixels of row r at offsets[r] in column order (a 256-wide inclusive scan per chunk)
__global__ void __launch_bounds__(CLOUD_THREADS)
cloud_scatter_kernel(int width, const float* __restrict__ depth, const unsigned char* __restrict__ mask, int mask_w,
                     const int* __restrict__ row_idx, const int* __restrict__ col_idx, double fx, double fy, double cx, double cy,
                     double ds, const int* __restrict__ offsets, double* __restrict__ pts) {
  __shared__ int s[CLOUD_THREADS];
  const int r = blockIdx.x, tid = threadIdx.x;
  int base = offsets[r];
  for (int c0 = 0; c0 < width; c0 += CLOUD_THREADS) {
    const int c = c0 + tid;
    double z = 0.0;
    const int f = (c < width && cloud_pixel(depth, mask, mask_w, row_idx, col_idx, width, r, c, ds, &z)) ? 1 : 0;
    s[tid] = f;
    __syncthreads();
    for (int off = 1; off < CLOUD_THREADS; off <<= 1) {
      const int u = tid >= off ? s[tid - off] : 0;
      __syncthreads();
      s[tid] += u;
      __syncthreads();
    }
    if (f) back_project(r, c, z, fx, fy, cx, cy, pts + 3 * (size_t)(base + s[tid] - 1));
    const int total = s[CLOUD_THREADS - 1];
    __syncthreads();
    base += total;
  }
}

// dense: every pixel at its own index, a NaN row where z == 0 (pyrapose_node.py:186); no mask
__global__ void cloud_dense_kernel(int width, int hw, const float* __restrict__ depth, double fx, double fy, double cx, double cy,
                                   double ds, double* __restrict__ pts) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= hw) return;
  const int r = p / width, c = p - r * width;
  const double z = (double)depth[p] * ds;
  double* o = pts + 3 * (size_t)p;
  if (z == 0.0) {
    o[0] = o[1] = o[2] = __longlong_as_double(0x7FF8000000000000LL);
  } else {
    back_project(r, c, z, fx, fy, cx, cy, o);
  }
}

extern "C" size_t pp_cloud_from_depth_workspace_bytes(int height, int width) {
  if (height <= 0 || width <= 0) return 0;
  return pp_align256((size_t)height * sizeof(int));
}

extern "C" int pp_cloud_from_depth_f64(pp_ctx* ctx, int height, int width, const float* depth, const unsigned char* mask, int mask_h,
                                       int mask_w, const int* row_idx, const int* col_idx, double fx, double fy, double cx, double cy,
                                       double ds, int dense, void* workspace, double* pts, int* row_offsets) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, height > 0 && width > 0 && height <= 65535 && width <= 65535 && (long long)height * width <= 0x7FFFFFFFLL / 3,
               PP_ERR_SHAPE, "pp_cloud_from_depth_f64: need a non-empty image of at most 65535 x 65535 pixels");
  PP_CHECK_ARG(ctx, depth && pts, PP_ERR_ARG, "pp_cloud_from_depth_f64: null argument");
  PP_CHECK_ARG(ctx, fx != 0.0 && fy != 0.0 && isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy) && isfinite(ds), PP_ERR_ARG,
               "pp_cloud_from_depth_f64: need finite intrinsics with fx, fy != 0 and a finite ds");
  if (dense) {
    const int hw = height * width;
    hipLaunchKernelGGL(cloud_dense_kernel, dim3((hw + 255) / 256), dim3(256), 0, ctx->stream, width, hw, depth, fx, fy, cx, cy, ds, pts);
    PP_CHECK_LAUNCH(ctx, "pp_cloud_from_depth_f64");
    return PP_OK;
  }
  PP_CHECK_ARG(ctx, workspace && row_offsets, PP_ERR_ARG, "pp_cloud_from_depth_f64: null workspace or row_offsets");
  PP_CHECK_ARG(ctx, !mask || (mask_h > 0 && mask_w > 0 && row_idx && col_idx), PP_ERR_ARG,
               "pp_cloud_from_depth_f64: a mask needs its shape and the row / column index maps");
  int* row_cnt = (int*)workspace;
  hipLaunchKernelGGL(cloud_count_kernel, dim3(height), dim3(CLOUD_THREADS), 0, ctx->stream, width, depth, mask, mask_w, row_idx, col_idx,
                     ds, row_cnt);
  hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, height, (const int*)row_cnt, row_offsets, (int*)nullptr);
  hipLaunchKernelGGL(cloud_scatter_kernel, dim3(height), dim3(CLOUD_THREADS), 0, ctx->stream, width, depth, mask, mask_w, row_idx, col_idx,
                     fx, fy, cx, cy, ds, (const int*)row_offsets, pts);
  PP_CHECK_LAUNCH(ctx, "pp_cloud_from_depth_f64");
  return PP_OK;
}

// ---- voxel down-sampling ---------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(VOX_THREADS) voxel_bound_kernel(int n, const double* __restrict__ pts, double* __restrict__ lo) {
  __shared__ double red[3][VOX_THREADS];
  const int tid = threadIdx.x;
  double m0 = DBL_MAX, m1 = DBL_MAX, m2 = DBL_MAX;
  for (int i = tid; i < n; i += VOX_THREADS) {
    m0 = fmin(m0, pts[3 * (size_t)i]);
    m1 = fmin(m1, pts[3 * (size_t)i + 1]);
    m2 = fmin(m2, pts[3 * (size_t)i + 2]);
  }
  red[0][tid] = m0;
  red[1][tid] = m1;
  red[2][tid] = m2;
  __syncthreads();
  for (int s = VOX_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] = fmin(red[0][tid], red[0][tid + s]);
      red[1][tid] = fmin(red[1][tid], red[1][tid + s]);
      red[2][tid] = fmin(red[2][tid], red[2][tid + s]);
    }
    __syncthreads();
  }
  if (tid < 3) lo[tid] = red[tid][0];
}

// key = ix << 42 | iy << 21 | iz (ascending key = ascending (ix, iy, iz)); an index outside [0, 2^21) gives key -1
__global__ void voxel_key_kernel(int n, const double* __restrict__ pts, double voxel, const double* __restrict__ lo,
                                 long long* __restrict__ keys) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long long key = 0;
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double ref = (pts[3 * (size_t)i + a] - (lo[a] - voxel * 0.5)) / voxel;
    const double f = floor(ref);
    ok = ok && f >= 0.0 && f < 2097152.0;
    key = (key << 21) | (ok ? (long long)f : 0);
  }
  keys[i] = ok ? key : -1;
}

// one thread per voxel: its points perm[seg[v] .. seg[v+1]) summed in that (original point) order, then divided
__global__ void voxel_mean_kernel(int n_vox, const double* __restrict__ pts, const double* __restrict__ nrm,
                                  const long long* __restrict__ perm, const long long* __restrict__ seg, double* __restrict__ out_pts,
                                  double* __restrict__ out_nrm) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_vox) return;
  const long long k0 = seg[v], k1 = seg[v + 1];
  double p0 = 0.0, p1 = 0.0, p2 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0;
  for (long long k = k0; k < k1; ++k) {
    const long long i = perm[k];
    p0 += pts[3 * i];
    p1 += pts[3 * i + 1];
    p2 += pts[3 * i + 2];
    if (nrm) {
      q0 += nrm[3 * i];
      q1 += nrm[3 * i + 1];
      q2 += nrm[3 * i + 2];
    }
  }
  const double cnt = (double)(k1 - k0);
  out_pts[3 * (size_t)v] = p0 / cnt;
  out_pts[3 * (size_t)v + 1] = p1 / cnt;
  out_pts[3 * (size_t)v + 2] = p2 / cnt;
  if (nrm) {
    const double len = sqrt((q0 * q0 + q1 * q1) + q2 * q2);
    out_nrm[3 * (size_t)v] = len > 0.0 ? q0 / len : 0.0;
    out_nrm[3 * (size_t)v + 1] = len > 0.0 ? q1 / len : 0.0;
    out_nrm[3 * (size_t)v + 2] = len > 0.0 ? q2 / len : 0.0;
  }
}

extern "C" size_t pp_voxel_workspace_bytes(int n) { return n > 0 ? 256 : 0; }

extern "C" int pp_voxel_keys_f64(pp_ctx* ctx, int n, const double* pts, double voxel, void* workspace, long long* keys) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n > 0, PP_ERR_SHAPE, "pp_voxel_keys_f64: need at least one point");
  PP_CHECK_ARG(ctx, pts && workspace && keys, PP_ERR_ARG, "pp_voxel_keys_f64: null argument");
  PP_CHECK_ARG(ctx, voxel > 0.0 && isfinite(voxel), PP_ERR_ARG, "pp_voxel_keys_f64: voxel size must be positive");
  double* lo = (double*)workspace;
  hipLaunchKernelGGL(voxel_bound_kernel, dim3(1), dim3(VOX_THREADS), 0, ctx->stream, n, pts, lo);
  hipLaunchKernelGGL(voxel_key_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, pts, voxel, (const double*)lo, keys);
  PP_CHECK_LAUNCH(ctx, "pp_voxel_keys_f64");
  return PP_OK;
}

extern "C" int pp_voxel_means_f64(pp_ctx* ctx, int n, const double* pts, const double* normals, const long long* perm, int n_vox,
                                  const long long* seg, double* out_pts, double* out_normals) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n > 0 && n_vox > 0 && n_vox <= n, PP_ERR_SHAPE, "pp_voxel_means_f64: need 1 <= n_vox <= n");
  PP_CHECK_ARG(ctx, pts && perm && seg && out_pts && (!normals || out_normals), PP_ERR_ARG, "pp_voxel_means_f64: null argument");
  hipLaunchKernelGGL(voxel_mean_kernel, dim3((n_vox + 255) / 256), dim3(256), 0, ctx->stream, n_vox, pts, normals, perm, seg, out_pts,
                     out_normals);
  PP_CHECK_LAUNCH(ctx, "pp_voxel_means_f64");
  return PP_OK;
}

// ---- normals ---------------------------------------------------------------------------------------------------------------

// one Jacobi rotation of the symmetric N x N matrix a, zeroing a[P][Q]; v accumulates the rotations (columns = eigenvectors)
template <int N, int P, int Q>
__device__ __forceinline__ void jacobi_rot(double (&a)[N][N], double (&v)[N][N]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[P][P] = a[P][P] - t * apq;
  a[Q][Q] = a[Q][Q] + t * apq;
  a[P][Q] = 0.0;
  a[Q][P] = 0.0;
#pragma unroll
  for (int r = 0; r < N; ++r) {
    if (r == P || r == Q) continue;
    const double arp = a[r][P], arq = a[r][Q];
    a[r][P] = c * arp - s * arq;
    a[P][r] = a[r][P];
    a[r][Q] = s * arp + c * arq;
    a[Q][r] = a[r][Q];
  }
#pragma unroll
  for (int r = 0; r < N; ++r) {
    const double vp = v[r][P], vq = v[r][Q];
    v[r][P] = c * vp - s * vq;
    v[r][Q] = s * vp + c * vq;
  }
}

__device__ __forceinline__ void jacobi3(double (&a)[3][3], double (&v)[3][3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < NRM_SWEEPS; ++sweep) {
    jacobi_rot<3, 0, 1>(a, v);
    jacobi_rot<3, 0, 2>(a, v);
    jacobi_rot<3, 1, 2>(a, v);
  }
}

__global__ void __launch_bounds__(NRM_THREADS)
normals_kernel(int n, const double* __restrict__ pts, double r2, int max_nn, double* __restrict__ normals, int* __restrict__ nbr) {
  __shared__ double tx[NRM_THREADS], ty[NRM_THREADS], tz[NRM_THREADS];
  __shared__ double ld[NRM_MAXNN][NRM_THREADS];
  __shared__ int li[NRM_MAXNN][NRM_THREADS];
  const int tid = threadIdx.x, i = blockIdx.x * NRM_THREADS + tid;
  const bool active = i < n;
  const double px = active ? pts[3 * (size_t)i] : 0.0, py = active ? pts[3 * (size_t)i + 1] : 0.0, pz = active ? pts[3 * (size_t)i + 2] : 0.0;
  int cnt = 0;
  for (int j0 = 0; j0 < n; j0 += NRM_THREADS) {
    __syncthreads();
    if (j0 + tid < n) {
      tx[tid] = pts[3 * (size_t)(j0 + tid)];
      ty[tid] = pts[3 * (size_t)(j0 + tid) + 1];
      tz[tid] = pts[3 * (size_t)(j0 + tid) + 2];
    }
    __syncthreads();
    const int lim = min(NRM_THREADS, n - j0);
    for (int k = 0; k < lim; ++k) {
      const double dx = px - tx[k], dy = py - ty[k], dz = pz - tz[k];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (!(d2 <= r2)) continue;
      int pos;
      if (cnt < max_nn) {
        pos = cnt++;
      } else if (d2 < ld[max_nn - 1][tid]) {
        pos = max_nn - 1;
      } else {
        continue;
      }
      while (pos > 0 && ld[pos - 1][tid] > d2) {
        ld[pos][tid] = ld[pos - 1][tid];
        li[pos][tid] = li[pos - 1][tid];
        --pos;
      }
      ld[pos][tid] = d2;
      li[pos][tid] = j0 + k;
    }
  }
  if (!active) return;
  if (nbr)
    for (int k = 0; k < max_nn; ++k) nbr[(size_t)i * max_nn + k] = k < cnt ? li[k][tid] : -1;
  double* o = normals + 3 * (size_t)i;
  if (cnt < 3) {
    o[0] = o[1] = o[2] = 0.0;
    return;
  }
  double m0 = 0.0, m1 = 0.0, m2 = 0.0;
  for (int k = 0; k < cnt; ++k) {
    const int j = li[k][tid];
    m0 += pts[3 * (size_t)j];
    m1 += pts[3 * (size_t)j + 1];
    m2 += pts[3 * (size_t)j + 2];
  }
  const double inv = 1.0 / (double)cnt;
  m0 *= inv;
  m1 *= inv;
  m2 *= inv;
  double a[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  for (int k = 0; k < cnt; ++k) {
    const int j = li[k][tid];
    const double d[3] = {pts[3 * (size_t)j] - m0, pts[3 * (size_t)j + 1] - m1, pts[3 * (size_t)j + 2] - m2};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = r; c < 3; ++c) a[r][c] += d[r] * d[c];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = r; c < 3; ++c) {
      a[r][c] *= inv;
      a[c][r] = a[r][c];
    }
  double v[3][3];
  jacobi3(a, v);
  // the smallest eigenvalue, the first of equals
  const int k = (a[1][1] < a[0][0]) ? ((a[2][2] < a[1][1]) ? 2 : 1) : ((a[2][2] < a[0][0]) ? 2 : 0);
  double nx = k == 0 ? v[0][0] : (k == 1 ? v[0][1] : v[0][2]);
  double ny = k == 0 ? v[1][0] : (k == 1 ? v[1][1] : v[1][2]);
  double nz = k == 0 ? v[2][0] : (k == 1 ? v[2][1] : v[2][2]);
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  nx /= len;
  ny /= len;
  nz /= len;
  if ((nx * px + ny * py) + nz * pz > 0.0) {
    nx = -nx;
    ny = -ny;
    nz = -nz;
  }
  o[0] = nx;
  o[1] = ny;
  o[2] = nz;
}

extern "C" size_t pp_estimate_normals_workspace_bytes(int n, int max_nn) {
  (void)n;
  (void)max_nn;
  return 0;
}

extern "C" int pp_estimate_normals_f64(pp_ctx* ctx, int n, const double* pts, double radius, int max_nn, void* workspace, double* normals,
                                       int* neighbors) {
  (void)workspace;
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n > 0, PP_ERR_SHAPE, "pp_estimate_normals_f64: need at least one point");
  PP_CHECK_ARG(ctx, pts && normals, PP_ERR_ARG, "pp_estimate_normals_f64: null argument");
  PP_CHECK_ARG(ctx, radius > 0.0 && isfinite(radius) && max_nn >= 1 && max_nn <= NRM_MAXNN, PP_ERR_ARG,
               "pp_estimate_normals_f64: need radius > 0 and 1 <= max_nn <= %d", NRM_MAXNN);
  hipLaunchKernelGGL(normals_kernel, dim3((n + NRM_THREADS - 1) / NRM_THREADS), dim3(NRM_THREADS), 0, ctx->stream, n, pts, radius * radius,
                     max_nn, normals, neighbors);
  PP_CHECK_LAUNCH(ctx, "pp_estimate_normals_f64");
  return PP_OK;
}

// ---- ICP -------------------------------------------------------------------------------------------------------------------

struct icp_state {
  double R[9], t[3];
  double fitness, rmse;
  int iters, status, done, pad;
};

__global__ void icp_init_kernel(int P, const int* __restrict__ so, const int* __restrict__ to, const double* __restrict__ init,
                                icp_state* __restrict__ st) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  icp_state s;
  const double* T = init + 16 * p;  // row-major 4x4
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) s.R[3 * r + c] = T[4 * r + c];
    s.t[r] = T[4 * r + 3];
  }
  s.fitness = 0.0;
  s.rmse = 0.0;
  s.iters = 0;
  s.pad = 0;
  const bool empty = so[p + 1] <= so[p] || to[p + 1] <= to[p];
  s.status = empty ? PP_ICP_TOO_FEW : PP_ICP_OK;
  s.done = empty ? 1 : 0;
  st[p] = s;
}

// grid (source tiles, problems): nearest target of each transformed source point, per-tile partial sums
__global__ void __launch_bounds__(ICP_TILE)
icp_corr_kernel(int max_tiles, const int* __restrict__ so, const int* __restrict__ to, const double* __restrict__ src,
                const double* __restrict__ tgt, const double* __restrict__ tgt_n, double max_d2, int plane, const icp_state* __restrict__ st,
                int* __restrict__ corr, double* __restrict__ partial) {
  __shared__ double lx[ICP_TILE], ly[ICP_TILE], lz[ICP_TILE];
  __shared__ double red[ICP_TILE / 64][ICP_NV];
  const int p = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const int s0 = so[p], s1 = so[p + 1];
  if (s0 + tile * ICP_TILE >= s1) return;
  if (st[p].done) return;
  const double* R = st[p].R;
  const double* T = st[p].t;
  const int i = s0 + tile * ICP_TILE + tid;
  const bool active = i < s1;
  double x = 0.0, y = 0.0, z = 0.0;
  if (active) {
    const double a = src[3 * (size_t)i], b = src[3 * (size_t)i + 1], c = src[3 * (size_t)i + 2];
    x = ((R[0] * a + R[1] * b) + R[2] * c) + T[0];
    y = ((R[3] * a + R[4] * b) + R[5] * c) + T[1];
    z = ((R[6] * a + R[7] * b) + R[8] * c) + T[2];
  }
  const int t0 = to[p], t1 = to[p + 1];
  double best = DBL_MAX;
  int bj = -1;
  for (int j0 = t0; j0 < t1; j0 += ICP_TILE) {
    __syncthreads();
    const int j = j0 + tid;
    if (j < t1) {
      // point-to-plane: a target without a normal is never a correspondence
      const bool use = !plane || tgt_n[3 * (size_t)j] != 0.0 || tgt_n[3 * (size_t)j + 1] != 0.0 || tgt_n[3 * (size_t)j + 2] != 0.0;
      lx[tid] = use ? tgt[3 * (size_t)j] : INFINITY;
      ly[tid] = use ? tgt[3 * (size_t)j + 1] : INFINITY;
      lz[tid] = use ? tgt[3 * (size_t)j + 2] : INFINITY;
    }
    __syncthreads();
    const int lim = min(ICP_TILE, t1 - j0);
    for (int k = 0; k < lim; ++k) {
      const double dx = x - lx[k], dy = y - ly[k], dz = z - lz[k];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 < best) {
        best = d2;
        bj = j0 + k;
      }
    }
  }
  const bool ok = active && bj >= 0 && best <= max_d2;
  if (active) corr[i] = ok ? bj - t0 : -1;
  double v[ICP_NV];
#pragma unroll
  for (int k = 0; k < ICP_NV; ++k) v[k] = 0.0;
  if (ok) {
    const double qx = tgt[3 * (size_t)bj], qy = tgt[3 * (size_t)bj + 1], qz = tgt[3 * (size_t)bj + 2];
    if (plane) {
      const double nx = tgt_n[3 * (size_t)bj], ny = tgt_n[3 * (size_t)bj + 1], nz = tgt_n[3 * (size_t)bj + 2];
      const double j0 = y * nz - z * ny, j1 = z * nx - x * nz, j2 = x * ny - y * nx;
      const double r = ((x - qx) * nx + (y - qy) * ny) + (z - qz) * nz;
      // JTJ upper triangle row by row, then JTr (J = [j0 j1 j2 nx ny nz])
      v[0] = j0 * j0; v[1] = j0 * j1; v[2] = j0 * j2; v[3] = j0 * nx; v[4] = j0 * ny; v[5] = j0 * nz;
      v[6] = j1 * j1; v[7] = j1 * j2; v[8] = j1 * nx; v[9] = j1 * ny; v[10] = j1 * nz;
      v[11] = j2 * j2; v[12] = j2 * nx; v[13] = j2 * ny; v[14] = j2 * nz;
      v[15] = nx * nx; v[16] = nx * ny; v[17] = nx * nz;
      v[18] = ny * ny; v[19] = ny * nz;
      v[20] = nz * nz;
      v[21] = j0 * r; v[22] = j1 * r; v[23] = j2 * r; v[24] = nx * r; v[25] = ny * r; v[26] = nz * r;
    } else {
      v[0] = x; v[1] = y; v[2] = z; v[3] = qx; v[4] = qy; v[5] = qz;
      v[6] = x * qx; v[7] = x * qy; v[8] = x * qz;
      v[9] = y * qx; v[10] = y * qy; v[11] = y * qz;
      v[12] = z * qx; v[13] = z * qy; v[14] = z * qz;
    }
    v[27] = 1.0;
    v[28] = best;
  }
  // wave tree (lane l += lane l + off, off = 32 .. 1), then the waves in order
#pragma unroll
  for (int k = 0; k < ICP_NV; ++k)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < ICP_NV; ++k) red[wave][k] = v[k];
  __syncthreads();
  if (tid < ICP_NV) {
    double s = red[0][tid];
    for (int w = 1; w < ICP_TILE / 64; ++w) s += red[w][tid];
    partial[((size_t)p * max_tiles + tile) * ICP_STRIDE + tid] = s;
  }
}

__device__ __forceinline__ void jacobi4(double (&a)[4][4], double (&v)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) v[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < ICP_SWEEPS; ++sweep) {
    jacobi_rot<4, 0, 1>(a, v);
    jacobi_rot<4, 0, 2>(a, v);
    jacobi_rot<4, 0, 3>(a, v);
    jacobi_rot<4, 1, 2>(a, v);
    jacobi_rot<4, 1, 3>(a, v);
    jacobi_rot<4, 2, 3>(a, v);
  }
}

// point-to-point: the rotation of Horn's quaternion method (the top eigenvector of the 4x4 matrix built from the
// cross-covariance), which is Kabsch / Umeyama without scale with the reflection fix; t = q_mean - R s_mean
__device__ __forceinline__ bool solve_point(const double* S, double n, double* Ru, double* tu) {
  const double ms[3] = {S[0] / n, S[1] / n, S[2] / n}, mq[3] = {S[3] / n, S[4] / n, S[5] / n};
  double C[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) C[a][b] = S[6 + 3 * a + b] / n - ms[a] * mq[b];
  const double Sxx = C[0][0], Sxy = C[0][1], Sxz = C[0][2], Syx = C[1][0], Syy = C[1][1], Syz = C[1][2], Szx = C[2][0], Szy = C[2][1],
               Szz = C[2][2];
  double N[4][4] = {{(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy}};
  double V[4][4];
  jacobi4(N, V);
  // the largest eigenvalue, the first of equals
  int k = 0;
  double best = N[0][0];
  if (N[1][1] > best) { k = 1; best = N[1][1]; }
  if (N[2][2] > best) { k = 2; best = N[2][2]; }
  if (N[3][3] > best) { k = 3; best = N[3][3]; }
  double qw = k == 0 ? V[0][0] : (k == 1 ? V[0][1] : (k == 2 ? V[0][2] : V[0][3]));
  double qx = k == 0 ? V[1][0] : (k == 1 ? V[1][1] : (k == 2 ? V[1][2] : V[1][3]));
  double qy = k == 0 ? V[2][0] : (k == 1 ? V[2][1] : (k == 2 ? V[2][2] : V[2][3]));
  double qz = k == 0 ? V[3][0] : (k == 1 ? V[3][1] : (k == 2 ? V[3][2] : V[3][3]));
  const double len = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
  if (!(len > 0.0)) return false;
  qw /= len;
  qx /= len;
  qy /= len;
  qz /= len;
  Ru[0] = ((qw * qw + qx * qx) - qy * qy) - qz * qz;
  Ru[1] = 2.0 * (qx * qy - qw * qz);
  Ru[2] = 2.0 * (qx * qz + qw * qy);
  Ru[3] = 2.0 * (qx * qy + qw * qz);
  Ru[4] = ((qw * qw - qx * qx) + qy * qy) - qz * qz;
  Ru[5] = 2.0 * (qy * qz - qw * qx);
  Ru[6] = 2.0 * (qx * qz - qw * qy);
  Ru[7] = 2.0 * (qy * qz + qw * qx);
  Ru[8] = ((qw * qw - qx * qx) - qy * qy) + qz * qz;
#pragma unroll
  for (int a = 0; a < 3; ++a) tu[a] = mq[a] - ((Ru[3 * a] * ms[0] + Ru[3 * a + 1] * ms[1]) + Ru[3 * a + 2] * ms[2]);
  return true;
}

// point-to-plane: JTJ x = -JTr by LDL^T (a pivot <= 1e-12 x the largest diagonal entry is singular), then
// R = Rz(x2) Ry(x1) Rx(x0), t = x[3:6] (Open3D's TransformVector6dToMatrix4d)
__device__ __forceinline__ bool solve_plane(const double* S, double* Ru, double* tu) {
  double A[6][6], b[6];
#pragma unroll
  for (int r = 0, k = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c, ++k) {
      A[r][c] = S[k];
      A[c][r] = S[k];
    }
  double dmax = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    b[r] = -S[21 + r];
    dmax = fmax(dmax, A[r][r]);
  }
  double L[6][6], d[6];
  bool ok = dmax > 0.0;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
#pragma unroll
    for (int q = 0; q < j; ++q) s -= (L[j][q] * L[j][q]) * d[q];
    d[j] = s;
    ok = ok && s > 1e-12 * dmax;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double u = A[i][j];
#pragma unroll
      for (int q = 0; q < j; ++q) u -= (L[i][q] * L[j][q]) * d[q];
      L[i][j] = u / s;
    }
  }
  if (!ok) return false;
  double x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
#pragma unroll
    for (int q = 0; q < i; ++q) s -= L[i][q] * x[q];
    x[i] = s;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = x[i] / d[i];
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = x[i];
#pragma unroll
    for (int q = i + 1; q < 6; ++q) s -= L[q][i] * x[q];
    x[i] = s;
  }
  const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
  Ru[0] = cg * cb;
  Ru[1] = (cg * sb) * sa - sg * ca;
  Ru[2] = (cg * sb) * ca + sg * sa;
  Ru[3] = sg * cb;
  Ru[4] = (sg * sb) * sa + cg * ca;
  Ru[5] = (sg * sb) * ca - cg * sa;
  Ru[6] = -sb;
  Ru[7] = cb * sa;
  Ru[8] = cb * ca;
  tu[0] = x[3];
  tu[1] = x[4];
  tu[2] = x[5];
  return true;
}

// one thread per problem: the tiles' partials in tile order -> fitness / rmse, convergence test, update
__global__ void __launch_bounds__(64) icp_solve_kernel(int P, int max_tiles, int pass, int max_iteration, int plane, double rel_fitness, double rel_rmse,
                                 const int* __restrict__ so, const double* __restrict__ partial, icp_state* __restrict__ st) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  icp_state s = st[p];
  if (s.done) return;
  const int ns = so[p + 1] - so[p], tiles = min((ns + ICP_TILE - 1) / ICP_TILE, max_tiles);
  double S[ICP_NV];
#pragma unroll
  for (int k = 0; k < ICP_NV; ++k) S[k] = 0.0;
  for (int tl = 0; tl < tiles; ++tl) {
    const double* q = partial + ((size_t)p * max_tiles + tl) * ICP_STRIDE;
#pragma unroll
    for (int k = 0; k < ICP_NV; ++k) S[k] += q[k];
  }
  const double n = S[27];
  const double fitness = n / (double)ns, rmse = n > 0.0 ? sqrt(S[28] / n) : 0.0;
  const bool converged = pass > 0 && fabs(s.fitness - fitness) < rel_fitness && fabs(s.rmse - rmse) < rel_rmse;
  s.fitness = fitness;
  s.rmse = rmse;
  if (converged || pass >= max_iteration) {
    s.done = 1;
  } else if (n < (plane ? 6.0 : 3.0)) {
    s.status = PP_ICP_TOO_FEW;
    s.done = 1;
  } else {
    double Ru[9], tu[3];
    if (!(plane ? solve_plane(S, Ru, tu) : solve_point(S, n, Ru, tu))) {
      s.status = PP_ICP_SINGULAR;
      s.done = 1;
    } else {
      double R2[9], t2[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R2[3 * r + c] = (Ru[3 * r] * s.R[c] + Ru[3 * r + 1] * s.R[3 + c]) + Ru[3 * r + 2] * s.R[6 + c];
        t2[r] = ((Ru[3 * r] * s.t[0] + Ru[3 * r + 1] * s.t[1]) + Ru[3 * r + 2] * s.t[2]) + tu[r];
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) s.R[k] = R2[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) s.t[k] = t2[k];
      s.iters += 1;
    }
  }
  st[p] = s;
}

__global__ void icp_out_kernel(int P, const icp_state* __restrict__ st, double* __restrict__ R, double* __restrict__ t,
                               double* __restrict__ fitness, double* __restrict__ rmse, int* __restrict__ iters, int* __restrict__ status) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const icp_state s = st[p];
  for (int k = 0; k < 9; ++k) R[9 * p + k] = s.R[k];
  for (int k = 0; k < 3; ++k) t[3 * p + k] = s.t[k];
  fitness[p] = s.fitness;
  rmse[p] = s.rmse;
  iters[p] = s.iters;
  status[p] = s.status;
}

static size_t icp_layout(int P, int max_src, char* base, icp_state** st, double** partial) {
  const int max_tiles = (max_src + ICP_TILE - 1) / ICP_TILE;
  const size_t a = pp_align256((size_t)P * sizeof(icp_state));
  if (st) *st = (icp_state*)base;
  if (partial) *partial = (double*)(base + a);
  return a + pp_align256((size_t)P * max_tiles * ICP_STRIDE * sizeof(double));
}

extern "C" size_t pp_icp_workspace_bytes(int n_problems, int max_source_points) {
  if (n_problems <= 0 || n_problems > 65535 || max_source_points <= 0) return 0;
  return icp_layout(n_problems, max_source_points, nullptr, nullptr, nullptr);
}

extern "C" int pp_icp_f64(pp_ctx* ctx, int n_problems, const int* src_offsets, const int* tgt_offsets, int max_source_points,
                          const double* src, const double* tgt, const double* tgt_normals, const double* init,
                          double max_correspondence_distance, int max_iteration, double relative_fitness, double relative_rmse, int mode,
                          void* workspace, size_t workspace_bytes, double* R_out, double* t_out, double* fitness, double* inlier_rmse,
                          int* iterations, int* status, int* corr) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n_problems > 0 && n_problems <= 65535 && max_source_points > 0, PP_ERR_SHAPE,
               "pp_icp_f64: need 1..65535 problems and max_source_points > 0");
  PP_CHECK_ARG(ctx, src_offsets && tgt_offsets && src && tgt && init && workspace && R_out && t_out && fitness && inlier_rmse && iterations &&
                        status && corr, PP_ERR_ARG, "pp_icp_f64: null argument");
  PP_CHECK_ARG(ctx, mode == PP_ICP_POINT_TO_POINT || mode == PP_ICP_POINT_TO_PLANE, PP_ERR_ARG, "pp_icp_f64: unknown mode %d", mode);
  PP_CHECK_ARG(ctx, mode == PP_ICP_POINT_TO_POINT || tgt_normals, PP_ERR_ARG, "pp_icp_f64: point-to-plane needs target normals");
  PP_CHECK_ARG(ctx, max_correspondence_distance > 0.0 && isfinite(max_correspondence_distance) && max_iteration >= 0 &&
                        max_iteration <= 100000 && relative_fitness >= 0.0 && relative_rmse >= 0.0, PP_ERR_ARG,
               "pp_icp_f64: need max_correspondence_distance > 0, 0 <= max_iteration <= 100000 and non-negative relative thresholds");
  icp_state* st;
  double* partial;
  const size_t need = icp_layout(n_problems, max_source_points, (char*)workspace, &st, &partial);
  PP_CHECK_ARG(ctx, workspace_bytes >= need, PP_ERR_ARG, "pp_icp_f64: workspace of %zu bytes, need %zu", workspace_bytes, need);
  const int max_tiles = (max_source_points + ICP_TILE - 1) / ICP_TILE, plane = mode == PP_ICP_POINT_TO_PLANE;
  const double max_d2 = max_correspondence_distance * max_correspondence_distance;
  const dim3 pg((n_problems + 63) / 64);
  hipLaunchKernelGGL(icp_init_kernel, pg, dim3(64), 0, ctx->stream, n_problems, src_offsets, tgt_offsets, init, st);
  for (int pass = 0; pass <= max_iteration; ++pass) {
    hipLaunchKernelGGL(icp_corr_kernel, dim3(max_tiles, n_problems), dim3(ICP_TILE), 0, ctx->stream, max_tiles, src_offsets, tgt_offsets,
                       src, tgt, tgt_normals, max_d2, plane, (const icp_state*)st, corr, partial);
    hipLaunchKernelGGL(icp_solve_kernel, pg, dim3(64), 0, ctx->stream, n_problems, max_tiles, pass, max_iteration, plane, relative_fitness,
                       relative_rmse, src_offsets, (const double*)partial, st);
  }
  hipLaunchKernelGGL(icp_out_kernel, pg, dim3(64), 0, ctx->stream, n_problems, (const icp_state*)st, R_out, t_out, fitness, inlier_rmse,
                     iterations, status);
  PP_CHECK_LAUNCH(ctx, "pp_icp_f64");
  return PP_OK;
}
