// Model geometry the evaluation tail and the target assignment take as given: the diameter of a model's point set (what a BOP
// dataset's models_info.json calls 'diameter'; bop_toolkit's misc.calc_pts_diameter) and greedy farthest-point sampling of
// control points (the reference's offline FPS.py:37-94, and the standard min-distance rule).  float64 like their numpy.
//   d2(a, b) = (dx * dx + dy * dy) + dz * dz       with exactly that association (numpy's (diff * diff).sum(axis=1) on rows of 3)
//   diameter: max over i <= j of d2(p_i, p_j), the pair that attains it (lowest i, then lowest j); the root is the host's
//   farthest points: k greedy picks per model, argmax of a running score, the lowest index on ties
//   symmetry score: per candidate transformation S_k, max over i of min over j of d2(S_k p_i, q_j) -- the squared one-sided
//   Hausdorff distance of the moved source to the target -- and the (i, j) that attains it (lowest i, for it the lowest j)
// Maxima, minima and (rule 1) sums in the order chosen: results do not depend on timing.
// Compiled with -ffp-contract=off: products and sums are rounded one by one as written.
#include "pose_common.h"

#define DIAMETER_MAX_PTS (1 << 24)   // i and j fit 24 bits each: one 48-bit key orders the pairs
#define DIAMETER_MAX_CHUNKS 64       // chunks of j tiles per row of tiles at most: bounds the partials
#define FPS_THREADS 1024

__device__ __forceinline__ double dist2(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

// ---- diameter ---------------------------------------------------------------------------------------------------------
// Triangular tiling: tiles of POSE_TILE points; workgroup (bi, c) holds tile bi one point per thread in registers and sweeps
// the j tiles of chunk c (tiles [c * jc, (c + 1) * jc), from bi on) staged in LDS one at a time -- every lane reads the same
// address, a broadcast.  partial[c][bi] = the workgroup's (d2, i, j); a workgroup whose chunk lies left of the diagonal
// writes d2 = -1 (no pair).  Tail lanes (i >= n) hold no pair and tail points of a j tile are never read.

static inline int diameter_tiles(int n) { return (n + POSE_TILE - 1) / POSE_TILE; }
static inline int diameter_jc(int tiles) { return (tiles + DIAMETER_MAX_CHUNKS - 1) / DIAMETER_MAX_CHUNKS; }  // j tiles per chunk

// the workgroup's best (d2, lowest i, then lowest j) of per-thread candidates (d2 < 0: none), returned to every thread
__device__ __forceinline__ void best_pair256(double& d2, int& i, int& j, double* red, unsigned long long* key) {
  double m[1] = {d2};
  if (threadIdx.x == 0) *key = ~0ull;
  tile_max256(m, red);  // (its barriers order the reset of key before the minima below)
  if (d2 == m[0] && d2 >= 0.0) atomicMin(key, ((unsigned long long)(unsigned)i << 24) | (unsigned long long)(unsigned)j);
  __syncthreads();
  const unsigned long long k = *key == ~0ull ? 0ull : *key;  // (no candidate at all: d2 = -1 and the pair (0, 0))
  d2 = m[0];
  i = (int)(k >> 24);
  j = (int)(k & 0xffffffu);
  __syncthreads();
}

template <bool DIAG>
__device__ __forceinline__ void diameter_sweep(const double* __restrict__ s, int lim, int j0, int i, double x, double y, double z,
                                               double& best, int& bj) {
#pragma unroll 4
  for (int k = 0; k < lim; ++k) {
    const double q = dist2(x, y, z, s[3 * k], s[3 * k + 1], s[3 * k + 2]);
    const bool take = DIAG ? (q > best && j0 + k >= i) : q > best;  // rising j and a strict comparison: the lowest j stays
    best = take ? q : best;
    bj = take ? j0 + k : bj;
  }
}

__global__ void __launch_bounds__(POSE_TILE)
diameter_tile_kernel(int n, int tiles, int jc, const double* __restrict__ pts, double* __restrict__ part_d2, int2* __restrict__ part_ij) {
  __shared__ double s[3 * POSE_TILE];
  __shared__ double red[POSE_TILE / 64];
  __shared__ unsigned long long key;
  const int tid = threadIdx.x, bi = blockIdx.x, c = blockIdx.y;
  const int t_begin = max(bi, c * jc), t_end = min(tiles, (c + 1) * jc);
  const size_t slot = (size_t)c * tiles + bi;
  if (t_begin >= t_end) {  // uniform over the workgroup
    if (tid == 0) {
      part_d2[slot] = -1.0;
      part_ij[slot] = make_int2(0, 0);
    }
    return;
  }
  const int i = bi * POSE_TILE + tid;
  const bool mine = i < n;
  double x = 0.0, y = 0.0, z = 0.0;
  if (mine) {
    x = pts[3 * (size_t)i];
    y = pts[3 * (size_t)i + 1];
    z = pts[3 * (size_t)i + 2];
  }
  double best = -1.0;
  int bj = 0;
  for (int t = t_begin; t < t_end; ++t) {
    const int j0 = t * POSE_TILE, lim = min(POSE_TILE, n - j0);
    __syncthreads();
    for (int e = tid; e < 3 * lim; e += POSE_TILE) s[e] = pts[3 * (size_t)j0 + e];
    __syncthreads();
    if (mine) {
      if (t == bi)
        diameter_sweep<true>(s, lim, j0, i, x, y, z, best, bj);
      else
        diameter_sweep<false>(s, lim, j0, i, x, y, z, best, bj);
    }
  }
  int wi = i;
  best_pair256(best, wi, bj, red, &key);
  if (tid == 0) {
    part_d2[slot] = best;
    part_ij[slot] = make_int2(wi, bj);
  }
}

// one workgroup: the partials in a fixed order with the tie rule
__global__ void __launch_bounds__(POSE_TILE)
diameter_finish_kernel(long long n_part, const double* __restrict__ part_d2, const int2* __restrict__ part_ij, double* __restrict__ d2,
                       int* __restrict__ pair) {
  __shared__ double red[POSE_TILE / 64];
  __shared__ unsigned long long key;
  double best = -1.0;
  int bi = 0, bj = 0;
  for (long long p = threadIdx.x; p < n_part; p += POSE_TILE) {
    const double q = part_d2[p];
    const int2 ij = part_ij[p];
    if (q > best || (q == best && q >= 0.0 && (ij.x < bi || (ij.x == bi && ij.y < bj)))) {
      best = q;
      bi = ij.x;
      bj = ij.y;
    }
  }
  best_pair256(best, bi, bj, red, &key);
  if (threadIdx.x == 0) {
    d2[0] = best;
    pair[0] = bi;
    pair[1] = bj;
  }
}

static inline size_t diameter_partials(int n) {
  const int tiles = diameter_tiles(n), jc = diameter_jc(tiles);
  return (size_t)tiles * ((tiles + jc - 1) / jc);
}

extern "C" size_t pp_pts_diameter_workspace_bytes(int n) {
  if (n <= 0 || n > DIAMETER_MAX_PTS) return 0;
  return pp_align256(diameter_partials(n) * sizeof(double)) + diameter_partials(n) * sizeof(int2);
}

extern "C" int pp_pts_diameter_f64(pp_ctx* ctx, int n, const double* pts, void* workspace, size_t workspace_bytes, double* d2, int* pair) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n >= 1 && n <= DIAMETER_MAX_PTS, PP_ERR_SHAPE, "pp_pts_diameter_f64: need 1..%d points, got %d", DIAMETER_MAX_PTS, n);
  PP_CHECK_ARG(ctx, pts && workspace && d2 && pair, PP_ERR_ARG, "pp_pts_diameter_f64: null argument");
  PP_CHECK_ARG(ctx, workspace_bytes >= pp_pts_diameter_workspace_bytes(n), PP_ERR_ARG,
               "pp_pts_diameter_f64: workspace of %zu bytes, need %zu (pp_pts_diameter_workspace_bytes)", workspace_bytes,
               pp_pts_diameter_workspace_bytes(n));
  const int tiles = diameter_tiles(n), jc = diameter_jc(tiles), chunks = (tiles + jc - 1) / jc;
  const size_t n_part = diameter_partials(n);
  double* part_d2 = (double*)workspace;
  int2* part_ij = (int2*)((char*)workspace + pp_align256(n_part * sizeof(double)));
  hipLaunchKernelGGL(diameter_tile_kernel, dim3(tiles, chunks), dim3(POSE_TILE), 0, ctx->stream, n, tiles, jc, pts, part_d2, part_ij);
  hipLaunchKernelGGL(diameter_finish_kernel, dim3(1), dim3(POSE_TILE), 0, ctx->stream, (long long)n_part, (const double*)part_d2,
                     (const int2*)part_ij, d2, pair);
  PP_CHECK_LAUNCH(ctx, "pp_pts_diameter_f64");
  return PP_OK;
}

// ---- symmetry score: one-sided Hausdorff distance of a moved point set ------------------------------------------------------
// d2[k] = max_i min_j d2(S_k src_i, tgt_j).  Workgroup (tile, chunk) holds one source tile, one point per thread, moved once by
// each of the chunk's SYM_HD_CHUNK candidates (pose.hip's rigid() association) in registers, and sweeps ALL target tiles staged
// in LDS one at a time (broadcast reads: the three loads of a target point serve SYM_HD_CHUNK pairs).  The sweep keeps the
// running minimum only; partial[k][tile] = (the tile's largest minimum, the lowest i that has it).  Tail lanes (i >= n_src) hold
// no point: their minimum counts as -1, below every squared distance.  Tail entries of a target tile are never read.  A last
// chunk with fewer candidates repeats its last one in the spare slots and drops their results.
// The finish, one workgroup per candidate: the partials in a fixed order (lowest i on ties), then for that one source point the
// lowest j whose d2 EQUALS the minimum -- the same operations on the same operands give the same bits.

#define SYM_HD_CHUNK 4
#define SYM_HD_MAX_CAND 65535

__device__ __forceinline__ void rigid3(const double* __restrict__ R, const double* __restrict__ t, double x, double y, double z, double* ox,
                                       double* oy, double* oz) {  // pose.hip's rigid(): left to right
  *ox = R[0] * x + R[1] * y + R[2] * z + t[0];
  *oy = R[3] * x + R[4] * y + R[5] * z + t[1];
  *oz = R[6] * x + R[7] * y + R[8] * z + t[2];
}

__global__ void __launch_bounds__(POSE_TILE)
sym_hausdorff_tile_kernel(int n_src, int n_tgt, int n_cand, const double* __restrict__ src, const double* __restrict__ tgt,
                          const double* __restrict__ S_R, const double* __restrict__ S_t, double* __restrict__ part_d2,
                          int* __restrict__ part_i) {
  __shared__ double s[3 * POSE_TILE];
  __shared__ double red[SYM_HD_CHUNK * (POSE_TILE / 64)];
  __shared__ unsigned long long key[SYM_HD_CHUNK];
  const int tid = threadIdx.x, tile = blockIdx.x, k0 = blockIdx.y * SYM_HD_CHUNK;
  const int nk = min(SYM_HD_CHUNK, n_cand - k0);  // >= 1: the grid has ceil(n_cand / SYM_HD_CHUNK) chunks
  const int i = tile * POSE_TILE + tid;
  const bool mine = i < n_src;
  double mx[SYM_HD_CHUNK], my[SYM_HD_CHUNK], mz[SYM_HD_CHUNK], best[SYM_HD_CHUNK];
  {
    double x = 0.0, y = 0.0, z = 0.0;
    if (mine) {
      x = src[3 * (size_t)i];
      y = src[3 * (size_t)i + 1];
      z = src[3 * (size_t)i + 2];
    }
#pragma unroll
    for (int k = 0; k < SYM_HD_CHUNK; ++k) {
      const int kk = k0 + min(k, nk - 1);
      rigid3(S_R + 9 * (size_t)kk, S_t + 3 * (size_t)kk, x, y, z, &mx[k], &my[k], &mz[k]);
      best[k] = __builtin_inf();
    }
  }
  for (int j0 = 0; j0 < n_tgt; j0 += POSE_TILE) {
    const int lim = min(POSE_TILE, n_tgt - j0);
    __syncthreads();
    for (int e = tid; e < 3 * lim; e += POSE_TILE) s[e] = tgt[3 * (size_t)j0 + e];
    __syncthreads();
    if (mine) {
#pragma unroll 4
      for (int j = 0; j < lim; ++j) {
        const double qx = s[3 * j], qy = s[3 * j + 1], qz = s[3 * j + 2];
#pragma unroll
        for (int k = 0; k < SYM_HD_CHUNK; ++k) {
          const double q = dist2(mx[k], my[k], mz[k], qx, qy, qz);
          best[k] = q < best[k] ? q : best[k];
        }
      }
    }
  }
  double m[SYM_HD_CHUNK];
#pragma unroll
  for (int k = 0; k < SYM_HD_CHUNK; ++k) {
    best[k] = mine ? best[k] : -1.0;
    m[k] = best[k];
  }
  if (tid < SYM_HD_CHUNK) key[tid] = ~0ull;
  tile_max256(m, red);  // (its barriers order the reset of key before the minima below)
#pragma unroll
  for (int k = 0; k < SYM_HD_CHUNK; ++k)
    if (mine && best[k] == m[k]) atomicMin(&key[k], (unsigned long long)(unsigned)i);
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < SYM_HD_CHUNK; ++k)
      if (k < nk) {
        const size_t slot = (size_t)(k0 + k) * gridDim.x + tile;
        part_d2[slot] = m[k];
        part_i[slot] = (int)key[k];  // (every tile has a point: some lane set the key)
      }
  }
}

// grid (candidates): the candidate's partials, tile by tile -> d2, the lowest i that attains it, then the lowest j of that i
__global__ void __launch_bounds__(POSE_TILE)
sym_hausdorff_finish_kernel(int n_tgt, int tiles, const double* __restrict__ src, const double* __restrict__ tgt,
                            const double* __restrict__ S_R, const double* __restrict__ S_t, const double* __restrict__ part_d2,
                            const int* __restrict__ part_i, double* __restrict__ d2, int* __restrict__ arg) {
  __shared__ double red[POSE_TILE / 64];
  __shared__ unsigned long long key;
  const int tid = threadIdx.x, k = blockIdx.x;
  double best = -1.0;
  int bi = 0, none = 0;
  for (int t = tid; t < tiles; t += POSE_TILE) {  // rising tiles hold rising i: a strict comparison keeps the lowest
    const double q = part_d2[(size_t)k * tiles + t];
    if (q > best) {
      best = q;
      bi = part_i[(size_t)k * tiles + t];
    }
  }
  best_pair256(best, bi, none, red, &key);
  double x, y, z;
  rigid3(S_R + 9 * (size_t)k, S_t + 3 * (size_t)k, src[3 * (size_t)bi], src[3 * (size_t)bi + 1], src[3 * (size_t)bi + 2], &x, &y, &z);
  if (tid == 0) key = ~0ull;
  __syncthreads();
  for (int j = tid; j < n_tgt; j += POSE_TILE)
    if (dist2(x, y, z, tgt[3 * (size_t)j], tgt[3 * (size_t)j + 1], tgt[3 * (size_t)j + 2]) == best) {
      atomicMin(&key, (unsigned long long)(unsigned)j);
      break;  // this thread's further j are higher
    }
  __syncthreads();
  if (tid == 0) {
    d2[k] = best;
    arg[2 * k] = bi;
    arg[2 * k + 1] = key == ~0ull ? 0 : (int)key;  // (no j equals the minimum only when it is NaN)
  }
}

static inline size_t sym_hausdorff_partials(int n_src, int n_cand) { return (size_t)n_cand * diameter_tiles(n_src); }

extern "C" size_t pp_sym_hausdorff_workspace_bytes(int n_src, int n_cand) {
  if (n_src <= 0 || n_src > DIAMETER_MAX_PTS || n_cand <= 0 || n_cand > SYM_HD_MAX_CAND) return 0;
  return pp_align256(sym_hausdorff_partials(n_src, n_cand) * sizeof(double)) + sym_hausdorff_partials(n_src, n_cand) * sizeof(int);
}

extern "C" int pp_sym_hausdorff_f64(pp_ctx* ctx, int n_src, const double* src, int n_tgt, const double* tgt, int n_cand, const double* S_R,
                                    const double* S_t, void* workspace, size_t workspace_bytes, double* d2, int* arg) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n_src >= 1 && n_src <= DIAMETER_MAX_PTS && n_tgt >= 1 && n_tgt <= DIAMETER_MAX_PTS, PP_ERR_SHAPE,
               "pp_sym_hausdorff_f64: need 1..%d source and 1..%d target points, got %d and %d", DIAMETER_MAX_PTS, DIAMETER_MAX_PTS, n_src,
               n_tgt);
  PP_CHECK_ARG(ctx, n_cand >= 1 && n_cand <= SYM_HD_MAX_CAND, PP_ERR_SHAPE, "pp_sym_hausdorff_f64: need 1..%d candidates, got %d",
               SYM_HD_MAX_CAND, n_cand);
  PP_CHECK_ARG(ctx, src && tgt && S_R && S_t && workspace && d2 && arg, PP_ERR_ARG, "pp_sym_hausdorff_f64: null argument");
  PP_CHECK_ARG(ctx, workspace_bytes >= pp_sym_hausdorff_workspace_bytes(n_src, n_cand), PP_ERR_ARG,
               "pp_sym_hausdorff_f64: workspace of %zu bytes, need %zu (pp_sym_hausdorff_workspace_bytes)", workspace_bytes,
               pp_sym_hausdorff_workspace_bytes(n_src, n_cand));
  const int tiles = diameter_tiles(n_src), chunks = (n_cand + SYM_HD_CHUNK - 1) / SYM_HD_CHUNK;
  const size_t n_part = sym_hausdorff_partials(n_src, n_cand);
  double* part_d2 = (double*)workspace;
  int* part_i = (int*)((char*)workspace + pp_align256(n_part * sizeof(double)));
  hipLaunchKernelGGL(sym_hausdorff_tile_kernel, dim3(tiles, chunks), dim3(POSE_TILE), 0, ctx->stream, n_src, n_tgt, n_cand, src, tgt, S_R, S_t,
                     part_d2, part_i);
  hipLaunchKernelGGL(sym_hausdorff_finish_kernel, dim3(n_cand), dim3(POSE_TILE), 0, ctx->stream, n_tgt, tiles, src, tgt, S_R, S_t,
                     (const double*)part_d2, (const int*)part_i, d2, arg);
  PP_CHECK_LAUNCH(ctx, "pp_sym_hausdorff_f64");
  return PP_OK;
}

// ---- farthest points --------------------------------------------------------------------------------------------------
// One workgroup of FPS_THREADS per model, no grid-wide synchronisation: thread t owns the points t, t + FPS_THREADS, ... of
// its model.  The first of them and its running score stay in registers (a model of up to FPS_THREADS points never touches
// the workspace); the scores of the others live in score[] (workspace, one double per point of the launch).  Every pick:
// update each score against the point chosen last, then a workgroup argmax where the lowest index wins ties.
//   rule 0: score = min over the chosen of d2                                  (+inf before the first pick)
//   rule 1: score = sum over the chosen, in the order chosen, of sqrt(d2) to the chosen point ROUNDED TO FLOAT32; a point
//           that any chosen point is nearer to than min_dist is blocked for good: it is stored as -1 and scores 0.0

template <int RULE>
__device__ __forceinline__ double fps_update(double score, double x, double y, double z, double cx, double cy, double cz, double min_d) {
  const double q = dist2(x, y, z, cx, cy, cz);
  if (RULE == 0) return q < score ? q : score;
  const double d = __dsqrt_rn(q);
  return (score < 0.0 || d < min_d) ? -1.0 : score + d;
}

// the workgroup's largest v and the lowest index that holds it, returned to every thread (v >= 0 of a thread with points,
// -1 / INT_MAX of one without); red_v / red_i: FPS_THREADS / 64 entries each
__device__ __forceinline__ void fps_argmax(double& v, int& i, double* red_v, int* red_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
  if (lane == 0) {
    red_v[wave] = v;
    red_i[wave] = i;
  }
  __syncthreads();
  v = red_v[0];
  i = red_i[0];
  for (int w = 1; w < FPS_THREADS / 64; ++w) {
    const double ov = red_v[w];
    const int oi = red_i[w];
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
  __syncthreads();
}

template <int RULE>
__global__ void __launch_bounds__(FPS_THREADS)
farthest_points_kernel(int k, const double* __restrict__ pts_all, const int* __restrict__ offsets, const double* __restrict__ min_dist,
                       const int* __restrict__ start, double* __restrict__ score_all, int* __restrict__ index) {
  __shared__ double red_v[FPS_THREADS / 64];
  __shared__ int red_i[FPS_THREADS / 64];
  const int tid = threadIdx.x, m = blockIdx.x;
  const int off = offsets[m], n = offsets[m + 1] - off;  // n >= 1: checked on the host
  const double* pts = pts_all + 3 * (size_t)off;
  double* score = score_all + off;
  int* out = index + (size_t)m * k;
  const double min_d = RULE == 1 ? min_dist[m] : 0.0;
  const bool mine = tid < n;
  double x0 = 0.0, y0 = 0.0, z0 = 0.0;
  if (mine) {
    x0 = pts[3 * (size_t)tid];
    y0 = pts[3 * (size_t)tid + 1];
    z0 = pts[3 * (size_t)tid + 2];
  }
  int chosen;
  if (start) {
    chosen = min(max(start[m], 0), n - 1);
  } else {  // FPS.py:40-42: the first maximum of the norm, restated on its square
    double v = -1.0;
    chosen = 0x7fffffff;
    if (mine) {
      v = (x0 * x0 + y0 * y0) + z0 * z0;
      chosen = tid;
    }
    for (int i = tid + FPS_THREADS; i < n; i += FPS_THREADS) {
      const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
      const double q = (x * x + y * y) + z * z;
      if (q > v) {
        v = q;
        chosen = i;
      }
    }
    fps_argmax(v, chosen, red_v, red_i);
  }
  double s0 = RULE == 0 ? __builtin_inf() : 0.0;
  for (int i = tid + FPS_THREADS; i < n; i += FPS_THREADS) score[i] = s0;  // each thread reads back only what it wrote itself
  if (tid == 0) out[0] = chosen;
  for (int pick = 1; pick < k; ++pick) {
    double cx = pts[3 * (size_t)chosen], cy = pts[3 * (size_t)chosen + 1], cz = pts[3 * (size_t)chosen + 2];
    if (RULE == 1) {  // control_points is a float32 array (FPS.py:37, 83-84)
      cx = (double)(float)cx;
      cy = (double)(float)cy;
      cz = (double)(float)cz;
    }
    double v = -1.0;
    int best = 0x7fffffff;
    if (mine) {
      s0 = fps_update<RULE>(s0, x0, y0, z0, cx, cy, cz, min_d);
      v = s0 < 0.0 ? 0.0 : s0;
      best = tid;
    }
    for (int i = tid + FPS_THREADS; i < n; i += FPS_THREADS) {
      const double s = fps_update<RULE>(score[i], pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], cx, cy, cz, min_d);
      score[i] = s;
      const double u = s < 0.0 ? 0.0 : s;
      if (u > v) {
        v = u;
        best = i;
      }
    }
    fps_argmax(v, best, red_v, red_i);
    chosen = best;
    if (tid == 0) out[pick] = chosen;
  }
}

extern "C" size_t pp_farthest_points_workspace_bytes(int n_total) {
  if (n_total <= 0) return 0;
  return (size_t)n_total * sizeof(double);
}

extern "C" int pp_farthest_points_f64(pp_ctx* ctx, int n_model, int n_total, const double* pts, const int* offsets_host,
                                      const int* offsets_dev, int k, int rule, const double* min_dist, const int* start, void* workspace,
                                      size_t workspace_bytes, int* index) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n_model >= 1 && n_total >= 1 && k >= 1, PP_ERR_SHAPE,
               "pp_farthest_points_f64: need at least one model, one point and k >= 1, got %d models, %d points, k = %d", n_model, n_total, k);
  PP_CHECK_ARG(ctx, rule == 0 || rule == 1, PP_ERR_ARG, "pp_farthest_points_f64: rule must be 0 (min) or 1 (sum), got %d", rule);
  PP_CHECK_ARG(ctx, pts && offsets_host && offsets_dev && workspace && index && (min_dist || rule == 0), PP_ERR_ARG,
               "pp_farthest_points_f64: null argument");
  PP_CHECK_ARG(ctx, offsets_host[0] == 0 && offsets_host[n_model] == n_total, PP_ERR_ARG,
               "pp_farthest_points_f64: offsets must run from 0 to n_total = %d", n_total);
  for (int m = 0; m < n_model; ++m) {
    const long long n_m = (long long)offsets_host[m + 1] - offsets_host[m];
    PP_CHECK_ARG(ctx, n_m >= 0, PP_ERR_ARG, "pp_farthest_points_f64: offsets must not decrease (model %d)", m);
    PP_CHECK_ARG(ctx, n_m >= 1, PP_ERR_SHAPE, "pp_farthest_points_f64: model %d is empty", m);
    PP_CHECK_ARG(ctx, rule == 1 || k <= n_m, PP_ERR_SHAPE, "pp_farthest_points_f64: rule 0 picks k = %d distinct points, model %d has %lld", k,
                 m, n_m);
  }
  PP_CHECK_ARG(ctx, workspace_bytes >= pp_farthest_points_workspace_bytes(n_total), PP_ERR_ARG,
               "pp_farthest_points_f64: workspace of %zu bytes, need %zu (pp_farthest_points_workspace_bytes)", workspace_bytes,
               pp_farthest_points_workspace_bytes(n_total));
  if (rule == 0)
    hipLaunchKernelGGL(farthest_points_kernel<0>, dim3(n_model), dim3(FPS_THREADS), 0, ctx->stream, k, pts, offsets_dev, min_dist, start,
                       (double*)workspace, index);
  else
    hipLaunchKernelGGL(farthest_points_kernel<1>, dim3(n_model), dim3(FPS_THREADS), 0, ctx->stream, k, pts, offsets_dev, min_dist, start,
                       (double*)workspace, index);
  PP_CHECK_LAUNCH(ctx, "pp_farthest_points_f64");
  return PP_OK;
}
