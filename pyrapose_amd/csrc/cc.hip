// Connected components of byte planes: pp_cc_label (labels numbered as scipy.ndimage.label numbers them, per-component
// statistics) and pp_cc_select (label planes to instance masks).  The rule is written out in include/pyrapose_hip.h and restated
// in tests/cc_np.py.  What the reference's area clustering (encode_area, annotate_val_LineMOD.py:88-130) hands to a PCL binary.
// Integers only; every output is a pure function of the inputs.
//
//   tile     one workgroup per 32 x 32 tile and plane, 4 pixels per thread.  Labels in LDS start as the pixel's index in the tile
//            (lab[i] <= i, and lab[i] is always a pixel of i's component: both hold for ever).  A round lowers lab[i] to the
//            smallest label among i and its compatible neighbours, then jumps lab[i] <- lab[lab[i]] twice.  A round without
//            the jumps gives pixel i the minimum over its geodesic ball of radius `round`; the jumps only lower values further, and
//            a geodesic path inside a tile has fewer than CC_TILE_PX steps: a quiet round comes within CC_TILE_PX rounds.  At the
//            fixed point lab is constant on a component of the tile, <= its smallest index and a member: the smallest index.
//   seam     one thread per pixel beside a tile seam: union with the compatible neighbours across it (cc_union).
//   flatten  every foreground pixel replaces its label by its root.  A union attaches the larger root to the smaller, so the
//            root of a component is its smallest raster index: the pixel that fixes scipy's numbering.
//   number   one workgroup per plane walks it in chunks of CC_SCAN_CHUNK with a carry: an exclusive scan of the root flags.  A
//            root of rank k < M also starts its stats row (its own x and y: it is the first pixel, so y_min is final).
//   stats    one thread per pixel: labels = rank[root] + 1; the lanes of a wave that share a label fold their pixel into one
//            lane by butterflies, and that lane issues the integer atomics.
// No loop waits for another workgroup.  The three `while` loops (the chases of cc_find, the retry of cc_union) count their steps
// against H W -- each step strictly lowers a positive index -- and the tile rounds against CC_TILE_PX; a loop that reaches its
// bound stops and sets the error word, it never spins.  No kernel uses scratch (-Rpass-analysis=kernel-resource-usage).
#include "pose_common.h"

#define CC_TILE 32
#define CC_TILE_PX (CC_TILE * CC_TILE)
#define CC_THREADS 256
#define CC_PX (CC_TILE_PX / CC_THREADS)  // pixels per thread of the tile pass
#define CC_SCAN_THREADS 1024
#define CC_SCAN_PX 8                     // consecutive pixels per thread and chunk of the numbering scan
#define CC_SCAN_CHUNK (CC_SCAN_THREADS * CC_SCAN_PX)
#define CC_MAX_COMPONENTS 65535
#define CC_MAX_GRID 65535
#define CC_ERR_TILE 1   // bits of the error word: the tile pass, a chase, the retry loop of a union reached its bound
#define CC_ERR_CHASE 2
#define CC_ERR_UNION 4

// (relaxed device-scope accesses: a stale value is an older parent, still a smaller pixel of the same component)
__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x in plane L: at most `bound` = H W steps, each to a strictly smaller index
__device__ __forceinline__ int cc_find(const int* L, int x, int bound, int* err) {
  int steps = 0;
  int parent = cc_load(L + x);
  while (parent != x) {
    if (++steps > bound) {
      atomicOr(err, CC_ERR_CHASE);
      break;
    }
    x = parent;
    parent = cc_load(L + x);
  }
  return x;
}

// Join the trees of a and b: chase both roots, attach the larger to the smaller with atomicMin.  Where the larger root was
// attached elsewhere in the meantime the atomicMin still left it pointing at the smaller of the two targets; the other target
// and that smaller one are joined next.  max(a, b) falls strictly from retry to retry: at most `bound` = H W of them.
__device__ __forceinline__ void cc_union(int* L, int a, int b, int bound, int* err) {
  int tries = 0;
  while (true) {
    a = cc_find(L, a, bound, err);
    b = cc_find(L, b, bound, err);
    if (a == b) return;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicMin(L + hi, lo);
    if (old == hi) return;
    if (++tries > bound) {
      atomicOr(err, CC_ERR_UNION);
      return;
    }
    a = old;
    b = lo;
  }
}

// v: the byte that decides compatibility -- the plane's byte in value mode, 0 / 1 in binary mode
__device__ __forceinline__ unsigned char cc_byte(unsigned char v, int value_mode) { return value_mode ? v : (unsigned char)(v != 0); }

__global__ void __launch_bounds__(CC_THREADS)
cc_tile_kernel(int N, int H, int W, const unsigned char* __restrict__ planes, int conn8, int value_mode, int* __restrict__ L, int* err) {
  __shared__ int lab[CC_TILE_PX];
  __shared__ unsigned char val[CC_TILE_PX];
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * CC_TILE, ty0 = blockIdx.y * CC_TILE;
  for (int plane = blockIdx.z; plane < N; plane += gridDim.z) {
    const size_t base = (size_t)plane * H * W;
#pragma unroll
    for (int k = 0; k < CC_PX; ++k) {
      const int i = tid + k * CC_THREADS, x = tx0 + (i & (CC_TILE - 1)), y = ty0 + i / CC_TILE;
      const unsigned char v = (x < W && y < H) ? cc_byte(planes[base + (size_t)y * W + x], value_mode) : (unsigned char)0;
      val[i] = v;
      lab[i] = i;
    }
    __syncthreads();
    bool quiet = false;
    for (int round = 0; round < CC_TILE_PX; ++round) {
      int changed = 0;
#pragma unroll
      for (int k = 0; k < CC_PX; ++k) {
        const int i = tid + k * CC_THREADS, lx = i & (CC_TILE - 1), ly = i / CC_TILE;
        const unsigned char v = val[i];
        if (v == 0) continue;
        const int mine = lab[i];
        int m = mine;
        const bool l = lx > 0, r = lx < CC_TILE - 1, u = ly > 0, d = ly < CC_TILE - 1;
        if (l && val[i - 1] == v) m = min(m, lab[i - 1]);
        if (r && val[i + 1] == v) m = min(m, lab[i + 1]);
        if (u && val[i - CC_TILE] == v) m = min(m, lab[i - CC_TILE]);
        if (d && val[i + CC_TILE] == v) m = min(m, lab[i + CC_TILE]);
        if (conn8) {
          if (u && l && val[i - CC_TILE - 1] == v) m = min(m, lab[i - CC_TILE - 1]);
          if (u && r && val[i - CC_TILE + 1] == v) m = min(m, lab[i - CC_TILE + 1]);
          if (d && l && val[i + CC_TILE - 1] == v) m = min(m, lab[i + CC_TILE - 1]);
          if (d && r && val[i + CC_TILE + 1] == v) m = min(m, lab[i + CC_TILE + 1]);
        }
        if (m < mine) {
          lab[i] = m;  // (only the owner writes lab[i]; the neighbours' reads race with it, and either value is valid)
          changed = 1;
        }
      }
      if (__syncthreads_or(changed) == 0) {
        quiet = true;
        break;
      }
#pragma unroll
      for (int jump = 0; jump < 2; ++jump) {
#pragma unroll
        for (int k = 0; k < CC_PX; ++k) {
          const int i = tid + k * CC_THREADS;
          if (val[i]) lab[i] = lab[lab[i]];
        }
        __syncthreads();
      }
    }
    if (!quiet && tid == 0) atomicOr(err, CC_ERR_TILE);
#pragma unroll
    for (int k = 0; k < CC_PX; ++k) {
      const int i = tid + k * CC_THREADS, x = tx0 + (i & (CC_TILE - 1)), y = ty0 + i / CC_TILE;
      if (x < W && y < H) {
        const int root = lab[i];
        L[base + (size_t)y * W + x] = val[i] ? (ty0 + root / CC_TILE) * W + tx0 + (root & (CC_TILE - 1)) : -1;
      }
    }
    __syncthreads();  // the next plane's tile goes where this one's was read
  }
}

// Seam pixels of a plane, n_v = ((W - 1) / 32) H beside a vertical seam (x % 32 == 31, x + 1 < W) and then ((H - 1) / 32) W
// above a horizontal one.  The first kind joins (x + 1, y - 1 .. y + 1), the second (x - 1 .. x + 1, y + 1): every pair of
// adjacent pixels in different tiles is met from its left or its upper pixel, the diagonal pairs at a corner from both.
__global__ void __launch_bounds__(CC_THREADS)
cc_seam_kernel(int N, int H, int W, const unsigned char* __restrict__ planes, int conn8, int value_mode, int* L, int* err) {
  const long long n_v = (long long)((W - 1) / CC_TILE) * H, n_h = (long long)((H - 1) / CC_TILE) * W;
  const long long t = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (t >= n_v + n_h) return;
  int x, y, dx0, dx1, dy0, dy1;
  if (t < n_v) {
    x = (int)(t / H) * CC_TILE + CC_TILE - 1, y = (int)(t % H);
    dx0 = dx1 = 1, dy0 = conn8 ? -1 : 0, dy1 = conn8 ? 1 : 0;
  } else {
    const long long s = t - n_v;
    y = (int)(s / W) * CC_TILE + CC_TILE - 1, x = (int)(s % W);
    dy0 = dy1 = 1, dx0 = conn8 ? -1 : 0, dx1 = conn8 ? 1 : 0;
  }
  const int bound = H * W, p = y * W + x;
  for (int plane = blockIdx.y; plane < N; plane += gridDim.y) {
    const size_t base = (size_t)plane * H * W;
    const unsigned char v = cc_byte(planes[base + p], value_mode);
    if (v == 0) continue;
    for (int dy = dy0; dy <= dy1; ++dy)
      for (int dx = dx0; dx <= dx1; ++dx) {
        const int qx = x + dx, qy = y + dy;
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        const int q = qy * W + qx;
        if (cc_byte(planes[base + q], value_mode) == v) cc_union(L + base, p, q, bound, err);
      }
  }
}

__global__ void __launch_bounds__(CC_THREADS)
cc_flatten_kernel(int N, int H, int W, int* L, int* err) {
  const long long p = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  const int bound = H * W;
  if (p >= bound) return;
  for (int plane = blockIdx.y; plane < N; plane += gridDim.y) {
    int* Lp = L + (size_t)plane * H * W;
    if (cc_load(Lp + p) < 0) continue;
    // (other threads read Lp[p] on their own chases: the old parent and the root both lead to the root)
    __hip_atomic_store(Lp + p, cc_find(Lp, (int)p, bound, err), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// rank[p] = the number of roots before p, written at the roots only; counts[plane] = the number of roots
__global__ void __launch_bounds__(CC_SCAN_THREADS)
cc_number_kernel(int N, int H, int W, const unsigned char* __restrict__ planes, int value_mode, const int* __restrict__ L,
                 int* __restrict__ rank, int M, int* __restrict__ counts, int* __restrict__ stats) {
  __shared__ int s_wave[CC_SCAN_THREADS / 64];
  __shared__ int s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, HW = H * W;
  for (int plane = blockIdx.x; plane < N; plane += gridDim.x) {
    const size_t base = (size_t)plane * HW;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (long long chunk = 0; chunk < HW; chunk += CC_SCAN_CHUNK) {
      const long long p0 = chunk + (long long)tid * CC_SCAN_PX;
      unsigned int flags = 0;
#pragma unroll
      for (int k = 0; k < CC_SCAN_PX; ++k)
        if (p0 + k < HW && L[base + p0 + k] == (int)(p0 + k)) flags |= 1u << k;
      const int own = __popc(flags);
      int incl = own;  // inclusive scan over the wave
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      if (lane == 63) s_wave[wave] = incl;
      __syncthreads();
      int before = s_carry + incl - own, total = 0;
#pragma unroll
      for (int w = 0; w < CC_SCAN_THREADS / 64; ++w) {
        const int c = s_wave[w];
        before += w < wave ? c : 0;
        total += c;
      }
#pragma unroll
      for (int k = 0; k < CC_SCAN_PX; ++k) {
        if (!(flags >> k & 1u)) continue;
        const int p = (int)(p0 + k), r = before + __popc(flags & ((1u << k) - 1u));
        rank[base + p] = r;
        if (r < M) {
          int* row = stats + ((size_t)plane * M + r) * 6;
          const int x = p % W, y = p / W;
          row[1] = x, row[2] = y, row[3] = x, row[4] = y;  // (row[0], the area, stays 0 for the atomic adds)
          row[5] = value_mode ? (int)planes[base + p] : 1;
        }
      }
      __syncthreads();  // everyone has read s_carry and s_wave
      if (tid == 0) s_carry += total;
      __syncthreads();
    }
    if (tid == 0) counts[plane] = s_carry;
    __syncthreads();
  }
}

__device__ __forceinline__ long long cc_wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int cc_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int cc_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ void __launch_bounds__(CC_THREADS)
cc_stats_kernel(int N, int H, int W, const int* __restrict__ L, const int* __restrict__ rank, const int* __restrict__ weight, int M,
                int* __restrict__ labels, int* stats, long long* sums) {
  const long long p = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  const int HW = H * W, lane = threadIdx.x & 63;
  const bool inside = p < HW;
  const int x = inside ? (int)(p % W) : 0, y = inside ? (int)(p / W) : 0;
  for (int plane = blockIdx.y; plane < N; plane += gridDim.y) {
    const size_t base = (size_t)plane * HW;
    int label = 0;
    if (inside) {
      const int root = L[base + p];
      if (root >= 0) label = rank[base + root] + 1;
      labels[base + p] = label;
    }
    const int mine = label <= M ? label : 0;  // components beyond M are numbered, not measured
    const long long w = (mine && weight) ? (long long)weight[base + p] : 0;
    unsigned long long todo = __ballot(mine != 0);
    for (int it = 0; it < 64 && todo; ++it) {  // one turn per distinct label among the wave's 64 pixels
      const int leader = __ffsll((long long)todo) - 1;
      const int cur = __shfl(mine, leader, 64);
      const bool in = mine == cur;
      const unsigned long long members = __ballot(in);
      const long long sx = cc_wave_sum(in ? x : 0), sy = cc_wave_sum(in ? y : 0), sw = cc_wave_sum(in ? w : 0);
      const int x_lo = cc_wave_min(in ? x : 0x7fffffff), x_hi = cc_wave_max(in ? x : -1), y_hi = cc_wave_max(in ? y : -1);
      if (lane == leader) {
        int* row = stats + ((size_t)plane * M + (cur - 1)) * 6;
        unsigned long long* srow = (unsigned long long*)(sums + ((size_t)plane * M + (cur - 1)) * 3);
        atomicAdd(row + 0, __popcll(members));
        atomicMin(row + 1, x_lo);
        atomicMax(row + 3, x_hi);
        atomicMax(row + 4, y_hi);
        atomicAdd(srow + 0, (unsigned long long)sx);
        atomicAdd(srow + 1, (unsigned long long)sy);
        if (weight) atomicAdd(srow + 2, (unsigned long long)sw);
      }
      todo &= ~members;
    }
  }
}

static size_t cc_workspace_bytes(int N, int H, int W) { return pp_align256(4) + 2 * pp_align256((size_t)N * H * W * 4); }

extern "C" int pp_cc_label(pp_ctx* ctx, int N, int H, int W, const unsigned char* planes, int connectivity, int mode, const int* weight,
                           int max_components, void* workspace, size_t workspace_bytes, int* labels, int* counts, int* stats,
                           long long* sums) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, N >= 1 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), PP_ERR_SHAPE,
               "pp_cc_label: need N >= 1 planes of H, W >= 1 with H W < 2^31, got %d of %d x %d", N, H, W);
  PP_CHECK_ARG(ctx, connectivity == 4 || connectivity == 8, PP_ERR_ARG, "pp_cc_label: connectivity %d, need 4 or 8", connectivity);
  PP_CHECK_ARG(ctx, mode == PP_CC_BINARY || mode == PP_CC_VALUE, PP_ERR_ARG, "pp_cc_label: mode %d, need 0 (binary) or 1 (value)", mode);
  PP_CHECK_ARG(ctx, max_components >= 1 && max_components <= CC_MAX_COMPONENTS, PP_ERR_ARG, "pp_cc_label: max_components %d, need 1..%d",
               max_components, CC_MAX_COMPONENTS);
  PP_CHECK_ARG(ctx, planes && workspace && labels && counts && stats && sums, PP_ERR_ARG, "pp_cc_label: null argument");
  PP_CHECK_ARG(ctx, workspace_bytes >= cc_workspace_bytes(N, H, W) && ((uintptr_t)workspace & 255u) == 0, PP_ERR_ARG,
               "pp_cc_label: workspace of %zu bytes, need %zu, 256-byte aligned", workspace_bytes, cc_workspace_bytes(N, H, W));
  // (a plane of H W < 2^31 pixels has fewer than 2^21 tiles in all, but a column of them may pass the grid's y limit)
  PP_CHECK_ARG(ctx, (H + CC_TILE - 1) / CC_TILE <= CC_MAX_GRID, PP_ERR_SHAPE, "pp_cc_label: H = %d is more than %d tiles high", H, CC_MAX_GRID);
  const int HW = H * W, M = max_components, conn8 = connectivity == 8;
  const size_t P = (size_t)N * HW;
  int* err = (int*)workspace;
  int* L = (int*)((char*)workspace + pp_align256(4));
  int* rank = (int*)((char*)L + pp_align256(P * 4));
  PP_HIP(ctx, hipMemsetAsync(err, 0, 4, ctx->stream));
  PP_HIP(ctx, hipMemsetAsync(stats, 0, (size_t)N * M * 6 * sizeof(int), ctx->stream));
  PP_HIP(ctx, hipMemsetAsync(sums, 0, (size_t)N * M * 3 * sizeof(long long), ctx->stream));
  const int gz = N < CC_MAX_GRID ? N : CC_MAX_GRID;
  const dim3 tiles((W + CC_TILE - 1) / CC_TILE, (H + CC_TILE - 1) / CC_TILE, gz);
  hipLaunchKernelGGL(cc_tile_kernel, tiles, dim3(CC_THREADS), 0, ctx->stream, N, H, W, planes, conn8, mode, L, err);
  const long long n_seam = (long long)((W - 1) / CC_TILE) * H + (long long)((H - 1) / CC_TILE) * W;
  if (n_seam > 0) {
    hipLaunchKernelGGL(cc_seam_kernel, dim3((unsigned)((n_seam + CC_THREADS - 1) / CC_THREADS), gz), dim3(CC_THREADS), 0, ctx->stream, N, H,
                       W, planes, conn8, mode, L, err);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((HW + CC_THREADS - 1) / CC_THREADS, gz), dim3(CC_THREADS), 0, ctx->stream, N, H, W, L, err);
  }
  hipLaunchKernelGGL(cc_number_kernel, dim3(gz), dim3(CC_SCAN_THREADS), 0, ctx->stream, N, H, W, planes, mode, (const int*)L, rank, M, counts,
                     stats);
  hipLaunchKernelGGL(cc_stats_kernel, dim3((HW + CC_THREADS - 1) / CC_THREADS, gz), dim3(CC_THREADS), 0, ctx->stream, N, H, W, (const int*)L,
                     (const int*)rank, weight, M, labels, stats, sums);
  PP_CHECK_LAUNCH(ctx, "pp_cc_label");
  return PP_OK;
}

// 4 pixels per thread where H W is a multiple of 4 and the pointers allow it (VEC), else one
template <bool VEC>
__global__ void __launch_bounds__(CC_THREADS)
cc_select_kernel(int N, int HW, int S, const int* __restrict__ labels, const int* __restrict__ slot_plane, const int* __restrict__ slot_label,
                 unsigned char* __restrict__ masks) {
  const long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  const int n = VEC ? HW / 4 : HW;
  if (i >= n) return;
  for (int s = blockIdx.y; s < S; s += gridDim.y) {
    const int plane = slot_plane[s], want = slot_label[s];
    const bool live = plane >= 0 && plane < N && want > 0;
    if (VEC) {
      unsigned int m = 0;
      if (live) {
        const int4 v = ((const int4*)(labels + (size_t)plane * HW))[i];
        m = (unsigned)(v.x == want) | (unsigned)(v.y == want) << 8 | (unsigned)(v.z == want) << 16 | (unsigned)(v.w == want) << 24;
      }
      ((unsigned int*)(masks + (size_t)s * HW))[i] = m;
    } else {
      masks[(size_t)s * HW + i] = live ? (unsigned char)(labels[(size_t)plane * HW + i] == want) : (unsigned char)0;
    }
  }
}

extern "C" int pp_cc_select(pp_ctx* ctx, int N, int H, int W, const int* labels, int S, const int* slot_plane, const int* slot_label,
                            unsigned char* masks) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, N >= 1 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), PP_ERR_SHAPE,
               "pp_cc_select: need N >= 1 planes of H, W >= 1 with H W < 2^31, got %d of %d x %d", N, H, W);
  PP_CHECK_ARG(ctx, S >= 0, PP_ERR_SHAPE, "pp_cc_select: %d slots", S);
  if (S == 0) return PP_OK;
  PP_CHECK_ARG(ctx, labels && slot_plane && slot_label && masks, PP_ERR_ARG, "pp_cc_select: null argument");
  const int HW = H * W, gy = S < CC_MAX_GRID ? S : CC_MAX_GRID;
  const bool vec = HW % 4 == 0 && pp_is_aligned16(labels) && ((uintptr_t)masks & 3u) == 0;
  const int n = vec ? HW / 4 : HW;
  const dim3 grid((n + CC_THREADS - 1) / CC_THREADS, gy);
  if (vec)
    hipLaunchKernelGGL(cc_select_kernel<true>, grid, dim3(CC_THREADS), 0, ctx->stream, N, HW, S, labels, slot_plane, slot_label, masks);
  else
    hipLaunchKernelGGL(cc_select_kernel<false>, grid, dim3(CC_THREADS), 0, ctx->stream, N, HW, S, labels, slot_plane, slot_label, masks);
  PP_CHECK_LAUNCH(ctx, "pp_cc_select");
  return PP_OK;
}
