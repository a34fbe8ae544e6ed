// Depth-hole filling: layered inpainting, the step the reference takes with cv2.inpaint(depth, depth == 0, 5, INPAINT_NS) before
// get_normal (annotate_val_LineMOD.py:206-221 and six more of its annotation scripts).  The project's own method (the rule is
// written out in include/pyrapose_hip.h and restated in tests/depth_inpaint_np.py): holes are filled layer by layer, a layer being
// the pixels at one chessboard distance L from the nearest known pixel; a pixel of layer k is the weighted mean of the pixels of
// layers < k in its (2 radius + 1)^2 window, taken in row-major order, w = 1 / ((dx^2 + dy^2)(1 + L(q))), all float64, every
// product, sum and quotient rounded on its own (-ffp-contract=off).  A layer reads only lower layers (a Jacobi step per layer), so
// the result does not depend on how pixels are spread over lanes, workgroups or launches: the outputs are the restatement's bits.
//
//   rows      half a wave (DI_TILE = 32 lanes) per image row, DI_ROWS rows per workgroup: g = the distance along the row to its
//             nearest known pixel (DI_FAR: the row has none).  A row is taken in segments of 32 pixels, a lane per pixel: the
//             nearest known pixel on the left is a running maximum across the lanes (shuffles of width 32) carried from segment to
//             segment, then the same from the right.  Also v = hole ? 0 : depth as float64 and the image's counts of holes and of
//             known pixels (folded across the 32 lanes first, one integer atomic per row and counter).
//   columns   a lane per pixel, 32 x 8 pixels per workgroup: L(x, y) = min over y' of max(|y - y'|, g(x, y')), scanning outwards
//             from y and stopping once |dy| reaches the best value so far.  An image without a known pixel gets DI_FAR everywhere.
//             Counts the pixels to fill (1 <= L <= limit) per layer: the first DI_HBINS layers in an LDS histogram that is flushed
//             with one atomic per used bin, the others straight into global memory; the image's pixels to fill and largest L
//             are folded over each wave (ballot, butterfly), then over the waves: one atomic per workgroup.
//   scan      exclusive_scan_kernel of pose_common.h over the layers' counts; its offsets are read back once (the only host
//             synchronisation): they give the number of fill launches and each one's size.
//   scatter   counting sort of the pixels to fill by layer: a workgroup reserves its range of every low layer with one atomic,
//             its lanes take their places inside through LDS atomics.  The order inside a layer is left to the atomics: it has no
//             part in the result.
//   fill      one launch per layer k over that layer's pixels of all images, a lane per pixel.  Ordering between layers is
//             launch order on the stream and nothing else.
//   minmax    rescale only: per image the smallest and largest filled value and the largest input depth, as integer atomics on
//             the bits of non-negative doubles (the minimum as the maximum of the complemented bits, so that zero is the neutral
//             element of all three): exact and order-free.  Folded over each wave by a butterfly, then over the waves: one atomic per workgroup.
//   finish    rescale, the rounding to float32, and the counts.
// No floating-point atomics, no waiting of one workgroup on another.
#include "pose_common.h"

#define DI_TILE 32          // lanes per row in `rows`, pixels per row of a workgroup in `columns`
#define DI_ROWS 8           // rows per workgroup in both
#define DI_THREADS 256
#define DI_MAX_SIDE 4096
#define DI_MAX_IMG 65535
#define DI_MIN_SIDE 3
#define DI_MAX_RADIUS 8
#define DI_MAX_DIST 65535
#define DI_FAR 65535        // g of a row, L of an image, without a known pixel
#define DI_BINS DI_MAX_SIDE // layers 0..4095: L <= max(H, W) - 1
#define DI_HBINS 64         // layers counted in LDS
#define DI_CNT 4            // ints per image in the workspace: holes, pixels to fill, largest layer, known pixels

__device__ __forceinline__ bool di_is_hole(const float* __restrict__ depth, const unsigned char* __restrict__ hole_mask, size_t px) {
  return hole_mask ? hole_mask[px] != 0 : depth[px] == 0.0f;
}

__global__ void __launch_bounds__(DI_THREADS)
di_rows_kernel(int n_rows, int H, int W, const float* __restrict__ depth, const unsigned char* __restrict__ hole_mask,
               unsigned short* __restrict__ g, double* __restrict__ v, int* __restrict__ cnt) {
  const int lane = threadIdx.x % DI_TILE;
  const long long r = (long long)blockIdx.x * DI_ROWS + threadIdx.x / DI_TILE;
  const bool live = r < n_rows;  // (a dead half-wave runs along with its shuffles and stores nothing)
  const size_t base = (size_t)(live ? r : 0) * W;
  const int n_seg = (W + DI_TILE - 1) / DI_TILE;
  const int NEG = -(1 << 20), POS = 1 << 20;
  int carry = NEG, holes = 0, known = 0;
  for (int s = 0; s < n_seg; ++s) {
    const int x = s * DI_TILE + lane;
    const bool in = live && x < W;
    const bool hole = in && di_is_hole(depth, hole_mask, base + x);
    int last = (in && !hole) ? x : NEG;
    for (int d = 1; d < DI_TILE; d <<= 1) {
      const int t = __shfl_up(last, d, DI_TILE);
      if (lane >= d) last = max(last, t);
    }
    last = max(last, carry);
    carry = __shfl(last, DI_TILE - 1, DI_TILE);
    if (in) {
      g[base + x] = (unsigned short)min(x - last, DI_FAR);
      v[base + x] = hole ? 0.0 : (double)depth[base + x];
      holes += hole ? 1 : 0;
      known += hole ? 0 : 1;
    }
  }
  carry = POS;
  for (int s = n_seg - 1; s >= 0; --s) {
    const int x = s * DI_TILE + lane;
    const bool in = live && x < W;
    const int left = in ? (int)g[base + x] : DI_FAR;  // (this lane's own store)
    int next = (in && left == 0) ? x : POS;
    for (int d = 1; d < DI_TILE; d <<= 1) {
      const int t = __shfl_down(next, d, DI_TILE);
      if (lane + d < DI_TILE) next = min(next, t);
    }
    next = min(next, carry);
    carry = __shfl(next, 0, DI_TILE);
    if (in) g[base + x] = (unsigned short)min(left, min(next - x, DI_FAR));
  }
  for (int o = DI_TILE / 2; o > 0; o >>= 1) {
    holes += __shfl_xor(holes, o, DI_TILE);
    known += __shfl_xor(known, o, DI_TILE);
  }
  if (live && lane == 0) {
    int* c = cnt + (size_t)(r / H) * DI_CNT;
    if (holes) atomicAdd(c + 0, holes);
    if (known) atomicAdd(c + 3, known);
  }
}

__global__ void __launch_bounds__(DI_THREADS)
di_columns_kernel(int H, int W, int limit, const unsigned short* __restrict__ g, unsigned short* __restrict__ L, int* __restrict__ cnt,
                  int* __restrict__ hist) {
  __shared__ int bins[DI_HBINS];
  __shared__ int wave_fill[DI_THREADS / 64], wave_top[DI_THREADS / 64];
  const int img = blockIdx.z, tid = threadIdx.x;
  const int x = blockIdx.x * DI_TILE + tid % DI_TILE, y = blockIdx.y * DI_ROWS + tid / DI_TILE;
  if (tid < DI_HBINS) bins[tid] = 0;
  __syncthreads();
  int* c = cnt + (size_t)img * DI_CNT;
  int top = 0;
  bool mine = false;
  if (x < W && y < H) {
    const unsigned short* gi = g + (size_t)img * H * W;
    int best = DI_FAR;
    if (c[3] != 0) {  // (written by the launch before this one)
      best = gi[(size_t)y * W + x];
      for (int dy = 1; dy < best; ++dy) {
        const bool up = y - dy >= 0, down = y + dy < H;
        if (!up && !down) break;
        if (up) best = min(best, max(dy, (int)gi[(size_t)(y - dy) * W + x]));
        if (down) best = min(best, max(dy, (int)gi[(size_t)(y + dy) * W + x]));
      }
    }
    L[((size_t)img * H + y) * W + x] = (unsigned short)best;
    if (best != DI_FAR && best > 0) {
      top = best;
      mine = best <= limit;
      if (mine) {
        if (best < DI_HBINS) atomicAdd(&bins[best], 1);
        else atomicAdd(hist + best, 1);
      }
    }
  }
  // the image's counters: folded over each wave's 64 lanes (ballot, butterfly), then over the waves through LDS by plain stores:
  // one global atomic per workgroup and counter
  const int to_fill = __popcll(__ballot(mine));
  for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
  if ((tid & 63) == 0) {
    wave_fill[tid >> 6] = to_fill;
    wave_top[tid >> 6] = top;
  }
  __syncthreads();
  if (tid == 0) {
    int f = 0, t = 0;
    for (int w = 0; w < DI_THREADS / 64; ++w) {
      f += wave_fill[w];
      t = max(t, wave_top[w]);
    }
    if (f) atomicAdd(c + 1, f);
    if (t) atomicMax(c + 2, t);
  }
  if (tid < DI_HBINS && bins[tid]) atomicAdd(hist + tid, bins[tid]);
}

__global__ void __launch_bounds__(DI_THREADS)
di_scatter_kernel(unsigned int n_px, int limit, const unsigned short* __restrict__ L, int* __restrict__ cursor, unsigned int* __restrict__ list) {
  __shared__ int bins[DI_HBINS];
  __shared__ int first[DI_HBINS];
  const int tid = threadIdx.x;
  const unsigned int i = blockIdx.x * DI_THREADS + tid;
  if (tid < DI_HBINS) bins[tid] = 0;
  __syncthreads();
  const int l = i < n_px ? (int)L[i] : 0;
  const bool mine = l >= 1 && l <= limit;
  int place = 0;
  if (mine && l < DI_HBINS) place = atomicAdd(&bins[l], 1);
  __syncthreads();
  if (tid < DI_HBINS && bins[tid]) first[tid] = atomicAdd(cursor + tid, bins[tid]);
  __syncthreads();
  if (mine) list[l < DI_HBINS ? first[l] + place : atomicAdd(cursor + l, 1)] = i;
}

__global__ void __launch_bounds__(DI_THREADS)
di_fill_kernel(int k, int begin, int count, int H, int W, int radius, const unsigned int* __restrict__ list,
               const unsigned short* __restrict__ L, double* __restrict__ v) {
  const int i = blockIdx.x * DI_THREADS + threadIdx.x;
  if (i >= count) return;
  const unsigned int p = list[begin + i];
  const unsigned int hw = (unsigned int)(H * W);
  const unsigned int img = p / hw, rem = p - img * hw;
  const int y = (int)(rem / (unsigned int)W), x = (int)(rem - (unsigned int)y * W);
  const size_t base = (size_t)img * hw;
  double num = 0.0, den = 0.0;
  const int y0 = max(y - radius, 0), y1 = min(y + radius, H - 1), x0 = max(x - radius, 0), x1 = min(x + radius, W - 1);
  for (int qy = y0; qy <= y1; ++qy) {
    const int dy = qy - y;
    for (int qx = x0; qx <= x1; ++qx) {
      const size_t q = base + (size_t)qy * W + qx;
      const int lq = L[q];
      if (lq >= k) continue;
      const int dx = qx - x;
      const double w = 1.0 / (double)((dx * dx + dy * dy) * (1 + lq));
      num = num + w * v[q];
      den = den + w;
    }
  }
  v[base + rem] = num / den;
}

// the workgroup's largest a, b, c (unsigned 64-bit patterns) into dst[0..3): a butterfly over each wave's 64 lanes, the waves'
// values through LDS by plain stores, one global atomic per workgroup and value (skipped for 0, the neutral element)
__device__ __forceinline__ void di_group_max3(unsigned long long a, unsigned long long b, unsigned long long c,
                                              unsigned long long (*slot)[DI_THREADS / 64], unsigned long long* dst) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long ua = __shfl_xor(a, o, 64), ub = __shfl_xor(b, o, 64), uc = __shfl_xor(c, o, 64);
    a = ua > a ? ua : a;
    b = ub > b ? ub : b;
    c = uc > c ? uc : c;
  }
  if ((threadIdx.x & 63) == 0) {
    slot[0][threadIdx.x >> 6] = a;
    slot[1][threadIdx.x >> 6] = b;
    slot[2][threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long m = 0ull;
    for (int w = 0; w < DI_THREADS / 64; ++w) m = slot[threadIdx.x][w] > m ? slot[threadIdx.x][w] : m;
    if (m) atomicMax(dst + threadIdx.x, m);
  }
}

// mm[img] = (~bits of the smallest v, bits of the largest v, bits of the largest depth); v and depth are >= 0 and not NaN
__global__ void __launch_bounds__(DI_THREADS)
di_minmax_kernel(int HW, const float* __restrict__ depth, const double* __restrict__ v, unsigned long long* __restrict__ mm) {
  __shared__ unsigned long long slot[3][DI_THREADS / 64];
  const int img = blockIdx.y, i = blockIdx.x * DI_THREADS + threadIdx.x;
  unsigned long long a = 0ull, b = 0ull, c = 0ull;
  if (i < HW) {
    const double val = v[(size_t)img * HW + i], d = (double)depth[(size_t)img * HW + i];
    const unsigned long long vb = val > 0.0 ? (unsigned long long)__double_as_longlong(val) : 0ull;  // (-0.0 counts as 0.0)
    a = ~vb;
    b = vb;
    c = d > 0.0 ? (unsigned long long)__double_as_longlong(d) : 0ull;
  }
  di_group_max3(a, b, c, slot, mm + 3 * (size_t)img);
}

__global__ void __launch_bounds__(DI_THREADS)
di_finish_kernel(int HW, int rescale, const float* __restrict__ depth, const double* __restrict__ v, const int* __restrict__ cnt,
                 const unsigned long long* __restrict__ mm, float* __restrict__ filled_f32, double* __restrict__ filled_f64,
                 int* __restrict__ counts) {
  const int img = blockIdx.y, i = blockIdx.x * DI_THREADS + threadIdx.x;
  const int* c = cnt + (size_t)img * DI_CNT;
  if (counts && i < 3) counts[3 * img + i] = c[i];
  if (i >= HW || (!filled_f32 && !filled_f64)) return;
  const size_t px = (size_t)img * HW + i;
  double val;
  if (c[3] == 0) {
    val = (double)depth[px];  // no known pixel: the image as it came
  } else {
    val = v[px];
    if (rescale) {
      const double lo = __longlong_as_double((long long)~mm[3 * img]), hi = __longlong_as_double((long long)mm[3 * img + 1]);
      const double top = __longlong_as_double((long long)mm[3 * img + 2]);
      if (hi > lo) val = ((val - lo) / (hi - lo)) * top;
    }
  }
  if (filled_f64) filled_f64[px] = val;
  if (filled_f32) filled_f32[px] = (float)val;
}

static inline bool di_shape_ok(int n_img, int H, int W) {
  return n_img >= 1 && n_img <= DI_MAX_IMG && H >= DI_MIN_SIDE && W >= DI_MIN_SIDE && H <= DI_MAX_SIDE && W <= DI_MAX_SIDE && (long long)n_img * H * W < (1ll << 31);
}

// ints: cnt [n,4], the layers' counts [DI_BINS], their offsets [DI_BINS + 1] and cursors [DI_BINS]; mm [n,3] 64-bit; then per pixel
// g and L uint16, the sorted list uint32, v float64
static inline size_t di_head_bytes(int n_img) { return pp_align256(sizeof(int) * ((size_t)DI_CNT * n_img + 3 * DI_BINS + 1)); }
extern "C" size_t pp_depth_inpaint_workspace_bytes(int n_img, int H, int W) {
  if (!di_shape_ok(n_img, H, W)) return 0;
  const size_t px = (size_t)n_img * H * W;
  return di_head_bytes(n_img) + pp_align256(24 * (size_t)n_img) + 2 * pp_align256(2 * px) + pp_align256(4 * px) + pp_align256(8 * px);
}

extern "C" int pp_depth_inpaint(pp_ctx* ctx, int n_img, int H, int W, const float* depth, const unsigned char* hole_mask, int radius,
                                int max_dist, int rescale, void* workspace, size_t workspace_bytes, float* filled_f32, double* filled_f64,
                                unsigned short* layer_u16, int* counts) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, di_shape_ok(n_img, H, W), PP_ERR_SHAPE,
               "pp_depth_inpaint: need 1..%d images of %d..%d x %d..%d pixels, fewer than 2^31 in all, got %d of %d x %d", DI_MAX_IMG,
               DI_MIN_SIDE, DI_MAX_SIDE, DI_MIN_SIDE, DI_MAX_SIDE, n_img, H, W);
  PP_CHECK_ARG(ctx, depth && workspace, PP_ERR_ARG, "pp_depth_inpaint: null argument");
  PP_CHECK_ARG(ctx, radius >= 1 && radius <= DI_MAX_RADIUS, PP_ERR_ARG, "pp_depth_inpaint: radius %d, need 1..%d", radius, DI_MAX_RADIUS);
  PP_CHECK_ARG(ctx, max_dist >= 0 && max_dist <= DI_MAX_DIST, PP_ERR_ARG, "pp_depth_inpaint: max_dist %d, need 0 (no limit) .. %d", max_dist,
               DI_MAX_DIST);
  PP_CHECK_ARG(ctx, rescale == 0 || rescale == 1, PP_ERR_ARG, "pp_depth_inpaint: rescale must be 0 or 1, got %d", rescale);
  PP_CHECK_ARG(ctx, filled_f32 || filled_f64 || layer_u16 || counts, PP_ERR_ARG, "pp_depth_inpaint: no output asked for");
  PP_CHECK_ARG(ctx, workspace_bytes >= pp_depth_inpaint_workspace_bytes(n_img, H, W), PP_ERR_ARG,
               "pp_depth_inpaint: workspace of %zu bytes, need %zu (pp_depth_inpaint_workspace_bytes)", workspace_bytes,
               pp_depth_inpaint_workspace_bytes(n_img, H, W));
  const size_t px = (size_t)n_img * H * W, head = di_head_bytes(n_img), mm_bytes = pp_align256(24 * (size_t)n_img);
  char* at = (char*)workspace;
  int* cnt = (int*)at;
  int* hist = cnt + (size_t)DI_CNT * n_img;
  int* offsets = hist + DI_BINS;
  int* cursor = offsets + DI_BINS + 1;
  unsigned long long* mm = (unsigned long long*)(at + head);
  at += head + mm_bytes;
  unsigned short* g = (unsigned short*)at;
  at += pp_align256(2 * px);
  unsigned short* L = layer_u16 ? layer_u16 : (unsigned short*)at;
  at += pp_align256(2 * px);
  unsigned int* list = (unsigned int*)at;
  at += pp_align256(4 * px);
  double* v = (double*)at;
  // the deepest layer an image of this size can have, cut at max_dist: the layers that are filled, and the bins that are scanned
  const int deepest = (H > W ? H : W) - 1, limit = (max_dist == 0 || max_dist > deepest) ? deepest : max_dist;
  const bool fill = filled_f32 || filled_f64;
  const dim3 block(DI_THREADS);
  PP_HIP(ctx, hipMemsetAsync(workspace, 0, head + mm_bytes, ctx->stream));
  const int n_rows = n_img * H;
  hipLaunchKernelGGL(di_rows_kernel, dim3((n_rows + DI_ROWS - 1) / DI_ROWS), block, 0, ctx->stream, n_rows, H, W, depth, hole_mask, g, v, cnt);
  hipLaunchKernelGGL(di_columns_kernel, dim3((W + DI_TILE - 1) / DI_TILE, (H + DI_ROWS - 1) / DI_ROWS, n_img), block, 0, ctx->stream, H, W,
                     limit, (const unsigned short*)g, L, cnt, hist);
  const dim3 grid_img((H * W + DI_THREADS - 1) / DI_THREADS, n_img);
  if (fill) {
    hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, limit + 1, (const int*)hist, offsets, cursor);
    hipLaunchKernelGGL(di_scatter_kernel, dim3((unsigned int)((px + DI_THREADS - 1) / DI_THREADS)), block, 0, ctx->stream, (unsigned int)px,
                       limit, (const unsigned short*)L, cursor, list);
    PP_CHECK_LAUNCH(ctx, "pp_depth_inpaint");
    int offsets_host[DI_BINS + 1];
    PP_HIP(ctx, hipMemcpyAsync(offsets_host, offsets, (size_t)(limit + 2) * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 1; k <= limit; ++k) {
      const int begin = offsets_host[k], count = offsets_host[k + 1] - begin;
      if (begin == offsets_host[limit + 1]) break;  // nothing from here on
      if (count > 0)
        hipLaunchKernelGGL(di_fill_kernel, dim3((count + DI_THREADS - 1) / DI_THREADS), block, 0, ctx->stream, k, begin, count, H, W, radius,
                           (const unsigned int*)list, (const unsigned short*)L, v);
    }
    if (rescale) hipLaunchKernelGGL(di_minmax_kernel, grid_img, block, 0, ctx->stream, H * W, depth, (const double*)v, mm);
  }
  if (fill || counts)
    hipLaunchKernelGGL(di_finish_kernel, grid_img, block, 0, ctx->stream, H * W, rescale, depth, (const double*)v, (const int*)cnt,
                       (const unsigned long long*)mm, filled_f32, filled_f64, counts);
  PP_CHECK_LAUNCH(ctx, "pp_depth_inpaint");
  return PP_OK;
}
