// The small kernels around the plane-format convolutions, with their entry points: the split of activations, gradients and weights
// into (hi, lo) planes, the power-of-two scale of the gradient chain, and the 32-row block flags / lists of the sparse passes.
// Exports the capture pass and the list compaction to the other conv3 units (conv3.h).
#include "conv3_unit.h"
#include "conv3.h"

namespace {

// ---- activation / gradient split: f32 [rows][ld] -> bf16 hi/lo planes with the same geometry ----
__global__ void split_planes_kernel(size_t n8, const float4* __restrict__ src, uint4* __restrict__ hi, uint4* __restrict__ lo,
                                    const float* __restrict__ scale) {
  const float sc = scale ? *scale : 1.f;  // (a power of two: exact)
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    uint4 h, l;
    float4 a = src[2 * i], b = src[2 * i + 1];
    a.x *= sc; a.y *= sc; a.z *= sc; a.w *= sc;
    b.x *= sc; b.y *= sc; b.z *= sc; b.w *= sc;
    split8(a, b, &h, &l);
    hi[2 * i] = h;  // packed planes: group i = 32 bytes, hi then lo (lo = hi + 16 bytes)
    lo[2 * i] = l;
  }
}

// The power of two the gradient chain travels multiplied by (halves stop at 6e-8, loss gradients are ~1e-7): every loss
// gradient is bounded by ~1 / max(1, positives of its head) (focal: |dL/dlogit| <= 1 / n, orthogonal_l1: <= 0.125 / n), so
// 2^G = 2^8 * 2^floor(log2(max(1, min positives))) keeps the largest element near 2^8 and leaves 2^8 of headroom for the
// growth through the backward chain; scale2 = {2^G, 2^-G}.
__global__ void grad_scale_kernel(const int* __restrict__ counts, int n_counts, float* __restrict__ scale2, int base_log2) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int n = 0x7fffffff;
    for (int i = 0; i < n_counts; ++i) n = counts[i] < n ? counts[i] : n;
    n = n < 1 ? 1 : n;
    int e = 0;
    while ((n >> (e + 1)) != 0) ++e;
    const float s = __uint_as_float((unsigned)(127 + base_log2 + e) << 23);
    scale2[0] = s;
    scale2[1] = 1.f / s;
  }
}

// ---- which 32-row blocks of a gradient tensor hold a non-zero? (input of the row-block skip of bwd-weight / bwd-data) ----
__global__ void row_block_flags_kernel(const float* __restrict__ x, int rows, int ld, int cols4, unsigned char* __restrict__ flags) {
  const int blk = blockIdx.x, r0 = blk * 32;
  const int nr = rows - r0 < 32 ? rows - r0 : 32;
  int any = 0;
  for (int i = threadIdx.x; i < nr * cols4; i += blockDim.x) {
    const int r = i / cols4, c = i - r * cols4;
    const float4 v = *reinterpret_cast<const float4*>(x + (long long)(r0 + r) * ld + 4 * c);
    any |= (v.x != 0.f) | (v.y != 0.f) | (v.z != 0.f) | (v.w != 0.f);  // NaN != 0: a block with a NaN is kept
  }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) flags[blk] = any ? 1 : 0;
}

// the same scan of a tensor stored as bf16 (hi, lo) planes: value != 0 <=> a magnitude bit is set in hi or lo
// within (may be NULL): only the blocks flagged there can hold a non-zero (the caller knows the others are zero): they are not read
__global__ void row_block_flags_planes_kernel(const uint2* __restrict__ hi, const uint2* __restrict__ lo, int rows, int ld4, int cols4,
                                              unsigned char* __restrict__ flags, const unsigned char* __restrict__ within) {
  const int blk = blockIdx.x, r0 = blk * 32;
  if (within && !within[blk]) {  // (uniform)
    if (threadIdx.x == 0) flags[blk] = 0;
    return;
  }
  const int nr = rows - r0 < 32 ? rows - r0 : 32;
  int any = 0;
  for (int i = threadIdx.x; i < nr * cols4; i += blockDim.x) {
    const int r = i / cols4, c = i - r * cols4;
    const long long o = pk4((long long)(r0 + r) * ld4 + c);
    const uint2 h = hi[o], l = lo[o];
    any |= fmt_any_nonzero(h.x | h.y, l.x | l.y) ? 1 : 0;
  }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) flags[blk] = any ? 1 : 0;
}

// ordered compaction by ONE workgroup: list[0] = count, list[1 ..] = the flagged block indices, ascending
__global__ void row_block_compact_kernel(const unsigned char* __restrict__ flags, int n_blocks, int* __restrict__ list) {
  __shared__ int wave_cnt[4];
  __shared__ int base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n_blocks; i0 += 256) {
    const int i = i0 + tid;
    const bool f = i < n_blocks && flags[i] != 0;
    const unsigned long long m = __ballot(f);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wave_cnt[w];
    if (f) list[1 + off + before] = i;
    __syncthreads();
    if (tid == 0) base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    __syncthreads();
  }
  if (tid == 0) list[0] = base;
}

// ---- weight split: f32 HWIO [tap*cin + ci][ld_w] -> bf16 hi/lo planes in both k-contiguous layouts ----
__device__ __forceinline__ void split_weights_tile(int tap, int ci0, int co0, int cin, int cout, int ld_w, const float* __restrict__ w,
                                                   unsigned short* __restrict__ fwd_hi, unsigned short* __restrict__ fwd_lo, int cout_rows,
                                                   unsigned short* __restrict__ dg_hi, unsigned short* __restrict__ dg_lo, int dg_ld) {
  // 32x32 (ci x co) tiles through LDS so that both layouts are written with contiguous rows
  __shared__ unsigned short t_hi[32][33], t_lo[32][33];
  const int tx = threadIdx.x, ty = threadIdx.y;  // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int ci = ci0 + j, co = co0 + tx;
    float v = 0.f;
    if (ci < cin && co < cout) v = w[((long long)tap * cin + ci) * ld_w + co];
    unsigned short uh, ul;
    fmt_encode_weight(v, &uh, &ul);
    t_hi[j][tx] = uh;
    t_lo[j][tx] = ul;
    if (dg_hi && ci < cin && co < dg_ld) {  // bwd-data layout: [tap][ci][co], co contiguous
      const long long o = ((long long)tap * cin + ci) * dg_ld + co;
      dg_hi[o] = uh;
      dg_lo[o] = ul;
    }
  }
  __syncthreads();
  if (fwd_hi) {
    for (int j = ty; j < 32; j += 8) {  // forward layout: [tap][co][ci], ci contiguous
      const int co = co0 + j, ci = ci0 + tx;
      if (co < cout_rows && ci < cin) {
        const long long o = ((long long)tap * cout_rows + co) * cin + ci;
        fwd_hi[o] = t_hi[tx][j];
        fwd_lo[o] = t_lo[tx][j];
      }
    }
  }
}

__global__ void split_weights_kernel(int taps, int cin, int cout, int ld_w, const float* __restrict__ w,
                                     unsigned short* __restrict__ fwd_hi, unsigned short* __restrict__ fwd_lo, int cout_rows,
                                     unsigned short* __restrict__ dg_hi, unsigned short* __restrict__ dg_lo, int dg_ld) {
  split_weights_tile(blockIdx.z, blockIdx.y * 32, blockIdx.x * 32, cin, cout, ld_w, w, fwd_hi, fwd_lo, cout_rows, dg_hi, dg_lo, dg_ld);
}

// every tensor of a model in ONE launch (the optimizer step re-splits ~80 tensors; 80 launches of ~5 us were 2 % of a step)
__global__ void split_weights_batch_kernel(int n_jobs, const pp_split_job* __restrict__ jobs) {
  int lo = 0, hi = n_jobs - 1;  // last job with tile_begin <= blockIdx.x (uniform)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].tile_begin <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const pp_split_job j = jobs[lo];
  const int dg_ld = (j.cout + 31) / 32 * 32;
  const int tiles_co = dg_ld / 32, tiles_ci = j.cin / 32;
  int t = (int)blockIdx.x - j.tile_begin;
  const int co_t = t % tiles_co;
  t /= tiles_co;
  const int ci_t = t % tiles_ci, tap = t / tiles_ci;
  split_weights_tile(tap, ci_t * 32, co_t * 32, j.cin, j.cout, j.ld_w, j.w, (unsigned short*)j.fwd_hi, (unsigned short*)j.fwd_lo, j.cout,
                     (unsigned short*)j.dg_hi, (unsigned short*)j.dg_lo, dg_ld);
}

// both pp_split_planes entry points (scale: NULL, or a power of two on the device)
static int split_planes_impl(pp_ctx* ctx, size_t n, const float* src, void* hi, void* lo, const float* scale) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, src && hi && lo && n % 8 == 0, PP_ERR_ARG, "pp_split_planes_bf16x3: n must be a multiple of 8");
  PP_CHECK_ARG(ctx, pp_is_aligned16(src) && pp_is_packed(hi, lo), PP_ERR_ALIGN, "pp_split_planes_bf16x3: alignment / packed planes (lo = hi + 16 bytes)");
  if (n == 0) return PP_OK;
  size_t blocks = (n / 8 + 255) / 256;
  const size_t cap = (size_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 8;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, n / 8, (const float4*)src, (uint4*)hi, (uint4*)lo, scale);
  PP_CHECK_LAUNCH(ctx, "pp_split_planes_bf16x3");
  return PP_OK;
}

}  // namespace

void PP_API(pp3_split_capture_pass)(hipStream_t st, const IgemmParams& p, void* chi, void* clo) {
  const size_t n8 = (size_t)(p.src_rows * (long long)p.ld_src / 8);
  size_t blocks = (n8 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n8, (const float4*)p.src, (uint4*)chi, (uint4*)clo, (const float*)nullptr);
}

void PP_API(pp3_launch_row_block_compact)(hipStream_t st, const unsigned char* flags, int n_blocks, int* list) {
  hipLaunchKernelGGL(row_block_compact_kernel, dim3(1), dim3(256), 0, st, flags, n_blocks, list);
}

extern "C" {

int PP_API(pp_row_block_list)(pp_ctx* ctx, const float* x, int rows, int ld, int cols, unsigned char* flags, int* list) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, x && flags && list && rows > 0 && cols > 0 && cols <= ld && ld % 4 == 0 && pp_is_aligned16(x), PP_ERR_ARG,
               "pp_row_block_list: bad tensor (ld %% 4 == 0, 16-byte aligned)");
  const int nb = (rows + 31) / 32, cols4 = (cols + 3) / 4;
  PP_CHECK_ARG(ctx, 4 * cols4 <= ld, PP_ERR_SHAPE, "pp_row_block_list: cols rounded up to 4 exceed ld");
  hipLaunchKernelGGL(row_block_flags_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, x, rows, ld, cols4, flags);
  PP_API(pp3_launch_row_block_compact)(ctx->stream, flags, nb, list);
  PP_CHECK_LAUNCH(ctx, "pp_row_block_list");
  return PP_OK;
}

int PP_API(pp_row_block_list_planes_within)(pp_ctx* ctx, const void* x_hi, const void* x_lo, int rows, int ld, int cols,
                                               const unsigned char* within, unsigned char* flags, int* list) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, x_hi && x_lo && flags && list && rows > 0 && cols > 0 && cols <= ld && ld % 8 == 0 && pp_is_packed(x_hi, x_lo), PP_ERR_ARG,
               "pp_row_block_list_planes: bad tensor (ld %% 8 == 0, packed planes)");
  const int nb = (rows + 31) / 32, cols4 = (cols + 3) / 4;
  PP_CHECK_ARG(ctx, 4 * cols4 <= ld, PP_ERR_SHAPE, "pp_row_block_list_planes: cols rounded up to 4 exceed ld");
  hipLaunchKernelGGL(row_block_flags_planes_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, (const uint2*)x_hi, (const uint2*)x_lo, rows,
                     ld / 4, cols4, flags, within);
  PP_API(pp3_launch_row_block_compact)(ctx->stream, flags, nb, list);
  PP_CHECK_LAUNCH(ctx, "pp_row_block_list_planes");
  return PP_OK;
}

int PP_API(pp_row_block_list_planes)(pp_ctx* ctx, const void* x_hi, const void* x_lo, int rows, int ld, int cols, unsigned char* flags,
                                        int* list) {
  return PP_API(pp_row_block_list_planes_within)(ctx, x_hi, x_lo, rows, ld, cols, nullptr, flags, list);
}

int PP_API(pp_split_planes_bf16x3)(pp_ctx* ctx, size_t n, const float* src, void* hi, void* lo) {
  return split_planes_impl(ctx, n, src, hi, lo, nullptr);
}

int PP_API(pp_split_planes_scaled_bf16x3)(pp_ctx* ctx, size_t n, const float* src, void* hi, void* lo, const float* scale_dev) {
  return split_planes_impl(ctx, n, src, hi, lo, scale_dev);
}

int PP_API(pp_grad_scale_from_counts_adj)(pp_ctx* ctx, const int* counts_dev, int n_counts, float* scale2_dev, int log2_adjust) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, counts_dev && scale2_dev && n_counts >= 1 && n_counts <= 16 && log2_adjust >= -16 && log2_adjust <= 16, PP_ERR_ARG,
               "pp_grad_scale_from_counts: bad arguments");
  hipLaunchKernelGGL(grad_scale_kernel, dim3(1), dim3(64), 0, ctx->stream, counts_dev, n_counts, scale2_dev,
                     pp_conv_switches().gscale_log2 + log2_adjust);
  PP_CHECK_LAUNCH(ctx, "pp_grad_scale_from_counts");
  return PP_OK;
}
int PP_API(pp_grad_scale_from_counts)(pp_ctx* ctx, const int* counts_dev, int n_counts, float* scale2_dev) {
  return PP_API(pp_grad_scale_from_counts_adj)(ctx, counts_dev, n_counts, scale2_dev, 0);
}

int PP_API(pp_conv_split_weights_bf16x3_batch)(pp_ctx* ctx, int n_jobs, const pp_split_job* jobs_dev, int total_tiles) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n_jobs >= 0 && total_tiles >= 0 && (n_jobs == 0 || jobs_dev), PP_ERR_ARG, "pp_conv_split_weights_bf16x3_batch: bad arguments");
  if (n_jobs == 0 || total_tiles == 0) return PP_OK;
  hipLaunchKernelGGL(split_weights_batch_kernel, dim3((unsigned)total_tiles), dim3(32, 8), 0, ctx->stream, n_jobs, jobs_dev);
  PP_CHECK_LAUNCH(ctx, "pp_conv_split_weights_bf16x3_batch");
  return PP_OK;
}

int PP_API(pp_conv_split_weights_bf16x3)(pp_ctx* ctx, const pp_conv_desc* d, const float* w, void* fwd_hi, void* fwd_lo,
                                            void* dg_hi, void* dg_lo) {
  PP_REQUIRE_CTX(ctx);
  int rc = check_desc(ctx, d, "pp_conv_split_weights_bf16x3");
  if (rc) return rc;
  PP_CHECK_ARG(ctx, w && ((fwd_hi && fwd_lo) || (dg_hi && dg_lo)), PP_ERR_ARG, "pp_conv_split_weights_bf16x3: null tensor");
  PP_CHECK_ARG(ctx, d->cin % 32 == 0, PP_ERR_SHAPE, "pp_conv_split_weights_bf16x3: cin %d must be a multiple of 32", d->cin);
  const int taps = d->kh * d->kw;
  const int dg_ld = (d->cout + 31) / 32 * 32;
  dim3 grid((unsigned)((dg_ld + 31) / 32), (unsigned)((d->cin + 31) / 32), (unsigned)taps);
  hipLaunchKernelGGL(split_weights_kernel, grid, dim3(32, 8), 0, ctx->stream, taps, d->cin, d->cout, d->ld_w, w,
                     (unsigned short*)fwd_hi, (unsigned short*)fwd_lo, d->cout, (unsigned short*)dg_hi, (unsigned short*)dg_lo, dg_ld);
  PP_CHECK_LAUNCH(ctx, "pp_conv_split_weights_bf16x3");
  return PP_OK;
}

}  // extern "C"
