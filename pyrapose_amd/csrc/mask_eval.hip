// Segmentation metrics on the device (include/pyrapose_hip.h states every rule; DESIGN.md 7b the layout):
//   pp_mask_confusion     (tp, fp, fn) of the mask head's output against its training target, per threshold and class
//   pp_mask_pack          byte masks -> 64 pixels per word (one wave ballot per word), area and non-empty word range per mask
//   pp_mask_iou_pairs     IoU of every (detection slot, ground truth) pair of an image from the packed words
//   pp_mask_rle           run lengths (COCO's uncompressed counts) in row- or column-major order; pp_mask_from_rle back
// pp_det_match_iou, the matching on that IoU, is det_match_kernel's second IoU source in det_eval.hip.
// Integer arithmetic throughout (integer atomics only: exact in any order), one float64 division per IoU.  Restated in
// tests/mask_eval_np.py; every output is byte-identical to it and from run to run.  Compiled with -ffp-contract=off.
#include "pose_common.h"

#define MASK_TILE 256                   // threads of every workgroup here: 4 waves
#define MASK_WAVES (MASK_TILE / 64)
#define MASK_TD PP_MASK_IOU_TILE_DET    // detections of a pp_mask_iou_pairs tile: one per wave
#define MASK_TG PP_MASK_IOU_TILE_GT     // ground truths of a tile: each wave's accumulators
#define MASK_CONF_CHUNK 16384           // elements of pred a workgroup of mask_confusion_kernel takes per step
#define MASK_CONF_MAX_BLOCKS 2048

static_assert(MASK_TD == MASK_WAVES, "one wave per detection of a tile");

struct mask_thresholds {
  double v[PP_DET_MAX_THR];
};

// ---- pp_mask_confusion ----------------------------------------------------------------------------------------------------
// A workgroup walks chunks of MASK_CONF_CHUNK consecutive elements of pred (coalesced), its partial counts [T][C][3] as ints in
// LDS; a lane adds only where a count is not zero (background pixels, the bulk, add nothing).  At the end every non-zero
// partial is folded into counts with one 64-bit integer atomic.
static __global__ __launch_bounds__(MASK_TILE) void mask_confusion_kernel(long long n_elem, int C, int T, const float* __restrict__ pred,
                                                                         const float* __restrict__ target, mask_thresholds thr,
                                                                         unsigned long long* __restrict__ counts) {
  extern __shared__ int s_cnt[];  // [T][C][3]
  const int tid = threadIdx.x, n_cell = T * C * 3;
  for (int i = tid; i < n_cell; i += MASK_TILE) s_cnt[i] = 0;
  __syncthreads();
  const long long n_chunk = (n_elem + MASK_CONF_CHUNK - 1) / MASK_CONF_CHUNK;
  for (long long chunk = blockIdx.x; chunk < n_chunk; chunk += gridDim.x) {
    const long long e0 = chunk * MASK_CONF_CHUNK;
    const long long row0 = e0 / C;
    const int c0 = (int)(e0 - row0 * C);
    const int n = (int)(n_elem - e0 < MASK_CONF_CHUNK ? n_elem - e0 : MASK_CONF_CHUNK);
    for (int i = tid; i < n; i += MASK_TILE) {
      const int q = c0 + i;  // < C + MASK_CONF_CHUNK
      const int dr = q / C, c = q - dr * C;
      const double p = (double)pred[e0 + i];
      const bool set = target[(row0 + dr) * (C + 1) + c] != 0.0f;
      for (int t = 0; t < T; ++t) {
        const bool on = p > thr.v[t];  // NaN: not predicted
        if (on || set) atomicAdd(&s_cnt[(t * C + c) * 3 + (on ? (set ? 0 : 1) : 2)], 1);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < n_cell; i += MASK_TILE) {
    const int v = s_cnt[i];
    if (v) atomicAdd(&counts[i], (unsigned long long)v);
  }
}

extern "C" int pp_mask_confusion(pp_ctx* ctx, int batch, int n_pix, int n_class, const float* pred, const float* target, int n_thr,
                                 const double* thresholds, long long* counts) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n_thr >= 1 && n_thr <= PP_DET_MAX_THR, PP_ERR_ARG, "pp_mask_confusion: need 1..%d thresholds, got %d", PP_DET_MAX_THR, n_thr);
  PP_CHECK_ARG(ctx, batch >= 1 && n_pix >= 1 && n_class >= 1 && n_class <= PP_MASK_MAX_CLASS, PP_ERR_SHAPE,
               "pp_mask_confusion: need batch, n_pix >= 1 and 1 <= n_class <= %d", PP_MASK_MAX_CLASS);
  PP_CHECK_ARG(ctx, (long long)batch * n_pix * (n_class + 1) < (1ll << 31), PP_ERR_SHAPE,
               "pp_mask_confusion: batch * n_pix * (n_class + 1) must stay below 2^31");
  PP_CHECK_ARG(ctx, pred && target && thresholds && counts, PP_ERR_ARG, "pp_mask_confusion: null argument");
  mask_thresholds thr = {};
  for (int t = 0; t < n_thr; ++t) {
    PP_CHECK_ARG(ctx, thresholds[t] == thresholds[t], PP_ERR_ARG, "pp_mask_confusion: threshold %d is NaN", t);
    thr.v[t] = thresholds[t];
  }
  const long long n_elem = (long long)batch * n_pix * n_class;
  const long long n_chunk = (n_elem + MASK_CONF_CHUNK - 1) / MASK_CONF_CHUNK;
  const int blocks = (int)(n_chunk < MASK_CONF_MAX_BLOCKS ? n_chunk : MASK_CONF_MAX_BLOCKS);
  const size_t cells = (size_t)n_thr * n_class * 3;
  PP_HIP(ctx, hipMemsetAsync(counts, 0, cells * sizeof(long long), ctx->stream));
  hipLaunchKernelGGL(mask_confusion_kernel, dim3(blocks), dim3(MASK_TILE), cells * sizeof(int), ctx->stream, n_elem, n_class, n_thr, pred,
                     target, thr, (unsigned long long*)counts);
  PP_CHECK_LAUNCH(ctx, "pp_mask_confusion");
  return PP_OK;
}

// ---- pp_mask_pack ---------------------------------------------------------------------------------------------------------
// One workgroup per mask; wave w takes the words w, w + 4, ...: lane l reads pixel 64 k + l, the ballot is the word (a pixel at
// or past H W reads as 0, so the tail bits are zero).  Area and the first / last non-empty word per wave, then through LDS.
static __global__ __launch_bounds__(MASK_TILE) void mask_pack_kernel(int HW, int n_word, const unsigned char* __restrict__ masks,
                                                                    unsigned long long* __restrict__ words, long long* __restrict__ area,
                                                                    int* __restrict__ word_range) {
  __shared__ long long s_area[MASK_WAVES];
  __shared__ int s_first[MASK_WAVES], s_last[MASK_WAVES];
  const size_t n = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned char* m = masks + n * (size_t)HW;
  unsigned long long* w = words + n * (size_t)n_word;
  long long a = 0;
  int first = n_word, last = -1;
  for (int k = wave; k < n_word; k += MASK_WAVES) {
    const long long p = (long long)k * 64 + lane;
    const bool on = p < HW && m[p] != 0;
    const unsigned long long word = __ballot(on);
    if (lane == 0) w[k] = word;
    if (word) {
      a += __popcll(word);
      first = first < k ? first : k;
      last = k;
    }
  }
  if (lane == 0) {
    s_area[wave] = a;
    s_first[wave] = first;
    s_last[wave] = last;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < MASK_WAVES; ++i) {
      a += s_area[i];
      first = first < s_first[i] ? first : s_first[i];
      last = last > s_last[i] ? last : s_last[i];
    }
    area[n] = a;
    word_range[2 * n] = last < 0 ? 0 : first;
    word_range[2 * n + 1] = last + 1;  // an empty mask: [0, 0)
  }
}

static int mask_shape_ok(pp_ctx* ctx, const char* who, int n_mask, int H, int W) {
  PP_CHECK_ARG(ctx, n_mask >= 0 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31), PP_ERR_SHAPE,
               "%s: need n_mask >= 0, H, W >= 1 and H * W < 2^31", who);
  return PP_OK;
}

extern "C" int pp_mask_pack(pp_ctx* ctx, int n_mask, int H, int W, const unsigned char* masks, unsigned long long* words, long long* area,
                            int* word_range) {
  PP_REQUIRE_CTX(ctx);
  const int rc = mask_shape_ok(ctx, "pp_mask_pack", n_mask, H, W);
  if (rc != PP_OK) return rc;
  if (n_mask == 0) return PP_OK;
  PP_CHECK_ARG(ctx, masks && words && area && word_range, PP_ERR_ARG, "pp_mask_pack: null argument");
  const int HW = H * W, n_word = (int)(((long long)HW + 63) / 64);
  hipLaunchKernelGGL(mask_pack_kernel, dim3(n_mask), dim3(MASK_TILE), 0, ctx->stream, HW, n_word, masks, words, area, word_range);
  PP_CHECK_LAUNCH(ctx, "pp_mask_pack");
  return PP_OK;
}

// ---- pp_mask_iou_pairs ----------------------------------------------------------------------------------------------------
// A workgroup takes a tile of MASK_TD detection slots x MASK_TG ground truths of one image.  Wave w owns slot d0 + w: its lanes
// stride over the slot's non-empty word range, each word read once and ANDed with the same word of the tile's MASK_TG ground
// truths (where that word lies in their range), so a detection's words leave memory once per MASK_TG pairs and the MASK_TG
// ground-truth rows are shared by the tile's waves through the CU's cache.  Integer sums, a butterfly, one division.
static __global__ __launch_bounds__(MASK_TILE) void mask_iou_kernel(
    int D, int n_word, int tiles_d, int tiles_g, const unsigned long long* __restrict__ det_words, const long long* __restrict__ det_area,
    const int* __restrict__ det_range, const int* __restrict__ det_labels, const unsigned long long* __restrict__ gt_words,
    const long long* __restrict__ gt_area, const int* __restrict__ gt_range, const int* __restrict__ gt_offsets, double* __restrict__ iou,
    long long* __restrict__ inter_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per_image = tiles_d * tiles_g;
  const int b = blockIdx.x / per_image, rest = blockIdx.x - b * per_image;
  const int td = rest / tiles_g, tg = rest - td * tiles_g;
  const int g0 = gt_offsets[b];
  const int ng = gt_offsets[b + 1] - g0;
  const int gb = tg * MASK_TG, d = td * MASK_TD + wave;
  if (gb >= ng || d >= D) return;  // (wave-uniform)
  const size_t slot = (size_t)b * D + d;
  const bool padding = det_labels != nullptr && det_labels[slot] < 0;
  int lo = det_range[2 * slot], hi = det_range[2 * slot + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > n_word ? n_word : hi;
  if (padding) hi = lo;
  int glo[MASK_TG], ghi[MASK_TG], acc[MASK_TG];
#pragma unroll
  for (int j = 0; j < MASK_TG; ++j) {
    const bool have = gb + j < ng;
    glo[j] = have ? gt_range[2 * (size_t)(g0 + gb + j)] : 0;
    ghi[j] = have ? gt_range[2 * (size_t)(g0 + gb + j) + 1] : 0;
    ghi[j] = ghi[j] > n_word ? n_word : ghi[j];
    acc[j] = 0;
  }
  const unsigned long long* dw = det_words + slot * (size_t)n_word;
  for (int k = lo + lane; k < hi; k += 64) {
    const unsigned long long a = dw[k];
#pragma unroll
    for (int j = 0; j < MASK_TG; ++j)
      if (k >= glo[j] && k < ghi[j]) acc[j] += __popcll(a & gt_words[(size_t)(g0 + gb + j) * n_word + k]);
  }
#pragma unroll
  for (int j = 0; j < MASK_TG; ++j)
    for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
  if (lane == 0) {
    const long long ad = padding ? 0 : det_area[slot];
    double* out = iou + (size_t)D * (size_t)g0 + (size_t)d * ng;
    long long* out_i = inter_out ? inter_out + (size_t)D * (size_t)g0 + (size_t)d * ng : nullptr;
#pragma unroll
    for (int j = 0; j < MASK_TG; ++j) {
      if (gb + j >= ng) break;
      const long long uni = ad + (padding ? 0 : gt_area[g0 + gb + j]) - acc[j];
      out[gb + j] = uni > 0 ? (double)acc[j] / (double)uni : 0.0;
      if (out_i) out_i[gb + j] = acc[j];
    }
  }
}

extern "C" int pp_mask_iou_pairs(pp_ctx* ctx, int batch, int n_det, int n_gt, int H, int W, const unsigned long long* det_words,
                                 const long long* det_area, const int* det_range, const int* det_labels,
                                 const unsigned long long* gt_words, const long long* gt_area, const int* gt_range,
                                 const int* gt_offsets_host, const int* gt_offsets_dev, double* iou, long long* inter) {
  PP_REQUIRE_CTX(ctx);
  const int rc = mask_shape_ok(ctx, "pp_mask_iou_pairs", 0, H, W);
  if (rc != PP_OK) return rc;
  PP_CHECK_ARG(ctx, batch >= 1 && n_gt >= 0, PP_ERR_ARG, "pp_mask_iou_pairs: batch must be >= 1, n_gt >= 0");
  PP_CHECK_ARG(ctx, n_det >= 0 && n_det <= PP_DET_MAX_DET, PP_ERR_ARG, "pp_mask_iou_pairs: %d detection slots per image, the limit is %d",
               n_det, PP_DET_MAX_DET);
  PP_CHECK_ARG(ctx, (long long)n_det * n_gt < (1ll << 31), PP_ERR_ARG, "pp_mask_iou_pairs: n_det * n_gt pairs must stay below 2^31");
  PP_CHECK_ARG(ctx, gt_offsets_host && gt_offsets_dev, PP_ERR_ARG, "pp_mask_iou_pairs: null argument");
  PP_CHECK_ARG(ctx, gt_offsets_host[0] == 0 && gt_offsets_host[batch] == n_gt, PP_ERR_ARG, "pp_mask_iou_pairs: gt_offsets must run from 0 to n_gt");
  int max_ng = 0;
  for (int b = 0; b < batch; ++b) {
    const int n = gt_offsets_host[b + 1] - gt_offsets_host[b];
    PP_CHECK_ARG(ctx, n >= 0, PP_ERR_ARG, "pp_mask_iou_pairs: gt_offsets decrease at image %d", b);
    PP_CHECK_ARG(ctx, n <= PP_DET_MAX_GT, PP_ERR_ARG, "pp_mask_iou_pairs: image %d has %d ground truths, the limit is %d", b, n, PP_DET_MAX_GT);
    max_ng = n > max_ng ? n : max_ng;
  }
  if (n_det == 0 || n_gt == 0) return PP_OK;  // no pairs
  PP_CHECK_ARG(ctx, det_words && det_area && det_range && gt_words && gt_area && gt_range && iou, PP_ERR_ARG, "pp_mask_iou_pairs: null argument");
  const int tiles_d = (n_det + MASK_TD - 1) / MASK_TD, tiles_g = (max_ng + MASK_TG - 1) / MASK_TG;
  const long long blocks = (long long)batch * tiles_d * tiles_g;
  PP_CHECK_ARG(ctx, blocks < (1ll << 31), PP_ERR_SHAPE, "pp_mask_iou_pairs: batch * tiles must stay below 2^31");
  const int n_word = (int)(((long long)H * W + 63) / 64);
  hipLaunchKernelGGL(mask_iou_kernel, dim3((unsigned)blocks), dim3(MASK_TILE), 0, ctx->stream, n_det, n_word, tiles_d, tiles_g, det_words,
                     det_area, det_range, det_labels, gt_words, gt_area, gt_range, gt_offsets_dev, iou, inter);
  PP_CHECK_LAUNCH(ctx, "pp_mask_iou_pairs");
  return PP_OK;
}

// ---- pp_mask_rle / pp_mask_from_rle ---------------------------------------------------------------------------------------
// Position p of the run order: pixel p (row-major) or pixel (p % H) W + p / H (column-major).  A boundary sits at p >= 1 where
// the pixel differs from the one before, and at p = 0 where the first pixel is set (the leading zero run then has length 0).
__device__ __forceinline__ bool rle_pixel(const unsigned char* m, int p, int H, int W, int order) {
  return m[order == PP_MASK_ORDER_ROW ? (size_t)p : (size_t)(p % H) * W + p / H] != 0;
}
__device__ __forceinline__ bool rle_boundary(const unsigned char* m, int p, int H, int W, int order) {
  const bool v = rle_pixel(m, p, H, W, order);
  return p == 0 ? v : v != rle_pixel(m, p - 1, H, W, order);
}

// One workgroup per mask, a wave per 64 positions, the flags as a ballot.  WRITE = false: n_run[mask] = boundaries + 1.
// WRITE = true: boundary number r (counted by popcounts: the lanes below, the waves below, the steps before) at position p writes
// counts[run_offsets[mask] + r] = p - (the boundary before it, or 0); the last run ends at H W.
template <bool WRITE>
static __global__ __launch_bounds__(MASK_TILE) void mask_rle_kernel(int H, int W, int order, const unsigned char* __restrict__ masks,
                                                                   int* __restrict__ n_run, const int* __restrict__ run_offsets,
                                                                   int* __restrict__ counts) {
  __shared__ int s_n[MASK_WAVES], s_last[MASK_WAVES];
  const int HW = H * W;
  const size_t n = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned char* m = masks + n * (size_t)HW;
  int* out = WRITE ? counts + run_offsets[n] : nullptr;
  int carry_n = 0, carry_last = 0;  // boundaries before this step, and the position of the last one (0: none)
  for (int base = 0; base < HW; base += MASK_TILE) {  // (HW < 2^31 - MASK_TILE is checked on the host)
    const int p = base + threadIdx.x;
    const bool f = p < HW && rle_boundary(m, p, H, W, order);
    const unsigned long long flags = __ballot(f);
    const unsigned long long below = flags & ((1ull << lane) - 1ull);
    if (lane == 0) {
      s_n[wave] = __popcll(flags);
      s_last[wave] = flags ? base + wave * 64 + 63 - __clzll((long long)flags) : -1;
    }
    __syncthreads();
    int rank = carry_n, prev = carry_last, total = carry_n, last = carry_last;
    for (int i = 0; i < MASK_WAVES; ++i) {
      if (i < wave) {
        rank += s_n[i];
        prev = s_last[i] >= 0 ? s_last[i] : prev;
      }
      total += s_n[i];
      last = s_last[i] >= 0 ? s_last[i] : last;
    }
    if (WRITE && f) {
      if (below) prev = base + wave * 64 + 63 - __clzll((long long)below);
      out[rank + __popcll(below)] = p - prev;
    }
    carry_n = total;
    carry_last = last;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (WRITE) out[carry_n] = HW - carry_last;
    else n_run[n] = carry_n + 1;
  }
}

extern "C" size_t pp_mask_rle_workspace_bytes(int n_mask) { return n_mask < 0 ? 0 : pp_align256((size_t)(n_mask > 0 ? n_mask : 1) * sizeof(int)); }

extern "C" int pp_mask_rle(pp_ctx* ctx, int n_mask, int H, int W, int order, const unsigned char* masks, void* workspace,
                           size_t workspace_bytes, long long capacity, int* run_offsets, int* run_offsets_host, int* counts) {
  PP_REQUIRE_CTX(ctx);
  const int rc = mask_shape_ok(ctx, "pp_mask_rle", n_mask, H, W);
  if (rc != PP_OK) return rc;
  PP_CHECK_ARG(ctx, n_mask >= 1 && (long long)n_mask * ((long long)H * W + 1) < (1ll << 31) && (long long)H * W < (1ll << 31) - MASK_TILE,
               PP_ERR_SHAPE, "pp_mask_rle: need n_mask >= 1 and n_mask * (H * W + 1) < 2^31");
  PP_CHECK_ARG(ctx, order == PP_MASK_ORDER_ROW || order == PP_MASK_ORDER_COLUMN, PP_ERR_ARG, "pp_mask_rle: unknown order %d", order);
  PP_CHECK_ARG(ctx, masks && workspace && run_offsets && run_offsets_host && capacity >= 0 && (counts || capacity == 0), PP_ERR_ARG,
               "pp_mask_rle: null argument or negative capacity");
  PP_CHECK_ARG(ctx, workspace_bytes >= pp_mask_rle_workspace_bytes(n_mask), PP_ERR_ARG, "pp_mask_rle: workspace of %zu bytes, need %zu",
               workspace_bytes, pp_mask_rle_workspace_bytes(n_mask));
  int* n_run = (int*)workspace;
  hipLaunchKernelGGL(mask_rle_kernel<false>, dim3(n_mask), dim3(MASK_TILE), 0, ctx->stream, H, W, order, masks, n_run, (const int*)nullptr,
                     (int*)nullptr);
  hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, n_mask, (const int*)n_run, run_offsets, (int*)nullptr);
  PP_CHECK_LAUNCH(ctx, "pp_mask_rle");
  PP_HIP(ctx, hipMemcpyAsync(run_offsets_host, run_offsets, (size_t)(n_mask + 1) * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  PP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int n = 0; n < n_mask; ++n)
    PP_CHECK_ARG(ctx, run_offsets_host[n + 1] <= capacity, PP_ERR_ARG,
                 "pp_mask_rle: mask %d brings the runs to %d, the capacity is %lld (all %d masks need %d); nothing was written", n,
                 run_offsets_host[n + 1], capacity, n_mask, run_offsets_host[n_mask]);
  hipLaunchKernelGGL(mask_rle_kernel<true>, dim3(n_mask), dim3(MASK_TILE), 0, ctx->stream, H, W, order, masks, (int*)nullptr,
                     (const int*)run_offsets, counts);
  PP_CHECK_LAUNCH(ctx, "pp_mask_rle");
  return PP_OK;
}

// One workgroup per mask over its runs in steps of MASK_TILE: an inclusive scan of the lengths in LDS with a carry gives each
// run its first position; the thread of an odd run (the set ones) writes its 255s.  The masks were zeroed by the entry point.
static __global__ __launch_bounds__(MASK_TILE) void mask_from_rle_kernel(int H, int W, int order, const int* __restrict__ run_offsets,
                                                                        const int* __restrict__ counts, unsigned char* __restrict__ masks) {
  __shared__ int s[MASK_TILE];
  __shared__ int carry;
  const int HW = H * W, tid = threadIdx.x;
  const size_t n = blockIdx.x;
  const int r0 = run_offsets[n], nr = run_offsets[n + 1] - r0;
  unsigned char* m = masks + n * (size_t)HW;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nr; base += MASK_TILE) {
    const int i = base + tid;
    const int len = i < nr ? counts[r0 + i] : 0;
    s[tid] = len;
    __syncthreads();
    for (int off = 1; off < MASK_TILE; off <<= 1) {
      const int u = tid >= off ? s[tid - off] : 0;
      __syncthreads();
      s[tid] += u;
      __syncthreads();
    }
    const int start = carry + s[tid] - len;
    if ((i & 1) && len > 0 && start >= 0 && start <= HW - len) {  // (the host copy of the counts has been checked)
      for (int p = start; p < start + len; ++p) m[order == PP_MASK_ORDER_ROW ? (size_t)p : (size_t)(p % H) * W + p / H] = 255;
    }
    __syncthreads();
    if (tid == MASK_TILE - 1) carry += s[MASK_TILE - 1];
    __syncthreads();
  }
}

extern "C" int pp_mask_from_rle(pp_ctx* ctx, int n_mask, int H, int W, int order, const int* run_offsets_host, const int* counts_host,
                                const int* run_offsets, const int* counts, unsigned char* masks) {
  PP_REQUIRE_CTX(ctx);
  const int rc = mask_shape_ok(ctx, "pp_mask_from_rle", n_mask, H, W);
  if (rc != PP_OK) return rc;
  PP_CHECK_ARG(ctx, n_mask >= 1 && (long long)n_mask * H * W < (1ll << 40), PP_ERR_SHAPE, "pp_mask_from_rle: need n_mask >= 1");
  PP_CHECK_ARG(ctx, order == PP_MASK_ORDER_ROW || order == PP_MASK_ORDER_COLUMN, PP_ERR_ARG, "pp_mask_from_rle: unknown order %d", order);
  PP_CHECK_ARG(ctx, run_offsets_host && counts_host && run_offsets && counts && masks, PP_ERR_ARG, "pp_mask_from_rle: null argument");
  PP_CHECK_ARG(ctx, run_offsets_host[0] == 0, PP_ERR_ARG, "pp_mask_from_rle: run_offsets must start at 0");
  const long long HW = (long long)H * W;
  for (int n = 0; n < n_mask; ++n) {
    const int a = run_offsets_host[n], b = run_offsets_host[n + 1];
    PP_CHECK_ARG(ctx, b >= a, PP_ERR_ARG, "pp_mask_from_rle: run_offsets decrease at mask %d", n);
    long long sum = 0;
    for (int i = a; i < b; ++i) {
      PP_CHECK_ARG(ctx, counts_host[i] >= 0, PP_ERR_ARG, "pp_mask_from_rle: mask %d has a negative run length", n);
      sum += counts_host[i];
    }
    PP_CHECK_ARG(ctx, sum == HW, PP_ERR_ARG, "pp_mask_from_rle: the runs of mask %d add up to %lld, the image has %lld pixels", n, sum, HW);
  }
  PP_HIP(ctx, hipMemsetAsync(masks, 0, (size_t)n_mask * (size_t)HW, ctx->stream));
  hipLaunchKernelGGL(mask_from_rle_kernel, dim3(n_mask), dim3(MASK_TILE), 0, ctx->stream, H, W, order, run_offsets, counts, masks);
  PP_CHECK_LAUNCH(ctx, "pp_mask_from_rle");
  return PP_OK;
}
