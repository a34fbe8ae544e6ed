// pp_vote_cluster: each (image, class) vote list of pp_score_threshold_compact split into object instances before PnP.
// The reference has no such step -- it pools every vote of a class into one RANSAC problem because "occurences of 2 or more
// instances not possible in LINEMOD" (utils/tless_eval.py:378); on T-LESS scenes that hold several instances of one object the
// pooled problem mixes their poses.  This is the library's own step, restated in tests/cluster_np.py.
//
// One workgroup per (image, class), greedy rounds like the per-class suppression of detect.hip:
//   vote box  = axis-aligned box of the vote's 8 predicted corners (float32 min / max: exact); a vote with a non-finite
//               corner (or an anchor index outside [0, n)) is invalid: it never leads, never joins, instance -1
//   leader    = the unassigned valid vote with the highest class score (float32 compare), ties -> lowest position in the list
//               (= lowest anchor index: the list is ascending)
//   members   = the leader and every unassigned valid vote with IoU(leader box, vote box) > iou_thr; IoU in float64 on the
//               float32 boxes, no "+1", every product and sum rounded on its own (compiled with -ffp-contract=off)
//   kept      = at least min_votes members -> next instance id; otherwise the members are dropped (-1); consumed either way
//   stop      = nothing unassigned, max_instances kept, or max_rounds leaders
// Regrouping (anchor indices instance-major, ascending within an instance) happens in the round that keeps a cluster: the
// offset of a kept cluster is the number of votes kept before it, and an ordered ballot compaction writes its members.
//
// Work split: wave w of the workgroup owns one contiguous slice of the vote list in every pass, lane l the votes slice + l +
// 64 i -- so a vote's state (in `inst`: -2 unassigned, -1 out, >= 0 instance) is read and written by one thread only, the
// leader search is an integer max over (score, position) keys and the member count an integer sum: bit-identical run to run
// and independent of the batch.  Boxes and scores of the first VC_CACHE votes are cached in LDS, the rest are recomputed from
// boxes3d each round, so any count up to cap works without a workspace.
#include "pp_internal.h"

#define VC_THREADS 512
#define VC_WAVES (VC_THREADS / 64)
#define VC_CACHE 2048  // votes whose box and score stay in LDS (20 bytes each)

// (score, position) -> key whose unsigned order is score ascending, then position descending; 0 is below every key
__device__ __forceinline__ unsigned long long vc_key(float s, int v) {
  unsigned int b = __float_as_uint(s + 0.0f);  // -0 -> +0: the float compare sees them equal
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((unsigned long long)b << 32) | (unsigned int)(0x7fffffff - v);
}

__device__ __forceinline__ bool vc_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// box = (x1, y1, x2, y2) of the 8 corners at p; false when a corner is not finite
__device__ __forceinline__ bool vc_box(const float* __restrict__ p, float4& box) {
  float x1 = p[0], y1 = p[1], x2 = p[0], y2 = p[1];
  bool fin = vc_finite(p[0]) && vc_finite(p[1]);
#pragma unroll
  for (int j = 1; j < 8; ++j) {
    const float x = p[2 * j], y = p[2 * j + 1];
    fin = fin && vc_finite(x) && vc_finite(y);
    x1 = fminf(x1, x); y1 = fminf(y1, y);
    x2 = fmaxf(x2, x); y2 = fmaxf(y2, y);
  }
  box = make_float4(x1, y1, x2, y2);
  return fin;
}

__device__ __forceinline__ double vc_iou(const float4 a, const float4 b) {
  double w = fmin((double)a.z, (double)b.z) - fmax((double)a.x, (double)b.x);
  double h = fmin((double)a.w, (double)b.w) - fmax((double)a.y, (double)b.y);
  w = w > 0.0 ? w : 0.0;
  h = h > 0.0 ? h : 0.0;
  const double inter = w * h;
  const double area_a = ((double)a.z - (double)a.x) * ((double)a.w - (double)a.y);
  const double area_b = ((double)b.z - (double)b.x) * ((double)b.w - (double)b.y);
  const double ua = (area_a + area_b) - inter;
  return ua > 0.0 ? inter / ua : 0.0;
}

__global__ __launch_bounds__(VC_THREADS) void vote_cluster_kernel(
    int n, int C, int cap, const float* __restrict__ boxes3d, const float* __restrict__ scores, const int* __restrict__ idx,
    const int* __restrict__ counts, double iou_thr, int min_votes, int max_inst, int max_rounds, int* inst, int* __restrict__ order,
    int* __restrict__ inst_offsets, int* __restrict__ n_inst, int* __restrict__ leader, float* __restrict__ inst_box) {
  const int c = blockIdx.x, b = blockIdx.y;
  const size_t cell = (size_t)b * C + c;
  int cnt = counts[cell];
  if (cnt > cap) cnt = cap;  // pp_score_threshold_compact counts every hit and lists the first cap
  if (cnt <= 0) return;      // the entry point has filled this cell's outputs
  const float* box_b = boxes3d + (size_t)b * n * 16;
  const float* score_b = scores + (size_t)b * n * C + c;
  const int* idx_row = idx + cell * cap;
  int* inst_row = inst + cell * cap;
  int* order_row = order + cell * cap;

  __shared__ float4 s_box[VC_CACHE];
  __shared__ float s_score[VC_CACHE];
  __shared__ unsigned long long s_key[VC_WAVES];
  __shared__ int s_cnt[VC_WAVES];
  __shared__ float4 s_lead;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = (((cnt + VC_WAVES - 1) / VC_WAVES) + 63) & ~63;  // slice length, a multiple of the wave
  const int lo = wave * per < cnt ? wave * per : cnt;
  const int hi = lo + per < cnt ? lo + per : cnt;

  for (int v = lo + lane; v < hi; v += 64) {
    const int a = idx_row[v];
    bool ok = a >= 0 && a < n;
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.f;
    if (ok) {
      ok = vc_box(box_b + (size_t)a * 16, box);
      s = score_b[(size_t)a * C];
    }
    if (v < VC_CACHE) {
      s_box[v] = box;
      s_score[v] = s;
    }
    inst_row[v] = ok ? -2 : -1;
  }

  int n_kept = 0, total = 0;  // uniform across the workgroup
  for (int round = 0; round < max_rounds && n_kept < max_inst; ++round) {
    // leader: max (score, -position) over the unassigned votes
    unsigned long long best = 0ull;
    for (int v = lo + lane; v < hi; v += 64) {
      if (inst_row[v] != -2) continue;
      const float s = v < VC_CACHE ? s_score[v] : score_b[(size_t)idx_row[v] * C];
      const unsigned long long k = vc_key(s, v);
      best = k > best ? k : best;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const unsigned long long o = __shfl_xor(best, d, 64);
      best = o > best ? o : best;
    }
    if (lane == 0) s_key[wave] = best;
    __syncthreads();
    best = s_key[0];
#pragma unroll
    for (int w = 1; w < VC_WAVES; ++w) best = s_key[w] > best ? s_key[w] : best;
    if (best == 0ull) break;  // nothing unassigned (uniform: every thread read the same keys)
    const int lv = 0x7fffffff - (int)(unsigned int)(best & 0xffffffffull);
    if (lv >= lo && lv < hi && ((lv - lo) & 63) == lane) {  // the thread that owns the leader publishes its box
      float4 box;
      if (lv < VC_CACHE) box = s_box[lv];
      else vc_box(box_b + (size_t)idx_row[lv] * 16, box);
      s_lead = box;
    }
    __syncthreads();
    const float4 L = s_lead;

    // members: tentatively given the id this cluster gets if it is kept
    int m = 0;
    for (int v = lo + lane; v < hi; v += 64) {
      if (inst_row[v] != -2) continue;
      bool in = v == lv;
      if (!in) {
        float4 box;
        if (v < VC_CACHE) box = s_box[v];
        else vc_box(box_b + (size_t)idx_row[v] * 16, box);
        in = vc_iou(L, box) > iou_thr;
      }
      if (in) {
        inst_row[v] = n_kept;
        ++m;
      }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m += __shfl_xor(m, d, 64);
    if (lane == 0) s_cnt[wave] = m;
    __syncthreads();
    int members = 0, before = 0;
#pragma unroll
    for (int w = 0; w < VC_WAVES; ++w) {
      before += w < wave ? s_cnt[w] : 0;
      members += s_cnt[w];
    }

    if (members >= min_votes) {
      // ordered scatter of this instance's anchors: slices are contiguous and ascending, so wave w starts after waves < w
      int pos = total + before;
      for (int v0 = lo; v0 < hi; v0 += 64) {
        const int v = v0 + lane;
        const bool in = v < hi && inst_row[v] == n_kept;
        const unsigned long long bal = __ballot(in);
        if (in) order_row[pos + __popcll(bal & ((1ull << lane) - 1ull))] = idx_row[v];
        pos += __popcll(bal);
      }
      if (threadIdx.x == 0) {
        inst_offsets[cell * (max_inst + 1) + n_kept] = total;
        leader[cell * max_inst + n_kept] = idx_row[lv];
        float* ob = inst_box + (cell * max_inst + n_kept) * 4;
        ob[0] = L.x; ob[1] = L.y; ob[2] = L.z; ob[3] = L.w;
      }
      total += members;
      ++n_kept;
    } else {
      for (int v = lo + lane; v < hi; v += 64)
        if (inst_row[v] == n_kept) inst_row[v] = -1;
    }
    __syncthreads();  // s_key, s_cnt and s_lead are rewritten by the next round
  }

  for (int v = lo + lane; v < hi; v += 64)
    if (inst_row[v] == -2) inst_row[v] = -1;
  for (int k = n_kept + threadIdx.x; k <= max_inst; k += VC_THREADS) inst_offsets[cell * (max_inst + 1) + k] = total;
  if (threadIdx.x == 0) n_inst[cell] = n_kept;
}

extern "C" size_t pp_vote_cluster_workspace_bytes(int batch, int n_class, int cap, int max_instances) {
  (void)batch; (void)n_class; (void)cap; (void)max_instances;
  return 0;  // per-vote state lives in `inst`, boxes are cached in LDS or recomputed
}

extern "C" int pp_vote_cluster(pp_ctx* ctx, int batch, int n, int n_class, int cap, const float* boxes3d, const float* scores,
                               const int* idx, const int* counts, double iou_thr, int min_votes, int max_instances, int max_rounds,
                               void* workspace, int* inst, int* order, int* inst_offsets, int* n_inst, int* leader, float* inst_box) {
  PP_REQUIRE_CTX(ctx);
  (void)workspace;
  PP_CHECK_ARG(ctx, boxes3d && scores && idx && counts && inst && order && inst_offsets && n_inst && leader && inst_box, PP_ERR_ARG,
               "pp_vote_cluster: null argument");
  PP_CHECK_ARG(ctx, batch > 0 && n > 0 && n_class > 0 && cap >= 1 && min_votes >= 1 && max_instances >= 1 && max_rounds >= 1, PP_ERR_ARG,
               "pp_vote_cluster: batch, n, n_class, cap, min_votes, max_instances and max_rounds must be >= 1");
  PP_CHECK_ARG(ctx, iou_thr >= 0.0 && iou_thr < 1.0, PP_ERR_ARG, "pp_vote_cluster: iou_thr must be in [0, 1)");
  PP_CHECK_ARG(ctx, batch <= 65535 && (long long)batch * n_class * ((long long)max_instances + 1) < (1ll << 31), PP_ERR_SHAPE,
               "pp_vote_cluster: unsupported size (images <= 65535, images * classes * (max_instances + 1) < 2^31)");
  const size_t cells = (size_t)batch * n_class;
  // the values of everything the kernel does not reach: padding, unused instance slots and every empty (image, class)
  PP_HIP(ctx, hipMemsetAsync(inst, 0xff, cells * cap * sizeof(int), ctx->stream));
  PP_HIP(ctx, hipMemsetAsync(order, 0xff, cells * cap * sizeof(int), ctx->stream));
  PP_HIP(ctx, hipMemsetAsync(leader, 0xff, cells * max_instances * sizeof(int), ctx->stream));
  PP_HIP(ctx, hipMemsetAsync(inst_offsets, 0, cells * ((size_t)max_instances + 1) * sizeof(int), ctx->stream));
  PP_HIP(ctx, hipMemsetAsync(n_inst, 0, cells * sizeof(int), ctx->stream));
  PP_HIP(ctx, hipMemsetAsync(inst_box, 0, cells * max_instances * 4 * sizeof(float), ctx->stream));
  hipLaunchKernelGGL(vote_cluster_kernel, dim3(n_class, batch), dim3(VC_THREADS), 0, ctx->stream, n, n_class, cap, boxes3d, scores, idx,
                     counts, iou_thr, min_votes, max_instances, max_rounds, inst, order, inst_offsets, n_inst, leader, inst_box);
  PP_CHECK_LAUNCH(ctx, "pp_vote_cluster");
  return PP_OK;
}
