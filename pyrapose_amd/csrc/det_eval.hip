// 2-D detection average precision on the device: pp_det_match, pp_det_pr_curve, pp_det_ap (include/pyrapose_hip.h states every
// rule; DESIGN.md 7b the layout).  Two rule sets:
//   PP_DET_RULE_REFERENCE  utils/eval.py:187-211 (evaluate): "+1" IoU of compute_overlap.pyx, first-maximum ground truth, no
//                          fall-back to the second best; pinned through tests/golden/detection_ap.npz
//   PP_DET_RULE_COCO       pycocotools' evaluateImg without crowd and area ranges, restated; parity unpinned
// and two integrations of the curve: PP_DET_AP_AREA (utils/eval.py:42-54 _compute_ap) and PP_DET_AP_101 (COCO's 101 recall points).
// Restated in tests/det_eval_np.py.  Compiled with -ffp-contract=off; no atomics anywhere: every result is bit-identical run to
// run and independent of the batch an image sits in.
#include <math.h>

#include "box_iou.h"
#include "pose_common.h"

#define DET_MAX_DET PP_DET_MAX_DET  // detection slots per image the LDS layout of det_match_kernel holds
#define DET_MAX_GT PP_DET_MAX_GT    // ground truth per image it holds
#define DET_MAX_THR PP_DET_MAX_THR  // thresholds per launch = waves per workgroup
#define DET_CHUNK PP_DET_SCAN_CHUNK // detections per scan step of det_pr_curve_kernel = its workgroup size
#define DET_IOU_BOXES 0  // det_match_kernel computes the IoU from the two boxes (pp_det_match)
#define DET_IOU_MATRIX 1 // it reads the IoU from a pair matrix, pp_mask_iou_pairs' layout (pp_det_match_iou)

struct det_thresholds {
  double v[DET_MAX_THR];
};

// score -> key whose unsigned order is the score's (-0 and +0 equal, as the float compare has them)
__device__ __forceinline__ unsigned long long det_key(double s) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(s + 0.0);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// One workgroup per image, one wave per threshold.
//   1. every thread: the image's ground truth (box, label, ignore flag) and the detections' score keys into LDS
//   2. every thread: rank counting -- rank(d) = number of valid slots e with key(e) > key(d), or key(e) == key(d) and e < d;
//      s_order[rank] = d.  A slot whose label is outside [0, C) is padding: not ranked, match -1, det_ignored 0.
//   3. wave t walks s_order.  Lane l owns the ground truth l, l + 64, ... of the image: it alone reads and writes their taken
//      flags (s_taken[t][.]) and computes their IoU with the detection; a butterfly picks the wave's winner under the rule's
//      tie-break; the owner of the winner decides and marks it, lane 0 writes the outcome.
// SRC = DET_IOU_MATRIX: `det_boxes` is the pair matrix instead (the IoU of slot d and ground truth g of image b at
// D * gt_offsets[b] + d * ng_b + g), `gt_boxes` is not read and s_gt is not filled.  The kernel's arguments are the same for
// both sources, so the box instantiations are the instructions they were before the second source existed.
template <int RULE, int SRC>
__global__ __launch_bounds__(64 * DET_MAX_THR) void det_match_kernel(
    int D, int C, int T, const double* __restrict__ det_boxes, const double* __restrict__ det_scores, const int* __restrict__ det_labels,
    const double* __restrict__ gt_boxes, const int* __restrict__ gt_labels, const unsigned char* __restrict__ gt_ignore,
    const int* __restrict__ gt_offsets, det_thresholds thr, int* __restrict__ match, unsigned char* __restrict__ det_ignored) {
  __shared__ double s_gt[DET_MAX_GT][4];
  __shared__ int s_meta[DET_MAX_GT];  // label, or -1 - label for an ignored ground truth; INT_MIN for a label outside [0, C)
  __shared__ unsigned long long s_key[DET_MAX_DET];
  __shared__ unsigned short s_order[DET_MAX_DET];
  __shared__ unsigned char s_taken[DET_MAX_THR][DET_MAX_GT];
  __shared__ int s_nvalid;

  const int b = blockIdx.x, B = gridDim.x;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, t = tid >> 6;
  const int g0 = gt_offsets[b];
  int ng = gt_offsets[b + 1] - g0;
  ng = ng < 0 ? 0 : (ng > DET_MAX_GT ? DET_MAX_GT : ng);  // (the entry point has checked the host copy)
  const double* box_b = det_boxes + (SRC == DET_IOU_BOXES ? (size_t)b * D * 4 : (size_t)D * (size_t)g0);
  const double* score_b = det_scores + (size_t)b * D;
  const int* label_b = det_labels + (size_t)b * D;
  int* match_t = match + ((size_t)t * B + b) * D;
  unsigned char* ign_t = det_ignored + ((size_t)t * B + b) * D;

  if (tid == 0) s_nvalid = 0;
  for (int g = tid; g < ng; g += nthr) {
    if (SRC == DET_IOU_BOXES) {
      const double* p = gt_boxes + (size_t)(g0 + g) * 4;
      const double x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
      s_gt[g][0] = x1; s_gt[g][1] = y1; s_gt[g][2] = x2; s_gt[g][3] = y2;
    }
    const int l = gt_labels[g0 + g];
    const bool ig = gt_ignore != nullptr && gt_ignore[g0 + g] != 0;
    s_meta[g] = (l < 0 || l >= C) ? (int)0x80000000 : (ig ? -1 - l : l);
  }
  for (int g = lane; g < ng; g += 64) s_taken[t][g] = 0;
  for (int d = tid; d < D; d += nthr) {
    const int l = label_b[d];
    s_key[d] = (l >= 0 && l < C) ? det_key(score_b[d]) : 0ull;  // 0 is below every key: padding
  }
  __syncthreads();
  for (int d = tid; d < D; d += nthr) {
    const unsigned long long k = s_key[d];
    if (k == 0ull) continue;
    int rank = 0;
    for (int e = 0; e < D; ++e) {
      const unsigned long long o = s_key[e];
      rank += (o > k || (o == k && e < d)) ? 1 : 0;
    }
    s_order[rank] = (unsigned short)d;
  }
  // the valid slots, counted in slot order by the first wave (an integer sum)
  if (t == 0) {
    int n = 0;
    for (int d = lane; d < D; d += 64) n += s_key[d] != 0ull ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) s_nvalid = n;
  }
  __syncthreads();
  if (t >= T) return;
  const int nvalid = s_nvalid;

  // padding slots: nothing else writes them
  for (int d = lane; d < D; d += 64) {
    if (s_key[d] == 0ull) {
      match_t[d] = -1;
      ign_t[d] = 0;
    }
  }
  if (nvalid == 0) return;
  if (ng == 0) {  // every detection of an image without ground truth is a false positive
    for (int k = lane; k < nvalid; k += 64) {
      const int d = s_order[k];
      match_t[d] = -1;
      ign_t[d] = 0;
    }
    return;
  }

  const double thr_t = thr.v[t];
  const double thr_coco = thr_t < 1.0 - 1e-10 ? thr_t : 1.0 - 1e-10;
  for (int k = 0; k < nvalid; ++k) {
    const int d = s_order[k];
    const int label = label_b[d];
    double dx1 = 0.0, dy1 = 0.0, dx2 = 0.0, dy2 = 0.0;
    if (SRC == DET_IOU_BOXES) {
      dx1 = box_b[4 * d]; dy1 = box_b[4 * d + 1]; dx2 = box_b[4 * d + 2]; dy2 = box_b[4 * d + 3];
    }
    const double* iou_d = box_b + (size_t)d * ng;  // (SRC = DET_IOU_MATRIX only)
    // this lane's candidate: `cls` 1 for a ground truth that is not ignored, 0 for an ignored one, -1 for none
    int best_g = -1, best_cls = -1;
    double best = 0.0;
    for (int g = lane; g < ng; g += 64) {
      const int m = s_meta[g];
      if (RULE == PP_DET_RULE_REFERENCE) {
        if (m != label) continue;
        double v;
        if (SRC == DET_IOU_BOXES) {
          const double gx1 = s_gt[g][0], gy1 = s_gt[g][1], gx2 = s_gt[g][2], gy2 = s_gt[g][3];
          v = iou_plus1(dx1, dy1, dx2, dy2, gx1, gy1, gx2, gy2, (gx2 - gx1 + 1) * (gy2 - gy1 + 1));
        } else {
          v = iou_d[g];
        }
        if (best_g < 0 || v > best) {  // first maximum: ascending g, strict >
          best = v;
          best_g = g;
          best_cls = 1;
        }
      } else {
        const int cls = m == label ? 1 : (m == -1 - label ? 0 : -1);
        if (cls < 0 || s_taken[t][g]) continue;
        double v;
        if (SRC == DET_IOU_BOXES) {
          const double gx1 = s_gt[g][0], gy1 = s_gt[g][1], gx2 = s_gt[g][2], gy2 = s_gt[g][3];
          v = iou_plain(dx1, dy1, dx2, dy2, gx1, gy1, gx2, gy2, (gx2 - gx1) * (gy2 - gy1));
        } else {
          v = iou_d[g];
        }
        if (!(v >= thr_coco)) continue;
        // a ground truth that is not ignored beats an ignored one (the search stops before them); then the higher IoU; then the
        // later one in visiting order (ascending g within each kind)
        if (cls > best_cls || (cls == best_cls && v >= best)) {
          best = v;
          best_g = g;
          best_cls = cls;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(best, o, 64);
      const int og = __shfl_xor(best_g, o, 64);
      const int oc = __shfl_xor(best_cls, o, 64);
      bool take;
      if (RULE == PP_DET_RULE_REFERENCE) take = og >= 0 && (best_g < 0 || ov > best || (ov == best && og < best_g));
      else take = oc > best_cls || (oc == best_cls && oc >= 0 && (ov > best || (ov == best && og > best_g)));
      if (take) {
        best = ov;
        best_g = og;
        best_cls = oc;
      }
    }
    // the owner of the winner decides and marks it
    int hit = 0;
    if (best_g >= 0 && (best_g & 63) == lane) {
      if (RULE == PP_DET_RULE_REFERENCE) {
        hit = (best >= thr_t && !s_taken[t][best_g]) ? 1 : 0;
        if (hit) s_taken[t][best_g] = 1;
      } else {
        hit = 1;
        s_taken[t][best_g] = 1;
      }
    }
    hit = best_g >= 0 ? __shfl(hit, best_g & 63, 64) : 0;
    if (lane == 0) {
      match_t[d] = hit ? g0 + best_g : -1;
      ign_t[d] = (hit && best_cls == 0) ? 1 : 0;
    }
  }
}

// npos[c] = ground truth of class c that is not ignored, over the whole batch: one workgroup per class, an integer sum
static __global__ __launch_bounds__(POSE_TILE) void det_npos_kernel(int n_gt, const int* __restrict__ gt_labels,
                                                                   const unsigned char* __restrict__ gt_ignore, int* __restrict__ npos) {
  __shared__ int s[POSE_TILE];
  const int c = blockIdx.x, tid = threadIdx.x;
  int n = 0;
  for (int g = tid; g < n_gt; g += POSE_TILE) n += (gt_labels[g] == c && !(gt_ignore && gt_ignore[g])) ? 1 : 0;
  s[tid] = n;
  __syncthreads();
  for (int w = POSE_TILE / 2; w > 0; w >>= 1) {
    if (tid < w) s[tid] += s[tid + w];
    __syncthreads();
  }
  if (tid == 0) npos[c] = s[0];
}

// pp_det_match and pp_det_match_iou: the common checks and the two launches.  iou == nullptr: boxes.
static int det_match_launch(pp_ctx* ctx, const char* who, int batch, int n_det, int n_gt, int n_class, const double* det_boxes,
                            const double* iou, const double* det_scores, const int* det_labels, const double* gt_boxes,
                            const int* gt_labels, const unsigned char* gt_ignore, const int* gt_offsets_host, const int* gt_offsets_dev,
                            int n_thr, const double* thresholds, int rule, int* match, unsigned char* det_ignored, int* npos) {
  const bool boxes = iou == nullptr;
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, rule == PP_DET_RULE_REFERENCE || rule == PP_DET_RULE_COCO, PP_ERR_ARG, "%s: unknown rule %d", who, rule);
  PP_CHECK_ARG(ctx, n_thr >= 1 && n_thr <= DET_MAX_THR, PP_ERR_ARG, "%s: need 1..%d thresholds, got %d", who, DET_MAX_THR, n_thr);
  PP_CHECK_ARG(ctx, batch >= 1 && n_class >= 1 && n_gt >= 0, PP_ERR_ARG, "%s: batch and n_class must be >= 1, n_gt >= 0", who);
  PP_CHECK_ARG(ctx, n_det >= 0 && n_det <= DET_MAX_DET, PP_ERR_ARG, "%s: %d detection slots per image, the limit is %d", who, n_det,
               DET_MAX_DET);
  PP_CHECK_ARG(ctx, (long long)n_thr * batch * n_det < (1ll << 31), PP_ERR_ARG, "%s: T * batch * n_det must stay below 2^31", who);
  PP_CHECK_ARG(ctx, boxes || (long long)n_det * n_gt < (1ll << 31), PP_ERR_ARG, "%s: n_det * n_gt pairs must stay below 2^31", who);
  PP_CHECK_ARG(ctx, thresholds && gt_offsets_host && gt_offsets_dev && npos, PP_ERR_ARG, "%s: null argument", who);
  PP_CHECK_ARG(ctx, n_det == 0 || ((boxes ? det_boxes != nullptr : true) && det_scores && det_labels && match && det_ignored), PP_ERR_ARG,
               "%s: null detection tensor", who);
  PP_CHECK_ARG(ctx, n_gt == 0 || ((boxes ? gt_boxes != nullptr : true) && gt_labels), PP_ERR_ARG, "%s: null ground-truth tensor", who);
  PP_CHECK_ARG(ctx, rule == PP_DET_RULE_COCO || gt_ignore == nullptr, PP_ERR_ARG,
               "%s: the reference rule has no ignored ground truth (gt_ignore must be NULL)", who);
  det_thresholds thr = {};
  for (int t = 0; t < n_thr; ++t) {
    const double v = thresholds[t];
    PP_CHECK_ARG(ctx, v >= 0.0 && v <= 1.0 && (t == 0 || v > thresholds[t - 1]), PP_ERR_ARG,
                 "%s: thresholds must increase within [0, 1]", who);
    thr.v[t] = v;
  }
  PP_CHECK_ARG(ctx, gt_offsets_host[0] == 0 && gt_offsets_host[batch] == n_gt, PP_ERR_ARG, "%s: gt_offsets must run from 0 to n_gt", who);
  for (int b = 0; b < batch; ++b) {
    const int n = gt_offsets_host[b + 1] - gt_offsets_host[b];
    PP_CHECK_ARG(ctx, n >= 0, PP_ERR_ARG, "%s: gt_offsets decrease at image %d", who, b);
    PP_CHECK_ARG(ctx, n <= DET_MAX_GT, PP_ERR_ARG, "%s: image %d has %d ground truths, the limit is %d", who, b, n, DET_MAX_GT);
  }
  hipLaunchKernelGGL(det_npos_kernel, dim3(n_class), dim3(POSE_TILE), 0, ctx->stream, n_gt, gt_labels, gt_ignore, npos);
  if (n_det > 0 && boxes) {
    auto kernel = rule == PP_DET_RULE_REFERENCE ? det_match_kernel<PP_DET_RULE_REFERENCE, DET_IOU_BOXES>
                                                : det_match_kernel<PP_DET_RULE_COCO, DET_IOU_BOXES>;
    hipLaunchKernelGGL(kernel, dim3(batch), dim3(64 * n_thr), 0, ctx->stream, n_det, n_class, n_thr, det_boxes, det_scores, det_labels,
                       gt_boxes, gt_labels, gt_ignore, gt_offsets_dev, thr, match, det_ignored);
  } else if (n_det > 0 && (n_gt > 0 || iou)) {
    auto kernel = rule == PP_DET_RULE_REFERENCE ? det_match_kernel<PP_DET_RULE_REFERENCE, DET_IOU_MATRIX>
                                                : det_match_kernel<PP_DET_RULE_COCO, DET_IOU_MATRIX>;
    hipLaunchKernelGGL(kernel, dim3(batch), dim3(64 * n_thr), 0, ctx->stream, n_det, n_class, n_thr, iou, det_scores, det_labels,
                       (const double*)nullptr, gt_labels, gt_ignore, gt_offsets_dev, thr, match, det_ignored);
  }
  PP_CHECK_LAUNCH(ctx, who);
  return PP_OK;
}

extern "C" int pp_det_match(pp_ctx* ctx, int batch, int n_det, int n_gt, int n_class, const double* det_boxes, const double* det_scores,
                            const int* det_labels, const double* gt_boxes, const int* gt_labels, const unsigned char* gt_ignore,
                            const int* gt_offsets_host, const int* gt_offsets_dev, int n_thr, const double* thresholds, int rule,
                            int* match, unsigned char* det_ignored, int* npos) {
  return det_match_launch(ctx, "pp_det_match", batch, n_det, n_gt, n_class, det_boxes, nullptr, det_scores, det_labels, gt_boxes, gt_labels,
                          gt_ignore, gt_offsets_host, gt_offsets_dev, n_thr, thresholds, rule, match, det_ignored, npos);
}

extern "C" int pp_det_match_iou(pp_ctx* ctx, int batch, int n_det, int n_gt, int n_class, const double* iou, const double* det_scores,
                                const int* det_labels, const int* gt_labels, const unsigned char* gt_ignore, const int* gt_offsets_host,
                                const int* gt_offsets_dev, int n_thr, const double* thresholds, int rule, int* match,
                                unsigned char* det_ignored, int* npos) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, iou != nullptr, PP_ERR_ARG, "pp_det_match_iou: null IoU matrix (one double is enough when there are no pairs)");
  return det_match_launch(ctx, "pp_det_match_iou", batch, n_det, n_gt, n_class, nullptr, iou, det_scores, det_labels, nullptr, gt_labels,
                          gt_ignore, gt_offsets_host, gt_offsets_dev, n_thr, thresholds, rule, match, det_ignored, npos);
}

// One workgroup of DET_CHUNK threads per (class, threshold): the class's segment of `order` in chunks with a carry.
//   forward: tp / fp as inclusive int32 sums (an ignored detection adds to neither), recall and precision from them
//   reverse: prec_env[i] = max(precision[i], prec_env[i + 1]) from the segment's end (a maximum is exact in any order)
static __global__ __launch_bounds__(DET_CHUNK) void det_pr_curve_kernel(
    int N, long long BD, const int* __restrict__ order, const int* __restrict__ class_offsets, const int* __restrict__ match,
    const unsigned char* __restrict__ det_ignored, const int* __restrict__ npos, int* __restrict__ tp_out, int* __restrict__ fp_out,
    double* __restrict__ recall, double* prec_env) {
  __shared__ int s_tp[DET_CHUNK], s_fp[DET_CHUNK];
  __shared__ double s_max[DET_CHUNK];
  __shared__ int c_tp, c_fp;
  __shared__ double c_max;
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  int lo = class_offsets[c], hi = class_offsets[c + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > N ? N : hi;
  if (hi <= lo) return;
  const int n = hi - lo;
  const int* match_t = match + (size_t)t * BD;
  const unsigned char* ign_t = det_ignored + (size_t)t * BD;
  const size_t row = (size_t)t * N + lo;
  const double np_c = (double)npos[c];
  if (tid == 0) {
    c_tp = 0;
    c_fp = 0;
    c_max = 0.0;  // the sentinel _compute_ap appends to the precision (eval.py:43)
  }
  __syncthreads();
  for (int base = 0; base < n; base += DET_CHUNK) {
    const int i = base + tid;
    int a = 0, f = 0;
    if (i < n) {
      const long long det = order[lo + i];
      if (det >= 0 && det < BD && !ign_t[det]) {
        a = match_t[det] >= 0 ? 1 : 0;
        f = 1 - a;
      }
    }
    s_tp[tid] = a;
    s_fp[tid] = f;
    __syncthreads();
    for (int off = 1; off < DET_CHUNK; off <<= 1) {
      const int ua = tid >= off ? s_tp[tid - off] : 0;
      const int uf = tid >= off ? s_fp[tid - off] : 0;
      __syncthreads();
      s_tp[tid] += ua;
      s_fp[tid] += uf;
      __syncthreads();
    }
    if (i < n) {
      const int tpi = c_tp + s_tp[tid], fpi = c_fp + s_fp[tid];
      tp_out[row + i] = tpi;
      fp_out[row + i] = fpi;
      const double tpd = (double)tpi, den = tpd + (double)fpi;
      recall[row + i] = np_c > 0.0 ? tpd / np_c : 0.0;                                    // eval.py:228
      prec_env[row + i] = tpd / (den > 2.220446049250313e-16 ? den : 2.220446049250313e-16);  // eval.py:229
    }
    __syncthreads();
    if (tid == DET_CHUNK - 1) {
      c_tp += s_tp[tid];
      c_fp += s_fp[tid];
    }
    __syncthreads();  // also: this workgroup's precision stores are visible to its reverse pass
  }
  for (int base = 0; base < n; base += DET_CHUNK) {
    const int i = n - 1 - (base + tid);  // thread 0 holds the chunk's last element
    s_max[tid] = i >= 0 ? prec_env[row + i] : 0.0;
    __syncthreads();
    for (int off = 1; off < DET_CHUNK; off <<= 1) {
      const double u = tid >= off ? s_max[tid - off] : 0.0;
      __syncthreads();
      s_max[tid] = u > s_max[tid] ? u : s_max[tid];
      __syncthreads();
    }
    if (i >= 0) prec_env[row + i] = c_max > s_max[tid] ? c_max : s_max[tid];
    __syncthreads();
    if (tid == DET_CHUNK - 1) c_max = c_max > s_max[tid] ? c_max : s_max[tid];
    __syncthreads();
  }
}

extern "C" int pp_det_pr_curve(pp_ctx* ctx, int n_thr, int n_order, int n_class, long long n_slots, const int* order,
                               const int* class_offsets, const int* match, const unsigned char* det_ignored, const int* npos, int* tp,
                               int* fp, double* recall, double* prec_env) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, n_thr >= 1 && n_thr <= DET_MAX_THR, PP_ERR_ARG, "pp_det_pr_curve: need 1..%d thresholds, got %d", DET_MAX_THR, n_thr);
  PP_CHECK_ARG(ctx, n_class >= 1 && n_order >= 0 && n_slots >= n_order && n_slots * n_thr < (1ll << 31), PP_ERR_ARG,
               "pp_det_pr_curve: need n_class >= 1, 0 <= n_order <= n_slots, T * n_slots < 2^31");
  PP_CHECK_ARG(ctx, class_offsets && npos, PP_ERR_ARG, "pp_det_pr_curve: null argument");
  if (n_order == 0) return PP_OK;
  PP_CHECK_ARG(ctx, order && match && det_ignored && tp && fp && recall && prec_env, PP_ERR_ARG, "pp_det_pr_curve: null argument");
  hipLaunchKernelGGL(det_pr_curve_kernel, dim3(n_class, n_thr), dim3(DET_CHUNK), 0, ctx->stream, n_order, n_slots, order, class_offsets,
                     match, det_ignored, npos, tp, fp, recall, prec_env);
  PP_CHECK_LAUNCH(ctx, "pp_det_pr_curve");
  return PP_OK;
}

// One workgroup of POSE_TILE threads per (class, threshold).
//   AREA: thread k sums the terms of its contiguous range [k per, (k + 1) per), per = ceil(n / POSE_TILE), in ascending order
//         from 0.0, then tile_sum256's halving tree over the POSE_TILE partials
//   101:  thread k < 101 looks up recall point k, thread 0 adds the 101 values in index order
static __global__ __launch_bounds__(POSE_TILE) void det_ap_kernel(int N, int C, int mode, const int* __restrict__ class_offsets,
                                                                 const int* __restrict__ npos, const double* __restrict__ recall,
                                                                 const double* __restrict__ prec_env, double* __restrict__ ap,
                                                                 double* __restrict__ recall_final) {
  __shared__ double red[POSE_TILE];
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const size_t cell = (size_t)t * C + c;
  int lo = class_offsets[c], hi = class_offsets[c + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > N ? N : hi;
  const int n = hi > lo ? hi - lo : 0;
  if (npos[c] <= 0) {  // eval.py:214-216: (0, 0); COCO leaves such a class at -1, out of every mean
    if (tid == 0) {
      ap[cell] = mode == PP_DET_AP_AREA ? 0.0 : -1.0;
      recall_final[cell] = mode == PP_DET_AP_AREA ? 0.0 : -1.0;
    }
    return;
  }
  const double* rec = recall + (size_t)t * N + lo;
  const double* env = prec_env + (size_t)t * N + lo;
  double result;
  if (mode == PP_DET_AP_AREA) {
    const int per = (n + POSE_TILE - 1) / POSE_TILE;
    const int j0 = tid * per < n ? tid * per : n;
    const int j1 = j0 + per < n ? j0 + per : n;
    double s = 0.0;
    for (int j = j0; j < j1; ++j) {
      const double prev = j > 0 ? rec[j - 1] : 0.0, cur = rec[j];  // mrec = (0, recall..., 1): the last term has precision 0
      if (cur != prev) s += (cur - prev) * env[j];                  // eval.py:51-54
    }
    result = tile_sum256(s, red);
  } else {
    double q = 0.0;
    if (tid < 101) {
      const double r = tid == 100 ? 1.0 : (double)tid * 0.01;  // np.linspace(0, 1, 101)
      int a = 0, z = n;                                         // np.searchsorted(recall, r, side='left')
      while (a < z) {
        const int m = (a + z) >> 1;
        if (rec[m] < r) a = m + 1;
        else z = m;
      }
      q = a < n ? env[a] : 0.0;
    }
    red[tid] = q;
    __syncthreads();
    result = 0.0;
    if (tid == 0) {
      for (int k = 0; k < 101; ++k) result += red[k];
      result = result / 101.0;
    }
  }
  if (tid == 0) {
    ap[cell] = result;
    recall_final[cell] = n > 0 ? rec[n - 1] : 0.0;
  }
}

extern "C" int pp_det_ap(pp_ctx* ctx, int n_thr, int n_order, int n_class, const int* class_offsets, const int* npos,
                         const double* recall, const double* prec_env, int mode, double* ap, double* recall_final) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, mode == PP_DET_AP_AREA || mode == PP_DET_AP_101, PP_ERR_ARG, "pp_det_ap: unknown integration %d", mode);
  PP_CHECK_ARG(ctx, n_thr >= 1 && n_thr <= DET_MAX_THR, PP_ERR_ARG, "pp_det_ap: need 1..%d thresholds, got %d", DET_MAX_THR, n_thr);
  PP_CHECK_ARG(ctx, n_class >= 1 && n_order >= 0 && (long long)n_thr * n_order < (1ll << 31), PP_ERR_ARG,
               "pp_det_ap: need n_class >= 1, n_order >= 0, T * n_order < 2^31");
  PP_CHECK_ARG(ctx, class_offsets && npos && ap && recall_final && (n_order == 0 || (recall && prec_env)), PP_ERR_ARG,
               "pp_det_ap: null argument");
  hipLaunchKernelGGL(det_ap_kernel, dim3(n_class, n_thr), dim3(POSE_TILE), 0, ctx->stream, n_order, n_class, mode, class_offsets, npos,
                     recall, prec_env, ap, recall_final);
  PP_CHECK_LAUNCH(ctx, "pp_det_ap");
  return PP_OK;
}
