// Shared pieces of the implicit-GEMM convolution kernels (conv.hip: f32 MFMA; the conv3 units and conv4.hip: 3 x bf16 MFMA):
// row-space geometry, the gather (row -> source offset per tap), the XCD-aware tile order, descriptor checks
// and the facts conv_plan.h's planners read.
#pragma once
#include <stdlib.h>

#include <type_traits>

#include "conv_plan.h"
#include "pp_internal.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));

struct SegGeo {
  int row_begin;      // first row (m) of the segment in the space the kernel enumerates
  int src_row_begin;  // first row of the segment in the gathered tensor
  int OH, OW;         // cells per image in the enumerated space
  int SH, SW;         // cells per image in the gathered tensor
};

struct IgemmParams {
  const float* src;
  const float* wgt;
  float* out;
  const float* bias;
  const float* addend;
  const float* mask_src;
  int ld_src, ld_w, ld_out, ld_add, ld_mask;
  int relu;
  int M, n_seg;
  SegGeo seg[PP_MAX_SEG];
  int Cred;        // reduction channels per tap (multiple of 16, or 4 for the packed-RGB stem)
  int Nout;        // output channels
  int w_tap_rows;  // weight rows per tap (= cin of the forward conv)
  int kh, kw;
  int mul, tsign, off_y, off_x, div;  // src = (pos*mul + tap*tsign + off) / div
  int n_tiles_n;
  long long src_rows;  // rows of the gathered tensor (all segments)
  // weight tap of loop tap (ty, tx) = (w_ty0 + w_tstep*ty) * w_kw + (w_tx0 + w_tstep*tx); identity: 0, 1, 0, kw
  int w_ty0, w_tx0, w_tstep, w_kw, w_taps;  // w_taps: taps in the weight planes (kh * kw of the conv)
  // stride-2 bwd-data by parity class: enumerated row (n, y', x') of the class grid seg[0].OH x OW is written to (and
  // reads addend / mask at) row (n*sc_H + 2y' + sc_cy) * sc_W + 2x' + sc_cx of the full tensor
  int sc_on, sc_H, sc_W, sc_cy, sc_cx;
  // epilogue operands stored as bf16 (hi, lo) planes instead of f32 (pp_conv_opts.add_hi / add_lo / mask_hi): the addend / residual
  // (value = hi + lo, geometry [rows][ld_add]) and the ReLU source (only its hi plane is read: hi > 0 <=> value > 0,
  // geometry [rows][ld_mask]).  When set they replace `addend` / `mask_src`.
  const void* add_hi;
  const void* add_lo;
  const void* mask_hi;
  int x_ty_inner;  // igemm3x: loop order of the (kernel row, channel chunk) groups
  int m_off;       // igemm3x / splitk_finish_kernel: first output row of THIS launch (the rows below belong to another launch:
                   // the remainder of a launch whose full rounds igemm4x_kernel took); split-K slices hold rows m_off .. M - 1
};

// the weight-gradient kernels (conv3_wgrad.hip: wgrad3 / wgrad3f; conv4.hip: wgrad3r)
struct Wgrad3Params {
  int ld_src, ld_dy, ld_w;
  int M, n_seg;
  SegGeo seg[PP_MAX_SEG];
  int Cin, Cout;
  int kh, kw, stride, pad_t, pad_l;
  int k_tiles_per_tap, n_tiles_k, n_tiles_n, splits, rows_per_split;
  int max_wraps;  // ceil(32 / narrowest level width): row wraps one 32-row step can cross
  int sp_min_steps;  // SP: listed 32-row blocks one workgroup should at least reduce (fewer splits when the list is short)
  long long src_rows;
  const float* inv_scale;  // device scalar 2^-G (NULL: 1): dy travels multiplied by 2^G (pp_ctx_set_grad_scale), dW / dbias leave unscaled
  // wgrad3r (conv4.hip), dense reduction: the position space with one pad behind every image row -- first position of each level, total
  int pos_begin[PP_MAX_SEG];
  int Mp;
};

// Workgroups are dealt round-robin over the 8 XCDs (block b -> XCD b % 8, each with a private L2).
// Remap so that every XCD walks a CONTIGUOUS range of logical tiles: the N-tiles of one M-tile (same A
// rows) and neighbouring M-tiles (overlapping 3x3 halos, same weight step) then share one L2.
// Bijective for any grid size (cdna_hip_programming.md T1).  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int b, int n) {
  const int q = n >> 3, r = n & 7;
  const int x = b & 7, j = b >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
}

template <int V>
struct VecT;
template <>
struct VecT<1> { typedef float type; };
template <>
struct VecT<2> { typedef float2 type; };
template <>
struct VecT<4> { typedef float4 type; };

__device__ __forceinline__ float vec_get(float v, int) { return v; }
__device__ __forceinline__ float vec_get(float2 v, int i) { return i == 0 ? v.x : v.y; }
__device__ __forceinline__ float vec_get(float4 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

struct RowPos {
  int ybase, xbase, rowbase, SH, SW;
  bool ok;
};

// m -> (segment, image, y, x) -> gather bases.  n_seg <= PP_MAX_SEG, uniform loop + selects.
__device__ __forceinline__ RowPos decode_row(const IgemmParams& p, int m) {
  RowPos r;
  r.ok = m < p.M;
  int rb = p.seg[0].row_begin, sb = p.seg[0].src_row_begin, OH = p.seg[0].OH, OW = p.seg[0].OW,
      SH = p.seg[0].SH, SW = p.seg[0].SW;
  for (int s = 1; s < p.n_seg; ++s) {
    if (m >= p.seg[s].row_begin) {
      rb = p.seg[s].row_begin; sb = p.seg[s].src_row_begin; OH = p.seg[s].OH; OW = p.seg[s].OW;
      SH = p.seg[s].SH; SW = p.seg[s].SW;
    }
  }
  int local = r.ok ? m - rb : 0;
  int hw = OH * OW;
  int n = local / hw;
  int rem = local - n * hw;
  int y = rem / OW;
  int x = rem - y * OW;
  r.ybase = y * p.mul + p.off_y;
  r.xbase = x * p.mul + p.off_x;
  r.rowbase = sb + n * SH * SW;
  r.SH = SH;
  r.SW = SW;
  return r;
}

__device__ __forceinline__ bool tap_offset(const IgemmParams& p, const RowPos& r, int ty, int tx, long long* off) {
  int sy = r.ybase + ty * p.tsign;
  int sx = r.xbase + tx * p.tsign;
  bool ok = r.ok;
  if (p.div > 1) {
    ok = ok && (sy % p.div == 0) && (sx % p.div == 0);
    sy /= p.div;
    sx /= p.div;
  }
  ok = ok && ((unsigned)sy < (unsigned)r.SH) && ((unsigned)sx < (unsigned)r.SW);
  *off = ok ? (long long)(r.rowbase + sy * r.SW + sx) * p.ld_src : 0;
  return ok;
}


// ---- host side ----
static int fill_segs(pp_ctx* ctx, const pp_conv_desc* d, bool enumerate_out, SegGeo* seg, int* M_out, long long* src_rows_out = nullptr) {
  // enumerate_out: rows enumerate the OUTPUT space and gather from the input (fwd, wgrad);
  // otherwise rows enumerate the INPUT space and gather from the output-space tensor (bwd-data).
  const pp_rowspace* e = enumerate_out ? &d->out : &d->in;
  const pp_rowspace* g = enumerate_out ? &d->in : &d->out;
  long long rb = 0, sb = 0;
  for (int s = 0; s < e->n_seg; ++s) {
    seg[s].row_begin = (int)rb;
    seg[s].src_row_begin = (int)sb;
    seg[s].OH = e->h[s]; seg[s].OW = e->w[s];
    seg[s].SH = g->h[s]; seg[s].SW = g->w[s];
    rb += (long long)e->n_img * e->h[s] * e->w[s];
    sb += (long long)g->n_img * g->h[s] * g->w[s];
  }
  *M_out = (int)rb;
  if (src_rows_out) *src_rows_out = sb;
  (void)ctx;
  return 0;
}

static int check_desc(pp_ctx* ctx, const pp_conv_desc* d, const char* who) {
  PP_CHECK_ARG(ctx, d != nullptr, PP_ERR_ARG, "%s: null descriptor", who);
  PP_CHECK_ARG(ctx, pp_rowspace_ok(&d->in) && pp_rowspace_ok(&d->out), PP_ERR_SHAPE, "%s: bad row space", who);
  PP_CHECK_ARG(ctx, d->in.n_seg == d->out.n_seg && d->in.n_img == d->out.n_img, PP_ERR_SHAPE,
               "%s: in/out row spaces disagree", who);
  PP_CHECK_ARG(ctx, d->kh > 0 && d->kw > 0 && d->kh <= 7 && d->kw <= 7 && d->stride >= 1 && d->stride <= 2, PP_ERR_SHAPE,
               "%s: unsupported kernel %dx%d stride %d", who, d->kh, d->kw, d->stride);
  PP_CHECK_ARG(ctx, d->cin > 0 && d->cout > 0 && (d->cin % 16 == 0 || d->cin == 4), PP_ERR_SHAPE,
               "%s: cin %d must be a multiple of 16 (or 4 for the packed stem)", who, d->cin);
  PP_CHECK_ARG(ctx, d->ld_w % 16 == 0 && d->ld_w >= d->cout, PP_ERR_SHAPE, "%s: ld_w %d (cout %d) must be a multiple of 16", who,
               d->ld_w, d->cout);
  PP_CHECK_ARG(ctx, d->ld_x % 4 == 0 && d->ld_x >= d->cin, PP_ERR_SHAPE, "%s: ld_x %d < cin %d or not a multiple of 4", who, d->ld_x, d->cin);
  PP_CHECK_ARG(ctx, d->ld_y % 4 == 0 && d->ld_y >= ((d->cout + 3) & ~3), PP_ERR_SHAPE,
               "%s: ld_y %d must be a multiple of 4 and >= cout %d rounded up to 4", who, d->ld_y, d->cout);
  PP_CHECK_ARG(ctx, d->pad_t >= 0 && d->pad_l >= 0 && d->pad_t < d->kh && d->pad_l < d->kw, PP_ERR_SHAPE, "%s: bad padding", who);
  for (int s = 0; s < d->in.n_seg; ++s) {
    // every output cell must lie inside the (bottom/right zero-extended) input: OH <= ceil((H + pad_t)/stride)
    PP_CHECK_ARG(ctx, (d->out.h[s] - 1) * d->stride - d->pad_t < d->in.h[s] && (d->out.w[s] - 1) * d->stride - d->pad_l < d->in.w[s],
                 PP_ERR_SHAPE, "%s: output %dx%d does not fit input %dx%d", who, d->out.h[s], d->out.w[s], d->in.h[s], d->in.w[s]);
  }
  if (d->in.n_seg > 1) PP_CHECK_ARG(ctx, d->stride == 1, PP_ERR_SHAPE, "%s: multi-level row spaces need stride 1", who);
  return PP_OK;
}


// ---- the descriptor's part of the launch parameters, per pass (the entry points add pointers and epilogue fields) ----
static void igemm_geometry_fwd(pp_ctx* ctx, const pp_conv_desc* d, IgemmParams& p) {
  p.ld_src = d->ld_x; p.ld_w = d->ld_w; p.ld_out = d->ld_y;
  p.n_seg = d->in.n_seg;
  fill_segs(ctx, d, true, p.seg, &p.M, &p.src_rows);
  p.Cred = d->cin; p.Nout = d->cout; p.w_tap_rows = d->cin;
  p.kh = d->kh; p.kw = d->kw;
  p.mul = d->stride; p.tsign = 1; p.off_y = -d->pad_t; p.off_x = -d->pad_l; p.div = 1;
  p.w_ty0 = 0; p.w_tx0 = 0; p.w_tstep = 1; p.w_kw = d->kw; p.w_taps = d->kh * d->kw;
}
static void igemm_geometry_bwd_data(pp_ctx* ctx, const pp_conv_desc* d, IgemmParams& p) {
  p.ld_src = d->ld_y; p.ld_w = d->ld_w; p.ld_out = d->ld_x;
  p.n_seg = d->in.n_seg;
  fill_segs(ctx, d, false, p.seg, &p.M, &p.src_rows);
  p.Cred = (d->cout + 31) / 32 * 32; p.Nout = d->cin; p.w_tap_rows = d->cin;
  p.kh = d->kh; p.kw = d->kw;
  p.mul = 1; p.tsign = -1; p.off_y = d->pad_t; p.off_x = d->pad_l; p.div = d->stride;
  p.w_ty0 = 0; p.w_tx0 = 0; p.w_tstep = 1; p.w_kw = d->kw; p.w_taps = d->kh * d->kw;
}
static void wgrad_geometry(pp_ctx* ctx, const pp_conv_desc* d, Wgrad3Params& p) {
  p.ld_src = d->ld_x; p.ld_dy = d->ld_y; p.ld_w = d->ld_w;
  p.n_seg = d->in.n_seg;
  fill_segs(ctx, d, true, p.seg, &p.M, &p.src_rows);
  p.Cin = d->cin; p.Cout = d->cout;
  p.kh = d->kh; p.kw = d->kw; p.stride = d->stride; p.pad_t = d->pad_t; p.pad_l = d->pad_l;
}

// every level: enumerated grid == gathered grid (a "same" convolution on an unchanged grid)
static bool segs_same_grid(const SegGeo* seg, int n_seg) {
  bool same = true;
  for (int i = 0; i < n_seg && same; ++i) same = seg[i].OH == seg[i].SH && seg[i].OW == seg[i].SW && seg[i].row_begin == seg[i].src_row_begin;
  return same;
}

// ---- the facts of a launch (conv_plan.h), from its parameters, operand forms and resources ----
static PpIgemmFacts igemm_facts(const IgemmParams& p, int w_rows, int w_ld8, bool planes_in, bool f32_in, bool planes_out, bool f32_out,
                                bool capture, bool flags, int n_cu, bool ws, long long ws_bytes) {
  PpIgemmFacts f = {};
  f.M = p.M; f.Nout = p.Nout; f.Cred = p.Cred; f.kh = p.kh; f.kw = p.kw; f.ld_out = p.ld_out; f.ld_src = p.ld_src;
  f.w_rows = w_rows; f.w_ld8 = w_ld8; f.w_taps = p.w_taps; f.div = p.div; f.mul = p.mul; f.sc_on = p.sc_on; f.w_tstep = p.w_tstep; f.w_tx0 = p.w_tx0;
  f.src_rows = p.src_rows;
  for (int i = 0; i < p.n_seg; ++i) f.max_sw = p.seg[i].SW > f.max_sw ? p.seg[i].SW : f.max_sw;
  f.same_grid = segs_same_grid(p.seg, p.n_seg);
  f.planes_in = planes_in; f.f32_in = f32_in; f.planes_out = planes_out; f.f32_out = f32_out; f.capture = capture; f.flags = flags;
  f.n_cu = pp_cus(n_cu); f.ws = ws; f.ws_bytes = ws_bytes;
  return f;
}

// fills p.pos_begin / p.Mp (wgrad3r's position space: every image row followed by one pad) on the way
static PpWgradFacts wgrad_facts(Wgrad3Params& p, bool planes, bool list, bool lazy_in, int fmt, int n_cu, bool ws, long long ws_bytes,
                                bool dw_aligned, bool dbias_aligned) {
  PpWgradFacts f = {};
  f.M = p.M; f.Cin = p.Cin; f.Cout = p.Cout; f.kh = p.kh; f.kw = p.kw; f.stride = p.stride; f.pad_t = p.pad_t; f.pad_l = p.pad_l;
  f.ld_src = p.ld_src; f.ld_dy = p.ld_dy; f.ld_w = p.ld_w; f.src_rows = p.src_rows;
  f.min_ow = f.min_hw = 1 << 30;
  f.list_levels_aligned = true;
  long long pos = 0;
  for (int i = 0; i < p.n_seg; ++i) {
    f.min_ow = p.seg[i].OW < f.min_ow ? p.seg[i].OW : f.min_ow;
    f.min_hw = p.seg[i].OH * p.seg[i].OW < f.min_hw ? p.seg[i].OH * p.seg[i].OW : f.min_hw;
    if (i + 1 < p.n_seg && p.seg[i + 1].row_begin % 32 != 0) f.list_levels_aligned = false;
    const long long rows = (i + 1 < p.n_seg ? p.seg[i + 1].row_begin : p.M) - p.seg[i].row_begin;
    p.pos_begin[i] = (int)pos;
    pos += rows / p.seg[i].OW * (p.seg[i].OW + 1);
  }
  p.Mp = (int)pos;
  f.Mp = pos;
  f.same_grid = segs_same_grid(p.seg, p.n_seg);
  f.planes = planes; f.list = list; f.lazy_in = lazy_in; f.fmt = fmt;
  f.n_cu = pp_cus(n_cu); f.ws = ws; f.ws_bytes = ws_bytes; f.dw_aligned = dw_aligned; f.dbias_aligned = dbias_aligned;
  return f;
}

// Stride-2 bwd-data as four stride-1 launches, one per parity class (cy, cx) of the input grid: input cell
// (2y'+cy, 2x'+cx) only receives the taps ty = ty0 + 2i with ty0 = (cy + pad_t) & 1 (x alike), from output cell
// y' + (cy + pad_t - ty0)/2 - i.  The single-launch form spends 3/4 of its MFMAs on taps that the divisibility
// mask zeroes; here every MFMA is useful and classes without taps (1x1 kernels) only run the epilogue.
// p: the whole data gradient; false when a class does not meet igemm3f's conditions (the caller keeps the one launch).
// the fields of a launch that differ between the parity classes (host: one launch per class; device: the merged launch, where
// every workgroup takes the geometry of its own class)
__host__ __device__ __forceinline__ void igemm_set_class(IgemmParams& r, const PpS2Class& c) {
  r.kh = c.kh; r.kw = c.kw;
  r.off_y = c.off_y; r.off_x = c.off_x;
  r.w_ty0 = c.w_ty0; r.w_tx0 = c.w_tx0;
  r.seg[0].OH = c.OH; r.seg[0].OW = c.OW;
  r.M = c.M;
  r.sc_cy = c.cy; r.sc_cx = c.cx;
}
static bool igemm_parity_classes(const pp_conv_desc* d, const IgemmParams& p, bool all_planes, IgemmParams cls[4]) {
  const int H = d->in.h[0], W = d->in.w[0];
  PpS2Class geo[4];
  pp_s2_classes(d->in.n_img, H, W, d->kh, d->kw, d->pad_t, d->pad_l, geo);
  for (int c = 0; c < 4; ++c) {
    IgemmParams& r = cls[c];
    r = p;
    r.div = 1;
    r.w_tstep = 2; r.w_kw = d->kw;
    igemm_set_class(r, geo[c]);  // (kh == 0: no taps -- class_fill_kernel, or the epilogue alone in the merged launch)
    r.sc_on = 1; r.sc_H = H; r.sc_W = W;
    if (r.M > 0 && r.kh > 0 &&
        !(pp_igemm_fast_ok(igemm_facts(r, d->cin, r.Cred / 8, all_planes, !all_planes, all_planes, !all_planes, false, false, 0, false, 0)) && r.M < (1 << 24)))
      return false;
  }
  return true;
}

// ---- which launches a call is made of: one function each for the entry points of conv3.hip and for pp_conv_plan_text ----
// pp_conv_opts.out_flags of the forward pass (only the flagged 32-row output blocks): plane-stored input, one output form, 3x3
// stride 1 pad 1 on an unchanged grid, no residual
static bool fwd_listed_ok(const pp_conv_desc* d, const PpIgemmFacts& f, bool residual) {
  return f.planes_in && f.f32_out != f.planes_out && !f.capture && !residual && d->stride == 1 && d->kh == 3 && d->kw == 3 && d->pad_t == 1 &&
         d->pad_l == 1 && pp_igemm_fast_ok(f) && f.same_grid;
}

struct DgradRoute {
  bool listed;    // one launch over the listed blocks, tile 64 listed_tm x 128
  int listed_tm;
  bool classes;   // stride 2: the parity classes cls[] (those without taps only fill)
  IgemmParams cls[4];
};
// p, f: the whole data gradient.  A lazy dy needs r->listed.
static void dgrad_route(const pp_conv_desc* d, const IgemmParams& p, const PpIgemmFacts& f, bool skip_scratch, DgradRoute* r) {
  const bool all_f32 = f.f32_in && f.f32_out && !f.planes_in && !f.planes_out, all_planes = f.planes_in && f.planes_out && !f.f32_out;
  const PpDgradRouteFacts rf = {d->stride, d->kh, d->kw, d->pad_t, d->pad_l, d->in.n_seg, all_f32, all_planes, f.capture, p.bias != nullptr,
                                f.flags, skip_scratch, pp_igemm_fast_ok(f), f.same_grid};
  r->listed = pp_dgrad_listed_ok(rf);
  r->listed_tm = pp_conv_switches().sparse_dgrad == 22 ? 2 : 1;
  r->classes = pp_dgrad_classes_ok(rf) && igemm_parity_classes(d, p, all_planes, r->cls);
}
// The merged stride-2 data gradient (pp_conv2d_nhwc_bwd_data_s2_bf16x3, PP_PLAN_BWD_DATA_S2): the same classes in ONE launch.
// Every class runs on the tile the planner gives the class with the most taps (f, pl: its facts and plan -- what the per-class
// route launches it with); g: the concatenated grid.  p, f_all: the whole data gradient.  ok = false: the call is refused.
struct DgradS2Route {
  bool ok;
  IgemmParams cls[4];
  PpIgemmFacts f;
  PpIgemmPlan pl;
  PpS2Merged g;
};
static void dgrad_s2_route(const pp_conv_desc* d, const IgemmParams& p, const PpIgemmFacts& f_all, DgradS2Route* r) {
  const bool all_f32 = f_all.f32_in && f_all.f32_out && !f_all.planes_in && !f_all.planes_out,
             all_planes = f_all.planes_in && f_all.planes_out && !f_all.f32_out;
  const PpDgradRouteFacts rf = {d->stride, d->kh, d->kw, d->pad_t, d->pad_l, d->in.n_seg, all_f32, all_planes, f_all.capture, p.bias != nullptr,
                                f_all.flags, false, pp_igemm_fast_ok(f_all), f_all.same_grid};
  r->ok = pp_dgrad_s2_ok(rf) && !f_all.capture && !f_all.flags && igemm_parity_classes(d, p, all_planes, r->cls);
  if (!r->ok) return;
  PpS2Class geo[4];
  pp_s2_classes(d->in.n_img, d->in.h[0], d->in.w[0], d->kh, d->kw, d->pad_t, d->pad_l, geo);
  const PpS2Merged order = pp_s2_merge(geo, 64, 64, p.Nout);  // (any tile: only the order is read)
  const IgemmParams& heavy = r->cls[2 * order.c[0].cy + order.c[0].cx];
  r->f = igemm_facts(heavy, f_all.w_rows, f_all.w_ld8, all_planes, !all_planes, all_planes, !all_planes, false, false, f_all.n_cu, f_all.ws,
                     f_all.ws_bytes);
  r->pl = pp_plan_igemm(r->f);
  r->g = pp_s2_merge(geo, 64 * r->pl.tm, 64 * r->pl.tn, p.Nout);
  r->ok = r->pl.family == PP_IGEMM3F_CLASS && r->pl.splits == 1 && order.c[0].kh > 0;
}
// the launches in order: gemm(params, is_class, listed) for every GEMM, fill(params) for a class without taps
template <class Gemm, class Fill>
static void dgrad_launches(DgradRoute& r, IgemmParams& p, Gemm gemm, Fill fill) {
  if (!r.classes) {
    gemm(p, false, r.listed);
    return;
  }
  for (int c = 0; c < 4; ++c) {
    if (r.cls[c].M <= 0) continue;
    if (r.cls[c].kh > 0) gemm(r.cls[c], true, false);
    else fill(r.cls[c]);
  }
}
