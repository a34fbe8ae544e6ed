// Implicit-GEMM convolution with float32-class accuracy at TWO matrix-core units per product ("f16c8"; rounds 1-2 used three
// bf16 MFMAs per product, "bf16x3": the entry points keep that name):
//   x = x_hi + x_lo:  x_hi = f16(x) (11-bit significand, |x| saturates at 65504),  x_lo8 = e5m2((x - x_hi) * 2^12);  same for w
//   x*w ~= x_hi*w_hi                                 v_mfma_f32_32x32x16_f16
//        + (x_hi8*w_lo8 + x_lo8*w_hi8) * 2^-12       v_mfma_scale_f32_32x32x64_f8f6f4 on e5m2 operands (x_hi8 = e5m2(x_hi)), E8M0
//                                                    scale 2^-12: twice the cycles of the f16 form for four times the K
// so a 32-deep k-step of a 32x32 block is 2 f16 MFMAs + 1 scaled MFMA = 4 issue units instead of the 6 of bf16x3, with the
// loads, LDS images and staging of the bf16x3 kernels unchanged.  Measured per launch against bf16x3 on the same box
// (profiles/r03_p16_*): forward / bwd-data 1.16-1.19x, weight gradient 1.15x; error against float64 2.1e-5 (bf16x3: 4.5e-6;
// per-kernel bar 1e-4, tests/test_gpu_conv.py).  Same gather, row spaces, fusions and LDS-staged epilogue as conv.hip.
//
// Plane format ("P16", same packed geometry as before): hi plane = IEEE halves; lo plane = per element TWO e5m2 bytes,
// [e5m2(x_hi) | e5m2((x - x_hi) * 2^12) << 8] for gathered operands (activations, gradients) and the two bytes swapped for
// weights -- so that the two lo-plane fragments a lane reads per 32-deep step (2 x 16 bytes) ARE the 32-byte operands of the
// scaled MFMA: slot pairs are (x_hi8, w_lo8) and (x_lo8, w_hi8), no byte shuffling in the loop.  value = hi + lo8 * 2^-12
// (within 2^-15 of x).  Gradients travel scaled by a power of two (pp_grad_scale: halves stop at 6e-8) and the weight
// gradient divides it out.
//
// Fragment maps (cdna_hip_programming.md section 3): lane l (r = l & 31, h = l >> 5) holds A[row r][k = 8h + j] and
// B[k = 8h + j][col r], j = 0..7 -> one 16-byte LDS read per operand and plane.  LDS image per operand plane:
// [4 k-octets][rows][8 x 16 bit], rows of octet o rotated by 2*o so that both the 16-byte stores of the staging
// threads (4 threads per row) and the 512-byte fragment reads are bank-conflict free.
#include "conv3_unit.h"
#include "conv3.h"
#include "conv4.h"

// This unit holds the entry points of the forward, data-gradient, stem and weight-gradient passes: argument checks, the launch
// parameters, facts -> plan (conv_plan.h) -> one call into a launcher of conv3.h / conv4.h.  The kernels are in conv3_igemm.hip,
// conv3_igemm4x.hip, conv3_wgrad.hip and conv4.hip; the small kernels around them, with their own entry points, in conv3_aux.hip.
namespace {

static PpIgemmFacts igemm3_facts(const pp_ctx* ctx, const IgemmParams& p, const Igemm3Args& a) {
  return igemm_facts(p, a.w_rows, a.w_ld8, a.ahi != nullptr, p.src != nullptr, a.ohi != nullptr, p.out != nullptr, a.chi != nullptr,
                     a.flags != nullptr, ctx->n_cu, ctx->ws != nullptr, (long long)ctx->ws_bytes);
}

// facts -> plan -> launch of one forward / data-gradient GEMM
static void dispatch3(pp_ctx* ctx, IgemmParams& p, const Igemm3Args& a) {
  const PpIgemmFacts f = igemm3_facts(ctx, p, a);
  const PpIgemmPlan pl = pp_plan_igemm(f);
  pp_plan_debug(f, pl);
  PP_API(pp3_launch_igemm)(ctx->stream, p, a, pl);
}

// the merged stride-2 data gradient: the route planned it (p: the shared fields of its classes)
static void dispatch3m(pp_ctx* ctx, IgemmParams& p, const Igemm3Args& a, const DgradS2Route& r) {
  pp_plan_debug(r.f, r.pl, r.g);
  PP_API(pp3_launch_igemm_s2)(ctx->stream, p, a, r);
}

// the launch over the listed 32-row blocks (tm: 2 = 128 x 128 tiles, 1 = 64 x 128)
static void dispatch3_rowlist(pp_ctx* ctx, IgemmParams& p, const Igemm3Args& a, int tm, const unsigned char* dy_flags, unsigned char* out_flags,
                              int* out_list, bool fill) {
  PpIgemmFacts f = igemm3_facts(ctx, p, a);
  f.listed = true;
  f.listed_tm = tm;
  const PpIgemmPlan pl = pp_plan_igemm(f);
  PP_API(pp3_launch_igemm_rowlist)(ctx->stream, p, a, pl, dy_flags, out_flags, out_list, fill);
}

// both data-gradient entry points (who): merged = pp_conv2d_nhwc_bwd_data_s2_bf16x3, which takes the epilogue planes as its only
// options, launches igemm3m where its route applies and refuses every other call
static int bwd_data_impl(pp_ctx* ctx, const char* who, bool merged, const pp_conv_desc* d, const float* dy, const void* dy_hi, const void* dy_lo,
                         const void* w_hi, const void* w_lo, const float* addend, int ld_add, const float* relu_src, int ld_rs, float* dx,
                         void* dx_hi, void* dx_lo, const pp_conv_opts* opts) {
  PP_REQUIRE_CTX(ctx);
  int rc = pp_conv_opts_take(ctx, opts,
                             merged ? (PP_OPT_ADD | PP_OPT_MASK)
                                    : (PP_OPT_CAPTURE | PP_OPT_ADD | PP_OPT_MASK | PP_OPT_SKIP | PP_OPT_LAZY_OUT | PP_OPT_LAZY_IN),
                             who);
  if (rc) return rc;
  void *const chi = opts->capture_hi, *const clo = opts->capture_lo;
  unsigned char* const skip_flags = opts->skip_flags;
  const bool skip_scratch_ok = skip_flags != nullptr && opts->skip_list != nullptr;
  const void *const ep_ah = opts->add_hi, *const ep_al = opts->add_lo, *const ep_mh = opts->mask_hi;
  rc = check_desc(ctx, d, who);
  PP_CHECK_ARG(ctx, !(ep_ah && addend) && !(ep_mh && relu_src), PP_ERR_ARG,
               "%s: addend / relu_src given both as f32 and as planes", who);
  PP_CHECK_ARG(ctx, (!ep_ah || (ld_add >= d->cin && ld_add % 4 == 0)) && (!ep_mh || (ld_rs >= d->cin && ld_rs % 4 == 0)), PP_ERR_SHAPE,
               "%s: addend / relu_src planes", who);
  if (rc) return rc;
  PP_CHECK_ARG(ctx, !chi || (dy && !dy_hi && pp_is_packed(chi, clo)), PP_ERR_ARG, "%s: split capture needs the f32 operand", who);
  PP_CHECK_ARG(ctx, (dy || (dy_hi && dy_lo)) && w_hi && w_lo && (dx || (dx_hi && dx_lo)), PP_ERR_ARG, "%s: null tensor", who);
  PP_CHECK_ARG(ctx, (dy_hi == nullptr) == (dy_lo == nullptr) && d->ld_y % 8 == 0, PP_ERR_ARG, "%s: planes / ld_y", who);
  PP_CHECK_ARG(ctx, pp_is_packed(dy_hi, dy_lo) && pp_is_packed(dx_hi, dx_lo), PP_ERR_ALIGN,
               "%s: planes must be packed (lo = hi + 16 bytes, 16-byte aligned)", who);
  PP_CHECK_ARG(ctx, (!dx_hi || (d->cin % 8 == 0 && d->ld_x % 8 == 0)) && (!ep_ah || ld_add % 8 == 0) && (!ep_mh || ld_rs % 8 == 0), PP_ERR_SHAPE,
               "%s: planes need channel counts and leading dimensions %% 8 == 0", who);
  const int cred = (d->cout + 31) / 32 * 32;
  PP_CHECK_ARG(ctx, d->cin % 16 == 0 && d->ld_y >= cred && d->ld_y % 4 == 0, PP_ERR_SHAPE,
               "%s: dy needs ld_y >= %d (cout rounded up to 32, zero padded)", who, cred);
  PP_CHECK_ARG(ctx, (!dy || pp_is_aligned16(dy)) && pp_is_aligned16(w_hi) && pp_is_aligned16(w_lo) && (!dx || pp_is_aligned16(dx)), PP_ERR_ALIGN,
               "%s: tensors must be 16-byte aligned", who);
  PP_CHECK_ARG(ctx, (!addend || (ld_add >= d->cin && ld_add % 4 == 0 && pp_is_aligned16(addend))) &&
                        (!relu_src || (ld_rs >= d->cin && ld_rs % 4 == 0 && pp_is_aligned16(relu_src))),
               PP_ERR_SHAPE, "%s: addend / relu_src", who);
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  p.src = dy; p.out = dx; p.bias = nullptr; p.addend = addend; p.mask_src = relu_src;
  p.add_hi = ep_ah; p.add_lo = ep_al; p.mask_hi = ep_mh;
  igemm_geometry_bwd_data(ctx, d, p);
  p.ld_add = ld_add; p.ld_mask = ld_rs;
  p.relu = 0;
  PP_CHECK_ARG(ctx, (dx_hi == nullptr) == (dx_lo == nullptr) && (!dx_hi || (d->ld_x % 4 == 0 && pp_is_aligned16(dx_hi) && pp_is_aligned16(dx_lo))),
               PP_ERR_ARG, "%s: output planes", who);
  const Igemm3Args a = {dy_hi, dy_lo, w_hi, w_lo, d->cin, cred / 8, dx_hi, dx_lo, chi, clo, skip_flags, ctx->ws};
  if (merged) {
    DgradS2Route s2;
    dgrad_s2_route(d, p, igemm3_facts(ctx, p, a), &s2);
    PP_CHECK_ARG(ctx, s2.ok, PP_ERR_ARG,
                 "%s: needs stride 2, one level, operands all float32 or all planes, and classes the branch-free loop can run "
                 "(pp_conv2d_nhwc_bwd_data_bf16x3 takes every other call)", who);
    IgemmParams q = s2.cls[0];  // (the fields the classes share; the kernel takes the rest from the class of each workgroup)
    dispatch3m(ctx, q, a, s2);
    PP_CHECK_LAUNCH(ctx, who);
    return PP_OK;
  }
  DgradRoute route;
  dgrad_route(d, p, igemm3_facts(ctx, p, a), skip_scratch_ok, &route);
  // Contract of the hint's scratch (pp_row_block_list_planes_within relies on it): after this call the second n_blocks bytes
  // of the flags buffer flag every 32-row block of dx that may hold a non-zero -- the dilated list when the listed launch
  // runs, everything otherwise.
  PP_CHECK_ARG(ctx, !opts->lazy_in || route.listed, PP_ERR_ARG,
               "%s: dy was declared lazy (unwritten outside its flagged blocks) but the listed-block launch "
               "does not apply to this call", who);
  const int nb = (p.M + 31) / 32;
  if (skip_scratch_ok && !route.listed) PP_HIP(ctx, hipMemsetAsync(skip_flags + nb, 1, (size_t)nb, ctx->stream));
  const Igemm3Args ac = {dy_hi, dy_lo, w_hi, w_lo, d->cin, cred / 8, dx_hi, dx_lo, nullptr, nullptr, nullptr, ctx->ws};
  if (route.classes && chi) PP_API(pp3_split_capture_pass)(ctx->stream, p, chi, clo);
  dgrad_launches(
      route, p,
      [&](IgemmParams& q, bool is_class, bool listed) {
        if (listed) dispatch3_rowlist(ctx, q, a, route.listed_tm, skip_flags, skip_flags + nb, opts->skip_list + nb + 1, !opts->lazy_out);
        else dispatch3(ctx, q, is_class ? ac : a);
      },
      [&](IgemmParams& q) {
        PP_API(pp3_launch_class_fill)(ctx->stream, q, pp_finish_blocks(q.M, q.Nout, pp_cus(ctx->n_cu)), addend, relu_src, dx, dx_hi, dx_lo);
      });
  PP_CHECK_LAUNCH(ctx, who);
  return PP_OK;
}

}  // namespace

extern "C" {

int PP_API(pp_conv2d_nhwc_fwd_bf16x3)(pp_ctx* ctx, const pp_conv_desc* d, const float* x, const void* x_hi, const void* x_lo,
                                         const void* w_hi, const void* w_lo, const float* bias, const float* residual, int ld_res,
                                         int relu, float* y, void* y_hi, void* y_lo, const pp_conv_opts* opts) {
  PP_REQUIRE_CTX(ctx);
  int rc = pp_conv_opts_take(ctx, opts, PP_OPT_CAPTURE | PP_OPT_ADD | PP_OPT_OUT, "pp_conv2d_nhwc_fwd_bf16x3");
  if (rc) return rc;
  void *const chi = opts->capture_hi, *const clo = opts->capture_lo;
  const void *const ep_ah = opts->add_hi, *const ep_al = opts->add_lo;  // the residual as planes
  rc = check_desc(ctx, d, "pp_conv2d_nhwc_fwd_bf16x3");
  PP_CHECK_ARG(ctx, !(ep_ah && residual), PP_ERR_ARG, "pp_conv2d_nhwc_fwd_bf16x3: residual given both as f32 and as planes");
  PP_CHECK_ARG(ctx, !ep_ah || (ld_res % 4 == 0 && ld_res >= ((d->cout + 3) & ~3)), PP_ERR_SHAPE, "pp_conv2d_nhwc_fwd_bf16x3: residual planes");
  if (rc) return rc;
  PP_CHECK_ARG(ctx, !chi || (x && !x_hi && pp_is_packed(chi, clo)), PP_ERR_ARG, "pp_conv2d_nhwc_fwd_bf16x3: split capture needs the f32 operand");
  PP_CHECK_ARG(ctx, (x || (x_hi && x_lo)) && w_hi && w_lo && (y || (y_hi && y_lo)), PP_ERR_ARG, "pp_conv2d_nhwc_fwd_bf16x3: null tensor");
  PP_CHECK_ARG(ctx, (x_hi == nullptr) == (x_lo == nullptr), PP_ERR_ARG, "pp_conv2d_nhwc_fwd_bf16x3: x_hi and x_lo go together");
  PP_CHECK_ARG(ctx, d->cin % 32 == 0 && d->ld_x % 8 == 0, PP_ERR_SHAPE, "pp_conv2d_nhwc_fwd_bf16x3: cin %d must be a multiple of 32, ld_x of 8", d->cin);
  PP_CHECK_ARG(ctx, pp_is_packed(x_hi, x_lo) && pp_is_packed(y_hi, y_lo), PP_ERR_ALIGN,
               "pp_conv2d_nhwc_fwd_bf16x3: planes must be packed (lo = hi + 16 bytes, 16-byte aligned)");
  PP_CHECK_ARG(ctx, !y_hi || (d->cout % 8 == 0 && d->ld_y % 8 == 0), PP_ERR_SHAPE, "pp_conv2d_nhwc_fwd_bf16x3: output planes need cout, ld_y %% 8 == 0");
  PP_CHECK_ARG(ctx, !ep_ah || (ld_res % 8 == 0 && d->cout % 8 == 0), PP_ERR_SHAPE, "pp_conv2d_nhwc_fwd_bf16x3: residual planes need cout, ld_res %% 8 == 0");
  PP_CHECK_ARG(ctx, (!x || pp_is_aligned16(x)) && pp_is_aligned16(w_hi) && pp_is_aligned16(w_lo) && (!y || pp_is_aligned16(y)), PP_ERR_ALIGN,
               "pp_conv2d_nhwc_fwd_bf16x3: tensors must be 16-byte aligned");
  PP_CHECK_ARG(ctx, !residual || (ld_res % 4 == 0 && ld_res >= ((d->cout + 3) & ~3) && pp_is_aligned16(residual)), PP_ERR_SHAPE,
               "pp_conv2d_nhwc_fwd_bf16x3: residual");
  PP_CHECK_ARG(ctx, !bias || pp_is_aligned16(bias), PP_ERR_ALIGN, "pp_conv2d_nhwc_fwd_bf16x3: bias alignment");
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  p.src = x; p.out = y; p.bias = bias; p.addend = residual; p.mask_src = nullptr;
  p.add_hi = ep_ah; p.add_lo = ep_al;
  igemm_geometry_fwd(ctx, d, p);
  p.ld_add = ld_res; p.ld_mask = 0;
  p.relu = relu;
  PP_CHECK_ARG(ctx, (y_hi == nullptr) == (y_lo == nullptr) && (!y_hi || (d->ld_y % 4 == 0 && pp_is_aligned16(y_hi) && pp_is_aligned16(y_lo))),
               PP_ERR_ARG, "pp_conv2d_nhwc_fwd_bf16x3: output planes");
  const Igemm3Args a = {x_hi, x_lo, w_hi, w_lo, d->cout, d->cin / 8, y_hi, y_lo, chi, clo, nullptr, ctx->ws};
  if (opts->out_flags) {
    // only the flagged 32-row output blocks (the listed-block launch of the sparse data gradient, without dilation and fill):
    // plane-stored input, 3x3 stride 1 pad 1 on an unchanged grid, no residual
    const bool ok = fwd_listed_ok(d, igemm3_facts(ctx, p, a), residual != nullptr || ep_ah != nullptr);
    PP_CHECK_ARG(ctx, ok, PP_ERR_SHAPE, "pp_conv2d_nhwc_fwd_bf16x3: out_flags needs a 3x3 stride-1 'same' conv on plane-stored input");
    dispatch3_rowlist(ctx, p, a, 2, nullptr, const_cast<unsigned char*>(opts->out_flags) /* (only read: no dilation without dy_flags) */,
                      opts->out_list, false);
    PP_CHECK_LAUNCH(ctx, "pp_conv2d_nhwc_fwd_bf16x3");
    return PP_OK;
  }
  dispatch3(ctx, p, a);
  PP_CHECK_LAUNCH(ctx, "pp_conv2d_nhwc_fwd_bf16x3");
  return PP_OK;
}

// out_flags[b] = 1 when a flagged block of in_flags lies within one pixel (2-D, 32-row granularity) of block b of the row
// space of a 3x3 stride-1 'same' conv d (the blocks of its input that the flagged blocks of its output read, and vice versa)
int PP_API(pp_row_block_dilate)(pp_ctx* ctx, const pp_conv_desc* d, const unsigned char* in_flags, unsigned char* out_flags) {
  PP_REQUIRE_CTX(ctx);
  int rc = check_desc(ctx, d, "pp_row_block_dilate");
  if (rc) return rc;
  PP_CHECK_ARG(ctx, in_flags && out_flags && in_flags != out_flags, PP_ERR_ARG, "pp_row_block_dilate: two distinct flag buffers");
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  p.n_seg = d->in.n_seg;
  fill_segs(ctx, d, true, p.seg, &p.M, &p.src_rows);
  const bool same = d->stride == 1 && d->kh == 3 && d->kw == 3 && segs_same_grid(p.seg, p.n_seg);
  PP_CHECK_ARG(ctx, same, PP_ERR_SHAPE, "pp_row_block_dilate: 3x3 stride-1 conv on an unchanged grid");
  const int nb = (p.M + 31) / 32;
  PP_API(pp3_launch_rl_dilate)(ctx->stream, p, in_flags, out_flags, nb);
  PP_CHECK_LAUNCH(ctx, "pp_row_block_dilate");
  return PP_OK;
}

// The 7x7 stride-2 RGB stem on the bf16 path.  Input: the packed 4-channel image inside a zero frame [n_img][Hp][Wp][4] with
// the image at (3, 3) (pp_pack_rgb_to_4_padded / pp_preprocess_caffe_u8_padded), Hp >= H + 6, Wp >= W + 8, Wp even.  Each
// kernel ROW (7 taps x 4 channels = 28 contiguous floats of the frame, padded to 32) is one tap of a 7x1 convolution over
// 32 "channels" that overlap between neighbouring pixels -- the gather of igemm3f needs nothing else: base offset of pixel
// (2 oy + ty, 2 ox), 32 consecutive floats.  Weights: planes [7][cout][32] with plane row ty, column tx * 4 + c (zeros for
// c == 3 and tx == 7), see Engine._build_stem.  224 of the executed 7 x 32 reduction steps are 147 algorithmic.
int PP_API(pp_stem7x7s2_fwd_bf16x3)(pp_ctx* ctx, int n_img, int H, int W, int Hp, int Wp, const float* x4p, const void* w_hi,
                                       const void* w_lo, int cout, const float* bias, int relu, float* y, int ld_y) {
  PP_REQUIRE_CTX(ctx);
  PP_CHECK_ARG(ctx, x4p && w_hi && w_lo && y && pp_is_aligned16(x4p) && pp_is_aligned16(y) && pp_is_aligned16(w_hi) && pp_is_aligned16(w_lo),
               PP_ERR_ARG, "pp_stem7x7s2_fwd_bf16x3: null / unaligned tensor");
  PP_CHECK_ARG(ctx, n_img > 0 && H > 0 && W > 0 && Hp >= H + 6 && Wp >= W + 8 && Wp % 2 == 0 && cout > 0 && ld_y % 4 == 0 && ld_y >= ((cout + 3) & ~3),
               PP_ERR_SHAPE, "pp_stem7x7s2_fwd_bf16x3: bad geometry");
  const int OH = (H + 6 - 7) / 2 + 1, OW = (W + 6 - 7) / 2 + 1;
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  p.src = x4p; p.out = y; p.bias = bias;
  p.ld_src = 4; p.ld_out = ld_y;
  p.relu = relu;
  p.n_seg = 1;
  p.seg[0].row_begin = 0; p.seg[0].src_row_begin = 0;
  p.seg[0].OH = OH; p.seg[0].OW = OW; p.seg[0].SH = Hp; p.seg[0].SW = Wp;
  p.M = n_img * OH * OW;
  p.src_rows = (long long)n_img * Hp * Wp;
  p.Cred = 32; p.Nout = cout; p.w_tap_rows = 32;
  p.kh = 7; p.kw = 1;
  p.mul = 2; p.tsign = 1; p.off_y = 0; p.off_x = 0; p.div = 1;
  p.w_ty0 = 0; p.w_tx0 = 0; p.w_tstep = 1; p.w_kw = 1; p.w_taps = 7;
  const Igemm3Args a = {nullptr, nullptr, w_hi, w_lo, cout, 4, nullptr, nullptr, nullptr, nullptr, nullptr, ctx->ws};
  PP_CHECK_ARG(ctx, pp_igemm_fast_ok(igemm3_facts(ctx, p, a)), PP_ERR_SHAPE, "pp_stem7x7s2_fwd_bf16x3: frame too large for 31-bit offsets");
  dispatch3(ctx, p, a);
  PP_CHECK_LAUNCH(ctx, "pp_stem7x7s2_fwd_bf16x3");
  return PP_OK;
}

int PP_API(pp_conv2d_nhwc_bwd_data_bf16x3)(pp_ctx* ctx, const pp_conv_desc* d, const float* dy, const void* dy_hi, const void* dy_lo,
                                              const void* w_hi, const void* w_lo, const float* addend, int ld_add,
                                              const float* relu_src, int ld_rs, float* dx, void* dx_hi, void* dx_lo,
                                              const pp_conv_opts* opts) {
  return bwd_data_impl(ctx, "pp_conv2d_nhwc_bwd_data_bf16x3", false, d, dy, dy_hi, dy_lo, w_hi, w_lo, addend, ld_add, relu_src, ld_rs, dx, dx_hi,
                       dx_lo, opts);
}
int PP_API(pp_conv2d_nhwc_bwd_data_s2_bf16x3)(pp_ctx* ctx, const pp_conv_desc* d, const float* dy, const void* dy_hi, const void* dy_lo,
                                                 const void* w_hi, const void* w_lo, const float* addend, int ld_add,
                                                 const float* relu_src, int ld_rs, float* dx, void* dx_hi, void* dx_lo,
                                                 const pp_conv_opts* opts) {
  return bwd_data_impl(ctx, "pp_conv2d_nhwc_bwd_data_s2_bf16x3", true, d, dy, dy_hi, dy_lo, w_hi, w_lo, addend, ld_add, relu_src, ld_rs, dx,
                       dx_hi, dx_lo, opts);
}

int PP_API(pp_conv2d_nhwc_bwd_weight_bf16x3)(pp_ctx* ctx, const pp_conv_desc* d, const float* x, const float* dy, const void* x_hi,
                                                const void* x_lo, const void* dy_hi, const void* dy_lo, float* dw, float* dbias,
                                                const pp_conv_opts* opts) {
  PP_REQUIRE_CTX(ctx);
  int rc = pp_conv_opts_take(ctx, opts, PP_OPT_SKIP | PP_OPT_LAZY_IN, "pp_conv2d_nhwc_bwd_weight_bf16x3");
  if (rc) return rc;
  const int* const skip_list = opts->skip_list;
  const bool lazy_in = opts->lazy_in != 0;  // dy may hold anything outside the listed blocks
  rc = check_desc(ctx, d, "pp_conv2d_nhwc_bwd_weight_bf16x3");
  if (rc) return rc;
  const bool planes = x_hi && x_lo && dy_hi && dy_lo;
  PP_CHECK_ARG(ctx, ((x && dy) || planes) && dw, PP_ERR_ARG, "pp_conv2d_nhwc_bwd_weight_bf16x3: null tensor");
  PP_CHECK_ARG(ctx, planes || !(x_hi || x_lo || dy_hi || dy_lo), PP_ERR_ARG, "pp_conv2d_nhwc_bwd_weight_bf16x3: all four planes or none");
  PP_CHECK_ARG(ctx, !planes || (d->ld_x % 8 == 0 && d->ld_y % 8 == 0), PP_ERR_SHAPE, "pp_conv2d_nhwc_bwd_weight_bf16x3: planes need ld % 8 == 0");
  PP_CHECK_ARG(ctx, !planes || (pp_is_packed(x_hi, x_lo) && pp_is_packed(dy_hi, dy_lo)), PP_ERR_ALIGN,
               "pp_conv2d_nhwc_bwd_weight_bf16x3: planes must be packed (lo = hi + 16 bytes, 16-byte aligned)");
  PP_CHECK_ARG(ctx, d->cin % 64 == 0, PP_ERR_SHAPE, "pp_conv2d_nhwc_bwd_weight_bf16x3: cin %d must be a multiple of 64", d->cin);
  PP_CHECK_ARG(ctx, d->ld_y % 4 == 0 && d->ld_x % 4 == 0, PP_ERR_SHAPE, "pp_conv2d_nhwc_bwd_weight_bf16x3: leading dims must be multiples of 4");
  PP_CHECK_ARG(ctx, (!x || pp_is_aligned16(x)) && (!dy || pp_is_aligned16(dy)), PP_ERR_ALIGN,
               "pp_conv2d_nhwc_bwd_weight_bf16x3: tensors must be 16-byte aligned");
  Wgrad3Params p;
  memset(&p, 0, sizeof(p));
  wgrad_geometry(ctx, d, p);
  p.inv_scale = (planes && ctx->grad_scale) ? ctx->grad_scale + 1 : nullptr;  // (f32 operands are never scaled)
  const PpWgradFacts f = wgrad_facts(p, planes, skip_list != nullptr, lazy_in, PP_FMT, ctx->n_cu, ctx->ws != nullptr, (long long)ctx->ws_bytes,
                                     pp_is_aligned16(dw), pp_is_aligned16(dbias));
  const PpWgradPlan pl = pp_plan_wgrad(f);
  PP_CHECK_ARG(ctx, !pl.refused, PP_ERR_ARG,
               "pp_conv2d_nhwc_bwd_weight_bf16x3: dy was declared lazy (unwritten outside its listed blocks) but the listed-block reduction "
               "does not apply to this call");
  pp_plan_debug(f, pl);
  p.k_tiles_per_tap = pl.k_tiles_per_tap; p.n_tiles_k = pl.n_tiles_k; p.n_tiles_n = pl.n_tiles_n;
  p.splits = pl.splits; p.rows_per_split = pl.rows_per_split; p.max_wraps = pl.max_wraps; p.sp_min_steps = pl.sp_min_steps;
  const void* const xhi = planes ? x_hi : nullptr;
  if (pl.family == PP_WGRAD3R || pl.family == PP_WGRAD3W)
    PP_API(pp4_launch_wgrad3r)(ctx->stream, p, pl.grid, pl.family == PP_WGRAD3W, x_hi, x_lo, dy_hi, dy_lo, dw, dbias, skip_list);
  else
    PP_API(pp3_launch_wgrad)(ctx->stream, p, pl, x, dy, xhi, x_lo, dy_hi, dy_lo, dw, dbias, skip_list, ctx->ws);
  PP_CHECK_LAUNCH(ctx, "pp_conv2d_nhwc_bwd_weight_bf16x3");
  return PP_OK;
}

}  // extern "C"
