// Forwards the plane-format-dependent entry points of the conv3 units (conv3.hip, conv3_aux.hip) to the build the context asks for
// (pp_ctx_set_planes_format: 0 = bf16 pairs / bf16x3 arithmetic, 1 = P16 / f16c8 arithmetic; csrc/planes_fmt.h).
#include "conv_common.h"

extern "C" int pp_row_block_list_fmt0(pp_ctx* ctx, const float* x, int rows, int ld, int cols, unsigned char* flags, int* list);
extern "C" int pp_row_block_list_fmt1(pp_ctx* ctx, const float* x, int rows, int ld, int cols, unsigned char* flags, int* list);
extern "C" int pp_row_block_list_planes_within_fmt0(pp_ctx* ctx, const void* x_hi, const void* x_lo, int rows, int ld, int cols, const unsigned char* within, unsigned char* flags, int* list);
extern "C" int pp_row_block_list_planes_within_fmt1(pp_ctx* ctx, const void* x_hi, const void* x_lo, int rows, int ld, int cols, const unsigned char* within, unsigned char* flags, int* list);
extern "C" int pp_row_block_list_planes_fmt0(pp_ctx* ctx, const void* x_hi, const void* x_lo, int rows, int ld, int cols, unsigned char* flags, int* list);
extern "C" int pp_row_block_list_planes_fmt1(pp_ctx* ctx, const void* x_hi, const void* x_lo, int rows, int ld, int cols, unsigned char* flags, int* list);
extern "C" int pp_split_planes_bf16x3_fmt0(pp_ctx* ctx, size_t n, const float* src, void* hi, void* lo);
extern "C" int pp_split_planes_bf16x3_fmt1(pp_ctx* ctx, size_t n, const float* src, void* hi, void* lo);
extern "C" int pp_split_planes_scaled_bf16x3_fmt0(pp_ctx* ctx, size_t n, const float* src, void* hi, void* lo, const float* scale_dev);
extern "C" int pp_split_planes_scaled_bf16x3_fmt1(pp_ctx* ctx, size_t n, const float* src, void* hi, void* lo, const float* scale_dev);
extern "C" int pp_grad_scale_from_counts_fmt0(pp_ctx* ctx, const int* counts_dev, int n_counts, float* scale2_dev);
extern "C" int pp_grad_scale_from_counts_adj_fmt0(pp_ctx* ctx, const int* counts_dev, int n_counts, float* scale2_dev, int log2_adjust);
extern "C" int pp_grad_scale_from_counts_adj_fmt1(pp_ctx* ctx, const int* counts_dev, int n_counts, float* scale2_dev, int log2_adjust);
extern "C" int pp_grad_scale_from_counts_fmt1(pp_ctx* ctx, const int* counts_dev, int n_counts, float* scale2_dev);
extern "C" int pp_conv_split_weights_bf16x3_batch_fmt0(pp_ctx* ctx, int n_jobs, const pp_split_job* jobs_dev, int total_tiles);
extern "C" int pp_conv_split_weights_bf16x3_batch_fmt1(pp_ctx* ctx, int n_jobs, const pp_split_job* jobs_dev, int total_tiles);
extern "C" int pp_conv_split_weights_bf16x3_fmt0(pp_ctx* ctx, const pp_conv_desc* d, const float* w, void* fwd_hi, void* fwd_lo, void* dgrad_hi, void* dgrad_lo);
extern "C" int pp_conv_split_weights_bf16x3_fmt1(pp_ctx* ctx, const pp_conv_desc* d, const float* w, void* fwd_hi, void* fwd_lo, void* dgrad_hi, void* dgrad_lo);
extern "C" int pp_conv2d_nhwc_fwd_bf16x3_fmt0(pp_ctx* ctx, const pp_conv_desc* d, const float* x, const void* x_hi, const void* x_lo, const void* w_fwd_hi, const void* w_fwd_lo, const float* bias, const float* residual, int ld_res, int relu, float* y, void* y_hi, void* y_lo, const pp_conv_opts* opts);
extern "C" int pp_conv2d_nhwc_fwd_bf16x3_fmt1(pp_ctx* ctx, const pp_conv_desc* d, const float* x, const void* x_hi, const void* x_lo, const void* w_fwd_hi, const void* w_fwd_lo, const float* bias, const float* residual, int ld_res, int relu, float* y, void* y_hi, void* y_lo, const pp_conv_opts* opts);
extern "C" int pp_row_block_dilate_fmt0(pp_ctx* ctx, const pp_conv_desc* d, const unsigned char* in_flags, unsigned char* out_flags);
extern "C" int pp_row_block_dilate_fmt1(pp_ctx* ctx, const pp_conv_desc* d, const unsigned char* in_flags, unsigned char* out_flags);
extern "C" int pp_stem7x7s2_fwd_bf16x3_fmt0(pp_ctx* ctx, int n_img, int H, int W, int Hp, int Wp, const float* x4p, const void* w_hi, const void* w_lo, int cout, const float* bias, int relu, float* y, int ld_y);
extern "C" int pp_stem7x7s2_fwd_bf16x3_fmt1(pp_ctx* ctx, int n_img, int H, int W, int Hp, int Wp, const float* x4p, const void* w_hi, const void* w_lo, int cout, const float* bias, int relu, float* y, int ld_y);
extern "C" int pp_conv2d_nhwc_bwd_data_bf16x3_fmt0(pp_ctx* ctx, const pp_conv_desc* d, const float* dy, const void* dy_hi, const void* dy_lo, const void* w_dgrad_hi, const void* w_dgrad_lo, const float* addend, int ld_add, const float* relu_src, int ld_rs, float* dx, void* dx_hi, void* dx_lo, const pp_conv_opts* opts);
extern "C" int pp_conv2d_nhwc_bwd_data_s2_bf16x3_fmt0(pp_ctx* ctx, const pp_conv_desc* d, const float* dy, const void* dy_hi, const void* dy_lo, const void* w_dgrad_hi, const void* w_dgrad_lo, const float* addend, int ld_add, const float* relu_src, int ld_rs, float* dx, void* dx_hi, void* dx_lo, const pp_conv_opts* opts);
extern "C" int pp_conv2d_nhwc_bwd_data_bf16x3_fmt1(pp_ctx* ctx, const pp_conv_desc* d, const float* dy, const void* dy_hi, const void* dy_lo, const void* w_dgrad_hi, const void* w_dgrad_lo, const float* addend, int ld_add, const float* relu_src, int ld_rs, float* dx, void* dx_hi, void* dx_lo, const pp_conv_opts* opts);
extern "C" int pp_conv2d_nhwc_bwd_data_s2_bf16x3_fmt1(pp_ctx* ctx, const pp_conv_desc* d, const float* dy, const void* dy_hi, const void* dy_lo, const void* w_dgrad_hi, const void* w_dgrad_lo, const float* addend, int ld_add, const float* relu_src, int ld_rs, float* dx, void* dx_hi, void* dx_lo, const pp_conv_opts* opts);
extern "C" int pp_conv2d_nhwc_bwd_weight_bf16x3_fmt0(pp_ctx* ctx, const pp_conv_desc* d, const float* x, const float* dy, const void* x_hi, const void* x_lo, const void* dy_hi, const void* dy_lo, float* dw, float* dbias, const pp_conv_opts* opts);
extern "C" int pp_conv2d_nhwc_bwd_weight_bf16x3_fmt1(pp_ctx* ctx, const pp_conv_desc* d, const float* x, const float* dy, const void* x_hi, const void* x_lo, const void* dy_hi, const void* dy_lo, float* dw, float* dbias, const pp_conv_opts* opts);

extern "C" int pp_row_block_list(pp_ctx* ctx, const float* x, int rows, int ld, int cols, unsigned char* flags, int* list) {
  return (ctx && ctx->planes_fmt == 1) ? pp_row_block_list_fmt1(ctx, x, rows, ld, cols, flags, list) : pp_row_block_list_fmt0(ctx, x, rows, ld, cols, flags, list);
}
extern "C" int pp_row_block_list_planes_within(pp_ctx* ctx, const void* x_hi, const void* x_lo, int rows, int ld, int cols, const unsigned char* within, unsigned char* flags, int* list) {
  return (ctx && ctx->planes_fmt == 1) ? pp_row_block_list_planes_within_fmt1(ctx, x_hi, x_lo, rows, ld, cols, within, flags, list) : pp_row_block_list_planes_within_fmt0(ctx, x_hi, x_lo, rows, ld, cols, within, flags, list);
}
extern "C" int pp_row_block_list_planes(pp_ctx* ctx, const void* x_hi, const void* x_lo, int rows, int ld, int cols, unsigned char* flags, int* list) {
  return (ctx && ctx->planes_fmt == 1) ? pp_row_block_list_planes_fmt1(ctx, x_hi, x_lo, rows, ld, cols, flags, list) : pp_row_block_list_planes_fmt0(ctx, x_hi, x_lo, rows, ld, cols, flags, list);
}
extern "C" int pp_split_planes_bf16x3(pp_ctx* ctx, size_t n, const float* src, void* hi, void* lo) {
  return (ctx && ctx->planes_fmt == 1) ? pp_split_planes_bf16x3_fmt1(ctx, n, src, hi, lo) : pp_split_planes_bf16x3_fmt0(ctx, n, src, hi, lo);
}
extern "C" int pp_split_planes_scaled_bf16x3(pp_ctx* ctx, size_t n, const float* src, void* hi, void* lo, const float* scale_dev) {
  return (ctx && ctx->planes_fmt == 1) ? pp_split_planes_scaled_bf16x3_fmt1(ctx, n, src, hi, lo, scale_dev) : pp_split_planes_scaled_bf16x3_fmt0(ctx, n, src, hi, lo, scale_dev);
}
extern "C" int pp_grad_scale_from_counts(pp_ctx* ctx, const int* counts_dev, int n_counts, float* scale2_dev) {
  return (ctx && ctx->planes_fmt == 1) ? pp_grad_scale_from_counts_fmt1(ctx, counts_dev, n_counts, scale2_dev) : pp_grad_scale_from_counts_fmt0(ctx, counts_dev, n_counts, scale2_dev);
}
extern "C" int pp_grad_scale_from_counts_adj(pp_ctx* ctx, const int* counts_dev, int n_counts, float* scale2_dev, int log2_adjust) {
  return (ctx && ctx->planes_fmt == 1) ? pp_grad_scale_from_counts_adj_fmt1(ctx, counts_dev, n_counts, scale2_dev, log2_adjust) : pp_grad_scale_from_counts_adj_fmt0(ctx, counts_dev, n_counts, scale2_dev, log2_adjust);
}
extern "C" int pp_conv_split_weights_bf16x3_batch(pp_ctx* ctx, int n_jobs, const pp_split_job* jobs_dev, int total_tiles) {
  return (ctx && ctx->planes_fmt == 1) ? pp_conv_split_weights_bf16x3_batch_fmt1(ctx, n_jobs, jobs_dev, total_tiles) : pp_conv_split_weights_bf16x3_batch_fmt0(ctx, n_jobs, jobs_dev, total_tiles);
}
extern "C" int pp_conv_split_weights_bf16x3(pp_ctx* ctx, const pp_conv_desc* d, const float* w, void* fwd_hi, void* fwd_lo, void* dgrad_hi, void* dgrad_lo) {
  return (ctx && ctx->planes_fmt == 1) ? pp_conv_split_weights_bf16x3_fmt1(ctx, d, w, fwd_hi, fwd_lo, dgrad_hi, dgrad_lo) : pp_conv_split_weights_bf16x3_fmt0(ctx, d, w, fwd_hi, fwd_lo, dgrad_hi, dgrad_lo);
}
extern "C" int pp_conv2d_nhwc_fwd_bf16x3(pp_ctx* ctx, const pp_conv_desc* d, const float* x, const void* x_hi, const void* x_lo, const void* w_fwd_hi, const void* w_fwd_lo, const float* bias, const float* residual, int ld_res, int relu, float* y, void* y_hi, void* y_lo, const pp_conv_opts* opts) {
  return (ctx && ctx->planes_fmt == 1) ? pp_conv2d_nhwc_fwd_bf16x3_fmt1(ctx, d, x, x_hi, x_lo, w_fwd_hi, w_fwd_lo, bias, residual, ld_res, relu, y, y_hi, y_lo, opts) : pp_conv2d_nhwc_fwd_bf16x3_fmt0(ctx, d, x, x_hi, x_lo, w_fwd_hi, w_fwd_lo, bias, residual, ld_res, relu, y, y_hi, y_lo, opts);
}
extern "C" int pp_row_block_dilate(pp_ctx* ctx, const pp_conv_desc* d, const unsigned char* in_flags, unsigned char* out_flags) {
  return (ctx && ctx->planes_fmt == 1) ? pp_row_block_dilate_fmt1(ctx, d, in_flags, out_flags) : pp_row_block_dilate_fmt0(ctx, d, in_flags, out_flags);
}
extern "C" int pp_stem7x7s2_fwd_bf16x3(pp_ctx* ctx, int n_img, int H, int W, int Hp, int Wp, const float* x4p, const void* w_hi, const void* w_lo, int cout, const float* bias, int relu, float* y, int ld_y) {
  return (ctx && ctx->planes_fmt == 1) ? pp_stem7x7s2_fwd_bf16x3_fmt1(ctx, n_img, H, W, Hp, Wp, x4p, w_hi, w_lo, cout, bias, relu, y, ld_y) : pp_stem7x7s2_fwd_bf16x3_fmt0(ctx, n_img, H, W, Hp, Wp, x4p, w_hi, w_lo, cout, bias, relu, y, ld_y);
}
extern "C" int pp_conv2d_nhwc_bwd_data_bf16x3(pp_ctx* ctx, const pp_conv_desc* d, const float* dy, const void* dy_hi, const void* dy_lo, const void* w_dgrad_hi, const void* w_dgrad_lo, const float* addend, int ld_add, const float* relu_src, int ld_rs, float* dx, void* dx_hi, void* dx_lo, const pp_conv_opts* opts) {
  return (ctx && ctx->planes_fmt == 1) ? pp_conv2d_nhwc_bwd_data_bf16x3_fmt1(ctx, d, dy, dy_hi, dy_lo, w_dgrad_hi, w_dgrad_lo, addend, ld_add, relu_src, ld_rs, dx, dx_hi, dx_lo, opts) : pp_conv2d_nhwc_bwd_data_bf16x3_fmt0(ctx, d, dy, dy_hi, dy_lo, w_dgrad_hi, w_dgrad_lo, addend, ld_add, relu_src, ld_rs, dx, dx_hi, dx_lo, opts);
}
extern "C" int pp_conv2d_nhwc_bwd_data_s2_bf16x3(pp_ctx* ctx, const pp_conv_desc* d, const float* dy, const void* dy_hi, const void* dy_lo, const void* w_dgrad_hi, const void* w_dgrad_lo, const float* addend, int ld_add, const float* relu_src, int ld_rs, float* dx, void* dx_hi, void* dx_lo, const pp_conv_opts* opts) {
  return (ctx && ctx->planes_fmt == 1) ? pp_conv2d_nhwc_bwd_data_s2_bf16x3_fmt1(ctx, d, dy, dy_hi, dy_lo, w_dgrad_hi, w_dgrad_lo, addend, ld_add, relu_src, ld_rs, dx, dx_hi, dx_lo, opts) : pp_conv2d_nhwc_bwd_data_s2_bf16x3_fmt0(ctx, d, dy, dy_hi, dy_lo, w_dgrad_hi, w_dgrad_lo, addend, ld_add, relu_src, ld_rs, dx, dx_hi, dx_lo, opts);
}
extern "C" int pp_conv2d_nhwc_bwd_weight_bf16x3(pp_ctx* ctx, const pp_conv_desc* d, const float* x, const float* dy, const void* x_hi, const void* x_lo, const void* dy_hi, const void* dy_lo, float* dw, float* dbias, const pp_conv_opts* opts) {
  return (ctx && ctx->planes_fmt == 1) ? pp_conv2d_nhwc_bwd_weight_bf16x3_fmt1(ctx, d, x, dy, x_hi, x_lo, dy_hi, dy_lo, dw, dbias, opts) : pp_conv2d_nhwc_bwd_weight_bf16x3_fmt0(ctx, d, x, dy, x_hi, x_lo, dy_hi, dy_lo, dw, dbias, opts);
}

extern "C" int pp_conv_s2_merged(void) { return pp_sw_s2_merged() ? 1 : 0; }

// The plan of a call as text, without a context (include/pyrapose_hip.h): the facts come from the same functions the entry points
// of conv3.hip use, the plans from conv_plan.h.
extern "C" int pp_conv_plan_text(const pp_conv_desc* d, int pass, unsigned forms, int planes_fmt, int n_cu, size_t ws_bytes, char* buf,
                                 int buf_bytes) {
  if (!buf || buf_bytes <= 0 || pass < PP_PLAN_FWD || pass > PP_PLAN_BWD_DATA_S2) return PP_ERR_ARG;
  const int rc = check_desc(nullptr, d, "pp_conv_plan_text");
  if (rc) return rc;
  const bool planes_in = forms & PP_PLAN_PLANES_IN, planes_out = forms & PP_PLAN_PLANES_OUT, f32_out = (forms & PP_PLAN_F32_OUT) || !planes_out,
             capture = forms & PP_PLAN_CAPTURE, list = forms & PP_PLAN_LIST, lazy_in = forms & PP_PLAN_LAZY_IN;
  const bool ws = ws_bytes > 0;
  int at = 0;
  buf[0] = 0;
  if (pass == PP_PLAN_BWD_WEIGHT) {
    if (d->cin % 64 != 0) return PP_ERR_SHAPE;
    Wgrad3Params p;
    memset(&p, 0, sizeof(p));
    wgrad_geometry(nullptr, d, p);
    const PpWgradFacts f = wgrad_facts(p, planes_in, list, lazy_in, planes_fmt, n_cu, ws, (long long)ws_bytes, true, true);
    return pp_plan_print(buf, buf_bytes, at, f, pp_plan_wgrad(f), true);
  }
  IgemmParams p;
  memset(&p, 0, sizeof(p));
  if (pass == PP_PLAN_FWD) {
    if (d->cin % 32 != 0) return PP_ERR_SHAPE;
    igemm_geometry_fwd(nullptr, d, p);
    PpIgemmFacts f = igemm_facts(p, d->cout, d->cin / 8, planes_in, !planes_in, planes_out, f32_out, capture, false, n_cu, ws, (long long)ws_bytes);
    if (list) {  // pp_conv_opts.out_flags
      if (!fwd_listed_ok(d, f, false)) return PP_ERR_SHAPE;
      f.listed = true;
      f.listed_tm = 2;
    }
    return pp_plan_print(buf, buf_bytes, at, f, pp_plan_igemm(f), true);
  }
  if (d->cin % 16 != 0) return PP_ERR_SHAPE;
  igemm_geometry_bwd_data(nullptr, d, p);
  const int w_rows = d->cin, w_ld8 = p.Cred / 8;
  const PpIgemmFacts f = igemm_facts(p, w_rows, w_ld8, planes_in, !planes_in, planes_out, f32_out, capture, list, n_cu, ws, (long long)ws_bytes);
  if (pass == PP_PLAN_BWD_DATA_S2) {  // pp_conv2d_nhwc_bwd_data_s2_bf16x3: its options are the epilogue planes alone
    DgradS2Route s2;
    s2.ok = false;
    if (!(forms & (PP_PLAN_LIST | PP_PLAN_LAZY_IN | PP_PLAN_LAZY_OUT))) dgrad_s2_route(d, p, f, &s2);
    if (!s2.ok) return pp_plan_append(buf, buf_bytes, at, "igemm3 s2 refused: not a stride-2, one-level, all-f32 or all-planes data gradient\n");
    return pp_plan_print(buf, buf_bytes, at, s2.f, s2.pl, s2.g, true);
  }
  DgradRoute route;
  dgrad_route(d, p, f, list, &route);
  if (lazy_in && !route.listed) return pp_plan_append(buf, buf_bytes, at, "igemm3 refused: lazy dy without a listed-block launch\n");
  dgrad_launches(
      route, p,
      [&](IgemmParams& q, bool is_class, bool listed) {
        PpIgemmFacts fq = igemm_facts(q, w_rows, w_ld8, planes_in, !planes_in, planes_out, f32_out, capture && !is_class, list && !is_class, n_cu, ws,
                                      (long long)ws_bytes);
        fq.listed = listed;
        fq.listed_tm = route.listed_tm;
        at = pp_plan_print(buf, buf_bytes, at, fq, pp_plan_igemm(fq), true);
      },
      [&](IgemmParams& q) {
        at = pp_plan_append(buf, buf_bytes, at, "class M %d N %d: no taps class_fill | grid=%u\n", q.M, q.Nout,
                            pp_finish_blocks(q.M, q.Nout, pp_cus(n_cu)));
      });
  return at;
}
