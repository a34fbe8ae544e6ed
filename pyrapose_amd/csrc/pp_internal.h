// Internal helpers shared by the HIP translation units of libpyrapose_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "pyrapose_hip.h"

struct pp_ctx {
  int device;
  hipStream_t stream;
  int n_cu;
  char name[128];
  char err[512];
  float* ws;        // caller-provided scratch for split-K partial sums (slices)
  size_t ws_bytes;
  int planes_fmt;          // format of every (hi, lo) plane pair this context sees: 0 = bf16 pairs (bf16x3), 1 = P16 (f16c8)
  const float* grad_scale; // device {2^G, 2^-G}: the gradient planes this context's weight gradients read carry the factor 2^G
};

static inline int pp_fail(pp_ctx* ctx, int code, const char* fmt, ...) {
  if (ctx) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

#define PP_REQUIRE_CTX(ctx) \
  do {                      \
    if (!(ctx)) return PP_ERR_NOCTX; \
  } while (0)

#define PP_CHECK_ARG(ctx, cond, code, ...)            \
  do {                                                \
    if (!(cond)) return pp_fail(ctx, code, __VA_ARGS__); \
  } while (0)

// Launch-error check: hipGetLastError is not a synchronisation.
#define PP_CHECK_LAUNCH(ctx, what)                                                   \
  do {                                                                               \
    hipError_t e__ = hipGetLastError();                                              \
    if (e__ != hipSuccess)                                                           \
      return pp_fail(ctx, (int)e__, "%s: launch failed: %s", what, hipGetErrorString(e__)); \
  } while (0)

#define PP_HIP(ctx, call)                                                                        \
  do {                                                                                           \
    hipError_t e__ = (call);                                                                     \
    if (e__ != hipSuccess) return pp_fail(ctx, (int)e__, "%s: %s", #call, hipGetErrorString(e__)); \
  } while (0)

static inline long long pp_rowspace_rows(const pp_rowspace* rs) {
  long long r = 0;
  for (int s = 0; s < rs->n_seg; ++s) r += (long long)rs->n_img * rs->h[s] * rs->w[s];
  return r;
}

static inline int pp_rowspace_ok(const pp_rowspace* rs) {
  if (rs->n_img <= 0 || rs->n_seg <= 0 || rs->n_seg > PP_MAX_SEG) return 0;
  for (int s = 0; s < rs->n_seg; ++s)
    if (rs->h[s] <= 0 || rs->w[s] <= 0) return 0;
  return pp_rowspace_rows(rs) < (1ll << 31);
}

static inline int pp_is_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
// packed (hi, lo) planes: one buffer of 32-byte groups (8 channels: 16 bytes of hi, 16 bytes of lo); lo = hi + 16 bytes
static inline int pp_is_packed(const void* hi, const void* lo) {
  return (hi == nullptr && lo == nullptr) || (hi != nullptr && (const char*)lo == (const char*)hi + 16 && pp_is_aligned16(hi));
}

// pp_conv_opts of a *_bf16x3 convolution call, checked before anything else: NULL becomes the all-zero struct, the field groups
// outside `takes` (those the entry point `who` does not consume) must be null / zero, the others well formed.
enum { PP_OPT_CAPTURE = 1, PP_OPT_ADD = 2, PP_OPT_MASK = 4, PP_OPT_SKIP = 8, PP_OPT_LAZY_OUT = 16, PP_OPT_LAZY_IN = 32, PP_OPT_OUT = 64 };
static inline int pp_conv_opts_take(pp_ctx* ctx, const pp_conv_opts*& o, unsigned takes, const char* who) {
  static const pp_conv_opts none = {};
  if (!o) o = &none;
  const struct { unsigned group; bool set; const char* name; } fields[] = {
      {PP_OPT_CAPTURE, o->capture_hi != nullptr, "capture_hi"}, {PP_OPT_CAPTURE, o->capture_lo != nullptr, "capture_lo"},
      {PP_OPT_ADD, o->add_hi != nullptr, "add_hi"},             {PP_OPT_ADD, o->add_lo != nullptr, "add_lo"},
      {PP_OPT_MASK, o->mask_hi != nullptr, "mask_hi"},          {PP_OPT_SKIP, o->skip_flags != nullptr, "skip_flags"},
      {PP_OPT_SKIP, o->skip_list != nullptr, "skip_list"},      {PP_OPT_OUT, o->out_flags != nullptr, "out_flags"},
      {PP_OPT_OUT, o->out_list != nullptr, "out_list"},         {PP_OPT_LAZY_OUT, o->lazy_out != 0, "lazy_out"},
      {PP_OPT_LAZY_IN, o->lazy_in != 0, "lazy_in"}};
  for (const auto& f : fields) PP_CHECK_ARG(ctx, !f.set || (takes & f.group), PP_ERR_ARG, "%s: pp_conv_opts.%s is not an option of this call", who, f.name);
  PP_CHECK_ARG(ctx, (o->capture_hi == nullptr) == (o->capture_lo == nullptr) && pp_is_aligned16(o->capture_hi) && pp_is_aligned16(o->capture_lo),
               PP_ERR_ARG, "%s: pp_conv_opts.capture_hi and capture_lo go together, 16-byte aligned", who);
  PP_CHECK_ARG(ctx, (o->add_hi == nullptr) == (o->add_lo == nullptr), PP_ERR_ARG, "%s: pp_conv_opts.add_hi and add_lo go together", who);
  PP_CHECK_ARG(ctx, pp_is_packed(o->add_hi, o->add_lo) && pp_is_aligned16(o->mask_hi), PP_ERR_ALIGN,
               "%s: pp_conv_opts epilogue planes must be packed (lo = hi + 16 bytes) and 16-byte aligned", who);
  PP_CHECK_ARG(ctx, (o->out_flags == nullptr) == (o->out_list == nullptr), PP_ERR_ARG, "%s: pp_conv_opts.out_flags and out_list go together", who);
  PP_CHECK_ARG(ctx, !(o->lazy_out || o->lazy_in) || (o->skip_flags && o->skip_list), PP_ERR_ARG,
               "%s: pp_conv_opts.lazy_out / lazy_in go with skip_flags and skip_list", who);
  return PP_OK;
}
