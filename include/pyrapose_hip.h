/* pyrapose_hip.h -- C ABI of the MI355X-native PyraPose hot path (gfx950 / CDNA4).
 *
 * Drop-in boundary for the path SURVEY.md §8 scopes: ResNet-50 -> PyraPose feature pyramid ->
 * shared heads (forward + backward), its losses, optimizer, and the anchor / target / decode ops.
 * The reference has no operator ABI for this path (it is a Keras graph); each entry
 * point below names the reference symbol (file:line, relative to the reference repo root) whose
 * arithmetic it replaces.  The reference's only real C ABI (`uncertainty_pnp/src/ext.h:1-9`) sets
 * the house style: caller-owned buffers, plain pointers and sizes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - tensors are NHWC float32 matrices `[rows][ld]` (row = (image, y, x), ld >= channels);
 *   - all launches are asynchronous on the ctx stream; no hidden device synchronisation;
 *   - return: 0 ok; < 0 argument / shape error detected on the host before any launch;
 *     > 0 a hipError_t.  Never throws, never aborts.  `pp_last_error_string` gives detail.
 *   - one ctx per (process, device, stream); calls on one ctx are not thread-safe, calls on
 *     different ctxs are independent.
 */
#ifndef PYRAPOSE_HIP_H
#define PYRAPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_OK 0
#define PP_ERR_ARG (-1)
#define PP_ERR_SHAPE (-2)
#define PP_ERR_ALIGN (-3)
#define PP_ERR_NOCTX (-4)
#define PP_ERR_UNSUPPORTED (-5) /* an optional dependency is missing (librccl.so for the pp_comm_* / pp_allreduce_* entry points) */
#define PP_ERR_COMM (-6)        /* RCCL returned an error (text in pp_last_error) */

#define PP_MAX_SEG 5

typedef struct pp_ctx pp_ctx;

/* ---- context -------------------------------------------------------------------------- */
int pp_ctx_create(pp_ctx** out, int device, void* hip_stream);
void pp_ctx_destroy(pp_ctx* ctx);
int pp_ctx_set_stream(pp_ctx* ctx, void* hip_stream);
/* Optional scratch for the bf16x3 convolutions (any contents).  With it, launches whose output tiles cannot fill the
 * chip split their reduction over S workgroups per tile: each writes its partial sums to slice s of the scratch and a
 * finishing pass adds the slices in a fixed order and applies bias / residual / mask / ReLU (deterministic, no
 * atomics).  A launch uses S * rows * ld_out * 4 bytes.  One buffer per context (= per stream); NULL, 0 removes it. */
int pp_ctx_set_workspace(pp_ctx* ctx, void* device_buffer, size_t bytes);
/* Row-block skip for sparse gradients.  The 3D-box loss (losses.py:321-408, orthogonal_l1) keeps only the rows with anchor
 * state 1, so the gradient that flows back through the 3D-box head is exactly zero away from the positive anchors (and
 * stays so layer after layer, dilated by one pixel per 3x3 conv).  pp_row_block_list scans a gradient tensor x [rows][ld]
 * (first `cols` columns) once: flags[b] = 1 when the 32-row block b holds a non-zero (or a NaN), list = {count, the flagged
 * block indices ascending}.  With nb = ceil(rows/32): flags holds 2 nb bytes and list 2 (nb + 1) ints of device memory --
 * the first halves are the result, the second halves scratch of the bwd-data launch that takes the hint (after that launch the
 * second nb bytes of `flags` flag every block of dx that may hold a non-zero: the dilated blocks, or all of them when the
 * launch ran dense; without an addend dx is zero in the others -- pp_row_block_list_planes_within takes that as `within`).
 * The pair goes to a backward launch as the skip_flags / skip_list fields of its pp_conv_opts (below). */
int pp_row_block_list(pp_ctx* ctx, const float* x, int rows, int ld, int cols, unsigned char* flags, int* list);
/* the same scan of a tensor stored as bf16 (hi, lo) planes ([rows][ld] each) */
int pp_row_block_list_planes(pp_ctx* ctx, const void* x_hi, const void* x_lo, int rows, int ld, int cols, unsigned char* flags, int* list);
/* the same, reading only the blocks flagged in `within` ([n_blocks] bytes; NULL = all): for a tensor the caller knows to be zero
 * elsewhere -- the data gradient a row-block-skip launch has just written is zero outside the blocks that launch listed (the
 * second n_blocks bytes of ITS flags buffer), so the scan for the next layer reads 10-25 % of the tensor instead of all of it. */
int pp_row_block_list_planes_within(pp_ctx* ctx, const void* x_hi, const void* x_lo, int rows, int ld, int cols, const unsigned char* within,
                                    unsigned char* flags, int* list);
const char* pp_last_error_string(pp_ctx* ctx);
const char* pp_version(void);
/* number of compute units / name of the device the ctx is bound to (for bench metadata) */
int pp_device_info(pp_ctx* ctx, int* n_cu, char* name_host, int name_len);

/* ---- convolution family ---------------------------------------------------------------
 * Replaces the TensorFlow conv kernels behind every keras.layers.Conv2D of
 *   models/retinanet.py:9-54,57-98,101-131 (heads), :180-214 (__create_sparceFPN) and
 *   keras_resnet.models.ResNet50 called at models/resnet.py:87 (backbone).
 * Implicit-GEMM direct convolution (no im2col buffer) on v_mfma_f32_32x32x2_f32.
 *
 * A "row space" is a list of up to PP_MAX_SEG segments; segment s holds n_img images of
 * h[s] x w[s] cells, stored image-major, and rows are numbered segment after segment.  One
 * segment = an ordinary NHWC tensor; several segments = pyramid levels that share weights
 * (models/retinanet.py:224-225) processed by ONE launch.
 */
typedef struct {
  int n_img;             /* images per segment (batch) */
  int n_seg;             /* 1..PP_MAX_SEG */
  int h[PP_MAX_SEG];     /* cells per image, per segment */
  int w[PP_MAX_SEG];
} pp_rowspace;

typedef struct {
  pp_rowspace in;        /* geometry of x (forward input) */
  pp_rowspace out;       /* geometry of y (forward output); out.n_seg == in.n_seg */
  int cin, cout;         /* logical channels */
  int kh, kw, stride;    /* square stride */
  int pad_t, pad_l;      /* top / left zero padding (TF 'same' with stride 2 on even extents pads
                            bottom/right only -> pad_t = pad_l = 0; ZeroPadding2D(1) -> 1) */
  int ld_x, ld_y, ld_w;  /* leading dimensions (floats): x rows, y rows, weight rows.
                            weights are Keras HWIO flattened: w[(ky*kw+kx)*cin + ci][co], ld_w >= cout,
                            ld_w % 16 == 0, padding columns zero. cin % 16 == 0, or cin == 4 (packed-RGB stem:
                            the weight buffer then holds kh*kw*4 rows rounded up to a multiple of 16, zero rows). */
} pp_conv_desc;

/* y = [relu]( conv(x, w) + bias + residual ).  bias / residual may be NULL.  residual has y's shape
 * with leading dimension ld_res. */
int pp_conv2d_nhwc_fwd(pp_ctx* ctx, const pp_conv_desc* d, const float* x, const float* w,
                       const float* bias, const float* residual, int ld_res, int relu, float* y);

/* dx = mask( conv_transpose(dy, w) + addend ),  mask(v) = relu_src > 0 ? v : 0 (relu_src NULL = no mask).
 * dy rows have ld_y floats with channels >= cout zero up to the next multiple of 16.
 * addend / relu_src have dx's shape (leading dims ld_add / ld_rs). */
int pp_conv2d_nhwc_bwd_data(pp_ctx* ctx, const pp_conv_desc* d, const float* dy, const float* w,
                            const float* addend, int ld_add, const float* relu_src, int ld_rs, float* dx);

/* dw += x^T (*) dy  (atomic accumulation into a caller-zeroed HWIO buffer, ld_w);  if dbias != NULL,
 * dbias[co] += sum_rows dy[row][co]. */
int pp_conv2d_nhwc_bwd_weight(pp_ctx* ctx, const pp_conv_desc* d, const float* x, const float* dy,
                              float* dw, float* dbias);

/* ---- float32-class convolution on the bf16 matrix cores ("bf16x3") ---------------------------------------
 * Same operators as above with every product evaluated as x_hi*w_hi + x_hi*w_lo + x_lo*w_hi on
 * v_mfma_f32_32x32x16_bf16 (f32 accumulation; ~2^-16 relative error per product, 5.3x the f32-MFMA rate).
 * Activations stay float32; weights are split once per optimizer step into bf16 (hi, lo) planes:
 *   forward planes  [tap][cout][cin]              (cin % 32 == 0)
 *   bwd-data planes [tap][cin][cout rounded to 32] (zero padded)
 * Any of the plane pairs may be NULL in pp_conv_split_weights_bf16x3. */
int pp_conv_split_weights_bf16x3(pp_ctx* ctx, const pp_conv_desc* d, const float* w, void* fwd_hi, void* fwd_lo,
                                 void* dgrad_hi, void* dgrad_lo);
/* The same for many tensors in one launch.  jobs_dev: DEVICE array of n_jobs entries; job i owns the tiles
 * [tile_begin, tile_begin + taps * (cin/32) * ceil(cout/32)) of the launch, tile_begin ascending from 0;
 * total_tiles = the sum.  Plane pointers as in pp_conv_split_weights_bf16x3 (either pair may be NULL). */
typedef struct pp_split_job {
  const float* w;      /* f32 HWIO [taps*cin][ld_w] */
  void* fwd_hi; void* fwd_lo; void* dg_hi; void* dg_lo;
  int taps, cin, cout, ld_w;
  int tile_begin, reserved;
} pp_split_job;
int pp_conv_split_weights_bf16x3_batch(pp_ctx* ctx, int n_jobs, const pp_split_job* jobs_dev, int total_tiles);
/* Sparse FORWARD of a head whose loss reads a few rows only (training; the 3D-box head: orthogonal_l1 keeps the rows with anchor
 * state 1, losses.py:332-333 -- every other output row of that head is dead in train_on_batch).
 * pp_positive_row_blocks: flags[b] = 1 when the 32-row block b of the head's row space holds an anchor whose last target column
 * (state, column stride - 1 of y_true [n_img][cells][A][stride]) is 1.  pp_row_block_dilate: the blocks within one pixel of a
 * flagged block (what a 3x3 stride-1 conv d reads to produce the flagged blocks): applied once per layer from the head's output
 * back to its first conv.  The flags of a layer go to its forward launch as the
 * out_flags field of its pp_conv_opts (below).  Exact for the loss, its gradient and the weight gradients (the backward reads
 * those activations only where its own row-block skip goes); the caller opts in. */
int pp_positive_row_blocks(pp_ctx* ctx, const pp_rowspace* rs, int A, int stride, const float* y_true, unsigned char* flags);
int pp_row_block_dilate(pp_ctx* ctx, const pp_conv_desc* d, const unsigned char* in_flags, unsigned char* out_flags);
/* f32 tensor of n elements (n % 8 == 0) -> bf16 (hi, lo) planes with the same [rows][ld] geometry.  Convs that are
 * given planes for their gathered operand skip the conversion inside the kernel (the f32 pointer may then be NULL). */
int pp_split_planes_bf16x3(pp_ctx* ctx, size_t n, const float* src, void* hi, void* lo);
/* Format of every (hi, lo) plane pair the *_bf16x3 / *_v entry points of this context read and write -- and with it the arithmetic
 * of the convolutions on them (csrc/planes_fmt.h).  0 (default): bf16 pairs, value = hi + lo, three bf16 MFMAs per product
 * ("bf16x3", 4.5e-6 per launch against float64).  1: "P16" -- hi = IEEE half, lo = two e5m2 bytes per element (e5m2(x), e5m2((x - hi)
 * * 2^12); swapped for weights), value = hi + lo8 * 2^-12; one f16 MFMA + half a block-scaled e5m2 MFMA per 16-deep step ("f16c8":
 * 2 MFMA units per product instead of 3, 2.1e-5 per launch, |x| clamped to 28672).  Same packed geometry, same entry points; a
 * tensor written under one format must be read under the same one.  pp_convert_planes re-encodes n elements (n % 8 == 0) from one
 * format into the other, multiplied by scale2_dev[scale_index] when scale2_dev != NULL (pp_grad_scale_from_counts), and set to zero
 * where the tensor whose hi plane is relu_src_hi (same geometry, either format; NULL: none) is not positive -- the ReLU a gradient
 * passes when it crosses the boundary backwards. */
int pp_ctx_set_planes_format(pp_ctx* ctx, int fmt);
int pp_convert_planes(pp_ctx* ctx, size_t n, const void* src_hi, const void* src_lo, int src_fmt, void* dst_hi, void* dst_lo, int dst_fmt,
                      const float* scale2_dev, int scale_index, const void* relu_src_hi);
/* The gradient chain travels multiplied by a power of two (the hi plane holds IEEE halves, which stop at 6e-8; loss gradients are
 * ~1e-7): pp_grad_scale_from_counts writes scale2 = {2^G, 2^-G} with 2^G = 2^8 * 2^floor(log2(max(1, min_i counts[i]))) -- every loss
 * gradient of losses.py:22-68 / :321-408 is bounded by ~1 / max(1, positives of its head); pp_split_planes_scaled_bf16x3 is
 * pp_split_planes_bf16x3 of src * scale_dev[0] (the three loss gradients); every gradient a bwd-data launch or a pointwise kernel
 * derives from them carries the same factor; pp_ctx_set_grad_scale (persistent; NULL = none) makes the weight-gradient launches of
 * this context multiply dW / dbias by scale2[1] when their operands are planes. */
int pp_grad_scale_from_counts(pp_ctx* ctx, const int* counts_dev, int n_counts, float* scale2_dev);
/* the same with G shifted by log2_adjust (-16 .. 16): a caller whose loss weights differ from the reference's defaults (losses.py:
 * orthogonal_l1 weight 0.125, focal alpha 0.25) takes the headroom out of / puts it into the scale -- Engine: -ceil(log2(largest ratio)) */
int pp_grad_scale_from_counts_adj(pp_ctx* ctx, const int* counts_dev, int n_counts, float* scale2_dev, int log2_adjust);
int pp_split_planes_scaled_bf16x3(pp_ctx* ctx, size_t n, const float* src, void* hi, void* lo, const float* scale_dev);
int pp_ctx_set_grad_scale(pp_ctx* ctx, const float* scale2_dev);

/* Per-launch options of the three *_bf16x3 convolution entry points below: passed with the call (NULL = all zero), read
 * before anything is launched, never kept.  A field the entry point does not consume must be NULL / 0: PP_ERR_ARG. */
typedef struct pp_conv_opts {
  /* Split capture (fwd, bwd-data): the call, which must be given its gathered operand (x / dy) as float32, also writes that
   * operand's bf16 (hi, lo) split into these planes -- the output of pp_split_planes_bf16x3 on it ([rows][ld] geometry; columns
   * past the channels the conv reads are left untouched).  The kernel has the converted values in registers anyway; the
   * weight-gradient launch of the same layer (all four planes) then skips its own conversion.  hi and lo go together. */
  void* capture_hi;
  void* capture_lo;
  /* Epilogue planes (fwd: residual; bwd-data: addend, relu_src): the call reads those epilogue operands from bf16 (hi, lo)
   * planes instead of float32 tensors -- the storage format of every activation and gradient a bf16x3 conv produces when its
   * output is requested as planes only (value = hi + lo, 4 bytes per element like float32, so no conv ever converts inside its
   * loop).  The call's ld_res / ld_add / ld_rs arguments give the row pitch of the planes; its float32 residual / addend /
   * relu_src argument must then be NULL.  Of the ReLU source only the hi plane is read (hi > 0 <=> value > 0; bwd-data only).
   * Any of the three may be NULL (add_hi and add_lo go together). */
  const void* add_hi;
  const void* add_lo;
  const void* mask_hi;
  /* Row-block skip (bwd-data, bwd-weight): the (flags, list) pair pp_row_block_list wrote for the call's dy.  The bwd-weight
   * call reduces over the listed blocks of dy only; the bwd-data call (3x3, stride 1, pad 1) computes only the 32-row blocks of
   * dx that a flagged block of dy can reach (dilated by one pixel in 2-D, compacted four to a tile) and writes mask?(addend or
   * 0) to the others -- and WRITES the second halves of both buffers (not const).  A block of zero rows contributes exactly 0.0
   * to every sum: the results are those of the dense launch (up to the order of the float32 atomics between reduction splits;
   * the one exception is an Inf / NaN operand opposite an exact zero, which the dense launch turns into NaN and this one into
   * 0).  Launches that cannot use the pair run dense. */
  unsigned char* skip_flags;
  int* skip_list;
  /* Sparse forward (fwd; 3x3, stride 1, pad 1, plane-stored input, no residual): the call computes the flagged 32-row output
   * blocks only (compacted four to a tile; out_list = scratch of n_blocks + 1 ints) and leaves every other output row as it is.
   * flags and list go together. */
  const unsigned char* out_flags;
  int* out_list;
  /* Lazy sparse gradients (beside skip_flags and skip_list; without them: PP_ERR_ARG).  lazy_out (bwd-data): a call that runs
   * the listed-block launch leaves the rows of dx outside the blocks it computes UNTOUCHED instead of writing mask?(addend or 0)
   * to them -- legitimate when every reader of that dx goes by flags: a scan restricted to the computed blocks
   * (pp_row_block_list_planes_within with the second half of this call's flags), a listed-block bwd-weight, a listed-block
   * bwd-data (whose gather never fetches a row outside the flagged blocks of its dy).  lazy_in (bwd-data, bwd-weight): the dy of
   * the call is such a tensor; the call FAILS (PP_ERR_ARG) instead of running a launch that would read the unwritten rows.  The
   * 3D-box head's backward uses both: four fill passes of 103 MB per training step are not made. */
  int lazy_out;
  int lazy_in;
} pp_conv_opts;
#ifdef __cplusplus
static_assert(sizeof(pp_conv_opts) == 9 * sizeof(void*) + 2 * sizeof(int), "pp_conv_opts: pointers, then ints, no padding");
#else
_Static_assert(sizeof(pp_conv_opts) == 9 * sizeof(void*) + 2 * sizeof(int), "pp_conv_opts: pointers, then ints, no padding");
#endif

int pp_conv2d_nhwc_fwd_bf16x3(pp_ctx* ctx, const pp_conv_desc* d, const float* x, const void* x_hi, const void* x_lo,
                              const void* w_fwd_hi, const void* w_fwd_lo, const float* bias, const float* residual,
                              int ld_res, int relu, float* y, void* y_hi, void* y_lo, const pp_conv_opts* opts);
/* y_hi / y_lo (may be NULL): the epilogue also writes the output pre-split, so that the consumer convs skip the split.
 * With planes given, y (fwd) / dx (bwd_data) may be NULL: the output then exists only as planes. */
/* dy rows need ld_y >= cout rounded up to 32 with zero padding. */
int pp_conv2d_nhwc_bwd_data_bf16x3(pp_ctx* ctx, const pp_conv_desc* d, const float* dy, const void* dy_hi,
                                   const void* dy_lo, const void* w_dgrad_hi, const void* w_dgrad_lo,
                                   const float* addend, int ld_add, const float* relu_src, int ld_rs, float* dx,
                                   void* dx_hi, void* dx_lo, const pp_conv_opts* opts);
/* The stride-2 data gradient in ONE launch: same arguments and, bit for bit, the same dx as pp_conv2d_nhwc_bwd_data_bf16x3, which
 * runs such a gradient as one launch per parity class (cy, cx) of the input grid and fills the classes no tap reaches (three of
 * four for a 1x1 kernel) with a pointwise pass.  Here the tile grids of the classes are one grid, heaviest class first, and a class
 * without taps runs the epilogue alone: dx = relu_src?(addend or 0) there.  For stride 2, one level, operands all float32 (dy, dx)
 * or all planes (dy_hi / dy_lo, dx_hi / dx_lo, dx NULL); of pp_conv_opts only add_hi / add_lo / mask_hi.  Every other call is refused
 * with PP_ERR_ARG before anything is launched -- it never falls back to another route. */
int pp_conv2d_nhwc_bwd_data_s2_bf16x3(pp_ctx* ctx, const pp_conv_desc* d, const float* dy, const void* dy_hi,
                                      const void* dy_lo, const void* w_dgrad_hi, const void* w_dgrad_lo,
                                      const float* addend, int ld_add, const float* relu_src, int ld_rs, float* dx,
                                      void* dx_hi, void* dx_lo, const pp_conv_opts* opts);
/* 1 unless PP_CONV3_S2MERGED=0 (read at every call): whether a caller that has both routes should take the one above -- the
 * Engine asks when it builds its backward plan.  The entry points themselves do not look at the switch. */
int pp_conv_s2_merged(void);
/* dw += x^T (*) dy; operands either f32 (split on the fly) or all four planes; same contract as
 * pp_conv2d_nhwc_bwd_weight, cin % 64 == 0. */
int pp_conv2d_nhwc_bwd_weight_bf16x3(pp_ctx* ctx, const pp_conv_desc* d, const float* x, const float* dy,
                                     const void* x_hi, const void* x_lo, const void* dy_hi, const void* dy_lo,
                                     float* dw, float* dbias, const pp_conv_opts* opts);

/* Host only, no context: which kernels the three entry points above WOULD launch for descriptor d, as text -- one line per launch
 * in the wording of the PP_CONV_DEBUG trace, then the kernel family and, behind " | ", the plan's numbers as key=value.  Built
 * from the same facts and by the same planner as the launches themselves (csrc/conv_plan.h), under the PP_* switches of the
 * calling process.  pass: PP_PLAN_FWD / PP_PLAN_BWD_DATA / PP_PLAN_BWD_WEIGHT.  forms: PP_PLAN_* bits -- how the call would give
 * its operands (gathered operand and, for the weight gradient, both operands as planes; output as planes and / or f32, f32 when
 * neither bit is set; split capture; skip_flags + skip_list, or out_flags + out_list in the forward pass; lazy_in; lazy_out).
 * planes_fmt as pp_ctx_set_planes_format, n_cu and ws_bytes as the context would hold them (ws_bytes 0: no scratch).
 * Returns the bytes written to buf (text is cut at buf_bytes - 1) or a PP_ERR_* code. */
#define PP_PLAN_FWD 0
#define PP_PLAN_BWD_DATA 1
#define PP_PLAN_BWD_WEIGHT 2
#define PP_PLAN_BWD_DATA_S2 3 /* pp_conv2d_nhwc_bwd_data_s2_bf16x3: one line, or a "refused" line where the call would return PP_ERR_ARG */
#define PP_PLAN_PLANES_IN 1u
#define PP_PLAN_PLANES_OUT 2u
#define PP_PLAN_F32_OUT 4u
#define PP_PLAN_CAPTURE 8u
#define PP_PLAN_LIST 16u
#define PP_PLAN_LAZY_IN 32u
#define PP_PLAN_LAZY_OUT 64u
int pp_conv_plan_text(const pp_conv_desc* d, int pass, unsigned forms, int planes_fmt, int n_cu, size_t ws_bytes, char* buf,
                      int buf_bytes);

/* ---- data-parallel gradient exchange on RCCL -----------------------------------------------------------
 * The reference trains on one device (bin/train.py:82-89: the multi_gpu_model branch is disabled); what its single-device
 * semantics fix is that the loss normalisers count positives over the WHOLE batch (losses.py:62-66, :402-405) and that Adam clips
 * by the GLOBAL gradient norm (bin/train.py:101).  With the batch sharded per image over one process per GPU that takes a SUM
 * all-reduce of the three positive counts and a SUM all-reduce of the flat gradient buffer -- here as plain entry points on a
 * communicator the library owns, so that the engine decides the stream (its own), the bucket and the moment (pyrapose_amd/
 * parallel.py launches a bucket as soon as the last weight-gradient kernel that writes into it is enqueued).
 * librccl.so is loaded with dlopen on first use (PP_RCCL_LIB overrides the name); without it these calls return
 * PP_ERR_UNSUPPORTED and pp_comm_available() is 0.  id128: the 128 bytes of an ncclUniqueId -- rank 0 calls pp_comm_unique_id and
 * hands the bytes to every rank by any channel; pp_comm_init is collective over the `world` ranks (one communicator per process,
 * bound to the context's device).  All-reduces run in place, asynchronously, on the context's stream. */
typedef struct pp_comm pp_comm;
int pp_comm_available(void);
int pp_comm_unique_id(pp_ctx* ctx, void* id128);
int pp_comm_init(pp_ctx* ctx, int world, int rank, const void* id128, pp_comm** out);
int pp_comm_destroy(pp_comm* comm);
int pp_allreduce_bucket(pp_ctx* ctx, pp_comm* comm, float* buf, size_t count);
int pp_allreduce_counts(pp_ctx* ctx, pp_comm* comm, int* counts, int n);

/* ---- pooling / resampling / pointwise --------------------------------------------------
 * keras_resnet pool1 = MaxPooling2D(3, strides 2, 'same') (called via models/resnet.py:87). */
int pp_maxpool3x3s2_fwd(pp_ctx* ctx, int n_img, int h, int w, int c, const float* x, int oh, int ow, float* y);
/* UpsampleLike: layers/_misc.py:96-109 -> backend/tf_backend.py:28-35 (tf.image.resize NEAREST, TF 2.1:
 * src = floor((dst + 0.5) * in / out)).   out = up(src) + other  (other may be NULL). */
int pp_upsample_nearest_add_fwd(pp_ctx* ctx, int n_img, int sh, int sw, int th, int tw, int c,
                                const float* src, const float* other, float* out);
/* dsrc = base + sum over the target cells that map to each source cell of dtarget (base may be NULL) */
int pp_upsample_nearest_add_bwd(pp_ctx* ctx, int n_img, int sh, int sw, int th, int tw, int c,
                                const float* dtarget, const float* base, float* dsrc);
/* out = a + b (+ c)   (keras.layers.Add, models/retinanet.py:198-211); b, c may be NULL */
int pp_add_n(pp_ctx* ctx, size_t n, const float* a, const float* b, const float* c, float* out);
/* y = max(x, 0): the stand-alone Activation('relu') between P6 and the P7 conv of __create_pyramid_features
 * (models/retinanet.py:154).  Its backward is the relu_src mask of the consumer's pp_conv2d_nhwc_bwd_data*. */
int pp_relu_fwd(pp_ctx* ctx, size_t n, const float* x, float* y);
/* The same pointwise ops on tensors in either storage format: a view is a float32 tensor (f32) or a pair of bf16 (hi, lo)
 * planes with the same [rows][ld] geometry (value = hi + lo); an OUTPUT view may carry both, and both are then written.
 * Inputs that may be NULL in the float32 entry points may be NULL views (all three pointers NULL) here. */
typedef struct pp_tview {
  const float* f32;
  const void* hi;
  const void* lo;
} pp_tview;
int pp_add_n_v(pp_ctx* ctx, size_t n, const pp_tview* a, const pp_tview* b, const pp_tview* c, const pp_tview* out);
int pp_relu_fwd_v(pp_ctx* ctx, size_t n, const pp_tview* x, const pp_tview* y);
int pp_upsample_nearest_add_fwd_v(pp_ctx* ctx, int n_img, int sh, int sw, int th, int tw, int c, const pp_tview* src,
                                  const pp_tview* other, const pp_tview* out);
int pp_upsample_nearest_add_bwd_v(pp_ctx* ctx, int n_img, int sh, int sw, int th, int tw, int c, const pp_tview* dtarget,
                                  const pp_tview* base, const pp_tview* dsrc);
/* planes -> float32 (value = hi + lo), n % 4 == 0: the inverse of pp_split_planes_bf16x3 up to 2^-17 */
int pp_merge_planes_bf16x3(pp_ctx* ctx, size_t n, const void* hi, const void* lo, float* dst);
/* Audit of a P16 tensor [rows][ld] (packed planes, columns < cols; ld, cols % 8 == 0; the context must be in plane format 1): ADDS to
 * stats5_dev[0..3] (uint64, device) the elements looked at, the non-zero halves, the halves AT the encode's clamp (|h| >= 28 672) and
 * the subnormal halves (0 < |h| < 2^-14); stats5_dev[4] = max(stats5_dev[4], largest |half| seen as its 15 bits).  within (may be NULL): uint8 flags of the 32-row blocks to look at.  The P16 encode clamps
 * and a half underflows silently (csrc/p16.h); this is how a caller sees whether a step came near either end: Engine.p16_stats(),
 * asserted in tests/test_gpu_parity.py, printed by bench.py.  No reference counterpart (the reference computes in float32). */
int pp_planes_stats(pp_ctx* ctx, const void* hi, const void* lo, long long rows, int ld, int cols, const unsigned char* within,
                    unsigned long long* stats5_dev);
/* [n_img,h,w,3] -> [n_img,h,w,4] zero-padded channel (feeds conv1 as cin == 4) */
int pp_pack_rgb_to_4(pp_ctx* ctx, size_t n_pixels, const float* x3, float* x4);
/* utils/image.py:35-62 preprocess_image(mode='caffe') + preprocessing/generator.py:319-336 compute_inputs in one pass:
 * images_u8 [n_img,H,W,3] uint8 (BGR as the reference reads them; image b occupies the upper-left sizes_hw[b] = (h, w)
 * corner of the frame) -> x4 [n_img,H,W,4] float32 = pixel - (103.939, 116.779, 123.68) inside the image, 0 in the
 * padding and in channel 3.  sizes_hw is a HOST array of 2*n_img ints (n_img <= 64). */
int pp_preprocess_caffe_u8(pp_ctx* ctx, int n_img, int H, int W, const int* sizes_hw_host, const unsigned char* images_u8,
                           float* x4);
/* ---- geometric augmentation / resize of the input pipeline ------------------------------------------
 * Replace the reference's OpenCV calls: utils/image.py:150-216 apply_transform (cv2.warpAffine of the uint8 image, INTER_LINEAR,
 * border per TransformParameters: 'constant' / 'nearest' = replicate), :219-230 apply_transform2mask (cv2.warpAffine of the
 * id mask, INTER_NEAREST, BORDER_CONSTANT 0), :281-323 compute_resize_scale / resize_image (cv2.resize, fx = fy = scale).
 * OpenCV's fixed-point scheme for 8-bit images, in integer arithmetic (bit-exact against oracle/image_np.py; OpenCV itself is
 * not installed: parity unpinned).  mats_host: n_img (<= 64) row-major 2x3 FORWARD matrices as the reference passes them to
 * cv2.warpAffine (the kernels invert them like OpenCV does).  interpolation 0 = nearest (1 channel), 1 = linear (1 or 3
 * channels); border 0 = constant (cval), 1 = replicate.  src / dst: [n_img][H][W][channels] uint8, distinct buffers. */
int pp_warp_affine_u8(pp_ctx* ctx, int n_img, int H, int W, int channels, const double* mats_host, int interpolation, int border,
                      int cval, const unsigned char* src, unsigned char* dst);
/* compute_resize_scale (host): min side -> min_side unless the max side would exceed max_side */
int pp_resize_scale(int rows, int cols, int min_side, int max_side, double* scale);
/* cv2.resize(img, None, fx = fy = scale) bilinear: dst [n_img][DH][DW][channels] with DH = round(SH * scale), DW = round(SW * scale) */
int pp_resize_linear_u8(pp_ctx* ctx, int n_img, int SH, int SW, int channels, double scale, int DH, int DW, const unsigned char* src,
                        unsigned char* dst);
/* ---- photometric augmentation of the input pipeline -----------------------------------------------------------------
 * The apply half of the imgaug chain of utils/image.py:154-191 (blur, hue / saturation / grayscale, brightness, contrast) on
 * uint8 BGR batches; the host samples one ordered op list per image and builds every table (pyrapose_amd/utils/photometric.py).
 * After every op the image is rounded to uint8 and the next op reads those bytes.  The op definitions, float32 expression
 * by expression, are in the header comment of pyrapose_amd/csrc/photo.hip; tests/photo_np.py restates them and the device
 * result is byte-identical to it.  Parity with imgaug / OpenCV is unpinned (neither is installed).
 * Offsets are byte offsets into the pool, multiples of 4.
 *   PP_PHOTO_LUT        off0: 3 x 256 bytes, one table per channel
 *   PP_PHOTO_GRAY       f0: alpha in [0,1] towards the luma
 *   PP_PHOTO_HUESAT     f0: dh (H in [0,180), wraps), f1: ds (S in [0,255], saturates); both integers
 *   PP_PHOTO_BLEND      off0: 2 x 3 x 256 bytes (first, second); off1: {int32 mh, int32 mw, float32 mask[mh][mw]}, mh, mw <= 32
 *   PP_PHOTO_CONV       k odd <= 7; off0: k x k float32 taps (correlation, reflect-101 border)
 *   PP_PHOTO_MEDIAN     k in {3,5,7} (replicate border)
 *   PP_PHOTO_BILATERAL  k odd <= 7; off0: k x k float32 space weights (0 outside the circle); off1: 766 float32 colour weights
 *                       indexed by |db|+|dg|+|dr| (reflect-101 border) */
enum { PP_PHOTO_NONE = 0, PP_PHOTO_LUT = 1, PP_PHOTO_GRAY = 2, PP_PHOTO_HUESAT = 3, PP_PHOTO_BLEND = 4, PP_PHOTO_CONV = 5, PP_PHOTO_MEDIAN = 6,
       PP_PHOTO_BILATERAL = 7 };
typedef struct pp_photo_op {
  int kind; /* PP_PHOTO_LUT .. PP_PHOTO_BILATERAL */
  int k;
  int off0, off1;
  float f0, f1;
} pp_photo_op;
/* Image n runs ops_host[op_offsets_host[n] .. op_offsets_host[n+1]) in order (at most 32; none: a copy); n_img <= 64, channels
 * must be 3.  op_offsets_host, ops_host and pool_host are HOST arrays, read during the call only (the op records travel as
 * kernel arguments); pool_dev is the caller's device copy of the same pool_bytes bytes, 16-byte aligned, uploaded in stream
 * order before the call (the upload and the lifetime of its source are the caller's, in whatever way its allocator tracks
 * them).  A malformed program (unknown op, even k, k > 7, an offset outside the pool or not a multiple of 4, a blend mask
 * larger than 32 x 32) is PP_ERR_ARG before anything is launched; the kernels take every size from the checked host copy.
 * src / dst: [n_img][H][W][3] uint8, distinct device buffers; workspace: pp_photo_workspace_bytes device bytes (the ping-pong
 * batch), 16-byte aligned.  No host synchronisation. */
size_t pp_photo_workspace_bytes(int n_img, int H, int W);
int pp_photo_augment_u8(pp_ctx* ctx, int n_img, int H, int W, int channels, const int* op_offsets_host, const pp_photo_op* ops_host,
                        const unsigned char* pool_host, size_t pool_bytes, const unsigned char* pool_dev, const unsigned char* src,
                        unsigned char* dst, void* workspace, size_t workspace_bytes);
/* The same two producers writing into a zero frame [n_img][Hp][Wp][4] with the image at (pad, pad): the input layout of
 * pp_stem7x7s2_fwd_bf16x3 (pad = 3). */
int pp_pack_rgb_to_4_padded(pp_ctx* ctx, int n_img, int H, int W, int Hp, int Wp, int pad, const float* x3, float* x4p);
int pp_preprocess_caffe_u8_padded(pp_ctx* ctx, int n_img, int H, int W, int Hp, int Wp, int pad, const int* sizes_hw_host,
                                  const unsigned char* images_u8, float* x4p);
/* keras_resnet conv1 (ZeroPadding2D(3) + Conv2D(64, 7, strides 2), models/resnet.py:87) + folded BN + ReLU on the bf16x3
 * path: x4p as above (Hp >= H + 6, Wp >= W + 8, even), weight planes [7][cout][32] (kernel row ty, column tx * 4 + c),
 * y [n_img * OH * OW][ld_y] with OH = (H - 1) / 2 + 1. */
int pp_stem7x7s2_fwd_bf16x3(pp_ctx* ctx, int n_img, int H, int W, int Hp, int Wp, const float* x4p, const void* w_hi,
                            const void* w_lo, int cout, const float* bias, int relu, float* y, int ld_y);

/* ---- head output export ---------------------------------------------------------------
 * Head convs write level-major matrices [rows][ld]; Keras concatenates the per-level reshapes on
 * axis 1 (models/retinanet.py:224-229) and applies sigmoid to cls / mask (:52, :96).
 * out[b][level_off + cell*A + a][v] = f(src[row(level,b,cell)][a*V + v]),  f = sigmoid or identity. */
int pp_export_head(pp_ctx* ctx, const pp_rowspace* rs, int n_anchor, int n_val, const float* src, int ld,
                   int apply_sigmoid, float* out);

/* ---- losses -----------------------------------------------------------------------------
 * counts[0..2] += #(state == 1) in y_true_3dbox / y_true_cls / y_true_mask (last column).
 * Normalisers of losses.py:62-66 and :402-405 (over the WHOLE batch). */
int pp_count_positives(pp_ctx* ctx, size_t rows_box, const float* y_box, size_t rows_cls, int c_cls,
                       const float* y_cls, size_t rows_mask, int c_mask, const float* y_mask, int* counts);
/* focal(alpha, gamma): losses.py:22-68 (cls and mask heads, bin/train.py:98-99).
 * logits: level-major [rows][ld] pre-sigmoid; y_true: Keras layout (B, N, C+1);
 * loss_sum += sum(focal)/normaliser; dlogits (same layout as logits, padding channels zeroed)
 * = d(loss)/d(logit) * loss_weight.  normaliser = max(1, *count).  dlogits may be NULL. */
int pp_sigmoid_focal_fwd_bwd(pp_ctx* ctx, const pp_rowspace* rs, int n_anchor, int n_class,
                             const float* logits, int ld, const float* y_true, float alpha, float gamma,
                             const int* count, float loss_weight, float* loss_sum, float* dlogits);
/* orthogonal_l1(weight .125, sigma 3): losses.py:321-408 ('3Dbox', bin/train.py:97). */
int pp_orth_smoothl1_fwd_bwd(pp_ctx* ctx, const pp_rowspace* rs, int n_anchor, const float* pred, int ld,
                             const float* y_true, float weight, float sigma, const int* count,
                             float loss_weight, float* loss_sum, float* dpred);

/* ---- optimizer: keras 2.3.1 Adam(lr, clipnorm) as compiled at bin/train.py:101 --------
 * A parameter set is a flat float32 buffer cut into tensors described by pp_param_desc. */
typedef struct {
  long long offset;      /* first element in the flat buffers */
  long long count;       /* elements (rows * ld) */
  int ld;                /* row length; scale index = element % ld */
  int trainable;         /* 0 = frozen (models/resnet.py:100-103) */
  long long scale_off;   /* offset into `scales` of the per-output-channel frozen-BN scale, or -1 */
  float l2;              /* kernel_regularizer l2 coefficient (models/retinanet.py:108), else 0 */
} pp_param_desc;

typedef struct pp_optimizer pp_optimizer;
int pp_optimizer_create(pp_ctx* ctx, pp_optimizer** out, const pp_param_desc* descs_host, int n_desc,
                        long long total);
void pp_optimizer_destroy(pp_optimizer* opt);
/* gnorm_sq[0] = sum over trainable tensors of || scale * g_eff + 2*l2*w ||^2 (fixed reduction order).
 * l2_loss (may be NULL) += sum l2 * w^2. */
int pp_grad_global_norm(pp_ctx* ctx, pp_optimizer* opt, const float* w_master, const float* g_eff,
                        const float* scales, float* gnorm_sq, float* l2_loss);
/* One Adam step with global-norm clipping (scale every gradient by clipnorm/norm when norm >= clipnorm);
 * rewrites w_eff = w_master * scale.  `step` is 1-based: lr_t = lr*sqrt(1-beta2^t)/(1-beta1^t). */
int pp_adam_step_clipnorm(pp_ctx* ctx, pp_optimizer* opt, float* w_master, float* w_eff, const float* g_eff,
                          const float* scales, float* m, float* v, const float* gnorm_sq, float lr,
                          float beta1, float beta2, float eps, float clipnorm, long long step);

/* ---- anchors / targets / decode -----------------------------------------------------------
 * utils/anchors.py:447-478 (generate_anchors) -- host, float64, bit-exact op order. */
int pp_generate_base_anchors_host(int base_size, const float* ratios_host, int n_ratios,
                                  const float* scales_host, int n_scales, double* out_host);
/* utils/anchors.py:415-444 + :372-412: all levels, float64 [N,4].  base_anchors_host: [n_levels][A][4]. */
int pp_anchors_shift_f64(pp_ctx* ctx, int n_levels, const int* feat_h_host, const int* feat_w_host,
                         const int* strides_host, int n_anchor, const double* base_anchors_host,
                         double* anchors_out);
/* layers/_misc.py:60-71 -> backend/common.py:93-116: float32 device-side anchors [N,4]. */
int pp_anchors_shift_f32(pp_ctx* ctx, int n_levels, const int* feat_h_host, const int* feat_w_host,
                         const int* strides_host, int n_anchor, const double* base_anchors_host,
                         float* anchors_out);
/* utils/compute_overlap.pyx:13-53: float64 IoU, '+1' convention, [N,K] row-major. */
int pp_compute_overlap_f64(pp_ctx* ctx, int n, const double* boxes, int k, const double* query, double* overlaps);
/* utils/anchors.py:290-318: first-max argmax + thresholds. state: 1 positive, -1 ignore, 0 background. */
int pp_compute_gt_annotations(pp_ctx* ctx, int n, const double* anchors, int k, const double* gt_boxes,
                              double negative_overlap, double positive_overlap, int* argmax, signed char* state);

/* utils/anchors.py:72-287 anchor_targets_bbox, whole batch in one call.
 * Ground truth is packed: image b owns gt_offset_host[b] .. gt_offset_host[b+1]-1.
 *   gt_boxes  [G,4] f64 (x1,y1,x2,y2);  gt_labels [G] i32;  gt_box3d [G,16] f64 projected corner
 *   pixels (anchors.py:207-215 is evaluated by pp_project_box3d_host);  gt_mask_ids [G] i32;
 *   id_masks: uint8 [B, mask_h, mask_w] object-id images, image b valid in its top-left
 *   mask_hw_host[b] = (h, w) corner (NULL = all full size);  image_hw_host [B,2] unpadded image sizes.
 * Outputs (float32, Keras layout, fully written): regression [B,N,17], labels [B,N,C+1],
 * mask [B,MH*MW,C+1] with (MH,MW) = level-3 shape of image 0. */
int pp_anchor_targets(pp_ctx* ctx, int n_anchor_total, const double* anchors, int batch,
                      const int* gt_offset_host, const double* gt_boxes, const int* gt_labels,
                      const double* gt_box3d, const int* gt_mask_ids, const unsigned char* id_masks,
                      int mask_h, int mask_w, const int* mask_hw_host, const int* image_hw_host, int num_classes,
                      double negative_overlap, double positive_overlap, int out_mh, int out_mw,
                      float* regression, float* labels, float* mask);
/* utils/anchors.py:207-215 + toPix_array :562-567 (host, float64; quat2mat = transforms3d 0.3.1). */
int pp_project_box3d_host(const double* pose7_host, const double* box8x3_host, const double* cam4_host,
                          double* out16_host);
/* PIL NEAREST index map used at anchors.py:158 (host). */
int pp_pil_nearest_index_host(int n_in, int n_out, int* out_host);

/* layers/_misc.py:195-197 -> backend/common.py:25-56: boxes3D = anchors (+) 0.2 * reg * (w|h), float32. */
int pp_box3d_decode(pp_ctx* ctx, int batch, int n, const float* anchors, const float* regression, float* boxes3d);
/* utils/linemod_eval.py:317-319: per (image, class) ascending indices with score > thr.
 * idx_out [B,C,cap] (int32, -1 padded), counts [B,C]. */
int pp_score_threshold_compact(pp_ctx* ctx, int batch, int n, int n_class, const float* scores, float thr,
                               int cap, int* idx_out, int* counts);
/* layers/filter_detections.py:21-118 (class-specific, NMS on).  boxes [N,4], boxes3d [N,16],
 * scores [N,C] for ONE image.  Outputs padded with -1 to max_det.  workspace >= pp_filter_workspace_bytes. */
size_t pp_filter_workspace_bytes(int n, int n_class, int max_det);
int pp_filter_detections(pp_ctx* ctx, int n, int n_class, const float* boxes, const float* boxes3d,
                         const float* scores, float score_thr, float iou_thr, int max_det, void* workspace,
                         float* out_boxes, float* out_boxes3d, float* out_scores, int* out_labels);
/* The same for n_img images in one set of launches (the Keras layer maps filter_detections over the batch,
 * filter_detections.py:182-196): tensors gain a leading image dimension, workspace >= n_img * pp_filter_workspace_bytes. */
int pp_filter_detections_batch(pp_ctx* ctx, int n_img, int n, int n_class, const float* boxes, const float* boxes3d,
                               const float* scores, float score_thr, float iou_thr, int max_det, void* workspace,
                               float* out_boxes, float* out_boxes3d, float* out_scores, int* out_labels);

/* ---- pose-error metrics of the evaluation tail -------------------------------------------------------
 * utils/pose_error.py:210-228 add() and :231-246 adi(), as called at utils/linemod_eval.py:525-531 (decision:
 * error < 0.1 * model diameter).  float64; n_pose (R, t) pairs against ONE model point set pts [n_pts,3];
 * R row-major [n_pose,3,3], t [n_pose,3]; out [n_pose].  workspace >= pp_pose_error_workspace_bytes. */
size_t pp_pose_error_workspace_bytes(int n_pose, int n_pts);
int pp_pose_add_f64(pp_ctx* ctx, int n_pose, int n_pts, const double* pts, const double* R_est, const double* t_est,
                    const double* R_gt, const double* t_gt, void* workspace, double* out);
int pp_pose_adi_f64(pp_ctx* ctx, int n_pose, int n_pts, const double* pts, const double* R_est, const double* t_est,
                    const double* R_gt, const double* t_gt, void* workspace, double* out);

/* ---- depth renderer and the VSD / reprojection pose errors (tless_eval.py:470-471, 651-662) -------------------------
 * Depth pass of utils/hodan_renderer.py (mode='depth', :121-143, :185-225, :548-553) as called by pose_error.py:124-128:
 * n_pose poses of ONE mesh, verts [n_vert,3] float64 (model units, the unit of t and of the output depth), faces [n_tri,3]
 * int32 (indices out of range skip the triangle), R row-major [n_pose,3,3], t [n_pose,3], K4 [n_pose,4] = (fx, fy, cx, cy)
 * float64 (skew ignored).  Out depth [n_pose,height,width] float32: camera-frame Z of the nearest surface point, interpolated
 * perspective-correctly, at pixel (r, c) sampled at (u, v) = (c + 0.5, r + 0.5); 0 = empty; fragments with Z outside
 * [clip_near, clip_far] dropped.  Deviations: a triangle with a vertex at Z <= 0 is skipped (not clipped); pixel centres on an
 * edge follow the top-left rule.  Bit-identical run to run.  workspace_bytes >= pp_render_workspace_bytes (0: bad shape). */
size_t pp_render_workspace_bytes(int n_pose, int n_vert, int n_tri, int width, int height);
int pp_render_depth_f32(pp_ctx* ctx, int n_pose, int n_vert, const double* verts, int n_tri, const int* faces, const double* R,
                        const double* t, const double* K4, int width, int height, double clip_near, double clip_far, void* workspace,
                        size_t workspace_bytes, float* depth);
/* Colour renderer: the 'rgb' / 'rgb+depth' modes of utils/hodan_renderer.py (shaders :22-103, _draw_rgb :480-518) beside the
 * depth pass above.  Mesh, poses, K4, image size and clip range as in pp_render_depth_f32; colors [n_vert,3] float64 in
 * [0, 1] (may be NULL when no colour output is asked for); normals [n_vert,3] float64, NULL allowed only with flat shading;
 * shading 0 = flat, 1 = phong; ambient_weight in [0, 1]; light_cam_pos and bg_color: HOST arrays of 3 (passed to the kernels by
 * value), the light in the OpenCV camera frame, bg_color in [0, 1].
 * Outputs, each optional (NULL = skip), at least one required:
 *   depth   [n_pose,height,width] float32: the bits pp_render_depth_f32 gives on the same inputs
 *   tri_id  [n_pose,height,width] int32: the triangle shown, -1 where there is none.  The nearest fragment wins and, among
 *           fragments of equal float32 depth, the smallest triangle index (one 64-bit key per pixel, (depth bits) << 32 | index,
 *           resolved with an integer minimum): bit-identical run to run
 *   rgb_f32 [n_pose,height,width,3] float32 and rgb_u8 [...] uint8 = rintf(rgb_f32 * 255.0f), channel order RGB.
 * Shading, float64, evaluated by the raster workgroup on its resolved tile: with the winning triangle's edge weights w_i,
 * q_i = w_i / Z_i / sum_j (w_j / Z_j) (perspective-correct) and an attribute a = (q0 a0 + q1 a1) + q2 a2; c = interpolated
 * colour; per vertex P = R p + t, N = normalize(R n), L = normalize(light - P); l = normalize(interp L); phong: n =
 * normalize(interp N) (back-facing normals are not flipped: ambient only); flat: n = normalize((P1 - P0) x (P2 - P0)), sign
 * chosen so that n . P0 < 0 (facing the viewer whatever the winding); d = max(l . n, 0) (0 for a zero-length n or l);
 * rgb = (float)(min(ambient_weight + d, 1) * c).  A pixel without a fragment holds bg_color, id -1 and depth 0.
 * Deviations from the reference: the 3-vector normal is normalised (the reference normalises u_nm * vec4(normal, 1) over four
 * components); parity with an OpenGL driver unpinned (restated: tests/render_rgb_np.py).  Textured meshes: pp_render_rgbd_tex.
 * workspace_bytes >= pp_render_rgbd_workspace_bytes (0: bad shape). */
size_t pp_render_rgbd_workspace_bytes(int n_pose, int n_vert, int n_tri, int width, int height);
int pp_render_rgbd(pp_ctx* ctx, int n_pose, int n_vert, const double* verts, const double* colors, const double* normals, int n_tri,
                   const int* faces, const double* R, const double* t, const double* K4, int width, int height, double clip_near,
                   double clip_far, int shading, double ambient_weight, const double* light_cam_pos, const double* bg_color,
                   void* workspace, size_t workspace_bytes, float* depth, int* tri_id, float* rgb_f32, unsigned char* rgb_u8);
/* Textured variant of pp_render_rgbd: the other branch of the reference's fragment shaders (hodan_renderer.py:56-57, 72-76,
 * 98-102, set up at :319-332 and :398-403), rgb = light_w * texture2D(u_texture, v_texcoord).  Everything as in pp_render_rgbd --
 * same passes, one launch of the same raster kernel text compiled with the sampler, the same depth and tri_id bits -- except that
 * the vertex colours are replaced by
 *   uv   [n_vert,2] float64 on the device, texture coordinates (not per pose: read as they are)
 *   tex  [tex_h,tex_w,4] uint8 RGBX on the device, 4-byte aligned, rows in the order of the image file (top row first); the
 *        fourth byte is ignored, a texel is one aligned 32-bit load at a 32-bit offset: tex_w, tex_h in 1 ... 16384 and
 *        tex_w * tex_h <= 2^28 (PP_ERR_SHAPE otherwise, and 0 from pp_render_rgbd_tex_workspace_bytes)
 *   filter 0 = nearest, 1 = bilinear; wrap 0 = clamp to edge, 1 = repeat.
 * A call with only depth / tri_id outputs needs neither uv nor tex (filter, wrap and the size are then not looked at when tex
 * is NULL).  Sampling rule, float64 without contraction, in exactly this order (tests/render_tex_np.py restates it):
 *   u = (q0 u0 + q1 u1) + q2 u2 and likewise v, with the perspective-correct weights q_i above;
 *   x = u * tex_w, y = v * tex_h: GL texel space.  The reference uploads np.flipud(image) and GL's t = 0 is the first uploaded
 *     row, so v = 0 is the BOTTOM row of the image file: GL texel (i, j) is tex[tex_h - 1 - j][i].  The kernel does the flip;
 *   x or y not finite (bad input only): x = y = 0.5, the centre of GL texel (0, 0) -- no index is computed from a NaN;
 *   wrap(i, n): clamp min(max(i, 0), n - 1); repeat i - n * floor(i / n) on integers, so negative coordinates wrap correctly.
 *     The floors are converted to integers after clamping them to +-2^30;
 *   nearest: texel (wrap(floor(x), tex_w), wrap(floor(y), tex_h));
 *   bilinear: xs = x - 0.5, i0 = floor(xs), fx = xs - i0, i1 = i0 + 1, both wrapped independently; the same for y (ys, j0, fy,
 *     j1); per channel, with cab = (double)byte / 255.0 of texel (ia, jb):
 *       c = ((1 - fx) * c00 + fx * c10) * (1 - fy) + ((1 - fx) * c01 + fx * c11) * fy;
 *   rgb = (float)(light_w * c), light_w = min(ambient_weight + d, 1) exactly as in pp_render_rgbd; uint8, bg_color, id -1 and
 *   depth 0 as there.
 * No mip-mapping and no anisotropic filtering: glumpy's default texture object has none, and to our reading its defaults are
 * GL_NEAREST with clamp-to-edge -- that reading is unpinned (glumpy is not at hand), as parity with an OpenGL driver is for
 * the rest of the pass.  The alpha channel is not used. */
size_t pp_render_rgbd_tex_workspace_bytes(int n_pose, int n_vert, int n_tri, int width, int height, int tex_w, int tex_h);
int pp_render_rgbd_tex(pp_ctx* ctx, int n_pose, int n_vert, const double* verts, const double* uv, const unsigned char* tex, int tex_w,
                       int tex_h, int filter, int wrap, const double* normals, int n_tri, const int* faces, const double* R,
                       const double* t, const double* K4, int width, int height, double clip_near, double clip_far, int shading,
                       double ambient_weight, const double* light_cam_pos, const double* bg_color, void* workspace,
                       size_t workspace_bytes, float* depth, int* tri_id, float* rgb_f32, unsigned char* rgb_u8);
/* vsd() of pose_error.py:105-176 (with depth_im_to_dist_im :43-61 and the visibility masks :15-40) on rendered depth images:
 * n problems, depth_est / depth_gt [n,height,width] float32, depth_test float32 (uint16 sensor depth converts exactly) at
 * depth_test + i * test_stride (0: one scene depth shared by all problems, or width * height), K4 [n,4] = (fx, fy, cx, cy)
 * float64, delta (visibility tolerance, compared in float32 as there) and tau (misalignment tolerance) in depth units,
 * cost_type 0 = 'step' (cost = |d_gt - d_est| >= tau), 1 = 'tlinear' (min(|d_gt - d_est| / tau, 1)).
 * Out e [n] float64 (1.0 when the union is empty), and, when not null, the intersection / union pixel counts [n] int64.
 * Fixed-order reductions.  workspace >= pp_vsd_workspace_bytes. */
size_t pp_vsd_workspace_bytes(int n, int width, int height);
int pp_vsd_f64(pp_ctx* ctx, int n, int width, int height, const float* depth_test, long long test_stride, const float* depth_est,
               const float* depth_gt, const double* K4, double delta, double tau, int cost_type, void* workspace, double* e,
               long long* inter, long long* uni);
/* VSD at n_tau misalignment tolerances in one pass over the pixels -- what BOP's AR_VSD needs (ten taus of 0.05 ... 0.5 x the
 * object diameter, delta = 15 mm, thresholds of correctness 0.05 ... 0.5) -- plus the counts behind the visible fraction of
 * the ground-truth object.  depth_*, test_stride, K4, delta and cost_type as in pp_vsd_f64.  taus: HOST array of n_tau
 * (1 ... 16) positive, strictly increasing tolerances in depth units, shared by the launch and passed to the kernel by value.
 * visib_mode 0: the rule of pp_vsd_f64 (the reference's estimate_visib_mask: a pixel without sensor depth is never
 * visible).  visib_mode 1: BOP 2019's rule (bop_toolkit's visibility.estimate_visib_mask with visib_mode 'bop19'; parity with
 * bop_toolkit unpinned: its definition restated, tests/vsd_bop_np.py): a model pixel is visible when d_model > 0 and
 * (float32(d_model) - float32(d_test) <= delta or d_test == 0).  In both modes the estimate's mask is then widened by
 * visib_gt && d_est > 0.  A pixel's three distances and both masks are computed once and serve every tau; the 'step' cost is
 * a histogram in integer arithmetic (a pixel of the intersection falls into the one bin that counts the taus <= |d_gt - d_est|).
 * Out e [n,n_tau] float64: (cost_t + (union - inter)) / union, 1.0 at every tau when the union is empty; column t carries the
 * bits pp_vsd_f64 returns at taus[t] in mode 0 (same blocks and summation order).  inter, uni, visib_gt (pixels in the
 * ground-truth visibility mask), px_gt (pixels with d_gt > 0): [n] int64 each, NULL = skip; visib_gt / px_gt is BOP's
 * visib_fract.  Fixed-order reductions and integer counts only: bit-identical run to run.
 * workspace >= pp_vsd_multi_workspace_bytes (0: bad shape). */
size_t pp_vsd_multi_workspace_bytes(int n, int width, int height, int n_tau);
int pp_vsd_multi_f64(pp_ctx* ctx, int n, int width, int height, const float* depth_test, long long test_stride,
                     const float* depth_est, const float* depth_gt, const double* K4, double delta, int n_tau, const double* taus,
                     int cost_type, int visib_mode, void* workspace, double* e, long long* inter, long long* uni,
                     long long* visib_gt, long long* px_gt);
/* Ground truth of n_scene scenes from the depth renders of their instances: what the training path reads besides the image.
 * depth_stack [n_inst,canvas_h,canvas_w] float32: pp_render_depth_f32 outputs (one call per distinct mesh), instances
 * scene_offsets[s] .. scene_offsets[s+1] belong to scene s (the offsets convention of pp_pnp_ransac_f64; given twice, as a
 * HOST array that is checked before anything is launched and as its device copy that the kernels read; a scene may be
 * empty and holds at most 255 instances: PP_ERR_SHAPE).  The image is the width x height window of the canvas at
 * (off_x, off_y) (PP_ERR_SHAPE unless it lies inside); K4 [n_inst,4] = (fx, fy, cx, cy) float64 in IMAGE coordinates.
 * depth_test: sensor depth float32 at depth_test + s * test_stride (0: one image shared by the scenes, or width * height)
 * with scene_depth NULL; or NULL, then scene_depth [n_scene,height,width] float32 is written -- per pixel the smallest
 * positive instance depth, 0 where there is none (a synthetic scene's depth image) -- and stands in for it.
 * Per instance, with d_gt its depth and d_test the scene's (in-image pixels only):
 *   px_count [n_inst,3] int64 = px_count_all (d_gt > 0, whole canvas), px_count_valid (in image, d_gt > 0 and d_test > 0),
 *     px_count_visib (in image, in the 'bop19' mask of pp_vsd_multi_f64 visib_mode 1, compared in float32 as there)
 *   bbox_obj [n_inst,4] int32: (x, y, w, h) of the d_gt > 0 pixels of the whole canvas in image coordinates (may be negative
 *     or reach past the image), w = x_max - x_min, h = y_max - y_min;  bbox_visib [n_inst,4]: the same of the visible mask;
 *     both are (-1, -1, -1, -1) when px_count_visib is 0
 *   mask_full / mask_visib [n_inst,height,width] uint8 0 / 255 (NULL = skip): d_gt > 0 and the visible mask.
 * The counts and boxes restate bop_toolkit's calc_gt_info and the masks its calc_gt_masks (parity with bop_toolkit unpinned:
 * the definitions restated, tests/scene_gt_np.py).  id_image [n_scene,height,width] uint8: the 1-based index within its scene
 * of the LAST instance whose visible mask holds the pixel, 0 where none does: annotation_scripts/annotate_BOP.py:363-374
 * (mask_img = np.where(obj_mask > 0, mask_id, mask_img) in instance order, later instances overwrite earlier ones).
 * Integer counts, minima and maxima only: bit-identical run to run.  workspace_bytes >= pp_scene_gt_workspace_bytes (0: bad
 * shape). */
size_t pp_scene_gt_workspace_bytes(int n_inst, int canvas_w, int canvas_h);
int pp_scene_gt_info(pp_ctx* ctx, int n_inst, int n_scene, const int* scene_offsets_host, const int* scene_offsets_dev,
                     int canvas_w, int canvas_h, int width, int height, int off_x, int off_y, const float* depth_stack,
                     const double* K4, const float* depth_test, long long test_stride, double delta, void* workspace,
                     size_t workspace_bytes, float* scene_depth, unsigned char* id_image, long long* px_count, int* bbox_obj,
                     int* bbox_visib, unsigned char* mask_full, unsigned char* mask_visib);
/* A scene's image from its instances' colour renders: id_image [n_scene,height,width] uint8 of pp_scene_gt_info (window =
 * the whole canvas), colors [n_inst,height,width,3] uint8 (pp_render_rgbd's rgb_u8 in scene order), scene_offsets as in
 * pp_scene_gt_info (same checks, same codes).  A pixel with id k > 0 takes the colour of instance scene_offsets[s] + k - 1,
 * any other pixel the background: background [n_scene,height,width,3] uint8 or, when that is NULL, the HOST constant
 * bg_const [3].  Inputs are RGB; channel_order 0 writes RGB, 1 BGR (every pixel reversed).  out [n_scene,height,width,3]
 * uint8.  Bytes are selected, never computed: byte-identical to its numpy restatement. */
int pp_scene_compose_u8(pp_ctx* ctx, int n_inst, int n_scene, const int* scene_offsets_host, const int* scene_offsets_dev, int width,
                        int height, const unsigned char* id_image, const unsigned char* colors, const unsigned char* background,
                        const unsigned char* bg_const, int channel_order, unsigned char* out);
/* reproj() of pose_error.py:179-207: mean over pts [n_pts,3] of the distance in pixels between K (R_est p + t_est) and
 * K (R_gt p + t_gt), each projection rounded to float32 and the norm taken in float32 as there (the mean is summed in float64:
 * within 1e-5 relative of the reference's float32 mean).  K9 [n_pose,3,3] row-major float64, the rest as pp_pose_add_f64;
 * out [n_pose] pixels.  workspace >= pp_pose_error_workspace_bytes(n_pose, n_pts). */
int pp_pose_reproj_f64(pp_ctx* ctx, int n_pose, int n_pts, const double* pts, const double* K9, const double* R_est,
                       const double* t_est, const double* R_gt, const double* t_gt, void* workspace, double* out);

/* ---- BOP's symmetry-aware pose errors MSSD / MSPD (csrc/pose.hip) ---------------------------------------------------
 * bop_toolkit's pose_error.mssd / mspd (parity with bop_toolkit unpinned: its definition restated, tests/pose_sym_np.py) for
 * n_pose pose pairs of ONE model pts [n_pts,3] and one symmetry set shared by the launch: S_R [n_sym,3,3] row-major, S_t
 * [n_sym,3] (utils/symmetry.py: get_symmetry_transformations, identity first).  With G_s = (R_gt S_R[s], R_gt S_t[s] + t_gt):
 *   MSSD = min_s max_i || (R_est p_i + t_est) - (G_s.R p_i + G_s.t) ||                         (unit of pts and t)
 *   MSPD = min_s max_i || proj(K, R_est, t_est, p_i) - proj(K, G_s.R, G_s.t, p_i) ||           (pixels, K9 [n_pose,3,3])
 * float64 throughout (the projection is the one of pp_pose_reproj_f64 without its rounding to float32).  out [n_pose];
 * best_sym [n_pose] int32 (NULL = skip): the symmetry that attains the minimum, the lowest index on ties.  Maxima and minima
 * only: bit-identical run to run.  n_pose <= 65535, n_sym <= 8 * 65535.  workspace >= pp_pose_sym_workspace_bytes. */
size_t pp_pose_sym_workspace_bytes(int n_pose, int n_pts, int n_sym);
int pp_pose_mssd_f64(pp_ctx* ctx, int n_pose, int n_pts, int n_sym, const double* pts, const double* S_R, const double* S_t,
                     const double* R_est, const double* t_est, const double* R_gt, const double* t_gt, void* workspace, double* out,
                     int* best_sym);
int pp_pose_mspd_f64(pp_ctx* ctx, int n_pose, int n_pts, int n_sym, const double* pts, const double* S_R, const double* S_t,
                     const double* K9, const double* R_est, const double* t_est, const double* R_gt, const double* t_gt,
                     void* workspace, double* out, int* best_sym);

/* ---- RANSAC-PnP of the evaluation tail ----------------------------------------------------------------
 * In place of cv2.solvePnPRansac(obj_points, est_points, K, None, iterationsCount=300, reprojectionError=5.0,
 * confidence=0.99, flags=cv2.SOLVEPNP_ITERATIVE) + cv2.Rodrigues at utils/linemod_eval.py:479-485 (same call in the
 * other *_eval.py): n_problems independent problems (one per detected class and image) in one launch; problem p owns
 * the correspondences offsets[p] .. offsets[p+1] (device int array) of obj [N,3] / img [N,2] (float64, pixels) and the
 * intrinsics K4[p] = (fx, fy, cx, cy).  points_per_vote = 8 for the reference's layout (k votes x the 8 cuboid corners,
 * linemod_eval.py:421-431): a hypothesis then takes six distinct corners, each from a random vote; 0 = unstructured.
 * Out: R [P,3,3] row-major (what cv2.Rodrigues(rvec) returns), t [P,3], n_inliers [P], inlier_mask [N] (1 = squared
 * reprojection error < reproj_error^2), ok [P] (0: fewer than 4 inliers / no valid sample; R = I, t = 0 then).
 * Deterministic for a given seed (counter-based draws, fixed-order reductions).  OpenCV is not in the reference tree:
 * the estimator is this library's own (csrc/pnp.hip, restated in oracle/pnp_np.py) -- parity with cv2 is unpinned.
 * workspace >= pp_pnp_ransac_workspace_bytes.  All iterations are run (no confidence-based early exit). */
size_t pp_pnp_ransac_workspace_bytes(int n_problems, int iterations);
int pp_pnp_ransac_f64(pp_ctx* ctx, int n_problems, const int* offsets_dev, int n_points_total, const double* obj,
                      const double* img, const double* K4, int iterations, double reproj_error, unsigned long long seed,
                      int points_per_vote, void* workspace, double* R_out, double* t_out, int* n_inliers,
                      unsigned char* inlier_mask, int* ok);

/* ---- ICP refinement of estimated poses against scene depth (csrc/icp.hip) -------------------------------------------
 * The block of PyraPose_ROS_wrapper/scripts/pyrapose_node.py:run_estimation (:662-756; the same block at
 * utils/ycbv_eval.py:424-526, 812-896 and the get_evaluation* helpers of tless_eval.py:23-65), which runs on the CPU through
 * Open3D / OpenCV there.  float64 throughout, fixed-order reductions: every result is bitwise independent of the batch it runs
 * in and of the run. */
#define PP_ICP_POINT_TO_POINT 0
#define PP_ICP_POINT_TO_PLANE 1
#define PP_ICP_OK 0
#define PP_ICP_TOO_FEW 1   /* fewer than 6 (plane) / 3 (point) correspondences: the last pose is kept */
#define PP_ICP_SINGULAR 2  /* the update's linear system is singular: the last pose is kept */
/* create_point_cloud (pyrapose_node.py:170-189) with the class mask of :602-604 applied.  depth float32 [height,width]
 * (device); point (r, c) = (((c - cx) z) / fx, ((r - cy) z) / fy, z) with z = depth * ds in float64.
 * dense != 0: every pixel at index r * width + c of pts [height*width,3], an all-NaN row where z == 0 (as :186); mask,
 * workspace and row_offsets unused.  dense == 0: only pixels with a finite, non-zero z whose mask cell
 * mask[row_idx[r] * mask_w + col_idx[c]] (uint8 [mask_h,mask_w], NULL = no mask; row_idx / col_idx from
 * pp_pil_nearest_index_host, device int32) is non-zero, compacted in row-major pixel order (count per row, scan, scatter);
 * row_offsets [height+1] (device) gets each row's first output index and the total.
 * workspace >= pp_cloud_from_depth_workspace_bytes. */
size_t pp_cloud_from_depth_workspace_bytes(int height, int width);
int pp_cloud_from_depth_f64(pp_ctx* ctx, int height, int width, const float* depth, const unsigned char* mask, int mask_h, int mask_w,
                            const int* row_idx, const int* col_idx, double fx, double fy, double cx, double cy, double ds, int dense,
                            void* workspace, double* pts, int* row_offsets);
/* Open3D voxel_down_sample (pyrapose_node.py:679-680), in two device steps around a stable sort of the keys by the caller:
 * pp_voxel_keys_f64: keys [n] int64 of floor((p - (min_bound - voxel/2)) / voxel) per axis packed as ix << 42 | iy << 21 | iz
 * (-1 when an index leaves [0, 2^21)); workspace >= pp_voxel_workspace_bytes (holds min_bound).
 * pp_voxel_means_f64: perm [n] int64 (the stable sort order of the keys), seg [n_vox+1] int64 (the first sorted position of
 * each distinct key and n): out_pts [n_vox,3] the mean of each voxel's points summed in original point order; normals
 * (optional) are summed the same way and renormalised into out_normals (0 when they cancel).  Output order = ascending key
 * (Open3D's hash order is not reproducible). */
size_t pp_voxel_workspace_bytes(int n);
int pp_voxel_keys_f64(pp_ctx* ctx, int n, const double* pts, double voxel, void* workspace, long long* keys);
int pp_voxel_means_f64(pp_ctx* ctx, int n, const double* pts, const double* normals, const long long* perm, int n_vox,
                       const long long* seg, double* out_pts, double* out_normals);
/* Open3D estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) (pyrapose_node.py:681-682, 694, 731): per point the
 * max_nn (<= 32) nearest points within radius (itself included, |d|^2 <= radius^2, equal distances to the lower index), the
 * float64 covariance about their mean, the eigenvector of its smallest eigenvalue (6 cyclic Jacobi sweeps), oriented toward
 * the camera at the origin (n . p <= 0).  Fewer than 3 neighbours: zero normal.  normals [n,3]; neighbors (optional)
 * [n,max_nn] int32, nearest first, -1 padded.  workspace >= pp_estimate_normals_workspace_bytes (0 today). */
size_t pp_estimate_normals_workspace_bytes(int n, int max_nn);
int pp_estimate_normals_f64(pp_ctx* ctx, int n, const double* pts, double radius, int max_nn, void* workspace, double* normals,
                            int* neighbors);
/* Open3D registration_icp (pyrapose_node.py:734-735, tless_eval.py:23-65) for n_problems independent problems: problem p owns
 * source points src_offsets[p] .. src_offsets[p+1] and target points tgt_offsets[p] .. (device int32 offsets into src / tgt
 * [.,3]); max_source_points >= the largest source count; init [P,4,4] row-major.  Per pass: each source point under the
 * current pose takes its nearest target (strict <, lowest index wins; in point-to-plane mode targets with a zero normal are
 * skipped) when |d| <= max_correspondence_distance; fitness = n_corr / n_source, inlier_rmse = sqrt(SSE / n_corr) (0 without
 * correspondences).  Update: point-to-plane (Open3D's linearisation: J = [(s x n)^T, n^T], r = (s - q) . n, JTJ x = -JTr by
 * LDL^T, R = Rz(x2) Ry(x1) Rx(x0), t = x[3:]) or point-to-point (Kabsch without scale, proper rotation), applied on the left.
 * Stop when |d fitness| < relative_fitness and |d rmse| < relative_rmse against the previous pass, or after max_iteration
 * updates.  Out: R [P,3,3], t [P,3], fitness, inlier_rmse [P] at the final pose, iterations [P] (updates applied),
 * status [P] (PP_ICP_*), corr [n_source_total] the target index (relative to tgt_offsets[p]) of each source point's
 * correspondence at the final pose, -1 for none (left untouched for a problem without source or target points).
 * workspace_bytes >= pp_icp_workspace_bytes. */
size_t pp_icp_workspace_bytes(int n_problems, int max_source_points);
int pp_icp_f64(pp_ctx* ctx, int n_problems, const int* src_offsets, const int* tgt_offsets, int max_source_points, const double* src,
               const double* tgt, const double* tgt_normals, const double* init, double max_correspondence_distance, int max_iteration,
               double relative_fitness, double relative_rmse, int mode, void* workspace, size_t workspace_bytes, double* R_out,
               double* t_out, double* fitness, double* inlier_rmse, int* iterations, int* status, int* corr);

/* ---- uncertainty-weighted PnP refinement of voted poses (csrc/wpnp.hip) ---------------------------------------------
 * The reference's uncertainty_pnp/ (src/uncertainty_pnp.cpp:7-92, a Ceres problem; wrapped by un_pnp_utils.py:6-121 and
 * prepared, switched off, at utils/linemod_eval.py:488-496 and utils/occlusion_eval.py:493), batched on the device.  Ceres,
 * glog, SuiteSparse, cffi and cv2 are not in the reference tree: the minimiser is this library's own Levenberg-Marquardt
 * (header comment of csrc/wpnp.hip, restated in tests/wpnp_np.py) -- parity with Ceres is unpinned.  Pinned: the cost function
 * (the functor of uncertainty_pnp.cpp:17-33) and its minimum.  float64, fixed-order reductions: every result is bitwise
 * independent of the batch it runs in and of the run. */
#define PP_WPNP_FULL 0       /* W = (cov / n_eff + sigma_floor^2 I)^(-1/2): whitening by the covariance of the mean */
#define PP_WPNP_ISO 1        /* un_pnp_utils.py:75-83, 103-104: wxx = wyy = 1 / lambda_max(cov), wxy = 0; 0 where cov_xx < 1e-5 */
#define PP_WPNP_CONVERGED 0
#define PP_WPNP_MAX_ITER 1
#define PP_WPNP_TOO_FEW 2    /* fewer than 3 correspondences with a non-zero weight: the start pose is returned */
#define PP_WPNP_SINGULAR 3   /* a pivot of the damped 6x6 system is not positive and finite: the start pose is returned */
#define PP_WPNP_BEHIND 4     /* a weighted point behind the camera at the start: the start pose is returned */
/* From votes to per-corner statistics.  Problem p owns the correspondences offsets[p] .. offsets[p+1] (device int32, multiples
 * of points_per_vote) of img [N,2], laid out as k_p votes x points_per_vote corners (linemod_eval.py:421-431).  vote_weight
 * [N / points_per_vote] (the class score of each vote; NULL = 1; votes with a weight <= 0 are left out), inlier_mask [N] uint8
 * (what pp_pnp_ransac_f64 returns; NULL = all).  Per problem and corner, over the votes left in: wsum [P,ppv], count [P,ppv]
 * (int32), the weighted mean mu [P,ppv,2], the weighted population covariance about it cov [P,ppv,3] = (xx, xy, yy) (two
 * passes), n_eff = (sum w)^2 / sum w^2, and wgt [P,ppv,3] = (wxx, wxy, wyy) by `mode` (PP_WPNP_FULL takes sigma_floor, pixels;
 * lambda_min <= 0, possible only with sigma_floor = 0, gives W = 0).  count < 2: W = 0; count = 0: every output 0.
 * Deviation: the reference has no such step on the device -- it aggregates votes in numpy where it does at all.
 * workspace >= pp_vote_stats_workspace_bytes (0 today). */
size_t pp_vote_stats_workspace_bytes(int n_problems, int points_per_vote);
int pp_vote_stats_f64(pp_ctx* ctx, int n_problems, const int* offsets_dev, int n_points_total, const double* img,
                      int points_per_vote, const double* vote_weight, const unsigned char* inlier_mask, int mode,
                      double sigma_floor, void* workspace, double* wsum, int* count, double* mu, double* cov, double* n_eff,
                      double* wgt);
/* uncertainty_pnp() of uncertainty_pnp.cpp:61-92 for n_problems independent problems in one call: problem p owns the
 * correspondences offsets[p] .. offsets[p+1] of obj [N,3], img [N,2], wgt [N,3] = (wxx, wxy, wyy); K4 [P,4] = (fx, fy, cx,
 * cy); start R_init [P,3,3] row-major, t_init [P,3] (device; the kernel takes the rotation's logarithm).  Cost: 1/2 sum |W (proj(
 * Rodrigues(w) x + t) - u)|^2 over the correspondences with a non-zero weight, parameters (w, t) as there.  Minimiser:
 * Levenberg-Marquardt with Marquardt scaling (diagonal clamped to [1e-6, 1e32], lambda0 = 1e-4, step accepted when the gain ratio
 * exceeds 1e-3: Ceres' defaults), lambda by Nielsen's rule; a trial pose with a weighted point at p_z <= 0 is rejected.  Stops on
 * max |g| < gradient_tol, |delta| <= parameter_tol (|x| + parameter_tol), cost decrease <= function_tol * cost, or after
 * max_iterations trial poses (Ceres' defaults: 1e-10, 1e-8, 1e-6, 50).  Deviations: Ceres' DENSE_SCHUR / trust-region bookkeeping
 * is not reproduced (same minimum, other iterates); the seed pose is an argument, not cv2.solvePnP(P3P).
 * Out: R [P,3,3], t [P,3], rvec [P,3]; cost_init, cost_final [P] (cost_final <= cost_init exactly); iterations [P] (passes over
 * the correspondences); status [P] (PP_WPNP_*); pose_cov [P,6,6] (NULL = skip) = (J^T J)^-1 at the final pose in (w, t) order,
 * zeros when not invertible or when the start pose is returned.  Problems of at most 64 correspondences run one per wave,
 * larger ones one per workgroup; the choice depends on the problem alone.
 * workspace >= pp_pnp_refine_weighted_workspace_bytes (0 today). */
size_t pp_pnp_refine_weighted_workspace_bytes(int n_problems, int n_points_total);
int pp_pnp_refine_weighted_f64(pp_ctx* ctx, int n_problems, const int* offsets_dev, int n_points_total, const double* obj,
                               const double* img, const double* wgt, const double* K4, const double* R_init, const double* t_init,
                               int max_iterations, double gradient_tol, double parameter_tol, double function_tol, void* workspace,
                               double* R_out, double* t_out, double* rvec_out, double* cost_init, double* cost_final,
                               int* iterations, int* status, double* pose_cov);

/* ---- clustering of each class's votes into object instances (csrc/cluster.hip) --------------------------------------
 * Replaces nothing in the reference -- a stated deviation: the reference pools every vote of a class into one RANSAC problem
 * and scores it against the first annotation of that class, because "occurences of 2 or more instances not possible in
 * LINEMOD" (utils/tless_eval.py:378); T-LESS scenes do hold several instances of one object.  This step, the library's own,
 * decides which votes form a problem; everything after it is already batched over problems (pp_pnp_ransac_f64, ...).
 * One workgroup per (image, class), directly on the outputs of pp_score_threshold_compact: boxes3d [B,N,16], scores [B,N,C]
 * float32, idx [B,C,cap] (ascending anchors, -1 padded), counts [B,C] (values above cap count as cap).
 *   vote box: axis-aligned box of the vote's 8 corners, float32 min / max.  A vote with a non-finite corner (or an anchor
 *     outside [0, n)) is invalid: it never leads, never joins, instance -1.
 *   IoU: float64 on the float32 boxes, no "+1": w = max(0, min(x2a,x2b) - max(x1a,x1b)), h likewise, inter = w h,
 *     ua = (x2a-x1a)(y2a-y1a) + (x2b-x1b)(y2b-y1b) - inter, iou = inter / ua if ua > 0 else 0; every product and sum
 *     rounded on its own (no FMA contraction), as numpy does it.
 *   rounds: the leader is the unassigned valid vote with the highest class score (float32 compare, ties -> lowest anchor);
 *     its members are the leader and every unassigned valid vote with iou(leader, vote) > iou_thr; members are consumed
 *     whether or not the cluster is kept; a cluster of at least min_votes members is kept and gets the next instance id
 *     (dense from 0 in order of creation), a smaller one is dropped (-1).  Stops when nothing valid is unassigned, when
 *     max_instances clusters are kept, or after max_rounds leaders; what is still unassigned gets -1.
 * Out: inst [B,C,cap] int32 instance id per input vote (-1: padding, dropped, invalid); order [B,C,cap] the anchor indices of
 * the kept votes, instance-major and ascending within an instance, -1 padded; inst_offsets [B,C,max_instances+1] into order
 * (entries past n_inst repeat the total); n_inst [B,C]; leader [B,C,max_instances] anchor index (-1 unused); inst_box
 * [B,C,max_instances,4] float32 (x1, y1, x2, y2) of the leader's vote box (0 unused).  Integer reductions in a fixed order:
 * bit-identical run to run and independent of the batch a problem sits in.  Any count up to cap works (boxes beyond the LDS
 * cache are recomputed from boxes3d); an empty (image, class) costs one workgroup that exits at once.
 * Errors: null pointers, batch / n / n_class / cap / min_votes / max_instances / max_rounds < 1, iou_thr outside [0, 1):
 * PP_ERR_ARG.  workspace >= pp_vote_cluster_workspace_bytes (0 today: workspace may be NULL). */
size_t pp_vote_cluster_workspace_bytes(int batch, int n_class, int cap, int max_instances);
int pp_vote_cluster(pp_ctx* ctx, int batch, int n, int n_class, int cap, const float* boxes3d, const float* scores,
                    const int* idx, const int* counts, double iou_thr, int min_votes, int max_instances, int max_rounds,
                    void* workspace, int* inst, int* order, int* inst_offsets, int* n_inst, int* leader, float* inst_box);

/* ---- model geometry: diameter and farthest-point control points (csrc/model_info.hip) ------------------------------------
 * What the evaluation tail takes as given from a dataset's models_info.json (the 'diameter' the ADD decision and VSD's taus
 * scale with) and from the reference's offline FPS.py (features.json), computed from the model's points.  float64; with
 *   d2(a, b) = (dx dx + dy dy) + dz dz        in exactly that association, every product and sum rounded on its own
 * (numpy's (diff * diff).sum(axis=1) on rows of three).  Parity with bop_toolkit's misc.calc_pts_diameter and with a run of
 * FPS.py is unpinned: both definitions restated, tests/model_info_np.py.
 *
 * pp_pts_diameter_f64: pts [n,3], 1 <= n <= 2^24 (PP_ERR_SHAPE otherwise).
 *   d2 [1]   = max over i <= j of d2(p_i, p_j); the diameter is its square root, taken on the host (math.sqrt, as
 *              calc_pts_diameter does after its .max()), so the device result is a maximum of exactly rounded sums
 *   pair [2] = int32 (i, j), i <= j, a pair that attains it: the lowest i, then the lowest j.  n = 1: d2 = 0, pair (0, 0).
 *   Points past n take no part (a partial tile's tail is not a set of zero points).  Maxima only: bit-identical run to run.
 *   workspace_bytes >= pp_pts_diameter_workspace_bytes(n) (0: bad n), workspace not NULL: PP_ERR_ARG otherwise.
 *
 * pp_farthest_points_f64: greedy farthest-point sampling of k points from each of n_model point sets in ONE launch (one
 *   workgroup per model).  pts [n_total,3]: the sets concatenated; offsets [n_model+1] int32 from 0 to n_total, given twice
 *   as pp_scene_gt_info's scene_offsets are: the HOST copy is checked before anything is launched, the kernel reads the
 *   device copy.  start [n_model] int32 (device): each model's first pick (clamped into the model), or NULL: the first
 *   maximum of (x x + y y) + z z (FPS.py:40-42, argmax of the norm restated on squares).  Then k - 1 times: update every
 *   point's running score against the point chosen last, pick the first maximum (np.argmax: the lowest index on ties).
 *     rule 0 ("min"): score_i = min over the chosen c of d2(p_i, p_c); no square root is taken.  k <= every model's size.
 *     rule 1 ("sum"): FPS.py:62-94.  score_i = sum over the chosen c, added in the order chosen, of sqrt(d2(p_i, q_c)), q_c
 *       being p_c ROUNDED TO FLOAT32 (control_points is a float32 array, :37, :83-84); the score counts as 0.0 if any
 *       sqrt(d2(p_i, q_c)) < min_dist[model] (float64 [n_model], device; FPS.py:55-59 passes (x_dim + y_dim + z_dim) / 7).
 *       When every score is 0 the pick is index 0.  k may exceed a model's size.
 *   index [n_model,k] int32: the picks as indices WITHIN their model.  Fixed order: bit-identical run to run.
 *   Errors before anything is launched: n_model, n_total or k < 1, an empty model, k > a model's size under rule 0:
 *   PP_ERR_SHAPE; null pointers (min_dist may be NULL under rule 0), rule outside {0, 1}, offsets that decrease or do not run
 *   from 0 to n_total, workspace_bytes < pp_farthest_points_workspace_bytes(n_total): PP_ERR_ARG.
 *
 * pp_sym_hausdorff_f64: how far each of n_cand rigid transformations moves a point set off a target set -- the score behind
 *   utils.model_info.find_symmetries / symmetry_residuals (the 'symmetries_discrete' / 'symmetries_continuous' entries of
 *   models_info).  src [n_src,3], tgt [n_tgt,3] (may be the same pointer), S_R [n_cand,3,3] row-major, S_t [n_cand,3]; for
 *   every candidate k
 *     d2 [k]     = max over i of min over j of d2(S_k src_i, tgt_j), the SQUARED one-sided Hausdorff distance of the moved
 *                  source to the target; S_k p = R[0] x + R[1] y + R[2] z + t[0] (and rows 1, 2), summed left to right as the
 *                  pose errors move a point; the root is the host's
 *     arg [k,2]  = int32 (i, j): the lowest i that attains the maximum, and for that i the lowest j that attains its minimum.
 *   Points past n_src / n_tgt take no part (a partial tile's tail is not a set of zero points).  Maxima and minima only, no
 *   float atomics: bit-identical to the numpy restatement (tests/model_sym_np.py) and run to run.  All n_cand n_src n_tgt pairs
 *   are visited in one launch plus one finish launch.  Inputs must be finite.
 *   Errors before anything is launched: n_src or n_tgt outside 1..2^24, n_cand outside 1..65535: PP_ERR_SHAPE; null pointers,
 *   workspace_bytes < pp_sym_hausdorff_workspace_bytes(n_src, n_cand) (0: bad n_src or n_cand): PP_ERR_ARG.
 *   Parity with any dataset's hand-annotated symmetries is unpinned: no dataset was at hand. */
size_t pp_sym_hausdorff_workspace_bytes(int n_src, int n_cand);
int pp_sym_hausdorff_f64(pp_ctx* ctx, int n_src, const double* src, int n_tgt, const double* tgt, int n_cand, const double* S_R,
                         const double* S_t, void* workspace, size_t workspace_bytes, double* d2, int* arg);
size_t pp_pts_diameter_workspace_bytes(int n);
int pp_pts_diameter_f64(pp_ctx* ctx, int n, const double* pts, void* workspace, size_t workspace_bytes, double* d2, int* pair);
size_t pp_farthest_points_workspace_bytes(int n_total);
int pp_farthest_points_f64(pp_ctx* ctx, int n_model, int n_total, const double* pts, const int* offsets_host, const int* offsets_dev,
                           int k, int rule, const double* min_dist, const int* start, void* workspace, size_t workspace_bytes,
                           int* index);

/* ---- mesh geometry: face normals, area, volume, vertex normals, surface samples (csrc/mesh.hip) --------------------------
 * What a mesh that brings no normals and too few vertices to stand for its surface needs before it can be rendered with phong
 * shading or measured by the point-set metrics.  float64; every product and sum rounded on its own; squared lengths and dot
 * products associate as (x x' + y y') + z z'.  The reference computes none of this and no library that does was at hand: the
 * rules are this project's, restated in tests/mesh_np.py, which every output is bit-identical to, as it is from run to run
 * ("restated, unpinned").  No float atomics; integer atomics never decide a result.  Inputs must be finite.
 * Common to the three: pts [n_v,3], faces [n_f,3] int32, 1 <= n_v, n_f <= 2^22 and 1 <= n_samples <= 2^24 (PP_ERR_SHAPE
 * otherwise); null pointers (but those named optional) and a workspace shorter than the entry point's *_workspace_bytes (0: a
 * refused size) are PP_ERR_ARG; both are checked before anything is launched.  No host synchronisation, no workgroup waits on
 * another, every loop is bounded by the sizes.  A face that names a vertex outside 0..n_v-1 counts as degenerate everywhere:
 * zero normal, zero area, in no adjacency list, never sampled; its points are never read.
 *
 * pp_mesh_face_geometry_f64:
 *   normal [n_f,3] = (p1 - p0) x (p2 - p0), not normalised; area2 [n_f] = its length by sqrt, twice the face's area
 *   totals [8]     = {sum area2, sum p0 . normal (six times the signed volume), sum area2 (p0 + p1 + p2) [3] (the numerator
 *                    of the area-weighted centroid: divide by 3 totals[0]), max area2 (exact), 0, 0}
 *                    The sums run in one fixed order: chunks of 256 faces in face order, each by the halving tree of the VSD
 *                    tile sums (lane t += lane t + 128, + 64, ... + 1; a missing face adds +0.0), then the chunks in order.
 *   status [1]     = int32: bit 0 a face names a vertex out of range, bit 1 every area is zero
 *
 * pp_mesh_vertex_normals_f64: face_normal and totals as pp_mesh_face_geometry_f64 wrote them for the same mesh.
 *   vnormal [n_v,3]     = the sum of the normals of the vertex's incident faces, added one by one in ascending face index (a
 *                         face that lists the vertex twice is added twice), divided by the sum's length; (0,0,0) for a zero
 *                         sum.  Area weighting: the normals are not normalised first.  outward != 0: every normal is negated
 *                         when totals[1] < 0 (inward winding); the sign is read on the device.
 *   adj_offsets [n_v+1] = int32, CSR: the faces of vertex v are adj_faces[adj_offsets[v] .. adj_offsets[v+1])
 *   adj_faces [3 n_f]   = int32, ascending within each vertex; entries past adj_offsets[n_v] are -1
 *   The ascending order is reached by ranking each segment after an atomic fill: cost sum over the vertices of valence^2,
 *   spread over valence lanes each; the result does not depend on the order the atomics land in.
 *
 * pp_mesh_sample_surface_f64: n_samples points uniform by area.  face_normal, area2, totals as above.
 *   q_f = floor(ldexp(area2_f, 39 - ilogb(totals[5]))), so the largest lies in [2^39, 2^40); cum = the inclusive integer scan.
 *   Sample i: word(j) = splitmix64(splitmix64(4 seed + j) + i) mod 2^64; u = word(0) in mode 0; in mode 1 the Weyl sequence
 *   u = splitmix64(4 seed + 3) + i 0x9E3779B97F4A7C15 mod 2^64 (low discrepancy over the area).  The face is the first f with
 *   cum[f] > high 64 bits of u * cum[n_f-1].  A face with q_f = 0 -- one that covers less than 2^-39 of the largest face -- is
 *   never chosen: that is the rule.  r1, r2 = (word(1) >> 11) 2^-53, (word(2) >> 11) 2^-53; s = sqrt(r1); a = 1 - s,
 *   b = s (1 - r2), c = s r2.
 *   Outputs, each skipped when NULL:
 *     points [n,3]        = (a p0 + b p1) + c p2 per coordinate
 *     face [n]            = int32
 *     bary [n,3]          = (a, b, c)
 *     normals [n,3]       = the face's normal / area2, negated when outward != 0 and totals[1] < 0
 *     attr_out [n,n_attr] = the same blend of the rows of attr [n_v,n_attr], 1 <= n_attr <= 8 (PP_ERR_SHAPE otherwise; attr
 *                           must not be NULL then); n_attr is not looked at when attr_out is NULL
 *   When every area is zero (status bit 1) every output is zero and face is -1.  mode other than 0 or 1: PP_ERR_ARG. */
size_t pp_mesh_face_geometry_workspace_bytes(int n_f);
int pp_mesh_face_geometry_f64(pp_ctx* ctx, int n_v, int n_f, const double* pts, const int* faces, void* workspace,
                              size_t workspace_bytes, double* normal, double* area2, double* totals, int* status);
size_t pp_mesh_vertex_normals_workspace_bytes(int n_v, int n_f);
int pp_mesh_vertex_normals_f64(pp_ctx* ctx, int n_v, int n_f, const int* faces, const double* face_normal, const double* totals,
                               int outward, void* workspace, size_t workspace_bytes, double* vnormal, int* adj_offsets,
                               int* adj_faces);
size_t pp_mesh_sample_surface_workspace_bytes(int n_f);
int pp_mesh_sample_surface_f64(pp_ctx* ctx, int n_v, int n_f, const double* pts, const int* faces, const double* face_normal,
                               const double* area2, const double* totals, int n_samples, unsigned long long seed, int mode,
                               int outward, int n_attr, const double* attr, void* workspace, size_t workspace_bytes,
                               double* points, int* face, double* bary, double* normals, double* attr_out);

/* ---- 2-D detection average precision (csrc/det_eval.hip) -----------------------------------------------------------------
 * utils/eval.py:147-235 (evaluate, the 'mAP' of callbacks/eval.py) and BOP's detection score (COCO AP with ignored ground
 * truth) on the device: greedy matching per image, then true / false positive scans, precision envelope and the integral per
 * (threshold, class).  float64, every product, quotient and sum rounded on its own; no atomics: bit-identical run to run and
 * independent of the batch an image sits in.  The reference rule is pinned to the reference's evaluate through
 * tests/golden/detection_ap.npz; the COCO rule and the 101-point integration restate pycocotools (cocoeval.py evaluateImg /
 * accumulate) and their parity with it is unpinned.  All of it is restated in tests/det_eval_np.py.
 *
 * pp_det_match: detections of `batch` images against their ground truth, at n_thr IoU thresholds in one launch.
 *   in   det_boxes [B,D,4] (x1, y1, x2, y2), det_scores [B,D] float64, det_labels [B,D] int32 -- the layout
 *        pp_filter_detections_batch writes, widened to float64.  A slot whose label is outside [0, n_class) is padding (-1 is
 *        what the filter writes); padding may sit anywhere in a row.  Scores must not be NaN, boxes must be finite.
 *        gt_boxes [G,4] float64, gt_labels [G] int32, gt_ignore [G] uint8 or NULL (none ignored), gt_offsets [B+1] int32 from 0
 *        to G, given twice as pp_farthest_points_f64's are: the HOST copy is checked before anything is launched, the kernel
 *        reads the device copy.  A ground truth whose label is outside [0, n_class) matches nothing and is not counted.
 *        thresholds [n_thr] float64 on the HOST, strictly increasing within [0, 1].
 *   out  match [T,B,D] int32: the global ground-truth index (into gt_boxes) the detection is matched to, or -1
 *        det_ignored [T,B,D] uint8: 1 for a detection that counts neither as true nor as false positive
 *        npos [n_class] int32: ground truth per class over the whole batch, the ignored ones left out
 *   Detections of an image are visited in descending score, equal scores (float compare: -0 == +0) by the lower slot.
 *   rule PP_DET_RULE_REFERENCE (utils/eval.py:187-211):
 *     IoU of pp_compute_overlap_f64 (the "+1" convention; the same device function, detection as `boxes` row, ground truth as
 *     `query` row).  A detection looks at EVERY ground truth of its own label in its image, taken or not, and picks the first
 *     maximum (np.argmax: the lowest index on ties).  It is a true positive (match = that index) iff that maximum is >= the
 *     threshold and that ground truth has not been taken; otherwise a false positive (-1) -- no fall-back to the second best.
 *     No ground truth of its label: false positive.  det_ignored is all 0; gt_ignore must be NULL (PP_ERR_ARG).
 *   rule PP_DET_RULE_COCO (pycocotools evaluateImg without crowd and area ranges):
 *     IoU = i / (area_d + area_g - i), i = w h of the intersection, areas (x2 - x1)(y2 - y1), no "+1"; 0 unless w > 0 and h > 0.
 *     Ground truth of the detection's label is visited not-ignored first, then ignored, each in input order; taken ones are
 *     skipped.  The detection takes the one with the highest IoU >= min(threshold, 1 - 1e-10); among equal IoUs the LATER one in
 *     visiting order; the search stops at the first ignored ground truth once a not-ignored match is held, so an ignored one is
 *     taken only when no not-ignored one qualifies.  A matched ground truth is consumed, ignored or not; a detection matched
 *     to an ignored one has det_ignored = 1.  Unmatched: match -1, det_ignored 0 (a false positive).
 *   Layout: one workgroup per image, one wave per threshold.  The score order is computed once per workgroup by rank
 *   counting in LDS; a wave's lanes stride over the image's ground truth (held in LDS), each lane owning the taken flags
 *   (LDS, per threshold) of its own ground truth; a 64-lane butterfly under the rule's tie-break picks the match.
 *   Limits (PP_ERR_ARG before anything is launched): 1 <= n_thr <= PP_DET_MAX_THR; 0 <= D <= PP_DET_MAX_DET; at most
 *   PP_DET_MAX_GT ground truths in one image; offsets that decrease or do not run from 0 to G; batch, n_class < 1;
 *   T * B * D >= 2^31; thresholds not increasing or outside [0, 1]; unknown rule; null pointers (D = 0: the detection tensors
 *   and outputs may be NULL and only npos is written).  Labels live on the device and are not looked at by this entry point:
 *   the Python wrapper (ops.det_match) refuses labels >= n_class; here they are padding as said above.
 *
 * pp_det_pr_curve: the curves of every (threshold, class) over the detections of all images in one global order.
 *   in   order [N] int32: flat slots b * D + d of the non-padding detections, class-major; class_offsets [n_class+1] int32
 *        (device) into it; within a class the caller's order stands (ops.det_order: descending score, then ascending slot).
 *        match, det_ignored [T,n_slots] and npos [n_class] as pp_det_match wrote them, n_slots = B * D.
 *   out  tp, fp [T,N] int32: inclusive running counts within the class's segment; a detection with det_ignored adds to neither
 *        recall [T,N]   = tp / npos                          (utils/eval.py:228; 0 where npos is 0)
 *        prec_env [T,N] = reverse running maximum, from the segment's end, of tp / max(tp + fp, 2^-52)   (:229, :46-47)
 *   One workgroup per (class, threshold) scans its segment in chunks of PP_DET_SCAN_CHUNK with a carry, forward for the
 *   counts, backward for the envelope; any segment length works, an empty one writes nothing.
 *   Errors: n_thr outside 1..PP_DET_MAX_THR, n_class < 1, N < 0 or > n_slots, T * n_slots >= 2^31, null pointers: PP_ERR_ARG.
 *
 * pp_det_ap: ap [T,n_class] and recall_final [T,n_class] (the segment's last recall, 0 for an empty segment) from those curves.
 *   mode PP_DET_AP_AREA (_compute_ap, utils/eval.py:42-54): with r_-1 = 0, the sum over the segment's points j where
 *     r_j != r_j-1 of (r_j - r_j-1) * prec_env_j -- each r a quotient as stored, the difference taken of the two quotients (the
 *     closing term of _compute_ap, (1 - r_last) * 0, adds nothing).  Order of the sum, n the segment length: thread k of 256
 *     adds the terms of j in [k per, min(n, (k + 1) per)), per = ceil(n / 256), in ascending j onto 0.0; the 256 partials
 *     p_k are then folded by the halving tree p_k += p_k+s for s = 128, 64, ..., 1 (k < s); the result is p_0.
 *     A class with npos = 0: ap = 0, recall_final = 0 (eval.py:214-216 returns (0, 0)).
 *   mode PP_DET_AP_101 (COCO accumulate): for k = 0..100, r_k = k * 0.01 (1.0 for k = 100: np.linspace(0, 1, 101)), i_k = the
 *     first j with recall_j >= r_k (np.searchsorted, side 'left'), q_k = prec_env at i_k, or 0 when there is none;
 *     ap = (((q_0 + q_1) + q_2) + ... + q_100) / 101.  A class with npos = 0: ap = -1, recall_final = -1 (left out of means).
 *   Errors: unknown mode, n_thr outside 1..PP_DET_MAX_THR, n_class < 1, N < 0, T * N >= 2^31, null pointers: PP_ERR_ARG. */
#define PP_DET_RULE_REFERENCE 0
#define PP_DET_RULE_COCO 1
#define PP_DET_AP_AREA 0
#define PP_DET_AP_101 1
#define PP_DET_MAX_THR 16
#define PP_DET_MAX_DET 1024
#define PP_DET_MAX_GT 1024
#define PP_DET_SCAN_CHUNK 256
int pp_det_match(pp_ctx* ctx, int batch, int n_det, int n_gt, int n_class, const double* det_boxes, const double* det_scores,
                 const int* det_labels, const double* gt_boxes, const int* gt_labels, const unsigned char* gt_ignore,
                 const int* gt_offsets_host, const int* gt_offsets_dev, int n_thr, const double* thresholds, int rule, int* match,
                 unsigned char* det_ignored, int* npos);
int pp_det_pr_curve(pp_ctx* ctx, int n_thr, int n_order, int n_class, long long n_slots, const int* order, const int* class_offsets,
                    const int* match, const unsigned char* det_ignored, const int* npos, int* tp, int* fp, double* recall,
                    double* prec_env);
int pp_det_ap(pp_ctx* ctx, int n_thr, int n_order, int n_class, const int* class_offsets, const int* npos, const double* recall,
              const double* prec_env, int mode, double* ap, double* recall_final);

/* ---- segmentation metrics (csrc/mask_eval.hip; pp_det_match_iou in csrc/det_eval.hip) -------------------------------------
 * The third output of the network, the per-class mask head, and instance masks (utils.scene_gt's mask_visib of ground-truth or
 * estimated poses): semantic tp / fp / fn against the training target, COCO's mask AP as BOP's segmentation task scores it
 * (pack -> pairwise IoU -> matching on that IoU -> pp_det_pr_curve / pp_det_ap unchanged) and run-length encodings.  The
 * reference scores none of this: it thresholds the mask output at 0.5 and writes a picture (linemod_eval.py:336-369); its
 * rle_encode (annotation_scripts/misc.py:42-51) is pinned through tests/golden/mask_rle.npz.  Integer arithmetic, integer
 * atomics only (exact in any order) and one float64 division per IoU: byte-identical to the numpy restatement
 * (tests/mask_eval_np.py) and run to run.  Parity with pycocotools / bop_toolkit is restated, unpinned; the compressed RLE
 * string, crowd regions and area ranges are out of scope.
 *
 * pp_mask_confusion: one pass over the mask head's output.
 *   in   pred [B,M,C] float32 (device): the sigmoid values; target [B,M,C+1] float32 (device): the training target as
 *        pp_anchor_targets writes it and pp_count_positives reads it (the last channel, the any-object flag, is not read);
 *        thresholds [n_thr] float64 on the HOST, 1 <= n_thr <= PP_DET_MAX_THR, any order, not NaN.
 *   out  counts [T,C,3] int64 (zeroed by the call): tp, fp, fn.  A pixel is predicted at threshold t iff (double)pred > thr_t
 *        (the reference's obj_mask > 0.5; NaN is not predicted, -0 equals +0); it is set iff target[..., c] != 0.
 *   A workgroup walks chunks of 16384 consecutive elements of pred, its partial counts as ints in LDS (T C 3 of them, dynamic),
 *   and folds the non-zero ones into counts with 64-bit integer atomics.
 *   Errors before anything is launched: n_thr out of range, a NaN threshold, null pointers: PP_ERR_ARG; B, M < 1, C outside
 *   1..PP_MASK_MAX_CLASS, B M (C + 1) >= 2^31: PP_ERR_SHAPE.
 *
 * pp_mask_pack: byte masks to bits.
 *   in   masks [N,H,W] uint8 (device), non-zero = set.
 *   out  words [N,ceil(H W / 64)] uint64: bit i of word k is pixel 64 k + i in row-major order, the tail bits of the last word 0;
 *        area [N] int64; word_range [N,2] int32: the first non-empty word and one past the last, [0, 0) for an empty mask.
 *   One workgroup of 4 waves per mask; a wave's ballot over 64 pixels is one word.
 *   Errors: N < 0, H or W < 1, H W >= 2^31: PP_ERR_SHAPE; null pointers (N > 0): PP_ERR_ARG.  N = 0 does nothing.
 *
 * pp_mask_iou_pairs: the IoU of every (detection slot, ground truth) pair of each image.
 *   in   detections in padded slots: slot d of image b is packed mask b D + d of det_words [B D,n_word], det_area, det_range
 *        (pp_mask_pack's outputs); det_labels [B,D] int32 or NULL: a slot with a label < 0 is padding, its mask is not read and
 *        its pairs are 0.  Ground truth packed over the batch, gt_words [G,n_word], gt_area, gt_range, with gt_offsets [B+1]
 *        given twice as pp_det_match's are (the HOST copy is checked, the kernel reads the device copy).
 *   out  iou [D G] float64: the pair (b, d, g) at pair_offsets[b] + d ng_b + g, pair_offsets[b] = D gt_offsets[b] (the images
 *        in order, each a [D,ng_b] matrix); inter [D G] int64 in the same layout, or NULL.
 *        inter = sum of popcount(det word & gt word) over the overlap of the two word ranges; iou = inter / (area_d + area_g -
 *        inter), the one division in float64 of the exact integers; 0.0 when the union is 0.
 *   Tiling: a workgroup takes PP_MASK_IOU_TILE_DET slots x PP_MASK_IOU_TILE_GT ground truths of one image; each of its waves
 *   owns one slot, strides its lanes over the slot's word range and ANDs each word with the tile's ground truths.
 *   Errors before anything is launched: D > PP_DET_MAX_DET, an image with more than PP_DET_MAX_GT ground truths, offsets that
 *   decrease or do not run from 0 to G, D G >= 2^31, batch < 1, null pointers: PP_ERR_ARG; H W >= 2^31, too many tiles:
 *   PP_ERR_SHAPE.  D = 0 or G = 0: nothing to write, PP_OK.
 *
 * pp_det_match_iou: pp_det_match with the IoU read from that matrix (iou [D G], never NULL: any one double when there are no
 *   pairs) instead of computed from boxes.  Ranking, tie-breaks, both rules, gt_ignore, padding, npos, outputs, limits and
 *   errors are pp_det_match's (the same kernel with a second IoU source; under PP_DET_RULE_REFERENCE the matrix stands where
 *   the "+1" IoU stood), plus D G >= 2^31: PP_ERR_ARG.  Its outputs feed pp_det_pr_curve / pp_det_ap.
 *
 * pp_mask_rle: run lengths of byte masks, COCO's uncompressed `counts`: the lengths of the alternating runs starting with the
 *   zero run (length 0 when the first pixel is set), in order PP_MASK_ORDER_ROW (row-major: the reference's rle_encode) or
 *   PP_MASK_ORDER_COLUMN (column-major: COCO's).
 *   in   masks [N,H,W] uint8 (device); workspace of pp_mask_rle_workspace_bytes(N) bytes; capacity: the int32 entries counts holds.
 *   out  run_offsets [N+1] int32 (device) and run_offsets_host [N+1] (HOST, always written once the arguments pass): the runs
 *        of mask n are counts[run_offsets[n] .. run_offsets[n+1]); counts [capacity] int32 (device).
 *   Three launches: count the boundaries per mask (a wave's ballot flags 64 positions), scan the counts, then write each run
 *   at its place.  Between the second and the third the call copies run_offsets to the host and waits for the stream (it is
 *   not capturable): where the runs exceed capacity it returns PP_ERR_ARG naming the first mask that does not fit and the
 *   total needed, and writes NOTHING to counts -- no run is ever truncated.
 *   Errors before anything is launched: N < 1, N (H W + 1) >= 2^31: PP_ERR_SHAPE; unknown order, null pointers, a workspace
 *   that is too small, capacity < 0: PP_ERR_ARG.
 *
 * pp_mask_from_rle: the runs back to byte masks of 0 / 255.  run_offsets and counts on the device and the same on the HOST:
 *   the host copy is checked before anything is launched -- offsets from 0 that do not decrease, no negative length, each
 *   mask's lengths adding up to H W exactly, else PP_ERR_ARG.  Shapes and order as pp_mask_rle. */
#define PP_MASK_MAX_CLASS 256
#define PP_MASK_IOU_TILE_DET 4
#define PP_MASK_IOU_TILE_GT 4
#define PP_MASK_ORDER_ROW 0
#define PP_MASK_ORDER_COLUMN 1
int pp_mask_confusion(pp_ctx* ctx, int batch, int n_pix, int n_class, const float* pred, const float* target, int n_thr,
                      const double* thresholds, long long* counts);
int pp_mask_pack(pp_ctx* ctx, int n_mask, int H, int W, const unsigned char* masks, unsigned long long* words, long long* area,
                 int* word_range);
int pp_mask_iou_pairs(pp_ctx* ctx, int batch, int n_det, int n_gt, int H, int W, const unsigned long long* det_words,
                      const long long* det_area, const int* det_range, const int* det_labels, const unsigned long long* gt_words,
                      const long long* gt_area, const int* gt_range, const int* gt_offsets_host, const int* gt_offsets_dev, double* iou,
                      long long* inter);
int pp_det_match_iou(pp_ctx* ctx, int batch, int n_det, int n_gt, int n_class, const double* iou, const double* det_scores,
                     const int* det_labels, const int* gt_labels, const unsigned char* gt_ignore, const int* gt_offsets_host,
                     const int* gt_offsets_dev, int n_thr, const double* thresholds, int rule, int* match, unsigned char* det_ignored,
                     int* npos);
size_t pp_mask_rle_workspace_bytes(int n_mask);
int pp_mask_rle(pp_ctx* ctx, int n_mask, int H, int W, int order, const unsigned char* masks, void* workspace, size_t workspace_bytes,
                long long capacity, int* run_offsets, int* run_offsets_host, int* counts);
int pp_mask_from_rle(pp_ctx* ctx, int n_mask, int H, int W, int order, const int* run_offsets_host, const int* counts_host,
                     const int* run_offsets, const int* counts, unsigned char* masks);

/* ---- normal images from depth maps (csrc/depth_image.hip) ----------------------------------------------------------------
 * The reference's get_normal (annotation_scripts/Augmentations.py:394-467, copied into its annotate_* / augment_* scripts):
 * the surface-normal image it writes as every sample's _dep.png, and the smoothed depth.  float64 from the first filter tap on,
 * every product, sum and quotient rounded on its own; maxima by integer atomics on the bits of non-negative doubles, no float
 * atomics: bit-identical to the numpy restatement (tests/depth_normals_np.py) and run to run.  Pinned to the reference's own
 * function through tests/golden/depth_normals.npz wherever its smoothed depth is not exactly 0 (there its cross product of two
 * parallel tangents is rounding noise).  The hole filling that precedes it in the reference's three-value variants is
 * pp_depth_inpaint below (the project's own fill rule, not cv2.inpaint's; parity with OpenCV is not pinned).
 *
 * pp_depth_normals_f64: n_img images in one call (the batch rides on a grid dimension).
 *   in   depth [n,H,W] float32 (device), finite and >= 0 (NaN is not handled); intr [n,3] float64 (device) = (fx, cx, cy) per
 *        image -- fy takes no part, as in the reference; fx != 0 and |x - cx|, |y - cy| < 32768 (the reference's int16 table is
 *        not wrapped); taps [17] float64 on the HOST: the weights exp(-x^2 / 8) / sum of
 *        scipy.ndimage.gaussian_filter(depth, 2), each in (0, 1), from the caller so that it and its check share one exp.
 *   1. d = the separable filter, rows (axis 0) then columns, border mode 'reflect' (d c b a | a b c d, mirrored again and again
 *      where a line is shorter than the radius 8); a pass adds its 17 products onto the first one in increasing tap index.
 *   2. u = trunc(x - cx), v = trunc(y - cy) toward zero, c = 1 / fx; (gy, gx) = np.gradient(d, 2, edge_order=2): (d[i+1] -
 *      d[i-1]) / 4 inside, (-0.75 d[0] + d[1]) - 0.25 d[2] and (0.25 d[-3] - d[-2]) + 0.75 d[-1] on the first and last line.
 *   3. v_x = (d c + (u c) gx, (v c) gx, gx), v_y = ((u c) gy, d c + (v c) gy, gy), n = v_x x v_y (each component a difference
 *      of two products), n / sqrt((n0 n0 + n1 n1) + n2 n2), NaN -> 0 and +-inf -> +-DBL_MAX (np.nan_to_num), 0 where d > 2000.
 *   out  each may be NULL (skipped), at least one must not be:
 *        signed_f64 [n,H,W,3]         that n;  normals_f64 [n,H,W,3] its absolute value (what for_vis = 1 returns first)
 *        depth_smoothed_f64 [n,H,W]   d (for_vis = 1) or d s (for_vis = 0), the reference's second return value
 *        normals_u8 [n,H,W,3]         for_vis = 0 only (PP_ERR_ARG with for_vis = 1): with s = 1 / max d and
 *                                     m = n (1 - (d s - 0.5)), trunc(m (255 / max m)); both maxima per image, max m over all
 *                                     three components
 *   Degenerate images: where an image's max d or max m is 0 the reference divides by zero; here that image's normals_u8 and
 *   depth_smoothed_f64 (for_vis = 0) are all zero.
 *   Launches: smooth (one launch, both passes from an LDS tile of 32 x 32 pixels with an 8-pixel halo), normals, and for
 *   for_vis = 0 an encode pass that recomputes the normal instead of storing it; d is kept in the workspace.
 *   Errors before anything is launched: n_img outside 1..65535, H or W outside 3..16384, n_img H W >= 2^31: PP_ERR_SHAPE; null
 *   depth / intr / taps / workspace, no output, a tap outside (0, 1), for_vis outside {0, 1}, workspace_bytes <
 *   pp_depth_normals_workspace_bytes(n_img, H, W) (0: a refused shape): PP_ERR_ARG. */
size_t pp_depth_normals_workspace_bytes(int n_img, int H, int W);
int pp_depth_normals_f64(pp_ctx* ctx, int n_img, int H, int W, const float* depth, const double* intr, const double* taps_host,
                         int for_vis, void* workspace, size_t workspace_bytes, double* normals_f64, unsigned char* normals_u8,
                         double* depth_smoothed_f64, double* signed_f64);

/* ---- depth-sensor simulation (csrc/depth_aug.hip) -------------------------------------------------------------------------
 * The reference's augmentDepth (annotation_scripts/Augmentations.py:10-134; augment_syn_LineMOD.py:273-418 and
 * augment_syn_Tless.py:219-356 with their `method` switch): a rendered depth map made to look like a Kinect frame.  Integer
 * work on the mask, float64 from the first average on, every product, sum and quotient rounded on its own; no atomics and no
 * reduction across lanes: bit-identical to the numpy restatement (tests/depth_aug_np.py) and run to run.
 * Pinned: the majority filter to scipy.signal.medfilt2d and the opening to scipy.ndimage's grey erosion / dilation
 * (tests/test_depth_aug_cpu.py).  Not pinned, restated from OpenCV's documented rules: morphologyEx's default border, resize
 * INTER_LINEAR, GaussianBlur's BORDER_REFLECT_101 and tap weights -- and OpenCV computes a float32 image in float32 where this
 * is float64.  Not the reference's at all: the simplex noise (the project's own; pyfastnoisesimd's bits cannot be had) and the
 * standard normals, which the caller supplies as a field (the device draws none: log and cos would not be numpy's bits).
 *
 * One float64 row of PP_DA_P values per image, on the device (params) and the same rows on the HOST (params_host, validated
 * and used to decide which launches are needed; the kernels read the device copy): */
#define PP_DA_K_OPEN 0      /* box of the opening, 1 | 3 | 5 | 7 */
#define PP_DA_K_MED 1       /* window of the majority (median) filter, 1 | 3 | 5 | 7 */
#define PP_DA_K_BLUR 2      /* taps of the blur, 1 | 3 | 5 | 7 */
#define PP_DA_TAPS 3        /* 7 slots: the first k_blur hold cv2.getGaussianKernel's weights, from the caller (one exp for all) */
#define PP_DA_DEPTH_NOISE 10
#define PP_DA_SENSOR 11     /* 0 | 1: the half-resolution sensor stage */
#define PP_DA_SIMPLEX 12    /* 0 | 1: the simplex warp (the reference's method 0 = both, 1 = sensor only, 2 = simplex only) */
#define PP_DA_FREQ 13       /* in [0, 16] */
#define PP_DA_OCTAVES 14    /* 1..8 */
#define PP_DA_LACUNARITY 15 /* in (0, 4] */
#define PP_DA_GAIN 16
#define PP_DA_W_XY 17
#define PP_DA_W_Z 18
#define PP_DA_JITTER_LO 19  /* 3 values, one per noise field; |.| <= 65536 */
#define PP_DA_JITTER_HI 22  /* 3 values */
#define PP_DA_SEED 25       /* an integer in [0, 2^53) */
#define PP_DA_P 26
/* pp_depth_augment: n_img images in one call (the batch rides on a grid dimension).
 *   in   depth [n,H,W] float32 (device; millimetres, finite, >= 0); mask [n,H,W] uint8 (device; non-zero = foreground);
 *        z [n,h2,w2] float32 standard normals (device; may be NULL when no image has sensor = 1), h2 = rint(H / 2) and
 *        w2 = rint(W / 2), half to even (cv2's cvRound).
 *   A  shadow and halve (one launch; a 32 x 32 tile with a 9-pixel halo as bytes in LDS).  m0 = mask != 0; erode with the
 *      k_open x k_open box, then dilate with it, pixels outside the image taking no part in either; m = (set pixels in the
 *      zero-padded k_med x k_med window) > k_med^2 / 2; d1 = m ? depth : 0.  With sensor: d2[y,x] = 0.5 a + 0.5 b of rows
 *      min(2y, H-1) and min(2y+1, H-1), a and b each 0.5 p + 0.5 q of columns min(2x, W-1) and min(2x+1, W-1).
 *   B  sensor (one launch on the half-size image; a 32 x 32 tile with a 3-pixel halo in LDS).  res = ((d2 / 1000) 1.41421356)^2
 *      (the square one product); b = the k_blur taps along each row, then along each column, border reflect_101
 *      (gfedcb|abcdefgh, mirrored again and again on a short line), a pass adding its products onto the first one in
 *      increasing tap index; q = res != 0 ? rint(b / res) res : 0 (half to even); s = q + (q depth_noise) z.
 *   C  warp (one launch, a lane per pixel).  D = d1 without sensor; with it the bilinear up-sampling of s, evaluated from s
 *      where it is needed and never stored: f = (x + 0.5)(w2 / W) - 0.5, sx = floor(f), frac = f - sx; sx < 0 -> (0, 0);
 *      sx >= w2 - 1 -> (w2 - 1, 0); (1 - frac) l + frac r along the columns of each of the two rows, then between the rows.
 *      simplex = 0: out = D.  Otherwise V_f, f = 0..2, = sum_o gain^o N(p lacunarity^o; seed + o) / sum_o gain^o (both sums
 *      from 0.0 in increasing o, the powers by repeated multiplication), p = (j_f freq, y freq, x freq),
 *      j_f = lo_f + (hi_f - lo_f) u, u = (splitmix64(splitmix64(4 seed + f) + (y W + x)) >> 11) 2^-53; N: Gustavson's 3-D
 *      simplex noise, its hash, corner order and scale (32) in the comment at the head of csrc/depth_aug.hip.  a = D 0.001;
 *      fx = x + (a w_xy) V0, fy = y + (a w_xy) V1, clamped to [0, W-1] / [0, H-1], truncated; out = D(fy, fx) + (a w_z) V2,
 *      then out > 0 ? out : 0.
 *   out  each may be NULL (skipped, with the launches nobody needs), at least one must not be:
 *        depth_f32 [n,H,W] out rounded once to float32 (what feeds pp_depth_normals_f64); depth_f64 [n,H,W] out;
 *        mask_u8 [n,H,W] m as 0 / 255; half_f64 [n,h2,w2] s (zeros for an image without sensor);
 *        sensor_f64 [n,H,W] D (d1 for an image without sensor)
 *   Errors before anything is launched: n_img outside 1..65535, H or W outside 8..16384: PP_ERR_SHAPE; a null depth / mask /
 *   params / params_host / workspace, no output, a kernel size not in {1, 3, 5, 7}, octaves not an integer in 1..8, sensor or
 *   simplex not 0 / 1, a seed that is no integer in [0, 2^53), freq, lacunarity or a jitter bound out of range, any parameter
 *   not finite, z NULL while an image has sensor = 1, workspace_bytes < pp_depth_augment_workspace_bytes(n_img, H, W)
 *   (0: a refused shape): PP_ERR_ARG. */
size_t pp_depth_augment_workspace_bytes(int n_img, int H, int W);
int pp_depth_augment(pp_ctx* ctx, int n_img, int H, int W, const float* depth, const unsigned char* mask, const double* params,
                     const double* params_host, const float* z, void* workspace, size_t workspace_bytes, float* depth_f32,
                     double* depth_f64, unsigned char* mask_u8, double* half_f64, double* sensor_f64);

/* ---- depth-hole filling (csrc/depth_inpaint.hip) --------------------------------------------------------------------------
 * What the reference does with cv2.inpaint(depth, depth == 0, 5, cv2.INPAINT_NS) at the head of get_normal in seven of its
 * scripts (annotate_val_LineMOD.py:206-221, annotate_val_LM_BOP.py, annotate_val_LMO_BOP.py, annotate_val_YCBV_BOP.py,
 * prepare_val_LineMOD_RGB.py, augment_syn_LineMOD.py, augment_syn_Tless.py), and the rescaling that follows it there.  The
 * method is the project's own, of the same kind as OpenCV's (holes filled from their rim inwards by distance-weighted means)
 * but order-free: OpenCV's fast marching is a sequential priority queue, and OpenCV is not a dependency, so parity with
 * cv2.inpaint is not pinned.  float64 throughout where cv2 is float32, every product, sum and quotient rounded on its own; no
 * floating-point atomics: bit-identical to the numpy restatement (tests/depth_inpaint_np.py) and run to run.  The layer map is
 * pinned to scipy.ndimage.distance_transform_cdt(metric='chessboard') (tests/test_depth_inpaint_cpu.py).
 *
 * pp_depth_inpaint: n_img images in one call.
 *   in   depth [n,H,W] float32 (device), finite and >= 0 (NaN is not handled); hole_mask [n,H,W] uint8 (device; non-zero = hole)
 *        or NULL: a hole is depth == 0; radius 1..8 (the reference's inPaiDia 5 is radius 5); max_dist 0..65535, 0 = no limit;
 *        rescale 0 | 1.
 *   1. Layer map.  L = the chessboard distance from a pixel to the nearest known (non-hole) pixel of its image, 0 on known
 *      pixels.  Pixels outside the image do not exist: they are neither known nor holes.  An image without a known pixel has
 *      L = 65535 everywhere, is returned as it came (the input depth, no rescaling) and counts
 *      (H W, 0, 0).
 *   2. Fill.  v = depth as float64 on known pixels and 0 on holes.  For k = 1, 2, ... every pixel p with L(p) = k, and
 *      k <= max_dist where a limit is set, gets v(p) = (sum_q w v(q)) / (sum_q w) over the q of the (2 radius + 1)^2 window
 *      around p that lie inside the image and have L(q) < k, taken in row-major order, both sums from 0.0,
 *      w = 1.0 / (double)((dx^2 + dy^2)(1 + L(q))) with the product an integer.  Layer k reads layers < k only, so the result
 *      does not depend on the order inside a layer; a pixel of layer k has a neighbour of layer k - 1 at chessboard distance 1,
 *      so the sums are never empty.  Holes beyond max_dist stay 0.
 *   3. rescale = 1 (the reference's lines 216-219): v <- ((v - min v) / (max v - min v)) max depth per image, min v and max v
 *      over the filled image and max depth over the input, each exact (integer atomics on the bits of non-negative doubles).
 *      Where max v = min v the image stays as it is (the reference divides by zero there).
 *   out  each may be NULL (skipped, with the launches nobody needs), at least one must not be:
 *        filled_f32 [n,H,W] v rounded once to float32 (what feeds pp_depth_normals_f64); filled_f64 [n,H,W] v;
 *        layer_u16 [n,H,W] L; counts [n,3] int32: holes, pixels to fill (1 <= L, and L <= max_dist under a limit), the largest
 *        L of the image whether or not max_dist cuts it off (0 without holes or without known pixels).
 *   Launches: row distances (half a wave of 32 lanes per row), the layer map with a histogram of the layers (32 x 8 pixels per
 *   workgroup), and for the filled outputs a scan of the histogram, a counting sort of the pixels to fill by layer, ONE HOST
 *   SYNCHRONISATION that reads the layers' offsets back, one fill launch per non-empty layer over that layer's pixels of all
 *   images, the extrema for rescale = 1, and a last pass that rescales and rounds.  Not capturable in a graph for that reason.
 *   Workspace: pp_depth_inpaint_workspace_bytes(n_img, H, W) = a(4 (4 n + 12289)) + a(24 n) + 2 a(2 P) + a(4 P) + a(8 P) bytes
 *   with P = n H W and a(b) = b rounded up to a multiple of 256 (0: a refused shape).
 *   Errors before anything is launched: n_img outside 1..65535, H or W outside 3..4096, n_img H W >= 2^31: PP_ERR_SHAPE; a null
 *   depth / workspace, radius outside 1..8, max_dist outside 0..65535, rescale outside {0, 1}, no output, workspace_bytes too
 *   small: PP_ERR_ARG. */
size_t pp_depth_inpaint_workspace_bytes(int n_img, int H, int W);
int pp_depth_inpaint(pp_ctx* ctx, int n_img, int H, int W, const float* depth, const unsigned char* hole_mask, int radius,
                     int max_dist, int rescale, void* workspace, size_t workspace_bytes, float* filled_f32, double* filled_f64,
                     unsigned short* layer_u16, int* counts);

/* ---- evaluation overlays: boxes, wireframes, discs, bitmap text and an id layer over uint8 images (overlay.hip) ----
 * What the reference draws with OpenCV: cv2.rectangle and cv2.putText for detections and annotations
 * (utils/visualization.py), twelve cv2.line calls per projected 3-D box and cv2.circle per voted corner
 * (linemod_eval.py:537-620), draw_axis (annotation_scripts/misc.py:8), and the mask head's output as an image
 * (linemod_eval.py:343-369).  The rules below are the project's own: exact integer coverage tests, no Bresenham stepping, no
 * anti-aliasing (the reference passes LINE_AA to cv2.rectangle), no Hershey font -- glyph bitmaps travel in the records, the
 * library holds no font.  OpenCV is not a dependency, so parity with cv2 is not pinned.  Integer arithmetic only, no atomics, no
 * floating point: the result is a pure function of the inputs, byte for byte the numpy restatement (tests/overlay_np.py) and the
 * same run to run.
 *
 * pp_draw_overlay_u8: B images in ONE launch, no workspace, no host synchronisation (capturable in a graph).
 *   in   images [B,H,W,3] uint8 (device).  The channel order is the caller's: a colour names channels by index.
 *        prims [n_total,8] int32 and image_offsets [B+1] int32 (device): image b owns the records image_offsets[b] ..
 *        image_offsets[b+1], painted in list order, later over earlier.  The offsets are read on the device and never checked on
 *        the host: each is cut to 0 .. n_total and an end below its begin is an empty list.  n_total may be 0 with prims NULL.
 *        ids [B,H,W] uint8 (device) or NULL: the id layer; palette [256] int32 (device) packed colours, entry 0 is never drawn;
 *        id_mode: bit 0 = fill, bit 1 = outline (0: the id layer is off; ignored with ids NULL); outline_width 1..4.
 *   out  out [B,H,W,3] uint8 (device).  It may be the same pointer as images (every pixel is read and written by one thread only);
 *        any other overlap of the two is undefined.
 *   Colour: c0 | c1 << 8 | c2 << 16 | A << 24, c_k the value of channel k.  Painting a pixel value p with it is, per channel,
 *        p <- (A c + (255 - A) p + 127) / 255 in integers: the identity at A = 0, a plain store at A = 255.
 *   Record: (kind, a0, a1, a2, a3, size, colour, reserved); reserved is not read.  Pixel (x, y), 0 <= x < W, 0 <= y < H:
 *     0 SEGMENT    (a0, a1) = P0, (a2, a3) = P1, size = thickness t, 1 <= t <= 64, every coordinate |v| <= 8192.  Covered iff
 *                  the squared distance from the pixel to the segment is <= t^2 / 4, exactly: with d = P1 - P0, L2 = d.d,
 *                  w = P - P0, s = w.d:  s <= 0: 4 |w|^2 <= t^2;  s >= L2: 4 |P - P1|^2 <= t^2;  otherwise
 *                  4 cross(d, w)^2 <= t^2 L2 (int64: |d|, |w| <= 2^14 per coordinate, |cross| <= 2^29, 4 cross^2 <= 2^60).
 *                  Round caps; P0 == P1 is the filled disc of diameter t (the reference's cv2.circle(..., 3, ..., -2) is t = 7:
 *                  4 |w|^2 <= 49, |w|^2 <= 12).  Rectangles and box wireframes are segments, built on the host.
 *     1 GLYPH      (a0, a1) = the top-left of an 8 x 8 cell grid, |v| <= 8192 (beyond it no cell reaches an image);
 *                  a2 = bits 0..31, a3 = bits 32..63 of a bitmap whose bit 8 row + col is cell (col, row);
 *                  size = scale | dilate << 8, scale 1..4, dilate 0..2, the bits above zero.  Position (qx, qy) lies in cell
 *                  (floor((qx - a0) / scale), floor((qy - a1) / scale)) where both are in 0..7.  Covered iff some position
 *                  within chessboard distance dilate of the pixel -- inside the image or not -- lies in a set cell.
 *     2 FILL_RECT  (a0, a1), (a2, a3): corners, inclusive, in any order, any int32; size is not read.
 *     Any other kind, or a field outside these ranges, paints nothing (tested once per record, not per pixel).
 *   Id layer, before the records, with L = ids at the pixel: fill paints every pixel with L != 0 with palette[L]; outline then
 *        paints (with palette[L] again, over the fill where both are on) every pixel with L != 0 for which some pixel within
 *        chessboard distance outline_width that lies inside the image has an id other than L (0 included): an inner contour.
 *        Pixels outside the image are ignored, so a label that runs into the image border has no contour along it.
 *   Launch: a workgroup of 256 threads per 32 x 32 tile and image, 4 adjacent pixels per thread held in registers from the one
 *   read to the one write; the id tile with its halo of 4 in LDS; the records in chunks of 256, those whose bounding box reaches
 *   the tile compacted into LDS in list order (ballot, popcount prefix), then walked by every pixel.  Every tile reads its
 *   image's whole list.
 *   Errors before anything is launched, PP_ERR_ARG each: B < 1, H or W outside 1..8192, n_total outside 0..2^24, a null images /
 *   out / image_offsets, null prims with n_total > 0, id_mode outside 0..3, ids without palette, outline_width outside 1..4
 *   while outlining (ids set and bit 1 of id_mode). */
int pp_draw_overlay_u8(pp_ctx* ctx, int B, int H, int W, const unsigned char* images, unsigned char* out, const int* prims,
                       const int* image_offsets, int n_total, const unsigned char* ids, const int* palette, int id_mode,
                       int outline_width);

/* ---- connected components: the mask head's planes, or an id image, to instance labels and masks (cc.hip) ----
 * The step between a class plane and instance masks, which the reference's area clustering hands to a PCL binary (encode_area,
 * annotate_val_LineMOD.py:88-130; its point-cloud smoothness condition is not restated).  Integers only: every output is a
 * pure function of the inputs, byte for byte the numpy restatement (tests/cc_np.py), whose labels are pinned to
 * scipy.ndimage.label (tests/test_cc_cpu.py).  Parity with cv2.connectedComponents, which numbers differently, is not pinned.
 *
 * pp_cc_label: N planes in one call, no host synchronisation (capturable in a graph).
 *   in   planes [N,H,W] uint8 (device); connectivity 4 | 8; mode PP_CC_BINARY: a non-zero byte is foreground and any two
 *        adjacent foreground pixels connect; PP_CC_VALUE: two adjacent pixels connect iff their bytes are equal and non-zero
 *        (an instance-id image, an arg-max class image); weight [N,H,W] int32 >= 0 (device) or NULL; max_components M.
 *   out  labels [N,H,W] int32: 0 on background; the components of a plane are numbered 1 .. n in the raster order
 *        (smallest y W + x) of their first pixels, whatever M is.
 *        counts [N] int32: n, also where n > M.
 *        stats [N,M,6] int32: area, x_min, y_min, x_max, y_max (inclusive), value (the component's byte in value mode, 1 in
 *        binary mode) of component k + 1 in row k; rows k >= min(n, M) are zero.
 *        sums [N,M,3] int64: the sums of x, of y and of weight over the component's pixels (0 without weight), rows as in stats.
 *   Launches: a workgroup per 32 x 32 tile labels its tile in LDS (minimum over the compatible neighbours, pointer jumping,
 *   until a round changes nothing) and writes each pixel the plane index of its tile-local root; a thread per pixel beside a
 *   tile seam joins the trees across it (atomicMin of the smaller root into the larger); every pixel then takes its root, which
 *   is the component's first raster pixel; one workgroup per plane scans the root flags in chunks with a carry; a last pass
 *   writes labels = rank of the root + 1 and folds the statistics with integer atomics.  No loop waits for another workgroup.
 *   Every data-dependent loop counts its steps against a bound from the sizes (1024 rounds of a tile, H W steps of a chase, H W
 *   retries of a union); one that reaches it stops and sets a bit in the error word, the first int32 of the workspace, which
 *   the call zeroes first: 1 the tile pass, 2 a chase, 4 a union.  The call cannot see the word without waiting for the device,
 *   so it is the caller who reads it, after the stream has drained; the outputs of a call whose word is not 0 are undefined.
 *   Workspace: a(4) + 2 a(4 N H W) bytes, a(b) = b rounded up to a multiple of 256: the error word, the parents, the ranks;
 *   256-byte aligned.
 *   Errors before anything is launched: N < 1, H or W < 1, H W >= 2^31, H > 32 * 65535: PP_ERR_SHAPE; connectivity, mode,
 *   max_components outside 1..65535, a null planes / workspace / output, workspace_bytes too small or misaligned: PP_ERR_ARG.
 *
 * pp_cc_select: masks [S,H,W] uint8 (device), masks[s] = (labels[slot_plane[s]] == slot_label[s]) as 0 / 1, one pixel pass,
 *   four pixels per dword store where H W is a multiple of 4.  labels [N,H,W] int32, slot_plane / slot_label [S] int32 (device).
 *   A slot with slot_plane outside 0 .. N - 1 or slot_label <= 0 gives a zero mask and reads no label plane; so does a label
 *   above its plane's count.  S = 0 does nothing.  Errors: the shape rules above and S < 0: PP_ERR_SHAPE; null: PP_ERR_ARG. */
#define PP_CC_BINARY 0
#define PP_CC_VALUE 1
int pp_cc_label(pp_ctx* ctx, int N, int H, int W, const unsigned char* planes, int connectivity, int mode, const int* weight,
                int max_components, void* workspace, size_t workspace_bytes, int* labels, int* counts, int* stats, long long* sums);
int pp_cc_select(pp_ctx* ctx, int N, int H, int W, const int* labels, int S, const int* slot_plane, const int* slot_label,
                 unsigned char* masks);

#ifdef __cplusplus
}
#endif
#endif /* PYRAPOSE_HIP_H */
