// Host-side launchers of the conv3 units (conv3_igemm.hip, conv3_igemm4x.hip, conv3_wgrad.hip, conv3_aux.hip; one build per plane
// format each, like conv4.hip / conv4.h), called from the entry points of conv3.hip and from one another.  Include after
// conv3_unit.h: the names carry the format through PP_API, so the two builds do not collide.  A launcher launches what its plan
// says (conv_plan.h made every decision): it reads no switch and plans nothing.
#pragma once
#include "conv_common.h"

// the operands of one forward / data-gradient launch, beside IgemmParams
struct Igemm3Args {
  const void *ahi, *alo, *whi, *wlo;  // gathered operand as planes (NULL: p.src), weight planes
  int w_rows, w_ld8;
  void *ohi, *olo;                    // output planes (may be NULL)
  void *chi, *clo;                    // may be NULL: also write the split of the gathered f32 operand (pp_conv_opts.capture_hi / capture_lo) --
                                      // inside the tap-row-reuse kernel where that one runs, by a separate pass over the operand otherwise
  const unsigned char* flags;         // may be NULL: the row-block flags of the gathered operand
  float* ws;                          // the context's scratch (may be NULL)
};

// ---- conv3_igemm.hip ----
// the launches of one plan of pp_plan_igemm (kernel, split-K finish, capture pass) on the plan's tile
void PP_API(pp3_launch_igemm)(hipStream_t st, IgemmParams& p, const Igemm3Args& a, const PpIgemmPlan& pl);
// the merged stride-2 data gradient (igemm3m_kernel): one launch on the route's tile; p: the fields its classes share
void PP_API(pp3_launch_igemm_s2)(hipStream_t st, IgemmParams& p, const Igemm3Args& a, const DgradS2Route& r);
// the launch over the listed 32-row blocks (pl: pp_plan_listed): dilate (dy_flags != NULL) -> compact -> igemm3f over the list ->
// split-K finish -> fill of the other blocks (fill).  scratch: n_blocks bytes + (n_blocks + 1) ints behind the caller's flags / list
void PP_API(pp3_launch_igemm_rowlist)(hipStream_t st, IgemmParams& p, const Igemm3Args& a, const PpIgemmPlan& pl, const unsigned char* dy_flags,
                                      unsigned char* out_flags, int* out_list, bool fill);
// a parity class without taps (class_fill_kernel): dx = mask?(addend or 0) at the class rows
void PP_API(pp3_launch_class_fill)(hipStream_t st, const IgemmParams& p, unsigned blocks, const float* addend, const float* mask, float* out, void* ohi,
                                   void* olo);
// rl_dilate_kernel over the n_blocks 32-row blocks of p's row space (p: n_seg, seg, M)
void PP_API(pp3_launch_rl_dilate)(hipStream_t st, const IgemmParams& p, const unsigned char* in_flags, unsigned char* out_flags, int n_blocks);

// ---- conv3_igemm4x.hip ----
// igemm4x_kernel for the whole rounds of a PP_IGEMM4X (256 x 128, pl.variant) or PP_IGEMM4X2 (128 x 128) plan; the caller launches
// the split-K tail of the last round
void PP_API(pp3_launch_igemm4x)(hipStream_t st, const IgemmParams& p, const Igemm3Args& a, const PpIgemmPlan& pl);

// ---- conv3_wgrad.hip ----
// the launches of one plan of pp_plan_wgrad (families PP_WGRAD3 / PP_WGRAD3F_*; kernel and slice finish) on the plan's tile
void PP_API(pp3_launch_wgrad)(hipStream_t st, const Wgrad3Params& p, const PpWgradPlan& pl, const float* x, const float* dy, const void* xhi,
                              const void* xlo, const void* dhi, const void* dlo, float* dw, float* dbias, const int* list, float* ctx_ws);

// ---- conv3_aux.hip ----
// the capture pass where the tap-row-reuse kernel does not run: the gathered f32 operand of p split into the planes chi / clo
void PP_API(pp3_split_capture_pass)(hipStream_t st, const IgemmParams& p, void* chi, void* clo);
// row_block_compact_kernel: list[0] = count, list[1 ..] = the flagged block indices, ascending
void PP_API(pp3_launch_row_block_compact)(hipStream_t st, const unsigned char* flags, int n_blocks, int* list);
