// Host-side launchers of conv4.hip (one build per plane format, like the conv3 units and conv3.h), called from conv3.hip's
// weight-gradient entry point and from launch_igemm3 (conv3_igemm.hip).
#pragma once
#include "conv_common.h"

// the persistent LDS-DMA GEMM of the 1x1 convolutions (igemm4p_kernel): p as launch_igemm3 fills it; splits > 1 writes partial sums to
// `ws` (the caller runs splitk_finish_kernel); grid: persistent workgroups (pp_plan_igemm: one per CU, or per item if fewer); nst = stages of the ring (3 or 4)
void pp4_launch_igemm4p_fmt0(hipStream_t st, IgemmParams& p, const void* ahi, const void* whi, const void* wlo, int w_rows, int w_ld8, void* ohi,
                             void* olo, int splits, float* ws, unsigned grid, int nst);
void pp4_launch_igemm4p_fmt1(hipStream_t st, IgemmParams& p, const void* ahi, const void* whi, const void* wlo, int w_rows, int w_ld8, void* ohi,
                             void* olo, int splits, float* ws, unsigned grid, int nst);

// the tap-row-reuse weight gradient of 3x3 stride-1 "same" convolutions on plane-stored operands (wgrad3r_kernel; w: wgrad3w_kernel):
// p and grid as pp_plan_wgrad laid them out
void pp4_launch_wgrad3r_fmt0(hipStream_t st, const Wgrad3Params& p, unsigned grid, bool w, const void* xhi, const void* xlo, const void* dhi,
                             const void* dlo, float* dw, float* dbias, const int* list);
void pp4_launch_wgrad3r_fmt1(hipStream_t st, const Wgrad3Params& p, unsigned grid, bool w, const void* xhi, const void* xlo, const void* dhi,
                             const void* dlo, float* dw, float* dbias, const int* list);
