// Prologue of every translation unit of the plane-format convolution family (conv3.hip, conv3_igemm.hip, conv3_igemm4x.hip,
// conv3_wgrad.hip, conv3_aux.hip, conv4.hip).  Each unit is compiled once per plane format (PP_FMT = 0: bf16 pairs / bf16x3,
// PP_FMT = 1: P16 / f16c8; planes_fmt.h, csrc/Makefile): its kernels and helpers have internal linkage, and whatever another unit or
// conv3_dispatch.hip calls carries the format in its name through PP_API -- the entry points pp_*, which conv3_dispatch.hip forwards
// to the build the context asks for (pp_ctx_set_planes_format), and the host launchers of conv3.h / conv4.h.
#pragma once
#include "conv_common.h"

#define PP_CAT_(a, b) a##b
#define PP_CAT(a, b) PP_CAT_(a, b)
#if PP_FMT == 1
#define PP_API(name) PP_CAT(name, _fmt1)
#else
#define PP_API(name) PP_CAT(name, _fmt0)
#endif

namespace {
#include "planes_fmt.h"

#include "conv3_shared.h"
}  // namespace
