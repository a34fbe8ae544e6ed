"""Thin torch-tensor wrappers over the C ABI (include/pyrapose_hip.h).

Every function takes CUDA(ROCm) float32/float64/int tensors, hands raw device pointers to the HIP
library on the ctx stream, and raises on a non-zero status.  torch is used only for memory and streams.
"""
import collections
import ctypes as C

import numpy as np
import torch

from ._lib import ConvDesc, ConvOpts, ParamDesc, RowSpace, TView, check, lib
from ._lib import check as check_status  # for wrappers that take a `check` argument of their own


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda, "pyrapose_amd ops need device tensors"
    return C.c_void_p(t.data_ptr())


class Context:
    """One per (process, device, stream): wraps pp_ctx."""

    def __init__(self, device=0, stream=None):
        if not torch.cuda.is_available():
            raise RuntimeError("pyrapose_amd: no GPU visible (torch.cuda.is_available() is False); "
                               "the HIP path has no CPU fallback")
        self.device = int(device)
        torch.cuda.set_device(self.device)
        self.handle = C.c_void_p()
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.stream = s
        check(lib.pp_ctx_create(C.byref(self.handle), self.device, C.c_void_p(s.cuda_stream)), None, "pp_ctx_create")

        self.planes_fmt = 0
        self._twin = None

    def use_stream(self, stream):
        # (the twin points back at this context: bind both handles here instead of forwarding, which would never return)
        for c in (self, self._twin):
            if c is not None:
                c.stream = stream
                check(lib.pp_ctx_set_stream(c.handle, C.c_void_p(stream.cuda_stream)), c.handle, "pp_ctx_set_stream")

    def twin(self, fmt):
        """This context for plane format `fmt` (0 bf16 pairs / bf16x3, 1 P16 / f16c8): itself, or -- created on first use -- a
        second context on the same stream, with the same split-K scratch, whose launches read and write the other format."""
        if int(fmt) == self.planes_fmt:
            return self
        if self._twin is None:
            t = Context(self.device, self.stream)
            set_planes_format(t, fmt)
            t._twin = self
            ws = getattr(self, "workspace", None)
            t.workspace = ws
            if ws is not None:
                check(lib.pp_ctx_set_workspace(t.handle, _ptr(ws), ws.numel() * 4), t.handle, "pp_ctx_set_workspace")
            self._twin = t
        assert self._twin.planes_fmt == int(fmt)
        return self._twin

    def set_workspace(self, nbytes):
        """Scratch for split-K convolutions (pp_ctx_set_workspace); 0 removes it."""
        self.workspace = torch.empty((int(nbytes) // 4,), dtype=torch.float32, device="cuda:%d" % self.device) if nbytes else None
        for c in (self, self._twin):
            if c is not None:
                c.workspace = self.workspace
                check(lib.pp_ctx_set_workspace(c.handle, _ptr(self.workspace), (int(nbytes) // 4) * 4 if nbytes else 0), c.handle,
                      "pp_ctx_set_workspace")

    def device_info(self):
        n = C.c_int(0)
        buf = C.create_string_buffer(128)
        check(lib.pp_device_info(self.handle, C.byref(n), buf, 128), self.handle)
        return n.value, buf.value.decode()

    def close(self):
        t, self._twin = self._twin, None
        if t is not None and t.handle:
            t._twin = None
            t.close()
        if self.handle:
            lib.pp_ctx_destroy(self.handle)
            self.handle = C.c_void_p()


def make_conv_desc(n_img, in_shapes, out_shapes, cin, cout, k, stride, pad_t, pad_l, ld_x, ld_y, ld_w):
    d = ConvDesc()
    d.in_ = RowSpace.make(n_img, in_shapes)
    d.out = RowSpace.make(n_img, out_shapes)
    d.cin, d.cout, d.kh, d.kw, d.stride = cin, cout, k, k, stride
    d.pad_t, d.pad_l, d.ld_x, d.ld_y, d.ld_w = pad_t, pad_l, ld_x, ld_y, ld_w
    return d


PLAN_FWD, PLAN_BWD_DATA, PLAN_BWD_WEIGHT, PLAN_BWD_DATA_S2 = 0, 1, 2, 3
PLAN_PLANES_IN, PLAN_PLANES_OUT, PLAN_F32_OUT, PLAN_CAPTURE, PLAN_LIST, PLAN_LAZY_IN, PLAN_LAZY_OUT = 1, 2, 4, 8, 16, 32, 64


def conv_plan_text(d, pass_, forms=0, planes_fmt=1, n_cu=256, ws_bytes=0):
    """Which kernels the bf16x3 entry points would launch for descriptor d (pp_conv_plan_text: host only, no context, no GPU):
    one line per launch, the PP_CONV_DEBUG wording + the kernel family + ' | ' + the plan's numbers as key=value"""
    buf = C.create_string_buffer(4096)
    n = lib.pp_conv_plan_text(C.byref(d), int(pass_), int(forms), int(planes_fmt), int(n_cu), int(ws_bytes), buf, len(buf))
    check(min(n, 0), None, "pp_conv_plan_text")
    return buf.value.decode()


def conv_fwd(ctx, d, x, w, bias, residual, relu, y):
    ld_res = residual.stride(0) if residual is not None else 0
    check(lib.pp_conv2d_nhwc_fwd(ctx.handle, C.byref(d), _ptr(x), _ptr(w), _ptr(bias), _ptr(residual), ld_res,
                                 int(bool(relu)), _ptr(y)), ctx.handle, "pp_conv2d_nhwc_fwd")


def conv_bwd_data(ctx, d, dy, w, addend, relu_src, dx):
    ld_add = addend.stride(0) if addend is not None else 0
    ld_rs = relu_src.stride(0) if relu_src is not None else 0
    check(lib.pp_conv2d_nhwc_bwd_data(ctx.handle, C.byref(d), _ptr(dy), _ptr(w), _ptr(addend), ld_add, _ptr(relu_src),
                                      ld_rs, _ptr(dx)), ctx.handle, "pp_conv2d_nhwc_bwd_data")


def conv_bwd_weight(ctx, d, x, dy, dw, dbias):
    check(lib.pp_conv2d_nhwc_bwd_weight(ctx.handle, C.byref(d), _ptr(x), _ptr(dy), _ptr(dw), _ptr(dbias)), ctx.handle,
          "pp_conv2d_nhwc_bwd_weight")


def conv_split_weights3(ctx, d, w, fwd_hi, fwd_lo, dg_hi, dg_lo):
    check(lib.pp_conv_split_weights_bf16x3(ctx.handle, C.byref(d), _ptr(w), _ptr(fwd_hi), _ptr(fwd_lo), _ptr(dg_hi), _ptr(dg_lo)),
          ctx.handle, "pp_conv_split_weights_bf16x3")


class SplitWeightsBatch(object):
    """Job table (device resident) for pp_conv_split_weights_bf16x3_batch: every listed tensor is re-split by one launch."""

    def __init__(self, jobs):
        """jobs: iterable of (desc, w, fwd_hi, fwd_lo, dg_hi, dg_lo) as for conv_split_weights3."""
        from ._lib import SplitJob
        jobs = list(jobs)
        arr = (SplitJob * max(len(jobs), 1))()
        tiles = 0
        self._keep = jobs  # the table holds raw pointers into these tensors
        for i, (d, w, fh, fl, dh, dl) in enumerate(jobs):
            if d.cin % 32:
                raise ValueError("SplitWeightsBatch: cin %d must be a multiple of 32" % d.cin)
            j = arr[i]
            j.w, j.fwd_hi, j.fwd_lo, j.dg_hi, j.dg_lo = [(t.data_ptr() if t is not None else None) for t in (w, fh, fl, dh, dl)]
            j.taps, j.cin, j.cout, j.ld_w, j.tile_begin = d.kh * d.kw, d.cin, d.cout, d.ld_w, tiles
            tiles += j.taps * (d.cin // 32) * ((d.cout + 31) // 32)
        self.n, self.tiles = len(jobs), tiles
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.table = host.cuda()

    def run(self, ctx):
        check(lib.pp_conv_split_weights_bf16x3_batch(ctx.handle, self.n, _ptr(self.table), self.tiles), ctx.handle,
              "pp_conv_split_weights_bf16x3_batch")


def new_planes(rows, ld, device="cuda", fill=0):
    """A tensor [rows][ld] (ld % 8 == 0) as PACKED bf16 planes: one buffer of rows * ld * 4 bytes cut into 32-byte groups of 8
    channels -- 16 bytes of hi, 16 bytes of lo (value = hi + lo).  Returns the (hi, lo) pair the C ABI takes: int16 views
    [rows, ld / 8, 8] of that buffer with lo.data_ptr() == hi.data_ptr() + 16; row slices of both stay valid pairs."""
    assert ld % 8 == 0, ld
    base = torch.full((rows, ld // 8, 2, 8), fill, dtype=torch.int16, device=device)
    return base[:, :, 0, :], base[:, :, 1, :]


def planes_ld(planes):
    """leading dimension (elements per row) of a packed plane pair"""
    return planes[0].stride(0) // 2


def set_planes_format(ctx, fmt):
    """0: bf16 pairs (bf16x3 arithmetic); 1: P16 (IEEE half + two e5m2 bytes; f16c8 arithmetic).  See pp_ctx_set_planes_format."""
    check(lib.pp_ctx_set_planes_format(ctx.handle, int(fmt)), ctx.handle, "pp_ctx_set_planes_format")
    ctx.planes_fmt = int(fmt)


def convert_planes(ctx, src, src_fmt, dst, dst_fmt, scale2=None, scale_index=0, relu_src_hi=None):
    """re-encode a plane pair into the other format (dst = src * scale2[scale_index] when scale2 is given; zero where the tensor
    with hi plane relu_src_hi is not positive)"""
    n = src[0].numel()
    check(lib.pp_convert_planes(ctx.handle, n, _ptr(src[0]), _ptr(src[1]), int(src_fmt), _ptr(dst[0]), _ptr(dst[1]), int(dst_fmt), _ptr(scale2),
                                int(scale_index), _ptr(relu_src_hi)), ctx.handle, "pp_convert_planes")


def planes_to_f32(planes, fmt=0):
    """the values of a plane pair as a float32 tensor [rows, ld] (torch arithmetic: tests / inspection).  fmt 0: bf16 pairs, hi + lo;
    fmt 1 (P16): hi = IEEE halves, the lo unit of a gathered-operand tensor is [e5m2(x) | e5m2(remainder * 2^12) << 8]."""
    hi, lo = planes
    rows = hi.shape[0]
    if fmt == 0:
        return (hi.contiguous().view(torch.bfloat16).float() + lo.contiguous().view(torch.bfloat16).float()).reshape(rows, -1)
    rem = (lo.contiguous().to(torch.int32) & 0xff00).to(torch.int16).view(torch.float16).float() / 4096.0
    return (hi.contiguous().view(torch.float16).float() + rem).reshape(rows, -1)


def weight_planes_to_f32(hi, lo, fmt=0):
    """the same for weight planes (P16: the lo unit's bytes are swapped, the remainder is its LOW byte)"""
    if fmt == 0:
        return hi.contiguous().view(torch.bfloat16).float() + lo.contiguous().view(torch.bfloat16).float()
    rem = ((lo.contiguous().to(torch.int32) & 0xff) << 8).to(torch.int16).view(torch.float16).float() / 4096.0
    return hi.contiguous().view(torch.float16).float() + rem


def split_planes3(ctx, src, hi, lo, scale=None):
    """scale: device float32 [2] = {2^G, 2^-G} (grad_scale_from_counts): the planes hold src * 2^G"""
    if scale is None:
        check(lib.pp_split_planes_bf16x3(ctx.handle, src.numel(), _ptr(src), _ptr(hi), _ptr(lo)), ctx.handle, "pp_split_planes_bf16x3")
    else:
        check(lib.pp_split_planes_scaled_bf16x3(ctx.handle, src.numel(), _ptr(src), _ptr(hi), _ptr(lo), _ptr(scale)), ctx.handle,
              "pp_split_planes_scaled_bf16x3")


def grad_scale_from_counts(ctx, counts, scale2, log2_adjust=0):
    check(lib.pp_grad_scale_from_counts_adj(ctx.handle, _ptr(counts), int(counts.numel()), _ptr(scale2), int(log2_adjust)), ctx.handle,
          "pp_grad_scale_from_counts")


def set_grad_scale(ctx, scale2):
    """persistent: the weight gradients of this context divide the gradient scale out (None: gradients are unscaled)"""
    ctx._grad_scale_keep = scale2
    check(lib.pp_ctx_set_grad_scale(ctx.handle, _ptr(scale2)), ctx.handle, "pp_ctx_set_grad_scale")


def row_block_list(ctx, x, cols, flags=None, blocks=None):
    """pp_row_block_list: x float32 [rows, ld] -> (flags uint8 [2 nb], list int32 [2 (1 + nb)]) with nb = ceil(rows / 32);
    the first halves hold the result, the second halves are scratch of the bwd-data launch that takes the hint."""
    rows, ld = x.shape
    nb = (rows + 31) // 32
    if flags is None:
        flags = torch.zeros((2 * nb,), dtype=torch.uint8, device=x.device)
    if blocks is None:
        blocks = torch.zeros((2 * (nb + 1),), dtype=torch.int32, device=x.device)
    check(lib.pp_row_block_list(ctx.handle, _ptr(x), rows, x.stride(0), int(cols), _ptr(flags), _ptr(blocks)), ctx.handle, "pp_row_block_list")
    return flags, blocks


def row_block_list_planes(ctx, planes, cols, flags, blocks, within=None):
    """pp_row_block_list_planes(_within): the same scan of a tensor stored as bf16 (hi, lo) planes [rows, ld]; within = uint8 flags of
    the only blocks that can hold a non-zero (the others are not read)"""
    hi, lo = planes
    rows = hi.shape[0]
    if within is not None:
        assert within.dtype == torch.uint8 and within.is_contiguous() and within.numel() >= (rows + 31) // 32
        check(lib.pp_row_block_list_planes_within(ctx.handle, _ptr(hi), _ptr(lo), rows, planes_ld(planes), int(cols), _ptr(within), _ptr(flags),
                                                  _ptr(blocks)), ctx.handle, "pp_row_block_list_planes_within")
    else:
        check(lib.pp_row_block_list_planes(ctx.handle, _ptr(hi), _ptr(lo), rows, planes_ld(planes), int(cols), _ptr(flags), _ptr(blocks)),
              ctx.handle, "pp_row_block_list_planes")
    return flags, blocks


def tview(t=None, planes=None):
    """pp_tview of a float32 tensor and / or a (hi, lo) plane pair; None, None = the NULL view"""
    v = TView()
    v.f32 = t.data_ptr() if t is not None else None
    v.hi = planes[0].data_ptr() if planes is not None else None
    v.lo = planes[1].data_ptr() if planes is not None else None
    v._keep = (t, planes)
    return v


def _numel(v):
    t, planes = v._keep
    return (t if t is not None else planes[0]).numel()


def add_n_v(ctx, a, b, c, out):
    null = TView()
    check(lib.pp_add_n_v(ctx.handle, _numel(a), C.byref(a), C.byref(b if b is not None else null), C.byref(c if c is not None else null),
                         C.byref(out)), ctx.handle, "pp_add_n_v")


def relu_fwd_v(ctx, x, y):
    check(lib.pp_relu_fwd_v(ctx.handle, _numel(x), C.byref(x), C.byref(y)), ctx.handle, "pp_relu_fwd_v")


def upsample_add_fwd_v(ctx, n_img, sh, sw, th, tw, c, src, other, out):
    null = TView()
    check(lib.pp_upsample_nearest_add_fwd_v(ctx.handle, n_img, sh, sw, th, tw, c, C.byref(src), C.byref(other if other is not None else null),
                                            C.byref(out)), ctx.handle, "pp_upsample_nearest_add_fwd_v")


def upsample_add_bwd_v(ctx, n_img, sh, sw, th, tw, c, dtarget, base, dsrc):
    null = TView()
    check(lib.pp_upsample_nearest_add_bwd_v(ctx.handle, n_img, sh, sw, th, tw, c, C.byref(dtarget), C.byref(base if base is not None else null),
                                            C.byref(dsrc)), ctx.handle, "pp_upsample_nearest_add_bwd_v")


def merge_planes3(ctx, planes, dst):
    check(lib.pp_merge_planes_bf16x3(ctx.handle, dst.numel(), _ptr(planes[0]), _ptr(planes[1]), _ptr(dst)), ctx.handle, "pp_merge_planes_bf16x3")


def planes_stats(ctx, planes, cols, stats, within=None):
    """pp_planes_stats: adds (elements, non-zero, at the clamp, subnormal) of a P16 tensor's halves to stats[0..3] and keeps the largest
    |half| (15 bits) in stats[4] (int64 [5], device);
    ctx must be the P16 twin; within = uint8 flags of the 32-row blocks to look at"""
    hi, lo = planes
    check(lib.pp_planes_stats(ctx.handle, _ptr(hi), _ptr(lo), int(hi.shape[0]), planes_ld(planes), int(cols), _ptr(within), _ptr(stats)), ctx.handle,
          "pp_planes_stats")
    return stats


def positive_row_blocks(ctx, rs, n_anchor, y_true, flags):
    """pp_positive_row_blocks: flags[b] = 1 where the 32-row block b of the row space rs holds an anchor with state 1
    (y_true [B, N, stride], state = last column)"""
    check(lib.pp_positive_row_blocks(ctx.handle, C.byref(rs), int(n_anchor), int(y_true.shape[-1]), _ptr(y_true), _ptr(flags)), ctx.handle,
          "pp_positive_row_blocks")
    return flags


def row_block_dilate(ctx, d, in_flags, out_flags):
    """pp_row_block_dilate: the blocks within one pixel (2-D) of a flagged block, on the grid of the 3x3 stride-1 conv d"""
    check(lib.pp_row_block_dilate(ctx.handle, C.byref(d), _ptr(in_flags), _ptr(out_flags)), ctx.handle, "pp_row_block_dilate")
    return out_flags


def _conv_opts(capture=None, add=None, mask_hi=None, skip=None, out=None, lazy_out=False, lazy_in=False):
    """the pp_conv_opts of one launch (include/pyrapose_hip.h); NULL when no option is given.  The library checks the combination."""
    if capture is None and add is None and mask_hi is None and skip is None and out is None and not (lazy_out or lazy_in):
        return None
    o = ConvOpts()
    o.capture_hi, o.capture_lo = map(_ptr, capture or (None, None))
    o.add_hi, o.add_lo = map(_ptr, add or (None, None))
    o.mask_hi = _ptr(mask_hi)
    o.skip_flags, o.skip_list = map(_ptr, skip or (None, None))
    o.out_flags, o.out_list = map(_ptr, out or (None, None))
    o.lazy_out, o.lazy_in = int(bool(lazy_out)), int(bool(lazy_in))
    return C.byref(o)


def conv_fwd3(ctx, d, x, w_hi, w_lo, bias, residual, relu, y, x_planes=None, y_planes=None, x_capture=None, res_planes=None,
              out_blocks=None):
    """x_capture = (hi, lo): the launch also writes the bf16 split of x (pp_conv_opts.capture_hi / capture_lo).
    res_planes = (hi, lo): the residual as planes (pp_conv_opts.add_hi / add_lo; `residual` must then be None).
    out_blocks = (flags, list): only the flagged 32-row output blocks are computed (pp_conv_opts.out_flags; list = scratch)."""
    ld_res = residual.stride(0) if residual is not None else (planes_ld(res_planes) if res_planes is not None else 0)
    xh, xl = x_planes if x_planes is not None else (None, None)
    yh, yl = y_planes if y_planes is not None else (None, None)
    check(lib.pp_conv2d_nhwc_fwd_bf16x3(ctx.handle, C.byref(d), _ptr(x), _ptr(xh), _ptr(xl), _ptr(w_hi), _ptr(w_lo), _ptr(bias),
                                        _ptr(residual), ld_res, int(bool(relu)), _ptr(y), _ptr(yh), _ptr(yl),
                                        _conv_opts(capture=x_capture, add=res_planes, out=out_blocks)), ctx.handle,
          "pp_conv2d_nhwc_fwd_bf16x3")


def conv_bwd_data3(ctx, d, dy, w_hi, w_lo, addend, relu_src, dx, dy_planes=None, dx_planes=None, dy_capture=None, dy_skip=None,
                   addend_planes=None, relu_src_hi=None, lazy_out=False, lazy_in=False):
    """dy_capture = (hi, lo): the launch also writes the bf16 split of dy (pp_conv_opts.capture_hi / capture_lo).
    dy_skip = (flags, list) from row_block_list(dy): tiles that only see zero blocks of dy skip their reduction.
    addend_planes = (hi, lo) / relu_src_hi = hi plane: those epilogue operands as planes (pp_conv_opts.add_hi / add_lo / mask_hi).
    lazy_out / lazy_in: pp_conv_opts.lazy_out / lazy_in (dx is left unwritten outside the computed blocks / dy is such a tensor)."""
    ld_add = addend.stride(0) if addend is not None else (planes_ld(addend_planes) if addend_planes is not None else 0)
    ld_rs = relu_src.stride(0) if relu_src is not None else (relu_src_hi.stride(0) // 2 if relu_src_hi is not None else 0)
    dh, dl = dy_planes if dy_planes is not None else (None, None)
    xh, xl = dx_planes if dx_planes is not None else (None, None)
    check(lib.pp_conv2d_nhwc_bwd_data_bf16x3(ctx.handle, C.byref(d), _ptr(dy), _ptr(dh), _ptr(dl), _ptr(w_hi), _ptr(w_lo), _ptr(addend),
                                             ld_add, _ptr(relu_src), ld_rs, _ptr(dx), _ptr(xh), _ptr(xl),
                                             _conv_opts(capture=dy_capture, add=addend_planes, mask_hi=relu_src_hi, skip=dy_skip,
                                                        lazy_out=lazy_out, lazy_in=lazy_in)), ctx.handle,
          "pp_conv2d_nhwc_bwd_data_bf16x3")


def conv_bwd_data3_s2(ctx, d, dy, w_hi, w_lo, addend, relu_src, dx, dy_planes=None, dx_planes=None, addend_planes=None, relu_src_hi=None):
    """pp_conv2d_nhwc_bwd_data_s2_bf16x3: the stride-2 data gradient with all parity classes in one launch -- the operands of
    conv_bwd_data3 (all float32 or all planes; no capture, no row-block skip) and bit for bit its result; any other call fails."""
    ld_add = addend.stride(0) if addend is not None else (planes_ld(addend_planes) if addend_planes is not None else 0)
    ld_rs = relu_src.stride(0) if relu_src is not None else (relu_src_hi.stride(0) // 2 if relu_src_hi is not None else 0)
    dh, dl = dy_planes if dy_planes is not None else (None, None)
    xh, xl = dx_planes if dx_planes is not None else (None, None)
    check(lib.pp_conv2d_nhwc_bwd_data_s2_bf16x3(ctx.handle, C.byref(d), _ptr(dy), _ptr(dh), _ptr(dl), _ptr(w_hi), _ptr(w_lo), _ptr(addend),
                                                ld_add, _ptr(relu_src), ld_rs, _ptr(dx), _ptr(xh), _ptr(xl),
                                                _conv_opts(add=addend_planes, mask_hi=relu_src_hi)), ctx.handle,
          "pp_conv2d_nhwc_bwd_data_s2_bf16x3")


def conv_s2_merged():
    """pp_conv_s2_merged: False under PP_CONV3_S2MERGED=0 (the Engine then keeps conv_bwd_data3 for its stride-2 data gradients)"""
    return bool(lib.pp_conv_s2_merged())


def conv_bwd_weight3(ctx, d, x, dy, dw, dbias, x_planes=None, dy_planes=None, dy_skip=None, lazy_in=False):
    """dy_skip = (flags, list) from row_block_list(dy): the reduction walks the listed 32-row blocks only.
    lazy_in: dy is unwritten outside those blocks (pp_conv_opts.lazy_in): fails unless the listed-block reduction runs."""
    xh, xl = x_planes if x_planes is not None else (None, None)
    dh, dl = dy_planes if dy_planes is not None else (None, None)
    check(lib.pp_conv2d_nhwc_bwd_weight_bf16x3(ctx.handle, C.byref(d), _ptr(x), _ptr(dy), _ptr(xh), _ptr(xl), _ptr(dh), _ptr(dl),
                                               _ptr(dw), _ptr(dbias), _conv_opts(skip=dy_skip, lazy_in=lazy_in)), ctx.handle,
          "pp_conv2d_nhwc_bwd_weight_bf16x3")


def maxpool3x3s2(ctx, n_img, h, w, c, x, oh, ow, y):
    check(lib.pp_maxpool3x3s2_fwd(ctx.handle, n_img, h, w, c, _ptr(x), oh, ow, _ptr(y)), ctx.handle, "pp_maxpool3x3s2_fwd")


def upsample_add_fwd(ctx, n_img, sh, sw, th, tw, c, src, other, out):
    check(lib.pp_upsample_nearest_add_fwd(ctx.handle, n_img, sh, sw, th, tw, c, _ptr(src), _ptr(other), _ptr(out)),
          ctx.handle, "pp_upsample_nearest_add_fwd")


def upsample_add_bwd(ctx, n_img, sh, sw, th, tw, c, dtarget, base, dsrc):
    check(lib.pp_upsample_nearest_add_bwd(ctx.handle, n_img, sh, sw, th, tw, c, _ptr(dtarget), _ptr(base), _ptr(dsrc)),
          ctx.handle, "pp_upsample_nearest_add_bwd")


def add_n(ctx, a, b, c, out):
    check(lib.pp_add_n(ctx.handle, a.numel(), _ptr(a), _ptr(b), _ptr(c), _ptr(out)), ctx.handle, "pp_add_n")


def relu_fwd(ctx, x, y):
    check(lib.pp_relu_fwd(ctx.handle, x.numel(), _ptr(x), _ptr(y)), ctx.handle, "pp_relu_fwd")


def warp_affine_u8(ctx, images_u8, matrices, interpolation="linear", border="replicate", cval=0, out=None):
    """cv2.warpAffine per image of a uint8 batch [B,H,W,3] or [B,H,W] (utils/image.py:207-214, :222-229): matrices = B forward
    2x3 (or 3x3) matrices on the host; interpolation 'linear' / 'nearest'; border 'replicate' ('nearest' fill mode) / 'constant'."""
    B, H, W = images_u8.shape[:3]
    ch = images_u8.shape[3] if images_u8.dim() == 4 else 1
    m = np.ascontiguousarray(np.asarray(matrices, np.float64).reshape(B, -1)[:, :6])
    if out is None:
        out = torch.empty_like(images_u8)
    check(lib.pp_warp_affine_u8(ctx.handle, B, H, W, ch, m.ctypes.data_as(C.POINTER(C.c_double)), {"nearest": 0, "linear": 1}[interpolation],
                                {"constant": 0, "replicate": 1}[border], int(cval), _ptr(images_u8), _ptr(out)), ctx.handle, "pp_warp_affine_u8")
    return out


def photo_augment_u8(ctx, images_u8, programs, out=None):
    """The photometric chain of utils/image.py:154-191 per image of a uint8 BGR batch [B,H,W,3]: programs = a
    utils.photometric.PhotoPrograms of B op lists (compile_chain / sample_programs).  Enqueues on the context's stream, which
    must be torch's current stream: the table pool goes up with a non-blocking torch copy from pinned memory, so torch's host
    allocator knows when the pinned block may be reused -- `programs` may be dropped as soon as this returns."""
    if images_u8.dim() != 4:
        raise ValueError("photo_augment_u8: a [B,H,W,3] batch, got %s" % (tuple(images_u8.shape),))
    B, H, W, ch = images_u8.shape
    assert images_u8.dtype == torch.uint8 and images_u8.is_contiguous()
    if len(programs) != B:
        raise ValueError("photo_augment_u8: %d programs for %d images" % (len(programs), B))
    if out is None:
        out = torch.empty_like(images_u8)
    nbytes = int(programs.pool.size)
    pool_dev = programs.pinned_pool().to(images_u8.device, non_blocking=True)
    ws = torch.empty(lib.pp_photo_workspace_bytes(B, H, W), dtype=torch.uint8, device=images_u8.device)
    offs, recs = programs.op_offsets, programs.ops
    check(lib.pp_photo_augment_u8(ctx.handle, B, H, W, ch, offs.ctypes.data, recs.ctypes.data if recs.size else None,
                                  programs.pool.ctypes.data if nbytes else None, nbytes, _ptr(pool_dev), _ptr(images_u8), _ptr(out), _ptr(ws),
                                  ws.numel()), ctx.handle, "pp_photo_augment_u8")
    return out


def resize_scale(rows, cols, min_side=480, max_side=640):
    s = C.c_double(0)
    check(lib.pp_resize_scale(int(rows), int(cols), int(min_side), int(max_side), C.byref(s)), None, "pp_resize_scale")
    return s.value


def resize_linear_u8(ctx, images_u8, scale):
    """cv2.resize(img, None, fx=scale, fy=scale) of a uint8 batch [B,H,W,3] or [B,H,W] (utils/image.py:307-323)."""
    B, H, W = images_u8.shape[:3]
    ch = images_u8.shape[3] if images_u8.dim() == 4 else 1
    dh, dw = int(np.rint(H * scale)), int(np.rint(W * scale))
    out = torch.empty((B, dh, dw) + ((ch,) if images_u8.dim() == 4 else ()), dtype=torch.uint8, device=images_u8.device)
    check(lib.pp_resize_linear_u8(ctx.handle, B, H, W, ch, float(scale), dh, dw, _ptr(images_u8), _ptr(out)), ctx.handle, "pp_resize_linear_u8")
    return out


def preprocess_caffe_u8(ctx, images_u8, sizes_hw, x4):
    """images_u8: cuda uint8 [B,H,W,3]; sizes_hw: B (h, w) pairs; x4: cuda float32 [B*H*W, 4] (the engine's stem input)."""
    Bn, H, W, _ = images_u8.shape
    assert images_u8.dtype == torch.uint8 and images_u8.is_contiguous()
    arr = (C.c_int * (2 * Bn))(*[int(v) for hw in sizes_hw for v in hw])
    check(lib.pp_preprocess_caffe_u8(ctx.handle, Bn, H, W, arr, _ptr(images_u8), _ptr(x4)), ctx.handle, "pp_preprocess_caffe_u8")


def pack_rgb_to_4_padded(ctx, x3, x4p, Hp, Wp, pad=3):
    Bn, H, W, _ = x3.shape
    check(lib.pp_pack_rgb_to_4_padded(ctx.handle, Bn, H, W, Hp, Wp, pad, _ptr(x3), _ptr(x4p)), ctx.handle, "pp_pack_rgb_to_4_padded")


def preprocess_caffe_u8_padded(ctx, images_u8, sizes_hw, x4p, Hp, Wp, pad=3):
    Bn, H, W, _ = images_u8.shape
    assert images_u8.dtype == torch.uint8 and images_u8.is_contiguous()
    arr = (C.c_int * (2 * Bn))(*[int(v) for hw in sizes_hw for v in hw])
    check(lib.pp_preprocess_caffe_u8_padded(ctx.handle, Bn, H, W, Hp, Wp, pad, arr, _ptr(images_u8), _ptr(x4p)), ctx.handle,
          "pp_preprocess_caffe_u8_padded")


def stem7x7s2_fwd3(ctx, n_img, H, W, Hp, Wp, x4p, w_hi, w_lo, cout, bias, relu, y):
    check(lib.pp_stem7x7s2_fwd_bf16x3(ctx.handle, n_img, H, W, Hp, Wp, _ptr(x4p), _ptr(w_hi), _ptr(w_lo), cout, _ptr(bias), int(bool(relu)),
                                      _ptr(y), y.stride(0)), ctx.handle, "pp_stem7x7s2_fwd_bf16x3")


def pack_rgb_to_4(ctx, x3, x4):
    check(lib.pp_pack_rgb_to_4(ctx.handle, x3.numel() // 3, _ptr(x3), _ptr(x4)), ctx.handle, "pp_pack_rgb_to_4")


def export_head(ctx, rs, n_anchor, n_val, src, apply_sigmoid, out):
    check(lib.pp_export_head(ctx.handle, C.byref(rs), n_anchor, n_val, _ptr(src), src.stride(0), int(apply_sigmoid), _ptr(out)),
          ctx.handle, "pp_export_head")


def count_positives(ctx, y_box, y_cls, y_mask, counts):
    rb = y_box.shape[0] * y_box.shape[1] if y_box is not None else 0
    rc = y_cls.shape[0] * y_cls.shape[1] if y_cls is not None else 0
    rm = y_mask.shape[0] * y_mask.shape[1] if y_mask is not None else 0
    cc = y_cls.shape[2] - 1 if y_cls is not None else 0
    cm = y_mask.shape[2] - 1 if y_mask is not None else 0
    check(lib.pp_count_positives(ctx.handle, rb, _ptr(y_box), rc, cc, _ptr(y_cls), rm, cm, _ptr(y_mask), _ptr(counts)),
          ctx.handle, "pp_count_positives")


def focal(ctx, rs, n_anchor, n_class, logits, y_true, alpha, gamma, count, loss_weight, loss_sum, dlogits):
    check(lib.pp_sigmoid_focal_fwd_bwd(ctx.handle, C.byref(rs), n_anchor, n_class, _ptr(logits), logits.stride(0),
                                       _ptr(y_true), alpha, gamma, _ptr(count), loss_weight, _ptr(loss_sum), _ptr(dlogits)),
          ctx.handle, "pp_sigmoid_focal_fwd_bwd")


def orth_l1(ctx, rs, n_anchor, pred, y_true, weight, sigma, count, loss_weight, loss_sum, dpred):
    check(lib.pp_orth_smoothl1_fwd_bwd(ctx.handle, C.byref(rs), n_anchor, _ptr(pred), pred.stride(0), _ptr(y_true), weight,
                                       sigma, _ptr(count), loss_weight, _ptr(loss_sum), _ptr(dpred)),
          ctx.handle, "pp_orth_smoothl1_fwd_bwd")


class Optimizer:
    def __init__(self, ctx, descs, total):
        arr = (ParamDesc * len(descs))(*descs)
        self.handle = C.c_void_p()
        self.ctx = ctx
        check(lib.pp_optimizer_create(ctx.handle, C.byref(self.handle), arr, len(descs), total), ctx.handle,
              "pp_optimizer_create")

    def grad_norm(self, w_master, g_eff, scales, gnorm_sq, l2_loss=None):
        check(lib.pp_grad_global_norm(self.ctx.handle, self.handle, _ptr(w_master), _ptr(g_eff), _ptr(scales),
                                      _ptr(gnorm_sq), _ptr(l2_loss)), self.ctx.handle, "pp_grad_global_norm")

    def adam_step(self, w_master, w_eff, g_eff, scales, m, v, gnorm_sq, lr, beta1, beta2, eps, clipnorm, step):
        check(lib.pp_adam_step_clipnorm(self.ctx.handle, self.handle, _ptr(w_master), _ptr(w_eff), _ptr(g_eff), _ptr(scales),
                                        _ptr(m), _ptr(v), _ptr(gnorm_sq), lr, beta1, beta2, eps, clipnorm, int(step)),
              self.ctx.handle, "pp_adam_step_clipnorm")

    def close(self):
        if self.handle:
            lib.pp_optimizer_destroy(self.handle)
            self.handle = C.c_void_p()


# ---- anchors / targets / decode -------------------------------------------------------------------
def _iarr(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def generate_base_anchors(base_size, ratios, scales):
    r = np.ascontiguousarray(ratios, np.float32)
    s = np.ascontiguousarray(scales, np.float32)
    out = np.empty((len(r) * len(s), 4), np.float64)
    check(lib.pp_generate_base_anchors_host(int(base_size), r.ctypes.data_as(C.POINTER(C.c_float)), len(r),
                                            s.ctypes.data_as(C.POINTER(C.c_float)), len(s),
                                            out.ctypes.data_as(C.POINTER(C.c_double))), None, "pp_generate_base_anchors_host")
    return out


def anchors_shift(ctx, feat_shapes, strides, base_anchors, dtype=torch.float64):
    """feat_shapes: [(h, w)] per level; base_anchors: float64 [L, A, 4] (numpy)."""
    base = np.ascontiguousarray(base_anchors, np.float64)
    L, A = base.shape[0], base.shape[1]
    n = sum(h * w for h, w in feat_shapes) * A
    out = torch.empty((n, 4), dtype=dtype, device="cuda")
    fn = lib.pp_anchors_shift_f64 if dtype == torch.float64 else lib.pp_anchors_shift_f32
    check(fn(ctx.handle, L, _iarr([h for h, _ in feat_shapes]), _iarr([w for _, w in feat_shapes]), _iarr(strides), A,
             base.ctypes.data_as(C.POINTER(C.c_double)), _ptr(out)), ctx.handle, "pp_anchors_shift")
    return out


def compute_overlap(ctx, boxes, query):
    n, k = boxes.shape[0], query.shape[0]
    out = torch.zeros((n, k), dtype=torch.float64, device="cuda")
    check(lib.pp_compute_overlap_f64(ctx.handle, n, _ptr(boxes), k, _ptr(query), _ptr(out)), ctx.handle, "pp_compute_overlap_f64")
    return out


def compute_gt_annotations(ctx, anchors, gt, neg=0.4, pos=0.5):
    n, k = anchors.shape[0], gt.shape[0]
    argmax = torch.empty((n,), dtype=torch.int32, device="cuda")
    state = torch.empty((n,), dtype=torch.int8, device="cuda")
    check(lib.pp_compute_gt_annotations(ctx.handle, n, _ptr(anchors), k, _ptr(gt), neg, pos, _ptr(argmax), _ptr(state)),
          ctx.handle, "pp_compute_gt_annotations")
    return argmax, state


def project_box3d(pose7, box8x3, cam4):
    p = np.ascontiguousarray(pose7, np.float64)
    b = np.ascontiguousarray(box8x3, np.float64)
    c = np.ascontiguousarray(cam4, np.float64)
    out = np.empty(16, np.float64)
    dp = C.POINTER(C.c_double)
    check(lib.pp_project_box3d_host(p.ctypes.data_as(dp), b.ctypes.data_as(dp), c.ctypes.data_as(dp), out.ctypes.data_as(dp)),
          None, "pp_project_box3d_host")
    return out


def pil_nearest_index(n_in, n_out):
    out = np.empty(n_out, np.int32)
    check(lib.pp_pil_nearest_index_host(n_in, n_out, out.ctypes.data_as(C.POINTER(C.c_int))), None, "pp_pil_nearest_index_host")
    return out


def anchor_targets(ctx, anchors, gt_offset, gt_boxes, gt_labels, gt_box3d, gt_mask_ids, id_masks, mask_hw, image_hw,
                   num_classes, out_mh, out_mw, neg=0.4, pos=0.5):
    """anchors: cuda f64 [N,4]; gt_* cuda tensors packed over the batch; id_masks cuda uint8 [B,H,W] or None."""
    B = len(gt_offset) - 1
    N = anchors.shape[0]
    reg = torch.empty((B, N, 17), dtype=torch.float32, device="cuda")
    lab = torch.empty((B, N, num_classes + 1), dtype=torch.float32, device="cuda")
    msk = torch.empty((B, out_mh * out_mw, num_classes + 1), dtype=torch.float32, device="cuda")
    mh, mw = (id_masks.shape[1], id_masks.shape[2]) if id_masks is not None else (0, 0)
    check(lib.pp_anchor_targets(ctx.handle, N, _ptr(anchors), B, _iarr(gt_offset), _ptr(gt_boxes), _ptr(gt_labels),
                                _ptr(gt_box3d), _ptr(gt_mask_ids), _ptr(id_masks), mh, mw,
                                _iarr(np.asarray(mask_hw).reshape(-1)) if mask_hw is not None else None,
                                _iarr(np.asarray(image_hw).reshape(-1)), num_classes, neg, pos, out_mh, out_mw,
                                _ptr(reg), _ptr(lab), _ptr(msk)), ctx.handle, "pp_anchor_targets")
    return reg, lab, msk


def box3d_decode(ctx, anchors_f32, regression):
    B, N = regression.shape[0], regression.shape[1]
    out = torch.empty_like(regression)
    check(lib.pp_box3d_decode(ctx.handle, B, N, _ptr(anchors_f32), _ptr(regression), _ptr(out)), ctx.handle, "pp_box3d_decode")
    return out


def score_threshold_compact(ctx, scores, thr=0.5, cap=None):
    B, N, Cc = scores.shape
    cap = int(cap or N)
    idx = torch.empty((B, Cc, cap), dtype=torch.int32, device="cuda")
    cnt = torch.empty((B, Cc), dtype=torch.int32, device="cuda")
    check(lib.pp_score_threshold_compact(ctx.handle, B, N, Cc, _ptr(scores), thr, cap, _ptr(idx), _ptr(cnt)), ctx.handle,
          "pp_score_threshold_compact")
    return idx, cnt


def filter_detections_batch(ctx, boxes, boxes3d, scores, score_thr=0.05, iou_thr=0.5, max_det=300):
    """boxes [B,N,4], boxes3d [B,N,16], scores [B,N,C] -> ([B,max_det,4], [B,max_det,16], [B,max_det], [B,max_det] int32)."""
    Bn, N, Cc = scores.shape
    ws = torch.empty((Bn * lib.pp_filter_workspace_bytes(N, Cc, max_det),), dtype=torch.uint8, device="cuda")
    ob = torch.empty((Bn, max_det, 4), dtype=torch.float32, device="cuda")
    o3 = torch.empty((Bn, max_det, 16), dtype=torch.float32, device="cuda")
    osc = torch.empty((Bn, max_det), dtype=torch.float32, device="cuda")
    ol = torch.empty((Bn, max_det), dtype=torch.int32, device="cuda")
    check(lib.pp_filter_detections_batch(ctx.handle, Bn, N, Cc, _ptr(boxes), _ptr(boxes3d), _ptr(scores), score_thr, iou_thr, max_det,
                                         _ptr(ws), _ptr(ob), _ptr(o3), _ptr(osc), _ptr(ol)), ctx.handle, "pp_filter_detections_batch")
    return ob, o3, osc, ol


def filter_detections(ctx, boxes, boxes3d, scores, score_thr=0.05, iou_thr=0.5, max_det=300):
    N, Cc = scores.shape
    ws = torch.empty((lib.pp_filter_workspace_bytes(N, Cc, max_det),), dtype=torch.uint8, device="cuda")
    ob = torch.empty((max_det, 4), dtype=torch.float32, device="cuda")
    o3 = torch.empty((max_det, 16), dtype=torch.float32, device="cuda")
    osc = torch.empty((max_det,), dtype=torch.float32, device="cuda")
    ol = torch.empty((max_det,), dtype=torch.int32, device="cuda")
    check(lib.pp_filter_detections(ctx.handle, N, Cc, _ptr(boxes), _ptr(boxes3d), _ptr(scores), score_thr, iou_thr, max_det,
                                   _ptr(ws), _ptr(ob), _ptr(o3), _ptr(osc), _ptr(ol)), ctx.handle, "pp_filter_detections")
    return ob, o3, osc, ol


# The pose tail (everything below): every argument error is a ValueError raised before anything is enqueued.  The wrappers share
# one tensor check (_arg), one offsets check (_check_offsets), one workspace allocation (_workspace) and one output allocation (_out).

_F32, _F64, _I32, _U8 = torch.float32, torch.float64, torch.int32, torch.uint8


def _arg(what, name, t, dtype, shape, optional=False):
    """Argument `name` of wrapper `what`: a cuda tensor of `dtype` and `shape` (None: a free dimension) -> t.contiguous();
    None passes where the argument is optional."""
    if t is None and optional:
        return None
    ok = torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and len(t.shape) == len(shape)
    if ok:  # (a plain loop costs less than all() over a generator: the small launches of the tail are host-bound)
        for s, d in zip(shape, t.shape):
            ok = ok and (s is None or s == d)
    if not ok:
        got = "a %s %s tensor %s" % (t.device.type, str(t.dtype)[6:], list(t.shape)) if torch.is_tensor(t) else type(t).__name__
        raise ValueError("%s: %s must be a cuda %s tensor [%s], got %s" %
                         (what, name, str(dtype)[6:], ",".join("*" if s is None else str(s) for s in shape), got))
    return t.contiguous()


def _check_offsets(what, offsets, n_total, check, multiple=1, name="offsets"):
    """offsets int32 [P+1] -> (offsets.contiguous(), their host copy).  With `check` they must rise from 0 to n_total in
    multiples of `multiple`; without it the host-side look (a sync) is skipped and the copy is None."""
    offsets = _arg(what, name, offsets, _I32, (None,))
    if offsets.numel() < 1:
        raise ValueError("%s: %s must hold P+1 >= 1 entries" % (what, name))
    if not check:
        return offsets, None
    o = offsets.cpu().numpy()
    if o[0] != 0 or o[-1] != n_total or (np.diff(o) < 0).any() or (o % multiple != 0).any():
        raise ValueError("%s: %s must rise from 0 to the number of points%s" %
                         (what, name, " in multiples of points_per_vote" if multiple > 1 else ""))
    return offsets, o


def _workspace(nbytes, refused=None):
    """The uint8 workspace a *_workspace_bytes call asks for, at least 1 byte.  0 bytes from an entry point that always needs
    some means the library refuses the shape: ValueError(refused) where given, otherwise the entry point's own check reports it."""
    if nbytes == 0 and refused:
        raise ValueError(refused)
    return torch.empty((max(1, nbytes),), dtype=_U8, device="cuda")


def _out(like, shape, dtype=_F64, fill=None):
    """an output on like's device: uninitialised, or filled with `fill` (one fill kernel)"""
    if fill is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    return torch.full(shape, fill, dtype=dtype, device=like.device)


_POSE_ARGS = (("K9", (3, 3)), ("R_est", (3, 3)), ("t_est", (3,)), ("R_gt", (3, 3)), ("t_gt", (3,)))


def _pose_args(what, pts, poses):
    """pts [n_pts,3] and the poses ([K9,] R_est, t_est, R_gt, t_gt) of one n, in ABI order -> (n, n_pts, checked poses)"""
    n, out = None, []
    for (name, tail), t in zip(_POSE_ARGS[-len(poses):], poses):
        out.append(_arg(what, name, t, _F64, (n,) + tail))
        n = n or int(out[0].shape[0])
    return n, int(pts.shape[0]), out


def _pose_mean(ctx, what, name, pts, *poses):
    """a per-pose mean over model points: entry point `name`, cuda float64 tensors in ABI order (pts [n_pts,3] first) -> float64 [n]"""
    pts = _arg(what, "pts", pts, _F64, (None, 3))
    n, n_pts, poses = _pose_args(what, pts, poses)
    ws = _workspace(lib.pp_pose_error_workspace_bytes(n, n_pts))
    out = _out(pts, (n,))
    check(getattr(lib, name)(ctx.handle, n, n_pts, _ptr(pts), *[_ptr(t) for t in poses], _ptr(ws), _ptr(out)), ctx.handle, name)
    return out


def pose_errors(ctx, pts, R_est, t_est, R_gt, t_gt, symmetric=False):
    """ADD (symmetric=False) or ADD-S / ADI (True) of n poses against one model: cuda float64 tensors
    pts [n_pts,3], R_* [n,3,3], t_* [n,3] -> float64 [n]."""
    return _pose_mean(ctx, "pose_errors", "pp_pose_adi_f64" if symmetric else "pp_pose_add_f64", pts, R_est, t_est, R_gt, t_gt)


def pose_reproj(ctx, pts, K9, R_est, t_est, R_gt, t_gt):
    """Mean 2-D reprojection error of n poses against one model (pp_pose_reproj_f64): cuda float64 tensors pts [n_pts,3],
    K9 [n,3,3], R_* [n,3,3], t_* [n,3] -> float64 [n] (pixels)."""
    return _pose_mean(ctx, "pose_reproj", "pp_pose_reproj_f64", pts, K9, R_est, t_est, R_gt, t_gt)


POSE_SYM_CHUNK = 8     # symmetries per workgroup of the MSSD / MSPD kernel (csrc/pose.hip)
POSE_SYM_RANGE = 2048  # model points per workgroup: every further range of this many points is one more workgroup


def _pose_sym(ctx, what, name, pts, S_R, S_t, poses, best_sym):
    """min over symmetries of a per-pose max over model points: entry point `name`, cuda float64 tensors, poses in ABI order
    ([K9,] R_est, t_est, R_gt, t_gt) -> (float64 [n], int32 [n] or None)."""
    pts = _arg(what, "pts", pts, _F64, (None, 3))
    S_R = _arg(what, "S_R", S_R, _F64, (None, 3, 3))
    n_sym = int(S_R.shape[0])
    S_t = _arg(what, "S_t", S_t, _F64, (n_sym, 3))
    n, n_pts, poses = _pose_args(what, pts, poses)
    ws = _workspace(lib.pp_pose_sym_workspace_bytes(n, n_pts, n_sym))
    out = _out(pts, (n,))
    sym = _out(pts, (n,), _I32) if best_sym else None
    check(getattr(lib, name)(ctx.handle, n, n_pts, n_sym, _ptr(pts), _ptr(S_R), _ptr(S_t), *[_ptr(t) for t in poses], _ptr(ws), _ptr(out),
                             _ptr(sym)), ctx.handle, name)
    return out, sym


def pose_mssd(ctx, pts, S_R, S_t, R_est, t_est, R_gt, t_gt, best_sym=True):
    """BOP's Maximum Symmetry-Aware Surface Distance of n poses against one model and one symmetry set (pp_pose_mssd_f64):
    cuda float64 tensors pts [n_pts,3], S_R [n_sym,3,3], S_t [n_sym,3] (utils.symmetry.stack_symmetries), R_* [n,3,3], t_*
    [n,3] -> (err float64 [n], best_sym int32 [n]: the symmetry attaining the minimum, lowest index on ties; None with
    best_sym=False)."""
    return _pose_sym(ctx, "pose_mssd", "pp_pose_mssd_f64", pts, S_R, S_t, (R_est, t_est, R_gt, t_gt), best_sym)


def pose_mspd(ctx, pts, S_R, S_t, K9, R_est, t_est, R_gt, t_gt, best_sym=True):
    """BOP's Maximum Symmetry-Aware Projection Distance (pp_pose_mspd_f64): as pose_mssd with K9 [n,3,3]; err in pixels."""
    return _pose_sym(ctx, "pose_mspd", "pp_pose_mspd_f64", pts, S_R, S_t, (K9, R_est, t_est, R_gt, t_gt), best_sym)


def pnp_ransac(ctx, offsets, obj, img, K4, iterations=300, reproj_error=5.0, seed=0, points_per_vote=8):
    """Batched RANSAC-PnP (pp_pnp_ransac_f64): cuda tensors offsets int32 [P+1], obj float64 [N,3], img float64 [N,2],
    K4 float64 [P,4] -> (R [P,3,3], t [P,3], n_inliers int32 [P], inlier mask uint8 [N], ok int32 [P]).  The offsets' values are
    not looked at on the host (callers build them on the device)."""
    offsets, _ = _check_offsets("pnp_ransac", offsets, None, False)
    P = int(offsets.numel()) - 1
    obj = _arg("pnp_ransac", "obj", obj, _F64, (None, 3))
    N = int(obj.shape[0])
    img = _arg("pnp_ransac", "img", img, _F64, (N, 2))
    K4 = _arg("pnp_ransac", "K4", K4, _F64, (P, 4))
    ws = _workspace(lib.pp_pnp_ransac_workspace_bytes(P, int(iterations)))
    R, t = _out(obj, (P, 3, 3)), _out(obj, (P, 3))
    n_in, mask, ok = _out(obj, (P,), _I32, 0), _out(obj, (max(N, 1),), _U8, 0), _out(obj, (P,), _I32, 0)
    check(lib.pp_pnp_ransac_f64(ctx.handle, P, _ptr(offsets), N, _ptr(obj), _ptr(img), _ptr(K4), int(iterations), float(reproj_error),
                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(points_per_vote), _ptr(ws), _ptr(R), _ptr(t), _ptr(n_in), _ptr(mask),
                                _ptr(ok)), ctx.handle, "pp_pnp_ransac_f64")
    return R, t, n_in, mask[:N], ok


def render_depth(ctx, verts, faces, R, t, K4, width, height, clip_near=100.0, clip_far=10000.0):
    """Depth images of one mesh at n poses (pp_render_depth_f32): cuda tensors verts float64 [n_vert,3], faces int32
    [n_tri,3], R float64 [n,3,3], t [n,3], K4 [n,4] = (fx, fy, cx, cy) -> float32 [n, height, width], 0 = empty."""
    verts = _arg("render_depth", "verts", verts, _F64, (None, 3))
    faces = _arg("render_depth", "faces", faces, _I32, (None, 3))
    R = _arg("render_depth", "R", R, _F64, (None, 3, 3))
    n, nv, nt = int(R.shape[0]), int(verts.shape[0]), int(faces.shape[0])
    t = _arg("render_depth", "t", t, _F64, (n, 3))
    K4 = _arg("render_depth", "K4", K4, _F64, (n, 4))
    nbytes = lib.pp_render_workspace_bytes(n, nv, nt, int(width), int(height))
    ws = _workspace(nbytes, "render_depth: unsupported shape (n=%d, vertices=%d, triangles=%d, %dx%d)" % (n, nv, nt, width, height))
    out = _out(verts, (n, int(height), int(width)), _F32)
    check(lib.pp_render_depth_f32(ctx.handle, n, nv, _ptr(verts), nt, _ptr(faces), _ptr(R), _ptr(t), _ptr(K4), int(width), int(height),
                                  float(clip_near), float(clip_far), _ptr(ws), nbytes, _ptr(out)), ctx.handle, "pp_render_depth_f32")
    return out


RENDER_SHADING = {"flat": 0, "phong": 1}
RENDER_OUTPUTS = {"depth": _F32, "tri_id": _I32, "rgb_f32": _F32, "rgb": _U8}  # in the ABI's order


RENDER_FILTER = {"nearest": 0, "bilinear": 1}
RENDER_WRAP = {"clamp": 0, "repeat": 1}


def _render_mesh(what, choices, outputs, verts, faces, R, t, K4):
    """what render_rgbd / render_rgbd_tex check first; choices: {kind: (value, its table)} -> (outputs as a tuple, verts, faces,
    R, t, K4, n, n_vert, n_tri)"""
    for kind, (value, table) in choices.items():
        if value not in table:
            raise ValueError("%s: unknown %s %r (%s)" % (what, kind, value, " | ".join(table)))
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    unknown = [o for o in outputs if o not in RENDER_OUTPUTS]
    if unknown or not outputs:
        raise ValueError("%s: outputs must name at least one of %s, got %r" % (what, " | ".join(RENDER_OUTPUTS), outputs))
    verts = _arg(what, "verts", verts, _F64, (None, 3))
    faces = _arg(what, "faces", faces, _I32, (None, 3))
    R = _arg(what, "R", R, _F64, (None, 3, 3))
    n, nv, nt = int(R.shape[0]), int(verts.shape[0]), int(faces.shape[0])
    return outputs, verts, faces, R, _arg(what, "t", t, _F64, (n, 3)), _arg(what, "K4", K4, _F64, (n, 4)), n, nv, nt


def _render_frame(what, outputs, verts, n, nv, nt, width, height, normals, light_cam_pos, bg_color, nbytes, texture=""):
    """and last: -> (normals, light, bg as the ABI takes them, workspace of nbytes, dict of the output tensors)"""
    normals = _arg(what, "normals", normals, _F64, (nv, 3), optional=True)
    light = (C.c_double * 3)(*(float(v) for v in np.asarray(light_cam_pos, np.float64).reshape(3)))
    bg = (C.c_double * 3)(*(float(v) for v in np.asarray(bg_color, np.float64).reshape(3)))
    ws = _workspace(nbytes, "%s: unsupported shape (n=%d, vertices=%d, triangles=%d, %dx%d%s)" % (what, n, nv, nt, width, height, texture))
    out = {k: _out(verts, (n, int(height), int(width)) + ((3,) if k.startswith("rgb") else ()), dt)
           for k, dt in RENDER_OUTPUTS.items() if k in outputs}
    return normals, light, bg, ws, out


def render_rgbd(ctx, verts, faces, R, t, K4, width, height, colors=None, normals=None, clip_near=100.0, clip_far=10000.0,
                shading="phong", ambient_weight=0.5, light_cam_pos=(0.0, 0.0, 0.0), bg_color=(0.0, 0.0, 0.0), outputs=("rgb", "depth")):
    """Shaded colour, depth and triangle ids of one mesh at n poses (pp_render_rgbd): cuda tensors as in render_depth plus
    colors float64 [n_vert,3] in [0, 1] (needed for 'rgb' / 'rgb_f32') and normals float64 [n_vert,3] (needed for phong
    shading); shading 'flat' | 'phong'; light_cam_pos in the OpenCV camera frame; outputs: any of 'rgb' (uint8 [n,h,w,3], RGB),
    'rgb_f32' (float32 [n,h,w,3]), 'depth' (float32 [n,h,w], the bits of render_depth), 'tri_id' (int32 [n,h,w], -1 = none)
    -> dict of the requested outputs."""
    outputs, verts, faces, R, t, K4, n, nv, nt = _render_mesh("render_rgbd", {"shading": (shading, RENDER_SHADING)}, outputs, verts, faces, R, t, K4)
    colors = _arg("render_rgbd", "colors", colors, _F64, (nv, 3), optional=True)
    nbytes = lib.pp_render_rgbd_workspace_bytes(n, nv, nt, int(width), int(height))
    normals, light, bg, ws, out = _render_frame("render_rgbd", outputs, verts, n, nv, nt, width, height, normals, light_cam_pos, bg_color, nbytes)
    check(lib.pp_render_rgbd(ctx.handle, n, nv, _ptr(verts), _ptr(colors), _ptr(normals), nt, _ptr(faces), _ptr(R), _ptr(t), _ptr(K4),
                             int(width), int(height), float(clip_near), float(clip_far), RENDER_SHADING[shading], float(ambient_weight),
                             light, bg, _ptr(ws), nbytes, *[_ptr(out.get(k)) for k in RENDER_OUTPUTS]), ctx.handle, "pp_render_rgbd")
    return out


def render_rgbd_tex(ctx, verts, faces, R, t, K4, width, height, uv=None, tex=None, filter="nearest", wrap="clamp", normals=None,
                    clip_near=100.0, clip_far=10000.0, shading="phong", ambient_weight=0.5, light_cam_pos=(0.0, 0.0, 0.0),
                    bg_color=(0.0, 0.0, 0.0), outputs=("rgb", "depth")):
    """render_rgbd of a textured mesh (pp_render_rgbd_tex): in place of colors, uv float64 [n_vert,2] and tex, a cuda uint8
    tensor [th,tw,4] (RGBX, the rows in the image file's order: v = 0 is its bottom row; the fourth byte is ignored), both
    needed for 'rgb' / 'rgb_f32'; filter 'nearest' | 'bilinear'; wrap 'clamp' | 'repeat'.  Everything else as in render_rgbd."""
    choices = {"shading": (shading, RENDER_SHADING), "filter": (filter, RENDER_FILTER), "wrap": (wrap, RENDER_WRAP)}
    outputs, verts, faces, R, t, K4, n, nv, nt = _render_mesh("render_rgbd_tex", choices, outputs, verts, faces, R, t, K4)
    uv = _arg("render_rgbd_tex", "uv", uv, _F64, (nv, 2), optional=True)
    tex = _arg("render_rgbd_tex", "tex", tex, _U8, (None, None, 4), optional=True)
    th, tw = (int(tex.shape[0]), int(tex.shape[1])) if tex is not None else (1, 1)
    nbytes = lib.pp_render_rgbd_tex_workspace_bytes(n, nv, nt, int(width), int(height), tw, th)
    normals, light, bg, ws, out = _render_frame("render_rgbd_tex", outputs, verts, n, nv, nt, width, height, normals, light_cam_pos, bg_color,
                                                nbytes, ", texture %dx%d" % (tw, th))
    check(lib.pp_render_rgbd_tex(ctx.handle, n, nv, _ptr(verts), _ptr(uv), _ptr(tex), tw, th, RENDER_FILTER[filter], RENDER_WRAP[wrap],
                                 _ptr(normals), nt, _ptr(faces), _ptr(R), _ptr(t), _ptr(K4), int(width), int(height), float(clip_near),
                                 float(clip_far), RENDER_SHADING[shading], float(ambient_weight), light, bg, _ptr(ws), nbytes,
                                 *[_ptr(out.get(k)) for k in RENDER_OUTPUTS]), ctx.handle, "pp_render_rgbd_tex")
    return out


VSD_COSTS = {"step": 0, "tlinear": 1}


def _vsd_args(what, depth_test, depth_est, depth_gt, K4):
    """the tensors of vsd() / vsd_multi(), checked -> (n, h, w, then in ABI order: depth_test, its stride between problems,
    depth_est, depth_gt, K4)"""
    de = _arg(what, "depth_est", depth_est, _F32, (None, None, None))
    n, h, w = (int(s) for s in de.shape)
    dg = _arg(what, "depth_gt", depth_gt, _F32, (n, h, w))
    shared = torch.is_tensor(depth_test) and depth_test.dim() == 2  # one scene [h,w] for all problems, else [n,h,w]
    dt = _arg(what, "depth_test", depth_test, _F32, (h, w) if shared else (n, h, w))
    K4 = _arg(what, "K4", K4, _F64, (n, 4))
    return n, h, w, dt, 0 if shared else h * w, de, dg, K4


def vsd(ctx, depth_test, depth_est, depth_gt, K4, delta, tau, cost_type="step"):
    """Visible Surface Discrepancy of n problems (pp_vsd_f64): cuda float32 depth_est / depth_gt [n,h,w], depth_test [h,w]
    (shared by all problems) or [n,h,w], K4 float64 [n,4] -> (e float64 [n], intersection int64 [n], union int64 [n])."""
    if cost_type not in VSD_COSTS:
        raise ValueError("vsd: unknown pixel matching cost %r (step | tlinear)" % (cost_type,))
    n, h, w, dt, stride, de, dg, K4 = _vsd_args("vsd", depth_test, depth_est, depth_gt, K4)
    ws = _workspace(lib.pp_vsd_workspace_bytes(n, w, h))
    e, inter, uni = _out(de, (n,)), _out(de, (n,), torch.int64), _out(de, (n,), torch.int64)
    check(lib.pp_vsd_f64(ctx.handle, n, w, h, _ptr(dt), stride, _ptr(de), _ptr(dg), _ptr(K4), float(delta), float(tau),
                         VSD_COSTS[cost_type], _ptr(ws), _ptr(e), _ptr(inter), _ptr(uni)), ctx.handle, "pp_vsd_f64")
    return e, inter, uni


VSD_VISIB = {"bop18": 0, "bop19": 1}


def vsd_multi(ctx, depth_test, depth_est, depth_gt, K4, delta, taus, cost_type="step", visib_mode="bop19"):
    """VSD of n problems at T misalignment tolerances in one pass over the pixels (pp_vsd_multi_f64): tensors as in vsd();
    taus: T = 1 ... 16 positive, strictly increasing host values; visib_mode 'bop18' (the rule of vsd()) or 'bop19' (a rendered
    pixel without sensor depth counts as visible) -> (e float64 [n,T], intersection, union, visib_gt, px_gt: int64 [n] each;
    visib_gt / px_gt is the visible fraction of the ground-truth object)."""
    if cost_type not in VSD_COSTS:
        raise ValueError("vsd_multi: unknown pixel matching cost %r (step | tlinear)" % (cost_type,))
    if visib_mode not in VSD_VISIB:
        raise ValueError("vsd_multi: unknown visibility rule %r (bop18 | bop19)" % (visib_mode,))
    taus = np.ascontiguousarray(np.asarray(taus, np.float64).reshape(-1))
    T = int(taus.size)
    n, h, w, dt, stride, de, dg, K4 = _vsd_args("vsd_multi", depth_test, depth_est, depth_gt, K4)
    ws = _workspace(lib.pp_vsd_multi_workspace_bytes(n, w, h, T))
    e = _out(de, (n, T))
    inter, uni, vis, px = (_out(de, (n,), torch.int64) for _ in range(4))
    check(lib.pp_vsd_multi_f64(ctx.handle, n, w, h, _ptr(dt), stride, _ptr(de), _ptr(dg), _ptr(K4), float(delta), T,
                               taus.ctypes.data_as(C.POINTER(C.c_double)), VSD_COSTS[cost_type], VSD_VISIB[visib_mode], _ptr(ws),
                               _ptr(e), _ptr(inter), _ptr(uni), _ptr(vis), _ptr(px)), ctx.handle, "pp_vsd_multi_f64")
    return e, inter, uni, vis, px


SCENE_GT_MAX_INSTANCES = 255  # per scene: the id image is uint8 and 0 is the background
SceneGT = collections.namedtuple("SceneGT", "px_count bbox_obj bbox_visib id_image scene_depth mask_full mask_visib")


def _scene_offsets(what, scene_offsets, S=None):
    """scene_offsets as S+1 host int32 values; S: the number of scenes they must fit, None = any (at least one)"""
    off = np.ascontiguousarray(np.asarray(scene_offsets).reshape(-1), np.int32)
    if (off.size < 2 if S is None else off.size != S + 1) or not np.array_equal(off, np.asarray(scene_offsets).reshape(-1)):
        raise ValueError("%s: scene_offsets must hold S+1 %s integers" % (what, ">= 2" if S is None else "= %d" % (S + 1)))
    return off


def scene_gt_info(ctx, depth_stack, scene_offsets, K4, depth_test=None, delta=15.0, window=None, masks=False):
    """Ground truth of S scenes from the depth renders of their instances (pp_scene_gt_info): cuda float32 depth_stack
    [n,ch,cw] (render_depth outputs stacked in scene order), scene_offsets: S+1 HOST integers rising from 0 to n (scene s owns
    the instances scene_offsets[s] .. scene_offsets[s+1], at most 255), K4 float64 [n,4] in image coordinates; window
    (off_x, off_y, w, h): the image inside the canvas, None = the whole canvas; depth_test: cuda float32 sensor depth [h,w]
    (shared by the scenes) or [S,h,w], None = compose the scene depth from the instances -> SceneGT(px_count int64 [n,3] =
    (all, valid, visib), bbox_obj int32 [n,4], bbox_visib int32 [n,4] as (x, y, w, h), id_image uint8 [S,h,w], scene_depth
    float32 [S,h,w] (None with depth_test), mask_full, mask_visib uint8 [n,h,w] 0 / 255 (None without masks))."""
    stack = _arg("scene_gt_info", "depth_stack", depth_stack, _F32, (None, None, None))
    n, ch, cw = (int(s) for s in stack.shape)
    off = _scene_offsets("scene_gt_info", scene_offsets)
    S = int(off.size) - 1
    ox, oy, w, h = (int(v) for v in (window if window is not None else (0, 0, cw, ch)))
    K4 = _arg("scene_gt_info", "K4", K4, _F64, (n, 4))
    shared = torch.is_tensor(depth_test) and depth_test.dim() == 2
    dt = _arg("scene_gt_info", "depth_test", depth_test, _F32, (h, w) if shared else (S, h, w), optional=True)
    nbytes = lib.pp_scene_gt_workspace_bytes(n, cw, ch)
    ws = _workspace(nbytes)
    shape = (S, max(h, 0), max(w, 0))
    out = SceneGT(_out(stack, (n, 3), torch.int64), _out(stack, (n, 4), _I32), _out(stack, (n, 4), _I32), _out(stack, shape, _U8),
                  _out(stack, shape, _F32) if dt is None else None,
                  *((_out(stack, (n,) + shape[1:], _U8) for _ in range(2)) if masks else (None, None)))
    off_dev = torch.from_numpy(off).to(stack.device)
    check(lib.pp_scene_gt_info(ctx.handle, n, S, off.ctypes.data_as(C.POINTER(C.c_int)), _ptr(off_dev), cw, ch, w, h, ox, oy, _ptr(stack),
                               _ptr(K4), _ptr(dt), 0 if shared else h * w, float(delta), _ptr(ws), nbytes, _ptr(out.scene_depth),
                               _ptr(out.id_image), _ptr(out.px_count), _ptr(out.bbox_obj), _ptr(out.bbox_visib), _ptr(out.mask_full),
                               _ptr(out.mask_visib)), ctx.handle, "pp_scene_gt_info")
    return out


CHANNEL_ORDERS = {"rgb": 0, "bgr": 1}


def scene_compose(ctx, id_image, colors, scene_offsets, background=(0, 0, 0), channel_order="bgr"):
    """The images of S scenes from their instances' colour renders (pp_scene_compose_u8): cuda uint8 id_image [S,h,w]
    (scene_gt_info's, whole canvas), colors [n,h,w,3] (render_rgbd's 'rgb' in scene order), scene_offsets as in scene_gt_info;
    background: a cuda uint8 tensor [S,h,w,3] or three HOST values 0 ... 255 (RGB, as the colours); channel_order of the
    result 'rgb' | 'bgr' -> cuda uint8 [S,h,w,3]."""
    if channel_order not in CHANNEL_ORDERS:
        raise ValueError("scene_compose: unknown channel order %r (rgb | bgr)" % (channel_order,))
    ids = _arg("scene_compose", "id_image", id_image, _U8, (None, None, None))
    S, h, w = (int(s) for s in ids.shape)
    colors = _arg("scene_compose", "colors", colors, _U8, (None, h, w, 3))
    n = int(colors.shape[0])
    off = _scene_offsets("scene_compose", scene_offsets, S)
    bg_image, bg_const = None, None
    if torch.is_tensor(background):
        bg_image = _arg("scene_compose", "background", background, _U8, (S, h, w, 3))
    else:
        bg = np.asarray(background).reshape(-1)
        if bg.size != 3 or not np.array_equal(bg, bg.astype(np.uint8)):
            raise ValueError("scene_compose: a constant background is three values 0 ... 255")
        bg_const = (C.c_ubyte * 3)(*(int(v) for v in bg))
    out = _out(ids, (S, h, w, 3), _U8)
    off_dev = torch.from_numpy(off).to(ids.device)
    check(lib.pp_scene_compose_u8(ctx.handle, n, S, off.ctypes.data_as(C.POINTER(C.c_int)), _ptr(off_dev), w, h, _ptr(ids), _ptr(colors),
                                  _ptr(bg_image), bg_const, CHANNEL_ORDERS[channel_order], _ptr(out)), ctx.handle, "pp_scene_compose_u8")
    return out


ICP_MODES = {"point_to_point": 0, "point_to_plane": 1}
ICP_STATUS = {0: "ok", 1: "too_few_correspondences", 2: "singular"}


def cloud_from_depth(ctx, depth, fx, fy, cx, cy, ds=1.0, mask=None, row_idx=None, col_idx=None, dense=False):
    """Back-projection of a depth image (pp_cloud_from_depth_f64): cuda float32 depth [h,w]; mask cuda uint8 [mh,mw] with cuda
    int32 row_idx [h] / col_idx [w] into it (None = every pixel).  dense: float64 [h*w,3] with all-NaN rows where z == 0;
    otherwise the valid masked pixels compacted in row-major order -> (float64 [n,3], row offsets int32 [h+1])."""
    depth = _arg("cloud_from_depth", "depth", depth, _F32, (None, None))
    h, w = (int(s) for s in depth.shape)
    mask = _arg("cloud_from_depth", "mask", mask, _U8, (None, None), optional=True)
    mh, mw = (int(s) for s in mask.shape) if mask is not None else (0, 0)
    # a mask needs both index maps; without one they are not read
    row_idx = _arg("cloud_from_depth", "row_idx", row_idx, _I32, (h,)) if mask is not None else None
    col_idx = _arg("cloud_from_depth", "col_idx", col_idx, _I32, (w,)) if mask is not None else None
    pts, offs = _out(depth, (h * w, 3)), _out(depth, (h + 1,), _I32)
    ws = _workspace(lib.pp_cloud_from_depth_workspace_bytes(h, w))
    check(lib.pp_cloud_from_depth_f64(ctx.handle, h, w, _ptr(depth), _ptr(mask), mh, mw, _ptr(row_idx), _ptr(col_idx), float(fx), float(fy),
                                      float(cx), float(cy), float(ds), int(bool(dense)), _ptr(ws), _ptr(pts), _ptr(offs)),
          ctx.handle, "pp_cloud_from_depth_f64")
    if dense:
        return pts
    n = int(offs[h].item())
    return pts[:n], offs


def _cloud(what, pts):
    """a non-empty cuda float64 point cloud [n,3] -> (pts.contiguous(), n)"""
    pts = _arg(what, "pts", pts, _F64, (None, 3))
    if pts.shape[0] < 1:
        raise ValueError("%s: pts must not be empty" % what)
    return pts, int(pts.shape[0])


def voxel_down_sample(ctx, pts, voxel, normals=None):
    """Open3D voxel_down_sample (pp_voxel_keys_f64, a stable torch sort, pp_voxel_means_f64): cuda float64 pts [n,3] (and
    normals [n,3]) -> (means [m,3], renormalised mean normals [m,3] or None), ascending voxel key order."""
    pts, n = _cloud("voxel_down_sample", pts)
    normals = _arg("voxel_down_sample", "normals", normals, _F64, (n, 3), optional=True)
    keys = _out(pts, (n,), torch.int64)
    ws = _workspace(lib.pp_voxel_workspace_bytes(n))
    check(lib.pp_voxel_keys_f64(ctx.handle, n, _ptr(pts), float(voxel), _ptr(ws), _ptr(keys)), ctx.handle, "pp_voxel_keys_f64")
    sk, perm = torch.sort(keys, stable=True)
    if bool((sk[:1] < 0).any()):
        raise ValueError("voxel_down_sample: non-finite points, or more than 2^21 voxels along an axis")
    _, counts = torch.unique_consecutive(sk, return_counts=True)
    m = int(counts.numel())
    seg = _out(pts, (m + 1,), torch.int64, 0)
    seg[1:] = torch.cumsum(counts, 0)
    out = _out(pts, (m, 3))
    out_n = _out(pts, (m, 3)) if normals is not None else None
    check(lib.pp_voxel_means_f64(ctx.handle, n, _ptr(pts), _ptr(normals), _ptr(perm.contiguous()), m, _ptr(seg), _ptr(out), _ptr(out_n)),
          ctx.handle, "pp_voxel_means_f64")
    return out, out_n


def estimate_normals(ctx, pts, radius, max_nn, return_neighbors=False):
    """Open3D estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) (pp_estimate_normals_f64): cuda float64 pts [n,3]
    -> normals [n,3] toward the camera, zero with fewer than 3 neighbours (and the neighbour lists int32 [n,max_nn])."""
    pts, n = _cloud("estimate_normals", pts)
    out = _out(pts, (n, 3))
    nbr = _out(pts, (n, int(max_nn)), _I32) if return_neighbors and int(max_nn) > 0 else None
    check(lib.pp_estimate_normals_f64(ctx.handle, n, _ptr(pts), float(radius), int(max_nn), None, _ptr(out), _ptr(nbr)), ctx.handle,
          "pp_estimate_normals_f64")
    return (out, nbr) if return_neighbors else out


def icp(ctx, src_offsets, tgt_offsets, src, tgt, init, max_correspondence_distance, max_iteration=30, relative_fitness=1e-6,
        relative_rmse=1e-6, mode="point_to_plane", tgt_normals=None):
    """Batched ICP (pp_icp_f64): cuda int32 offsets [P+1] into src [Ns,3] / tgt [Nt,3] (float64, checked on the host), init
    float64 [P,4,4], tgt_normals [Nt,3] for point_to_plane.
    -> (R [P,3,3], t [P,3], fitness [P], inlier_rmse [P], iterations int32 [P], status int32 [P], corr int32 [Ns])."""
    if mode not in ICP_MODES:
        raise ValueError("icp: unknown estimation %r (point_to_point | point_to_plane)" % (mode,))
    src, tgt = _arg("icp", "src", src, _F64, (None, 3)), _arg("icp", "tgt", tgt, _F64, (None, 3))
    Ns, Nt = int(src.shape[0]), int(tgt.shape[0])
    src_offsets, so = _check_offsets("icp", src_offsets, Ns, True, name="src_offsets")
    tgt_offsets, to = _check_offsets("icp", tgt_offsets, Nt, True, name="tgt_offsets")
    P = len(so) - 1
    if P < 1 or len(to) != P + 1:
        raise ValueError("icp: src_offsets and tgt_offsets must be [P+1] of one P >= 1")
    init = _arg("icp", "init", init, _F64, (P, 4, 4))
    tgt_normals = _arg("icp", "tgt_normals", tgt_normals, _F64, (Nt, 3), optional=mode != "point_to_plane")
    max_source_points = max(int(np.diff(so).max()), 1)
    nbytes = lib.pp_icp_workspace_bytes(P, max_source_points)
    ws = _workspace(nbytes, "icp: unsupported shape (%d problems)" % P)
    R, t, fit, rmse = _out(src, (P, 3, 3)), _out(src, (P, 3)), _out(src, (P,)), _out(src, (P,))
    iters, status, corr = _out(src, (P,), _I32), _out(src, (P,), _I32), _out(src, (max(Ns, 1),), _I32, -1)
    check(lib.pp_icp_f64(ctx.handle, P, _ptr(src_offsets), _ptr(tgt_offsets), max_source_points, _ptr(src), _ptr(tgt), _ptr(tgt_normals),
                         _ptr(init), float(max_correspondence_distance), int(max_iteration), float(relative_fitness), float(relative_rmse),
                         ICP_MODES[mode], _ptr(ws), nbytes, _ptr(R), _ptr(t), _ptr(fit), _ptr(rmse), _ptr(iters), _ptr(status), _ptr(corr)),
          ctx.handle, "pp_icp_f64")
    return R, t, fit, rmse, iters, status, corr[:Ns]


WPNP_MODES = {"full": 0, "iso": 1}
WPNP_CONVERGED, WPNP_MAX_ITER, WPNP_TOO_FEW, WPNP_SINGULAR, WPNP_BEHIND = 0, 1, 2, 3, 4


def vote_stats(ctx, offsets, img, points_per_vote=8, vote_weight=None, inlier_mask=None, mode="full", sigma_floor=0.5,
               check_offsets=True):
    """Per-corner statistics of corner votes (pp_vote_stats_f64): cuda tensors offsets int32 [P+1] (multiples of
    points_per_vote), img float64 [N,2] laid out as votes x points_per_vote, vote_weight float64 [N / points_per_vote] or
    None, inlier_mask uint8 [N] or None; mode 'full' (W = (cov / n_eff + sigma_floor^2 I)^(-1/2)) or 'iso' (1 / lambda_max).
    -> dict(wsum [P,ppv], count int32 [P,ppv], mu [P,ppv,2], cov [P,ppv,3], n_eff [P,ppv], wgt [P,ppv,3]).
    check_offsets=False skips the host-side look at the offsets (for callers that built them on the device)."""
    if mode not in WPNP_MODES:
        raise ValueError("vote_stats: unknown mode %r (full | iso)" % (mode,))
    ppv = int(points_per_vote)
    img = _arg("vote_stats", "img", img, _F64, (None, 2))
    N = int(img.shape[0])
    if ppv < 1 or ppv > 64 or N % ppv != 0:
        raise ValueError("vote_stats: points_per_vote must be 1..64 and divide the number of points")
    vw = _arg("vote_stats", "vote_weight", vote_weight, _F64, (N // ppv,), optional=True)
    mk = _arg("vote_stats", "inlier_mask", inlier_mask, _U8, (N,), optional=True)
    if not (0.0 <= float(sigma_floor) < 1e150):
        raise ValueError("vote_stats: sigma_floor must be finite and >= 0")
    offsets, _ = _check_offsets("vote_stats", offsets, N, check_offsets, ppv)
    P = int(offsets.numel()) - 1
    ws = _workspace(lib.pp_vote_stats_workspace_bytes(P, ppv))
    z = lambda *shape, dtype=_F64: _out(img, shape, dtype, 0)
    out = dict(wsum=z(P, ppv), count=z(P, ppv, dtype=_I32), mu=z(P, ppv, 2), cov=z(P, ppv, 3), n_eff=z(P, ppv), wgt=z(P, ppv, 3))
    check(lib.pp_vote_stats_f64(ctx.handle, P, _ptr(offsets), N, _ptr(img), ppv, _ptr(vw), _ptr(mk), WPNP_MODES[mode], float(sigma_floor),
                                _ptr(ws), _ptr(out["wsum"]), _ptr(out["count"]), _ptr(out["mu"]), _ptr(out["cov"]), _ptr(out["n_eff"]),
                                _ptr(out["wgt"])), ctx.handle, "pp_vote_stats_f64")
    return out


def pnp_refine_weighted(ctx, offsets, obj, img, wgt, K4, R_init, t_init, max_iterations=50, gradient_tol=1e-10, parameter_tol=1e-8,
                        function_tol=1e-6, pose_cov=True, check_offsets=True):
    """Batched weighted Levenberg-Marquardt PnP refinement (pp_pnp_refine_weighted_f64): cuda tensors offsets int32 [P+1],
    obj float64 [N,3], img [N,2], wgt [N,3] = (wxx, wxy, wyy), K4 [P,4], R_init [P,3,3], t_init [P,3].
    -> dict(R [P,3,3], t [P,3], rvec [P,3], cost_init [P], cost_final [P], iterations int32 [P], status int32 [P],
    pose_cov [P,6,6] or None).  Tolerances default to Ceres' (parity with Ceres unpinned: same cost, own minimiser)."""
    what = "pnp_refine_weighted"
    obj = _arg(what, "obj", obj, _F64, (None, 3))
    N = int(obj.shape[0])
    img, wgt = _arg(what, "img", img, _F64, (N, 2)), _arg(what, "wgt", wgt, _F64, (N, 3))
    offsets, _ = _check_offsets(what, offsets, N, check_offsets)
    P = int(offsets.numel()) - 1
    K4, R_init, t_init = _arg(what, "K4", K4, _F64, (P, 4)), _arg(what, "R_init", R_init, _F64, (P, 3, 3)), _arg(what, "t_init", t_init, _F64, (P, 3))
    if int(max_iterations) < 0 or not all(float(v) >= 0.0 for v in (gradient_tol, parameter_tol, function_tol)):
        raise ValueError("pnp_refine_weighted: max_iterations and the tolerances must be >= 0")
    ws = _workspace(lib.pp_pnp_refine_weighted_workspace_bytes(P, N))
    z = lambda *shape, dtype=_F64: _out(obj, shape, dtype, 0)
    out = dict(R=z(P, 3, 3), t=z(P, 3), rvec=z(P, 3), cost_init=z(P), cost_final=z(P), iterations=z(P, dtype=_I32), status=z(P, dtype=_I32),
               pose_cov=z(P, 6, 6) if pose_cov else None)
    check(lib.pp_pnp_refine_weighted_f64(ctx.handle, P, _ptr(offsets), N, _ptr(obj), _ptr(img), _ptr(wgt), _ptr(K4), _ptr(R_init), _ptr(t_init),
                                         int(max_iterations), float(gradient_tol), float(parameter_tol), float(function_tol), _ptr(ws),
                                         _ptr(out["R"]), _ptr(out["t"]), _ptr(out["rvec"]), _ptr(out["cost_init"]), _ptr(out["cost_final"]),
                                         _ptr(out["iterations"]), _ptr(out["status"]), _ptr(out["pose_cov"])), ctx.handle,
          "pp_pnp_refine_weighted_f64")
    return out


def vote_cluster(ctx, boxes3D, scores, idx, cnt, iou=0.5, min_votes=10, max_instances=8, max_rounds=None):
    """Each (image, class) vote list split into object instances by vote-box IoU (pp_vote_cluster; the library's own step, the
    reference assumes one object per class per image): cuda tensors boxes3D float32 [B,N,16], scores float32 [B,N,C], and
    idx int32 [B,C,cap], cnt int32 [B,C] as score_threshold_compact returns them.  Greedy rounds: the best-scored unassigned
    vote leads, every unassigned vote whose box overlaps the leader's with IoU > iou joins, a cluster of at least min_votes
    members becomes the next instance; at most max_instances instances and max_rounds (default 4 * max_instances) leaders.
    -> (inst int32 [B,C,cap] instance per input vote or -1, order int32 [B,C,cap] anchor indices instance-major (-1 padded),
    inst_offsets int32 [B,C,max_instances+1] into order, n_inst int32 [B,C], leader int32 [B,C,max_instances] anchor or -1,
    inst_box float32 [B,C,max_instances,4] the leader's (x1, y1, x2, y2))."""
    scores = _arg("vote_cluster", "scores", scores, _F32, (None, None, None))
    B, N, Cc = (int(s) for s in scores.shape)
    boxes3D = _arg("vote_cluster", "boxes3D", boxes3D, _F32, (B, N, 16))
    idx = _arg("vote_cluster", "idx", idx, _I32, (B, Cc, None))
    cap = int(idx.shape[2])
    cnt = _arg("vote_cluster", "cnt", cnt, _I32, (B, Cc))
    mi = int(max_instances)
    mr = 4 * mi if max_rounds is None else int(max_rounds)
    inst, order = _out(scores, (B, Cc, cap), _I32), _out(scores, (B, Cc, cap), _I32)
    offs, n_inst, leader = _out(scores, (B, Cc, max(mi, 0) + 1), _I32), _out(scores, (B, Cc), _I32), _out(scores, (B, Cc, max(mi, 1)), _I32)
    box = _out(scores, (B, Cc, max(mi, 1), 4), _F32)
    nb = lib.pp_vote_cluster_workspace_bytes(B, Cc, cap, mi)
    ws = _workspace(nb) if nb else None  # this entry point takes no workspace when it asks for none
    check(lib.pp_vote_cluster(ctx.handle, B, N, Cc, cap, _ptr(boxes3D), _ptr(scores), _ptr(idx), _ptr(cnt), float(iou), int(min_votes), mi, mr,
                              _ptr(ws), _ptr(inst), _ptr(order), _ptr(offs), _ptr(n_inst), _ptr(leader), _ptr(box)), ctx.handle,
          "pp_vote_cluster")
    return inst, order, offs, n_inst, leader, box


DIAMETER_TILE = 256    # points per tile of pp_pts_diameter_f64 (square tiles: one constant); a workgroup sweeps one tile pair
DIAMETER_MAX_CHUNKS = 64  # up to this many tiles a workgroup sweeps ONE j tile; beyond, ceil(tiles / 64) j tiles in a loop (a chunk)
FPS_THREADS = 1024    # threads of the one workgroup per model of pp_farthest_points_f64; a model's further points go through the workspace
FPS_RULES = {"min": 0, "sum": 1}


def pts_diameter(ctx, pts):
    """The farthest pair of one point set (pp_pts_diameter_f64): cuda float64 pts [n,3], 1 <= n <= 2^24 -> (d2 float64 [1] =
    max over i <= j of (dx dx + dy dy) + dz dz, pair int32 [2] = the (i, j) that attains it, lowest i then lowest j).  The
    diameter is math.sqrt(d2) on the host.  All n (n + 1) / 2 pairs are visited in ONE launch: 2^24 is what the pair key
    can address, not a size to use -- at the measured 3e12 pairs/s, 1 M points take about 0.2 s and 2^24 about 45 s."""
    pts = _arg("pts_diameter", "pts", pts, _F64, (None, 3))
    n = int(pts.shape[0])
    nbytes = lib.pp_pts_diameter_workspace_bytes(n)
    ws = _workspace(nbytes)
    d2, pair = _out(pts, (1,)), _out(pts, (2,), _I32)
    check(lib.pp_pts_diameter_f64(ctx.handle, n, _ptr(pts), _ptr(ws), nbytes, _ptr(d2), _ptr(pair)), ctx.handle, "pp_pts_diameter_f64")
    return d2, pair


def farthest_points(ctx, pts, offsets, k, rule="min", min_dist=None, start=None):
    """Greedy farthest-point sampling of k points from each of M point sets in one launch (pp_farthest_points_f64): cuda
    float64 pts [N,3] (the sets concatenated), offsets: M+1 HOST integers rising from 0 to N, rule 'min' (score = smallest
    squared distance to the chosen points; k <= every set's size) or 'sum' (the reference's FPS.py: score = sum of distances to
    the chosen points rounded to float32, 0 for a point nearer than min_dist to any of them; cuda float64 min_dist [M]),
    start: cuda int32 [M] first picks, None = the point of largest norm -> int32 [M,k] indices within each set, the lowest
    index on ties."""
    if rule not in FPS_RULES:
        raise ValueError("farthest_points: unknown rule %r (min | sum)" % (rule,))
    pts = _arg("farthest_points", "pts", pts, _F64, (None, 3))
    off = np.ascontiguousarray(np.asarray(offsets).reshape(-1), np.int32)
    if off.size < 2 or not np.array_equal(off, np.asarray(offsets).reshape(-1)):
        raise ValueError("farthest_points: offsets must hold M+1 >= 2 integers")
    M, N = int(off.size) - 1, int(pts.shape[0])
    min_dist = _arg("farthest_points", "min_dist", min_dist, _F64, (M,), optional=rule == "min")
    start = _arg("farthest_points", "start", start, _I32, (M,), optional=True)
    nbytes = lib.pp_farthest_points_workspace_bytes(N)
    ws = _workspace(nbytes)
    index = _out(pts, (M, max(int(k), 0)), _I32)
    off_dev = torch.from_numpy(off).to(pts.device)
    check(lib.pp_farthest_points_f64(ctx.handle, M, N, _ptr(pts), off.ctypes.data_as(C.POINTER(C.c_int)), _ptr(off_dev), int(k),
                                     FPS_RULES[rule], _ptr(min_dist), _ptr(start), _ptr(ws), nbytes, _ptr(index)), ctx.handle,
          "pp_farthest_points_f64")
    return index


SYM_HD_CHUNK = 4       # candidates per workgroup of pp_sym_hausdorff_f64: a staged target point serves this many pairs per thread
SYM_HD_MAX_CAND = 65535  # candidates per launch


def sym_hausdorff(ctx, src, tgt, S_R, S_t):
    """How far each of K rigid transformations moves src off tgt (pp_sym_hausdorff_f64): cuda float64 src [n,3], tgt [m,3] or
    None (= src), S_R [K,3,3], S_t [K,3] -> (d2 float64 [K] = max_i min_j of (dx dx + dy dy) + dz dz between S_k src_i and
    tgt_j, arg int32 [K,2] = the lowest i that attains the maximum and for it the lowest j that attains the minimum).  The
    distance is math.sqrt(d2) on the host.  1 <= n, m <= 2^24, 1 <= K <= 65535; all K n m pairs are visited in one launch."""
    src = _arg("sym_hausdorff", "src", src, _F64, (None, 3))
    tgt = src if tgt is None else _arg("sym_hausdorff", "tgt", tgt, _F64, (None, 3))
    S_R = _arg("sym_hausdorff", "S_R", S_R, _F64, (None, 3, 3))
    K = int(S_R.shape[0])
    S_t = _arg("sym_hausdorff", "S_t", S_t, _F64, (K, 3))
    n, m = int(src.shape[0]), int(tgt.shape[0])
    nbytes = lib.pp_sym_hausdorff_workspace_bytes(n, K)
    ws = _workspace(nbytes)
    d2, arg = _out(src, (K,)), _out(src, (K, 2), _I32)
    check(lib.pp_sym_hausdorff_f64(ctx.handle, n, _ptr(src), m, _ptr(tgt), K, _ptr(S_R), _ptr(S_t), _ptr(ws), nbytes, _ptr(d2), _ptr(arg)),
          ctx.handle, "pp_sym_hausdorff_f64")
    return d2, arg


DET_RULES = {"reference": 0, "coco": 1}       # PP_DET_RULE_*
DET_INTEGRATIONS = {"area": 0, "101": 1}      # PP_DET_AP_*
DET_MAX_THR = 16      # thresholds per pp_det_match launch (one wave each)
DET_MAX_DET = 1024    # detection slots per image its LDS layout holds
DET_MAX_GT = 1024     # ground truth per image it holds
DET_SCAN_CHUNK = 256  # detections per scan step of pp_det_pr_curve


def _det_labels_ok(what, name, labels, n_class, padding):
    """labels (cuda int32) all inside [0, n_class), or -1 where `padding` is allowed; a host look (one sync)"""
    if labels.numel() == 0:
        return
    lo, hi = int(labels.min()), int(labels.max())
    if hi >= n_class or lo < (-1 if padding else 0):
        raise ValueError("%s: %s must lie in [0, %d)%s, got %d..%d" % (what, name, n_class, " or be -1 (padding)" if padding else "", lo, hi))


def det_match(ctx, det_boxes, det_scores, det_labels, gt_boxes, gt_labels, gt_offsets, n_class, thresholds, rule="reference",
              gt_ignore=None, check=True):
    """Detections of B images matched to their ground truth at T IoU thresholds in one launch (pp_det_match): cuda tensors
    det_boxes float64 [B,D,4], det_scores float64 [B,D], det_labels int32 [B,D] (-1 = padding, anywhere in a row), gt_boxes
    float64 [G,4], gt_labels int32 [G], gt_offsets int32 [B+1] from 0 to G, gt_ignore uint8 [G] or None; thresholds: 1..16
    host floats, increasing within [0, 1]; rule 'reference' (utils/eval.py: "+1" IoU, first-maximum ground truth, no second
    choice; gt_ignore must be None) or 'coco' (pycocotools' evaluateImg without crowd, restated) -> (match int32 [T,B,D] global
    ground-truth index or -1, det_ignored uint8 [T,B,D], npos int32 [n_class] ground truth per class that is not ignored).
    D <= 1024 and at most 1024 ground truths per image.  The offsets are always looked at on the host; check=False skips the
    look at the labels (one more sync): labels outside [0, n_class) then count as padding / match nothing."""
    what = "det_match"
    if rule not in DET_RULES:
        raise ValueError("%s: unknown rule %r (reference | coco)" % (what, rule))
    thr = np.ascontiguousarray(np.asarray(thresholds, np.float64).reshape(-1))
    T = int(thr.size)
    if not 1 <= T <= DET_MAX_THR:
        raise ValueError("%s: need 1..%d thresholds, got %d" % (what, DET_MAX_THR, T))
    if not (np.all(thr >= 0.0) and np.all(thr <= 1.0) and np.all(np.diff(thr) > 0.0)):
        raise ValueError("%s: thresholds must increase within [0, 1]" % what)
    n_class = int(n_class)
    if n_class < 1:
        raise ValueError("%s: n_class must be >= 1" % what)
    det_scores = _arg(what, "det_scores", det_scores, _F64, (None, None))
    B, D = (int(s) for s in det_scores.shape)
    det_boxes = _arg(what, "det_boxes", det_boxes, _F64, (B, D, 4))
    det_labels = _arg(what, "det_labels", det_labels, _I32, (B, D))
    gt_boxes = _arg(what, "gt_boxes", gt_boxes, _F64, (None, 4))
    G = int(gt_boxes.shape[0])
    gt_labels = _arg(what, "gt_labels", gt_labels, _I32, (G,))
    gt_ignore = _arg(what, "gt_ignore", gt_ignore, _U8, (G,), optional=True)
    if gt_ignore is not None and rule == "reference":
        raise ValueError("%s: the reference rule has no ignored ground truth (gt_ignore must be None)" % what)
    if B < 1 or D > DET_MAX_DET or T * B * D >= 2 ** 31:
        raise ValueError("%s: need B >= 1, D <= %d and T * B * D < 2^31, got B = %d, D = %d" % (what, DET_MAX_DET, B, D))
    gt_offsets, off = _check_offsets(what, gt_offsets, G, True, name="gt_offsets")
    if off.size != B + 1:
        raise ValueError("%s: gt_offsets must hold B + 1 = %d entries, got %d" % (what, B + 1, off.size))
    if B and int(np.diff(off).max()) > DET_MAX_GT:
        raise ValueError("%s: an image has %d ground truths, the limit is %d" % (what, int(np.diff(off).max()), DET_MAX_GT))
    if check:
        _det_labels_ok(what, "det_labels", det_labels, n_class, True)
        _det_labels_ok(what, "gt_labels", gt_labels, n_class, False)
    off = np.ascontiguousarray(off, np.int32)
    match, ign = _out(det_scores, (T, B, D), _I32), _out(det_scores, (T, B, D), _U8)
    npos = _out(det_scores, (n_class,), _I32)
    check_status(lib.pp_det_match(ctx.handle, B, D, G, n_class, _ptr(det_boxes), _ptr(det_scores), _ptr(det_labels), _ptr(gt_boxes),
                                  _ptr(gt_labels), _ptr(gt_ignore), off.ctypes.data_as(C.POINTER(C.c_int)), _ptr(gt_offsets), T,
                                  thr.ctypes.data_as(C.POINTER(C.c_double)), DET_RULES[rule], _ptr(match), _ptr(ign), _ptr(npos)),
                 ctx.handle, "pp_det_match")
    return match, ign, npos


def det_order(det_scores, det_labels, n_class):
    """The global order pp_det_pr_curve scans: cuda det_scores [B,D], det_labels int32 [B,D] -> (order int32 [N]: the flat
    slots b * D + d of the detections with a label in [0, n_class), class-major, then descending score, then ascending flat
    slot; class_offsets int32 [n_class+1] into it).  torch.sort(stable=True) on the device: plumbing, not the hot path.
    The tie-break between equal scores is the library's own: the reference's np.argsort(-scores) (utils/eval.py:219, a
    quicksort) leaves the order of ties undefined, pycocotools sorts with a stable mergesort over its own detection list;
    the ascending flat slot is the stable order of the layout the detections arrive in."""
    n_class = int(n_class)
    s, l = det_scores.reshape(-1), det_labels.reshape(-1)
    slot = torch.nonzero((l >= 0) & (l < n_class)).reshape(-1)
    slot = slot[torch.sort(s[slot], descending=True, stable=True).indices]
    lab = l[slot].long()
    order = slot[torch.sort(lab, stable=True).indices].to(_I32)
    counts = torch.bincount(lab, minlength=n_class)
    offsets = torch.zeros((n_class + 1,), dtype=_I32, device=s.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return order, offsets


def _det_curve_args(what, class_offsets, npos, N, check):
    npos = _arg(what, "npos", npos, _I32, (None,))
    n_class = int(npos.shape[0])
    if n_class < 1:
        raise ValueError("%s: npos must hold at least one class" % what)
    class_offsets, off = _check_offsets(what, class_offsets, N, check, name="class_offsets")
    if class_offsets.numel() != n_class + 1:
        raise ValueError("%s: class_offsets must hold n_class + 1 = %d entries, got %d" % (what, n_class + 1, class_offsets.numel()))
    return class_offsets, npos, n_class


def det_pr_curve(ctx, order, class_offsets, match, det_ignored, npos, check=True):
    """True / false positive scans, recall and precision envelope of every (threshold, class) (pp_det_pr_curve): order int32
    [N] and class_offsets int32 [C+1] from det_order, match int32 [T,B,D], det_ignored uint8 [T,B,D] and npos int32 [C] from
    det_match -> (tp int32 [T,N], fp int32 [T,N] inclusive running counts within each class, recall float64 [T,N] = tp /
    npos, prec_env float64 [T,N] = reverse running maximum of tp / max(tp + fp, eps)).  check=False skips the host look at
    class_offsets (a sync); they must then rise from 0 to N."""
    what = "det_pr_curve"
    order = _arg(what, "order", order, _I32, (None,))
    N = int(order.shape[0])
    match = _arg(what, "match", match, _I32, (None, None, None))
    T, n_slots = int(match.shape[0]), int(match.shape[1]) * int(match.shape[2])
    det_ignored = _arg(what, "det_ignored", det_ignored, _U8, tuple(match.shape))
    if not 1 <= T <= DET_MAX_THR or N > n_slots or T * n_slots >= 2 ** 31:
        raise ValueError("%s: need 1..%d thresholds, N <= B * D and T * B * D < 2^31" % (what, DET_MAX_THR))
    class_offsets, npos, n_class = _det_curve_args(what, class_offsets, npos, N, check)
    tp, fp = _out(order, (T, N), _I32), _out(order, (T, N), _I32)
    recall, env = _out(order, (T, N)), _out(order, (T, N))
    check_status(lib.pp_det_pr_curve(ctx.handle, T, N, n_class, n_slots, _ptr(order), _ptr(class_offsets), _ptr(match), _ptr(det_ignored),
                                     _ptr(npos), _ptr(tp), _ptr(fp), _ptr(recall), _ptr(env)), ctx.handle, "pp_det_pr_curve")
    return tp, fp, recall, env


def det_ap(ctx, class_offsets, npos, recall, prec_env, integration="area", check=True):
    """Average precision per (threshold, class) from det_pr_curve's curves (pp_det_ap): integration 'area' (the reference's
    _compute_ap: sum of recall steps times the envelope; a class without ground truth gives 0) or '101' (COCO's 101 recall
    points; such a class gives -1 and is left out of means) -> (ap float64 [T,C], recall_final float64 [T,C])."""
    what = "det_ap"
    if integration not in DET_INTEGRATIONS:
        raise ValueError("%s: unknown integration %r (area | 101)" % (what, integration))
    recall = _arg(what, "recall", recall, _F64, (None, None))
    T, N = (int(s) for s in recall.shape)
    prec_env = _arg(what, "prec_env", prec_env, _F64, (T, N))
    if not 1 <= T <= DET_MAX_THR or T * N >= 2 ** 31:
        raise ValueError("%s: need 1..%d thresholds and T * N < 2^31" % (what, DET_MAX_THR))
    class_offsets, npos, n_class = _det_curve_args(what, class_offsets, npos, N, check)
    ap, rf = _out(recall, (T, n_class)), _out(recall, (T, n_class))
    check_status(lib.pp_det_ap(ctx.handle, T, N, n_class, _ptr(class_offsets), _ptr(npos), _ptr(recall), _ptr(prec_env),
                               DET_INTEGRATIONS[integration], _ptr(ap), _ptr(rf)), ctx.handle, "pp_det_ap")
    return ap, rf


MASK_MAX_CLASS = 256       # PP_MASK_MAX_CLASS: classes whose partial counts pp_mask_confusion holds in LDS
MASK_IOU_TILE = (4, 4)     # PP_MASK_IOU_TILE_DET x PP_MASK_IOU_TILE_GT: the pairs one workgroup of pp_mask_iou_pairs takes
MASK_ORDERS = {"row": 0, "column": 1, 0: 0, 1: 1}  # PP_MASK_ORDER_*
_I64 = torch.int64


def _host_f64(v):
    return np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1))


def mask_confusion(ctx, pred, target, thresholds=(0.5,)):
    """(tp, fp, fn) of the mask head's output against its training target (pp_mask_confusion): cuda float32 pred [B,M,C] (sigmoid
    values) and target [B,M,C+1] (as anchor_targets writes it; the last channel is not read); thresholds: 1..16 host floats.
    A pixel is predicted iff pred > threshold as a float64 compare (NaN: not predicted), set iff target != 0
    -> counts int64 [T,C,3]."""
    what = "mask_confusion"
    thr = _host_f64(thresholds)
    T = int(thr.size)
    if not 1 <= T <= DET_MAX_THR or np.isnan(thr).any():
        raise ValueError("%s: need 1..%d thresholds that are not NaN, got %d" % (what, DET_MAX_THR, T))
    pred = _arg(what, "pred", pred, _F32, (None, None, None))
    B, M, Cc = (int(s) for s in pred.shape)
    target = _arg(what, "target", target, _F32, (B, M, Cc + 1))
    if B < 1 or M < 1 or not 1 <= Cc <= MASK_MAX_CLASS or B * M * (Cc + 1) >= 2 ** 31:
        raise ValueError("%s: need B, M >= 1, 1 <= C <= %d and B * M * (C + 1) < 2^31, got %s" % (what, MASK_MAX_CLASS, list(pred.shape)))
    counts = _out(pred, (T, Cc, 3), _I64)
    check_status(lib.pp_mask_confusion(ctx.handle, B, M, Cc, _ptr(pred), _ptr(target), T, thr.ctypes.data_as(C.POINTER(C.c_double)),
                                       _ptr(counts)), ctx.handle, "pp_mask_confusion")
    return counts


def _mask_stack(what, name, masks):
    masks = _arg(what, name, masks, _U8, (None, None, None))
    N, H, W = (int(s) for s in masks.shape)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError("%s: %s needs H, W >= 1 and H * W < 2^31, got %s" % (what, name, list(masks.shape)))
    return masks, N, H, W


def mask_pack(ctx, masks):
    """Byte masks to bits (pp_mask_pack): cuda uint8 [N,H,W], non-zero = set -> (words int64 [N,ceil(H W / 64)] holding the
    uint64 bit patterns: bit i of word k is pixel 64 k + i in row-major order, tail bits 0; area int64 [N]; word_range int32
    [N,2]: first non-empty word and one past the last, [0, 0) for an empty mask)."""
    what = "mask_pack"
    masks, N, H, W = _mask_stack(what, "masks", masks)
    n_word = (H * W + 63) // 64
    words, area, rng = _out(masks, (N, n_word), _I64), _out(masks, (N,), _I64), _out(masks, (N, 2), _I32)
    check_status(lib.pp_mask_pack(ctx.handle, N, H, W, _ptr(masks), _ptr(words), _ptr(area), _ptr(rng)), ctx.handle, "pp_mask_pack")
    return words, area, rng


def _det_gt_offsets(what, gt_offsets, G, B):
    gt_offsets, off = _check_offsets(what, gt_offsets, G, True, name="gt_offsets")
    if off.size != B + 1:
        raise ValueError("%s: gt_offsets must hold B + 1 = %d entries, got %d" % (what, B + 1, off.size))
    if B and int(np.diff(off).max()) > DET_MAX_GT:
        raise ValueError("%s: an image has %d ground truths, the limit is %d" % (what, int(np.diff(off).max()), DET_MAX_GT))
    return gt_offsets, np.ascontiguousarray(off, np.int32)


def mask_iou_pairs(ctx, det_packed, gt_packed, gt_offsets, shape, n_det, det_labels=None, want_inter=False):
    """IoU of every (detection slot, ground truth) pair of each image (pp_mask_iou_pairs).  det_packed / gt_packed: the
    (words, area, word_range) triples of mask_pack over the detections' [B * D] slots (slot d of image b is mask b * D + d)
    and over the [G] ground truths; gt_offsets int32 [B+1] (cuda); shape = (H, W) of the masks; n_det = D; det_labels int32
    [B,D] or None: slots with a label < 0 are padding (not read, IoU 0) -> (iou float64 [D * G], pair_offsets int64 numpy
    [B+1]: pair (b, d, g) sits at pair_offsets[b] + d * ng_b + g; with want_inter also inter int64 [D * G])."""
    what = "mask_iou_pairs"
    H, W = int(shape[0]), int(shape[1])
    D = int(n_det)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError("%s: need H, W >= 1 and H * W < 2^31" % what)
    n_word = (H * W + 63) // 64
    dw = _arg(what, "det words", det_packed[0], _I64, (None, n_word))
    BD = int(dw.shape[0])
    if D < 0 or D > DET_MAX_DET or (D == 0 and BD) or (D and BD % D):
        raise ValueError("%s: %d packed detection masks are no multiple of D = %d <= %d" % (what, BD, D, DET_MAX_DET))
    da, dr = _arg(what, "det area", det_packed[1], _I64, (BD,)), _arg(what, "det word_range", det_packed[2], _I32, (BD, 2))
    gw = _arg(what, "gt words", gt_packed[0], _I64, (None, n_word))
    G = int(gw.shape[0])
    ga, gr = _arg(what, "gt area", gt_packed[1], _I64, (G,)), _arg(what, "gt word_range", gt_packed[2], _I32, (G, 2))
    gt_offsets = _arg(what, "gt_offsets", gt_offsets, _I32, (None,))
    B = BD // D if D else int(gt_offsets.numel()) - 1
    if B < 1 or D * G >= 2 ** 31:
        raise ValueError("%s: need B >= 1 and D * G < 2^31 pairs, got B = %d, D = %d, G = %d" % (what, B, D, G))
    det_labels = _arg(what, "det_labels", det_labels, _I32, (B, D), optional=True)
    gt_offsets, off = _det_gt_offsets(what, gt_offsets, G, B)
    iou = _out(gw, (D * G,))
    inter = _out(gw, (D * G,), _I64) if want_inter else None
    check_status(lib.pp_mask_iou_pairs(ctx.handle, B, D, G, H, W, _ptr(dw), _ptr(da), _ptr(dr), _ptr(det_labels), _ptr(gw), _ptr(ga),
                                       _ptr(gr), off.ctypes.data_as(C.POINTER(C.c_int)), _ptr(gt_offsets), _ptr(iou), _ptr(inter)),
                 ctx.handle, "pp_mask_iou_pairs")
    pair_offsets = off.astype(np.int64) * D
    return (iou, pair_offsets, inter) if want_inter else (iou, pair_offsets)


def det_match_iou(ctx, iou, det_scores, det_labels, gt_labels, gt_offsets, n_class, thresholds, rule="coco", gt_ignore=None, check=True):
    """det_match with the IoU read from a pair matrix instead of computed from boxes (pp_det_match_iou): iou float64 [D * G]
    in mask_iou_pairs' layout; everything else -- ranking, tie-breaks, both rules, gt_ignore, padding, the limits, check -- as
    det_match -> (match int32 [T,B,D], det_ignored uint8 [T,B,D], npos int32 [n_class]), which feed det_pr_curve / det_ap."""
    what = "det_match_iou"
    if rule not in DET_RULES:
        raise ValueError("%s: unknown rule %r (reference | coco)" % (what, rule))
    thr = _host_f64(thresholds)
    T = int(thr.size)
    if not 1 <= T <= DET_MAX_THR:
        raise ValueError("%s: need 1..%d thresholds, got %d" % (what, DET_MAX_THR, T))
    if not (np.all(thr >= 0.0) and np.all(thr <= 1.0) and np.all(np.diff(thr) > 0.0)):
        raise ValueError("%s: thresholds must increase within [0, 1]" % what)
    n_class = int(n_class)
    if n_class < 1:
        raise ValueError("%s: n_class must be >= 1" % what)
    det_scores = _arg(what, "det_scores", det_scores, _F64, (None, None))
    B, D = (int(s) for s in det_scores.shape)
    det_labels = _arg(what, "det_labels", det_labels, _I32, (B, D))
    gt_labels = _arg(what, "gt_labels", gt_labels, _I32, (None,))
    G = int(gt_labels.shape[0])
    if B < 1 or D > DET_MAX_DET or T * B * D >= 2 ** 31 or D * G >= 2 ** 31:
        raise ValueError("%s: need B >= 1, D <= %d, T * B * D < 2^31 and D * G < 2^31, got B = %d, D = %d, G = %d" %
                         (what, DET_MAX_DET, B, D, G))
    iou = _arg(what, "iou", iou, _F64, (D * G,))
    gt_ignore = _arg(what, "gt_ignore", gt_ignore, _U8, (G,), optional=True)
    if gt_ignore is not None and rule == "reference":
        raise ValueError("%s: the reference rule has no ignored ground truth (gt_ignore must be None)" % what)
    gt_offsets, off = _det_gt_offsets(what, gt_offsets, G, B)
    if check:
        _det_labels_ok(what, "det_labels", det_labels, n_class, True)
        _det_labels_ok(what, "gt_labels", gt_labels, n_class, False)
    if iou.numel() == 0:
        iou = _out(det_scores, (1,), fill=0.0)  # (the entry point wants a pointer)
    match, ign = _out(det_scores, (T, B, D), _I32), _out(det_scores, (T, B, D), _U8)
    npos = _out(det_scores, (n_class,), _I32)
    check_status(lib.pp_det_match_iou(ctx.handle, B, D, G, n_class, _ptr(iou), _ptr(det_scores), _ptr(det_labels), _ptr(gt_labels),
                                      _ptr(gt_ignore), off.ctypes.data_as(C.POINTER(C.c_int)), _ptr(gt_offsets), T,
                                      thr.ctypes.data_as(C.POINTER(C.c_double)), DET_RULES[rule], _ptr(match), _ptr(ign), _ptr(npos)),
                 ctx.handle, "pp_det_match_iou")
    return match, ign, npos


def _mask_order(what, order):
    if order not in MASK_ORDERS:
        raise ValueError("%s: unknown order %r (row | column)" % (what, order))
    return MASK_ORDERS[order]


def mask_rle(ctx, masks, order="row", capacity=None):
    """Run lengths of byte masks (pp_mask_rle): cuda uint8 [N,H,W]; order 'row' (row-major, the reference's rle_encode) or
    'column' (COCO's); capacity: the int32 entries to allocate for the runs, default N * (H * W + 1) bounded by 2^24 and grown
    once to what the library reports when that is too few (a capacity given by the caller is never grown: ValueError)
    -> (run_offsets int64 numpy [N+1], counts int32 cuda [run_offsets[N]]): COCO's uncompressed counts of mask n are
    counts[run_offsets[n]:run_offsets[n+1]], starting with the length of the leading zero run (0 when the first pixel is set)."""
    what = "mask_rle"
    order = _mask_order(what, order)
    masks, N, H, W = _mask_stack(what, "masks", masks)
    if N < 1 or N * (H * W + 1) >= 2 ** 31:
        raise ValueError("%s: need N >= 1 and N * (H * W + 1) < 2^31, got %s" % (what, list(masks.shape)))
    nbytes = lib.pp_mask_rle_workspace_bytes(N)
    ws = _workspace(nbytes)
    offs = _out(masks, (N + 1,), _I32)
    host = np.zeros(N + 1, np.int32)
    given = capacity is not None
    cap = int(capacity) if given else min(N * (H * W + 1), 1 << 24)
    if cap < 0:
        raise ValueError("%s: capacity must be >= 0" % what)
    while True:
        counts = _out(masks, (max(cap, 1),), _I32)
        rc = lib.pp_mask_rle(ctx.handle, N, H, W, order, _ptr(masks), _ptr(ws), nbytes, cap, _ptr(offs),
                             host.ctypes.data_as(C.POINTER(C.c_int)), _ptr(counts))
        if rc != 0 and not given and int(host[N]) > cap:
            cap = int(host[N])
            continue
        check_status(rc, ctx.handle, "pp_mask_rle")
        return host.astype(np.int64), counts[:int(host[N])]


def mask_from_rle(ctx, run_offsets, counts, shape, order="row"):
    """Runs back to byte masks of 0 / 255 (pp_mask_from_rle): run_offsets [N+1] and counts (host arrays or tensors: the host
    copy is checked, every mask's lengths must add up to H * W) -> cuda uint8 [N,H,W]."""
    what = "mask_from_rle"
    order = _mask_order(what, order)
    H, W = int(shape[0]), int(shape[1])
    off = np.ascontiguousarray((run_offsets.cpu().numpy() if torch.is_tensor(run_offsets) else np.asarray(run_offsets)).reshape(-1))
    cnt = np.ascontiguousarray((counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)).reshape(-1))
    N = int(off.size) - 1
    if N < 1 or H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError("%s: need N >= 1 masks, H, W >= 1 and H * W < 2^31" % what)
    if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != cnt.size or cnt.size >= 2 ** 31:
        raise ValueError("%s: run_offsets must rise from 0 to the number of counts (%d)" % (what, cnt.size))
    if cnt.size and (cnt.min() < 0 or cnt.max() >= 2 ** 31):
        raise ValueError("%s: run lengths must lie in [0, 2^31)" % what)
    off, cnt = off.astype(np.int32), cnt.astype(np.int32)
    sums = np.add.reduceat(np.concatenate([cnt.astype(np.int64), [0]]), off[:-1].astype(np.int64)) * (np.diff(off) > 0)
    if (sums != H * W).any():
        bad = int(np.nonzero(sums != H * W)[0][0])
        raise ValueError("%s: the runs of mask %d add up to %d, the image has %d pixels" % (what, bad, int(sums[bad]), H * W))
    dev = "cuda:%d" % ctx.device
    off_d = torch.from_numpy(off).to(dev)
    cnt_d = counts.to(device=dev, dtype=_I32).contiguous().reshape(-1) if torch.is_tensor(counts) and counts.is_cuda \
        else torch.from_numpy(cnt).to(dev)
    if cnt_d.numel() == 0:
        cnt_d = torch.zeros((1,), dtype=_I32, device=dev)
    masks = torch.empty((N, H, W), dtype=_U8, device=dev)
    check_status(lib.pp_mask_from_rle(ctx.handle, N, H, W, order, off.ctypes.data_as(C.POINTER(C.c_int)),
                                      (cnt if cnt.size else np.zeros(1, np.int32)).ctypes.data_as(C.POINTER(C.c_int)), _ptr(off_d),
                                      _ptr(cnt_d), _ptr(masks)), ctx.handle, "pp_mask_from_rle")
    return masks


DEPTH_NORMALS_TILE = 32   # pixels per edge of the LDS tile of pp_depth_normals_f64's smoothing launch (its halo: 8 more on every side)
DEPTH_NORMALS_OUTPUTS = {"normals": (_F64, (3,)), "normals_u8": (_U8, (3,)), "depth": (_F64, ()), "signed": (_F64, (3,))}  # in the ABI's order


def gaussian_taps(sigma=2.0, truncate=4.0):
    """The weights of scipy.ndimage.gaussian_filter(x, sigma) as a float64 host array: exp(-x^2 / (2 sigma^2)) over
    x = -r..r, r = int(truncate sigma + 0.5), divided by their sum.  pp_depth_normals_f64 takes them from here, so that the
    library and whoever restates it share one exp."""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return w / w.sum()


def depth_normals(ctx, depth, intr, for_vis=True, want=("normals", "depth")):
    """The reference's get_normal on n depth images (pp_depth_normals_f64): cuda tensors depth float32 [n,H,W] (finite, >= 0),
    intr float64 [n,3] = (fx, cx, cy) per image (the reference ignores fy); want: any of 'normals' (float64 [n,H,W,3], |unit
    normal|, 0 where the smoothed depth exceeds 2000), 'signed' (the same before abs), 'depth' (float64 [n,H,W], the smoothed
    depth; divided by its per-image maximum when for_vis is False) and, with for_vis False only, 'normals_u8' (uint8 [n,H,W,3],
    the image the reference writes as _dep.png) -> dict of the requested outputs.  An image whose smoothed depth, or whose
    scaled normal image, is all zero gives an all-zero 'normals_u8' and 'depth' under for_vis False."""
    what = "depth_normals"
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(o not in DEPTH_NORMALS_OUTPUTS for o in want):
        raise ValueError("%s: want must name at least one of %s, got %r" % (what, " | ".join(DEPTH_NORMALS_OUTPUTS), want))
    if for_vis and "normals_u8" in want:
        raise ValueError("%s: 'normals_u8' is an output of for_vis=False" % what)
    depth = _arg(what, "depth", depth, _F32, (None, None, None))
    n, H, W = (int(s) for s in depth.shape)
    intr = _arg(what, "intr", intr, _F64, (n, 3))
    nbytes = lib.pp_depth_normals_workspace_bytes(n, H, W)
    ws = _workspace(nbytes)  # (0 bytes: a refused shape, which the entry point reports)
    out = {k: _out(depth, (n, H, W) + tail, dt) for k, (dt, tail) in DEPTH_NORMALS_OUTPUTS.items() if k in want}
    taps = np.ascontiguousarray(gaussian_taps(2.0), np.float64)
    check(lib.pp_depth_normals_f64(ctx.handle, n, H, W, _ptr(depth), _ptr(intr), taps.ctypes.data_as(C.POINTER(C.c_double)),
                                   1 if for_vis else 0, _ptr(ws), nbytes, *[_ptr(out.get(k)) for k in DEPTH_NORMALS_OUTPUTS]),
          ctx.handle, "pp_depth_normals_f64")
    return out


DEPTH_AUG_TILE = 32   # pixels per edge of the LDS tiles of pp_depth_augment (halo: 9 more per side in launch A, 3 in launch B)
DEPTH_AUG_OUTPUTS = {"depth_f32": _F32, "depth_f64": _F64, "mask_u8": _U8, "half_f64": _F64, "sensor_f64": _F64}  # in the ABI's order
# a parameter row of pp_depth_augment (PP_DA_* of include/pyrapose_hip.h): name -> (first slot, slots)
DEPTH_AUG_PARAMS = {"k_open": (0, 1), "k_med": (1, 1), "k_blur": (2, 1), "blur_taps": (3, 7), "depth_noise": (10, 1), "sensor": (11, 1),
                    "simplex": (12, 1), "freq": (13, 1), "octaves": (14, 1), "lacunarity": (15, 1), "gain": (16, 1), "w_xy": (17, 1),
                    "w_z": (18, 1), "jitter_lo": (19, 3), "jitter_hi": (22, 3), "seed": (25, 1)}
DEPTH_AUG_P = 26


def depth_aug_half_size(n):
    """cv2's cvRound(n / 2), half to even: the side of pp_depth_augment's half-size image"""
    return n // 2 + ((n // 2) & 1 if n & 1 else 0)


def depth_aug_blur_taps(k, sigma):
    """cv2.getGaussianKernel(k, sigma) as a float64 host array: exp(-x^2 / (2 sigma^2)) over x = -(k-1)/2 .. (k-1)/2, divided
    by their sum; sigma <= 0 means cv2's 0.3 ((k - 1) 0.5 - 1) + 0.8.  pp_depth_augment takes them in its parameter rows, so
    that the library and whoever restates it share one exp."""
    k, sigma = int(k), float(sigma)
    if k not in (1, 3, 5, 7):
        raise ValueError("depth_aug_blur_taps: k must be 1, 3, 5 or 7, got %r" % (k,))
    if sigma <= 0:
        sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x = np.arange(k, dtype=np.float64) - (k - 1) // 2
    w = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return w / w.sum()


def depth_augment(ctx, depth, mask, params, z=None, want=("depth_f32",)):
    """The reference's augmentDepth on n depth images (pp_depth_augment): cuda tensors depth float32 [n,H,W] (millimetres,
    finite, >= 0) and mask uint8 [n,H,W] (non-zero = foreground); params a float64 HOST array [n, DEPTH_AUG_P], one row per
    image (DEPTH_AUG_PARAMS); z cuda float32 [n,h2,w2] standard normals (h2, w2 = depth_aug_half_size of H, W), needed when a
    row has sensor = 1; want: any of DEPTH_AUG_OUTPUTS -> dict of the requested outputs: 'depth_f32' / 'depth_f64' [n,H,W]
    the augmented depth, 'mask_u8' [n,H,W] the shadow mask as 0 / 255, 'half_f64' [n,h2,w2] the half-size sensor image,
    'sensor_f64' [n,H,W] the depth before the simplex warp."""
    what = "depth_augment"
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(o not in DEPTH_AUG_OUTPUTS for o in want):
        raise ValueError("%s: want must name at least one of %s, got %r" % (what, " | ".join(DEPTH_AUG_OUTPUTS), want))
    depth = _arg(what, "depth", depth, _F32, (None, None, None))
    n, H, W = (int(s) for s in depth.shape)
    mask = _arg(what, "mask", mask, _U8, (n, H, W))
    h2, w2 = depth_aug_half_size(H), depth_aug_half_size(W)
    z = _arg(what, "z", z, _F32, (n, h2, w2), optional=True)
    host = np.ascontiguousarray(params, np.float64)
    if host.shape != (n, DEPTH_AUG_P):
        raise ValueError("%s: params must be a host array [%d,%d], got %s" % (what, n, DEPTH_AUG_P, host.shape))
    dev = torch.from_numpy(host).to(depth.device)
    nbytes = lib.pp_depth_augment_workspace_bytes(n, H, W)
    ws = _workspace(nbytes)  # (0 bytes: a refused shape, which the entry point reports)
    shapes = {"half_f64": (n, h2, w2)}
    out = {k: _out(depth, shapes.get(k, (n, H, W)), dt) for k, dt in DEPTH_AUG_OUTPUTS.items() if k in want}
    check(lib.pp_depth_augment(ctx.handle, n, H, W, _ptr(depth), _ptr(mask), _ptr(dev), host.ctypes.data_as(C.POINTER(C.c_double)),
                               _ptr(z), _ptr(ws), nbytes, *[_ptr(out.get(k)) for k in DEPTH_AUG_OUTPUTS]), ctx.handle, "pp_depth_augment")
    return out


DEPTH_INPAINT_TILE = 32        # lanes per image row of pp_depth_inpaint's row pass, pixels per row of a workgroup of its layer pass
DEPTH_INPAINT_ROWS = 8         # image rows per workgroup in both
DEPTH_INPAINT_MAX_RADIUS = 8
DEPTH_INPAINT_MAX_DIST = 65535
DEPTH_INPAINT_MAX_SIDE = 4096
DEPTH_INPAINT_NO_LAYER = 65535  # 'layer' of every pixel of an image without a known pixel
DEPTH_INPAINT_OUTPUTS = {"filled_f32": _F32, "filled_f64": _F64, "layer": torch.uint16, "counts": _I32}  # in the ABI's order


def depth_inpaint(ctx, depth, hole_mask=None, radius=5, max_dist=0, rescale=False, want=("filled_f32",)):
    """Layered filling of depth holes on n images (pp_depth_inpaint, the rule in include/pyrapose_hip.h): cuda tensors depth
    float32 [n,H,W] (finite, >= 0) and hole_mask uint8 [n,H,W] (non-zero = hole; None: a hole is depth == 0); radius 1..8 of the
    window, max_dist the deepest layer that is filled (0: all), rescale the reference's stretch to [0, max depth]; want: any of
    DEPTH_INPAINT_OUTPUTS -> dict of the requested outputs: 'filled_f32' / 'filled_f64' [n,H,W], 'layer' uint16 [n,H,W] (the
    chessboard distance to the nearest known pixel; DEPTH_INPAINT_NO_LAYER in an image without one), 'counts' int32 [n,3] =
    (holes, pixels to fill, largest layer).  The filled outputs cost one host synchronisation."""
    what = "depth_inpaint"
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(o not in DEPTH_INPAINT_OUTPUTS for o in want):
        raise ValueError("%s: want must name at least one of %s, got %r" % (what, " | ".join(DEPTH_INPAINT_OUTPUTS), want))
    depth = _arg(what, "depth", depth, _F32, (None, None, None))
    n, H, W = (int(s) for s in depth.shape)
    hole_mask = _arg(what, "hole_mask", hole_mask, _U8, (n, H, W), optional=True)
    nbytes = lib.pp_depth_inpaint_workspace_bytes(n, H, W)
    ws = _workspace(nbytes)  # (0 bytes: a refused shape, which the entry point reports)
    out = {k: _out(depth, (n, 3) if k == "counts" else (n, H, W), dt) for k, dt in DEPTH_INPAINT_OUTPUTS.items() if k in want}
    check(lib.pp_depth_inpaint(ctx.handle, n, H, W, _ptr(depth), _ptr(hole_mask), int(radius), int(max_dist), 1 if rescale else 0,
                               _ptr(ws), nbytes, *[_ptr(out.get(k)) for k in DEPTH_INPAINT_OUTPUTS]), ctx.handle, "pp_depth_inpaint")
    return out


OVERLAY_SEGMENT, OVERLAY_GLYPH, OVERLAY_FILL_RECT = 0, 1, 2  # record kinds of pp_draw_overlay_u8
OVERLAY_TILE = 32            # pixels per side of a workgroup's tile
OVERLAY_CHUNK = 256          # records per pass over an image's list
OVERLAY_MAX_SIDE = 8192
OVERLAY_MAX_COORD = 8192     # |coordinate| of a segment's end points and of a glyph's corner
OVERLAY_MAX_THICK = 64
OVERLAY_MAX_SCALE = 4
OVERLAY_MAX_DILATE = 2
OVERLAY_MAX_OUTLINE = 4
OVERLAY_MAX_PRIMS = 1 << 24


def draw_overlay(ctx, images, prims, image_offsets, ids=None, palette=None, fill=False, outline=0, out=None):
    """An ordered list of primitives and an id layer painted over B images in one launch (pp_draw_overlay_u8, the rule in
    include/pyrapose_hip.h): cuda tensors images uint8 [B,H,W,3] (any channel order: colours go by channel index), prims int32
    [n,8] records (kind, a0, a1, a2, a3, size, colour, reserved), image_offsets int32 [B+1] (image b owns the records
    image_offsets[b] .. image_offsets[b+1], later over earlier; read on the device, not checked); the id layer: ids uint8
    [B,H,W] with palette int32 [256] packed colours (entry 0 is never drawn), fill: paint every labelled pixel, outline 0..4: the
    width of the inner contour, 0 = none.  out: None allocates the result, `images` draws in place, otherwise a cuda uint8
    [B,H,W,3] tensor that does not overlap images -> out."""
    what = "draw_overlay"
    if out is images and torch.is_tensor(images) and not images.is_contiguous():
        raise ValueError("%s: drawing in place needs contiguous images" % what)
    in_place = out is images
    images = _arg(what, "images", images, _U8, (None, None, None, 3))
    B, H, W = (int(s) for s in images.shape[:3])
    if B < 1 or not (1 <= H <= OVERLAY_MAX_SIDE and 1 <= W <= OVERLAY_MAX_SIDE):
        raise ValueError("%s: need at least one image of 1..%d x 1..%d pixels, got %d of %d x %d" % (what, OVERLAY_MAX_SIDE, OVERLAY_MAX_SIDE, B, H, W))
    prims = _arg(what, "prims", prims, _I32, (None, 8))
    n = int(prims.shape[0])
    if n > OVERLAY_MAX_PRIMS:
        raise ValueError("%s: %d records, at most %d" % (what, n, OVERLAY_MAX_PRIMS))
    image_offsets = _arg(what, "image_offsets", image_offsets, _I32, (B + 1,))
    ids = _arg(what, "ids", ids, _U8, (B, H, W), optional=True)
    palette = _arg(what, "palette", palette, _I32, (256,), optional=True)
    if ids is not None and palette is None:
        raise ValueError("%s: ids need a palette" % what)
    outline = int(outline)
    if not 0 <= outline <= OVERLAY_MAX_OUTLINE:
        raise ValueError("%s: outline %d, need 0 (none) .. %d" % (what, outline, OVERLAY_MAX_OUTLINE))
    if ids is None and (fill or outline):
        raise ValueError("%s: fill / outline need ids" % what)
    if in_place:
        out = images
    elif out is None:
        out = _out(images, (B, H, W, 3), _U8)
    else:
        ok = torch.is_tensor(out) and out.is_cuda and out.dtype == _U8 and tuple(out.shape) == (B, H, W, 3) and out.is_contiguous()
        if not ok:
            raise ValueError("%s: out must be a contiguous cuda uint8 tensor [%d,%d,%d,3]" % (what, B, H, W))
        if out.data_ptr() != images.data_ptr():
            lo, hi, size = out.data_ptr(), images.data_ptr(), B * H * W * 3
            if lo < hi + size and hi < lo + size:
                raise ValueError("%s: out overlaps images without being images" % what)
    id_mode = (1 if fill else 0) | (2 if outline else 0)
    check(lib.pp_draw_overlay_u8(ctx.handle, B, H, W, _ptr(images), _ptr(out), _ptr(prims) if n else None, _ptr(image_offsets), n,
                                 _ptr(ids), _ptr(palette), id_mode, max(outline, 1)), ctx.handle, "pp_draw_overlay_u8")
    return out


CC_TILE = 32                  # pixels per side of a workgroup's tile of pp_cc_label
CC_MAX_COMPONENTS = 65535
CC_MODES = ("binary", "value")  # in the ABI's order (PP_CC_BINARY, PP_CC_VALUE)
CC_ERRORS = {1: "the tile pass", 2: "a chase", 4: "a union"}  # bits of the error word


def cc_workspace_bytes(N, H, W):
    """the workspace of pp_cc_label: the error word, the parents and the ranks, each rounded up to 256 bytes"""
    return 256 + 2 * ((4 * N * H * W + 255) // 256 * 256)


def cc_label(ctx, planes, connectivity=8, mode="binary", weight=None, max_components=256, check=False):
    """Connected components of N planes in one call (pp_cc_label, the rule in include/pyrapose_hip.h): cuda tensors planes uint8
    [N,H,W] and weight int32 [N,H,W] (>= 0) or None; connectivity 4 | 8; mode 'binary' (non-zero = foreground) | 'value' (equal
    non-zero bytes connect); max_components M in 1..65535 -> dict: labels int32 [N,H,W] (0 = background, 1 .. n in the raster
    order of the components' first pixels: scipy.ndimage.label's numbering, never capped), counts int32 [N] (n, also beyond M),
    stats int32 [N,M,6] (area, x_min, y_min, x_max, y_max, value), sums int64 [N,M,3] (sum_x, sum_y, sum_w), rows from
    min(n, M) on zero, and error int32 [1]: the kernels' error word, 0 unless a loop reached its bound.  No host
    synchronisation; check=True reads the word here (one) and raises RuntimeError on a set bit."""
    what = "cc_label"  # (the scalars first: their refusals need no device tensor)
    if connectivity not in (4, 8):
        raise ValueError("%s: connectivity %r, need 4 or 8" % (what, connectivity))
    if mode not in CC_MODES:
        raise ValueError("%s: mode %r, need %s" % (what, mode, " | ".join(CC_MODES)))
    M = int(max_components)
    if M != max_components or not 1 <= M <= CC_MAX_COMPONENTS:
        raise ValueError("%s: max_components %r, need an integer in 1..%d" % (what, max_components, CC_MAX_COMPONENTS))
    planes, N, H, W = _mask_stack(what, "planes", planes)
    if N < 1:
        raise ValueError("%s: planes must hold at least one plane, got %s" % (what, list(planes.shape)))
    weight = _arg(what, "weight", weight, _I32, (N, H, W), optional=True)
    nbytes = cc_workspace_bytes(N, H, W)
    ws = _workspace(nbytes)
    out = dict(labels=_out(planes, (N, H, W), _I32), counts=_out(planes, (N,), _I32), stats=_out(planes, (N, M, 6), _I32),
               sums=_out(planes, (N, M, 3), _I64))
    check_status(lib.pp_cc_label(ctx.handle, N, H, W, _ptr(planes), int(connectivity), CC_MODES.index(mode), _ptr(weight), M, _ptr(ws),
                                 nbytes, _ptr(out["labels"]), _ptr(out["counts"]), _ptr(out["stats"]), _ptr(out["sums"])),
                 ctx.handle, "pp_cc_label")
    out["error"] = ws[:4].view(_I32)
    if check:
        word = int(out["error"].item())
        if word:
            raise RuntimeError("%s: %s reached its iteration bound (error word %d)" %
                               (what, ", ".join(v for k, v in CC_ERRORS.items() if word & k), word))
    return out


def cc_select(ctx, labels, slot_plane, slot_label):
    """Label planes to instance masks (pp_cc_select): cuda int32 tensors labels [N,H,W], slot_plane [S], slot_label [S] ->
    masks uint8 [S,H,W], masks[s] = (labels[slot_plane[s]] == slot_label[s]) as 0 / 1.  A slot with slot_plane < 0 (or past the
    last plane) or slot_label <= 0 is padding: an all-zero mask, no label plane read."""
    what = "cc_select"
    labels = _arg(what, "labels", labels, _I32, (None, None, None))
    N, H, W = (int(s) for s in labels.shape)
    if N < 1 or H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError("%s: labels needs N, H, W >= 1 and H * W < 2^31, got %s" % (what, list(labels.shape)))
    slot_plane = _arg(what, "slot_plane", slot_plane, _I32, (None,))
    S = int(slot_plane.shape[0])
    slot_label = _arg(what, "slot_label", slot_label, _I32, (S,))
    masks = _out(labels, (S, H, W), _U8)
    check_status(lib.pp_cc_select(ctx.handle, N, H, W, _ptr(labels), S, _ptr(slot_plane), _ptr(slot_label), _ptr(masks)), ctx.handle,
                 "pp_cc_select")
    return masks


MESH_THREADS = 256          # workgroup size of every kernel of csrc/mesh.hip = faces per chunk of the fixed-order float sums
MESH_SCAN_CHUNK = 1024      # quantised areas per workgroup of pp_mesh_sample_surface_f64's integer scan
MESH_MAX_ELEMS = 1 << 22    # vertices and faces at most
MESH_MAX_SAMPLES = 1 << 24
MESH_MAX_ATTR = 8
MESH_MODES = {"random": 0, "weyl": 1}
MESH_SAMPLE_OUTPUTS = ("points", "face", "bary", "normals", "attr_out")  # in the ABI's order


def _mesh_args(what, pts, faces):
    pts = _arg(what, "pts", pts, _F64, (None, 3))
    faces = _arg(what, "faces", faces, _I32, (None, 3))
    n_v, n_f = int(pts.shape[0]), int(faces.shape[0])
    if not (1 <= n_v <= MESH_MAX_ELEMS and 1 <= n_f <= MESH_MAX_ELEMS):
        raise ValueError("%s: need 1..2^22 vertices and faces, got %d and %d" % (what, n_v, n_f))
    return pts, faces, n_v, n_f


def mesh_face_geometry(ctx, pts, faces):
    """Per-face and whole-mesh geometry (pp_mesh_face_geometry_f64, the rules in include/pyrapose_hip.h): cuda float64 pts
    [n_v,3], int32 faces [n_f,3] -> dict: normal float64 [n_f,3] (the cross product, not normalised), area2 [n_f] (its length),
    totals [8] = (sum area2, six signed volumes, the centroid's numerator [3], max area2, 0, 0), status int32 [1] (bit 0: a
    face names a vertex out of range and counts as degenerate; bit 1: every area is zero).  Nothing is read back here."""
    what = "mesh_face_geometry"
    pts, faces, n_v, n_f = _mesh_args(what, pts, faces)
    nbytes = lib.pp_mesh_face_geometry_workspace_bytes(n_f)
    ws = _workspace(nbytes)
    out = dict(normal=_out(pts, (n_f, 3)), area2=_out(pts, (n_f,)), totals=_out(pts, (8,)), status=_out(pts, (1,), _I32))
    check(lib.pp_mesh_face_geometry_f64(ctx.handle, n_v, n_f, _ptr(pts), _ptr(faces), _ptr(ws), nbytes, _ptr(out["normal"]),
                                        _ptr(out["area2"]), _ptr(out["totals"]), _ptr(out["status"])), ctx.handle, "pp_mesh_face_geometry_f64")
    return out


def _mesh_geom(what, geom, n_f):
    if not isinstance(geom, dict):
        raise ValueError("%s: geom must be what mesh_face_geometry returned for this mesh" % what)
    return (_arg(what, "geom['normal']", geom.get("normal"), _F64, (n_f, 3)), _arg(what, "geom['area2']", geom.get("area2"), _F64, (n_f,)),
            _arg(what, "geom['totals']", geom.get("totals"), _F64, (8,)))


def mesh_vertex_normals(ctx, n_v, faces, geom, outward=True):
    """Area-weighted vertex normals and the vertex-to-face adjacency (pp_mesh_vertex_normals_f64): n_v vertices, cuda int32
    faces [n_f,3], geom = mesh_face_geometry's dict of the same mesh -> (vnormal float64 [n_v,3], adj_offsets int32 [n_v+1],
    adj_faces int32 [3 n_f]: the faces of vertex v ascending in adj_faces[adj_offsets[v]:adj_offsets[v+1]], -1 past the last).
    outward: all normals negated when the mesh's signed volume is negative; the sign is read on the device."""
    what = "mesh_vertex_normals"
    faces = _arg(what, "faces", faces, _I32, (None, 3))
    n_v, n_f = int(n_v), int(faces.shape[0])
    if not (1 <= n_v <= MESH_MAX_ELEMS and 1 <= n_f <= MESH_MAX_ELEMS):
        raise ValueError("%s: need 1..2^22 vertices and faces, got %d and %d" % (what, n_v, n_f))
    normal, _, totals = _mesh_geom(what, geom, n_f)
    nbytes = lib.pp_mesh_vertex_normals_workspace_bytes(n_v, n_f)
    ws = _workspace(nbytes)
    vnormal, offsets, adj = _out(faces, (n_v, 3)), _out(faces, (n_v + 1,), _I32), _out(faces, (3 * n_f,), _I32)
    check(lib.pp_mesh_vertex_normals_f64(ctx.handle, n_v, n_f, _ptr(faces), _ptr(normal), _ptr(totals), 1 if outward else 0, _ptr(ws), nbytes,
                                         _ptr(vnormal), _ptr(offsets), _ptr(adj)), ctx.handle, "pp_mesh_vertex_normals_f64")
    return vnormal, offsets, adj


def mesh_sample_surface(ctx, pts, faces, geom, n_samples, seed=0, mode="random", outward=True, attr=None,
                        want=("points", "face", "bary", "normals")):
    """n_samples points uniform by area (pp_mesh_sample_surface_f64): pts, faces and geom as above; seed an integer (taken mod
    2^64); mode 'random' (counter-based splitmix64 draws) | 'weyl' (a low-discrepancy sequence decides the face); attr: cuda
    float64 [n_v,n_attr], 1 <= n_attr <= 8, blended like the points into 'attr_out'; want: which of points [n,3], face int32
    [n], bary [n,3], normals [n,3] (the face's unit normal, outward as for the vertex normals) to compute ('attr_out' comes
    with attr) -> dict of cuda tensors.  A mesh whose areas are all zero gives zeros and face = -1."""
    what = "mesh_sample_surface"  # (the scalars first: their refusals need no device tensor)
    if mode not in MESH_MODES:
        raise ValueError("%s: mode %r, need random | weyl" % (what, mode))
    n = int(n_samples)
    if n != n_samples or not 1 <= n <= MESH_MAX_SAMPLES:
        raise ValueError("%s: n_samples %r, need an integer in 1..2^24" % (what, n_samples))
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(w not in MESH_SAMPLE_OUTPUTS[:4] for w in want):
        raise ValueError("%s: want must name some of %s, got %r" % (what, " | ".join(MESH_SAMPLE_OUTPUTS[:4]), want))
    pts, faces, n_v, n_f = _mesh_args(what, pts, faces)
    normal, area2, totals = _mesh_geom(what, geom, n_f)
    n_attr = 0
    if attr is not None:
        attr = _arg(what, "attr", attr, _F64, (n_v, None))
        n_attr = int(attr.shape[1])
        if not 1 <= n_attr <= MESH_MAX_ATTR:
            raise ValueError("%s: attr must hold 1..%d values per vertex, got %d" % (what, MESH_MAX_ATTR, n_attr))
        want = want + ("attr_out",)
    shapes = dict(points=((n, 3), _F64), face=((n,), _I32), bary=((n, 3), _F64), normals=((n, 3), _F64), attr_out=((n, n_attr), _F64))
    out = {w: _out(pts, *shapes[w]) for w in MESH_SAMPLE_OUTPUTS if w in want}
    nbytes = lib.pp_mesh_sample_surface_workspace_bytes(n_f)
    ws = _workspace(nbytes)
    check(lib.pp_mesh_sample_surface_f64(ctx.handle, n_v, n_f, _ptr(pts), _ptr(faces), _ptr(normal), _ptr(area2), _ptr(totals), n,
                                         int(seed) & (2 ** 64 - 1), MESH_MODES[mode], 1 if outward else 0, n_attr, _ptr(attr), _ptr(ws), nbytes,
                                         *[_ptr(out.get(w)) for w in MESH_SAMPLE_OUTPUTS]), ctx.handle, "pp_mesh_sample_surface_f64")
    return out
