"""GPU: the pointwise / resampling kernels and the stem packers of csrc/elementwise.hip against the host restatements of
tests/pointwise_np.py, element by element and bit for bit: every float32 form at its edges (1-pixel extents, odd sizes, channel
counts of one float4, -inf / +inf, absent optional operands), every view form over the combinations of input kind (float32 or
planes, per operand) and output kind (float32, planes, both), one case per kernel whose item count exceeds the launch's grid cap
(n_cu * 8 workgroups of 256) so that the grid-stride loop takes a second trip, and the packers' margins and refusals.

Planes inputs are made by split_planes3 and decoded with ops.planes_to_f32 (torch arithmetic); the expected result is the
operation applied in float32 to the decoded values, in the kernel's operand order."""
import itertools

import numpy as np
import pytest
import torch

from tests import pointwise_np as PN

pytestmark = pytest.mark.gpu

NAN = float("nan")
# (sh, sw -> th, tw): identity, 1 pixel, integer and non-integer factors, a factor > 2, one downsampling pair
PAIRS = [(1, 1, 1, 1), (1, 1, 2, 3), (3, 4, 6, 8), (17, 23, 34, 45), (34, 45, 68, 90), (2, 2, 5, 5), (5, 7, 5, 7), (6, 8, 3, 4)]


@pytest.fixture(scope="module")
def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context().twin(0)


@pytest.fixture(scope="module", params=[0, 1], ids=["bf16x3", "f16c8"])
def pctx(ctx, request):
    """the context once per plane format (csrc/planes_fmt.h): bf16 pairs, and P16"""
    return ctx.twin(request.param)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_dev(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def grid_cap(ctx):
    """items one launch of elementwise.hip covers before its grid-stride loop takes a second trip"""
    n_cu, _ = ctx.device_info()
    assert n_cu > 0
    return n_cu * 8 * 256


def rel_err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def values(rng, shape):
    """standard normal, kept away from zero: inside the range of both plane formats (P16: |x| <= 28 672, halves above 6e-8)"""
    x = rng.standard_normal(shape).astype(np.float32)
    return np.where(np.abs(x) < 1e-3, np.float32(1e-3), x)


# ---- float32 forms -------------------------------------------------------------------------------------------------------------
def pool_input(rng, family, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    if family == "negative":  # a zero from the padding would win every border window
        x = -np.abs(x) - np.float32(0.5)
    elif family == "inf":
        u = rng.uniform(size=shape)
        x[u < 0.3] = -np.inf
        x[u > 0.95] = np.inf
        x[0, :, :, 0] = -np.inf  # whole windows of -inf: the result is -inf, not the largest finite float and not 0
    return x


def check_maxpool(ctx, x):
    from pyrapose_amd import ops
    B, h, w, C = x.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    y = nan_dev(B * oh * ow, C)
    ops.maxpool3x3s2(ctx, B, h, w, C, dev(x), oh, ow, y)
    assert torch.equal(y.cpu().view(B, oh, ow, C), torch.from_numpy(PN.maxpool3x3s2(x))), x.shape


@pytest.mark.parametrize("family", ["normal", "negative", "inf"])
def test_maxpool(ctx, family):
    rng = np.random.default_rng(11)
    for (h, w), C, B in itertools.product(((1, 1), (1, 2), (2, 1), (2, 3), (3, 2), (12, 16), (13, 15)), (4, 12, 64), (1, 3)):
        check_maxpool(ctx, pool_input(rng, family, (B, h, w, C)))


def check_upsample(ctx, rng, B, sh, sw, th, tw, C, f64=True):
    from pyrapose_amd import ops
    src, oth = values(rng, (B, sh, sw, C)), values(rng, (B, th, tw, C))
    for other in (oth, None):
        out = nan_dev(B * th * tw, C)
        ops.upsample_add_fwd(ctx, B, sh, sw, th, tw, C, dev(src), dev(other) if other is not None else None, out)
        want = PN.upsample_add_fwd(src, th, tw, other)
        assert torch.equal(out.cpu().view(B, th, tw, C), torch.from_numpy(want)), (sh, sw, th, tw, C, other is not None)
    g, bs = values(rng, (B, th, tw, C)), values(rng, (B, sh, sw, C))
    for base in (bs, None):
        gs = nan_dev(B * sh * sw, C)
        ops.upsample_add_bwd(ctx, B, sh, sw, th, tw, C, dev(g), dev(base) if base is not None else None, gs)
        got = gs.cpu().view(B, sh, sw, C)
        # float32, in the kernel's order of additions (base, target rows, target columns): bit for bit
        assert torch.equal(got, torch.from_numpy(PN.upsample_add_bwd(g, sh, sw, base))), (sh, sw, th, tw, C, base is not None)
        if f64:
            assert rel_err(got.numpy(), PN.upsample_add_bwd(g, sh, sw, base, dtype=np.float64)) < 1e-6


@pytest.mark.parametrize("C", [4, 64])
def test_upsample_add_fwd_bwd(ctx, C):
    rng = np.random.default_rng(12)
    for (sh, sw, th, tw) in PAIRS:
        check_upsample(ctx, rng, 2, sh, sw, th, tw, C)


def check_add_n(ctx, rng, n):
    from pyrapose_amd import ops
    a, b, c = (values(rng, (n,)) for _ in range(3))
    for k in (1, 2, 3):
        out = nan_dev(n)
        ops.add_n(ctx, dev(a), dev(b) if k >= 2 else None, dev(c) if k >= 3 else None, out)
        want = a if k == 1 else (a + b if k == 2 else (a + b) + c)
        assert torch.equal(out.cpu(), torch.from_numpy(want)), (n, k)


def test_add_n(ctx):
    rng = np.random.default_rng(13)
    for n in (4, 1020, 4100):
        check_add_n(ctx, rng, n)


# ---- view forms ----------------------------------------------------------------------------------------------------------------
def split(ctx, t):
    from pyrapose_amd import ops
    hi, lo = ops.new_planes(t.shape[0], t.shape[1])
    ops.split_planes3(ctx, t, hi, lo)
    return hi, lo


class Operand:
    """one input tensor [rows, ld] of a view kernel as float32 ("f") or planes ("p"): .view for the launch, .val = the float32
    values the kernel reads (the tensor itself, or the host-side decode of its planes)"""

    def __init__(self, ctx, x, kind):
        from pyrapose_amd import ops
        self.t = dev(x)
        if kind == "p":
            self.planes = split(ctx, self.t)
            self.view = ops.tview(None, self.planes)
            self.val = ops.planes_to_f32(self.planes, ctx.planes_fmt).cpu().numpy().reshape(x.shape)
            assert rel_err(self.val, x) < 3.1e-5
        else:
            self.view = ops.tview(self.t)
            self.val = x


def check_out(ctx, okind, shape, launch, want, what):
    """run launch(out view) with a float32 output, a planes output or both (all prefilled with NaN) and hold each to `want`"""
    from pyrapose_amd import ops
    want = torch.from_numpy(np.ascontiguousarray(want, np.float32).reshape(shape))
    outf = nan_dev(*shape) if "f" in okind else None
    outp = ops.new_planes(shape[0], shape[1], fill=0x7fc0) if "p" in okind else None
    launch(ops.tview(outf, outp))
    if outf is not None:
        assert torch.equal(outf.cpu(), want), what
    if outp is not None:
        wh, wl = split(ctx, want.cuda())  # both output formats hold the same values
        assert torch.equal(outp[0], wh) and torch.equal(outp[1], wl), what
        dec = ops.planes_to_f32(outp, ctx.planes_fmt).cpu()
        assert float((dec - want).abs().max()) <= 3.1e-5 * float(want.abs().max()), what


KINDS, OUTS = ("f", "p"), ("f", "p", "fp")


@pytest.mark.parametrize("n", [8, 8000])
def test_add_n_v(pctx, n):
    from pyrapose_amd import ops
    ctx, rng = pctx, np.random.default_rng(21)
    xs = [values(rng, (n // 8, 8)) for _ in range(3)]
    for k in (1, 2, 3):
        for kinds in itertools.product(KINDS, repeat=k):
            o = [Operand(ctx, x, kd) for x, kd in zip(xs, kinds)]
            want = o[0].val if k == 1 else (o[0].val + o[1].val if k == 2 else (o[0].val + o[1].val) + o[2].val)
            v = [q.view for q in o] + [None, None]
            for okind in OUTS:
                check_out(ctx, okind, (n // 8, 8), lambda out: ops.add_n_v(ctx, v[0], v[1], v[2], out), want, (n, kinds, okind))


@pytest.mark.parametrize("n", [8, 8000])
def test_relu_fwd_v_values(pctx, n):
    from pyrapose_amd import ops
    ctx, rng = pctx, np.random.default_rng(22)
    x = values(rng, (n // 8, 8))
    x[0, :4] = (0.0, -0.0, 1.5, -1.5)  # exact zeros of both signs
    x.reshape(-1)[5::7] = 0.0
    x.reshape(-1)[6::11] = -0.0
    for kind in KINDS:
        o = Operand(ctx, x, kind)
        want = np.where(o.val > 0, o.val, np.float32(0))
        for okind in OUTS:
            check_out(ctx, okind, x.shape, lambda out: ops.relu_fwd_v(ctx, o.view, out), want, (n, kind, okind))


@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("pair", [(3, 4, 6, 8), (17, 23, 34, 45)], ids=["x2", "x1.96"])
def test_upsample_add_v(pctx, pair, C):
    from pyrapose_amd import ops
    ctx, rng, B = pctx, np.random.default_rng(23), 2
    sh, sw, th, tw = pair
    src, oth, g, bs = (values(rng, s) for s in ((B * sh * sw, C), (B * th * tw, C), (B * th * tw, C), (B * sh * sw, C)))
    S, T = (B, sh, sw, C), (B, th, tw, C)
    for ks, ko in itertools.product(KINDS, ("f", "p", None)):
        a, b = Operand(ctx, src, ks), (Operand(ctx, oth, ko) if ko else None)
        want = PN.upsample_add_fwd(a.val.reshape(S), th, tw, b.val.reshape(T) if b else None)
        for okind in OUTS:
            check_out(ctx, okind, oth.shape, lambda out: ops.upsample_add_fwd_v(ctx, B, sh, sw, th, tw, C, a.view, b.view if b else None, out),
                      want, ("fwd", pair, C, ks, ko, okind))
    for kg, kb in itertools.product(KINDS, ("f", "p", None)):
        a, b = Operand(ctx, g, kg), (Operand(ctx, bs, kb) if kb else None)
        want = PN.upsample_add_bwd(a.val.reshape(T), sh, sw, b.val.reshape(S) if b else None)
        for okind in OUTS:
            check_out(ctx, okind, src.shape, lambda out: ops.upsample_add_bwd_v(ctx, B, sh, sw, th, tw, C, a.view, b.view if b else None, out),
                      want, ("bwd", pair, C, kg, kb, okind))


def test_merge_planes(pctx):
    from pyrapose_amd import ops
    ctx, rng = pctx, np.random.default_rng(24)
    for n in (8, 8000):
        o = Operand(ctx, values(rng, (n // 8, 8)), "p")
        back = nan_dev(n // 8, 8)
        ops.merge_planes3(ctx, o.planes, back)
        assert torch.equal(back.cpu(), torch.from_numpy(o.val)), n


# ---- beyond the grid cap: the second trip of every grid-stride loop ----------------------------------------------------------------
def test_cap_add_n(ctx):
    n4 = grid_cap(ctx) + 1237
    assert n4 > grid_cap(ctx)
    check_add_n(ctx, np.random.default_rng(31), 4 * n4)


def test_cap_views(pctx):
    from pyrapose_amd import ops
    ctx, rng = pctx, np.random.default_rng(32)
    n8 = grid_cap(ctx) + 1237
    assert n8 > grid_cap(ctx)
    a, b, c = (values(rng, (n8, 8)) for _ in range(3))
    a.reshape(-1)[3::5] = 0.0
    a.reshape(-1)[4::9] = -0.0
    oa, ob, oc = Operand(ctx, a, "p"), Operand(ctx, b, "f"), Operand(ctx, c, "p")
    check_out(ctx, "fp", a.shape, lambda out: ops.add_n_v(ctx, oa.view, ob.view, oc.view, out), (oa.val + ob.val) + oc.val, "add_n_v")
    check_out(ctx, "fp", a.shape, lambda out: ops.relu_fwd_v(ctx, oa.view, out), np.where(oa.val > 0, oa.val, np.float32(0)), "relu_fwd_v")
    back = nan_dev(n8, 8)
    ops.merge_planes3(ctx, oa.planes, back)
    assert torch.equal(back.cpu(), torch.from_numpy(oa.val))


def test_cap_maxpool(ctx):
    cap, B, C = grid_cap(ctx), 2, 256
    oh = (int(np.ceil(np.sqrt(cap / (B * C // 4)))) + 1) | 1  # (odd: the item count is then no multiple of the workgroup size)
    h, w = 2 * oh - 1, 2 * oh - 1  # (256 CUs: 129 x 129 -> 65 x 65 x 2 x 64 = 540 800 float4)
    assert B * oh * oh * (C // 4) > cap and (B * oh * oh * (C // 4)) % 256 != 0
    check_maxpool(ctx, pool_input(np.random.default_rng(33), "negative", (B, h, w, C)))


def _cap_side(ctx, c4):
    """odd extent t with t * (t + 2) * c4 items beyond the cap; both extents odd, so the count is no multiple of the workgroup size"""
    return (int(np.sqrt(grid_cap(ctx) / c4)) + 2) | 1


def test_cap_upsample_fwd(ctx):
    from pyrapose_amd import ops
    rng, C = np.random.default_rng(34), 64
    th = _cap_side(ctx, C // 4)
    tw = th + 2
    sh, sw = (th + 1) // 2, (tw + 1) // 2
    assert th * tw * (C // 4) > grid_cap(ctx) and (th * tw * (C // 4)) % 256 != 0
    src, oth = values(rng, (1, sh, sw, C)), values(rng, (1, th, tw, C))
    out = nan_dev(th * tw, C)
    ops.upsample_add_fwd(ctx, 1, sh, sw, th, tw, C, dev(src), dev(oth), out)
    assert torch.equal(out.cpu().view(1, th, tw, C), torch.from_numpy(PN.upsample_add_fwd(src, th, tw, oth)))


def test_cap_upsample_bwd(ctx):
    from pyrapose_amd import ops
    rng, C = np.random.default_rng(35), 64
    sh = _cap_side(ctx, C // 4)
    sw = sh + 2
    th, tw = 2 * sh, 2 * sw + 1
    assert sh * sw * (C // 4) > grid_cap(ctx) and (sh * sw * (C // 4)) % 256 != 0
    g, base = values(rng, (1, th, tw, C)), values(rng, (1, sh, sw, C))
    gs = nan_dev(sh * sw, C)
    ops.upsample_add_bwd(ctx, 1, sh, sw, th, tw, C, dev(g), dev(base), gs)
    assert torch.equal(gs.cpu().view(1, sh, sw, C), torch.from_numpy(PN.upsample_add_bwd(g, sh, sw, base)))


def test_cap_packers(ctx):
    B = 3
    H = (int(np.sqrt(grid_cap(ctx) / B)) + 2) | 1
    W = H + 4
    Hp, Wp = H + 6, (W + 8 + 1) // 2 * 2
    # (the plain forms: pixels of the image; the padded ones cover the larger frame)
    assert B * H * W > grid_cap(ctx) and (B * H * W) % 256 != 0 and (B * Hp * Wp) % 256 != 0
    check_packers(ctx, np.random.default_rng(36), B, H, W, [(Hp, Wp, 3)], [(H, W), (H - 3, W - 1), (0, 0)])


# ---- packers ---------------------------------------------------------------------------------------------------------------------
def check_packers(ctx, rng, B, H, W, frames, sizes):
    """all four packers on one batch: NaN-prefilled outputs equal the restatement word for word (margin and channel 3 are written
    zeros, not leftovers)"""
    from pyrapose_amd import ops
    x3 = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    u8 = rng.integers(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    out = nan_dev(B * H * W, 4)
    ops.pack_rgb_to_4(ctx, dev(x3), out)
    assert np.array_equal(out.cpu().numpy().reshape(B, H, W, 4), PN.pack_rgb_padded(x3, H, W, 0))
    out.fill_(NAN)
    ops.preprocess_caffe_u8(ctx, dev(u8), sizes, out)
    assert np.array_equal(out.cpu().numpy().reshape(B, H, W, 4), PN.preprocess_caffe_u8_padded(u8, sizes, H, W, 0))
    for (Hp, Wp, pad) in frames:
        outp = nan_dev(B * Hp * Wp, 4)
        ops.pack_rgb_to_4_padded(ctx, dev(x3), outp, Hp, Wp, pad)
        assert np.array_equal(outp.cpu().numpy().reshape(B, Hp, Wp, 4), PN.pack_rgb_padded(x3, Hp, Wp, pad)), (Hp, Wp, pad)
        outp.fill_(NAN)
        ops.preprocess_caffe_u8_padded(ctx, dev(u8), sizes, outp, Hp, Wp, pad)
        assert np.array_equal(outp.cpu().numpy().reshape(B, Hp, Wp, 4), PN.preprocess_caffe_u8_padded(u8, sizes, Hp, Wp, pad)), (Hp, Wp, pad)


@pytest.mark.parametrize("hw", [(37, 49), (38, 50)])
def test_packers(ctx, hw):
    H, W = hw
    engine_frame = (H + 6, (W + 8 + 1) // 2 * 2, 3)  # the frame Engine gives the bf16x3 stem
    frames = [engine_frame, (H + 11, W + 15, 3), (H + 2, W + 1, 1), (H, W, 0)]
    for sizes in ([(H, W)] * 3, [(H - 5, W), (0, 0), (1, W - 7)]):
        check_packers(ctx, np.random.default_rng(41), 3, H, W, frames, sizes)


def test_packer_refusals(ctx):
    from pyrapose_amd import ops
    rng, B, H, W = np.random.default_rng(42), 3, 6, 7
    Hp, Wp = H + 6, 16
    x3, u8 = dev(rng.standard_normal((B, H, W, 3)).astype(np.float32)), dev(rng.integers(0, 256, size=(B, H, W, 3)).astype(np.uint8))
    big = nan_dev(80 * Hp * Wp, 4)  # (room for every refused geometry as well)
    with pytest.raises(ValueError):  # more than 64 images per call (their sizes travel as a kernel argument)
        ops.preprocess_caffe_u8(ctx, torch.zeros((65, H, W, 3), dtype=torch.uint8, device="cuda"), [(H, W)] * 65, big)
    with pytest.raises(ValueError):
        ops.preprocess_caffe_u8_padded(ctx, torch.zeros((65, H, W, 3), dtype=torch.uint8, device="cuda"), [(H, W)] * 65, big, Hp, Wp)
    for sizes in ([(H + 1, W)] + [(H, W)] * 2, [(H, W)] * 2 + [(H, W + 1)], [(-1, W)] + [(H, W)] * 2):  # an image outside the batch frame
        with pytest.raises(ValueError):
            ops.preprocess_caffe_u8(ctx, u8, sizes, big)
        with pytest.raises(ValueError):
            ops.preprocess_caffe_u8_padded(ctx, u8, sizes, big, Hp, Wp)
    for (hp, wp) in ((H + 2, Wp), (Hp, W + 2)):  # a frame smaller than H + pad / W + pad
        with pytest.raises(ValueError):
            ops.pack_rgb_to_4_padded(ctx, x3, big, hp, wp, 3)
        with pytest.raises(ValueError):
            ops.preprocess_caffe_u8_padded(ctx, u8, [(H, W)] * B, big, hp, wp, 3)
    assert bool(torch.isnan(big).all())  # no refused call wrote anything
    check_packers(ctx, rng, B, H, W, [(Hp, Wp, 3)], [(H, W), (2, 3), (0, 0)])
