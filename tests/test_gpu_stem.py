"""GPU: the 7x7 stride-2 RGB stem the engine runs on the planes path (pp_stem7x7s2_fwd_bf16x3: a 7x1 convolution over 32
overlapping "channels" of the zero-framed 4-channel image) against F.conv2d in float64 on the RGB image, once per plane format.
Bound: 1e-4 of the output's largest magnitude, the figure the bf16x3 convolution tests hold both arithmetics to."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
COUT = 64


@pytest.fixture(scope="module", params=[0, 1], ids=["bf16x3", "f16c8"])
def pctx(request):
    from pyrapose_amd.runtime import default_context
    return default_context().twin(request.param)


def rel_err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def out_hw(H, W):
    return (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1


def reference(x, w, bias, relu):
    """x [B,H,W,3], w [7,7,3,cout] (HWIO) in float64: ZeroPadding2D(3) + 7x7 / 2 -> [B*oh*ow, cout]"""
    y = F.conv2d(torch.as_tensor(x, dtype=torch.float64).permute(0, 3, 1, 2), torch.as_tensor(w, dtype=torch.float64).permute(3, 2, 0, 1),
                 None if bias is None else torch.as_tensor(bias, dtype=torch.float64), stride=2, padding=3)
    if relu:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[3]).numpy()


def stem_weight_rows(w, swapped=False):
    """the row-as-tap layout of the stem's weights, float32 [7 * 32, cout]: kernel row ty is one tap, its 32 "channels" are
    column tx * 4 + c of the frame (zeros for c == 3 and tx == 7).  swapped: the wrong layout c * 8 + tx, for the test that
    shows the comparison tells the two apart"""
    buf = np.zeros((7 * 32, w.shape[3]), np.float32)
    for ty, tx, c in itertools.product(range(7), range(7), range(3)):
        buf[ty * 32 + (c * 8 + tx if swapped else tx * 4 + c)] = w[ty, tx, c]
    return buf


def split_stem_weights(ctx, w, B, Hp, Wp, oh, ow, ld_y, swapped=False):
    """-> (hi, lo) planes [7][cout][32] by conv_split_weights3 on the descriptor of that 7x1 convolution (kw = 1, cin 32)"""
    from pyrapose_amd import ops
    cout = w.shape[3]
    d = ops.make_conv_desc(B, [(Hp, Wp)], [(oh, ow)], 32, cout, 7, 2, 0, 0, 32, ld_y, cout)
    d.kw = 1
    i16 = dict(dtype=torch.int16, device="cuda")
    hi, lo = torch.zeros((7, cout, 32), **i16), torch.zeros((7, cout, 32), **i16)
    ops.conv_split_weights3(ctx, d, torch.from_numpy(stem_weight_rows(w, swapped)).cuda(), hi, lo, None, None)
    return hi, lo


def run_stem(ctx, x, w, bias, relu, Hp, Wp, ld_y, swapped=False):
    """pack x into its frame and run the stem; y [B*oh*ow, ld_y] prefilled with NaN"""
    from pyrapose_amd import ops
    B, H, W, _ = x.shape
    oh, ow = out_hw(H, W)
    x4p = torch.full((B * Hp * Wp, 4), NAN, dtype=torch.float32, device="cuda")
    ops.pack_rgb_to_4_padded(ctx, torch.from_numpy(x).cuda(), x4p, Hp, Wp)
    hi, lo = split_stem_weights(ctx, w, B, Hp, Wp, oh, ow, ld_y, swapped)
    y = torch.full((B * oh * ow, ld_y), NAN, dtype=torch.float32, device="cuda")
    bd = torch.from_numpy(bias).cuda() if bias is not None else None
    ops.stem7x7s2_fwd3(ctx, B, H, W, Hp, Wp, x4p, hi, lo, w.shape[3], bd, relu, y)
    return y


def f32_stem(ctx, x, w, bias, relu):
    """the float32 stem (conv_fwd on the packed cin == 4 input), as test_gpu_conv.test_stem_7x7_rgb runs it"""
    from pyrapose_amd import ops
    B, H, W, _ = x.shape
    oh, ow = out_hw(H, W)
    cout = w.shape[3]
    w4 = np.concatenate([w, np.zeros((7, 7, 1, cout), w.dtype)], axis=2).reshape(-1, cout)
    buf = np.zeros(((w4.shape[0] + 15) // 16 * 16, cout), np.float32)
    buf[: w4.shape[0]] = w4
    x4 = torch.empty((B * H * W, 4), dtype=torch.float32, device="cuda")
    ops.pack_rgb_to_4(ctx, torch.from_numpy(x).cuda(), x4)
    d = ops.make_conv_desc(B, [(H, W)], [(oh, ow)], 4, cout, 7, 2, 3, 3, 4, cout, cout)
    y = torch.empty((B * oh * ow, cout), dtype=torch.float32, device="cuda")
    ops.conv_fwd(ctx, d, x4, torch.from_numpy(buf).cuda(), torch.from_numpy(bias).cuda() if bias is not None else None, None, relu, y)
    return y.cpu().numpy()


def make_case(H, W, B, seed=0):
    rng = np.random.default_rng([seed, H, W, B])
    x = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    w = (rng.standard_normal((7, 7, 3, COUT)) / 12.0).astype(np.float32)
    bias = rng.standard_normal((COUT,)).astype(np.float32)
    return x, w, bias


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [(38, 50), (37, 49), (7, 9), (8, 8)])
def test_stem_vs_float64(pctx, hw, B):
    ctx = pctx
    H, W = hw
    x, w, bias = make_case(H, W, B)
    minimal = (H + 6, (W + 8 + 1) // 2 * 2)  # the engine's frame
    roomy = (H + 9, minimal[1] + 4)          # extra rows below and columns to the right of it
    f32 = {}
    for (Hp, Wp), ld_y, epi in itertools.product((minimal, roomy), (64, 96), (True, False)):
        b = bias if epi else None
        want = reference(x, w, b, epi)
        y = run_stem(ctx, x, w, b, epi, Hp, Wp, ld_y).cpu().numpy()
        what = (hw, B, Hp, Wp, ld_y, epi)
        assert np.isfinite(y[:, :COUT]).all(), what
        e = rel_err(y[:, :COUT], want)
        assert e < 1e-4, (what, e)
        # the epilogue stores the columns below cout rounded up to 4 and nothing else (conv3_shared.h epilogue3: col_ok): the
        # rest of a wider row is left untouched -- here, still the NaN it was prefilled with
        assert np.isnan(y[:, COUT:]).all(), what
        if epi not in f32:
            f32[epi] = f32_stem(ctx, x, w, b, epi)
            assert rel_err(f32[epi], want) < 2e-5
        assert rel_err(y[:, :COUT], f32[epi]) < 1e-4 + 2e-5, what


def test_stem_weight_layout_is_tx_major(pctx):
    """the plane column of tap (tx, c) is tx * 4 + c: weights laid out with the two swapped (c * 8 + tx, also inside the 32
    columns) give the result of another convolution, far outside the bound -- the comparison above would not let it pass"""
    ctx = pctx
    x, w, _ = make_case(8, 8, 1, seed=5)
    want = reference(x, w, None, False)
    assert rel_err(run_stem(ctx, x, w, None, False, 14, 16, 64).cpu().numpy(), want) < 1e-4
    assert rel_err(run_stem(ctx, x, w, None, False, 14, 16, 64, swapped=True).cpu().numpy(), want) > 1e-2


def test_stem_refusals(pctx):
    from pyrapose_amd import ops
    ctx = pctx
    H, W, B = 8, 8, 1
    x, w, bias = make_case(H, W, B, seed=7)
    oh, ow = out_hw(H, W)
    hi, lo = split_stem_weights(ctx, w, B, 14, 16, oh, ow, 64)
    frame = torch.zeros((B * 20 * 20, 4), dtype=torch.float32, device="cuda")  # (room for every refused geometry as well)
    y = torch.full((B * oh * ow, 64), NAN, dtype=torch.float32, device="cuda")
    y32 = torch.full((2 * B * oh * ow, 32), NAN, dtype=torch.float32, device="cuda")
    for (Hp, Wp) in ((14, 17), (13, 16), (14, 14)):  # Wp odd; Hp < H + 6; Wp < W + 8
        with pytest.raises(ValueError):
            ops.stem7x7s2_fwd3(ctx, B, H, W, Hp, Wp, frame, hi, lo, COUT, None, False, y)
    with pytest.raises(ValueError):  # ld_y < cout
        ops.stem7x7s2_fwd3(ctx, B, H, W, 14, 16, frame, hi, lo, COUT, None, False, y32)
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(y32).all())  # no refused call wrote anything
    got = run_stem(ctx, x, w, bias, True, 14, 16, 64).cpu().numpy()
    assert rel_err(got, reference(x, w, bias, True)) < 1e-4
