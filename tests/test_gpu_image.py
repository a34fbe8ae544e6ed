"""GPU: the augmentation warp / resize kernels (pp_warp_affine_u8, pp_resize_linear_u8) against the numpy restatement of
OpenCV's fixed-point scheme (oracle/image_np.py): integer arithmetic on both sides -> bit-exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


def random_transform(rng, H, W):
    """the kind of matrix utils/transform.py:random_transform_generator produces: scaling 0.9..1.1 and a translation about the
    image centre (bin/train.py:189-199), plus a small rotation / shear to exercise every matrix entry"""
    s = rng.uniform(0.8, 1.2)
    a = rng.uniform(-0.2, 0.2)
    sh = rng.uniform(-0.1, 0.1)
    A = np.array([[s * np.cos(a), -s * np.sin(a + sh)], [s * np.sin(a), s * np.cos(a + sh)]])
    c = np.array([0.5 * W, 0.5 * H])
    t = c - A @ c + rng.uniform(-0.2, 0.2, 2) * np.array([W, H])
    return np.concatenate([A, t[:, None]], axis=1)


def test_warp_affine_bit_exact_vs_oracle(ctx):
    from oracle import image_np as IM
    from pyrapose_amd import ops
    rng = np.random.default_rng(0)
    B, H, W = 5, 97, 131
    img = rng.integers(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    msk = rng.integers(0, 4, size=(B, H, W)).astype(np.uint8)
    mats = [random_transform(rng, H, W) for _ in range(B)]
    mats[0] = np.array([[1.0, 0, 0], [0, 1.0, 0]])           # identity
    mats[1] = np.array([[1.0, 0, 7], [0, 1.0, -4]])          # integer shift
    d_img, d_msk = torch.from_numpy(img).cuda(), torch.from_numpy(msk).cuda()
    for border, cval in (("replicate", 0), ("constant", 0), ("constant", 17)):
        got = ops.warp_affine_u8(ctx, d_img, mats, "linear", border, cval).cpu().numpy()
        for b in range(B):
            want = IM.warp_affine_u8(img[b], mats[b], "linear", border, cval)
            assert np.array_equal(got[b], want), (border, cval, b, int(np.abs(got[b].astype(int) - want).max()))
    assert np.array_equal(ops.warp_affine_u8(ctx, d_img, mats, "linear", "replicate").cpu().numpy()[0], img[0])
    got = ops.warp_affine_u8(ctx, d_msk, mats, "nearest", "constant", 0).cpu().numpy()   # apply_transform2mask
    for b in range(B):
        assert np.array_equal(got[b], IM.warp_affine_u8(msk[b], mats[b], "nearest", "constant", 0)), b
    # 3x3 matrices (the reference carries homogeneous transforms and slices [:2]) are accepted as they are
    m33 = [np.vstack([m, [0, 0, 1]]) for m in mats]
    assert np.array_equal(ops.warp_affine_u8(ctx, d_msk, m33, "nearest", "constant", 0).cpu().numpy(), got)
    with pytest.raises(ValueError):
        ops.warp_affine_u8(ctx, d_img, mats, "nearest")      # nearest is the 1-channel mask path


def test_warp_at_640x480_batch8(ctx):
    """the bench batch shape: a quick whole-batch equality and a timing line"""
    from oracle import image_np as IM
    from pyrapose_amd import ops
    rng = np.random.default_rng(1)
    B, H, W = 8, 480, 640
    img = rng.integers(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    mats = [random_transform(rng, H, W) for _ in range(B)]
    d = torch.from_numpy(img).cuda()
    out = torch.empty_like(d)
    ops.warp_affine_u8(ctx, d, mats, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        ops.warp_affine_u8(ctx, d, mats, out=out)
    e1.record()
    torch.cuda.synchronize()
    print("warpAffine 8 x 640x480x3 uint8: %.1f us per batch" % (e0.elapsed_time(e1) * 100))
    got = out.cpu().numpy()
    for b in range(B):     # every image: the grid-stride loop wraps inside image 3
        assert np.array_equal(got[b], IM.warp_affine_u8(img[b], mats[b])), b


def test_resize_bit_exact_vs_oracle(ctx):
    from oracle import image_np as IM
    from pyrapose_amd import ops
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, size=(3, 60, 84, 3)).astype(np.uint8)
    d = torch.from_numpy(img).cuda()
    for scale in (1.0, 0.5, 2.0, 480 / 540, 640 / 84, 0.37):
        got = ops.resize_linear_u8(ctx, d, scale).cpu().numpy()
        for b in range(3):
            want = IM.resize_linear_u8(img[b], scale)
            assert got[b].shape == want.shape and np.array_equal(got[b], want), (scale, b)
    assert ops.resize_scale(480, 640) == 1.0 and ops.resize_scale(540, 720, 540, 720) == 1.0
    assert ops.resize_scale(400, 1200) == IM.compute_resize_scale((400, 1200, 3))
    g1 = ops.resize_linear_u8(ctx, torch.from_numpy(img[:, :, :, 0].copy()).cuda(), 0.5).cpu().numpy()
    assert np.array_equal(g1[1], IM.resize_linear_u8(img[1, :, :, 0], 0.5))


def test_lean_feed_with_device_augmentation(ctx):
    """Engine.train_step_from_annotations(transforms=...): identity transforms change nothing; a real transform gives the
    step that the same feed takes on the host-warped image and mask (oracle warp) -- losses equal."""
    import bench
    from oracle import image_np as IM
    from pyrapose_amd import arch
    from pyrapose_amd.engine import Engine
    B, H, W, C = 2, 96, 128, 5
    rng = np.random.default_rng(5)
    _, images, anns = bench.synth_batch(B, H, W, C, seed=3, side=(20, 50))
    u8 = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    Wt = arch.init_weights(C, seed=4)
    ident = [np.eye(3) for _ in range(B)]
    mats = [random_transform(rng, H, W) for _ in range(B)]

    def step(img, ann, tf):
        eng = Engine(ctx, C, B, H, W, weights=Wt, train=True)
        eng.train_step_from_annotations(torch.from_numpy(img).cuda(), ann, transforms=tf)
        torch.cuda.synchronize()
        out = eng.losses()
        eng.close()
        return out
    base = step(u8, anns, None)
    same = step(u8, anns, ident)
    assert all(abs(base[k] - same[k]) <= 1e-6 * max(abs(base[k]), 1e-6) for k in base)
    dev = step(u8, anns, mats)
    warped = np.stack([IM.warp_affine_u8(u8[b], mats[b], "linear", "replicate") for b in range(B)])
    anns_w = []
    for b, a in enumerate(anns):
        a2 = dict(a)
        a2["mask"] = [IM.warp_affine_u8(np.asarray(a["mask"][0], np.uint8), mats[b], "nearest", "constant", 0)]
        anns_w.append(a2)
    host = step(warped, anns_w, None)
    assert all(abs(dev[k] - host[k]) <= 1e-6 * max(abs(host[k]), 1e-6) for k in host), (dev, host)
    assert abs(dev["total"] - base["total"]) > 1e-4   # (the transform did change the step)


# ---- the warp and resize kernels at their edges (all bit-equal to oracle/image_np.py) ----
def edge_matrices(H, W):
    """forward 2x3 matrices that leave the comfortable middle: flips, a singular matrix, translations past the int16 saturation
    of the source position, translations that leave one row / column inside, strong scalings, sub-pixel shifts"""
    T = lambda tx, ty: [[1.0, 0, tx], [0, 1.0, ty]]
    named = [
        ("identity", T(0, 0)),
        ("hflip", [[-1.0, 0, W - 1], [0, 1.0, 0]]),
        ("vflip", [[1.0, 0, 0], [0, -1.0, H - 1]]),
        ("turn180", [[-1.0, 0, W - 1], [0, -1.0, H - 1]]),
        ("singular", [[1.0, 2.0, 5], [2.0, 4.0, 7]]),
        ("zero", [[0.0, 0, 0], [0, 0.0, 0]]),
        ("x+40000", T(40000, 0)), ("x-40000", T(-40000, 0)), ("y+40000", T(0, 40000)), ("y-40000", T(0, -40000)),
        ("last column only", T(W - 1, 0)), ("first column only", T(-(W - 1), 0)),
        ("last row only", T(0, H - 1)), ("first row only", T(0, -(H - 1))),
        ("one past: nothing inside", T(W, H)),
        ("scale 0.1", [[0.1, 0, 0], [0, 0.1, 0]]),
        ("scale 0.1 about the centre", [[0.1, 0, 0.45 * W], [0, 0.1, 0.45 * H]]),
        ("scale 8", [[8.0, 0, 0], [0, 8.0, 0]]),
        ("scale 8 about the centre", [[8.0, 0, -3.5 * W], [0, 8.0, -3.5 * H]]),
        ("half pixel", T(0.5, 0.5)), ("minus half pixel", T(-0.5, -0.5)),
        ("1/64 pixel: the rounding bit of the 1/32 grid", T(1 / 64, -1 / 64)),
        ("1/2048 pixel: the rounding bit of the 1/1024 grid", T(-1 / 2048, 1 / 2048)),
        ("flip and half pixel", [[-1.0, 0, W - 1.5], [0, -1.0, H - 1.5]]),
    ]
    return [n for n, _ in named], [np.array(m, np.float64) for _, m in named]


EDGE_SHAPES = [(37, 53), (2, 2), (2, 301), (301, 2)]


@pytest.mark.parametrize("hw", EDGE_SHAPES)
@pytest.mark.parametrize("channels", [3, 1])
def test_warp_linear_edge_matrices(ctx, hw, channels):
    from oracle import image_np as IM
    from pyrapose_amd import ops
    H, W = hw
    names, mats = edge_matrices(H, W)
    B = len(mats)
    rng = np.random.default_rng(H * 1000 + W + channels)
    img = rng.integers(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    img = img if channels == 3 else np.ascontiguousarray(img[..., 0])
    d = torch.from_numpy(img).cuda()
    for border, cval in (("replicate", 0), ("constant", 0), ("constant", 17)):
        got = ops.warp_affine_u8(ctx, d, mats, "linear", border, cval).cpu().numpy()
        for b in range(B):
            want = IM.warp_affine_u8(img[b], mats[b], "linear", border, cval)
            assert np.array_equal(got[b], want), (names[b], border, cval, int((got[b] != want).sum()))


@pytest.mark.parametrize("hw", EDGE_SHAPES)
def test_warp_nearest_edge_matrices(ctx, hw):
    """the mask path with the replicate border and with a non-zero border value, on a mask that holds 255"""
    from oracle import image_np as IM
    from pyrapose_amd import ops
    H, W = hw
    names, mats = edge_matrices(H, W)
    B = len(mats)
    rng = np.random.default_rng(H * 1000 + W)
    msk = rng.choice(np.array([0, 1, 2, 254, 255], np.uint8), size=(B, H, W))
    d = torch.from_numpy(msk).cuda()
    for border, cval in (("replicate", 0), ("constant", 0), ("constant", 255), ("constant", 7)):
        got = ops.warp_affine_u8(ctx, d, mats, "nearest", border, cval).cpu().numpy()
        for b in range(B):
            want = IM.warp_affine_u8(msk[b], mats[b], "nearest", border, cval)
            assert np.array_equal(got[b], want), (names[b], border, cval, int((got[b] != want).sum()))


def test_warp_batch_of_64_and_refusals(ctx):
    """PP_WARP_MAX_IMG = 64 matrices travel as one kernel argument: 64 distinct ones, every image checked; 65 refused.  Every
    refusal is a ValueError raised by the host check, before any launch."""
    from oracle import image_np as IM
    from pyrapose_amd import ops
    rng = np.random.default_rng(64)
    B, H, W = 64, 19, 23
    img = rng.integers(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    mats = [random_transform(rng, H, W) for _ in range(B)]
    d = torch.from_numpy(img).cuda()
    got = ops.warp_affine_u8(ctx, d, mats, "linear", "constant", 17).cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], IM.warp_affine_u8(img[b], mats[b], "linear", "constant", 17)), b
    msk = np.ascontiguousarray(img[..., 0])
    got = ops.warp_affine_u8(ctx, torch.from_numpy(msk).cuda(), mats, "nearest", "replicate").cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], IM.warp_affine_u8(msk[b], mats[b], "nearest", "replicate")), b
    d65 = torch.zeros((65, H, W, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ops.warp_affine_u8(ctx, d65, mats + mats[:1])
    I = [np.eye(3)]
    with pytest.raises(ValueError):
        ops.warp_affine_u8(ctx, torch.zeros((1, 1, 9, 3), dtype=torch.uint8, device="cuda"), I)        # H = 1
    with pytest.raises(ValueError):
        ops.warp_affine_u8(ctx, torch.zeros((1, 9, 1, 3), dtype=torch.uint8, device="cuda"), I)        # W = 1
    with pytest.raises(ValueError):
        ops.warp_affine_u8(ctx, d[:1], I, out=d[:1])                                                   # in place
    with pytest.raises(ValueError):
        ops.warp_affine_u8(ctx, d[:1], I, "linear", "constant", 256)                                   # cval
    with pytest.raises(ValueError):
        ops.warp_affine_u8(ctx, d[:1], I, "linear", "constant", -1)


def _stride_shape():
    """an [2, H, 1024] batch whose pixel count just exceeds the n_cu * 16 blocks x 256 threads the image kernels launch at most
    (1 048 576 on a 256-CU part): H = 2 * n_cu + 1 -> 4096 * n_cu + 2048 pixels, the last 2048 on the second trip"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B, H, W = 2, 2 * n_cu + 1, 1024
    assert B * H * W > n_cu * 16 * 256 and B * H * W < 2 * n_cu * 16 * 256
    return B, H, W


@pytest.mark.parametrize("interpolation", ["linear", "nearest"])
def test_warp_stride_loop_second_trip(ctx, interpolation):
    """every pixel compared; run into an output pre-filled with 0 and with 255, so that a pixel no thread wrote cannot pass"""
    from oracle import image_np as IM
    from pyrapose_amd import ops
    B, H, W = _stride_shape()
    rng = np.random.default_rng(H)
    shape = (B, H, W, 3) if interpolation == "linear" else (B, H, W)
    img = rng.integers(0, 256, size=shape).astype(np.uint8)
    mats = [random_transform(rng, H, W) for _ in range(B)]
    want = np.stack([IM.warp_affine_u8(img[b], mats[b], interpolation, "constant", 17) for b in range(B)])
    d = torch.from_numpy(img).cuda()
    for fill in (0, 255):
        out = torch.full_like(d, fill)
        ops.warp_affine_u8(ctx, d, mats, interpolation, "constant", 17, out=out)
        assert np.array_equal(out.cpu().numpy(), want), fill


def test_resize_stride_loop_second_trip(ctx):
    from oracle import image_np as IM
    from pyrapose_amd import ops
    B, H, W = _stride_shape()
    rng = np.random.default_rng(H + 1)
    src = rng.integers(0, 256, size=(B, (H + 1) // 2, W // 2, 3)).astype(np.uint8)     # x2 -> [2, H + 1, 1024]
    got = ops.resize_linear_u8(ctx, torch.from_numpy(src).cuda(), 2.0).cpu().numpy()
    assert got.shape == (B, H + 1, W, 3)
    for b in range(B):
        assert np.array_equal(got[b], IM.resize_linear_u8(src[b], 2.0)), b


RESIZE_CASES = [((1, 9), 1.0), ((1, 9), 2.0), ((1, 9), 3.0), ((1, 9), 7.62), ((9, 1), 1.0), ((9, 1), 2.0), ((9, 1), 3.0),
                ((9, 1), 7.62), ((1, 1), 1.0), ((1, 1), 3.0), ((1, 1), 7.62),
                ((60, 84), 0.0125), ((60, 84), 0.02), ((84, 60), 0.02),        # 1 x 1, one row (1 x 2), one column (2 x 1)
                ((60, 84), 0.05), ((60, 84), 3.0), ((60, 84), 7.62), ((61, 85), 0.05), ((61, 85), 7.62),
                ((5, 7), 0.5), ((7, 5), 0.5), ((60, 84), 0.37), ((60, 84), 480 / 540)]


@pytest.mark.parametrize("channels", [3, 1])
def test_resize_edge_shapes_and_scales(ctx, channels):
    from oracle import image_np as IM
    from pyrapose_amd import ops
    rng = np.random.default_rng(70 + channels)
    for (SH, SW), scale in RESIZE_CASES:
        src = rng.integers(0, 256, size=(2, SH, SW, 3)).astype(np.uint8)
        src = src if channels == 3 else np.ascontiguousarray(src[..., 0])
        got = ops.resize_linear_u8(ctx, torch.from_numpy(src).cuda(), scale).cpu().numpy()
        for b in range(2):
            want = IM.resize_linear_u8(src[b], scale)
            assert got[b].shape == want.shape and np.array_equal(got[b], want), (SH, SW, scale, b)
    assert ops.resize_linear_u8(ctx, torch.zeros((1, 5, 7), dtype=torch.uint8, device="cuda"), 0.5).shape == (1, 2, 4)   # 2.5 -> 2, 3.5 -> 4
    assert ops.resize_linear_u8(ctx, torch.zeros((1, 60, 84), dtype=torch.uint8, device="cuda"), 0.02).shape == (1, 1, 2)


def test_resize_refusals(ctx):
    """a wrong output size through the C ABI is refused with the size the call must have; a scale that rounds a side to 0 is refused"""
    import ctypes
    from pyrapose_amd import ops
    from pyrapose_amd._lib import check, lib
    src = torch.zeros((1, 60, 84, 3), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((1, 40, 50, 3), dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for dh, dw in ((31, 42), (30, 43), (29, 42), (42, 30)):         # 60 * 0.5 = 30, 84 * 0.5 = 42
        with pytest.raises(ValueError, match="30 x 42"):
            check(lib.pp_resize_linear_u8(ctx.handle, 1, 60, 84, 3, 0.5, dh, dw, p(src), p(dst)), ctx.handle, "pp_resize_linear_u8")
    check(lib.pp_resize_linear_u8(ctx.handle, 1, 60, 84, 3, 0.5, 30, 42, p(src), p(dst)), ctx.handle, "pp_resize_linear_u8")
    with pytest.raises(ValueError, match="0 x 1"):                  # rint(60 * 0.008 = 0.48) = 0, rint(84 * 0.008 = 0.672) = 1
        check(lib.pp_resize_linear_u8(ctx.handle, 1, 60, 84, 3, 0.008, 0, 1, p(src), p(dst)), ctx.handle, "pp_resize_linear_u8")
    with pytest.raises(ValueError):
        ops.resize_linear_u8(ctx, src, 0.008)
    with pytest.raises(ValueError):
        ops.resize_linear_u8(ctx, torch.zeros((1, 1, 9), dtype=torch.uint8, device="cuda"), 0.5)     # rint(0.5) = 0 rows
    with pytest.raises(ValueError):
        ops.resize_linear_u8(ctx, src, 0.0)
