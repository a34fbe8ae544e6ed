"""CPU: analytic known answers for the OpenCV restatement of the augmentation warp / resize (oracle/image_np.py).
OpenCV itself is not installed ("parity unpinned"): these pin what can be derived from the published algorithm alone."""
import numpy as np

from oracle import image_np as IM


def _img(rng, h=37, w=53, c=3):
    return rng.integers(0, 256, size=(h, w, c)).astype(np.uint8)


def test_identity_transform_returns_the_image():
    rng = np.random.default_rng(0)
    img = _img(rng)
    I = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    for border in ("replicate", "constant"):
        assert np.array_equal(IM.warp_affine_u8(img, I, "linear", border), img)
    assert np.array_equal(IM.warp_affine_u8(img[:, :, 0], I, "nearest", "constant"), img[:, :, 0])


def test_integer_translation_shifts_exactly():
    rng = np.random.default_rng(1)
    img = _img(rng)
    M = np.array([[1.0, 0, 5], [0, 1.0, -3]])   # dst(x, y) = src(x - 5, y + 3)
    out = IM.warp_affine_u8(img, M, "linear", "constant", cval=7)
    assert np.array_equal(out[:-3, 5:], img[3:, :-5])
    assert np.all(out[:, :4] == 7) and np.all(out[-2:, :] == 7)       # fully outside -> the border value
    rep = IM.warp_affine_u8(img, M, "linear", "replicate")
    assert np.array_equal(rep[:-3, 5:], img[3:, :-5]) and np.array_equal(rep[0, :5], np.repeat(img[3:4, 0], 5, axis=0))
    msk = IM.warp_affine_u8(img[:, :, 0], M, "nearest", "constant")
    assert np.array_equal(msk[:-3, 5:], img[3:, :-5, 0]) and not msk[:, :5].any()


def test_half_pixel_shift_blends_neighbours():
    img = np.zeros((4, 6, 1), np.uint8)
    img[:, 2] = 100
    img[:, 3] = 201
    out = IM.warp_affine_u8(img, np.array([[1.0, 0, 0.5], [0, 1.0, 0]]), "linear", "replicate")
    # dst(3) = (src(2) + src(3)) / 2 = 150.5 -> 151 with the +2^14 rounding; dst(2) = (0 + 100) / 2
    assert out[1, 3, 0] == 151 and out[1, 2, 0] == 50 and out[1, 4, 0] == 101


def test_scale_two_nearest_replicates_pixels():
    rng = np.random.default_rng(2)
    m = rng.integers(0, 5, size=(8, 10)).astype(np.uint8)
    out = IM.warp_affine_u8(m, np.array([[2.0, 0, 0], [0, 2.0, 0]]), "nearest", "constant")
    # source position = dst / 2 rounded half up at 1/1024 resolution: (x * 512 + 512) >> 10
    xs = (np.arange(10) * 512 + 512) >> 10
    ys = (np.arange(8) * 512 + 512) >> 10
    assert np.array_equal(out, m[ys][:, xs])


def test_resize_scale_and_identity():
    assert IM.compute_resize_scale((480, 640, 3)) == 1.0
    assert IM.compute_resize_scale((540, 720, 3), 540, 720) == 1.0
    assert abs(IM.compute_resize_scale((960, 1280, 3)) - 0.5) < 1e-15
    assert abs(IM.compute_resize_scale((400, 1200, 3)) - 640 / 1200) < 1e-15     # the max side limits
    rng = np.random.default_rng(3)
    img = _img(rng)
    assert np.array_equal(IM.resize_linear_u8(img, 1.0), img)
    # x0.5 on a constant image stays constant; on a 2x2 block pattern it gives the block means
    assert np.all(IM.resize_linear_u8(np.full((8, 8, 3), 93, np.uint8), 0.5) == 93)
    blk = np.kron(np.array([[10, 50], [90, 130]], np.uint8), np.ones((2, 2), np.uint8))
    assert np.array_equal(IM.resize_linear_u8(blk, 0.5), np.array([[10, 50], [90, 130]], np.uint8))
    up = IM.resize_linear_u8(np.array([[0, 100]], np.uint8), 2.0)   # positions -0.25, 0.25, 0.75, 1.25 -> 0, 25, 75, 100
    assert up.shape == (2, 4) and list(up[0]) == [0, 25, 75, 100]


def test_flip_reverses_columns_exactly():
    rng = np.random.default_rng(4)
    img = _img(rng)
    H, W = img.shape[:2]
    flip = np.array([[-1.0, 0, W - 1], [0, 1.0, 0]])     # dst(x, y) = src(W - 1 - x, y): every position an integer
    for border in ("replicate", "constant"):
        assert np.array_equal(IM.warp_affine_u8(img, flip, "linear", border, 9), img[:, ::-1])
        assert np.array_equal(IM.warp_affine_u8(img[:, :, 0], flip, "nearest", border, 9), img[:, ::-1, 0])
    vflip = np.array([[1.0, 0, 0], [0, -1.0, H - 1]])
    assert np.array_equal(IM.warp_affine_u8(img, vflip, "linear", "constant", 9), img[::-1])


def test_singular_matrix_fills_with_the_first_pixel():
    # determinant 0 -> cv::warpAffine takes 1 / D := 0, the inverse map is all zeros, every pixel reads src(0, 0)
    rng = np.random.default_rng(5)
    img = _img(rng)
    for M in (np.array([[1.0, 2, 5], [2, 4.0, 7]]), np.zeros((2, 3))):
        for border in ("replicate", "constant"):
            out = IM.warp_affine_u8(img, M, "linear", border, 9)
            assert np.array_equal(out, np.broadcast_to(img[0, 0], img.shape))
            assert np.all(IM.warp_affine_u8(img[:, :, 1], M, "nearest", border, 9) == img[0, 0, 1])


def test_translation_past_the_int16_range():
    # 40 000 px is beyond the +-32 768 at which remap saturates its positions: still "far outside", on the same side
    rng = np.random.default_rng(6)
    img = _img(rng)
    right = np.array([[1.0, 0, 40000], [0, 1.0, 0]])     # dst(x) = src(x - 40000): left of the image
    left = np.array([[1.0, 0, -40000], [0, 1.0, 0]])     # dst(x) = src(x + 40000): right of it
    down = np.array([[1.0, 0, 0], [0, 1.0, 40000]])
    for M in (right, left, down):
        assert np.all(IM.warp_affine_u8(img, M, "linear", "constant", 17) == 17)
        assert np.all(IM.warp_affine_u8(img[:, :, 0], M, "nearest", "constant", 255) == 255)
    for interp, src in (("linear", img), ("nearest", img[:, :, 0])):
        assert np.array_equal(IM.warp_affine_u8(src, left, interp, "replicate"), np.repeat(src[:, -1:], src.shape[1], axis=1))
        assert np.array_equal(IM.warp_affine_u8(src, right, interp, "replicate"), np.repeat(src[:, :1], src.shape[1], axis=1))
        assert np.array_equal(IM.warp_affine_u8(src, down, interp, "replicate"), np.repeat(src[:1], src.shape[0], axis=0))


def test_two_by_two_half_pixel_shift():
    # source position = dst - 0.5 on both axes: (1024 x - 512 + 16) >> 5 = 32 x - 16 -> sx = x - 1, ax = 16 (and the same in y);
    # the four weights are 16 * 16 * 32 = 8192 each, so dst = (sum of the 2 x 2 neighbourhood + 2) >> 2 with 0 outside
    img = np.array([[100, 50], [30, 201]], np.uint8)
    out = IM.warp_affine_u8(img, np.array([[1.0, 0, 0.5], [0, 1.0, 0.5]]), "linear", "constant", 0)
    # (100 + 2) >> 2, (100 + 50 + 2) >> 2, (100 + 30 + 2) >> 2, (100 + 50 + 30 + 201 + 2) >> 2
    assert out.tolist() == [[25, 38], [33, 95]]
    # the border value takes the place of the zeros: (100 + 3 * 8 + 2) >> 2, (150 + 2 * 8 + 2) >> 2, (130 + 16 + 2) >> 2
    out = IM.warp_affine_u8(img, np.array([[1.0, 0, 0.5], [0, 1.0, 0.5]]), "linear", "constant", 8)
    assert out.tolist() == [[31, 42], [37, 95]]


def test_resize_of_one_row_and_one_column():
    row = np.array([[0, 100, 50]], np.uint8)
    # x2: positions -0.25, 0.25, 0.75, 1.25, 1.75, 2.25 -> 0, 25, 75, 87.5, 62.5, 50; with the 11-bit weights 1536 / 512:
    # 87.5: ((100 * 1536 + 50 * 512) >> 4) * 2048 >> 16 = 350, (350 + 2) >> 2 = 88;  62.5: 250 -> 252 >> 2 = 63
    want = [0, 25, 75, 88, 63, 50]
    up = IM.resize_linear_u8(row, 2.0)
    assert up.shape == (2, 6) and up[0].tolist() == want and up[1].tolist() == want
    up = IM.resize_linear_u8(row.T.copy(), 2.0)
    assert up.shape == (6, 2) and up[:, 0].tolist() == want and up[:, 1].tolist() == want
    up = IM.resize_linear_u8(row[..., None].repeat(3, axis=2), 2.0)
    assert up.shape == (2, 6, 3) and up[1, :, 2].tolist() == want
    assert IM.resize_linear_u8(np.array([[77]], np.uint8), 3.0).tolist() == [[77] * 3] * 3
    assert IM.resize_linear_u8(np.zeros((1, 9), np.uint8), 1.0).shape == (1, 9)
    assert IM.resize_linear_u8(np.zeros((9, 1, 3), np.uint8), 0.5).shape == (4, 0, 3)   # rint(0.5) = 0: an empty side


def test_resize_output_size_rounds_half_to_even():
    # cv::resize: dsize = saturate_cast<int>(size * f) = rint: 5 * 0.5 = 2.5 -> 2 and 7 * 0.5 = 3.5 -> 4
    assert IM.resize_linear_u8(np.zeros((5, 7), np.uint8), 0.5).shape == (2, 4)
    assert IM.resize_linear_u8(np.zeros((7, 5, 3), np.uint8), 0.5).shape == (4, 2, 3)
