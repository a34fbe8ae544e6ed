"""CPU (no GPU): the numpy restatement of the photometric ops (tests/photo_np.py) against independent implementations and
analytic cases; the host sampler and packer of pyrapose_amd/utils/photometric.py."""
import numpy as np
import pytest

from tests import photo_np as PN
from pyrapose_amd.utils import photometric as PH


def _img(seed, h=37, w=53):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


# ---------------------------------------------------------------------------- against scipy
@pytest.mark.parametrize("k", [3, 5, 7])
def test_median_equals_scipy(k):
    ndi = pytest.importorskip("scipy.ndimage")
    img = _img(k)
    want = np.stack([ndi.median_filter(img[..., c], size=k, mode="nearest") for c in range(3)], axis=-1)
    assert np.array_equal(PN.median(img, k), want)


@pytest.mark.parametrize("name", ["gauss5", "gauss7", "avg3", "avg4", "avg7", "motion5", "motion7"])
def test_conv_within_one_level_of_scipy_float64(name):
    """float32 accumulation of <= 49 byte-valued terms cannot move a value by a level, only flip a rounding"""
    ndi = pytest.importorskip("scipy.ndimage")
    taps = dict(gauss5=PH.gaussian_taps(0.8), gauss7=PH.gaussian_taps(1.9), avg3=PH.average_taps(3), avg4=PH.average_taps(4),
                avg7=PH.average_taps(7), motion5=PH.motion_taps(5, 33.0, 0.4), motion7=PH.motion_taps(7, 200.0, -0.7))[name]
    img = _img(11)
    got = PN.conv(img, taps).astype(np.int32)
    ref = np.stack([ndi.correlate(img[..., c].astype(np.float64), taps.astype(np.float64), mode="mirror") for c in range(3)], axis=-1)
    want = np.clip(np.rint(ref), 0, 255).astype(np.int32)
    assert np.abs(got - want).max() <= 1
    assert np.mean(got != want) < 0.01  # (flipped roundings are rare)


# ---------------------------------------------------------------------------- analytic cases
def test_constant_image_is_a_fixed_point_of_every_blur():
    img = np.empty((20, 30, 3), np.uint8)
    img[...] = (17, 200, 99)
    space, colour = PH.bilateral_tables(7, 40.0, 30.0)
    for out in (PN.conv(img, PH.gaussian_taps(1.3)), PN.conv(img, PH.average_taps(5)), PN.conv(img, PH.average_taps(6)),
                PN.conv(img, PH.motion_taps(7, 45.0, 0.2)), PN.median(img, 5), PN.bilateral(img, space, colour)):
        assert np.array_equal(out, img)


def test_identities():
    img = _img(3)
    assert np.array_equal(PN.lut(img, PH.lut_identity()), img)
    assert np.array_equal(PN.gray(img, 0.0), img)
    assert np.array_equal(PN.huesat(img, 0, 0), img)
    for t in (PH.lut_add(0), PH.lut_multiply(1.0), PH.lut_gamma(1.0)):
        assert np.array_equal(t, PH.lut_identity())
    m = np.random.default_rng(0).uniform(size=(5, 9)).astype(np.float32)
    assert np.array_equal(PN.blend(img, PH.lut_identity(), PH.lut_identity(), m), img)


def test_one_hot_through_conv_returns_flipped_taps():
    k = 5
    taps = (np.arange(k * k, dtype=np.float32).reshape(k, k) + 1) / 255.0
    img = np.zeros((21, 21, 3), np.uint8)
    img[10, 10] = 255
    out = PN.conv(img, taps)
    want = np.clip(np.rint((taps * np.float32(255))[::-1, ::-1]), 0, 255).astype(np.uint8)
    for c in range(3):
        assert np.array_equal(out[8:13, 8:13, c], want)
    assert out.sum() == 3 * int(want.sum())


def test_gray_full_alpha_and_huesat_wraps():
    img = _img(5)
    g = PN.gray(img, 1.0)
    assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 1], g[..., 2])
    # a full turn of the hue is (up to the uint8 HSV round trip, the same for both) no turn
    assert np.array_equal(PN.huesat(img, 180, 1), PN.huesat(img, 0, 1))
    assert np.array_equal(PN.huesat(img, -170, 0), PN.huesat(img, 10, 0))
    # saturation saturates: removing all of it leaves grey pixels of the value V = max
    d = PN.huesat(img, 0, -255)
    assert np.array_equal(d[..., 0], img.max(axis=-1)) and np.array_equal(d[..., 0], d[..., 2])


def test_lut_composition_equals_sequential_application():
    rng = np.random.default_rng(1)
    a, b, c = PH.lut_add([3, -7, 10]), PH.lut_gamma([0.8, 1.1, 1.2]), PH.lut_sigmoid(6.0, 0.4)
    ramp = np.tile(np.arange(256, dtype=np.uint8)[:, None, None], (1, 1, 3))
    seq = PN.lut(PN.lut(PN.lut(ramp, a), b), c)
    fused = PH.fuse_luts([PH.op_lut(a), PH.op_lut(b), PH.op_lut(c)])
    assert len(fused) == 1
    assert np.array_equal(PN.lut(ramp, fused[0]["table"]), seq)
    img = rng.integers(0, 256, size=(9, 9, 3), dtype=np.uint8)
    assert np.array_equal(PN.lut(img, fused[0]["table"]), PN.lut(PN.lut(PN.lut(img, a), b), c))


def test_lut_builders():
    assert PH.lut_add(10)[0, 250] == 255 and PH.lut_add(-10)[2, 5] == 0
    assert PH.lut_linear_contrast(1.3)[1, 127] == 127
    t = PH.lut_multiply([0.75, 1.0, 1.25])
    assert t[0, 100] == 75 and t[1, 100] == 100 and t[2, 100] == 125
    assert np.all(np.diff(PH.lut_log(0.9).astype(int), axis=1) >= 0) and np.all(np.diff(PH.lut_sigmoid(5.0, 0.5).astype(int), axis=1) >= 0)


def test_taps_builders():
    for s in (0.05, 0.5, 1.0, 1.6, 2.0):
        t = PH.gaussian_taps(s)
        assert t.shape[0] in (5, 7) and abs(float(t.sum()) - 1) < 1e-6 and np.array_equal(t, t.T)
    assert PH.gaussian_kernel_size(1.5) == 5 and PH.gaussian_kernel_size(2.0) == 7
    assert PH.average_taps(4).shape == (5, 5) and np.all(PH.average_taps(4)[4] == 0) and np.all(PH.average_taps(4)[:, 4] == 0)
    assert PH.motion_taps(4, 10.0, 0.0).shape == (5, 5)
    v = PH.motion_taps(5, 0.0, 0.0)
    assert np.allclose(v[:, 2], 0.2) and np.count_nonzero(v) == 5
    assert [PH.bilateral_size(d) for d in range(1, 8)] == [3, 3, 3, 5, 5, 7, 7]
    space, colour = PH.bilateral_tables(7, 30.0, 20.0)
    assert space[0, 0] == 0 and space[0, 3] > 0 and space[3, 3] == 1 and colour[0] == 1 and colour.shape == (766,)


# ---------------------------------------------------------------------------- the sampler
RANGES = dict(gaussian=dict(sigma=(1e-3, 2.0)), average=dict(k=(3, 7)), median=dict(k=(3, 7)), bilateral=dict(d=(1, 7)),
              motion=dict(k=(3, 7), angle=(0, 360), direction=(-1, 1)), huesat=dict(value=(-15, 15)), grayscale=dict(alpha=(0, 0.2)),
              add=dict(value=(-10, 10)), multiply=dict(mul=(0.75, 1.25)), linear=dict(alpha=(0.7, 1.3)),
              freqnoise=dict(exponent=(-4, 0), size=(4, 16), mul=(0.75, 1.25), alpha=(0.7, 1.3)), gamma=dict(gamma=(0.75, 1.25)),
              sigmoid=dict(gain=(0, 10), cutoff=(0.25, 0.75)), log=dict(gain=(0.75, 1.0)))


def test_sampler_reproducible_per_seed():
    def draw(seed):
        return PH.sample_programs(np.random.default_rng(seed), 8)
    a, b, c = draw(7), draw(7), draw(8)
    assert np.array_equal(a.op_offsets, b.op_offsets) and np.array_equal(a.ops, b.ops) and np.array_equal(a.pool, b.pool)
    assert not (np.array_equal(a.op_offsets, c.op_offsets) and np.array_equal(a.pool, c.pool))


def test_sampler_structure_and_ranges():
    rng = np.random.default_rng(2024)
    seen_names, seen_kinds, orders = set(), set(), set()
    for _ in range(3000):
        chain = PH.sample_chain(rng)
        groups = {}
        for op in chain:
            seen_names.add(op["name"])
            seen_kinds.add(op["kind"])
            groups.setdefault((op["slot"], op["group"]), []).append(op)
            for key, (lo, hi) in RANGES[op["name"]].items():
                val = np.asarray(op["params"][key], np.float64)
                assert np.all(val >= lo) and np.all(val <= hi), (op["name"], key, val)
                assert val.size in (1, 3)
        slots = [s for s, _ in groups]
        assert len(set(slots)) == len(slots)  # one group per place in the order
        orders.add(tuple(g for _, g in sorted(groups)))
        count = {g: 0 for g in ("blur", "colour", "brightness", "contrast")}
        for (_, g), ops in groups.items():
            count[g] = len(ops)
        assert count["blur"] in (0, 1, 2) and count["colour"] in (0, 1, 2) and count["contrast"] in (0, 1, 2)
        # OneOf: one brightness member (Add then Multiply is one member of two ops)
        names = [op["name"] for (_, g), ops in groups.items() if g == "brightness" for op in ops]
        assert names in (["add", "multiply"], ["add"], ["multiply"], ["freqnoise"])
        # the members of a SomeOf are distinct
        for (_, g), ops in groups.items():
            if g != "brightness":
                assert len({op["name"] for op in ops}) == len(ops)
    assert seen_names == set(RANGES)
    assert seen_kinds == set(PH.KINDS)
    assert len(orders) > 24  # the four groups come in random order


def test_compile_never_emits_adjacent_luts_and_packs_in_bounds():
    rng = np.random.default_rng(5)
    progs = PH.compile_chain([PH.sample_chain(rng) for _ in range(500)])
    assert progs.op_offsets[0] == 0 and progs.op_offsets[-1] == progs.ops.size and len(progs) == 500
    lut_k = PH.KINDS["lut"]
    for i in range(500):
        kinds = progs.ops["kind"][progs.op_offsets[i]:progs.op_offsets[i + 1]]
        assert not np.any((kinds[1:] == lut_k) & (kinds[:-1] == lut_k))
        assert [PH.KINDS[op["kind"]] for op in progs.chains[i]] == kinds.tolist()
    assert np.all(progs.ops["off0"] % 4 == 0) and np.all(progs.ops["off1"] % 4 == 0)
    assert np.all(progs.ops["off0"] < max(progs.pool.size, 1)) and progs.pool.size % 4 == 0
    nb = np.isin(progs.ops["kind"], [PH.KINDS["conv"], PH.KINDS["median"], PH.KINDS["bilateral"]])
    assert np.all(progs.ops["k"][nb] % 2 == 1) and np.all(progs.ops["k"][nb] <= 7)


def test_fused_chain_equals_unfused_chain():
    rng = np.random.default_rng(9)
    img = _img(9, 24, 31)
    for _ in range(20):
        chain = PH.sample_chain(rng)
        assert np.array_equal(PN.apply_chain(img, PH.fuse_luts(chain)), PN.apply_chain(img, chain))


@pytest.mark.parametrize("bad", [
    [dict(kind="sharpen")],
    [PH.op_conv(np.ones((4, 4), np.float32) / 16)],
    [PH.op_conv(np.ones((9, 9), np.float32) / 81)],
    [PH.op_conv(np.ones((3, 5), np.float32) / 15)],
    [PH.op_median(4)],
    [PH.op_median(9)],
    [PH.op_bilateral(np.ones((8, 8), np.float32), np.ones(766, np.float32))],
    [PH.op_bilateral(np.ones((3, 3), np.float32), np.ones(256, np.float32))],
    [PH.op_gray(1.5)],
    [PH.op_huesat(400, 0)],
    [PH.op_blend(PH.lut_identity(), PH.lut_identity(), np.zeros((33, 4), np.float32))],
    [dict(kind="lut", table=np.zeros((3, 128), np.uint8))],
    [PH.op_gray(0.1)] * 33,
])
def test_malformed_programs_raise_value_error(bad):
    with pytest.raises(ValueError):
        PH.compile_chain([bad])


def test_library_entry_point_signature_null_context_and_sizes():
    """the C ABI without a device: a NULL context is PP_ERR_NOCTX (-4), the workspace is one ping-pong batch, and the numpy record
    is the size of pp_photo_op.  (The host validation of malformed programs needs a context: tests/test_gpu_photo.py.)"""
    import ctypes as C
    from pyrapose_amd import _lib
    offs = np.array([0, 1], np.int32)
    rec = np.array([(5, 3, 0, 0, 0, 0)], PH.OP_DTYPE)
    assert _lib.lib.pp_photo_augment_u8(None, 1, 8, 8, 3, offs.ctypes.data, rec.ctypes.data, None, 0, None, None, None, None, 0) == -4
    assert _lib.lib.pp_photo_workspace_bytes(2, 10, 12) == 2 * 10 * 12 * 3
    assert _lib.lib.pp_photo_workspace_bytes(0, 10, 12) == 0
    assert C.sizeof(C.c_int) * 4 + C.sizeof(C.c_float) * 2 == PH.OP_DTYPE.itemsize


# ---------------------------------------------------------------------------- independent restatements of the shared formulas
def test_huesat_against_colorsys():
    """HUESAT against the standard library's colorsys (float64, its own sector table): convert, quantise H to [0,180) and S to
    [0,255] as the op defines, shift, convert back.  Away from quantisation ties the two can differ only by a flipped final
    rounding: <= 1 level.  At a tie -- (30 n / d) or (255 d / V) exactly half-way between integers, decided here in integer
    arithmetic -- colorsys' different expression may round H or S the other way: one unit of H moves a channel by at most
    V s / 30 <= 8.5 levels, one unit of S by at most 1 level, plus the final rounding: <= 10."""
    import colorsys
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(40, 50, 3), dtype=np.uint8)
    img[:5] = img[:5, :, :1]          # greys
    img[5:10, :, 1] = img[5:10, :, 0]  # two equal channels
    for dh, ds in ((7, -12), (-11, 15), (90, 0), (0, 40), (-179, -255), (3, 255)):
        got = PN.huesat(img, dh, ds).astype(int)
        want = np.empty_like(got)
        tie = np.zeros(img.shape[:2], bool)
        for y in range(img.shape[0]):
            for x in range(img.shape[1]):
                b, g, r = (int(v) for v in img[y, x])
                h, s_, v = colorsys.rgb_to_hsv(r / 255.0, g / 255.0, b / 255.0)
                Hq = int(np.rint(h * 180.0)) % 180
                Sq = int(np.rint(s_ * 255.0))
                H2, S2 = (Hq + dh) % 180, min(max(Sq + ds, 0), 255)
                ro, go, bo = colorsys.hsv_to_rgb(H2 / 180.0, S2 / 255.0, v)
                want[y, x] = [int(np.clip(np.rint(c * 255.0), 0, 255)) for c in (bo, go, ro)]
                V, m = max(b, g, r), min(b, g, r)
                d = V - m
                n = (g - b) if V == r else ((b - r) if V == g else (r - g))
                tie[y, x] = d > 0 and (((60 * n) % d == 0 and ((60 * n) // d) % 2 == 1) or ((510 * d) % V == 0 and ((510 * d) // V) % 2 == 1))
        diff = np.abs(got - want).max(axis=-1)
        assert diff[~tie].max() <= 1, (dh, ds, int(diff[~tie].max()))
        assert diff.max() <= 10, (dh, ds, int(diff.max()))
        assert tie.mean() < 0.2


def test_bilateral_against_naive_float64():
    """BILATERAL against a per-pixel double loop in float64 that skips the taps outside the circle: float32 accumulation of
    <= 49 weighted byte values cannot move a quotient by a level, only flip its rounding"""
    img = _img(21, 14, 17)
    for d, sc, ss in ((3, 25.0, 80.0), (5, 10.0, 250.0), (7, 120.0, 15.0)):
        space, colour = PH.bilateral_tables(d, sc, ss)
        k = space.shape[0]
        r = k // 2
        H, W = img.shape[:2]
        want = np.empty(img.shape, int)
        for y in range(H):
            for x in range(W):
                num, den = np.zeros(3), 0.0
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        if dy * dy + dx * dx > r * r:
                            continue
                        yy, xx = y + dy, x + dx
                        yy = -yy if yy < 0 else (2 * H - 2 - yy if yy >= H else yy)
                        xx = -xx if xx < 0 else (2 * W - 2 - xx if xx >= W else xx)
                        q = img[yy, xx].astype(np.float64)
                        w = np.exp(-(dy * dy + dx * dx) / (2.0 * ss * ss)) * np.exp(-(np.abs(q - img[y, x]).sum() ** 2) / (2.0 * sc * sc))
                        num += w * q
                        den += w
                want[y, x] = np.clip(np.rint(num / den), 0, 255)
        got = PN.bilateral(img, space, colour).astype(int)
        assert np.abs(got - want).max() <= 1, (d, int(np.abs(got - want).max()))
        assert np.mean(got != want) < 0.01


def test_blend_alpha_against_float64_interpolation():
    """the BLEND sample positions against numpy's own linear interpolation in float64 at the stated positions
    (x + 0.5) * mw / W - 0.5, clamped: float32 positions and weights differ from it by a few ulps of values in [0, 1]"""
    rng = np.random.default_rng(8)
    for (H, W), (mh, mw) in (((48, 64), (4, 16)), ((97, 131), (12, 12)), ((13, 21), (32, 5)), ((30, 30), (1, 1))):
        mask = rng.uniform(size=(mh, mw)).astype(np.float32)
        u = np.clip((np.arange(W) + 0.5) * mw / W - 0.5, 0, mw - 1)
        v = np.clip((np.arange(H) + 0.5) * mh / H - 0.5, 0, mh - 1)
        rows = np.stack([np.interp(u, np.arange(mw), mask[i].astype(np.float64)) for i in range(mh)])
        want = np.stack([np.interp(v, np.arange(mh), rows[:, j]) for j in range(W)], axis=1)
        got = PN.blend_alpha(H, W, mask)
        assert got.shape == (H, W) and got.dtype == np.float32
        assert np.abs(got - want).max() <= 2e-5
    # a one-cell mask of a: the blend is exactly a * first + (1 - a) * second
    img = _img(4)
    out = PN.blend(img, PH.lut_identity(), PH.lut_add(100), np.array([[1.0]], np.float32))
    assert np.array_equal(out, img)
