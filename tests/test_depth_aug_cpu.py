"""The numpy restatement of the depth-sensor simulation (tests/depth_aug_np.py) against what pins it -- scipy's median filter
and grey morphology, the documented rules of the OpenCV calls it restates, its own invariants -- the host side of
ops / utils.depth_image, and the C ABI of the two entry points.  No device is needed.  OpenCV is not a dependency: parity
with cv2 itself is restated, not pinned."""
import os
import re

import numpy as np
import pytest

from pyrapose_amd import ops
from pyrapose_amd.utils import depth_image
from tests import depth_aug_np as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pp_depth_augment_workspace_bytes", "pp_depth_augment")
SHAPES = ((8, 8), (9, 11), (16, 13), (37, 53))


def scene(rng, H, W):
    """whole-millimetre tilted plane on a background at 0 and the foreground mask it comes from"""
    y, x = np.mgrid[0:H, 0:W]
    mask = rng.random((H, W)) < 0.7
    depth = np.where(mask, np.rint(600.0 + 7.0 * x + 11.0 * y), 0.0).astype(np.float32)
    return depth, mask.astype(np.uint8)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_majority_is_scipys_median(k):
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(k)
    for shape in SHAPES:
        for p in (0.3, 0.5, 0.7):
            m = (rng.random(shape) < p).astype(np.uint8)
            want = signal.medfilt2d((m * 255).astype(np.float64), kernel_size=k)
            assert np.array_equal(A.majority(m, k) * 255.0, want), (shape, p)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_opening_is_scipys_grey_morphology(k):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(10 + k)
    for shape in SHAPES:
        for p in (0.5, 0.8, 0.95):
            m = (rng.random(shape) < p).astype(np.uint8)
            eroded = ndimage.grey_erosion(m * np.uint8(255), size=(k, k), mode="constant", cval=255)
            want = ndimage.grey_dilation(eroded, size=(k, k), mode="constant", cval=0)
            got = A.opening(m, k) * np.uint8(255)
            assert got.dtype == want.dtype == np.uint8 and np.array_equal(got, want), (shape, p)
    assert np.array_equal(A.opening(m, 1), m) and np.array_equal(A.majority(m, 1), m)


def test_blur_taps():
    for k in (1, 3, 5, 7):
        for sigma in (0.0, -1.0, 0.2, 0.75, 1.5):
            w = ops.depth_aug_blur_taps(k, sigma)
            assert w.dtype == np.float64 and w.shape == (k,) and np.array_equal(w, A.blur_taps(k, sigma))
            assert abs(w.sum() - 1.0) <= 2 * np.finfo(np.float64).eps
            assert np.array_equal(w, w[::-1]) and (w >= 0).all() and w[k // 2] == w.max()
        s = 0.3 * ((k - 1) * 0.5 - 1) + 0.8  # cv2's rule for sigma <= 0
        assert np.array_equal(ops.depth_aug_blur_taps(k, 0.0), ops.depth_aug_blur_taps(k, s))
        assert np.array_equal(ops.depth_aug_blur_taps(k, -3.0), ops.depth_aug_blur_taps(k, s))
    assert ops.depth_aug_blur_taps(1, 0.7).tolist() == [1.0]
    x = np.arange(-2, 3, dtype=np.float64)
    w = np.exp(-x * x / (2 * 1.1 * 1.1))
    np.testing.assert_allclose(ops.depth_aug_blur_taps(5, 1.1), w / w.sum(), rtol=1e-15)
    for bad in (0, 2, 9):
        with pytest.raises(ValueError):
            ops.depth_aug_blur_taps(bad, 1.0)


def test_half_sizes_round_half_to_even_and_stay_inside():
    assert [A.half_size(w) for w in (8, 9, 10, 11)] == [4, 4, 5, 6]
    assert [ops.depth_aug_half_size(w) for w in (8, 9, 10, 11)] == [4, 4, 5, 6]
    for n in range(8, 200):
        h = A.half_size(n)
        assert h == ops.depth_aug_half_size(n) and 2 * (h - 1) <= n - 1 and min(2 * (h - 1) + 1, n - 1) <= n - 1
        s0, s1, frac = A._upsample_axis(n, h)  # and the way back up
        assert s0.min() >= 0 and s1.max() <= h - 1 and (frac >= 0).all() and (frac < 1).all()
    d = np.arange(9 * 11, dtype=np.float64).reshape(9, 11)
    got = A.halve(d)  # (asserts its own indices)
    assert got.shape == (4, 6) and got[0, 0] == (0 + 1 + 11 + 12) / 4.0
    assert got[3, 5] == (d[6, 10] + d[7, 10]) / 2.0  # the clamped last column: 2 * 5 + 1 = 11 -> 10


def test_reflect_101():
    assert A.reflect_101(np.arange(-3, 8), 5).tolist() == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    assert A.reflect_101(np.arange(-4, 6), 2).tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]  # shorter than the reach: again and again
    assert A.reflect_101(np.arange(-2, 3), 1).tolist() == [0, 0, 0, 0, 0]
    flat = np.full((6, 7), 812.0)
    assert np.array_equal(A.blur(flat, np.array([0.25, 0.5, 0.25])), flat)


def test_quantised_depth_is_a_multiple_of_its_resolution():
    rng = np.random.default_rng(2)
    depth, mask = scene(rng, 37, 53)
    d2 = A.halve(np.where(A.shadow_mask(mask, 3, 3) != 0, depth.astype(np.float64), 0.0))
    for k in (1, 3, 7):
        row = A.make_program(k_blur=k, blur_sigma=0.9, depth_noise=0.0)
        s, res = A.sensor(d2, row, rng.standard_normal(d2.shape).astype(np.float32))
        live = s != 0
        assert live.any() and (res[live] != 0).all() and not s[res == 0].any()
        ratio = s[live] / res[live]
        assert np.array_equal(np.rint(ratio) * res[live], s[live])


@pytest.mark.parametrize("octaves", [4, 8])
def test_simplex_noise(octaves):
    row = A.make_program(freq=0.2, octaves=octaves, seed=77)
    V = A.noise_fields(64, 64, row)
    again = A.noise_fields(64, 64, row.copy())
    other = A.noise_fields(64, 64, A.make_program(freq=0.2, octaves=octaves, seed=78))
    for v, a, o in zip(V, again, other):
        assert v.dtype == np.float64 and np.array_equal(v.view(np.int64), a.view(np.int64))
        assert not np.array_equal(v, o)
        print("octaves %d: max |V| = %.4f" % (octaves, np.abs(v).max()))
        assert np.abs(v).max() <= 1.0 and np.abs(v).max() > 0.2 and abs(v.mean()) < 0.1
    assert not np.array_equal(V[0], V[1])  # the fields differ through their jitter


def test_simplex_pieces():
    from oracle import pnp_np
    for v in (0, 1, 2 ** 63 + 12345, 2 ** 64 - 1):
        assert int(A.splitmix64(np.array([v], np.uint64))[0]) == pnp_np.splitmix64(v)
    u = A.jitter_u(5, 1, np.arange(4096, dtype=np.uint64))
    assert (u >= 0).all() and (u < 1).all() and 0.45 < u.mean() < 0.55 and len(np.unique(u)) == 4096
    gi = A.grad_index(np.arange(-600, 600), np.arange(1200) * 7 - 50, np.arange(1200) % 13, 9)
    assert gi.min() == 0 and gi.max() == 11 and np.bincount(gi).min() > 50
    assert np.array_equal(np.abs(A.GRAD).sum(axis=1), np.full(12, 2.0)) and len({tuple(g) for g in A.GRAD}) == 12
    assert A.simplex3(np.zeros(1), np.zeros(1), np.zeros(1), 3)[0] == 0.0  # a lattice point: every g . d term vanishes or is cut
    rng = np.random.default_rng(0)
    p = rng.uniform(-40, 40, size=(3, 200000))
    n = A.simplex3(p[0], p[1], p[2], 11)
    assert np.abs(n).max() <= 1.0 and np.abs(n).max() > 0.8
    # continuity: a step of 1e-6 moves the value by about 1e-5 at most (no corner picked out of order)
    n2 = A.simplex3(p[0] + 1e-6, p[1], p[2], 11)
    assert np.abs(n2 - n).max() < 1e-4


def test_method_1_leaves_the_warp_an_identity_and_method_2_never_reads_z():
    rng = np.random.default_rng(4)
    depth, mask = scene(rng, 16, 13)
    z = rng.standard_normal((8, 6)).astype(np.float32)
    out = A.depth_augment(depth, mask, A.make_program(method=1), z)
    assert np.array_equal(out["depth_f64"].view(np.int64), out["sensor_f64"].view(np.int64))
    assert np.array_equal(out["sensor_f64"], A.upsample(out["half_f64"], 16, 13)) and out["half_f64"].any()
    assert np.array_equal(out["depth_f32"], out["depth_f64"].astype(np.float32))

    class Untouchable:
        def __array__(self, *a, **k):
            raise AssertionError("z was read")

        def __getitem__(self, i):
            raise AssertionError("z was read")

    with pytest.raises(AssertionError):
        A.depth_augment(depth, mask, A.make_program(method=0), Untouchable())
    two = A.depth_augment(depth, mask, A.make_program(method=2), Untouchable())
    assert np.array_equal(two["depth_f64"], A.depth_augment(depth, mask, A.make_program(method=2), None)["depth_f64"])
    assert not two["half_f64"].any()
    d1 = np.where(two["mask_u8"] != 0, depth.astype(np.float64), 0.0)
    assert np.array_equal(two["sensor_f64"], d1) and not np.array_equal(two["depth_f64"], d1)
    assert (two["depth_f64"] >= 0).all() and set(np.unique(two["mask_u8"])) <= {0, 255}


@pytest.mark.parametrize("method", [0, 1, 2])
def test_sampler_draws_the_references_ranges(method):
    P = depth_image.sample_depth_programs(np.random.default_rng(method), 400, method)
    assert P.dtype == np.float64 and P.shape == (400, ops.DEPTH_AUG_P) and ops.DEPTH_AUG_P == A.P
    assert np.array_equal(P, A.sample_programs(np.random.default_rng(method), 400, method))  # the restatement's sampler, draw for draw
    col = lambda name: P[:, ops.DEPTH_AUG_PARAMS[name][0]:sum(ops.DEPTH_AUG_PARAMS[name])]
    for k in ("k_open", "k_med", "k_blur"):
        assert set(col(k).ravel()) == {3.0, 5.0, 7.0}
    for row in P:
        k = int(row[A.P_K_BLUR])
        taps = row[A.P_TAPS:A.P_TAPS + 7]
        assert abs(taps[:k].sum() - 1.0) < 1e-15 and not taps[k:].any()
    assert (col("depth_noise") >= 0.002).all() and (col("depth_noise") <= 0.004).all()
    assert (col("freq") >= 0.05).all() and (col("freq") <= 0.2).all()
    assert set(col("octaves").ravel()) == {4.0, 8.0}
    assert (col("lacunarity") == 2.1).all() and (col("gain") == 0.45).all()
    assert set(col("w_xy").ravel()) == ({2.0, 3.0, 4.0} if method == 2 else {1.0, 2.0, 3.0, 4.0})
    assert (col("w_z") >= 1e-4).all() and (col("w_z") <= 4e-3).all()
    assert (col("jitter_lo") == [0.001, 0.001, 0.01]).all() and (col("jitter_hi") == [0.01, 0.01, 0.1]).all()
    seed = col("seed").ravel()
    assert (seed == np.floor(seed)).all() and (seed >= 0).all() and (seed < 2 ** 31).all() and len(set(seed)) > 390
    flags = {(float(s), float(x)) for s, x in zip(col("sensor").ravel(), col("simplex").ravel())}
    assert flags == {{0: (1.0, 1.0), 1: (1.0, 0.0), 2: (0.0, 1.0)}[method]}
    # the five arguments of the augment_syn_* signature replace their draws and leave the others alone
    Q = depth_image.sample_depth_programs(np.random.default_rng(method), 400, method, 5, 7, 3, 0.0, 0.0035)
    assert (Q[:, :3] == [5, 7, 3]).all() and (Q[:, A.P_DEPTH_NOISE] == 0.0035).all()
    assert np.array_equal(Q[:, A.P_TAPS:A.P_TAPS + 3], np.tile(ops.depth_aug_blur_taps(3, 0.0), (400, 1)))
    assert np.array_equal(Q[:, A.P_SENSOR:], P[:, A.P_SENSOR:])
    with pytest.raises(ValueError):
        depth_image.sample_depth_programs(np.random.default_rng(0), 1, 3)


def test_layout_constants_agree():
    src = open(os.path.join(ROOT, "include", "pyrapose_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define PP_DA_([A-Z_]+) (\d+)", src)}
    assert consts.pop("P") == ops.DEPTH_AUG_P == A.P
    assert consts == {k.upper().replace("BLUR_TAPS", "TAPS"): v[0] for k, v in ops.DEPTH_AUG_PARAMS.items()}
    mine = {k[2:]: v for k, v in vars(A).items() if k.startswith("P_")}
    assert mine == consts
    slots = sorted(i for first, n in ops.DEPTH_AUG_PARAMS.values() for i in range(first, first + n))
    assert slots == list(range(ops.DEPTH_AUG_P))
    assert tuple(ops.DEPTH_AUG_OUTPUTS) == A.OUTPUTS and ops.DEPTH_AUG_TILE == 32


def test_argument_errors_need_no_device():
    m = depth_image
    P = m.sample_depth_programs(np.random.default_rng(0), 1)
    for bad in (np.zeros((8, 8)), np.zeros((1, 7, 8)), np.zeros((1, 8, 7)), np.zeros((0, 8, 8))):
        with pytest.raises(ValueError):
            m.augment_depth_batch(bad, None, P)
    with pytest.raises(ValueError):
        m.augmentDepth(np.zeros((2, 8, 8)), None, np.zeros((8, 8)))
    with pytest.raises(ValueError):
        m.augmentDepth(np.zeros((8, 8)), None, np.zeros((8, 8)), 3, 3, 3, 1.0, 0.003, 5)


def test_entry_points_declared_and_exported():
    from pyrapose_amd import _lib
    src = open(os.path.join(ROOT, "include", "pyrapose_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.EXPORTS and hasattr(_lib.lib, name)
    argtypes = _lib.lib.pp_depth_augment.argtypes
    decl = re.search(r"int pp_depth_augment\((.*?)\);", code, flags=re.S).group(1)
    assert len(argtypes) == len(decl.split(",")) == 16
    # host-side refusals need no device: a NULL context first, as everywhere; a refused shape has no workspace
    assert _lib.lib.pp_depth_augment(None, 1, 8, 8, None, None, None, None, None, None, 0, None, None, None, None, None) == -4
    for n, H, W in ((0, 8, 8), (65536, 8, 8), (1, 7, 8), (1, 8, 7), (1, 16385, 8), (1, 8, 16385)):
        assert _lib.lib.pp_depth_augment_workspace_bytes(n, H, W) == 0
    h2, w2 = ops.depth_aug_half_size(37), ops.depth_aug_half_size(53)
    a256 = lambda v: (v + 255) // 256 * 256
    assert _lib.lib.pp_depth_augment_workspace_bytes(2, 37, 53) == a256(2 * 37 * 53 * 4) + 2 * a256(2 * h2 * w2 * 8)
