"""GPU: the depth-sensor simulation on the device (pp_depth_augment, ops.depth_augment, utils.depth_image) against its float64
numpy restatement tests/depth_aug_np.py -- bit for bit, dtype and shape included, for every output: the same IEEE operations
in the same order, integer work on the mask -- at the edges of the LDS tiles, at both rounding directions of the half size,
with gathers that leave their tile and clamp at all four borders; then every refused argument, and end to end from the depth
renderer into the normal images."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import depth_aug_np as A
from tests import depth_normals_np as DN

pytestmark = pytest.mark.gpu

ALL = A.OUTPUTS


def shapes():
    from pyrapose_amd import ops
    T = ops.DEPTH_AUG_TILE
    return [(8, 8), (9, 11), (T - 1, T + 1), (T, T), (T + 1, 2 * T + 1), (37, 53)]


# per shape the two images' programs: the kernel sizes cover 3, 5, 7 (and 1 everywhere once), methods 0, 1, 2, octaves 4 and 8
PROGRAMS = [
    (dict(k_open=3, k_med=5, k_blur=7, blur_sigma=1.2, method=0, octaves=4, seed=11), dict(k_open=1, k_med=1, k_blur=1, method=0, octaves=8, seed=12)),
    (dict(k_open=5, k_med=3, k_blur=3, blur_sigma=0.0, method=1, octaves=4, seed=21), dict(k_open=3, k_med=7, k_blur=5, blur_sigma=0.6, method=2, octaves=8, seed=22)),
    (dict(k_open=7, k_med=7, k_blur=7, blur_sigma=1.5, method=0, octaves=8, seed=31), dict(k_open=3, k_med=3, k_blur=3, blur_sigma=1.0, method=2, octaves=4, seed=32)),
    (dict(k_open=5, k_med=5, k_blur=5, blur_sigma=0.9, method=2, octaves=8, seed=41), dict(k_open=7, k_med=3, k_blur=1, method=1, octaves=4, seed=42)),
    (dict(k_open=3, k_med=7, k_blur=5, blur_sigma=0.3, method=0, octaves=8, seed=51, w_xy=4.0), dict(k_open=7, k_med=5, k_blur=3, blur_sigma=1.4, method=1, octaves=4, seed=52)),
    # 37 x 53: a w_xy = 100, a = depth / 1000 >= 0.6, so a w_xy >= 60 >= max(H, W): most gathers leave their tile, many clamp
    (dict(k_open=3, k_med=3, k_blur=7, blur_sigma=0.8, method=0, octaves=4, seed=61, w_xy=100.0, w_z=0.004),
     dict(k_open=5, k_med=7, k_blur=3, blur_sigma=1.1, method=2, octaves=8, seed=62, w_xy=100.0, freq=0.2)),
]


def scene(rng, n, H, W):
    """a tilted plane of whole-millimetre depths on a background at 0; the foreground mask is a blob touching the top and the
    left border, with a one-pixel hole the median must fill, plus a one-pixel speck the opening must remove"""
    y, x = np.mgrid[0:H, 0:W]
    depth, mask = [], []
    for i in range(n):
        m = (y < (3 * H) // 4) & (x < (4 * W) // 5 - i)
        m[H // 3, W // 3] = False      # the hole
        m[H - 2, W - 2] = True         # the speck
        d = np.rint(600.0 + 50.0 * i + 7.0 * x + 11.0 * y + rng.integers(-2, 3, size=(H, W)))
        depth.append(np.where(m, d, 0.0))
        mask.append(m)
    return np.stack(depth).astype(np.float32), np.stack(mask).astype(np.uint8) * np.uint8(3)


def device(depth, mask, rows, z, want=ALL):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    out = ops.depth_augment(default_context(), torch.from_numpy(depth).cuda(), torch.from_numpy(mask).cuda(), rows,
                            None if z is None else torch.from_numpy(z).cuda(), want)
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_same(got, want, what):
    """every requested output: dtype, shape and bits (the float ones compared as integers, so that -0.0 is not 0.0)"""
    views = {np.dtype(np.float64): np.int64, np.dtype(np.float32): np.int32}
    for k, g in got.items():
        w = want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.dtype, w.shape)
        gi, wi = (g.view(views[g.dtype]), w.view(views[g.dtype])) if g.dtype in views else (g, w)
        bad = gi != wi
        print("%s %s: %d of %d values differ" % (what, k, int(bad.sum()), bad.size))
        assert not bad.any(), (what, k, np.argwhere(bad)[:4].tolist(), g[bad][:4], w[bad][:4])


@pytest.fixture(scope="module")
def problems():
    """per shape one batch of 2 with its programs, its normals and its restatement, computed once and shared"""
    rng = np.random.default_rng(23)
    out = {}
    for hw, progs in zip(shapes(), PROGRAMS):
        depth, mask = scene(rng, 2, *hw)
        rows = np.stack([A.make_program(**p) for p in progs])
        z = rng.standard_normal((2, A.half_size(hw[0]), A.half_size(hw[1]))).astype(np.float32)
        out[hw] = (depth, mask, rows, z, A.depth_augment_batch(depth, mask, rows, z))
    return out


def test_the_cases_cover_what_they_claim(problems):
    rows = np.concatenate([p[2] for p in problems.values()])
    for c in (A.P_K_OPEN, A.P_K_MED, A.P_K_BLUR):
        assert {1.0, 3.0, 5.0, 7.0} == set(rows[:, c])
    assert (rows[:, :3] == 1).all(axis=1).any()
    assert {(1.0, 1.0), (1.0, 0.0), (0.0, 1.0)} == {(r[A.P_SENSOR], r[A.P_SIMPLEX]) for r in rows}
    assert {4.0, 8.0} == set(rows[:, A.P_OCTAVES])
    for hw, (depth, mask, rows, z, want) in problems.items():
        H, W = hw
        m = want["mask_u8"]
        assert mask[:, H - 2, W - 2].all() and not mask[:, H // 3, W // 3].any() and mask[:, 0, 0].all(), hw
        for i in range(2):
            if rows[i, A.P_K_OPEN] > 1:
                assert m[i, H - 2, W - 2] == 0, hw      # the opening removes the speck
            if rows[i, A.P_K_MED] > 1:
                assert m[i, H // 3, W // 3] == 255, hw  # the median fills the hole
            assert m[i].any() and (m[i] == 0).any(), hw
            if min(H, W) > 11:  # (a 7 x 7 majority window leaves a blob of 6 x 8 pixels no border)
                assert m[i, 0].any() and m[i, :, 0].any(), hw  # the blob still touches two borders
        assert np.array_equal(depth, np.rint(depth)) and (depth[mask == 0] == 0).all()
    # the large-warp case: a w_xy >= max(H, W) on the foreground, gathers far from home and clamped at all four borders
    depth, mask, rows, z, want = problems[(37, 53)]
    H, W = 37, 53
    for i in range(2):
        D = want["sensor_f64"][i]
        fg = (want["mask_u8"][i] != 0) & (depth[i] > 0)  # (the filled hole has no depth)
        assert (depth[i][fg] * 0.001 * rows[i, A.P_W_XY]).min() >= max(H, W)
        V0, V1, _ = A.noise_fields(H, W, rows[i])
        y, x = np.mgrid[0:H, 0:W]
        fx, fy = x + (D * 0.001 * rows[i, A.P_W_XY]) * V0, y + (D * 0.001 * rows[i, A.P_W_XY]) * V1
        T = 8  # launch C's smallest tile edge
        assert ((np.abs(fx - x) > T) | (np.abs(fy - y) > T))[fg].mean() > 0.5
        assert (fx < 0).sum() > 20 and (fx > W - 1).sum() > 20 and (fy < 0).sum() > 20 and (fy > H - 1).sum() > 20


@pytest.mark.parametrize("hw", shapes())
def test_all_outputs_match_restatement(problems, hw):
    depth, mask, rows, z, want = problems[hw]
    got = device(depth, mask, rows, z)
    assert list(got) == list(ALL)
    assert_same(got, want, "%dx%d" % hw)
    assert_same(device(depth, mask, rows, z), got, "%dx%d again" % hw)  # a repeated call gives the same bits


def test_each_output_alone(problems):
    """every null-pointer path of the entry point, on the shape with partial tiles on both axes"""
    from pyrapose_amd import ops
    T = ops.DEPTH_AUG_TILE
    depth, mask, rows, z, want = problems[(T + 1, 2 * T + 1)]
    for k in ALL:
        got = device(depth, mask, rows, z, (k,))
        assert list(got) == [k]
        assert_same(got, want, "alone")


def test_simplex_only_batch_needs_no_z(problems):
    depth, mask, rows, z, _ = problems[(37, 53)]
    rows = rows.copy()
    rows[:, A.P_SENSOR] = 0
    assert_same(device(depth, mask, rows, None), A.depth_augment_batch(depth, mask, rows, None), "no z")


def test_bad_arguments_return_the_error_code():
    from pyrapose_amd import ops
    from pyrapose_amd._lib import lib
    from pyrapose_amd.runtime import default_context
    ctx = default_context()
    good = A.make_program()
    depth = torch.ones((1, 8, 8), dtype=torch.float32, device="cuda")
    mask = torch.ones((1, 8, 8), dtype=torch.uint8, device="cuda")
    z = torch.zeros((1, 4, 4), dtype=torch.float32, device="cuda")
    out = torch.empty((1, 8, 8), dtype=torch.float32, device="cuda")
    ws = torch.empty((1 << 16,), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    need = lib.pp_depth_augment_workspace_bytes(1, 8, 8)
    assert 0 < need <= ws.numel()

    def call(n=1, H=8, W=8, row=good, z_p=p(z), ws_bytes=ws.numel(), out_p=p(out), host=True, depth_p=p(depth)):
        host_rows = np.ascontiguousarray(row, np.float64).reshape(1, -1)
        dev = torch.from_numpy(host_rows).cuda()
        hp = host_rows.ctypes.data_as(C.POINTER(C.c_double)) if host else None
        return lib.pp_depth_augment(ctx.handle, n, H, W, depth_p, p(mask), p(dev), hp, z_p, p(ws), ws_bytes, out_p, None, None, None, None)

    def changed(slot, value):
        row = good.copy()
        row[slot] = value
        return row

    assert call() == 0
    for n, H, W in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 7, 8), (1, 8, 7), (1, 0, 8), (1, 16385, 8), (1, 8, 16385)):
        assert call(n, H, W) == -2, (n, H, W)  # PP_ERR_SHAPE
        assert lib.pp_depth_augment_workspace_bytes(n, H, W) == 0
    for slot in (A.P_K_OPEN, A.P_K_MED, A.P_K_BLUR):
        for k in (0, 2, 4, 9, -3, 3.5):
            assert call(row=changed(slot, k)) == -1, (slot, k)
    for o in (0, 9, 2.5, -1):
        assert call(row=changed(A.P_OCTAVES, o)) == -1, o
    for slot in (A.P_SENSOR, A.P_SIMPLEX):
        assert call(row=changed(slot, 2)) == -1 and call(row=changed(slot, 0.5)) == -1
    for seed in (-1, 2.0 ** 53, 0.5):
        assert call(row=changed(A.P_SEED, seed)) == -1, seed
    assert call(row=changed(A.P_W_Z, np.nan)) == -1 and call(row=changed(A.P_GAIN, np.inf)) == -1
    assert call(row=changed(A.P_FREQ, 17.0)) == -1 and call(row=changed(A.P_LACUNARITY, 0.0)) == -1
    assert call(z_p=None) == -1                                  # sensor = 1 without z
    assert call(z_p=None, row=A.make_program(method=2)) == 0     # simplex only needs none
    assert call(ws_bytes=need - 1) == -1
    assert call(ws_bytes=need) == 0
    assert call(out_p=None) == -1                                # no output
    assert call(host=False) == -1 and call(depth_p=None) == -1
    torch.cuda.synchronize()
    # and through the wrapper: ValueError
    with pytest.raises(ValueError):
        ops.depth_augment(ctx, depth, mask, changed(A.P_K_MED, 4)[None], z)
    with pytest.raises(ValueError):
        ops.depth_augment(ctx, depth, mask, good[None], None)
    with pytest.raises(ValueError):
        ops.depth_augment(ctx, depth, mask, good[None], z, ())
    with pytest.raises(ValueError):
        ops.depth_augment(ctx, depth.double(), mask, good[None], z)
    with pytest.raises(ValueError):
        ops.depth_augment(ctx, depth, mask, good[None, :-1], z)
    with pytest.raises(ValueError):
        ops.depth_augment(ctx, depth[:, :7], mask[:, :7], good[None], z)


def test_rendered_depth_end_to_end():
    """render_depth_batch -> augment_depth_batch -> normals_from_depth_batch(for_vis=False), all on device tensors"""
    from pyrapose_amd.utils.depth_image import augment_depth_batch, normals_from_depth_batch, sample_depth_programs
    from pyrapose_amd.utils.renderer import render_depth_batch
    pts = np.array([[-60, -40, 0], [60, -40, 10], [60, 40, 30], [-60, 40, -20], [0, 0, -50]], np.float64)
    faces = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [0, 2, 1], [0, 3, 2]])
    K = np.array([[120.0, 0, 26.2611], [0, 121.0, 18.049], [0, 0, 1]])
    R = np.stack([np.eye(3), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])])
    t = np.array([[0.0, 0, 400], [5.0, -3, 500]])
    depth = render_depth_batch({"pts": pts, "faces": faces}, (53, 37), K, R, t)
    host = depth.cpu().numpy()
    assert (host > 0).any() and (host == 0).any()
    programs = sample_depth_programs(np.random.default_rng(8), 2)
    z = np.random.default_rng(9).standard_normal((2, 18, 26)).astype(np.float32)
    noisy = augment_depth_batch(depth, None, programs, z=z)
    assert noisy.is_cuda and noisy.dtype == torch.float32 and tuple(noisy.shape) == (2, 37, 53)
    want = A.depth_augment_batch(host, (host > 0).astype(np.uint8), programs, z)
    assert_same({"depth_f32": noisy.cpu().numpy()}, want, "rendered")
    assert not np.array_equal(want["depth_f32"], host)
    n, d = normals_from_depth_batch(noisy, K, for_vis=False)
    intr = np.tile([K[0, 0], K[0, 2], K[1, 2]], (2, 1))
    ref = DN.depth_normals_batch(want["depth_f32"], intr, for_vis=False)
    assert_same({"normals_u8": n.cpu().numpy(), "depth": d.cpu().numpy()}, ref, "rendered normals")
    # z drawn on the device: reproducible from a generator, and something else than the supplied field
    g = torch.Generator(device="cuda")
    a = augment_depth_batch(depth, None, programs, generator=g.manual_seed(5))
    b = augment_depth_batch(depth, None, programs, generator=g.manual_seed(5))
    assert torch.equal(a, b) and not torch.equal(a, noisy)


def test_augmentDepth_nine_arguments_equals_the_batch_call():
    from pyrapose_amd.utils.depth_image import augment_depth_batch, augmentDepth, sample_depth_programs
    rng = np.random.default_rng(3)
    depth, mask = scene(rng, 1, 37, 53)
    depth, mask = depth[0].astype(np.float64), mask[0]
    for method in (0, 1, 2):
        got = augmentDepth(depth, None, mask, 5, 3, 7, 1.1, 0.003, method, rng=np.random.default_rng(40 + method))
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (37, 53)
        r = np.random.default_rng(40 + method)  # the same draws, by hand
        programs = sample_depth_programs(r, 1, method, 5, 3, 7, 1.1, 0.003)
        z = r.standard_normal((1, 18, 26), dtype=np.float32)
        assert (programs[0, :3] == [5, 3, 7]).all()
        batch = augment_depth_batch(depth[None], mask[None], programs, z=z)
        assert np.array_equal(got, batch[0].cpu().numpy().astype(np.float64))
        assert_same({"depth_f32": batch.cpu().numpy()}, A.depth_augment_batch(depth[None], mask[None], programs, z), "drop-in %d" % method)
    three = augmentDepth(depth, None, mask, rng=np.random.default_rng(1))  # the three-argument signature draws everything
    assert three.shape == (37, 53) and three.dtype == np.float64 and (three >= 0).all() and three.any()
