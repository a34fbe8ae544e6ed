"""GPU: the depth normal images on the device (pp_depth_normals_f64, ops.depth_normals, utils.depth_image) against their
float64 numpy restatement tests/depth_normals_np.py -- bit for bit, dtype and shape included, for every output in both modes:
the same IEEE operations in the same order, the two maxima exact -- at the edges of the smoothing tile and below the filter
radius; then against the reference's own get_normal through tests/golden/depth_normals.npz, within the bounds of
tests/test_depth_normals_cpu.py; then end to end from the depth renderer."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import depth_normals_np as DN
from tests.test_depth_normals_cpu import CASES, GOLDEN, check_against_golden

pytestmark = pytest.mark.gpu

ALL = {True: ("normals", "signed", "depth"), False: ("normals", "signed", "depth", "normals_u8")}


def shapes():
    from pyrapose_amd import ops
    T = ops.DEPTH_NORMALS_TILE
    return [(3, 3), (5, 7), (8, 9), (T - 1, T + 1), (T, T), (T + 1, 2 * T + 1), (37, 53)]


def device(depth, intr, for_vis, want):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    out = ops.depth_normals(default_context(), torch.from_numpy(np.ascontiguousarray(depth, np.float32)).cuda(),
                            torch.from_numpy(np.ascontiguousarray(intr, np.float64)).cuda(), for_vis, want)
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_same(got, want, what):
    """every requested output: dtype, shape and bits (the float64 ones compared as integers, so that -0.0 is not 0.0)"""
    for k, g in got.items():
        w = want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.dtype, w.shape)
        gi, wi = (g.view(np.int64), w.view(np.int64)) if g.dtype == np.float64 else (g, w)
        bad = gi != wi
        print("%s %s: %d of %d values differ" % (what, k, int(bad.sum()), bad.size))
        assert not bad.any(), (what, k, np.argwhere(bad)[:4].tolist(), g[bad][:4], w[bad][:4])


def synthetic(rng, n, H, W):
    """whole-number depths: a tilted plane with noise, a far block, one small zero hole; intrinsics off the integer grid"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = np.stack([np.rint(600.0 + 100.0 * i + 7.0 * x + 11.0 * y + rng.integers(-4, 5, size=(H, W))) for i in range(n)])
    depth[:, : max(1, H // 3), : max(1, W // 4)] += 1900.0
    depth[:, H // 2, W // 2] = 0.0
    intr = np.stack([[500.0 + 40.0 * i, 0.45 * W + 0.2611 + i, 0.55 * H + 0.049 - i] for i in range(n)])
    return depth.astype(np.float32), intr


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def problems():
    """per shape one batch of 2 and its restatement in both modes, computed once and shared"""
    rng = np.random.default_rng(17)
    out = {}
    for hw in shapes():
        depth, intr = synthetic(rng, 2, *hw)
        out[hw] = (depth, intr, {v: DN.depth_normals_batch(depth, intr, for_vis=v) for v in (True, False)})
    return out


@pytest.mark.parametrize("for_vis", [True, False])
@pytest.mark.parametrize("hw", shapes())
def test_all_outputs_match_restatement(problems, hw, for_vis):
    depth, intr, want = problems[hw]
    assert_same(device(depth, intr, for_vis, ALL[for_vis]), want[for_vis], "%dx%d vis=%d" % (hw + (int(for_vis),)))


@pytest.mark.parametrize("for_vis", [True, False])
def test_each_output_alone(problems, for_vis):
    """every null-pointer path of the entry point, on the shape with partial tiles on both axes"""
    from pyrapose_amd import ops
    T = ops.DEPTH_NORMALS_TILE
    depth, intr, want = problems[(T + 1, 2 * T + 1)]
    for k in ALL[for_vis]:
        got = device(depth, intr, for_vis, (k,))
        assert list(got) == [k]
        assert_same(got, want[for_vis], "alone vis=%d" % int(for_vis))


@pytest.mark.parametrize("name,for_vis", [(n, v) for n, modes in CASES.items() for v in modes])
def test_fixture_cases_match_restatement(golden, name, for_vis):
    """the four fixture cases, the ill-posed pixels of case C included: the same operations give the same noise"""
    fx, _fy, cx, cy = golden[name + "_intr"]
    depth = golden[name + "_depth"]
    want = DN.depth_normals_batch(depth[None], [[fx, cx, cy]], for_vis=for_vis)
    assert_same(device(depth[None], [[fx, cx, cy]], for_vis, ALL[for_vis]), want, "case %s vis=%d" % (name, int(for_vis)))
    if not for_vis:  # (cases C and D are pinned in one mode only; the device must still agree with the restatement in the other)
        return
    want = DN.depth_normals_batch(depth[None], [[fx, cx, cy]], for_vis=False)
    assert_same(device(depth[None], [[fx, cx, cy]], False, ALL[False]), want, "case %s vis=0" % name)


@pytest.mark.parametrize("name,for_vis", [(n, v) for n, modes in CASES.items() for v in modes])
def test_get_normal_matches_reference(golden, name, for_vis):
    """the device through the drop-in, against the reference's own return values: the bounds of the CPU test"""
    from pyrapose_amd.utils.depth_image import get_normal
    fx, fy, cx, cy = golden[name + "_intr"]
    n, d = get_normal(golden[name + "_depth"], fx=fx, fy=fy, cx=cx, cy=cy, for_vis=for_vis)
    assert isinstance(n, np.ndarray) and isinstance(d, np.ndarray)
    check_against_golden(golden, name, for_vis, n, d)


def test_maximum_in_the_last_pixel_of_the_last_tile():
    """(T+1) x (2T+1): the last tile is one pixel.  Image 0: a spike there, so the largest smoothed depth sits in it.  Image 1:
    everything beyond the far cut but a pit there, so the largest scaled normal component sits in the last, one-pixel-high row
    of tiles.  A tail read as zero, or a missed partial maximum, changes every uint8 value"""
    from pyrapose_amd import ops
    T = ops.DEPTH_NORMALS_TILE
    H, W = T + 1, 2 * T + 1
    depth = np.stack([np.full((H, W), 300.0, np.float32), np.full((H, W), 2100.0, np.float32)])
    depth[0, H - 1, W - 1] = 9000.0
    depth[1, H - 1, W - 1] = 0.0
    intr = np.tile([520.0, 0.5 * W + 0.2611, 0.5 * H + 0.049], (2, 1))
    want = DN.depth_normals_batch(depth, intr, for_vis=False)
    d0, d1 = DN.smooth(depth[0]), DN.smooth(depth[1])
    assert np.unravel_index(np.argmax(d0), d0.shape) == (H - 1, W - 1) and d0.max() <= 2000
    m = DN.depth_normals(depth[1], *intr[1])["normals"] * (1 - (d1 / d1.max() - 0.5))[:, :, None]
    assert m.max() > 0 and np.unravel_index(np.argmax(m.max(axis=2)), d1.shape)[0] == H - 1
    assert want["normals_u8"][0].max() == 255 and want["normals_u8"][1].max() == 255
    assert_same(device(depth, intr, False, ALL[False]), want, "last pixel")


def test_zero_image_inside_a_batch_and_intrinsics_per_image(problems):
    """a batch of 3 with different intrinsics, the middle image all zero: the per-image maxima must not leak, and the
    degenerate image gives an all-zero uint8 image and scaled depth"""
    rng = np.random.default_rng(5)
    depth, intr = synthetic(rng, 3, 37, 53)
    depth[1] = 0.0
    for for_vis in (True, False):
        want = DN.depth_normals_batch(depth, intr, for_vis=for_vis)
        got = device(depth, intr, for_vis, ALL[for_vis])
        assert_same(got, want, "batch of 3 vis=%d" % int(for_vis))
        assert not got["depth"][1].any() and not got["normals"][1].any()
        if not for_vis:
            assert not got["normals_u8"][1].any() and got["normals_u8"][0].max() == 255 and got["normals_u8"][2].max() == 255
    # each image alone gives what it gives inside the batch
    alone = device(depth[2:3], intr[2:3], False, ALL[False])
    assert_same({k: v[0] for k, v in alone.items()}, {k: v[2] for k, v in want.items()}, "image 2 alone")
    # everything beyond the far cut: the depth has a maximum, the scaled normal image has none
    far = np.full((1, 9, 11), 2500.0, np.float32)
    got = device(far, intr[:1], False, ALL[False])
    assert_same(got, DN.depth_normals_batch(far, intr[:1], for_vis=False), "all far")
    assert not got["normals_u8"].any() and not got["depth"].any()


def test_bad_arguments_return_the_error_code():
    from pyrapose_amd import ops
    from pyrapose_amd._lib import lib
    from pyrapose_amd.runtime import default_context
    ctx = default_context()
    intr = torch.tensor([[500.0, 3.5, 2.5]], dtype=torch.float64, device="cuda")
    ws = torch.empty((1 << 16,), dtype=torch.uint8, device="cuda")
    depth = torch.ones((1, 8, 8), dtype=torch.float32, device="cuda")
    out = torch.empty((1, 8, 8, 3), dtype=torch.float64, device="cuda")
    taps = np.ascontiguousarray(ops.gaussian_taps(2.0))
    tp = taps.ctypes.data_as(C.POINTER(C.c_double))
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(n, H, W, for_vis=1, normals=p(out), u8=None, ws_bytes=ws.numel(), taps_p=tp):
        return lib.pp_depth_normals_f64(ctx.handle, n, H, W, p(depth), p(intr), taps_p, for_vis, p(ws), ws_bytes, normals, u8, None, None)

    assert call(1, 8, 8) == 0
    for n, H, W in ((0, 8, 8), (-1, 8, 8), (1, 2, 8), (1, 8, 2), (1, 0, 8), (1, 8, 16385), (65536, 8, 8)):
        assert call(n, H, W) == -2, (n, H, W)  # PP_ERR_SHAPE
        assert lib.pp_depth_normals_workspace_bytes(n, H, W) == 0
    assert call(1, 8, 8, normals=None) == -1                # no output
    assert call(1, 8, 8, u8=p(out)) == -1                   # the uint8 image under for_vis = 1
    assert call(1, 8, 8, for_vis=2) == -1
    assert call(1, 8, 8, ws_bytes=lib.pp_depth_normals_workspace_bytes(1, 8, 8) - 1) == -1
    assert call(1, 8, 8, taps_p=None) == -1
    torch.cuda.synchronize()
    for bad in ((0, 8, 8), (1, 2, 8), (1, 8, 2)):  # and through the wrapper: ValueError
        with pytest.raises(ValueError):
            ops.depth_normals(ctx, torch.ones(bad, dtype=torch.float32, device="cuda"), intr[:bad[0]], True, ("normals",))
    with pytest.raises(ValueError):
        ops.depth_normals(ctx, depth, intr, True, ("normals_u8",))
    with pytest.raises(ValueError):
        ops.depth_normals(ctx, depth.double(), intr, True, ("normals",))
    with pytest.raises(ValueError):
        ops.depth_normals(ctx, depth, intr, True, ())


def test_taps_are_scipys():
    from pyrapose_amd import ops
    assert np.array_equal(ops.gaussian_taps(2.0), DN.gaussian_taps(2.0)) and ops.gaussian_taps(2.0).shape == (17,)


def test_rendered_depth_end_to_end():
    """render_depth_batch of a small mesh goes straight into normals_from_depth_batch, as a device tensor"""
    from pyrapose_amd.utils.depth_image import normals_from_depth_batch
    from pyrapose_amd.utils.renderer import render_depth_batch
    pts = np.array([[-60, -40, 0], [60, -40, 10], [60, 40, 30], [-60, 40, -20], [0, 0, -50]], np.float64)
    faces = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [0, 2, 1], [0, 3, 2]])
    K = np.array([[120.0, 0, 26.2611], [0, 121.0, 18.049], [0, 0, 1]])
    R = np.stack([np.eye(3), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])])
    t = np.array([[0.0, 0, 400], [5.0, -3, 500]])
    depth = render_depth_batch({"pts": pts, "faces": faces}, (53, 37), K, R, t)
    assert depth.is_cuda and depth.dtype == torch.float32 and tuple(depth.shape) == (2, 37, 53)
    host = depth.cpu().numpy()
    assert (host > 0).any() and (host == 0).any()
    intr = np.tile([K[0, 0], K[0, 2], K[1, 2]], (2, 1))
    for for_vis in (True, False):
        n, d = normals_from_depth_batch(depth, K, for_vis=for_vis)
        want = DN.depth_normals_batch(host, intr, for_vis=for_vis)
        assert_same({"normals" if for_vis else "normals_u8": n.cpu().numpy(), "depth": d.cpu().numpy()}, want, "rendered vis=%d" % int(for_vis))
    s, _ = normals_from_depth_batch(depth, K, signed=True)
    assert_same({"signed": s.cpu().numpy()}, DN.depth_normals_batch(host, intr), "rendered signed")
