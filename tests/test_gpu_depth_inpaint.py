"""GPU: the layered depth-hole filling on the device (pp_depth_inpaint, ops.depth_inpaint, utils.depth_image) against its
float64 numpy restatement tests/depth_inpaint_np.py -- bit for bit, dtype and shape included, for every output: the same IEEE
operations in the same order, the layer map and the counts integers, the extrema exact -- at the edges of the 32-lane row
segments and the 32 x 8 pixel workgroups, for the hole geometries at which the fill takes another path; then end to end from
the depth renderer through augmentDepth and into get_normal."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import depth_aug_np as A
from tests import depth_inpaint_np as I
from tests import depth_normals_np as DN
from tests.test_depth_inpaint_cpu import BORDER_HOLES, plane
from tests.test_gpu_depth_normals import assert_same

pytestmark = pytest.mark.gpu

ALL = I.OUTPUTS
T = 32   # ops.DEPTH_INPAINT_TILE (asserted below): lanes per row segment, pixels per row of a workgroup
R = 8    # ops.DEPTH_INPAINT_ROWS: image rows per workgroup
HB = 64  # DI_HBINS of csrc/depth_inpaint.hip: layers below it are counted and sorted through LDS, the others through global atomics
SHAPES = [(3, 3), (5, 7), (8, 9), (37, 53), (T - 1, T + 1), (T, T), (T + 1, 2 * T + 1), (R - 1, R + 1), (R, R), (R + 1, 2 * R + 1)]


def device(depth, mask=None, radius=5, max_dist=0, rescale=False, want=ALL):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda()
    out = ops.depth_inpaint(default_context(), torch.from_numpy(np.ascontiguousarray(depth, np.float32)).cuda(), m, radius, max_dist,
                            rescale, want)
    return {k: v.cpu().numpy() for k, v in out.items()}


def shape_case(rng, H, W):
    """a batch of 2: scattered holes with a block hole each, against the last row and column in the second image"""
    depth = np.stack([plane(rng, H, W, 0.15), plane(rng, H, W, 0.3)])
    depth[0, H // 4: H // 4 + max(1, H // 3), W // 3: W // 3 + max(1, W // 2)] = 0.0
    depth[1, H - max(1, H // 3):, W - max(1, W // 4):] = 0.0
    depth[:, 0, 0] = 700.0  # (a 3 x 3 image keeps a known pixel)
    return depth


def squares_case(r):
    """(T+12) x (T+12), a batch of 4: a single pixel at a workgroup corner, and squares of width 2r, 2r+1 and 2r+2 (the first whose
    centre sees no known pixel in its window) laid over the corner (x, y) = (T, T) of four workgroups"""
    rng = np.random.default_rng(100 + r)
    H, W = T + 12, T + 12
    depth = np.stack([plane(rng, H, W) for _ in range(4)])
    depth[0, T, T] = 0.0
    for i, w in enumerate((2 * r, 2 * r + 1, 2 * r + 2)):
        y0, x0 = T - w // 2, T - w // 2
        depth[1 + i, y0:y0 + w, x0:x0 + w] = 0.0
    return depth


def borders_case():
    rng = np.random.default_rng(3)
    depth = plane(rng, 12, 15)
    for name in ("top", "left", "bottom-right", "top-right"):
        depth[BORDER_HOLES[name]] = 0.0
    other = plane(rng, 12, 15)
    for name in ("bottom", "right", "top-left", "bottom-left"):
        other[BORDER_HOLES[name]] = 0.0
    rows = plane(rng, 12, 15)
    rows[BORDER_HOLES["first row"]] = rows[BORDER_HOLES["last column"]] = 0.0
    return np.stack([depth, other, rows])


def corner_case():
    depth = np.zeros((1, 9, 13), np.float32)
    depth[0, 0, 0] = 650.0  # one known pixel: layer max(y, x), 12 of them, the last one the 9 pixels of the far column
    return depth


def deep_case():
    """9 x (HB + 6), a batch of 2: one known pixel in a corner, so the layers 1 .. HB + 5 lie on both sides of the LDS histogram's
    last bin with 9 pixels each (fewer than a workgroup holds); and a shallow image, which the deep launches must leave alone"""
    rng = np.random.default_rng(21)
    deep = np.zeros((9, HB + 6), np.float32)
    deep[8, 0] = 700.0
    shallow = plane(rng, 9, HB + 6)
    shallow[3:6, 10:50] = 0.0
    return np.stack([deep, shallow])


def segment_case():
    """5 x 100: a hole 41 wide over the whole 32-pixel row segment 32..63, so the nearest known pixel is carried through a
    segment without one from both sides; in the second image the hole runs to the last column (no known pixel on the right)"""
    rng = np.random.default_rng(22)
    depth = np.stack([plane(rng, 5, 100), plane(rng, 5, 100)])
    depth[0, :, 30:71] = 0.0
    depth[1, 1:4, 25:] = 0.0
    return depth


def mixed_case():
    """no hole, a shallow hole, a deep hole: the number of fill launches comes from the deepest image"""
    rng = np.random.default_rng(11)
    depth = np.stack([plane(rng, 37, 53) for _ in range(3)])
    depth[1, 10:13, 20:24] = 0.0
    depth[2, 5:30, 8:40] = 0.0
    return depth


def masked_case():
    rng = np.random.default_rng(7)
    depth = np.stack([plane(rng, 16, 19, 0.1), plane(rng, 16, 19, 0.1)])
    mask = np.zeros(depth.shape, np.uint8)
    mask[0, 4:9, 5:12] = 3    # non-zero pixels marked as holes, zero pixels left known
    mask[1, 0:6, 13:] = 255
    mask[1, 9, 9] = 1
    assert ((depth == 0) & (mask == 0)).any() and ((depth != 0) & (mask != 0)).any()
    return depth, mask


def constant_case():
    a = np.full((10, 11), 812.0, np.float32)   # the means are off the constant by an ulp or two: max v > min v, stretched
    b = np.full((10, 11), 1024.0, np.float32)  # a power of two: the means are exact, max v = min v, left alone
    c = np.full((10, 11), 333.0, np.float32)   # no holes
    a[3:6, 4:8] = b[3:6, 4:8] = 0.0
    return np.stack([a, b, c])


def build_cases():
    """name -> (depth, mask, radius, max_dist, rescale)"""
    rng = np.random.default_rng(17)
    cases = {}
    for hw in SHAPES:
        depth = shape_case(rng, *hw)
        for rescale in (False, True):
            cases["%dx%d rescale=%d" % (hw + (int(rescale),))] = (depth, None, 5, 0, rescale)
    for r in (1, 5, 8):
        cases["squares r=%d" % r] = (squares_case(r), None, r, 0, False)
        cases["borders r=%d" % r] = (borders_case(), None, r, 0, r == 5)
    for max_dist in (0, 11, 12, 13):  # the largest layer is 12
        cases["corner max_dist=%d" % max_dist] = (corner_case(), None, 5, max_dist, max_dist == 12)
    cases["corner r=1"] = (corner_case(), None, 1, 0, False)
    for max_dist in (0, 4, 13):       # the deep hole of the mixed batch has 13 layers
        cases["mixed max_dist=%d" % max_dist] = (mixed_case(), None, 5, max_dist, False)
    cases["mixed rescale"] = (mixed_case(), None, 8, 0, True)
    for max_dist in (0, HB - 1, HB, HB + 1):  # the largest layer is HB + 5
        cases["deep max_dist=%d" % max_dist] = (deep_case(), None, 5, max_dist, max_dist == HB)
    cases["deep alone r=8"] = (deep_case()[:1], None, 8, 0, True)
    cases["segment"] = (segment_case(), None, 5, 0, False)
    depth, mask = masked_case()
    cases["mask"] = (depth, mask, 5, 0, False)
    cases["mask rescale"] = (depth, mask, 3, 2, True)
    cases["constant"] = (constant_case(), None, 2, 0, True)
    cases["constant plain"] = (constant_case(), None, 2, 0, False)
    return cases


CASES = build_cases()


@pytest.fixture(scope="module")
def wanted():
    """the restatement of every case, computed once and shared"""
    return {k: I.depth_inpaint_batch(*c) for k, c in CASES.items()}


def test_constants():
    from pyrapose_amd import ops
    import os
    import re
    assert ops.DEPTH_INPAINT_TILE == T and ops.DEPTH_INPAINT_ROWS == R
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyrapose_amd", "csrc", "depth_inpaint.hip")).read()
    assert int(re.search(r"#define DI_HBINS (\d+)", src).group(1)) == HB


@pytest.mark.parametrize("name", list(CASES))
def test_all_outputs_match_restatement(wanted, name):
    assert_same(device(*CASES[name]), wanted[name], name)


def test_the_cases_are_what_they_claim(wanted):
    for r in (1, 5, 8):
        c = wanted["squares r=%d" % r]["counts"]
        assert c[:, 0].tolist() == [1, 4 * r * r, (2 * r + 1) ** 2, (2 * r + 2) ** 2] and c[:, 2].tolist() == [1, r, r + 1, r + 1]
        assert np.array_equal(c[:, 0], c[:, 1])
    for max_dist, filled in ((0, 116), (11, 116 - 9), (12, 116), (13, 116)):
        w = wanted["corner max_dist=%d" % max_dist]
        assert w["counts"].tolist() == [[116, filled, 12]] and (w["filled_f64"][0, 8, 12] == 0) == (max_dist == 11)
    assert wanted["mixed max_dist=0"]["counts"].tolist() == [[0, 0, 0], [12, 12, 2], [800, 800, 13]]
    assert wanted["mixed max_dist=4"]["counts"].tolist() == [[0, 0, 0], [12, 12, 2], [800, 800 - 17 * 24, 13]]
    for max_dist, last in ((0, HB + 5), (HB - 1, HB - 1), (HB, HB), (HB + 1, HB + 1)):
        w = wanted["deep max_dist=%d" % max_dist]
        assert w["counts"].tolist() == [[9 * (HB + 6) - 1, 9 * last + 8, HB + 5], [120, 120, 2]]
        row = w["filled_f64"][0, 0]  # (row 0, column x: layer max(8, x))
        assert (row[:last + 1] > 0).all() and not row[last + 1:].any()
    assert wanted["segment"]["counts"].tolist() == [[205, 205, 21], [225, 225, 2]]
    assert wanted["segment"]["layer"][0, 2, 30:71].tolist() == list(range(1, 22)) + list(range(20, 0, -1))
    # an image without holes: its bits
    depth = CASES["mixed max_dist=0"][0]
    assert np.array_equal(wanted["mixed max_dist=0"]["filled_f32"][0], depth[0]) and not wanted["mixed max_dist=0"]["layer"][0].any()
    k = wanted["constant"]
    assert k["filled_f64"][0].min() == 0.0 and k["filled_f64"][0].max() == 812.0
    assert np.array_equal(k["filled_f64"][1], np.full((10, 11), 1024.0)) and np.array_equal(k["filled_f64"][2], np.full((10, 11), 333.0))


def test_images_without_holes_or_without_known_pixels():
    rng = np.random.default_rng(2)
    depth = np.stack([plane(rng, 9, 11), np.zeros((9, 11), np.float32), plane(rng, 9, 11)])
    mask = np.zeros(depth.shape, np.uint8)
    mask[2] = 1  # every pixel of a non-zero image masked
    for m in (None, mask):
        for rescale in (False, True):
            got = device(depth, m, 5, 0, rescale)
            assert_same(got, I.depth_inpaint_batch(depth, m, 5, 0, rescale), "degenerate rescale=%d" % int(rescale))
            assert not got["filled_f32"][1].any()
            if m is None:  # the zero image: all holes by the default rule, all known under the explicit mask
                assert got["counts"][1].tolist() == [99, 0, 0] and (got["layer"][1] == I.NO_LAYER).all()
            else:
                assert got["counts"][1].tolist() == [0, 0, 0] and not got["layer"][1].any()
                assert got["counts"][2].tolist() == [99, 0, 0] and np.array_equal(got["filled_f32"][2], depth[2])
            if not rescale:
                assert got["counts"][0].tolist() == [0, 0, 0] and np.array_equal(got["filled_f32"][0].view(np.int32), depth[0].view(np.int32))


def test_each_output_alone_and_run_to_run(wanted):
    """every null-pointer path of the entry point, on the shape with partial workgroups on both axes; and twice the same bits"""
    name = "%dx%d rescale=1" % (T + 1, 2 * T + 1)
    for k in ALL:
        got = device(*CASES[name], want=(k,))
        assert list(got) == [k]
        assert_same(got, wanted[name], "alone " + k)
    a, b = device(*CASES[name]), device(*CASES[name])
    assert_same(a, b, "run to run")
    assert_same(device(*CASES["mixed rescale"]), device(*CASES["mixed rescale"]), "run to run, mixed")


def test_each_image_alone_gives_what_it_gives_in_the_batch(wanted):
    depth = CASES["mixed rescale"][0]
    for i in range(3):
        alone = device(depth[i:i + 1], None, 8, 0, True)
        assert_same({k: v[0] for k, v in alone.items()}, {k: v[i] for k, v in wanted["mixed rescale"].items()}, "image %d alone" % i)


def test_bad_arguments_return_the_error_code():
    from pyrapose_amd import ops
    from pyrapose_amd._lib import lib
    from pyrapose_amd.runtime import default_context
    ctx = default_context()
    need = lib.pp_depth_inpaint_workspace_bytes(1, 8, 8)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    depth = torch.ones((1, 8, 8), dtype=torch.float32, device="cuda")
    out = torch.empty((1, 8, 8), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(n=1, H=8, W=8, depth_p=p(depth), radius=5, max_dist=0, rescale=0, ws_p=p(ws), ws_bytes=need, out_p=p(out)):
        return lib.pp_depth_inpaint(ctx.handle, n, H, W, depth_p, None, radius, max_dist, rescale, ws_p, ws_bytes, out_p, None, None, None)

    assert call() == 0
    for n, H, W in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 2, 8), (1, 8, 2), (1, 4097, 8), (1, 8, 4097)):
        assert call(n, H, W) == -2, (n, H, W)  # PP_ERR_SHAPE
    for kw in (dict(radius=0), dict(radius=9), dict(max_dist=-1), dict(max_dist=65536), dict(rescale=2), dict(depth_p=None),
               dict(ws_p=None), dict(ws_bytes=need - 1), dict(out_p=None)):
        assert call(**kw) == -1, kw            # PP_ERR_ARG
    assert call(max_dist=65535) == 0
    torch.cuda.synchronize()
    for bad in ((0, 8, 8), (1, 2, 8), (1, 8, 2)):  # and through the wrapper: ValueError
        with pytest.raises(ValueError):
            ops.depth_inpaint(ctx, torch.ones(bad, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        ops.depth_inpaint(ctx, depth, radius=9)
    with pytest.raises(ValueError):
        ops.depth_inpaint(ctx, depth.double())
    with pytest.raises(ValueError):
        ops.depth_inpaint(ctx, depth, torch.zeros((1, 8, 9), dtype=torch.uint8, device="cuda"))


def test_rendered_depth_end_to_end():
    """render_depth_batch -> augment_depth_batch -> inpaint_depth_batch -> normals_from_depth_batch on device tensors equals the
    three restatements chained; the one-call form and the reference's three-value get_normal; inpaint=None is untouched"""
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    from pyrapose_amd.utils.depth_image import (augment_depth_batch, get_normal_inpaint, inpaint_depth_batch, normals_from_depth_batch,
                                                sample_depth_programs)
    from pyrapose_amd.utils.renderer import render_depth_batch
    pts = np.array([[-60, -40, 0], [60, -40, 10], [60, 40, 30], [-60, 40, -20], [0, 0, -50]], np.float64)
    faces = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [0, 2, 1], [0, 3, 2]])
    K = np.array([[120.0, 0, 26.2611], [0, 121.0, 18.049], [0, 0, 1]])
    R = np.stack([np.eye(3), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])])
    t = np.array([[0.0, 0, 400], [5.0, -3, 500]])
    depth = render_depth_batch({"pts": pts, "faces": faces}, (53, 37), K, R, t)
    host = depth.cpu().numpy()
    programs = sample_depth_programs(np.random.default_rng(8), 2)
    z = np.random.default_rng(9).standard_normal((2, 18, 26)).astype(np.float32)
    intr = np.tile([K[0, 0], K[0, 2], K[1, 2]], (2, 1))
    noisy = augment_depth_batch(depth, None, programs, z=z)
    want_noisy = A.depth_augment_batch(host, (host > 0).astype(np.uint8), programs, z)["depth_f32"]
    assert (want_noisy == 0).any() and (want_noisy > 0).any()
    filled = inpaint_depth_batch(noisy, radius=5, max_dist=6, rescale=True)
    assert filled.is_cuda and filled.dtype == torch.float32 and tuple(filled.shape) == (2, 37, 53)
    want_filled = I.depth_inpaint_batch(want_noisy, None, 5, 6, True)
    assert_same({"filled_f32": filled.cpu().numpy()}, want_filled, "rendered, filled")
    assert (want_filled["counts"][:, 1] > 0).all() and (want_filled["filled_f32"] == 0).any()  # filled at the rim, the far background empty
    n, d = normals_from_depth_batch(filled, K, for_vis=False)
    ref = DN.depth_normals_batch(want_filled["filled_f32"], intr, for_vis=False)
    assert_same({"normals_u8": n.cpu().numpy(), "depth": d.cpu().numpy()}, ref, "rendered, normals of the filled depth")
    n3, d3, f3 = normals_from_depth_batch(noisy, K, for_vis=False, inpaint=dict(radius=5, max_dist=6, rescale=True))
    assert torch.equal(n3, n) and torch.equal(d3, d) and torch.equal(f3, filled)
    # the reference's three-value get_normal: radius 5, no limit, rescaled
    one = want_noisy[0]
    for for_vis in (True, False):
        got = get_normal_inpaint(one, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], for_vis=for_vis)
        assert len(got) == 3 and all(isinstance(a, np.ndarray) for a in got)
        f = I.depth_inpaint(one, None, 5, 0, True)["filled_f32"]
        ref = DN.depth_normals_batch(f[None], intr[:1], for_vis=for_vis)
        assert_same({"normals" if for_vis else "normals_u8": got[0][None], "depth": got[1][None], "filled_f32": got[2][None]},
                    dict(ref, filled_f32=f[None]), "get_normal_inpaint vis=%d" % int(for_vis))
        assert got[0].dtype == (np.float64 if for_vis else np.uint8) and got[0].shape == (37, 53, 3)
        assert got[1].dtype == np.float64 and got[2].dtype == np.float32 and got[1].shape == got[2].shape == (37, 53)
    # inpaint=None: the two values of before, from the same call of ops.depth_normals
    two = normals_from_depth_batch(noisy, K, inpaint=None)
    direct = ops.depth_normals(default_context(), noisy, torch.from_numpy(intr).cuda(), True, ("normals", "depth"))
    assert len(two) == 2 and torch.equal(two[0], direct["normals"]) and torch.equal(two[1], direct["depth"])
