"""The numpy restatement of the layered depth-hole filling (tests/depth_inpaint_np.py) against what pins it -- scipy's
chessboard distance transform for the layer map, the properties of a weighted mean for the values -- the host side of
ops / utils.depth_image, and the C ABI of the two entry points.  No device is needed.  OpenCV is not a dependency: parity with
cv2.inpaint is not pinned."""
import os
import re

import numpy as np
import pytest

from pyrapose_amd import ops
from pyrapose_amd.utils import depth_image
from tests import depth_inpaint_np as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pp_depth_inpaint_workspace_bytes", "pp_depth_inpaint")
RADII = (1, 5, ops.DEPTH_INPAINT_MAX_RADIUS)

# holes of a 12 x 15 image that touch each border and each corner, a whole first row / column, and all but one corner pixel
BORDER_HOLES = {
    "top": (slice(0, 3), slice(4, 9)), "bottom": (slice(-3, None), slice(4, 9)), "left": (slice(4, 9), slice(0, 3)),
    "right": (slice(4, 9), slice(-3, None)), "top-left": (slice(0, 4), slice(0, 4)), "top-right": (slice(0, 4), slice(-4, None)),
    "bottom-left": (slice(-4, None), slice(0, 4)), "bottom-right": (slice(-4, None), slice(-4, None)),
    "first row": (slice(0, 1), slice(None)), "last row": (slice(-1, None), slice(None)), "first column": (slice(None), slice(0, 1)),
    "last column": (slice(None), slice(-1, None))}


def border_mask(name):
    hole = np.zeros((12, 15), bool)
    hole[BORDER_HOLES[name]] = True
    return hole


def plane(rng, H, W, p_hole=0.0):
    """whole-millimetre tilted plane, all positive, with random single-pixel holes"""
    y, x = np.mgrid[0:H, 0:W]
    depth = np.rint(600.0 + 7.0 * x + 11.0 * y + rng.integers(-4, 5, size=(H, W))).astype(np.float32)
    depth[rng.random((H, W)) < p_hole] = 0.0
    return depth


def test_layer_map_is_scipys_chessboard_transform():
    """scipy.ndimage.distance_transform_cdt(hole, metric='chessboard') treats the image border as this rule does (pixels outside
    the image do not exist: they are no known pixels to measure a distance to): every border and corner case below agrees, none
    had to be left out.  Only the image without a known pixel differs -- scipy returns -1 there -- and is checked against the rule
    of the restatement, which stands: NO_LAYER everywhere."""
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    n = 0
    for _ in range(200):
        H, W = (int(s) for s in rng.integers(3, 40, size=2))
        hole = rng.random((H, W)) < rng.choice([0.3, 0.7, 0.95, 0.99])
        if hole.all():
            continue
        got = I.layer_map(hole)
        assert got.dtype == np.int64 and np.array_equal(got, ndimage.distance_transform_cdt(hole, metric="chessboard")), (H, W)
        n += 1
    assert n > 150
    for name in BORDER_HOLES:
        hole = border_mask(name)
        assert np.array_equal(I.layer_map(hole), ndimage.distance_transform_cdt(hole, metric="chessboard")), name
    hole = np.ones((9, 13), bool)
    hole[0, 0] = False  # one known pixel in a corner: a layer per diagonal band
    L = I.layer_map(hole)
    assert np.array_equal(L, ndimage.distance_transform_cdt(hole, metric="chessboard")) and L.max() == 12
    y, x = np.mgrid[0:9, 0:13]
    assert np.array_equal(L, np.maximum(y, x))
    assert not I.layer_map(np.zeros((4, 5), bool)).any()
    # the all-hole image: scipy has no answer (-1), the rule has
    assert (ndimage.distance_transform_cdt(np.ones((5, 6), bool), metric="chessboard") == -1).all()
    assert (I.layer_map(np.ones((5, 6), bool)) == I.NO_LAYER).all() and I.NO_LAYER == ops.DEPTH_INPAINT_NO_LAYER
    out = I.depth_inpaint(np.zeros((5, 6), np.float32))
    assert out["counts"].tolist() == [30, 0, 0] and not out["filled_f64"].any() and (out["layer"] == I.NO_LAYER).all()
    ramp = np.arange(1, 31, dtype=np.float32).reshape(5, 6)
    out = I.depth_inpaint(ramp, np.ones((5, 6), np.uint8), rescale=True)  # every pixel masked: the image as it came
    assert out["counts"].tolist() == [30, 0, 0] and np.array_equal(out["filled_f64"], ramp.astype(np.float64))


@pytest.mark.parametrize("radius", RADII)
def test_filled_values_are_means_of_known_values(radius):
    rng = np.random.default_rng(radius)
    depth = plane(rng, 23, 29, 0.2)
    depth[5:18, 8:21] = 0.0  # 13 x 13, 7 layers: its centre sees no known pixel in the windows of radius 1 and 5
    depth[0:3, 0:4] = 0.0
    depth[-2:, 10:] = 0.0
    known = depth != 0
    lo, hi = float(depth[known].min()), float(depth[known].max())
    L = I.layer_map(~known)
    for max_dist in (0, 3):
        out = I.depth_inpaint(depth, None, radius, max_dist)
        v = out["filled_f64"]
        assert v.dtype == np.float64 and out["filled_f32"].dtype == np.float32 and out["layer"].dtype == np.uint16
        assert np.array_equal(out["layer"], L) and np.array_equal(out["filled_f32"], v.astype(np.float32))
        assert np.array_equal(v[known].view(np.int64), depth[known].astype(np.float64).view(np.int64))  # known pixels keep their bits
        reach = (L >= 1) & ((L <= max_dist) if max_dist else True)
        assert reach.any() and (v[reach] > 0).all()            # nothing within reach is left at 0
        assert (v[reach] >= lo * (1 - 1e-12)).all() and (v[reach] <= hi * (1 + 1e-12)).all()
        assert not v[(L >= 1) & ~reach].any()                  # and nothing beyond it is touched
        assert out["counts"].tolist() == [int((~known).sum()), int(reach.sum()), int(L.max())]
    assert L.max() == 7 and (~reach).any()


def test_explicit_mask_and_rescale():
    rng = np.random.default_rng(7)
    depth = plane(rng, 16, 19, 0.1)
    mask = np.zeros(depth.shape, np.uint8)
    mask[4:9, 5:12] = 3          # non-zero pixels marked as holes ...
    zero_known = (depth == 0) & (mask == 0)
    assert zero_known.any()      # ... and zero pixels left known
    out = I.depth_inpaint(depth, mask, 5, 0)
    v = out["filled_f64"]
    assert out["counts"][0] == 35 and np.array_equal(v[mask == 0], depth[mask == 0].astype(np.float64)) and not v[zero_known].any()
    assert (v[mask != 0] >= 0).all() and (v[mask != 0] <= depth[mask == 0].max()).all()
    assert not np.array_equal(v[mask != 0], depth[mask != 0].astype(np.float64))
    # rescaled: minimum 0, maximum the largest input depth (a masked pixel's, here)
    depth[6, 7] = 5000.0
    r = I.depth_inpaint(depth, mask, 5, 0, rescale=True)["filled_f64"]
    assert r.min() == 0.0 and r.max() == 5000.0
    plain = I.depth_inpaint(plane(rng, 9, 11, 0.2), None, 3, 0, rescale=True)["filled_f64"]
    assert plain.min() == 0.0 and plain.max() > 0
    # a constant image is left alone (the reference divides by zero): one without holes, and one whose fill is exact -- with a
    # power of two every product w v and every sum is the same multiple of the weights', so the means are the constant itself.
    # (With another constant the means are off by an ulp or two, max v > min v, and the image is stretched like any other.)
    for flat in (np.full((7, 8), 812.0, np.float32), np.full((7, 8), 1024.0, np.float32)):
        if flat[0, 0] == 1024.0:
            flat[2:5, 3:6] = 0.0
        out = I.depth_inpaint(flat, None, 2, 0, rescale=True)["filled_f64"]
        assert np.array_equal(out, np.full((7, 8), float(flat[0, 0])))
    # a batch is its images one by one
    both = I.depth_inpaint_batch(np.stack([flat, flat * 2]), None, 2, 0, True)
    assert both["filled_f64"].shape == (2, 7, 8) and both["counts"].tolist() == [[9, 9, 2], [9, 9, 2]] and tuple(both) == I.OUTPUTS


def test_constants_agree():
    assert tuple(ops.DEPTH_INPAINT_OUTPUTS) == I.OUTPUTS and ops.DEPTH_INPAINT_MAX_RADIUS == I.MAX_RADIUS == 8
    assert ops.DEPTH_INPAINT_TILE == 32 and ops.DEPTH_INPAINT_ROWS == 8
    src = open(os.path.join(ROOT, "pyrapose_amd", "csrc", "depth_inpaint.hip")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define DI_([A-Z_]+) (\d+)\b", src)}
    assert consts["TILE"] == ops.DEPTH_INPAINT_TILE and consts["ROWS"] == ops.DEPTH_INPAINT_ROWS
    assert consts["MAX_RADIUS"] == ops.DEPTH_INPAINT_MAX_RADIUS and consts["MAX_DIST"] == ops.DEPTH_INPAINT_MAX_DIST
    assert consts["MAX_SIDE"] == ops.DEPTH_INPAINT_MAX_SIDE and consts["FAR"] == ops.DEPTH_INPAINT_NO_LAYER


def test_argument_errors_need_no_device():
    m = depth_image
    for bad in (np.zeros((8, 8)), np.zeros((1, 2, 8)), np.zeros((1, 8, 2)), np.zeros((0, 8, 8))):
        with pytest.raises(ValueError):
            m.inpaint_depth_batch(bad)
    with pytest.raises(ValueError):
        m.inpaint_depth_batch(np.ones((1, 8, 8)), hole_mask=np.zeros((1, 8, 9)))
    with pytest.raises(ValueError):  # nested lists are arrays too: the documented error, not an AttributeError
        m.inpaint_depth_batch(np.ones((1, 8, 8)).tolist(), hole_mask=np.zeros((1, 8, 9)).tolist())
    with pytest.raises(ValueError):
        m.inpaint_depth_batch(np.ones((8, 8)).tolist())
    for kw in (dict(radius=0), dict(radius=9), dict(max_dist=-1), dict(max_dist=65536)):
        with pytest.raises(ValueError):
            m.inpaint_depth_batch(np.ones((1, 8, 8)), **kw)
    with pytest.raises(ValueError):
        m.get_normal_inpaint(np.zeros((2, 8, 8)), 500.0, 500.0, 4.0, 4.0)
    with pytest.raises(ValueError):
        ops.depth_inpaint(None, None, want=())
    with pytest.raises(ValueError):
        ops.depth_inpaint(None, None, want=("filled",))
    with pytest.raises(ValueError):
        ops.depth_inpaint(None, np.zeros((1, 8, 8), np.float32))  # not a device tensor


def test_entry_points_declared_and_exported():
    from pyrapose_amd import _lib
    src = open(os.path.join(ROOT, "include", "pyrapose_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.EXPORTS and hasattr(_lib.lib, name)
    argtypes = _lib.lib.pp_depth_inpaint.argtypes
    decl = re.search(r"int pp_depth_inpaint\((.*?)\);", code, flags=re.S).group(1)
    assert len(argtypes) == len(decl.split(",")) == 15
    # pointers are void*, integers int, the byte count size_t -- in the header's order
    kinds = ["p" if "*" in a else ("z" if "size_t" in a else "i") for a in decl.split(",")]
    import ctypes as C
    assert [{C.c_void_p: "p", C.c_int: "i", C.c_size_t: "z"}[t] for t in argtypes] == kinds
    assert _lib.lib.pp_depth_inpaint_workspace_bytes.argtypes == [C.c_int] * 3 and _lib.lib.pp_depth_inpaint_workspace_bytes.restype == C.c_size_t
    # host-side refusals need no device: a NULL context first, as everywhere; a refused shape has no workspace
    assert _lib.lib.pp_depth_inpaint(None, 1, 8, 8, None, None, 5, 0, 0, None, 0, None, None, None, None) == -4
    for n, H, W in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 2, 8), (1, 8, 2), (1, 4097, 8), (1, 8, 4097), (128, 4096, 4096)):
        assert _lib.lib.pp_depth_inpaint_workspace_bytes(n, H, W) == 0, (n, H, W)
    a256 = lambda v: (v + 255) // 256 * 256
    for n, H, W in ((1, 3, 3), (2, 37, 53), (64, 480, 640), (1, 4096, 4096)):
        P = n * H * W
        want = a256(4 * (4 * n + 12289)) + a256(24 * n) + 2 * a256(2 * P) + a256(4 * P) + a256(8 * P)
        assert _lib.lib.pp_depth_inpaint_workspace_bytes(n, H, W) == want, (n, H, W)
