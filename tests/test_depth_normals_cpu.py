"""The numpy restatement of the depth normal images (tests/depth_normals_np.py) against the reference's own get_normal
(tests/golden/depth_normals.npz, written by tests/golden/make_golden_depth_normals.py), and the host-side argument handling of
utils.depth_image.  No device is needed.

Bounds.  The restatement adds a pass's 17 products in tap order, scipy folds the symmetric taps pairwise; nothing else differs.
Measured over the fixture when it was generated (numpy 2.2.6, scipy 1.15.3), at every pixel whose reference smoothed depth is
not exactly 0: normals 4.07e-14 absolute (case C; A 3.5e-14, B 2.7e-14, D 2.5e-15), smoothed depth 7.9e-16 relative; the uint8
images of cases A and B differ on no value.  Asserted: 100 x those, 4.1e-12 and 7.9e-14; both are far below the 1e-9 above which
something other than summation order would have to differ."""
import os
import warnings

import numpy as np
import pytest

from pyrapose_amd import ops
from pyrapose_amd.utils import depth_image
from tests import depth_normals_np as DN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_normals.npz")
CASES = {"A": (True, False), "B": (True, False), "C": (True,), "D": (True,)}
NORMALS_ATOL = 100 * 4.07e-14
DEPTH_RTOL = 100 * 7.9e-16
MAX_EXCLUDED = 0.10
U8_MAX_LEVELS, U8_MAX_SHARE = 1, 1e-4


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def check_against_golden(golden, name, for_vis, got_normals, got_depth):
    """the bounds both the restatement and the device must meet against the reference's returned pair"""
    tag = "%s_vis%d" % (name, int(for_vis))
    ref_n, ref_d = golden[tag + "_normals"], golden[tag + "_smoothed"]
    assert got_normals.shape == ref_n.shape and got_normals.dtype == ref_n.dtype
    assert got_depth.shape == ref_d.shape and got_depth.dtype == ref_d.dtype == np.float64
    keep = ref_d != 0
    assert 1.0 - keep.mean() < MAX_EXCLUDED
    rel = np.abs(got_depth - ref_d)[keep] / np.abs(ref_d[keep])
    print("%s: depth max rel diff %.3e (bound %.3e), excluded %.5f" % (tag, rel.max(), DEPTH_RTOL, 1.0 - keep.mean()))
    assert rel.max() <= DEPTH_RTOL
    if for_vis:
        diff = np.abs(got_normals - ref_n)[keep].max()
        print("%s: normals max abs diff %.3e (bound %.3e)" % (tag, diff, NORMALS_ATOL))
        assert diff <= NORMALS_ATOL
    else:
        assert ref_n.dtype == np.uint8
        du = np.abs(got_normals.astype(np.int32) - ref_n.astype(np.int32))
        print("%s: uint8 values that differ %d of %d, max %d" % (tag, int((du != 0).sum()), du.size, int(du.max())))
        assert du.max() <= U8_MAX_LEVELS
        assert (du != 0).sum() <= U8_MAX_SHARE * du.size


@pytest.mark.parametrize("name,for_vis", [(n, v) for n, modes in CASES.items() for v in modes])
def test_restatement_matches_reference(golden, name, for_vis):
    fx, _fy, cx, cy = golden[name + "_intr"]
    out = DN.depth_normals(golden[name + "_depth"], fx, cx, cy, for_vis=for_vis)
    check_against_golden(golden, name, for_vis, out["normals" if for_vis else "normals_u8"], out["depth"])


def test_fixture_is_what_the_issue_asks(golden):
    A, B, C, D = (golden[k + "_depth"] for k in "ABCD")
    assert A.min() > 0 and (golden["A_vis1_smoothed"] > 2000).any() and (golden["A_vis1_smoothed"] <= 2000).any()
    assert (B == 0).any() and golden["B_vis1_smoothed"].min() > 0
    assert (golden["C_vis1_smoothed"] == 0).any() and (C == 0).sum() <= C.size / 16
    assert D.shape == (5, 7)
    for k in "ABCD":  # float32, what the device takes, holds the depth exactly; cx, cy are off the integer grid and inside
        d, (fx, fy, cx, cy) = golden[k + "_depth"], golden[k + "_intr"]
        assert np.array_equal(d, d.astype(np.float32))
        assert cx != int(cx) and cy != int(cy) and 0 < cx < d.shape[1] - 1 and 0 < cy < d.shape[0] - 1
    assert "C_vis0_normals" not in golden and "D_vis0_normals" not in golden


def test_signed_is_the_normal_before_abs(golden):
    fx, _fy, cx, cy = golden["B_intr"]
    out = DN.depth_normals(golden["B_depth"], fx, cx, cy)
    assert np.array_equal(np.abs(out["signed"]), out["normals"])
    assert (out["signed"] < 0).any()
    length = np.linalg.norm(out["signed"], axis=2)
    far = out["depth"] > 2000
    assert np.all(length[far] == 0) and np.allclose(length[~far], 1.0, atol=1e-12)


def test_gaussian_matches_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    for shape in ((3, 3), (5, 7), (8, 9), (37, 53)):  # shorter than the radius: the padding mirrors again and again
        a = np.rint(rng.uniform(0, 3000, size=shape))
        np.testing.assert_allclose(DN.smooth(a), ndimage.gaussian_filter(a, 2), rtol=1e-13, atol=0)


def test_degenerate_images():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = DN.depth_normals(np.zeros((9, 11)), 500.0, 5.3, 4.2, for_vis=False)
        assert out["normals_u8"].dtype == np.uint8 and not out["normals_u8"].any()
        assert out["depth"].dtype == np.float64 and not out["depth"].any()
        # everything beyond the far cut: the depth has a maximum, the scaled normal image has none
        out = DN.depth_normals(np.full((9, 11), 2500.0), 500.0, 5.3, 4.2, for_vis=False)
        assert not out["normals_u8"].any() and not out["depth"].any()
        vis = DN.depth_normals(np.zeros((9, 11)), 500.0, 5.3, 4.2, for_vis=True)
        assert not vis["normals"].any() and not vis["signed"].any() and not vis["depth"].any()


# ---- utils.depth_image: what it checks before it needs a device -------------------------------------------------------------

def test_the_library_takes_the_restatements_taps():
    """one exp for both: ops.gaussian_taps is what the entry point is given"""
    w = ops.gaussian_taps(2.0)
    assert w.dtype == np.float64 and w.shape == (2 * DN.RADIUS + 1,) and np.array_equal(w, DN.gaussian_taps(2.0))
    assert np.array_equal(w, w[::-1]) and (w > 0).all() and abs(w.sum() - 1.0) < 1e-15
    assert ops.DEPTH_NORMALS_TILE >= 2 * DN.RADIUS


def test_intrinsics_forms():
    m = depth_image
    K = np.array([[572.4, 0, 325.26], [0, 573.6, 242.05], [0, 0, 1]])
    assert np.array_equal(m._intrinsics(K, 4), np.tile([572.4, 325.26, 242.05], (4, 1)))
    Ks = np.stack([K, 2 * K])
    assert np.array_equal(m._intrinsics(Ks, 2), np.array([[572.4, 325.26, 242.05], [1144.8, 650.52, 484.1]]))
    assert np.array_equal(m._intrinsics([500.0, 3.5, 2.5], 3), np.tile([500.0, 3.5, 2.5], (3, 1)))
    per = np.array([[500.0, 3.5, 2.5], [400.0, 1.5, 0.5]])
    assert np.array_equal(m._intrinsics(per, 2), per)
    assert np.array_equal(m._intrinsics(K, 3), np.tile([572.4, 325.26, 242.05], (3, 1)))  # one K, not three rows
    for bad in (np.zeros((2, 2)), np.zeros((3, 3, 3)), np.zeros(4)):
        with pytest.raises(ValueError):
            m._intrinsics(bad, 2)
    with pytest.raises(ValueError):
        m._intrinsics([0.0, 1.0, 1.0], 1)  # fx = 0
    with pytest.raises(ValueError):
        m._intrinsics([np.nan, 1.0, 1.0], 1)


def test_argument_errors_need_no_device():
    m = depth_image
    K = [500.0, 3.5, 2.5]
    with pytest.raises(ValueError):
        m.get_normal(np.zeros((2, 8, 8)), 500.0, 500.0, 3.5, 2.5)  # not [H,W]
    with pytest.raises(ValueError):
        m.normals_from_depth_batch(np.zeros((8, 8)), K)  # not [n,H,W]
    with pytest.raises(ValueError):
        m.normals_from_depth_batch(np.zeros((1, 2, 8)), K)  # H < 3
    with pytest.raises(ValueError):
        m.normals_from_depth_batch(np.zeros((1, 8, 2)), K)  # W < 3
    with pytest.raises(ValueError):
        m.normals_from_depth_batch(np.zeros((0, 8, 8)), K)  # no image
    with pytest.raises(ValueError):
        m.normals_from_depth_batch(np.zeros((1, 8, 8), np.complex128), K)
    with pytest.raises(ValueError):
        m.normals_from_depth_batch(np.zeros((1, 8, 8)), K, for_vis=False, signed=True)
