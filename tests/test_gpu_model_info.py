"""GPU: model geometry on the device (pp_pts_diameter_f64 / pp_farthest_points_f64, ops.pts_diameter / farthest_points,
utils.model_info) against the float64 numpy restatement tests/model_info_np.py -- bit for bit: the same IEEE operations in the
same order, maxima exact, ties to the lowest index -- at the edges of the diameter's tile and of the sampling workgroup."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import model_info_np as MN
from tests import render_np as RN

pytestmark = pytest.mark.gpu

CENTRE = np.array([1000.0, 1000.0, 1000.0])


def tile_sizes():
    from pyrapose_amd import ops
    T = ops.DIAMETER_TILE
    return sorted({1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T - 1, 1500})


def fps_sizes():
    from pyrapose_amd import ops
    W = ops.FPS_THREADS
    return [1, 2, W - 1, W, W + 1, 2 * W + 1]


def device_diameter(pts):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    d2, pair = ops.pts_diameter(default_context(), torch.from_numpy(np.ascontiguousarray(pts)).cuda())
    return d2.cpu().numpy(), pair.cpu().numpy()


def assert_diameter(pts, what, planted=None):
    got, want = device_diameter(pts), MN.diameter_np(pts)
    print(what, "device", got, "restatement", want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, got, want)
    if planted is not None:
        assert tuple(want[1]) == planted, (what, want, planted)   # (the test's own construction)
    return want


def far_cloud(rng, n):
    """random points of extent 1 around (1000, 1000, 1000): a tail lane taken for a zero point would win by a factor ~1700"""
    return CENTRE + rng.uniform(-0.5, 0.5, size=(n, 3))


def plant(pts, i, j):
    pts = pts.copy()
    pts[i] = CENTRE + (-5.0, 0.25, 0.0)
    pts[j] = CENTRE + (5.0, 0.0, -0.25)
    return pts


def tied_cloud(rng, n):
    """integer coordinates: the axis points (+-3, 0, 0), (0, +-3, 0), (0, 0, +-3) -- three pairs tied at 36 -- with two more
    copies of (3, 0, 0), scattered among points of {-1, 0, 1}^3 (no other pair reaches 36)"""
    pts = rng.integers(-1, 2, size=(n, 3)).astype(np.float64)
    special = [(3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, -3, 0), (0, 0, 3), (0, 0, -3), (3, 0, 0), (3, 0, 0)]
    where = rng.choice(n, size=min(n, len(special)), replace=False)
    pts[where] = np.array(special[:len(where)], np.float64)
    return pts


@pytest.mark.parametrize("n", tile_sizes())
def test_diameter_equals_the_restatement_bit_for_bit(n):
    from pyrapose_amd import ops
    T = ops.DIAMETER_TILE
    rng = np.random.default_rng(n)
    cloud = far_cloud(rng, n)
    d2, _ = assert_diameter(cloud, "n %d random" % n)
    assert d2[0] <= 3.0                                     # no zero point took part
    if n >= 2:
        assert_diameter(plant(cloud, 0, n - 1), "n %d planted first-last" % n, (0, n - 1))
    if n >= 8:
        t0 = 0 if n < T else (n // T - 1) * T              # the only tile, or the last full one
        i, j = t0 + 3, min(t0 + T, n) - 2
        assert i // T == j // T
        assert_diameter(plant(cloud, i, j), "n %d planted in diagonal tile" % n, (i, j))
    d2, _ = assert_diameter(tied_cloud(rng, n), "n %d tied" % n)
    assert d2[0] == (36.0 if n >= 2 else 0.0)


@pytest.mark.parametrize("cloud", ["random", "planted in the next chunk", "planted in the tail tile", "tied"])
def test_diameter_beyond_one_tile_per_workgroup(cloud):
    """Above ops.DIAMETER_MAX_CHUNKS tiles a workgroup sweeps a chunk of several j tiles in a loop (what every mesh of more than
    64 * 256 points takes): here 66 tiles, chunks of 2, a tail tile of one point.  Row 5's first chunk (tiles 4, 5) straddles
    the diagonal; the planted pairs start there and end in the next chunk and in the tail tile."""
    from pyrapose_amd import ops
    T, M = ops.DIAMETER_TILE, ops.DIAMETER_MAX_CHUNKS
    n = M * T + T + 1
    tiles = -(-n // T)
    assert tiles > M and -(-tiles // M) == 2 and n % T == 1
    rng = np.random.default_rng(n)
    if cloud == "tied":
        d2, _ = assert_diameter(tied_cloud(rng, n), "n %d tied" % n)
        assert d2[0] == 36.0
        return
    pts = far_cloud(rng, n)
    if cloud == "random":
        d2, _ = assert_diameter(pts, "n %d random" % n)
        assert d2[0] <= 3.0
    else:
        i = 5 * T + 3
        j = 6 * T + 7 if cloud == "planted in the next chunk" else n - 1
        assert (i // T) % 2 == 1 and (j // T) // 2 > (i // T) // 2
        assert_diameter(plant(pts, i, j), "n %d %s" % (n, cloud), (i, j))


def test_calc_pts_diameter_is_the_root_on_the_host_and_the_literal_loop():
    from pyrapose_amd.utils.model_info import calc_pts_diameter, pts_diameter
    rng = np.random.default_rng(300)
    pts = rng.normal(size=(300, 3)) * (40.0, 25.0, 60.0)
    d2, pair = MN.diameter_np(pts)
    d = calc_pts_diameter(pts)
    assert isinstance(d, float) and d == math.sqrt(d2[0]) and d == MN.calc_pts_diameter_np(pts)
    assert pts_diameter(pts, return_pair=True) == (d, (int(pair[0]), int(pair[1])))
    assert calc_pts_diameter(pts[:1]) == 0.0


def test_model_info_of_a_perturbed_sphere():
    from pyrapose_amd.utils.model_info import model_info, models_info, threeD_boxes
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations
    rng = np.random.default_rng(11)
    mesh = RN.sphere_mesh(50.0, 14, 20, scale=(1.0, 0.8, 1.3))
    mesh["pts"] = mesh["pts"] + rng.normal(scale=0.7, size=mesh["pts"].shape) + (2.0, -1.0, 4.0)
    pts = mesh["pts"]
    info = model_info(mesh)
    assert sorted(info) == ["diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z"]
    assert all(type(v) is float for v in info.values())
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    assert [info["min_" + a] for a in "xyz"] == list(lo) and [info["size_" + a] for a in "xyz"] == list(hi - lo)
    assert info["diameter"] == math.sqrt(MN.diameter_np(pts)[0][0])
    both = models_info({4: mesh, 2: pts[:100]})
    assert both[4] == info and both[2] == model_info(pts[:100]) and len(get_symmetry_transformations(both[2])) == 1
    assert np.array_equal(threeD_boxes(both), MN.three_boxes_np(both, 5))


def test_a_model_may_be_a_path_of_either_kind(tmp_path):
    from pyrapose_amd.utils.model_info import model_info, models_info
    pts = RN.box_mesh(2.0, 4.0, 6.0)["pts"]
    path = tmp_path / "obj_01.ply"
    path.write_text("ply\nformat ascii 1.0\nelement vertex 8\nproperty float x\nproperty float y\nproperty float z\nend_header\n" +
                    "".join("%r %r %r\n" % tuple(float(v) for v in p) for p in pts))
    want = model_info(pts)
    assert want["diameter"] == math.sqrt(56.0) and want["size_z"] == 6.0
    assert models_info({1: path, 2: str(path)}) == {1: want, 2: want}


def cloud_for_fps(rng, n):
    return rng.normal(size=(n, 3)) * (40.0, 25.0, 60.0) + (3.0, -2.0, 10.0)


@pytest.mark.parametrize("n", fps_sizes())
def test_farthest_points_equal_the_restatement(n):
    from pyrapose_amd.utils.model_info import farthest_points
    rng = np.random.default_rng(n)
    pts = cloud_for_fps(rng, n)
    for rule in ("min", "sum"):
        for k in sorted({1, 2, 8, min(n, 40)}):
            if rule == "min" and k > n:
                continue
            index, points = farthest_points(pts, k, rule)
            want = MN.farthest_np(pts, k, rule)
            print("n", n, "rule", rule, "k", k, "device", index, "restatement", want)
            assert index.dtype == np.int64 and np.array_equal(index, want), (n, rule, k)
            assert points.dtype == np.float64 and np.array_equal(points, pts[want])


@pytest.mark.parametrize("n", [1, 2, 37, 64])
def test_min_rule_with_k_equal_n_is_a_permutation(n):
    from pyrapose_amd.utils.model_info import farthest_points
    pts = cloud_for_fps(np.random.default_rng(100 + n), n)
    index, _ = farthest_points(pts, n, "min")
    assert np.array_equal(index, MN.farthest_np(pts, n, "min")) and sorted(index) == list(range(n))


def device_fps(pts_list, k, rule, min_dist=None, start=None):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pts_list])]).astype(np.int32)
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    out = ops.farthest_points(default_context(), dev(np.concatenate(pts_list), np.float64), offsets, k, rule, dev(min_dist, np.float64),
                              dev(start, np.int32))
    return out.cpu().numpy()


def test_a_batch_in_one_launch_equals_single_launches():
    from pyrapose_amd import ops
    W = ops.FPS_THREADS
    rng = np.random.default_rng(3)
    for sizes, rule, k in (((1, W + 1, 37), "min", 1), ((1, W + 1, 37), "sum", 8), ((5, W + 1, 37), "min", 5)):
        models = [cloud_for_fps(rng, n) for n in sizes]
        md = [MN.fps_min_dist_np(p) for p in models] if rule == "sum" else None
        got = device_fps(models, k, rule, md)
        assert got.dtype == np.int32 and got.shape == (3, k)
        for m, p in enumerate(models):
            single = device_fps([p], k, rule, None if md is None else md[m:m + 1])
            assert np.array_equal(got[m], single[0]) and np.array_equal(got[m], MN.farthest_np(p, k, rule)), (sizes, rule, m)


def test_every_candidate_ties_on_the_corners_of_a_cube():
    from pyrapose_amd.utils.model_info import farthest_points
    pts = RN.box_mesh(2.0, 2.0, 2.0)["pts"]
    index, _ = farthest_points(pts, 8, "min")
    want = MN.farthest_np(pts, 8, "min")
    assert np.array_equal(index, want) and sorted(index) == list(range(8))
    assert index[0] == 0 and index[1] == 7 and index[2] == 1    # equal norms: 0; its opposite corner; then six tied: the lowest


def test_given_start_and_start_by_norm_with_two_equal_norms():
    from pyrapose_amd.utils.model_info import farthest_points
    rng = np.random.default_rng(8)
    pts = rng.uniform(-4.0, 4.0, size=(50, 3))
    pts[31] = (0.0, 10.0, 0.0)
    pts[17] = (10.0, 0.0, 0.0)
    for rule in ("min", "sum"):
        index, _ = farthest_points(pts, 6, rule)
        assert index[0] == 17 and np.array_equal(index, MN.farthest_np(pts, 6, rule))
        index, _ = farthest_points(pts, 6, rule, start=40)
        assert index[0] == 40 and np.array_equal(index, MN.farthest_np(pts, 6, rule, start=40))


def test_sum_rule_with_every_point_blocked_picks_index_zero():
    from pyrapose_amd.utils.model_info import farthest_points
    pts = cloud_for_fps(np.random.default_rng(9), 1500)
    index, _ = farthest_points(pts, 6, "sum", min_dist=1.0e9)
    want = MN.farthest_np(pts, 6, "sum", min_dist=1.0e9)
    assert np.array_equal(index, want) and not index[1:].any() and index[0] != 0


def ring_cloud():
    """One far point c and 1500 points on a ring at almost the same distance from it (radius noise 1e-5), every coordinate a
    multiple of 2^-32 below 256: 40 significant bits, not float32 values.  Rounding c to float32 moves it by ~1e-6 sideways,
    far more than the gaps between the ring's distances to it."""
    rng = np.random.default_rng(0)
    phi = rng.uniform(0.0, 2.0 * np.pi, 1500)
    r = 80.0 + rng.uniform(-1.0e-5, 1.0e-5, 1500)
    pts = np.concatenate([np.stack([30.3 + r * np.cos(phi), 20.7 + r * np.sin(phi), np.full(1500, -50.0)], axis=1), [[30.3, 20.7, 150.1]]])
    return np.round(pts * 2.0 ** 32) / 2.0 ** 32


def test_sum_rule_rounds_the_chosen_point_to_float32():
    from pyrapose_amd.utils.model_info import farthest_points
    pts = ring_cloud()
    assert not np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    want, unrounded = MN.farthest_np(pts, 4, "sum"), MN.farthest_np(pts, 4, "sum", round32=False)
    # the restatement with and without the rounding differ on this cloud (checked here, on the CPU): a kernel that left the
    # rounding out could not pass
    assert want[0] == unrounded[0] == 1500 and not np.array_equal(want, unrounded)
    index, _ = farthest_points(pts, 4, "sum")
    print("device", index, "restatement", want, "without the rounding", unrounded)
    assert np.array_equal(index, want)


def test_control_points_of_two_models_in_one_launch():
    from pyrapose_amd.utils.model_info import control_points, farthest_points
    rng = np.random.default_rng(21)
    models = {9: {"pts": cloud_for_fps(rng, 1100)}, 2: cloud_for_fps(rng, 300)}
    for rule in ("sum", "min"):
        feats = control_points(models, 8, rule)
        assert list(feats) == [9, 2]
        for key, model in models.items():
            pts = model["pts"] if isinstance(model, dict) else model
            index, points = farthest_points(pts, 8, rule)
            assert np.array_equal(index, MN.farthest_np(pts, 8, rule))
            got = np.array(feats[key], np.float64)
            assert got.shape == (8, 3) and np.array_equal(got, points.astype(np.float32).astype(np.float64))
            assert np.array_equal(got.astype(np.float32).astype(np.float64), got)   # float32 values, as FPS.py lists them


# ---- argument errors: refused on the host side of the ABI, nothing launched ------------------------------------------------

def abi_fps(n_total, offsets, k, rule, workspace=True, pts_dtype=torch.float64):
    """pp_farthest_points_f64 called directly -> (status, message, the index buffer, filled with -7 beforehand)"""
    from pyrapose_amd._lib import lib
    from pyrapose_amd.runtime import default_context
    ctx = default_context()
    pts = torch.zeros((n_total, 3), dtype=pts_dtype, device="cuda")
    off = np.asarray(offsets, np.int32)
    off_dev = torch.from_numpy(off).cuda()
    M = off.size - 1
    md = torch.zeros((M,), dtype=torch.float64, device="cuda")
    nbytes = lib.pp_farthest_points_workspace_bytes(n_total)
    ws = torch.empty((max(1, nbytes),), dtype=torch.uint8, device="cuda")
    index = torch.full((M, k), -7, dtype=torch.int32, device="cuda")
    rc = lib.pp_farthest_points_f64(ctx.handle, M, n_total, C.c_void_p(pts.data_ptr()), off.ctypes.data_as(C.POINTER(C.c_int)),
                                    C.c_void_p(off_dev.data_ptr()), k, rule, C.c_void_p(md.data_ptr()), None,
                                    C.c_void_p(ws.data_ptr()) if workspace else None, nbytes, C.c_void_p(index.data_ptr()))
    msg = lib.pp_last_error_string(ctx.handle).decode() if rc else ""
    torch.cuda.synchronize()
    return rc, msg, index.cpu().numpy()


@pytest.mark.parametrize("what,offsets,k,rule,workspace,code,text", [
    ("k > n under rule 0", [0, 5, 9], 5, 0, True, -2, "rule 0 picks k = 5 distinct points, model 1 has 4"),
    ("empty model", [0, 5, 5, 9], 2, 1, True, -2, "model 1 is empty"),
    ("offsets that decrease", [0, 6, 4, 9], 2, 1, True, -1, "offsets must not decrease"),
    ("null workspace", [0, 5, 9], 2, 0, False, -1, "null argument"),
])
def test_farthest_points_argument_errors(what, offsets, k, rule, workspace, code, text):
    rc, msg, index = abi_fps(9, offsets, k, rule, workspace)
    assert rc == code and msg.startswith("pp_farthest_points_f64: ") and text in msg, (what, rc, msg)
    assert (index == -7).all()
    if workspace:   # and through the wrapper: ValueError with the code and that message
        with pytest.raises(ValueError, match=r"pp_farthest_points_f64 failed \(%d\).*%s" % (code, text.split(",")[0])):
            _ops_call(offsets, k, rule)
    rc, msg, index = abi_fps(9, [0, 5, 9], 2, 1)     # the same call with good arguments runs
    assert rc == 0 and (index == 0).all()


def _ops_call(offsets, k, rule):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    pts = torch.zeros((9, 3), dtype=torch.float64, device="cuda")
    md = torch.zeros((len(offsets) - 1,), dtype=torch.float64, device="cuda")
    return ops.farthest_points(default_context(), pts, offsets, k, "min" if rule == 0 else "sum", md)


def test_float32_points_and_bad_sizes_are_refused():
    from pyrapose_amd import ops
    from pyrapose_amd._lib import lib
    from pyrapose_amd.runtime import default_context
    ctx = default_context()
    pts32 = torch.zeros((9, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="farthest_points: pts must be a cuda float64 tensor"):
        ops.farthest_points(ctx, pts32, [0, 9], 2)
    with pytest.raises(ValueError, match="pts_diameter: pts must be a cuda float64 tensor"):
        ops.pts_diameter(ctx, pts32)
    with pytest.raises(ValueError, match=r"pp_pts_diameter_f64 failed \(-2\): pp_pts_diameter_f64: need 1\.\."):
        ops.pts_diameter(ctx, torch.zeros((0, 3), dtype=torch.float64, device="cuda"))
    assert lib.pp_pts_diameter_workspace_bytes(0) == 0 and lib.pp_pts_diameter_workspace_bytes((1 << 24) + 1) == 0
    pts = torch.zeros((9, 3), dtype=torch.float64, device="cuda")
    d2 = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    pair = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    nbytes = lib.pp_pts_diameter_workspace_bytes(9)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    for workspace, given, text in ((None, nbytes, "null argument"), (C.c_void_p(ws.data_ptr()), nbytes - 1, "workspace of")):
        rc = lib.pp_pts_diameter_f64(ctx.handle, 9, C.c_void_p(pts.data_ptr()), workspace, given, C.c_void_p(d2.data_ptr()),
                                     C.c_void_p(pair.data_ptr()))
        assert rc == -1 and text in lib.pp_last_error_string(ctx.handle).decode()
        torch.cuda.synchronize()
        assert float(d2.cpu()[0]) == -7.0 and (pair.cpu().numpy() == -7).all()
