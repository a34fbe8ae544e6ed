"""GPU: csrc/icp.hip stage by stage at its tile and batch edges (the inputs of tests/icp_cases.py) against the numpy restatement
(tests/icp_np.py) at the bars of tests/test_gpu_icp.py and, where cheap, against the independent references of
tests/icp_cases.py; every op runs twice and must give the same bits.  Then the host branches of utils.icp.refine_poses.
tests/test_icp_cases_cpu.py holds the preconditions that make the exact comparisons exact."""
import numpy as np
import pytest
import torch

from tests import icp_cases as C
from tests import icp_np as I
from tests.test_gpu_icp import K, add_err, scene, wedge_box_mesh
from tests.test_icp_cpu import rot

pytestmark = pytest.mark.gpu
MODES = ("point_to_plane", "point_to_point")


def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


def dev(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def twice(fn):
    """fn() -> tuple of cuda tensors / None; run twice, the same bits both times -> numpy arrays"""
    a, b = ([None if t is None else t.cpu().numpy() for t in fn()] for _ in range(2))
    for x, y in zip(a, b):
        assert (x is None and y is None) or (x.shape == y.shape and x.tobytes() == y.tobytes())
    return a


# ---- cloud ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", sorted(C.CLOUD_SHAPES))
def test_cloud_compaction_across_the_column_chunks(w):
    from pyrapose_amd import ops
    d = C.cloud_image(w)
    h = d.shape[0]
    dt = dev(d, torch.float32)
    for ds in (1.0, 0.001):
        for name, grid in C.cloud_masks(w).items():
            if grid is None:
                args, want = (), I.cloud_from_depth(d, *C.INTR, ds)
                ref, ref_offs = C.cloud_ref(d, *C.INTR, ds)
            else:
                mh, mw = grid.shape
                rows = np.arange(h, dtype=np.int32) if mh == h else ops.pil_nearest_index(mh, h)
                cols = np.arange(w, dtype=np.int32) if mw == w else ops.pil_nearest_index(mw, w)
                args = (dev(grid, torch.uint8), dev(rows, torch.int32), dev(cols, torch.int32))
                want = I.cloud_from_depth(d, *C.INTR, ds, grid, rows, cols)
                ref, ref_offs = C.cloud_ref(d, *C.INTR, ds, grid[rows][:, cols] != 0)
            pts, offs = twice(lambda: ops.cloud_from_depth(ctx(), dt, *C.INTR, ds, *args))
            assert pts.shape == want.shape and np.array_equal(pts, want), (w, ds, name)
            assert np.array_equal(pts, ref) and np.array_equal(offs, ref_offs), (w, ds, name)
            if name == "zero":
                assert pts.shape == (0, 3) and not offs.any()
        dense, = twice(lambda: (ops.cloud_from_depth(ctx(), dt, *C.INTR, ds, dense=True),))
        assert dense.shape == (h * w, 3)
        assert np.array_equal(dense, I.create_point_cloud(d, *C.INTR, ds), equal_nan=True)
        assert np.array_equal(dense, C.create_ref(d, *C.INTR, ds), equal_nan=True)


# ---- voxels --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(C.voxel_cases()))
def test_voxel_keys_and_means(name):
    from pyrapose_amd import ops
    p, v, nrm = C.voxel_cases()[name]
    want, want_n, _ = I.voxel_down_sample(p, v, nrm)
    ref, ref_n, _, _ = C.voxel_ref(p, v, nrm)
    got, got_n = twice(lambda: ops.voxel_down_sample(ctx(), dev(p), v, dev(nrm)))
    plain, none = twice(lambda: ops.voxel_down_sample(ctx(), dev(p), v))
    assert none is None and np.array_equal(plain, got)
    assert got.shape == want.shape == ref.shape                                  # the same voxels, in the dictionary's order
    assert np.abs(got - want).max() <= 1e-12 and np.abs(got - ref).max() <= 1e-12
    assert np.isfinite(got_n).all() and np.abs(got_n - want_n).max() <= 1e-12 and np.abs(got_n - ref_n).max() <= 1e-12
    if name == "one_big_voxel":
        assert np.array_equal(got, want)                                         # summed in original point order
    if name == "cancelling_normals":
        assert not got_n[0].any() and got_n[1].any()


def test_voxel_error_paths():
    from pyrapose_amd import ops
    p = C.voxel_cases()["n257"][0].copy()
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ops.voxel_down_sample(ctx(), dev(p), bad)
    p[100, 1] = np.nan
    with pytest.raises(ValueError):
        ops.voxel_down_sample(ctx(), dev(p), 5.0)
    with pytest.raises(ValueError):                                              # 3e6 voxels along x: past the 21 bits of a key
        ops.voxel_down_sample(ctx(), dev(np.array([[0.0, 0.0, 0.0], [3e6, 0.0, 0.0]])), 1.0)
    got = ops.voxel_down_sample(ctx(), dev(np.array([[0.0, 0.0, 0.0], [2e6, 0.0, 0.0]])), 1.0)[0]   # within them
    assert got.cpu().numpy().tolist() == [[0.0, 0.0, 0.0], [2e6, 0.0, 0.0]]


# ---- normals -------------------------------------------------------------------------------------------------------------

def normals(p, radius, max_nn):
    from pyrapose_amd import ops
    N, nb = twice(lambda: ops.estimate_normals(ctx(), dev(p), radius, max_nn, return_neighbors=True))
    assert nb.shape == (len(p), max_nn)
    lists = [row[row >= 0] for row in nb]
    assert all(np.array_equal(row[:len(j)], j) and (row[len(j):] == -1).all() for row, j in zip(nb, lists))   # -1 only as padding
    return N, lists


def same_lists(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n", C.NORMAL_SIZES)
def test_normals_on_a_jittered_surface(n):
    p = C.surface(n)
    N, nb = normals(p, 10.0, 10)
    wN, wnb = I.estimate_normals(p, 10.0, 10)
    ref_nb = C.neighbours_ref(p, 10.0, 10)
    assert same_lists(nb, wnb) and same_lists(nb, ref_nb)
    has = np.array([len(j) >= 3 for j in ref_nb])
    assert np.array_equal(np.abs(N).sum(1) > 0, has) and not N[~has].any()
    if has.any():
        assert C.angle(N[has], wN[has]).max() < 1e-9 and np.all(np.einsum("ij,ij->i", N[has], p[has]) <= 0)
        ref_N, W = C.normal_ref(p, ref_nb)
        gate = has & C.gap_ok(np.nan_to_num(W))
        assert (has & ~gate).sum() <= 0.05 * has.sum()
        assert C.angle(N[gate], ref_N[gate]).max() < 1e-9


@pytest.mark.parametrize("radius", C.LATTICE_RADII)
@pytest.mark.parametrize("max_nn", C.LATTICE_MAX_NN)
def test_normals_on_a_lattice_with_ties(radius, max_nn):
    g = C.lattice()
    N, nb = normals(g, radius, max_nn)
    assert same_lists(nb, C.neighbours_ref(g, radius, max_nn))                   # d2 == r r inside, ties to the lower index
    wN, wnb = I.estimate_normals(g, radius, max_nn)
    assert same_lists(nb, wnb)
    has = np.array([len(j) >= 3 for j in wnb])
    assert np.array_equal(np.abs(N).sum(1) > 0, has) and (max_nn >= 3 or not N.any())
    if has.any():                                                                 # degenerate eigenvalues: the restatement only
        assert C.angle(N[has], wN[has]).max() < 1e-9


def test_normals_on_degenerate_neighbourhoods_and_bad_arguments():
    from pyrapose_amd import ops
    for k in (0, 33, -1):
        with pytest.raises(ValueError):
            ops.estimate_normals(ctx(), dev(C.lattice()), 2.0, k, return_neighbors=True)
    for r in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError):
            ops.estimate_normals(ctx(), dev(C.lattice()), r, 10)
    N, nb = normals(C.isolated_points(), 10.0, 10)
    assert not N.any() and sorted(len(j) for j in nb) == [1, 1, 1, 2, 2]
    for p, want in C.coplanar_patches():
        N, _ = normals(p, 10.0, 10)
        assert np.abs(N - want).max() < 1e-12 and np.all(np.einsum("ij,ij->i", N, p) < 0)
        assert C.angle(N, I.estimate_normals(p, 10.0, 10)[0]).max() < 1e-9
    p, line = C.collinear_points()
    N, nb = normals(p, 7.0, 10)
    assert [len(j) for j in nb] == [3, 3, 3, 1, 1] and not N[3:].any() and np.isfinite(N).all()
    assert np.abs(np.linalg.norm(N[:3], axis=1) - 1.0).max() < 1e-12 and np.abs(N[:3] @ line).max() < 1e-9


# ---- ICP -----------------------------------------------------------------------------------------------------------------

def run_icp(problems, max_d, mode, max_iteration, **kw):
    """ops.icp on a packed batch, twice -> one dict per problem (R, t, fitness, inlier_rmse, iterations, status, corr)"""
    from pyrapose_amd import ops
    so = np.concatenate([[0], np.cumsum([len(p["source"]) for p in problems])]).astype(np.int32)
    to = np.concatenate([[0], np.cumsum([len(p["target"]) for p in problems])]).astype(np.int32)
    src = dev(np.concatenate([np.asarray(p["source"], np.float64).reshape(-1, 3) for p in problems]))
    tgt = dev(np.concatenate([np.asarray(p["target"], np.float64).reshape(-1, 3) for p in problems]))
    tn = dev(np.concatenate([np.asarray(p["target_normals"], np.float64).reshape(-1, 3) for p in problems])) if mode == "point_to_plane" else None
    init = dev(np.stack([p["init"] for p in problems]))
    R, t, fit, rmse, iters, status, corr = twice(lambda: ops.icp(ctx(), dev(so, torch.int32), dev(to, torch.int32), src, tgt, init, max_d,
                                                                 max_iteration, mode=mode, tgt_normals=tn, **kw))
    return [dict(R=R[p], t=t[p], fitness=float(fit[p]), inlier_rmse=float(rmse[p]), iterations=int(iters[p]), status=int(status[p]),
                 corr=corr[so[p]:so[p + 1]]) for p in range(len(problems))]


def restated(pr, max_d, mode, max_iteration):
    return I.registration_icp(pr["source"], pr["target"], pr["init"], max_d, max_iteration, estimation=mode, tgt_normals=pr["target_normals"])


def same_bits(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("R", "t", "fitness", "inlier_rmse", "iterations", "status", "corr"))


def check_against(g, w, rmse=True):
    """the bars of tests/test_gpu_icp.py (rmse=False: an inlier_rmse that is rounding noise about zero is not compared)"""
    assert g["status"] == w["status"] and g["iterations"] == w["iterations"] and g["fitness"] == w["fitness"]
    assert np.array_equal(g["corr"], w["corr"])
    assert np.abs(g["R"] - w["R"]).max() < 1e-9 and np.abs(g["t"] - w["t"]).max() < 1e-6
    assert not rmse or abs(g["inlier_rmse"] - w["inlier_rmse"]) <= 1e-12 * w["inlier_rmse"]


def check_at_init(g, pr, max_d, mode):
    w = restated(pr, max_d, mode, 0)
    check_against(g, w)
    T = np.asarray(pr["init"], np.float64)
    assert g["iterations"] == 0 and np.array_equal(g["R"], T[:3, :3]) and np.array_equal(g["t"], T[:3, 3])
    ref = C.corr_ref(pr["source"], pr["target"], pr["init"], max_d, pr["target_normals"] if mode == "point_to_plane" else None)
    assert np.array_equal(g["corr"], ref["corr"]) and g["fitness"] == ref["fitness"]
    assert abs(g["inlier_rmse"] - ref["inlier_rmse"]) <= 1e-12 * ref["inlier_rmse"]


@pytest.mark.parametrize("mode", MODES)
def test_correspondences_of_a_ragged_batch(mode):
    batch = list(C.ragged_batch())
    got = run_icp(batch, C.RAGGED_MAX_D, mode, 0)
    for g, pr in zip(got, batch):
        check_at_init(g, pr, C.RAGGED_MAX_D, mode)
        assert g["status"] == I.OK
    rev = run_icp(batch[::-1], C.RAGGED_MAX_D, mode, 0)[::-1]                     # another tile layout, the same answers
    assert all(same_bits(a, b) for a, b in zip(got, rev))


@pytest.mark.parametrize("mode", MODES)
def test_correspondence_ties_limits_and_missing_normals(mode):
    cases = C.explicit_problems()
    for max_d in sorted(set(c[1] for c in cases.values())):                       # one batch per distance limit
        names = [n for n in cases if cases[n][1] == max_d]
        got = run_icp([cases[n][0] for n in names], max_d, mode, 0)
        for n, g in zip(names, got):
            assert g["corr"].tolist() == cases[n][2][mode], n
            check_at_init(g, cases[n][0], max_d, mode)
    g, = run_icp([cases["no_normal_at_all"][0]], 10.0, mode, 30)
    assert g["status"] == I.TOO_FEW and g["iterations"] == 0 and np.array_equal(g["R"], np.eye(3)) and not g["t"].any()
    if mode == "point_to_plane":
        assert g["fitness"] == 0.0 and g["inlier_rmse"] == 0.0 and (g["corr"] == -1).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("max_iteration", [0, 3])
def test_sixty_five_problems_cross_the_per_problem_block(mode, max_iteration):
    batch = list(C.tiny_batch())
    got = run_icp(batch, C.RAGGED_MAX_D, mode, max_iteration)
    assert len(got) == 65
    for p, (g, pr) in enumerate(zip(got, batch)):
        if p in (C.TINY_NO_SOURCE, C.TINY_NO_TARGET):
            assert g["status"] == I.TOO_FEW and g["iterations"] == 0 and g["fitness"] == 0.0 and g["inlier_rmse"] == 0.0
            assert np.array_equal(g["R"], pr["init"][:3, :3]) and np.array_equal(g["t"], pr["init"][:3, 3]) and (g["corr"] == -1).all()
            continue
        assert same_bits(g, run_icp([pr], C.RAGGED_MAX_D, mode, max_iteration)[0]), p
        if max_iteration == 0:
            check_at_init(g, pr, C.RAGGED_MAX_D, mode)
    assert max_iteration == 0 or sum(g["iterations"] > 0 for g in got) > 32
    assert max_iteration == 0 or got[64]["iterations"] > 0


@pytest.mark.parametrize("mode", MODES)
def test_one_update_against_the_restatement_and_svd_or_solve(mode):
    batch = list(C.step_problems())
    for g, pr in zip(run_icp(batch, C.STEP_MAX_D, mode, 1), batch):
        check_against(g, restated(pr, C.STEP_MAX_D, mode, 1))
        R, t = C.one_update_ref(pr, C.STEP_MAX_D, mode)
        assert g["iterations"] == 1 and g["status"] == I.OK
        assert np.abs(g["R"] - R).max() < 1e-9 and np.abs(g["t"] - t).max() < 1e-6


def test_exact_correspondences_recover_the_transform():
    cases = C.exact_problems()
    got = run_icp([c[0] for c in cases.values()], 50.0, "point_to_point", 30)
    for g, (name, (pr, R, t)) in zip(got, cases.items()):
        assert g["status"] == I.OK and g["fitness"] == 1.0 and 1 <= g["iterations"] <= 3, name
        assert np.abs(g["R"] - R).max() < 1e-9 and np.abs(g["t"] - t).max() < 1e-6 and g["inlier_rmse"] < 1e-9, name
        check_against(g, restated(pr, 50.0, "point_to_point", 30), rmse=False)


def test_singular_normal_equations_and_the_correspondence_thresholds():
    pr = C.singular_plane_problem()
    g, = run_icp([pr], 10.0, "point_to_plane", 30)
    w = restated(pr, 10.0, "point_to_plane", 30)
    assert g["status"] == w["status"] == I.SINGULAR and g["iterations"] == w["iterations"] == 0 and g["fitness"] == 1.0
    assert g["R"].tobytes() == pr["init"][:3, :3].tobytes() and g["t"].tobytes() == pr["init"][:3, 3].tobytes()
    from pyrapose_amd.utils import icp
    r = icp.registration_icp(pr["source"], pr["target"], 10.0, pr["init"], target_normals=pr["target_normals"])
    assert r.status == "singular" and np.array_equal(r.transformation, pr["init"])
    for mode, k in (("point_to_plane", 5), ("point_to_plane", 6), ("point_to_point", 2), ("point_to_point", 3)):
        pr = C.threshold_problem(k)
        g, = run_icp([pr], 5.0, mode, 1)
        check_against(g, restated(pr, 5.0, mode, 1))
        if k in (5, 2):
            assert (g["corr"] >= 0).sum() == k and g["fitness"] == k / 10.0
            assert g["status"] == I.TOO_FEW and g["iterations"] == 0 and np.array_equal(g["R"], np.eye(3)) and not g["t"].any()
        else:
            assert g["status"] == I.OK and g["iterations"] == 1 and not np.array_equal(g["R"], np.eye(3))


# ---- refine_poses: host branches ------------------------------------------------------------------------------------------

def start(Rg, tg, seed):
    """a guess 3 degrees and 6 mm off (R, t in metres)"""
    rng = np.random.default_rng(seed)
    dt = rng.normal(size=3)
    return rot(rng.normal(size=3), 3.0) @ Rg, (tg + 6.0 * dt / np.linalg.norm(dt)) * 0.001


def test_z_gate_fallback_moves_the_model_onto_the_scene():
    from pyrapose_amd.utils import icp
    model = wedge_box_mesh()
    Rg, tg = rot([1.0, 1.0, 0.0], 40.0), np.array([20.0, -10.0, 700.0])
    depth, mask = scene(model, Rg, tg)
    depth = np.where(depth > tg[2] + 150.0, 0, depth).astype(np.uint16)           # the object alone: nothing 200 mm deeper
    R0, t0 = start(Rg, tg + np.array([0.0, 0.0, 200.0]), 1)
    a0 = add_err(R0, t0, Rg, tg * 0.001, model["pts"])
    assert a0 > 0.19
    R1, t1, info = icp.refine_pose(R0, t0, depth, mask, K, model, z_gate=75.0)
    a1 = add_err(R1, t1, Rg, tg * 0.001, model["pts"])
    assert info["refined"] and info["fitness"] > 0 and a1 < 0.5 * a0, (a0, a1, info)
    R2, t2, far = icp.refine_pose(R0, t0, depth, mask, K, model, z_gate=1000.0)   # the gate keeps everything: no fallback
    assert not far["refined"] and np.array_equal(R2, R0) and np.array_equal(t2, t0) and far["fitness"] == 0.0
    assert not np.array_equal(t1, t2)


def test_min_mask_pixels_is_an_exclusive_limit():
    from pyrapose_amd.utils import icp
    model = wedge_box_mesh()
    Rg, tg = rot([1.0, 1.0, 0.0], 40.0), np.array([0.0, 0.0, 700.0])
    depth, mask = scene(model, Rg, tg)
    R0, t0 = start(Rg, tg, 2)
    cells = np.nonzero(mask)[0]
    limit = 64 * (len(cells) - 1)                                                 # a cell of the 60 x 80 grid is 8 x 8 pixels
    fewer = mask.copy()
    fewer[cells[0]] = 0.0
    R1, t1, info = icp.refine_pose(R0, t0, depth, fewer, K, model, min_mask_pixels=limit)      # exactly at the limit: skipped
    assert not info["refined"] and np.array_equal(R1, R0) and np.array_equal(t1, t0) and info["iterations"] == 0
    R1, t1, info = icp.refine_pose(R0, t0, depth, mask, K, model, min_mask_pixels=limit)       # one cell more
    assert info["refined"] and info["iterations"] > 0 and info["fitness"] > 0.5
    assert icp.refine_pose(R0, t0, depth, fewer, K, model, min_mask_pixels=limit - 1)[2]["refined"]


def test_box_restricts_the_mask_to_one_instance():
    from pyrapose_amd.utils import icp
    model = wedge_box_mesh()
    pts = model["pts"]
    poses = [(rot([1.0, 1.0, 0.0], 40.0), np.array([-150.0, -20.0, 700.0])), (rot([0.2, 1.0, 0.5], 70.0), np.array([150.0, 20.0, 700.0]))]
    depths, masks, boxes, dets = [], [], [], []
    for k, (Rg, tg) in enumerate(poses):
        d, m = scene(model, Rg, tg)
        ys, xs = np.nonzero(d < tg[2] + 150.0)
        depths.append(d)
        masks.append(m)
        boxes.append([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1])
        R0, t0 = start(Rg, tg, 10 + k)
        dets.append(dict(cls=0, R=R0, t=t0))
    assert boxes[0][2] + 100 < boxes[1][0]                                        # well apart
    depth, mask = np.minimum(depths[0], depths[1]), np.maximum(masks[0], masks[1]).reshape(-1, 1)

    def good(out):
        res = []
        for (Rg, tg), det, o in zip(poses, dets, out):
            a0, a1 = add_err(det["R"], det["t"], Rg, tg * 0.001, pts), add_err(o["R"], o["t"], Rg, tg * 0.001, pts)
            res.append(bool(o["refined"] and a1 < 0.5 * a0))
        return res

    boxed = icp.refine_poses([dict(d, box=b) for d, b in zip(dets, boxes)], depth, mask, K, [model])
    assert good(boxed) == [True, True], boxed
    assert all("box" in o for o in boxed)
    assert not all(good(icp.refine_poses(dets, depth, mask, K, [model])))          # one channel, two objects: the gate sees both
    with pytest.raises(ValueError):
        icp.refine_poses([dict(dets[0], box=boxes[0])], depth, mask, K, [model], box_margin=-1)
    for bad in ([0.0, 0.0, np.nan, 10.0], [0.0, 0.0, np.inf, 10.0], [0.0, 0.0, 10.0]):
        with pytest.raises(ValueError):
            icp.refine_poses([dict(dets[0], box=bad)], depth, mask, K, [model])
