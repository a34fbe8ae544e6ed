"""CPU (no GPU): the numpy restatement of csrc/icp.hip (tests/icp_np.py) against the independent float64 references of
tests/icp_cases.py on every case family of tests/test_gpu_icp_stages.py, and the preconditions of those inputs (so that an exact
comparison on the GPU is exact by construction and not by luck)."""
import numpy as np
import pytest

from tests import icp_cases as C
from tests import icp_np as I

MODES = ("point_to_plane", "point_to_point")


def restated(pr, max_d, mode, max_iteration, **kw):
    return I.registration_icp(pr["source"], pr["target"], pr["init"], max_d, max_iteration, estimation=mode,
                              tgt_normals=pr["target_normals"], **kw)


def index_maps(grid, h, w):
    from pyrapose_amd import ops
    mh, mw = grid.shape
    rows = np.arange(h, dtype=np.int32) if mh == h else ops.pil_nearest_index(mh, h)
    cols = np.arange(w, dtype=np.int32) if mw == w else ops.pil_nearest_index(mw, w)
    return rows, cols


@pytest.mark.parametrize("w", sorted(C.CLOUD_SHAPES))
def test_cloud_restatement_equals_boolean_indexing(w):
    d = C.cloud_image(w)
    h = d.shape[0]
    z = d.astype(np.float64)
    ok = np.isfinite(z) & (z != 0)
    last = ((w - 1) // 256) * 256
    # the input's own design: an all-valid row, an all-invalid one with every invalid value, one valid only in its last chunk
    assert ok[0].all() and not ok[1].any() and ok[2].any() and not ok[2, :max(last, w - 3)].any() and (d[ok] < 0).any()
    if w >= len(C.INVALID):
        bad = d[1]
        assert (bad == 0).any() and np.signbit(bad[bad == 0]).any() and np.isnan(bad).any() and np.isposinf(bad).any() and np.isneginf(bad).any()
    if h > 3 and w > 1:
        assert 0.3 < ok[3:].mean() < 0.7
    for ds in (1.0, 0.001):
        want_all, offs_all = C.cloud_ref(d, *C.INTR, ds)
        assert len(want_all) == ok.sum() and (want_all[:, 2] < 0).any()
        for name, grid in C.cloud_masks(w).items():
            if grid is None:
                got, (want, offs) = I.cloud_from_depth(d, *C.INTR, ds), (want_all, offs_all)
            else:
                rows, cols = index_maps(grid, h, w)
                got = I.cloud_from_depth(d, *C.INTR, ds, grid, rows, cols)
                want, offs = C.cloud_ref(d, *C.INTR, ds, grid[rows][:, cols] != 0)
            assert got.dtype == np.float64 and np.array_equal(got, want), (w, ds, name)
            assert offs[0] == 0 and offs[-1] == len(want) and len(offs) == h + 1
            if name == "zero":
                assert len(want) == 0 and not offs.any()
            elif name != "none":
                assert 0 < len(want) and (w == 1 or len(want) < len(want_all))
        dense, ref = I.create_point_cloud(d, *C.INTR, ds), C.create_ref(d, *C.INTR, ds)
        assert np.array_equal(dense, ref, equal_nan=True)
        zz = (z * ds).reshape(-1)
        assert np.array_equal(np.isnan(ref).all(1), (zz == 0) | np.isnan(zz))      # only z == 0 and NaN depth give a NaN row
        assert np.array_equal(ref[np.isinf(zz), 2], zz[np.isinf(zz)])              # +-inf depth propagates


def test_voxel_restatement_equals_the_dictionary():
    cases = C.voxel_cases()
    for name, (p, v, nrm) in cases.items():
        n = len(p)
        got, got_n, keys = I.voxel_down_sample(p, v, nrm)
        want, want_n, ix, members = C.voxel_ref(p, v, nrm)
        assert np.array_equal(keys, (ix[:, 0] << 42) | (ix[:, 1] << 21) | ix[:, 2]), name          # membership and order
        assert np.array_equal(got, want), name                                                     # the same sequential sums
        assert np.array_equal(np.sort(np.concatenate(members)), np.arange(n))
        for k, m in enumerate(members):
            np.testing.assert_allclose(want[k], p[m].mean(0), rtol=1e-12, atol=0, err_msg=name)
        np.testing.assert_allclose(got_n, want_n, rtol=1e-12, atol=0, err_msg=name)
        assert np.isfinite(got_n).all() and np.array_equal(I.voxel_down_sample(p, v)[0], got)
        if name.startswith("n"):
            assert np.array_equal(np.argmin(p, 0), [n - 1] * 3) and (n == 1 or ((p < 0).any() and (p > 0).any()))
    lat, v, _ = cases["dyadic_faces"]
    on_face = ((lat - (lat.min(0) - v / 2)) / v) % 1.0 == 0
    assert on_face.any(0).all() and (~on_face).any(0).all() and (lat < 0).any() and (lat > 0).any()
    assert len(C.voxel_ref(*cases["one_voxel"][:2])[0]) == 1
    assert len(C.voxel_ref(*cases["own_voxels_257"][:2])[0]) == 257
    sizes = sorted(len(m) for m in C.voxel_ref(*cases["one_big_voxel"][:2])[3])
    assert sizes == [1] * 21 + [300]
    p, v, nrm = cases["cancelling_normals"]
    _, want_n, _, members = C.voxel_ref(p, v, nrm)
    assert members[0] == [0, 1, 4, 5] and not want_n[0].any() and abs(np.linalg.norm(want_n[1]) - 1.0) < 1e-15


def test_neighbour_lists_and_normals_equal_lexsort_and_eigh():
    """Measured on these inputs: the largest angle between the restatement's 6-sweep Jacobi normal and np.linalg.eigh's under
    the gap gate is 5.7e-16 rad; the gate excludes no point of any size (cap 5 %)."""
    worst, excluded = 0.0, 0
    for n in C.NORMAL_SIZES:
        p = C.surface(n)
        N, nb = I.estimate_normals(p, 10.0, 10)
        ref_nb = C.neighbours_ref(p, 10.0, 10)
        assert all(np.array_equal(a, b) for a, b in zip(nb, ref_nb)), n
        ref_N, W = C.normal_ref(p, ref_nb)
        has = np.array([len(j) >= 3 for j in ref_nb])
        assert np.array_equal(np.abs(N).sum(1) > 0, has) and (n < 3) == (not has.any())
        if not has.any():
            continue
        assert n < 63 or has.mean() > 0.9
        gate = C.gap_ok(W[has])
        assert (~gate).sum() <= 0.05 * has.sum(), (n, (~gate).sum())             # the reference alone stays within the cap
        ang = C.angle(N[has][gate], ref_N[has][gate])
        worst, excluded = max(worst, ang.max()), excluded + int((~gate).sum())
        assert ang.max() < 1e-9 and np.all(np.einsum("ij,ij->i", N[has], p[has]) <= 0)
    print("normals: largest angle to eigh %.3g rad, %d points excluded by the gate" % (worst, excluded))


def test_lattice_neighbour_lists_with_ties_and_overflow():
    g = C.lattice()
    d = g[:, None] - g[None]
    d2 = (d * d).sum(-1)
    assert np.array_equal(d2, np.round(d2))                                       # exact integers: ties are bit-equal
    for r in C.LATTICE_RADII:
        assert (d2 == r * r).any()                                                # a neighbour exactly on the radius
        inside = (d2 <= r * r).sum(1)
        for k in C.LATTICE_MAX_NN:
            N, nb = I.estimate_normals(g, r, k)
            ref = C.neighbours_ref(g, r, k)
            assert all(np.array_equal(a, b) for a, b in zip(nb, ref)), (r, k)
            assert np.array_equal([len(j) for j in nb], np.minimum(inside, k))
            if k < 3:
                assert not N.any()
            else:
                assert np.array_equal(np.abs(N).sum(1) > 0, np.minimum(inside, k) >= 3)
            # a list that overflows drops a neighbour as far away as one it keeps: the lower index stays
            cut = [i for i in range(len(g)) if inside[i] > k and np.sort(d2[i])[k - 1] == np.sort(d2[i])[k]]
            assert cut or k == 1 or not (inside > k).any(), (r, k)
    assert ((d2 <= 4.0).sum(1) == 33).any()                                       # one more than the kernel's 32 slots


def test_degenerate_neighbourhoods():
    N, nb = I.estimate_normals(C.isolated_points(), 10.0, 10)
    assert not N.any() and max(len(j) for j in nb) == 2
    for p, want in C.coplanar_patches():
        N, _ = I.estimate_normals(p, 10.0, 10)
        assert np.abs(N - want).max() < 1e-12 and np.all(N @ want > 0) and np.all(np.einsum("ij,ij->i", N, p) < 0)
    p, line = C.collinear_points()
    N, nb = I.estimate_normals(p, 7.0, 10)
    assert [len(j) for j in nb] == [3, 3, 3, 1, 1] and not N[3:].any()
    assert np.isfinite(N).all() and np.abs(np.linalg.norm(N[:3], axis=1) - 1.0).max() < 1e-12 and np.abs(N[:3] @ line).max() < 1e-9


def check_at_init(pr, max_d, mode, gap=True):
    """max_iteration = 0: the restatement reports corr / fitness / inlier_rmse at init, no update"""
    plane = mode == "point_to_plane"
    got = restated(pr, max_d, mode, 0)
    ref = C.corr_ref(pr["source"], pr["target"], pr["init"], max_d, pr["target_normals"] if plane else None)
    T = np.asarray(pr["init"], np.float64)
    assert got["iterations"] == 0 and np.array_equal(got["R"], T[:3, :3]) and np.array_equal(got["t"], T[:3, 3])
    if len(pr["source"]) == 0 or len(pr["target"]) == 0:
        assert got["status"] == I.TOO_FEW and got["fitness"] == 0.0 and got["inlier_rmse"] == 0.0 and not (got["corr"] >= 0).any()
        return ref
    if gap:
        # the nearest target is ahead of the second by more than 1e-9 relative, and no distance sits on the limit
        two = np.isfinite(ref["second"])
        assert np.all(ref["second"][two] - ref["best"][two] > 1e-9 * ref["second"][two])
        fin = np.isfinite(ref["best"])
        assert np.all(np.abs(ref["best"][fin] - max_d * max_d) > 1e-9 * max_d * max_d)
    assert np.array_equal(got["corr"], ref["corr"]) and got["fitness"] == ref["fitness"] and got["status"] == I.OK
    assert abs(got["inlier_rmse"] - ref["inlier_rmse"]) <= 1e-12 * ref["inlier_rmse"]
    return ref


@pytest.mark.parametrize("mode", MODES)
def test_correspondences_at_init_equal_all_pairs_argmin(mode):
    batch = C.ragged_batch()
    assert [len(p["source"]) for p in batch] == list(C.RAGGED_SRC) and set(len(p["target"]) for p in batch) == set(C.RAGGED_TGT)
    fit = [check_at_init(pr, C.RAGGED_MAX_D, mode)["fitness"] for pr in batch]
    assert 0.2 < np.mean(fit[1:]) < 0.9                                            # the limit cuts through the distances
    if mode == "point_to_plane":
        assert all((~pr["target_normals"].any(1)).any() for pr in batch if len(pr["target"]) > 100)   # targets without a normal
        differ = sum(not np.array_equal(C.corr_ref(p["source"], p["target"], p["init"], C.RAGGED_MAX_D)["corr"],
                                        C.corr_ref(p["source"], p["target"], p["init"], C.RAGGED_MAX_D, p["target_normals"])["corr"])
                     for p in batch)
        assert differ >= 4                                                          # and they change the answer
    for pr in C.tiny_batch():
        check_at_init(pr, C.RAGGED_MAX_D, mode)
    tiny = C.tiny_batch()
    assert len(tiny) == 65 and len(tiny[C.TINY_NO_SOURCE]["source"]) == 0 and len(tiny[C.TINY_NO_TARGET]["target"]) == 0


@pytest.mark.parametrize("mode", MODES)
def test_explicit_ties_limits_and_missing_normals(mode):
    plane = mode == "point_to_plane"
    cases = C.explicit_problems()
    for name, (pr, max_d, want) in cases.items():
        ref = check_at_init(pr, max_d, mode, gap=False)
        assert ref["corr"].tolist() == want[mode], name
    for name in ("duplicate_targets", "equidistant_targets"):
        pr, max_d, _ = cases[name]
        ref = C.corr_ref(pr["source"], pr["target"], pr["init"], max_d)
        assert np.array_equal(ref["best"], ref["second"]), name                    # the ties are bit-equal
    pr, max_d, _ = cases["at_max_distance"]
    assert C.corr_ref(pr["source"], pr["target"], pr["init"], max_d)["best"][0] == max_d * max_d
    got = restated(cases["no_normal_at_all"][0], 10.0, mode, 30)
    assert got["status"] == I.TOO_FEW and got["iterations"] == 0 and got["fitness"] == (0.0 if plane else 1.0)   # two source points


@pytest.mark.parametrize("mode", MODES)
def test_one_update_equals_svd_and_solve(mode):
    """Measured on these four problems, restatement against reference: point_to_point max |dR| 5.3e-15, max |dt| 6.8e-13 mm
    (Horn's quaternion by 10 Jacobi sweeps against Kabsch by SVD); point_to_plane max |dR| 8.0e-14, max |dt| 2.7e-12 mm (LDL^T
    against np.linalg.solve).  Both are more than 100x below the bars 1e-9 / 1e-6 mm."""
    dR = dt = 0.0
    for pr in C.step_problems():
        got = restated(pr, C.STEP_MAX_D, mode, 1)
        R, t = C.one_update_ref(pr, C.STEP_MAX_D, mode)
        assert got["iterations"] == 1 and got["status"] == I.OK and got["fitness"] > 0.5
        assert not np.array_equal(got["R"], pr["init"][:3, :3])
        dR, dt = max(dR, np.abs(got["R"] - R).max()), max(dt, np.abs(got["t"] - t).max())
    print("%s: max |dR| %.3g, max |dt| %.3g mm" % (mode, dR, dt))
    assert dR < 1e-9 and dt < 1e-6


def test_exact_singular_and_threshold_problems():
    for name, (pr, R, t) in C.exact_problems().items():
        ref = C.corr_ref(pr["source"], pr["target"], pr["init"], 50.0)
        assert np.array_equal(ref["corr"], np.arange(len(pr["source"]))), name     # every point starts with its partner
        got = restated(pr, 50.0, "point_to_point", 30)
        assert got["status"] == I.OK and got["fitness"] == 1.0 and np.abs(got["R"] - R).max() < 1e-9 and np.abs(got["t"] - t).max() < 1e-6
        if name == "coplanar":
            s = pr["source"] - pr["source"].mean(0)
            assert np.linalg.matrix_rank(s.T @ (pr["target"] - pr["target"].mean(0))) == 2
    pr = C.singular_plane_problem()
    got = restated(pr, 10.0, "point_to_plane", 30)
    assert got["status"] == I.SINGULAR and got["iterations"] == 0 and got["fitness"] == 1.0
    assert np.array_equal(got["R"], pr["init"][:3, :3]) and np.array_equal(got["t"], pr["init"][:3, 3])
    for mode, k in (("point_to_plane", 5), ("point_to_plane", 6), ("point_to_point", 2), ("point_to_point", 3)):
        pr = C.threshold_problem(k)
        ref = C.corr_ref(pr["source"], pr["target"], pr["init"], 5.0, pr["target_normals"] if mode == "point_to_plane" else None)
        assert (ref["corr"] >= 0).sum() == k and ref["corr"][:k].tolist() == list(range(1, k + 1))
        got = restated(pr, 5.0, mode, 1)
        if k in (5, 2):
            assert got["status"] == I.TOO_FEW and got["iterations"] == 0 and np.array_equal(got["R"], np.eye(3)) and got["fitness"] == k / 10.0
        else:
            assert got["status"] == I.OK and got["iterations"] == 1 and not np.array_equal(got["R"], np.eye(3))
