"""GPU: the ICP refinement path (csrc/icp.hip, utils.icp) against its numpy restatement (tests/icp_np.py), its determinism,
refinement on rendered RGB-D scenes, edge cases and the opt-in hook of the evaluation loop."""
import math

import numpy as np
import pytest
import torch

from tests import icp_np as I
from tests import render_np as RN
from tests.test_icp_cpu import asymmetric_cloud, rot

pytestmark = pytest.mark.gpu
K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def test_back_projection_matches_the_restatement():
    from pyrapose_amd import ops
    from pyrapose_amd.utils import icp
    rng = np.random.default_rng(0)
    d = rng.uniform(400, 1200, (48, 64)).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.2] = 0.0
    d[rng.uniform(size=d.shape) < 0.05] = np.nan
    got = icp.create_point_cloud(d, 572.4, 573.5, 31.2, 23.9, 1.0)
    assert got.shape == (48 * 64, 3) and np.array_equal(got, I.create_point_cloud(d, 572.4, 573.5, 31.2, 23.9, 1.0), equal_nan=True)
    assert np.array_equal(np.isnan(got).any(1), (d.reshape(-1) == 0) | np.isnan(d.reshape(-1)))
    Kc = np.array([[572.4, 0, 31.2], [0, 573.5, 23.9], [0, 0, 1.0]])
    full = icp.cloud_from_depth(d, Kc, ds=0.5).cpu().numpy()
    assert np.array_equal(full, I.cloud_from_depth(d, 572.4, 573.5, 31.2, 23.9, 0.5))
    grid = (rng.uniform(size=(6, 8)) < 0.5).astype(np.uint8)
    rows, cols = ops.pil_nearest_index(6, 48), ops.pil_nearest_index(8, 64)
    masked = icp.cloud_from_depth(d, Kc, mask=grid).cpu().numpy()
    want = I.cloud_from_depth(d, 572.4, 573.5, 31.2, 23.9, 1.0, grid, rows, cols)
    assert len(want) > 100 and np.array_equal(masked, want)
    assert icp.cloud_from_depth(d, Kc, mask=np.zeros((6, 8), np.uint8)).shape == (0, 3)


@pytest.mark.parametrize("h", [1023, 1024, 1025, 2049])  # below, at and past one 1024-row pass of the row scan; a third pass
def test_row_offsets_across_the_scan_width(h):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    rng = np.random.default_rng(h)
    w = 8
    d = rng.uniform(400, 1200, (h, w)).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.5] = 0.0
    dev = torch.from_numpy(d).cuda()
    pts, offs = ops.cloud_from_depth(default_context(), dev, 572.4, 573.5, 3.7, h / 2.0, dense=False)
    assert np.array_equal(offs.cpu().numpy(), np.concatenate([[0], np.cumsum((d != 0).sum(1))]))
    dense = ops.cloud_from_depth(default_context(), dev, 572.4, 573.5, 3.7, h / 2.0, dense=True).cpu().numpy()
    assert np.array_equal(pts.cpu().numpy(), dense[np.isfinite(dense).all(1)])


def surface_cloud(seed, n=900):
    rng = np.random.default_rng(seed)
    p, _ = asymmetric_cloud(n, seed)
    p = p @ rot(rng.normal(size=3), rng.uniform(0, 180)).T + np.array([20.0, -10.0, 700.0])
    return p + rng.normal(scale=0.3, size=p.shape)


def test_voxel_down_sampling_and_normals_match_the_restatement():
    from pyrapose_amd.utils import icp
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    p = surface_cloud(1)
    nrm = np.random.default_rng(2).normal(size=p.shape)
    v, vn = icp.voxel_down_sample(p, 5.0, normals=nrm)
    want, want_n, _ = I.voxel_down_sample(p, 5.0, nrm)
    assert v.shape == want.shape and np.abs(v.cpu().numpy() - want).max() <= 1e-12
    assert np.abs(vn.cpu().numpy() - want_n).max() <= 1e-12
    assert np.array_equal(icp.voxel_down_sample(p, 5.0).cpu().numpy(), v.cpu().numpy())
    q = want
    N, nb = ops.estimate_normals(default_context(), torch.from_numpy(q).cuda(), 10.0, 10, return_neighbors=True)
    N, nb = N.cpu().numpy(), nb.cpu().numpy()
    wN, wnb = I.estimate_normals(q, 10.0, 10)
    for i in range(len(q)):
        assert nb[i][nb[i] >= 0].tolist() == wnb[i].tolist()
    has = np.abs(wN).sum(1) > 0
    assert has.sum() > 0.8 * len(q) and np.array_equal(np.abs(N).sum(1) > 0, has)
    angle = 2.0 * np.arcsin(np.minimum(np.linalg.norm(N[has] - wN[has], axis=1) / 2.0, 1.0))
    assert angle.max() < 1e-9 and np.all(np.einsum("ij,ij->i", N[has], q[has]) <= 0)
    assert np.array_equal(icp.estimate_normals(q, 10.0, 10).cpu().numpy(), N)


def icp_problems(n_prob=20, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_prob):
        src, nrm = asymmetric_cloud(int(rng.integers(150, 260)), seed + k)
        R, t = rot(rng.normal(size=3), rng.uniform(0, 180)), np.array([rng.uniform(-50, 50), rng.uniform(-40, 40), rng.uniform(600, 900)])
        keep = rng.uniform(size=len(src)) < 0.85
        tgt = (src @ R.T + t)[keep] + rng.normal(scale=0.2, size=(keep.sum(), 3))
        tn = (nrm @ R.T)[keep]
        tgt = np.concatenate([tgt, t + rng.uniform(-120, 120, (20, 3))])          # outliers
        tn = np.concatenate([tn, np.zeros((20, 3))])                                # without normals: never plane targets
        dR = rot(rng.normal(size=3), rng.uniform(2, 5))
        dt = rng.normal(size=3)
        dt *= rng.uniform(5, 15) / np.linalg.norm(dt)
        T0 = np.eye(4)
        T0[:3, :3], T0[:3, 3] = dR @ R, t + dt
        out.append(dict(source=src, target=tgt, init=T0, target_normals=tn))
    return out


@pytest.mark.parametrize("mode", ["point_to_plane", "point_to_point"])
def test_icp_matches_the_restatement(mode):
    from pyrapose_amd.utils import icp
    probs = icp_problems()
    got = icp.registration_icp_batch(probs, 15.0, mode, max_iteration=30)
    moved = 0
    for pr, g in zip(probs, got):
        w = I.registration_icp(pr["source"], pr["target"], pr["init"], 15.0, 30, estimation=mode, tgt_normals=pr["target_normals"])
        assert g.status == "ok" and w["status"] == I.OK
        assert g.iterations == w["iterations"] and g.fitness == w["fitness"]
        corr = np.full(len(pr["source"]), -1)
        corr[g.correspondence_set[:, 0]] = g.correspondence_set[:, 1]
        assert np.array_equal(corr, w["corr"])
        assert np.abs(g.transformation[:3, :3] - w["R"]).max() < 1e-9
        assert np.abs(g.transformation[:3, 3] - w["t"]).max() < 1e-6
        assert abs(g.inlier_rmse - w["inlier_rmse"]) <= 1e-12 * w["inlier_rmse"]
        moved += g.iterations > 1
    assert moved == len(probs)


def test_icp_is_bitwise_deterministic_and_batch_independent():
    from pyrapose_amd.utils import icp
    probs = icp_problems(8, seed=11)
    for mode in ("point_to_plane", "point_to_point"):
        a = icp.registration_icp_batch(probs, 15.0, mode)
        b = icp.registration_icp_batch(probs, 15.0, mode)
        one = [icp.registration_icp(p["source"], p["target"], 15.0, p["init"], mode, target_normals=p["target_normals"]) for p in probs]
        rev = icp.registration_icp_batch(probs[::-1], 15.0, mode)[::-1]
        for x, y, z, u in zip(a, b, one, rev):
            for o in (y, z, u):
                assert np.array_equal(x.transformation.view(np.uint64), o.transformation.view(np.uint64))
                assert (x.fitness, x.inlier_rmse, x.iterations, x.status) == (o.fitness, o.inlier_rmse, o.iterations, o.status)
                assert np.array_equal(x.correspondence_set, o.correspondence_set)


def wedge_box_mesh():
    """a box with a smaller box standing off one corner of its top (asymmetric), metres, outward winding"""
    a = RN.box_mesh(0.08, 0.06, 0.11)
    b = RN.box_mesh(0.04, 0.03, 0.03)
    pts = np.concatenate([a["pts"], b["pts"] + np.array([0.025, 0.018, 0.07])])
    return {"pts": pts, "faces": np.concatenate([a["faces"], b["faces"] + 8])}


def scene(model, R, t_mm, W=640, H=480):
    """uint16 millimetre depth of the model at (R, t) in front of a plane 200 mm behind it, and the silhouette on the 60x80 grid"""
    from pyrapose_amd.utils.renderer import render
    mm = dict(model, pts=model["pts"] * 1000.0)
    obj = render(mm, (W, H), K, R, t_mm)
    z = t_mm[2] + 200.0
    plane = {"pts": np.array([[-2000, -2000, 0], [2000, -2000, 0], [2000, 2000, 0], [-2000, 2000, 0]], np.float64), "faces": np.array([[0, 1, 2], [0, 2, 3]])}
    bg = render(plane, (W, H), K, np.eye(3), [0.0, 0.0, z])
    depth = np.where(obj > 0, obj, bg)
    grid = (obj > 0).reshape(H // 8, 8, W // 8, 8).mean((1, 3)) > 0.5
    return np.round(depth).astype(np.uint16), grid.astype(np.float32).reshape(-1)


def add_err(R, t, Rg, tg, pts):
    return float(np.linalg.norm((pts @ R.T + t) - (pts @ Rg.T + tg), axis=1).mean())


def test_refine_pose_on_rendered_scenes():
    """Bars settled with the numpy restatement on the same scenes (tests/render_np.py, tests/icp_np.py): at the default 10 mm
    correspondence distance five of these six starts (2-5 degrees, 5-15 mm) refine to 0.9-1.4 mm ADD; one loses its
    correspondences (fitness 0.02) and keeps its input pose, refined=False."""
    from pyrapose_amd.utils import icp
    model = wedge_box_mesh()
    pts = model["pts"]
    dia = max(np.linalg.norm(p - q) for p in pts for q in pts)
    rng = np.random.default_rng(3)
    before, after, n_ref = [], [], 0
    for _ in range(6):
        Rg = rot(rng.normal(size=3), rng.uniform(20, 160))
        tg = np.array([rng.uniform(-60, 60), rng.uniform(-40, 40), rng.uniform(650, 850)])
        depth, mask = scene(model, Rg, tg)
        dt = rng.normal(size=3)
        dt *= rng.uniform(5, 15) / np.linalg.norm(dt)
        R0, t0 = rot(rng.normal(size=3), rng.uniform(2, 5)) @ Rg, (tg + dt) * 0.001
        R1, t1, info = icp.refine_pose(R0, t0, depth, mask, K, model)
        a0, a1 = add_err(R0, t0, Rg, tg * 0.001, pts), add_err(R1, t1, Rg, tg * 0.001, pts)
        if info["refined"]:
            n_ref += 1
            assert info["fitness"] > 0.9 and a1 < 0.5 * a0, (a0, a1, info)
        else:
            assert np.array_equal(R1, R0) and np.array_equal(t1, t0)
        before.append(a0)
        after.append(a1)
    assert n_ref >= 5, (before, after)
    assert np.median(after) < 0.01 * dia, (after, dia)


def test_edge_cases():
    from pyrapose_amd.utils import icp
    model = wedge_box_mesh()
    Rg, tg = rot([1.0, 1.0, 0.0], 40.0), np.array([0.0, 0.0, 700.0])
    depth, mask = scene(model, Rg, tg)
    R0, t0 = rot([0, 0, 1.0], 3.0) @ Rg, tg * 0.001 + 0.005
    for m in (np.zeros_like(mask), np.where(np.arange(mask.size) < 2, 1.0, 0.0)):     # empty, 2 cells = 128 pixels
        R1, t1, info = icp.refine_pose(R0, t0, depth, m, K, model)
        assert not info["refined"] and np.array_equal(R1, R0) and np.array_equal(t1, t0)
    # fewer than 6 correspondences: the status and the unchanged pose
    src, n = asymmetric_cloud(seed=1)
    T0 = np.eye(4)
    T0[:3, 3] = [1.0, 0.0, 0.0]
    r = icp.registration_icp(src[:4], src[:4], 10.0, T0, target_normals=n[:4])
    assert r.status == "too_few_correspondences" and np.array_equal(r.transformation, T0) and r.iterations == 0
    r = icp.registration_icp(src, src + 500.0, 10.0, np.eye(4), target_normals=n)
    assert r.status == "too_few_correspondences" and r.fitness == 0.0 and np.array_equal(r.transformation, np.eye(4))
    det = dict(cls=0, R=R0, t=t0)
    with pytest.raises(ValueError):
        icp.refine_poses([det], depth[None], mask.reshape(-1, 1), K, [model])
    with pytest.raises(ValueError):
        icp.refine_poses([det], depth, mask.reshape(-1, 1)[:100], K, [model])
    with pytest.raises(ValueError):
        icp.refine_poses([det], depth, mask.reshape(-1, 1), K[:2], [model])
    with pytest.raises(ValueError):                                                       # model in millimetres
        icp.refine_poses([det], depth, mask.reshape(-1, 1), K, [dict(model, pts=model["pts"] * 1e5)])
    with pytest.raises(ValueError):                                                       # translation in millimetres
        icp.refine_poses([dict(det, t=tg * 1000.0)], depth, mask.reshape(-1, 1), K, [model])
    with pytest.raises(ValueError):
        icp.registration_icp(src[:, :2], src, 10.0)
    with pytest.raises(ValueError):
        icp.registration_icp(src, src, 10.0, estimation="point_to_point_to_plane")
    with pytest.raises(ValueError):
        icp.registration_icp(src, src, 10.0)                                               # point_to_plane without normals
    with pytest.raises(ValueError):
        icp.voxel_down_sample(src, 0.0)


def test_evaluation_hook_refines_a_pose_off_along_the_optical_axis():
    from pyrapose_amd.utils import eval_pose
    from pyrapose_amd.utils.renderer import render
    rng = np.random.default_rng(5)
    Cn, N, H, W = 2, 2000, 480, 640
    sizes = [(0.08, 0.06, 0.11), (0.088, 0.066, 0.121)]
    models = [RN.box_mesh(*s) for s in sizes]
    boxes = np.stack([m["pts"] for m in models])
    dia = [float(np.linalg.norm(np.asarray(s))) for s in sizes]
    cases = []
    for lab, kind in ((0, "good"), (1, "deeper")):
        R = rot(rng.normal(size=3), rng.uniform(30, 150))
        t = np.array([rng.uniform(-50, 50), rng.uniform(-30, 30), rng.uniform(650, 800)])
        cases.append((lab, R, t, kind))

    def mat2quat(R):
        w = math.sqrt(max(1.0 + R[0, 0] + R[1, 1] + R[2, 2], 0.0)) / 2
        return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])

    cases = [(lab, eval_pose.quat2mat(mat2quat(R)), mat2quat(R), t, kind) for lab, R, t, kind in cases]

    class Gen(object):
        def size(self): return len(cases)
        def load_image(self, i): return np.full((H, W, 3), i, np.uint8)
        def preprocess_image(self, x): return x.astype(np.float32)
        def resize_image(self, x): return x, 1.0
        def load_annotations(self, i):
            lab, _R, q, t, _ = cases[i]
            return {"labels": np.array([float(lab)]), "poses": np.array([np.concatenate([t, q])])}

    def obj_depth(i):
        lab, R, _q, t, _ = cases[i]
        return render(dict(models[lab], pts=models[lab]["pts"] * 1000.0), (W, H), K, R, t)

    def load_depth(i):
        return np.round(obj_depth(i)).astype(np.uint16)

    def predict(x):
        i = int(x[0, 0, 0, 0])
        lab, R, _q, t, kind = cases[i]
        tt = t * 0.001 + (np.array([0.0, 0.0, 0.025]) if kind == "deeper" else 0.0)   # 25 mm along the optical axis
        Xc = boxes[lab] @ R.T + tt
        uv = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1)
        b3 = rng.uniform(0, 600, (1, N, 16)).astype(np.float32)
        sc = rng.uniform(0, 0.2, (1, N, Cn)).astype(np.float32)
        anchors = np.sort(rng.choice(N, 40, replace=False))
        b3[0, anchors] = (uv[None] + rng.normal(scale=0.05, size=(40, 8, 2))).reshape(40, 16)
        sc[0, anchors, lab] = 0.9
        mask = np.zeros((1, 4800, Cn), np.float32)
        mask[0, :, lab] = ((obj_depth(i) > 0).reshape(60, 8, 80, 8).mean((1, 3)) > 0.5).reshape(-1)
        return [b3, sc, mask]

    plain = eval_pose.evaluate_pose_metrics(Gen(), predict, boxes, models, dia, load_depth, K)
    refined = eval_pose.evaluate_pose_metrics(Gen(), predict, boxes, models, dia, load_depth, K,
                                              refine=dict(max_correspondence_distance=40.0))
    assert set(plain["errors"][0]) == {"image", "cls", "ok", "re", "te", "reproj", "vsd", "add"}
    p = {(e["image"], e["cls"]): e for e in plain["errors"]}
    r = {(e["image"], e["cls"]): e for e in refined["errors"]}
    assert p[(1, 1)]["add"] > 0.1 * dia[1] and p[(0, 0)]["add"] < 0.1 * dia[0]
    for key in r:
        assert r[key]["refined"] and r[key]["fitness"] > 0.3
        assert r[key]["add"] < 0.1 * dia[key[1]], (key, r[key]["add"])
    # the ADD < 0.1 d decision: the deeper pose fails it plain and passes it refined, the good one passes both
    assert plain["add_less"][1, 1:].tolist() == [1, 0] and refined["add_less"][1, 1:].tolist() == [1, 1]
    out = eval_pose.evaluate_add(Gen(), predict, boxes, [m["pts"] for m in models], dia, K, load_depth=load_depth,
                                 refine=dict(models=models, max_correspondence_distance=40.0))
    assert out["truePoses"].tolist() == [0, 1, 1] and all(len(e) == 5 and e[3] for e in out["errors"])
    base = eval_pose.evaluate_add(Gen(), predict, boxes, [m["pts"] for m in models], dia, K)
    assert base["truePoses"].tolist() == [0, 1, 0] and all(len(e) == 3 for e in base["errors"])
