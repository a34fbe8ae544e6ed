"""GPU: pp_vote_cluster (csrc/cluster.hip) against its numpy restatement (tests/cluster_np.py) -- every output array_equal --
and the per-instance path it opens: pose_decode.poses_from_outputs(instances=...), the two evaluation loops and the box
restriction of utils.icp.refine_poses.  The scenes' instance counts are settled on the CPU in tests/test_cluster_cpu.py."""
import numpy as np
import pytest
import torch

from tests import cluster_np as CN
from tests.test_oracle_pnp import BOX, K4, rot_err_deg

pytestmark = pytest.mark.gpu
KMAT = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])
NAMES = ("inst", "order", "inst_offsets", "n_inst", "leader", "inst_box")


@pytest.fixture(scope="module")
def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


def device_cluster(ctx, b3, sc, cap=None, **kw):
    from pyrapose_amd import ops
    b3, sc = torch.from_numpy(b3).cuda(), torch.from_numpy(sc).cuda()
    idx, cnt = ops.score_threshold_compact(ctx, sc, 0.5, cap)
    got = ops.vote_cluster(ctx, b3, sc, idx, cnt, **kw)
    return idx.cpu().numpy(), cnt.cpu().numpy(), [g.cpu().numpy() for g in got]


def assert_same(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


@pytest.fixture(scope="module")
def mixed():
    return CN.mixed_scene()


@pytest.mark.parametrize("cap", [None, 128])
def test_matches_the_restatement_exactly(ctx, mixed, cap):
    b3, sc, n_want = mixed
    idx, cnt, got = device_cluster(ctx, b3, sc, cap, iou=0.5, min_votes=10, max_instances=2)
    want = CN.vote_cluster(b3, sc, idx, cnt, 0.5, 10, 2)
    assert idx.shape[2] == (cap or 600) and np.array_equal(got[3], n_want)
    assert_same(got, want)


def test_batch_independence_and_determinism(ctx, mixed):
    b3, sc, _ = mixed
    _, _, both = device_cluster(ctx, b3, sc, iou=0.5, min_votes=10, max_instances=2)
    _, _, again = device_cluster(ctx, b3, sc, iou=0.5, min_votes=10, max_instances=2)
    _, _, alone = device_cluster(ctx, b3[1:], sc[1:], iou=0.5, min_votes=10, max_instances=2)
    for name, a, b, c in zip(NAMES, both, again, alone):
        assert np.array_equal(a, b) and np.array_equal(a[1:], c), name


def test_counts_beyond_the_lds_cache(ctx):
    b3, sc, sizes = CN.large_scene()
    idx, cnt, got = device_cluster(ctx, b3, sc, iou=0.5, min_votes=10, max_instances=8)
    assert cnt[0, 0] == 2500 and got[3][0, 0] == 3 and sorted(np.diff(got[2][0, 0, :4]).tolist()) == sorted(sizes)
    assert_same(got, CN.vote_cluster(b3, sc, idx, cnt, 0.5, 10, 8))
    # every stop rule on the same votes: max_rounds 1, max_instances 2, a min_votes only the largest instance reaches
    for kw in (dict(max_instances=8, max_rounds=1), dict(max_instances=2), dict(max_instances=8, min_votes=1000)):
        kw = dict(dict(iou=0.5, min_votes=10), **kw)
        _, _, got = device_cluster(ctx, b3, sc, **kw)
        assert_same(got, CN.vote_cluster(b3, sc, idx, cnt, kw["iou"], kw["min_votes"], kw["max_instances"], kw.get("max_rounds")))


def test_bad_arguments(ctx, mixed):
    from pyrapose_amd import ops
    from pyrapose_amd._lib import lib
    b3, sc = torch.from_numpy(mixed[0]).cuda(), torch.from_numpy(mixed[1]).cuda()
    idx, cnt = ops.score_threshold_compact(ctx, sc, 0.5)
    out = ops.vote_cluster(ctx, b3, sc, idx, cnt, max_instances=2)
    p = lambda t: t.data_ptr()

    def call(cap=600, iou=0.5, min_votes=10, mi=2, mr=8, boxes=p(b3), inst=p(out[0])):
        return lib.pp_vote_cluster(ctx.handle, 2, 600, 3, cap, boxes, p(sc), p(idx), p(cnt), iou, min_votes, mi, mr, None, inst, p(out[1]),
                                   p(out[2]), p(out[3]), p(out[4]), p(out[5]))

    assert call() == 0
    for kw in (dict(cap=0), dict(mi=0), dict(iou=1.0), dict(iou=-0.1), dict(iou=float("nan")), dict(min_votes=0), dict(mr=0),
               dict(boxes=None), dict(inst=None)):
        assert call(**kw) == -1, kw  # PP_ERR_ARG
    for kw in (dict(iou=1.0), dict(max_instances=0), dict(min_votes=0)):
        with pytest.raises(ValueError):
            ops.vote_cluster(ctx, b3, sc, idx, cnt, **kw)
    with pytest.raises(ValueError):
        ops.vote_cluster(ctx, b3, sc.double(), idx, cnt)
    assert lib.pp_vote_cluster_workspace_bytes(2, 3, 600, 2) == 0


def votes_of(b3, anchors):
    """(obj [8k,3], img [8k,2] as the device sees them: float32 votes widened, K) of one vote set"""
    k = len(anchors)
    return np.tile(BOX, (k, 1)), b3[0, anchors].astype(np.float64).reshape(-1, 2), KMAT


def test_two_instances_end_to_end(ctx):
    from pyrapose_amd.utils import pnp, pose_decode
    b3, sc, truth = CN.two_instance_scene()
    corners = np.stack([BOX, BOX])
    out = pose_decode.poses_from_outputs(b3, sc, corners, KMAT, iterations=120, seed=9, ctx=ctx, instances=dict(iou=0.5))
    assert [(o["image"], o["cls"], o["instance"]) for o in out] == [(0, 0, 0), (0, 0, 1), (0, 1, 0)]
    idx, cnt = CN.threshold_compact(sc)
    _, order, offs, n_inst, leader, box = CN.vote_cluster(b3, sc, idx, cnt, 0.5, 10, 8)
    sets = [order[0, c, offs[0, c, k]:offs[0, c, k + 1]] for c in range(2) for k in range(n_inst[0, c])]
    want = pnp.solve_pnp_batch([votes_of(b3, s) for s in sets], iterations=120, reproj_error=5.0, seed=9, points_per_vote=8, ctx=ctx)
    used = set()
    for o, s, (ok, R, t, inl), (c, k) in zip(out, sets, want, ((0, 0), (0, 1), (1, 0))):
        assert np.array_equal(o["votes"], s) and o["ok"] and ok and np.array_equal(o["inliers"], inl)
        assert np.abs(o["R"] - R).max() < 1e-8 and np.abs(o["t"] - t).max() < 1e-6
        assert o["leader"] == leader[0, c, k] and np.array_equal(o["box"], box[0, c, k]) and o["score"] == sc[0, o["leader"], c]
        # the pose this cluster belongs to: the one whose anchors hold its leader
        j = [i for i, tr in enumerate(truth) if tr[0] == c and o["leader"] in tr[3]]
        assert len(j) == 1 and j[0] not in used
        used.add(j[0])
        assert rot_err_deg(o["R"], truth[j[0]][1]) < 3.0, (c, k, rot_err_deg(o["R"], truth[j[0]][1]))
    assert len(used) == 3
    pooled = pose_decode.poses_from_outputs(b3, sc, corners, KMAT, iterations=120, seed=9, ctx=ctx)
    assert [(o["image"], o["cls"]) for o in pooled] == [(0, 0), (0, 1)] and "instance" not in pooled[0]
    with pytest.raises(ValueError):
        pose_decode.poses_from_outputs(b3, sc, corners, KMAT, ctx=ctx, instances=dict(threshold=0.5))


@pytest.mark.parametrize("weighting", [None, "corners"])
def test_single_instances_equal_the_pooled_path(ctx, weighting):
    from pyrapose_amd.utils import pose_decode
    b3, sc = CN.single_instance_scene()
    corners = np.stack([BOX, BOX, BOX])
    a = pose_decode.poses_from_outputs(b3, sc, corners, KMAT, seed=2, ctx=ctx, weighting=weighting)
    b = pose_decode.poses_from_outputs(b3, sc, corners, KMAT, seed=2, ctx=ctx, weighting=weighting, instances=dict(iou=0.5, max_instances=4))
    assert len(a) == len(b) == 6
    for x, y in zip(a, b):
        assert (x["image"], x["cls"], x["ok"]) == (y["image"], y["cls"], y["ok"]) and y["instance"] == 0
        for key in ("R", "t", "votes", "inliers"):
            assert np.array_equal(x[key], y[key]), key


def mat2quat(R):
    """rotation matrix -> unit quaternion (w, x, y, z), largest component first (stable near 180 degrees)"""
    q = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2]])
    i = int(np.argmax(q))
    s = 2.0 * np.sqrt(q[i])
    if i == 0:
        out = [s / 4, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif i == 1:
        out = [(R[2, 1] - R[1, 2]) / s, s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif i == 2:
        out = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s]
    else:
        out = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4]
    return np.array(out)


def test_evaluation_matches_every_annotation_of_a_class(ctx):
    """two annotations of class 0 and the network's votes for both: per instance both are detected and correct, pooled one
    detection is scored against the first annotation"""
    from pyrapose_amd.utils import eval_pose
    from tests import render_np as RN
    b3, sc, truth = CN.two_instance_scene()
    boxes = np.stack([BOX, BOX]) * 0.001  # metres; the votes are pixels, so the scene's poses hold with t in millimetres
    models = [RN.box_mesh(0.08, 0.06, 0.11)] * 2
    dia = [float(np.linalg.norm(BOX.max(0) - BOX.min(0))) * 0.001] * 2

    class Gen(object):
        def size(self): return 1
        def load_image(self, i): return np.zeros((480, 640, 3), np.uint8)
        def preprocess_image(self, x): return x.astype(np.float32)
        def resize_image(self, x): return x, 1.0
        def load_annotations(self, i):
            return {"labels": np.array([float(tr[0]) for tr in truth]), "poses": np.array([np.concatenate([tr[2], mat2quat(tr[1])]) for tr in truth])}

    predict = lambda x: [b3, sc, np.zeros((1, 4800, 2), np.float32)]
    depth = lambda i: np.full((480, 640), 2000, np.uint16)
    per = eval_pose.evaluate_pose_metrics(Gen(), predict, boxes, models, dia, depth, KMAT, instances=dict(iou=0.5))
    assert per["allPoses"].tolist() == [0, 2, 1] and per["trueDets"].tolist() == [0, 2, 1] and per["less5"].tolist() == [0, 2, 1]
    assert sorted((e["cls"], e["instance"], e["gt"]) for e in per["errors"])[2] == (1, 0, 2)
    assert sorted(e["gt"] for e in per["errors"]) == [0, 1, 2]
    pooled = eval_pose.evaluate_pose_metrics(Gen(), predict, boxes, models, dia, depth, KMAT)
    assert pooled["allPoses"].tolist() == [0, 2, 1] and pooled["trueDets"].tolist() == [0, 1, 1] and "gt" not in pooled["errors"][0]
    add = eval_pose.evaluate_add(Gen(), predict, boxes, [m["pts"] for m in models], dia, KMAT, instances=dict(iou=0.5))
    assert add["trueDets"].tolist() == [0, 2, 1] and add["truePoses"].tolist() == [0, 2, 1] and all(len(e) == 5 for e in add["errors"])
    base = eval_pose.evaluate_add(Gen(), predict, boxes, [m["pts"] for m in models], dia, KMAT)
    assert base["trueDets"].tolist() == [0, 1, 1] and all(len(e) == 3 for e in base["errors"])


def test_icp_refines_each_of_two_objects_that_share_a_mask(ctx):
    """Two objects of one class in one depth image, one mask channel over both.  With each detection's box the refinement sees
    one object: the bars of test_gpu_icp.py::test_refine_pose_on_rendered_scenes for a refined start (fitness > 0.9, the error
    more than halved, below 1 % of the diameter), here on the translation, and the very pose that the refinement gives for
    that object alone in front of the plane.  A detection without a box is treated as before.

    The poses are chosen, not drawn: point-to-plane ICP fixes the translation only along the normals of the faces it sees, and
    that test's random poses include one in six that does not refine (a pose that shows a face of the box almost edge-on lets
    the model slide along it, with one object as with two).  Each object here turns a corner of its box to the camera, so
    three faces are seen at the same angle and all three axes are held; the starts are 8 mm and 3 degrees off.  With the
    numpy restatement (tests/icp_np.py, tests/render_np.py) these scenes end 0.98 and 0.94 mm from the truth at fitness 0.917
    and 0.989, with or without the other object."""
    from pyrapose_amd.utils import icp
    from pyrapose_amd.utils.renderer import render
    from tests.test_gpu_icp import K, wedge_box_mesh
    from tests.test_icp_cpu import rot
    model = wedge_box_mesh()
    pts = model["pts"]
    dia = max(np.linalg.norm(p - q) for p in pts for q in pts)
    rng = np.random.default_rng(3)
    W, H = 640, 480
    mm = dict(model, pts=pts * 1000.0)
    plane = {"pts": np.array([[-2000, -2000, 0], [2000, -2000, 0], [2000, 2000, 0], [-2000, 2000, 0]], np.float64), "faces": np.array([[0, 1, 2], [0, 2, 3]])}
    bg = render(plane, (W, H), K, np.eye(3), [0.0, 0.0, 960.0])
    depth = bg
    sil = np.zeros((H, W), bool)
    dets, gts, alone = [], [], []

    def corner_view(signs, spin):
        """the rotation that turns the box's corner (signs) to the camera, then spins it about the optical axis"""
        c = np.asarray(signs, np.float64) / np.sqrt(3.0)
        return rot([0.0, 0.0, 1.0], spin) @ rot(np.cross(c, [0.0, 0.0, -1.0]), np.degrees(np.arccos(-c[2])))

    for Rg, tg in ((corner_view([1, 1, 1], 25.0), np.array([-120.0, -20.0, 740.0])), (corner_view([1, -1, 1], -50.0), np.array([120.0, 25.0, 770.0]))):
        obj = render(mm, (W, H), K, Rg, tg)
        depth = np.where(obj > 0, obj, depth)
        sil |= obj > 0
        alone.append((np.round(np.where(obj > 0, obj, bg)).astype(np.uint16),
                      ((obj > 0).reshape(H // 8, 8, W // 8, 8).mean((1, 3)) > 0.5).astype(np.float32).reshape(-1, 1)))
        dt = rng.normal(size=3)
        dt *= 8.0 / np.linalg.norm(dt)
        R0, t0 = rot(rng.normal(size=3), 3.0) @ Rg, (tg + dt) * 0.001
        Xc = pts @ R0.T + t0
        uv = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1)
        dets.append(dict(cls=0, R=R0, t=t0, box=np.array([uv[:, 0].min(), uv[:, 1].min(), uv[:, 0].max(), uv[:, 1].max()], np.float32)))
        gts.append(tg * 0.001)
    depth = np.round(depth).astype(np.uint16)
    mask = (sil.reshape(H // 8, 8, W // 8, 8).mean((1, 3)) > 0.5).astype(np.float32).reshape(-1, 1)
    out = icp.refine_poses(dets, depth, mask, K, [model], ctx=ctx)
    for d, o, tg in zip(dets, out, gts):
        e0, e1 = float(np.linalg.norm(d["t"] - tg)), float(np.linalg.norm(o["t"] - tg))
        print("icp two objects: te before %.5f after %.5f fitness %.3f refined %s (1%% of the diameter: %.5f)" % (e0, e1, o["fitness"], o["refined"], 0.01 * dia))
    for d, o, tg in zip(dets, out, gts):
        e0, e1 = float(np.linalg.norm(d["t"] - tg)), float(np.linalg.norm(o["t"] - tg))
        assert o["refined"] and o["fitness"] > 0.9 and e1 < 0.5 * e0 and e1 < 0.01 * dia, (e0, e1, o["fitness"])
        assert np.array_equal(o["box"], d["box"])
    # the box leaves exactly the cells of the one object: the same pose as with that object alone in the image
    for d, o, (depth1, mask1) in zip(dets, out, alone):
        one = icp.refine_poses([{k: v for k, v in d.items() if k != "box"}], depth1, mask1, K, [model], ctx=ctx)[0]
        assert one["refined"] and np.array_equal(one["R"], o["R"]) and np.array_equal(one["t"], o["t"]) and one["fitness"] == o["fitness"]
    # no box: the whole class mask as before -- a box that covers the image restricts nothing and gives the same result
    plain = icp.refine_poses([{k: v for k, v in d.items() if k != "box"} for d in dets], depth, mask, K, [model], ctx=ctx)
    whole = icp.refine_poses([dict(d, box=[0.0, 0.0, W, H]) for d in dets], depth, mask, K, [model], ctx=ctx)
    for a, b in zip(plain, whole):
        assert "box" not in a and a["refined"] == b["refined"] and np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"])
