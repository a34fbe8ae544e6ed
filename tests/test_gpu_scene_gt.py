"""GPU: scene ground truth from rendered instances (pp_scene_gt_info through ops.scene_gt_info and utils.scene_gt) against
the numpy restatement tests/scene_gt_np.py, which is fed the same device-rendered depth stack: everything is integer valued
(or a minimum of float32 values), so every comparison is exact.  A 70 x 45 image (no multiple of 32 or of 4), two scenes of 4
and 1 instances, two meshes (a 12-triangle box, a tetrahedron) interleaved within the first scene."""
import numpy as np
import pytest
import torch

from tests import render_np as RN
from tests import scene_gt_np as SN

pytestmark = pytest.mark.gpu
W, H, DELTA = 70, 45, 15.0
K = np.array([[150.0, 0.0, 35.3], [0.0, 150.0, 22.1], [0.0, 0.0, 1.0]])
BOX, TETRA = 1, 2


def tetra_mesh(s):
    v = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * s
    return {"pts": v, "faces": np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)}


MODELS = {BOX: RN.box_mesh(80.0, 60.0, 110.0), TETRA: tetra_mesh(20.0)}
_c, _s = np.cos(0.4), np.sin(0.4)
R_TURNED = np.array([[_c, 0.0, _s], [0.0, 1.0, 0.0], [-_s, 0.0, _c]])
# scene 0: the box cut by the left image border (0), a tetrahedron far behind it (1), a tetrahedron whose surface crosses the
# box's front face, so that the two are within DELTA of each other (2), a tetrahedron off screen (3); scene 1: a turned box
SCENES = [[{"obj_id": BOX, "R": np.eye(3), "t": [-100.0, 0.0, 450.0]},
           {"obj_id": TETRA, "cam_R_m2c": list(np.eye(3).reshape(-1)), "cam_t_m2c": [-137.0, 0.0, 700.0]},
           {"obj_id": TETRA, "R": np.eye(3), "t": [-75.0, -15.0, 390.0]},
           {"obj_id": TETRA, "R": np.eye(3), "t": [5000.0, 0.0, 600.0]}],
          [{"obj_id": BOX, "R": R_TURNED, "t": [3.0, -2.0, 600.0]}]]
CUT, HIDDEN, NEAR, OFF, TURNED = range(5)
OFFSETS = np.array([0, 4, 5], np.int32)


def render_stack(extent):
    """the instances of SCENES in scene order, rendered per mesh as utils.scene_gt does -> numpy float32 [5,ch,cw], window"""
    from pyrapose_amd.utils import scene_gt as SG
    from pyrapose_amd.utils.renderer import render_depth_batch
    plan = SG.plan_instances(SCENES)
    assert list(plan.groups) == [BOX, TETRA] and plan.order.tolist() == [0, 2, 3, 4, 1]
    Kr, canvas, window = K.copy(), (W, H), None
    if extent == "bop":
        Kr[0, 2] += W
        Kr[1, 2] += H
        canvas, window = (3 * W, 3 * H), (W, H, W, H)
    renders = [render_depth_batch(MODELS[o], canvas, Kr, plan.R[idx], plan.t[idx]) for o, idx in plan.groups.items()]
    return torch.cat(renders)[torch.from_numpy(plan.order).cuda()].cpu().numpy(), window


@pytest.fixture(scope="module")
def image_stack():
    stack, _ = render_stack("image")
    stack.setflags(write=False)
    return stack


@pytest.fixture(scope="module")
def sensor(image_stack):
    """per scene: the rounded scene in front of a plane at 2000, with a block without sensor values over a part of the turned box"""
    depth = np.stack([SN.compose_depth(image_stack[:4]), SN.compose_depth(image_stack[4:])])
    depth = np.where(depth > 0, np.round(depth), 2000.0).astype(np.float32)
    rows, cols = np.nonzero(image_stack[TURNED] > 0)
    depth[1, rows.min() + 2:rows.min() + 7, cols.min() + 3:cols.min() + 12] = 0.0
    depth.setflags(write=False)
    return depth


def same(got, want, scene_depth):
    """a SceneGT of ops.scene_gt_info against the restatement's dict, every field exactly"""
    for k in ("px_count", "bbox_obj", "bbox_visib", "id_image", "mask_full", "mask_visib"):
        a = getattr(got, k).cpu().numpy()
        assert a.dtype == want[k].dtype and np.array_equal(a, want[k]), (k, a, want[k])
    if scene_depth:
        a = got.scene_depth.cpu().numpy()
        assert a.dtype == np.float32 and np.array_equal(a, want["scene_depth"])
    else:
        assert got.scene_depth is None and want["scene_depth"] is None


def run_ops(stack, depth=None, window=None, masks=True):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    from pyrapose_amd.utils._host import k4, to_device
    return ops.scene_gt_info(default_context(), to_device(stack, torch.float32), OFFSETS, to_device(k4(K, len(stack))),
                             None if depth is None else to_device(depth, torch.float32), DELTA, window, masks)


def assert_scene_has_every_case(want, sensor_depth):
    """the properties the scene was built for, on the restatement's result"""
    n_all, n_valid, n_vis = want["px_count"].T
    assert n_all[CUT] > 100 and want["bbox_obj"][CUT][0] == 0                                   # 1. cut by the image border
    assert n_all[HIDDEN] > 0 and n_vis[HIDDEN] == 0                                            # 2. fully hidden
    assert want["bbox_obj"][HIDDEN].tolist() == [-1] * 4 and want["bbox_visib"][HIDDEN].tolist() == [-1] * 4
    assert want["px_count"][OFF].tolist() == [0, 0, 0] and want["bbox_obj"][OFF].tolist() == [-1] * 4        # 3. nothing rendered
    both = (want["mask_visib"][CUT] > 0) & (want["mask_visib"][NEAR] > 0)                       # 4. two visible on one pixel
    assert both.sum() >= 1 and (want["id_image"][0][both] == NEAR + 1).all()
    assert 0 < n_vis[CUT] < n_all[CUT] and 0 < n_vis[NEAR] <= n_all[NEAR]
    assert sorted(np.unique(want["id_image"][0]).tolist()) == [0, CUT + 1, NEAR + 1] and np.unique(want["id_image"][1]).tolist() == [0, 1]
    if sensor_depth:
        assert 0 < n_valid[TURNED] < n_vis[TURNED] == n_all[TURNED]                             # 5. no sensor value, yet visible
    else:
        assert (n_valid == n_all).all()


def test_counts_boxes_ids_and_masks_with_sensor_depth(image_stack, sensor):
    want = SN.scene_gt(image_stack, OFFSETS, K, sensor, DELTA)
    assert_scene_has_every_case(want, True)
    same(run_ops(image_stack, sensor), want, False)
    # one depth image shared by both scenes
    same(run_ops(image_stack, sensor[1]), SN.scene_gt(image_stack, OFFSETS, K, sensor[1], DELTA), False)
    # without the optional masks the rest is the same
    got = run_ops(image_stack, sensor, masks=False)
    assert got.mask_full is None and got.mask_visib is None and np.array_equal(got.px_count.cpu().numpy(), want["px_count"])
    assert np.array_equal(got.id_image.cpu().numpy(), want["id_image"])


def test_counts_boxes_ids_masks_and_composed_depth_without_sensor_depth(image_stack):
    want = SN.scene_gt(image_stack, OFFSETS, K, None, DELTA)
    assert_scene_has_every_case(want, False)
    assert (want["scene_depth"] > 0).sum() > 300 and (want["scene_depth"] == 0).sum() > 300
    same(run_ops(image_stack), want, True)


def test_window_not_aligned_to_four_pixels(image_stack):
    """the 70 x 45 renders as the canvas, the image a 41 x 30 window at (13, 6): groups of four start off the canvas' columns"""
    window = (13, 6, 41, 30)
    Kw = K.copy()
    Kw[0, 2] -= 13
    Kw[1, 2] -= 6
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    from pyrapose_amd.utils._host import k4, to_device
    want = SN.scene_gt(image_stack, OFFSETS, Kw, None, DELTA, window)
    assert want["bbox_obj"][CUT][0] == -13 and want["px_count"][CUT][0] == (image_stack[CUT] > 0).sum() > want["mask_full"][CUT].astype(bool).sum()
    got = ops.scene_gt_info(default_context(), to_device(image_stack, torch.float32), OFFSETS, to_device(k4(Kw, 5)), None, DELTA, window, True)
    same(got, want, True)


def test_utils_both_extents(image_stack, sensor):
    from pyrapose_amd.utils import scene_gt as SG
    results = {}
    for extent in ("image", "bop"):
        stack, window = render_stack(extent)
        if extent == "image":
            assert np.array_equal(stack, image_stack)                                           # the renderer repeats its bits
        for depth in (sensor, None):
            want = SN.scene_gt(stack, OFFSETS, K, depth, DELTA, window)
            got = SG.scene_gt_info(SCENES, MODELS, K, depth, (W, H), DELTA, extent, masks=True)
            flat = [row for rows in got.info for row in rows]
            assert [len(rows) for rows in got.info] == [4, 1]
            for i, row in enumerate(flat):
                assert sorted(row) == ["bbox_obj", "bbox_visib", "px_count_all", "px_count_valid", "px_count_visib", "visib_fract"]
                assert [row["px_count_all"], row["px_count_valid"], row["px_count_visib"]] == want["px_count"][i].tolist()
                assert row["bbox_obj"] == want["bbox_obj"][i].tolist() and row["bbox_visib"] == want["bbox_visib"][i].tolist()
                n_all, n_vis = int(want["px_count"][i][0]), int(want["px_count"][i][2])
                assert row["visib_fract"] == (n_vis / float(n_all) if n_all else 0.0)
            assert got.id_images.dtype == np.uint8 and np.array_equal(got.id_images, want["id_image"])
            assert np.array_equal(np.concatenate(got.mask_full), want["mask_full"])
            assert np.array_equal(np.concatenate(got.mask_visib), want["mask_visib"])
            assert [len(m) for m in got.mask_visib] == [4, 1]
            if depth is None:
                assert got.depth.dtype == np.float32 and np.array_equal(got.depth, want["scene_depth"])
            else:
                assert got.depth is None
            results[(extent, depth is None)] = flat
    assert results[("image", True)][OFF]["visib_fract"] == 0.0 and results[("bop", True)][OFF]["px_count_all"] == 0
    for composed in (True, False):
        image, bop = results[("image", composed)][CUT], results[("bop", composed)][CUT]
        assert bop["px_count_all"] > image["px_count_all"] and bop["bbox_obj"][0] < 0 == image["bbox_obj"][0]
        assert bop["bbox_visib"][0] == 0 and bop["px_count_visib"] > 0


def test_visible_fraction_is_that_of_visib_fract_batch(sensor):
    from pyrapose_amd.utils import pose_error as PE
    from pyrapose_amd.utils import scene_gt as SG
    got = SG.scene_gt_info(SCENES, MODELS, K, sensor, delta=DELTA)
    assert got.mask_full is None and got.depth is None
    fractions = []
    for s, instances in enumerate(SCENES):
        for inst, row in zip(instances, got.info[s]):
            R = inst["R"] if "R" in inst else inst["cam_R_m2c"]
            t = inst["t"] if "t" in inst else inst["cam_t_m2c"]
            one = PE.visib_fract_batch(np.reshape(R, (1, 3, 3)), np.reshape(t, (1, 3)), MODELS[inst["obj_id"]], sensor[s], K, DELTA)
            assert one.dtype == np.float64 and one[0] == row["visib_fract"]
            fractions.append(row["visib_fract"])
    assert 0.0 < fractions[CUT] < 1.0 and fractions[HIDDEN] == 0.0 and fractions[OFF] == 0.0 and fractions[TURNED] == 1.0


def test_two_calls_give_identical_bytes(image_stack, sensor):
    for depth in (sensor, None):
        a, b = run_ops(image_stack, depth), run_ops(image_stack, depth)
        for x, y in zip(a, b):
            assert (x is None and y is None) or x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_refused_arguments_launch_nothing(image_stack):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    from pyrapose_amd.utils._host import k4, to_device
    ctx = default_context()
    want = SN.scene_gt(image_stack, OFFSETS, K, None, DELTA)

    def call(stack=image_stack, offsets=OFFSETS, window=None, delta=DELTA, n=None):
        stack = to_device(stack, torch.float32)
        return ops.scene_gt_info(ctx, stack, offsets, to_device(k4(K, n or len(stack))), None, delta, window, True)

    def refused(code, **kw):
        with pytest.raises(ValueError, match=r"pp_scene_gt_info failed \(%d\)" % code):
            call(**kw)
        same(call(), want, True)                                                    # the next valid call works

    many = np.zeros((256, 4, 5), np.float32)
    refused(-2, stack=many, offsets=[0, 256])                                       # PP_ERR_SHAPE: 256 instances in one scene
    assert np.array_equal(call(stack=many[:255], offsets=[0, 255]).px_count.cpu().numpy(), np.zeros((255, 3), np.int64))
    refused(-2, window=(30, 0, 41, 45))                                             # the window leaves the canvas
    refused(-2, window=(0, 16, 70, 30))
    refused(-2, window=(-1, 0, 70, 45))
    refused(-1, offsets=[0, 3, 2, 5])                                               # PP_ERR_ARG: offsets that decrease
    refused(-1, offsets=[0, 4, 4])
    refused(-1, offsets=[1, 4, 5])
    refused(-1, delta=-1.0)
    refused(-1, delta=float("nan"))
    assert ops.lib.pp_scene_gt_workspace_bytes(0, 70, 45) == 0 and ops.lib.pp_scene_gt_workspace_bytes(5, 70, 20000) == 0
    assert ops.lib.pp_scene_gt_workspace_bytes(5, 70, 45) > 0
