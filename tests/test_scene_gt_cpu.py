"""CPU (no GPU): the numpy restatement of the scene ground-truth pass (tests/scene_gt_np.py) on hand-written 5 x 4 depth
images whose counts, boxes and ids are typed in below, and the host side of utils.scene_gt: grouping by mesh and the way back
to scene order, annotations_from_scene, and the argument errors that are raised before any device call (there is no device
here, so reaching one would fail otherwise)."""
import numpy as np
import pytest

from tests import scene_gt_np as SN

# fx = fy = 1000 with the principal point in the middle: a distance differs from its depth by less than 1e-5 relative, so the
# visibility decisions below can be read off the depths
K = np.array([[1000.0, 0.0, 2.0], [0.0, 1000.0, 1.5], [0.0, 0.0, 1.0]])
A = np.array([[500, 500, 0, 0, 0],
              [500, 500, 500, 0, 0],
              [0, 0, 0, 0, 0],
              [0, 0, 0, 0, 0]], np.float32)
B = np.array([[0, 510, 510, 0, 0],           # within 15 of A where they overlap
              [0, 510, 510, 0, 0],
              [0, 0, 0, 0, 0],
              [0, 0, 0, 0, 0]], np.float32)
C = np.array([[0, 0, 0, 0, 0],               # 400 behind A and B, free in row 2
              [900, 900, 900, 0, 0],
              [900, 900, 900, 0, 0],
              [0, 0, 0, 0, 0]], np.float32)
D = np.array([[0, 0, 0, 0, 0],               # a second scene
              [0, 0, 0, 0, 0],
              [0, 0, 0, 700, 700],
              [0, 0, 0, 700, 700]], np.float32)
Z = np.zeros((4, 5), np.float32)


def test_restatement_on_hand_written_images_without_sensor_depth():
    out = SN.scene_gt(np.stack([A, B, C, Z, D]), [0, 4, 5], K, None, 15.0)
    assert np.array_equal(out["scene_depth"][0], [[500, 500, 510, 0, 0], [500, 500, 500, 0, 0], [900, 900, 900, 0, 0], [0, 0, 0, 0, 0]])
    assert np.array_equal(out["scene_depth"][1], D) and out["scene_depth"].dtype == np.float32
    assert out["px_count"].tolist() == [[5, 5, 5], [4, 4, 4], [6, 6, 3], [0, 0, 0], [4, 4, 4]] and out["px_count"].dtype == np.int64
    assert out["bbox_obj"].tolist() == [[0, 0, 2, 1], [1, 0, 1, 1], [0, 1, 2, 1], [-1, -1, -1, -1], [3, 2, 1, 1]]
    assert out["bbox_visib"].tolist() == [[0, 0, 2, 1], [1, 0, 1, 1], [0, 2, 2, 0], [-1, -1, -1, -1], [3, 2, 1, 1]]
    assert out["bbox_obj"].dtype == np.int32
    # B (2) overwrites A (1) wherever both are visible, also where it lies behind A
    assert out["id_image"][0].tolist() == [[1, 2, 2, 0, 0], [1, 2, 2, 0, 0], [3, 3, 3, 0, 0], [0, 0, 0, 0, 0]]
    assert out["id_image"][1].tolist() == [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 1, 1], [0, 0, 0, 1, 1]]
    assert out["id_image"].dtype == np.uint8
    assert np.array_equal(out["mask_full"][2], np.where(C > 0, 255, 0)) and out["mask_full"].dtype == np.uint8
    assert out["mask_visib"][2].tolist() == [[0] * 5, [0] * 5, [255, 255, 255, 0, 0], [0] * 5]


def test_restatement_with_sensor_depth_a_hidden_instance_and_a_window():
    sensor = np.array([[496, 496, 496, 2000, 2000],
                       [496, 0, 496, 2000, 2000],
                       [496, 496, 496, 2000, 2000],
                       [2000, 2000, 2000, 2000, 2000]], np.float32)
    out = SN.scene_gt(np.stack([A, B, C]), [0, 3], K, sensor, 15.0)
    assert out["scene_depth"] is None
    # A: 5 px within 15 of the sensor (one of them without a sensor value); B: 510 - 496 = 14 as well; C: hidden but for
    # the pixel without a sensor value ('bop19')
    assert out["px_count"].tolist() == [[5, 4, 5], [4, 3, 4], [6, 5, 1]]
    assert out["bbox_visib"].tolist() == [[0, 0, 2, 1], [1, 0, 1, 1], [1, 1, 0, 0]]
    assert out["bbox_obj"][2].tolist() == [0, 1, 2, 1]
    assert out["id_image"][0].tolist() == [[1, 2, 2, 0, 0], [1, 3, 2, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    # with a sensor value there C is hidden everywhere: counts stay, boxes become -1
    full = np.where(sensor == 0, 496, sensor).astype(np.float32)
    out = SN.scene_gt(np.stack([A, B, C]), [0, 3], K, full, 15.0)
    assert out["px_count"][2].tolist() == [6, 6, 0]
    assert out["bbox_obj"][2].tolist() == [-1] * 4 and out["bbox_visib"][2].tolist() == [-1] * 4
    assert (out["id_image"] == 3).sum() == 0
    # a 3 x 2 window at (1, 1): counts of the canvas and of the window, boxes in window coordinates
    Kw = K.copy()
    Kw[0, 2] -= 1
    Kw[1, 2] -= 1
    out = SN.scene_gt(np.stack([A, C]), [0, 2], Kw, None, 15.0, window=(1, 1, 3, 2))
    assert out["scene_depth"][0].tolist() == [[500, 500, 0], [900, 900, 0]]
    assert out["px_count"].tolist() == [[5, 2, 2], [6, 4, 2]]
    assert out["bbox_obj"].tolist() == [[-1, -1, 2, 1], [-1, 0, 2, 1]] and out["bbox_visib"].tolist() == [[0, 0, 1, 0], [0, 1, 1, 0]]
    assert out["id_image"][0].tolist() == [[1, 1, 0], [2, 2, 0]]


def pose(obj_id, tag, bop=False):
    R, t = np.eye(3) * tag, [tag, tag + 0.25, tag + 0.5]
    return {"obj_id": obj_id, "cam_R_m2c": list(R.reshape(-1)), "cam_t_m2c": t} if bop else {"obj_id": obj_id, "R": R, "t": t}


def test_instances_of_interleaved_meshes_come_back_in_scene_order():
    from pyrapose_amd.utils import scene_gt as SG
    scenes = [[pose(7, 1), pose(3, 2, bop=True), pose(7, 3), pose(3, 4)], [], [pose(3, 5), pose(9, 6, bop=True)]]
    plan = SG.plan_instances(scenes)
    assert plan.scene_offsets.tolist() == [0, 4, 4, 6] and plan.scene_offsets.dtype == np.int32
    assert plan.scene_of.tolist() == [0, 0, 0, 0, 2, 2] and plan.obj_ids == [7, 3, 7, 3, 3, 9]
    assert list(plan.groups.items()) == [(7, [0, 2]), (3, [1, 3, 4]), (9, [5])]
    assert plan.R.shape == (6, 3, 3) and plan.t.shape == (6, 3) and plan.t[:, 0].tolist() == [1, 2, 3, 4, 5, 6]
    assert np.array_equal(plan.R[1], np.eye(3) * 2)                                  # BOP's flat cam_R_m2c
    # what the device does with it: one render per mesh, concatenated, then one gather
    renders = [plan.t[idx, 0] for idx in plan.groups.values()]
    assert np.concatenate(renders).tolist() == [1, 3, 2, 4, 5, 6]
    assert np.concatenate(renders)[plan.order].tolist() == [1, 2, 3, 4, 5, 6]
    empty = SG.plan_instances([[], []])
    assert empty.scene_offsets.tolist() == [0, 0, 0] and empty.R.shape == (0, 3, 3) and empty.order.shape == (0,)


def test_annotations_from_scene():
    from pyrapose_amd.utils import scene_gt as SG
    info = [{"bbox_obj": [0, 0, 9, 9], "bbox_visib": [2, 3, 4, 5], "px_count_all": 40, "px_count_valid": 40, "px_count_visib": 10,
             "visib_fract": 0.25},
            {"bbox_obj": [-1] * 4, "bbox_visib": [-1] * 4, "px_count_all": 7, "px_count_valid": 7, "px_count_visib": 0, "visib_fract": 0.0},
            {"bbox_obj": [1, 1, 2, 2], "bbox_visib": [1, 1, 2, 1], "px_count_all": 6, "px_count_valid": 0, "px_count_visib": 6, "visib_fract": 1.0}]
    got = SG.annotations_from_scene(info, [5, 8, 5])
    assert got == [{"category_id": 5, "bbox": [2, 3, 4, 5], "area": 20, "mask_id": 1, "feature_visibility": 0.25},
                   {"category_id": 8, "bbox": [-1] * 4, "area": 1, "mask_id": 2, "feature_visibility": 0.0},
                   {"category_id": 5, "bbox": [1, 1, 2, 1], "area": 2, "mask_id": 3, "feature_visibility": 1.0}]
    # an excluded object keeps its number in the id image (annotate_BOP.py:372-388: the counter runs before the exclusions)
    assert [a["mask_id"] for a in SG.annotations_from_scene(info, [5, 8, 5], skip=(8,))] == [1, 3]
    with pytest.raises(ValueError):
        SG.annotations_from_scene(info, [5, 8])


def test_argument_errors_come_before_any_device_call():
    import torch
    from pyrapose_amd import ops
    from pyrapose_amd.utils import scene_gt as SG
    models = {3: {"pts": np.eye(3), "faces": np.array([[0, 1, 2]])}}
    scene = [[pose(3, 1)]]
    K3 = np.array([[100.0, 0.0, 4.0], [0.0, 100.0, 3.0], [0.0, 0.0, 1.0]])
    bad = [dict(extent="canvas"), dict(delta=-1.0), dict(delta=float("nan")), dict(scenes=[]), dict(scenes=[[pose(4, 1)]]),
           dict(scenes=[[{"obj_id": 3, "R": np.eye(3)}]]), dict(scenes=[[{"obj_id": 3, "R": np.eye(2), "t": [0, 0, 1]}]]),
           dict(scenes=[[pose(3, 1)] * 256]), dict(im_size=None), dict(im_size=(0, 6)), dict(K=np.eye(4)), dict(K=np.zeros((2, 3, 3))),
           dict(depth=np.zeros((2, 6, 8))), dict(depth=np.zeros(8)), dict(depth=np.zeros((6, 8)), im_size=(8, 7))]
    for kw in bad:
        args = dict(scenes=scene, models=models, K=K3, depth=None, im_size=(8, 6))
        args.update(kw)
        with pytest.raises(ValueError):
            SG.scene_gt_info(**args)
    # no instance at all needs no device either
    out = SG.scene_gt_info([[], []], models, K3, im_size=(8, 6), masks=True)
    assert out.info == [[], []] and out.id_images.shape == (2, 6, 8) and not out.id_images.any() and out.depth.shape == (2, 6, 8)
    assert [m.shape for m in out.mask_visib] == [(0, 6, 8)] * 2
    # the device wrapper looks at its tensors before it calls the library
    with pytest.raises(ValueError):
        ops.scene_gt_info(None, torch.zeros((1, 6, 8)), [0, 1], torch.zeros((1, 4), dtype=torch.float64))
    assert ops.SCENE_GT_MAX_INSTANCES == 255
