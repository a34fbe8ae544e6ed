"""Host side of utils/model_info.py: the 3-D box corners in the reference's order (annotation_scripts/annotate_BOP.py:204-219
restated in tests/model_info_np.py), models_info.json written and read back, and the restatement's two diameter forms."""
import math

import numpy as np
import pytest

from tests import model_info_np as MN

INFO = {1: dict(diameter=7.5, min_x=-1.0, min_y=-2.0, min_z=-3.0, size_x=2.0, size_y=4.0, size_z=6.0),
        "3": dict(diameter=102.099, min_x=-37.9343, min_y=-38.7996, min_z=-45.8845, size_x=75.8686, size_y=77.5992, size_z=91.769)}


def test_boxes_have_the_reference_corner_order_at_the_index_of_the_key():
    from pyrapose_amd.utils.model_info import threeD_boxes
    boxes = threeD_boxes(INFO)
    assert boxes.dtype == np.float32 and boxes.shape == (4, 8, 3)
    want = [[1, 2, 3], [1, 2, -3], [1, -2, -3], [1, -2, 3], [-1, 2, 3], [-1, 2, -3], [-1, -2, -3], [-1, -2, 3]]
    assert np.array_equal(boxes[1], np.array(want, np.float32))
    assert not boxes[0].any() and not boxes[2].any()
    assert np.array_equal(boxes, MN.three_boxes_np(INFO, 4))
    v = INFO["3"]
    assert boxes[3, 0, 0] == np.float32(v["size_x"] + v["min_x"]) and boxes[3, 6, 2] == np.float32(v["min_z"])
    wide = threeD_boxes(INFO, n_classes=6)
    assert wide.shape == (6, 8, 3) and np.array_equal(wide[:4], boxes) and not wide[4:].any()
    with pytest.raises(ValueError):
        threeD_boxes(INFO, n_classes=3)


def test_scale_is_the_reference_factor():
    from pyrapose_amd.utils.model_info import threeD_boxes
    got = threeD_boxes(INFO, scale=0.001)
    assert np.array_equal(got, MN.three_boxes_np(INFO, 4, fac=0.001))
    assert np.allclose(got, threeD_boxes(INFO) * 0.001, rtol=1e-6, atol=0.0)


def test_models_info_round_trip_and_symmetries(tmp_path):
    from pyrapose_amd.utils.model_info import save_models_info
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations, load_models_info
    info = {int(k): v for k, v in INFO.items()}
    info[7] = dict(diameter=math.sqrt(2.0) / 3.0, min_x=-0.1, min_y=1e-300, min_z=-1.0 / 3.0, size_x=0.2, size_y=1e300, size_z=2.0 / 3.0)
    path = str(tmp_path / "models_info.json")
    save_models_info(path, info)
    back = load_models_info(path)
    assert back == info and all(isinstance(k, int) for k in back)
    for entry in back.values():
        syms = get_symmetry_transformations(entry)
        assert len(syms) == 1 and np.array_equal(syms[0]["R"], np.eye(3)) and not syms[0]["t"].any()


def test_min_dist_is_refused_under_the_min_rule():
    from pyrapose_amd.utils.model_info import farthest_points
    with pytest.raises(ValueError, match="min_dist belongs to rule 'sum'"):
        farthest_points(np.zeros((4, 3)), 2, "min", min_dist=1.0)
    with pytest.raises(ValueError, match="unknown rule"):
        farthest_points(np.zeros((4, 3)), 2, "max")


def test_the_two_restated_diameters_agree_bit_for_bit():
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(300, 3)) * (40.0, 25.0, 60.0) + (3.0, -2.0, 10.0)
    d2, pair = MN.diameter_np(pts, block=64)
    i, j = (int(v) for v in pair)
    assert i <= j and d2[0] == MN.d2_rows(pts[i:i + 1], pts[j:j + 1])[0, 0]
    assert math.sqrt(d2[0]) == MN.calc_pts_diameter_np(pts)
    assert np.array_equal(MN.diameter_np(pts, block=512)[0], d2) and np.array_equal(MN.diameter_np(pts, block=7)[1], pair)
