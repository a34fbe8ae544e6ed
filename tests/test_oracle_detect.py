"""CPU: hand tables for the numpy restatement of filter_detections (oracle/detect_np.py), the reference of the three filter
kernels (tests/test_gpu_detect.py).  TensorFlow is not installed ("parity unpinned"): every expectation below is worked out
by hand from the published rules -- IoU on sorted corners, suppress when IoU > threshold, scores > threshold, ties to the
lower index / the earlier position -- and none is computed by the oracle."""
import numpy as np

from oracle import detect_np as D

F = np.float32


def test_tf_iou_hand_values():
    a, b = F([0, 0, 10, 10]), F([0, 0, 10, 5])
    # areas 100 and 50, intersection 10 x 5 = 50, union 100 + 50 - 50 = 100 -> exactly 0.5
    assert D.tf_iou(a, b) == F(0.5) and D.tf_iou(b, a) == F(0.5)
    assert D.tf_iou(F([10, 10, 0, 0]), b) == F(0.5) and D.tf_iou(a, F([10, 5, 0, 0])) == F(0.5)   # reversed corners
    assert D.tf_iou(a, a) == F(1)
    assert D.tf_iou(a, F([3, 3, 3, 8])) == 0 and D.tf_iou(F([3, 3, 8, 3]), a) == 0                # zero area
    assert D.tf_iou(a, F([0, 10, 10, 20])) == 0 and D.tf_iou(a, F([20, 20, 30, 30])) == 0         # touching / apart
    # 4 x 4 against the same box moved by (1, 1): intersection 3 x 3 = 9, union 16 + 16 - 9 = 23
    assert D.tf_iou(F([0, 0, 4, 4]), F([1, 1, 5, 5])) == F(9) / F(23)


def test_tf_iou_many_is_tf_iou_row_by_row():
    rng = np.random.default_rng(0)
    B = rng.uniform(0, 40, size=(200, 4)).astype(F)      # corners in any order
    B[::7, 2] = B[::7, 0]                                # zero height
    B[3::11, 3] = B[3::11, 1]                            # zero width
    for a in (B[0], B[1], B[7], B[14], F([0, 0, 10, 10])):
        want = np.array([D.tf_iou(a, b) for b in B], F)
        assert D.tf_iou_many(a, B).tobytes() == want.tobytes()
    assert D.tf_iou_many(B[1], B[:0]).shape == (0,)


def test_nms_hand_cases():
    big, half = [0, 0, 10, 10], [0, 0, 10, 5]            # IoU exactly 0.5 (above)
    far = [50, 50, 60, 60]
    boxes = F([big, half, far])
    # suppression is IoU > threshold: at 0.5 the pair survives, at 0.49 the lower score goes
    assert list(D.non_max_suppression(boxes, F([0.9, 0.8, 0.7]), 10, 0.5)) == [0, 1, 2]
    assert list(D.non_max_suppression(boxes, F([0.9, 0.8, 0.7]), 10, 0.49)) == [0, 2]
    assert list(D.non_max_suppression(boxes, F([0.8, 0.9, 0.7]), 10, 0.49)) == [1, 2]
    # equal scores: the lower index is visited first, so it is the one that stays
    assert list(D.non_max_suppression(boxes, F([0.6, 0.6, 0.6]), 10, 0.49)) == [0, 2]
    assert list(D.non_max_suppression(boxes[[1, 0, 2]], F([0.6, 0.6, 0.6]), 10, 0.49)) == [0, 2]
    assert list(D.non_max_suppression(boxes, F([0.6, 0.6, 0.6]), 10, 0.5)) == [0, 1, 2]
    # max_output_size cuts the list after the best
    assert list(D.non_max_suppression(boxes, F([0.7, 0.8, 0.9]), 2, 0.5)) == [2, 1]
    assert list(D.non_max_suppression(boxes, F([0.7, 0.8, 0.9]), 1, 0.5)) == [2]
    assert len(D.non_max_suppression(boxes[:0], F([]), 5, 0.5)) == 0


def _five():
    """five pairwise disjoint boxes in a row; boxes3d row i holds 100 + i"""
    boxes = F([[0, 20 * i, 10, 20 * i + 10] for i in range(5)])
    boxes3d = np.repeat(F(100) + np.arange(5, dtype=F)[:, None], 16, axis=1)
    return boxes, boxes3d


def test_filter_detections_hand_table():
    boxes, boxes3d = _five()
    sc = F([[0.9, 0.5, 0.7, 0.1, 0.7],      # class 0: 0.5 equals the threshold -> out; candidates 0, 2, 4
            [0.5, 0.4, 0.0, 0.3, 0.2],      # class 1: nothing above the threshold -> skipped
            [0.7, 0.8, 0.2, 0.9, 0.3]]).T   # class 2: candidates 0, 1, 3
    # per-class selection order (score down, index up): class 0 -> 0, 2, 4; class 2 -> 3, 1, 0
    # concatenated positions: 0:(a0,c0,.9) 1:(a2,c0,.7) 2:(a4,c0,.7) 3:(a3,c2,.9) 4:(a1,c2,.8) 5:(a0,c2,.7)
    # top-k, score down and position up: positions 0, 3, 4, 1, 2, 5
    anchors, labels = [0, 3, 1, 2, 4, 0], [0, 2, 2, 0, 0, 2]
    scores = F([0.9, 0.9, 0.8, 0.7, 0.7, 0.7])
    ob, o3, osc, ol = D.filter_detections(boxes, boxes3d, sc, 0.5, 8, 0.5)
    assert ob.shape == (8, 4) and o3.shape == (8, 16) and osc.shape == (8,) and ol.shape == (8,) and ol.dtype == np.int32
    assert np.array_equal(ob[:6], boxes[anchors]) and np.array_equal(o3[:6], boxes3d[anchors])
    assert np.array_equal(osc[:6], scores) and list(ol[:6]) == labels
    assert np.all(ob[6:] == -1) and np.all(o3[6:] == -1) and np.all(osc[6:] == -1) and np.all(ol[6:] == -1)   # padding
    # max_detections = 4 cuts the same list, and limits each class's NMS to 4 as well (no change here: 3 per class)
    ob, o3, osc, ol = D.filter_detections(boxes, boxes3d, sc, 0.5, 4, 0.5)
    assert np.array_equal(ob, boxes[anchors[:4]]) and np.array_equal(osc, scores[:4]) and list(ol) == labels[:4]
    # max_detections = 2: class 0 keeps 0, 2 and class 2 keeps 3, 1 -> positions 0:(a0,.9) 1:(a2,.7) 2:(a3,.9) 3:(a1,.8)
    ob, o3, osc, ol = D.filter_detections(boxes, boxes3d, sc, 0.5, 2, 0.5)
    assert np.array_equal(ob, boxes[[0, 3]]) and np.array_equal(o3, boxes3d[[0, 3]]) and list(ol) == [0, 2]
    # nothing anywhere: all four outputs are padding
    for out in D.filter_detections(boxes, boxes3d, sc, 0.95, 3, 0.5):
        assert np.all(out == -1)


def test_filter_detections_signed_zero_scores_tie():
    """-0.0 == +0.0: with a negative threshold four disjoint boxes scored [-0, +0, -0, +0] are four equal scores and come
    out in index order"""
    boxes, boxes3d = _five()
    sc = F([-0.0, 0.0, -0.0, 0.0]).reshape(4, 1)
    ob, o3, osc, ol = D.filter_detections(boxes[:4], boxes3d[:4], sc, -1.0, 4, 0.5)
    assert np.array_equal(ob, boxes[:4]) and np.array_equal(o3, boxes3d[:4])
    assert np.all(osc == 0) and list(ol) == [0, 0, 0, 0]
