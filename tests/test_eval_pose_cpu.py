"""CPU (no GPU): the per-image loop shared by utils.eval_pose.evaluate_add and evaluate_pose_metrics (_scored_images) on a stub
generator, with pose_decode.poses_from_outputs replaced by scripted detections: which images are decoded, which detections
survive, how they are paired with annotations, and when depth is loaded."""
import numpy as np
import pytest

from pyrapose_amd.utils import eval_pose

K_FIXED = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
QUAT = [1.0, 0.0, 0.0, 0.0]
# annotations per image: labels and poses (x, y, z in millimetres, then a unit quaternion)
ANNOS = [
    dict(labels=[], poses=[]),                                                    # 0: no labels
    dict(labels=[2], poses=[[0.0, 0.0, 800.0] + QUAT]),                           # 1: class 1 is detected, only class 2 annotated
    dict(labels=[3, 1, 3], poses=[[100.0, 0.0, 800.0] + QUAT, [0.0, 0.0, 700.0] + QUAT, [-100.0, 0.0, 800.0] + QUAT]),  # 2
]


def det(cls, t, instance=0):
    return dict(cls=cls, R=np.eye(3), t=np.asarray(t, np.float64), ok=True, instance=instance)


# scripted detections per image (metres): image 2 has three detections of class 3 -- near annotation 2, far from both, near
# annotation 0 -- and one of class 1
DETS = {
    1: [det(1, [0.0, 0.0, 0.8])],
    2: [det(1, [0.0, 0.0, 0.7]), det(3, [-0.101, 0.0, 0.8], 0), det(3, [0.5, 0.5, 0.8], 1), det(3, [0.102, 0.0, 0.8], 2)],
}


class Gen:
    def size(self):
        return len(ANNOS)

    def load_image(self, i):
        return np.full((4, 4, 3), i, np.float32)

    def preprocess_image(self, im):
        return im

    def resize_image(self, im):
        return im, 1.0

    def load_annotations(self, i):
        return ANNOS[i]


def run(monkeypatch, K, instances, load_depth=None):
    decoded = []

    def scripted(boxes3D, scores, threeD_boxes, Kc, **kw):
        index = int(boxes3D[0, 0, 0, 0])
        decoded.append((index, np.array(Kc), kw))
        return [dict(d) for d in DETS[index]]

    monkeypatch.setattr(eval_pose.pose_decode, "poses_from_outputs", scripted)
    predict = lambda x: (x, None, None)                                           # the image carries its index to `scripted`
    decode_kw = dict(threeD_boxes=None, threshold=0.5, min_votes=10, seed=40, weighting=None)
    out = list(eval_pose._scored_images(Gen(), predict, decode_kw, K, None, load_depth, None, 0.001, instances))
    return out, decoded


@pytest.mark.parametrize("instances", [None, {}])
def test_images_detections_and_pairs(monkeypatch, instances):
    out, decoded = run(monkeypatch, K_FIXED, instances)
    assert [i for i, _K, _kw in decoded] == [1, 2]                                # the image without labels is not decoded
    assert [kw["seed"] for _i, _K, kw in decoded] == [41, 42] and all(kw["instances"] is instances for _i, _K, kw in decoded)
    assert [o[0] for o in out] == [1, 2] and [o[1] for o in out] == [[2], [3, 1, 3]]
    assert all(o[2] is ANNOS[o[0]] and np.array_equal(o[3], K_FIXED) and o[4] is None for o in out)
    assert out[0][6] == []                                                        # class 1 is not annotated in image 1: dropped
    got = [(cls, [(d["instance"], gi) for d, gi in pairs]) for cls, pairs in out[1][6]]
    if instances is None:   # every detection against the first annotation of its class
        assert got == [(1, [(0, 1)]), (3, [(0, 0), (1, 0), (2, 0)])]
    else:                   # one to one by translation error, in detection order; the far detection stays unmatched
        assert got == [(1, [(0, 1)]), (3, [(0, 2), (2, 0)])]


def test_callable_K_and_depth_only_where_a_detection_survives(monkeypatch):
    loaded = []

    def load_depth(i):
        loaded.append(i)
        return np.full((2, 2), i, np.uint16)

    out, decoded = run(monkeypatch, lambda i: K_FIXED * (1.0 + i), None, load_depth)
    assert [np.array_equal(Kc, K_FIXED * (1.0 + i)) for i, Kc, _kw in decoded] == [True, True]
    assert [np.array_equal(o[3], K_FIXED * (1.0 + o[0])) for o in out] == [True, True]
    assert loaded == [2]                                                          # image 1: no surviving detection, no depth
    assert out[0][4] is None and np.array_equal(out[1][4], np.full((2, 2), 2))
