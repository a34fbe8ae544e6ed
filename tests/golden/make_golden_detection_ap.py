#!/usr/bin/env python3
"""Golden vectors for the 2-D detection average precision (test infrastructure, runs ONLY in the build container).

Loads the reference's unmodified ``PyraPose/utils/eval.py`` from /root/reference into the scratch package make_golden.py
builds (its symlinked ``anchors.py`` and the reference's own ``compute_overlap.pyx`` cythonized there, nothing copied into this
repository), with stub modules for ``keras`` (``backend.image_data_format() -> 'channels_last'``), ``cv2``, ``progressbar`` (a
``progressbar.progressbar`` that returns its iterable) and ``.visualization`` (drawing is never reached: save_path is None).
Calls the reference's ``evaluate`` with the duck-typed generator and model of tests/det_eval_np.py, which serve seeded
synthetic detections and annotations, and writes tests/golden/detection_ap.npz: the inputs, the per-image detections the
reference selects (score threshold, best max_detections) and the returned (average_precision, num_annotations) per label.

The inputs stay where the reference is well defined: all detection scores of one class are distinct (its unstable
np.argsort(-scores) leaves ties undefined) and every box is float64 (its Cython overlap rejects float32); both are asserted.
The overlap is the Cython build, not a stand-in.  Nothing under tests/ with ``-m gpu`` reads /root/reference.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
from det_eval_np import FakeGenerator, FakeModel  # noqa: E402

REF = make_golden.REF
N_IMG, N_RAW, N_CLASS, MAX_DET, SCORE_THR, IOU_THR, SCALE = 14, 48, 6, 24, 0.05, 0.5, 2.0


def load_reference():
    ref_anchors, _overlap = make_golden.import_reference()
    utils = os.path.dirname(ref_anchors.__file__)
    os.symlink(os.path.join(REF, "PyraPose/utils/eval.py"), os.path.join(utils, "eval.py"))
    sys.modules["keras"].backend.image_data_format = lambda: "channels_last"
    pb = types.ModuleType("progressbar")
    pb.progressbar = lambda it, **kw: it
    sys.modules["progressbar"] = pb
    vis = types.ModuleType("PyraPose.utils.visualization")
    vis.draw_detections = vis.draw_annotations = None
    sys.modules["PyraPose.utils.visualization"] = vis
    import PyraPose.utils.eval as ref_eval
    return ref_eval


def make_inputs(rng):
    """classes 0..3 have annotations and detections; class 4 has detections only; class 5 (has_label False) has both and is
    reported nowhere.  Detections: jittered copies of ground truth (some twice: a duplicate is a false positive), shifted
    copies around the IoU threshold, and clutter; raw scores are distinct over the whole set, some below the score threshold;
    unused raw slots carry label -1 and score -1 as layers.FilterDetections pads them."""
    gt_boxes, gt_labels, gt_offsets = [], [], [0]
    boxes = np.zeros((N_IMG, N_RAW, 4), np.float64)
    labels = np.full((N_IMG, N_RAW), -1, np.int64)
    scores = np.full((N_IMG, N_RAW), -1.0, np.float64)
    pool = rng.permutation(N_IMG * N_RAW)  # distinct score ranks
    for i in range(N_IMG):
        n_gt = 0 if i == 3 else int(rng.integers(1, 9))
        xy = rng.integers(0, 500, size=(n_gt, 2)).astype(np.float64)
        wh = rng.integers(20, 120, size=(n_gt, 2)).astype(np.float64)
        g = np.concatenate([xy, xy + wh], axis=1)
        gl = rng.choice([0, 1, 2, 3, 5], size=n_gt)
        gt_boxes.append(g)
        gt_labels.append(gl)
        gt_offsets.append(gt_offsets[-1] + n_gt)
        k = 0
        for j in range(n_gt):
            for _ in range(int(rng.integers(0, 4))):  # 0..3 detections per ground truth
                shift = rng.choice([0.0, 2.0, 0.25, 0.5]) * wh[j] * rng.choice([-1.0, 1.0], size=2)
                boxes[i, k] = g[j] + np.concatenate([shift, shift]) + rng.integers(-3, 4, size=4)
                labels[i, k] = gl[j] if rng.uniform() < 0.85 else rng.integers(0, N_CLASS)
                k += 1
        for _ in range(int(rng.integers(2, 12)) if i != 5 else 0):  # clutter; image 5 has detections of ground truth only
            xy1 = rng.integers(0, 500, size=2).astype(np.float64)
            boxes[i, k] = np.concatenate([xy1, xy1 + rng.integers(20, 120, size=2)])
            labels[i, k] = rng.integers(0, N_CLASS)
            k += 1
        assert k <= N_RAW
        if i == 7:  # an image that exceeds max_detections
            while k < N_RAW - 4:
                xy1 = rng.integers(0, 500, size=2).astype(np.float64)
                boxes[i, k] = np.concatenate([xy1, xy1 + rng.integers(20, 120, size=2)])
                labels[i, k] = rng.integers(0, N_CLASS)
                k += 1
        scores[i, :k] = (pool[i * N_RAW:i * N_RAW + k] + 1.0) / (N_IMG * N_RAW + 1.0)
        perm = rng.permutation(N_RAW)  # the padding sits anywhere
        boxes[i], labels[i], scores[i] = boxes[i, perm], labels[i, perm], scores[i, perm]
    has_label = np.array([1, 1, 1, 1, 1, 0], np.uint8)
    return (boxes * SCALE, scores, labels, np.concatenate(gt_boxes), np.concatenate(gt_labels).astype(np.int64),
            np.asarray(gt_offsets, np.int32), has_label)


def main():
    ref = load_reference()
    rng = np.random.default_rng(20261019)
    raw_boxes, raw_scores, raw_labels, gt_boxes, gt_labels, gt_offsets, has_label = make_inputs(rng)
    assert raw_boxes.dtype == np.float64 and gt_boxes.dtype == np.float64, "the reference's Cython overlap rejects float32"
    live = raw_scores > SCORE_THR
    for c in range(N_CLASS):
        s = raw_scores[live & (raw_labels == c)]
        assert np.unique(s).size == s.size, "tied scores within a class: the reference's argsort is undefined there"
    gen = FakeGenerator(gt_boxes, gt_labels, gt_offsets, has_label, SCALE)
    res = ref.evaluate(gen, FakeModel(raw_boxes, raw_scores, raw_labels), iou_threshold=IOU_THR, score_threshold=SCORE_THR,
                       max_detections=MAX_DET)
    labels_out = np.array(sorted(res), np.int32)
    ap = np.array([float(res[l][0]) for l in labels_out], np.float64)
    num = np.array([float(res[l][1]) for l in labels_out], np.float64)
    # the detections evaluate() selects per image (eval.py:86-101), padded to max_detections with label -1
    det_boxes = np.zeros((N_IMG, MAX_DET, 4), np.float64)
    det_scores = np.zeros((N_IMG, MAX_DET), np.float64)
    det_labels = np.full((N_IMG, MAX_DET), -1, np.int32)
    for i in range(N_IMG):
        idx = np.where(raw_scores[i] > SCORE_THR)[0]
        idx = idx[np.argsort(-raw_scores[i, idx])[:MAX_DET]]
        det_boxes[i, :idx.size] = raw_boxes[i, idx] / SCALE
        det_scores[i, :idx.size] = raw_scores[i, idx]
        det_labels[i, :idx.size] = raw_labels[i, idx]
    out = dict(raw_boxes=raw_boxes, raw_scores=raw_scores, raw_labels=raw_labels.astype(np.int32), gt_boxes=gt_boxes,
               gt_labels=gt_labels.astype(np.int32), gt_offsets=gt_offsets, has_label=has_label, scale=np.float64(SCALE),
               iou_threshold=np.float64(IOU_THR), score_threshold=np.float64(SCORE_THR), max_detections=np.int32(MAX_DET),
               det_boxes=det_boxes, det_scores=det_scores, det_labels=det_labels, labels=labels_out, ap=ap, num_annotations=num)
    path = os.path.join(HERE, "detection_ap.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for l, a, n in zip(labels_out, ap, num):
        print("label %d: ap %.17g, %g annotations" % (l, a, n))


if __name__ == "__main__":
    main()
