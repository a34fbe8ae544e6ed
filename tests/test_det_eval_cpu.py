"""CPU (no GPU): the numpy restatement of the detection metrics (tests/det_eval_np.py) against the reference's own `evaluate`
through tests/golden/detection_ap.npz (made by tests/golden/make_golden_detection_ap.py from the unmodified utils/eval.py and
the reference's Cython overlap); utils.eval._compute_ap on hand-made curves; the two mean rules of callbacks.Evaluate; the ABI
of the three entry points."""
import os
import re
import warnings

import numpy as np
import pytest

import det_eval_np as DN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DET_ENTRIES = ("pp_det_match", "pp_det_pr_curve", "pp_det_ap")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "detection_ap.npz"))


@pytest.fixture(scope="module")
def restated(fixture):
    z = fixture
    return DN.evaluate(z["det_boxes"], z["det_scores"], z["det_labels"], z["gt_boxes"], z["gt_labels"], z["gt_offsets"],
                       len(z["has_label"]), [float(z["iou_threshold"])], "reference", "area")


def test_fixture_is_where_the_reference_is_defined(fixture):
    z = fixture
    assert z["det_boxes"].dtype == np.float64 and z["gt_boxes"].dtype == np.float64
    for c in range(len(z["has_label"])):
        s = z["det_scores"][z["det_labels"] == c]
        assert np.unique(s).size == s.size
    # the cases the fixture is there for: a label without annotations, one the generator does not have, an empty image,
    # an image cut at max_detections, several true positives
    assert 0.0 in z["num_annotations"] and not z["has_label"].all() and (np.diff(z["gt_offsets"]) == 0).any()
    assert ((z["det_labels"] >= 0).sum(axis=1) == int(z["max_detections"])).any()
    assert (z["ap"] > 0).sum() >= 3


def test_restatement_reproduces_the_reference(fixture, restated):
    z = fixture
    assert [int(l) for l in z["labels"]] == [c for c in range(len(z["has_label"])) if z["has_label"][c]]
    for l, ap_ref, num_ref in zip(z["labels"], z["ap"], z["num_annotations"]):
        n = int((z["det_labels"] == l).sum())
        assert float(restated["npos"][l]) == num_ref
        # Both sides add the same terms (r_j - r_j-1) * p_j: the recalls are the same quotients tp / npos, the envelope the same
        # maxima, so the terms agree bit for bit; only the ORDER of the sum differs (np.sum's pairwise tree there, contiguous
        # partials and a halving tree here).  There are at most n terms (one per detection of the class), each in [0, 1] and
        # the exact sum S <= 1 (the recall steps add up to at most 1, the precision is at most 1).  Any summation order of n
        # terms errs by at most (n - 1) u sum|x_i| + O(u^2) with u = 2^-53, so two orders differ by at most
        # 2 (n - 1) 2^-53 S < n 2^-52.
        assert abs(restated["ap"][0, l] - ap_ref) <= n * 2.0 ** -52, (l, restated["ap"][0, l], ap_ref)


def test_restatement_agrees_with_compute_ap(fixture, restated):
    """the kernel-order sum against the reference's formula applied to the same curves"""
    from pyrapose_amd.utils.eval import _compute_ap
    offs = restated["class_offsets"]
    for c in range(len(fixture["has_label"])):
        lo, hi = offs[c], offs[c + 1]
        if restated["npos"][c] == 0:
            continue
        keep = slice(lo, hi)
        tp, fp = restated["tp"][0, keep].astype(np.float64), restated["fp"][0, keep].astype(np.float64)
        ref = _compute_ap(tp / float(restated["npos"][c]), tp / np.maximum(tp + fp, np.finfo(np.float64).eps))
        assert abs(restated["ap"][0, c] - ref) <= max(hi - lo, 1) * 2.0 ** -52


def test_linspace_is_the_kernels_recall_grid():
    assert np.array_equal(np.linspace(0.0, 1.0, 101), np.array([k * 0.01 for k in range(100)] + [1.0]))


@pytest.mark.parametrize("recall, precision, expect", [
    ([], [], 0.0),                                                   # empty: only the sentinels, (1 - 0) * 0
    ([0.5], [1.0], 0.5),                                             # a single point
    ([0.25, 0.25, 0.5, 0.75], [1.0, 0.5, 2.0 / 3.0, 0.75], 0.25 * 1.0 + 0.25 * 0.75 + 0.25 * 0.75),  # precision rises: envelope
    ([0.5, 0.5, 0.5, 1.0], [1.0, 0.5, 1.0 / 3.0, 0.5], 0.5 * 1.0 + 0.5 * 0.5),                       # recall with repeats
])
def test_compute_ap_hand_made(recall, precision, expect):
    from pyrapose_amd.utils.eval import _compute_ap
    got = _compute_ap(np.array(recall, np.float64), np.array(precision, np.float64))
    assert got == expect
    # the restated kernel order on the same curve (envelope applied as the curve kernel does)
    if len(recall):
        env = np.maximum.accumulate(np.array(precision)[::-1])[::-1]
        assert DN.ap_area(np.array(recall), env) == expect


class _Gen(object):
    def label_to_name(self, label):
        return "c%d" % label


def test_evaluate_callback_mean_rules(monkeypatch):
    from pyrapose_amd import callbacks
    from pyrapose_amd.utils import eval as UE
    fake = {0: (0.5, 10.0), 1: (0.25, 30.0), 2: (0, 0)}  # one class without annotations
    seen = {}

    def fake_evaluate(generator, model, **kw):
        seen.update(kw, model=model)
        return fake

    monkeypatch.setattr(UE, "evaluate", fake_evaluate)
    cb = callbacks.Evaluate(_Gen(), iou_threshold=0.6, score_threshold=0.1, max_detections=50, verbose=0)
    cb.set_model("the model")
    logs = {}
    cb.on_epoch_end(0, logs)
    assert logs["mAP"] == cb.mean_ap == (0.5 + 0.25 + 0) / 2  # the class without annotations adds 0 and is not counted
    assert seen == dict(model="the model", iou_threshold=0.6, score_threshold=0.1, max_detections=50, save_path=None)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        cbw = callbacks.Evaluate(_Gen(), weighted_average=True, tensorboard=object(), verbose=0)
    assert len(w) == 1
    logs = {}
    cbw.on_epoch_end(3, logs)
    assert logs["mAP"] == cbw.mean_ap == (10.0 * 0.5 + 30.0 * 0.25 + 0 * 0) / (10.0 + 30.0 + 0)


def test_evaluate_refuses_save_path():
    from pyrapose_amd.utils.eval import evaluate
    with pytest.raises(NotImplementedError):
        evaluate(None, None, save_path="somewhere")


def test_bop_ignore():
    from pyrapose_amd.utils.eval import bop_ignore
    assert bop_ignore(np.array([0.0, 0.05, 0.1, 0.9])).tolist() == [1, 1, 0, 0]


def test_det_entry_points_declared_and_exported():
    from pyrapose_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "pyrapose_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in DET_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.EXPORTS and hasattr(_lib.lib, name)
    consts = dict(re.findall(r"#define (PP_DET_[A-Z0-9_]+) (\d+)", code))
    assert (ops.DET_MAX_THR, ops.DET_MAX_DET, ops.DET_MAX_GT, ops.DET_SCAN_CHUNK) == tuple(
        int(consts[k]) for k in ("PP_DET_MAX_THR", "PP_DET_MAX_DET", "PP_DET_MAX_GT", "PP_DET_SCAN_CHUNK"))
    assert ops.DET_MAX_DET >= 1024 and ops.DET_MAX_GT >= 1024
    assert ops.DET_RULES == {"reference": int(consts["PP_DET_RULE_REFERENCE"]), "coco": int(consts["PP_DET_RULE_COCO"])}
    assert ops.DET_INTEGRATIONS == {"area": int(consts["PP_DET_AP_AREA"]), "101": int(consts["PP_DET_AP_101"])}
    # host-side refusals of the C ABI need no device: a NULL context first, as everywhere
    assert _lib.lib.pp_det_match(None, 1, 0, 0, 1, None, None, None, None, None, None, None, None, 1, None, 0, None, None, None) == -4
