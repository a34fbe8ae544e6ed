"""The segmentation metrics without a device: the numpy restatement tests/mask_eval_np.py against a brute-force pixel loop, the
run-length strings against the reference's own rle_encode (tests/golden/mask_rle.npz, made by
tests/golden/make_golden_mask_rle.py), the encode -> decode round trip in both orders, the mask chain on filled rectangles
against the box chain under the COCO rule, the host arithmetic of utils.mask_eval, and the C ABI and argument checks of the new
entry points that need no device.  The device side is tests/test_gpu_mask_eval.py."""
import os
import re

import numpy as np
import pytest

import det_eval_np as DN
import mask_eval_np as MN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK_ENTRIES = ("pp_mask_confusion", "pp_mask_pack", "pp_mask_iou_pairs", "pp_det_match_iou", "pp_mask_rle_workspace_bytes", "pp_mask_rle",
                "pp_mask_from_rle")


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "mask_rle.npz"))


def rect_case(seed=5, B=3, D=6, n_gt=(0, 3, 5), n_class=2, H=24, W=40, ignore=True):
    """integer boxes inside a W x H image, at least 1 pixel wide and high; detections are shifted copies of ground truth or
    clutter; scores from a small set so that ties occur; one image without ground truth, one row with padding"""
    rng = np.random.default_rng(seed)
    gt_boxes, gt_labels = [], []
    det_boxes, det_scores = np.zeros((B, D, 4)), np.zeros((B, D))
    det_labels = np.full((B, D), -1, np.int32)
    for b in range(B):
        xy = np.stack([rng.integers(0, W - 12, n_gt[b]), rng.integers(0, H - 10, n_gt[b])], axis=1)
        g = np.concatenate([xy, xy + rng.integers(2, 10, size=(n_gt[b], 2))], axis=1).astype(np.float64)
        gl = rng.integers(0, n_class, n_gt[b]).astype(np.int32)
        gt_boxes.append(g)
        gt_labels.append(gl)
        for d in range(D if b != 1 else D - 2):
            if n_gt[b] and rng.uniform() < 0.7:
                j = rng.integers(0, n_gt[b])
                box = g[j] + np.array([1, 1, 1, 1]) * rng.integers(-1, 2) + np.array([0, 0, 1, 1]) * rng.integers(0, 2)
                det_labels[b, d] = gl[j]
            else:
                p = np.array([rng.integers(0, W - 12), rng.integers(0, H - 10)])
                box = np.concatenate([p, p + rng.integers(2, 10, 2)])
                det_labels[b, d] = rng.integers(0, n_class)
            det_boxes[b, d] = np.clip(box, 0, [W - 1, H - 1, W, H])
            det_boxes[b, d, 2:] = np.maximum(det_boxes[b, d, 2:], det_boxes[b, d, :2] + 1)
            det_scores[b, d] = rng.integers(1, 5) / 4.0
    offs = np.zeros(B + 1, np.int32)
    offs[1:] = np.cumsum(n_gt)
    case = dict(det_boxes=det_boxes, det_scores=det_scores, det_labels=det_labels, gt_boxes=np.concatenate(gt_boxes).reshape(-1, 4),
                gt_labels=np.concatenate(gt_labels), gt_offsets=offs, n_class=n_class, H=H, W=W)
    if ignore:
        case["gt_ignore"] = (rng.uniform(size=int(offs[-1])) < 0.3).astype(np.uint8)
    case["det_masks"] = MN.rect_masks(det_boxes.reshape(-1, 4), H, W).reshape(B, D, H, W)
    case["det_masks"][det_labels < 0] = 0
    case["gt_masks"] = MN.rect_masks(case["gt_boxes"], H, W)
    return case


def mask_chain_np(case, thresholds, rule, integration):
    """the mask AP chain in the restatement -> det_eval_np.evaluate's dict"""
    B, D = case["det_scores"].shape
    packed_d = MN.mask_pack(case["det_masks"].reshape(B * D, case["H"], case["W"]))
    packed_g = MN.mask_pack(case["gt_masks"])
    iou, _inter, _po = MN.mask_iou_pairs(packed_d, packed_g, case["gt_offsets"], D, case["det_labels"])
    match, ign, npos = MN.det_match_iou(iou, case["det_scores"], case["det_labels"], case["gt_labels"], case["gt_offsets"], case["n_class"],
                                        list(thresholds), rule, case.get("gt_ignore") if rule == "coco" else None)
    order, offs = DN.det_order(case["det_scores"], case["det_labels"], case["n_class"])
    tp, fp, recall, env = DN.pr_curve(order, offs, match, ign, npos)
    ap, rf = DN.det_ap(offs, npos, recall, env, integration)
    return dict(match=match, det_ignored=ign, npos=npos, order=order, class_offsets=offs, tp=tp, fp=fp, recall=recall, prec_env=env, ap=ap,
                recall_final=rf, iou=iou)


def test_packed_iou_equals_the_pixel_loop():
    rng = np.random.default_rng(0)
    H, W = 7, 19  # 133 pixels: three words, the last with 5 bits
    det = (rng.uniform(size=(5, H, W)) < 0.4).astype(np.uint8) * 3
    gt = (rng.uniform(size=(4, H, W)) < 0.5).astype(np.uint8)
    det[1] = 0                # an empty detection
    gt[2] = 0                 # and an empty ground truth: their pair has an empty union
    det[2, :] = 0
    det[2, 0, :5] = 1         # only the first word
    gt[3, :] = 0
    gt[3, -1, -5:] = 1        # only the last word: disjoint word ranges
    det[3] = gt[0]            # identical masks
    offs = np.array([0, 4])
    pd, pg = MN.mask_pack(det), MN.mask_pack(gt)
    assert pd[0].shape == (5, 3) and int(pd[0][0, 2]) < 1 << 5 and pd[1].tolist() == [int((m != 0).sum()) for m in det]
    assert pd[2][1].tolist() == [0, 0] and pd[2][2].tolist() == [0, 1] and pg[2][3].tolist() == [2, 3]
    iou, inter, po = MN.mask_iou_pairs(pd, pg, offs, 5)
    assert po.tolist() == [0, 20]
    for d in range(5):
        for g in range(4):
            assert iou[d * 4 + g] == MN.brute_iou(det[d], gt[g]), (d, g)
            assert inter[d * 4 + g] == int(((det[d] != 0) & (gt[g] != 0)).sum())
    assert iou[1 * 4 + 2] == 0.0 and iou[3 * 4 + 0] == 1.0 and iou[2 * 4 + 3] == 0.0


def test_rle_string_is_the_references():
    from pyrapose_amd.utils import mask_eval  # noqa: F401  (the module imports without a device)
    g = golden()
    assert len(g["masks"]) >= 12
    for m, s in zip(g["masks"], g["strings"]):
        assert MN.rle_string(m) == str(s)
    # the checkerboard that starts with a set pixel has the most runs a mask of its size can have: H W + 1
    assert max(len(MN.rle_counts(m, "row")) for m in g["masks"]) == g["masks"].shape[1] * g["masks"].shape[2] + 1


def test_rle_counts_edges():
    z, o = np.zeros((2, 3), np.uint8), np.ones((2, 3), np.uint8)
    assert MN.rle_counts(z, "row") == [6] and MN.rle_counts(o, "row") == [0, 6] and MN.rle_counts(o, "column") == [0, 6]
    m = np.array([[1, 0, 0], [0, 0, 1]], np.uint8)
    assert MN.rle_counts(m, "row") == [0, 1, 4, 1] and MN.rle_counts(m, "column") == [0, 1, 4, 1]
    m = np.array([[0, 1, 1], [0, 0, 1]], np.uint8)
    assert MN.rle_counts(m, "row") == [1, 2, 2, 1] and MN.rle_counts(m, "column") == [2, 1, 1, 2]
    board = (np.add.outer(np.arange(3), np.arange(5)) % 2 == 0).astype(np.uint8)  # starts with 1: H W + 1 runs
    assert MN.rle_counts(board, "row") == [0] + [1] * 15


@pytest.mark.parametrize("order", ["row", "column"])
def test_rle_round_trip(order):
    for m in golden()["masks"]:
        counts = MN.rle_counts(m, order)
        assert sum(counts) == m.size and all(c > 0 for c in counts[1:])
        assert np.array_equal(MN.mask_from_rle(counts, m.shape, order), m * 255)
    offs, flat = MN.mask_rle(golden()["masks"][:3], order)
    assert offs.tolist() == [0, 1, 3, 6] and flat.dtype == np.int32


def test_rectangle_masks_score_as_their_boxes_under_the_coco_rule():
    # integer corner boxes inside the image, x1 <= x < x2: the mask's area is (x2 - x1)(y2 - y1) and every intersection is
    # iw * ih, the integers iou_plain divides, so the IoU matrix, the match tables and the AP agree bit for bit
    case = rect_case()
    thr = list(np.linspace(0.5, 0.95, 10))
    want = DN.evaluate(case["det_boxes"], case["det_scores"], case["det_labels"], case["gt_boxes"], case["gt_labels"], case["gt_offsets"],
                       case["n_class"], thr, "coco", "101", case["gt_ignore"])
    got = mask_chain_np(case, thr, "coco", "101")
    assert (want["match"] >= 0).any() and want["det_ignored"].any()
    for k in ("match", "det_ignored", "npos", "tp", "fp", "recall", "prec_env", "ap", "recall_final"):
        assert np.array_equal(got[k], want[k]), k
    B, D = case["det_scores"].shape
    for b in range(B):
        g0, g1 = case["gt_offsets"][b], case["gt_offsets"][b + 1]
        for d in range(D):
            if case["det_labels"][b, d] >= 0 and g1 > g0:
                v = DN.iou_plain(case["det_boxes"][b, d], case["gt_boxes"][g0:g1])
                assert np.array_equal(got["iou"][D * g0 + d * (g1 - g0):D * g0 + (d + 1) * (g1 - g0)], v)


def test_confusion_restatement_and_scores():
    from pyrapose_amd.utils import mask_eval
    pred = np.array([[[0.5, 0.6], [np.nan, 0.4], [-0.0, 1.0], [0.7, 0.5000001]]], np.float32)
    target = np.array([[[1, 0, 1], [1, 1, 1], [0, 1, 1], [1, 0, 1]]], np.float32)
    c = MN.mask_confusion(pred, target, [0.0, 0.5])
    # threshold 0: -0 > 0 is false, NaN is not predicted; threshold 0.5: exactly 0.5 is not predicted
    assert c[0].tolist() == [[2, 0, 1], [2, 2, 0]] and c[1].tolist() == [[1, 0, 2], [1, 2, 1]]
    got = mask_eval.scores_from_counts(c)
    iou, prec, rec, miou = MN.scores(c)
    for k, w in (("iou", iou), ("precision", prec), ("recall", rec), ("miou", miou)):
        assert np.array_equal(got[k], w), k
    empty = mask_eval.scores_from_counts(np.zeros((1, 2, 3), np.int64))
    assert empty["iou"].tolist() == [[0.0, 0.0]] and empty["miou"].tolist() == [0.0]


def test_mask_entry_points_declared_and_exported():
    from pyrapose_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "pyrapose_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in MASK_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.EXPORTS and hasattr(_lib.lib, name)
    consts = dict(re.findall(r"#define (PP_MASK_[A-Z0-9_]+) (\d+)", code))
    assert ops.MASK_MAX_CLASS == int(consts["PP_MASK_MAX_CLASS"])
    assert ops.MASK_IOU_TILE == (int(consts["PP_MASK_IOU_TILE_DET"]), int(consts["PP_MASK_IOU_TILE_GT"])) == (MN.TILE_DET, MN.TILE_GT)
    assert (ops.MASK_ORDERS["row"], ops.MASK_ORDERS["column"]) == (int(consts["PP_MASK_ORDER_ROW"]), int(consts["PP_MASK_ORDER_COLUMN"]))
    lib = _lib.lib
    # a NULL context is refused first, as everywhere
    assert lib.pp_mask_confusion(None, 1, 1, 1, None, None, 1, None, None) == -4
    assert lib.pp_mask_pack(None, 1, 1, 1, None, None, None, None) == -4
    assert lib.pp_mask_iou_pairs(None, 1, 1, 0, 1, 1, None, None, None, None, None, None, None, None, None, None, None) == -4
    assert lib.pp_det_match_iou(None, 1, 0, 0, 1, None, None, None, None, None, None, None, 1, None, 1, None, None, None) == -4
    assert lib.pp_mask_rle(None, 1, 1, 1, 0, None, None, 0, 0, None, None, None) == -4
    assert lib.pp_mask_from_rle(None, 1, 1, 1, 0, None, None, None, None, None) == -4
    assert lib.pp_mask_rle_workspace_bytes(-1) == 0 and lib.pp_mask_rle_workspace_bytes(100) >= 400


def test_wrapper_argument_checks_need_no_device():
    import torch
    from pyrapose_amd import ops
    from pyrapose_amd.utils import mask_eval
    cpu_f32 = torch.zeros((1, 4, 2))
    with pytest.raises(ValueError, match="thresholds"):
        ops.mask_confusion(None, cpu_f32, cpu_f32, [])
    with pytest.raises(ValueError, match="thresholds"):
        ops.mask_confusion(None, cpu_f32, cpu_f32, [0.1] * 17)
    with pytest.raises(ValueError, match="NaN"):
        ops.mask_confusion(None, cpu_f32, cpu_f32, [float("nan")])
    with pytest.raises(ValueError, match="cuda"):
        ops.mask_confusion(None, cpu_f32, cpu_f32, [0.5])
    with pytest.raises(ValueError, match="cuda uint8"):
        ops.mask_pack(None, torch.zeros((1, 2, 2)))
    with pytest.raises(ValueError, match="order"):
        ops.mask_rle(None, torch.zeros((1, 2, 2), dtype=torch.uint8), order="diagonal")
    with pytest.raises(ValueError, match="rule"):
        ops.det_match_iou(None, None, None, None, None, None, 1, [0.5], rule="voc")
    with pytest.raises(ValueError, match="increase"):
        ops.det_match_iou(None, None, None, None, None, None, 1, [0.5, 0.5])
    with pytest.raises(ValueError, match="rule"):
        mask_eval.evaluate_masks(None, None, None, None, None, None, rule="voc")
    # decoding: the counts are checked on the host before anything reaches the device
    with pytest.raises(ValueError, match="add up to 5"):
        ops.mask_from_rle(None, [0, 2], [2, 3], (2, 3))
    with pytest.raises(ValueError, match="add up to 7"):
        ops.mask_from_rle(None, [0, 2, 4], [2, 4, 3, 4], (2, 3), order="column")
    with pytest.raises(ValueError, match="run_offsets"):
        ops.mask_from_rle(None, [0, 3], [2, 4], (2, 3))
    with pytest.raises(ValueError, match=r"\[0, 2\^31\)"):
        ops.mask_from_rle(None, [0, 2], [-1, 7], (2, 3))
    with pytest.raises(ValueError, match="uncompressed"):
        mask_eval.from_coco_rle({"size": [2, 3], "counts": "abc"})
    from pyrapose_amd.utils import eval_pose
    with pytest.raises(ValueError, match="mask_metrics"):
        eval_pose.evaluate_pose_metrics(None, None, None, None, [1.0], None, None, mask_metrics={"thresholds": (0.5,)})
