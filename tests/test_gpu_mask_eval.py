"""GPU: the segmentation-metric entry points (pp_mask_confusion, pp_mask_pack, pp_mask_iou_pairs, pp_det_match_iou, pp_mask_rle,
pp_mask_from_rle; csrc/mask_eval.hip, csrc/det_eval.hip) against the numpy restatement tests/mask_eval_np.py.  Every output is
compared byte for byte: the kernels do integer work and single float64 quotients.  Shapes are the smallest at which each
mechanism can go wrong: the wave width 64, the workgroup of 256, the 16384-element chunk of the confusion pass, the 4 x 4 pair
tile, one word more or less than a mask fills."""
import os

import numpy as np
import pytest

import det_eval_np as DN
import mask_eval_np as MN
from test_mask_eval_cpu import golden, mask_chain_np, rect_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


def same_bytes(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    want = np.asarray(want)
    if want.dtype == np.uint64:
        got = got.view(np.uint64)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == np.ascontiguousarray(want).tobytes(), what


# ---- pp_mask_confusion ------------------------------------------------------------------------------------------------------
def confusion_case(seed, B, M, C, thresholds, empty_target=False):
    rng = np.random.default_rng(seed)
    pred = rng.uniform(0, 1, size=(B, M, C)).astype(np.float32)
    flat = pred.reshape(-1)
    pick = rng.permutation(flat.size)
    special = [np.float32(t) for t in thresholds] + [np.float32(np.nan), np.float32(0.0), np.float32(-0.0), np.float32(1.0)]
    for i, v in enumerate(special * 2):  # values exactly at a threshold (where float32 holds it), NaN, +-0
        if i < pick.size:
            flat[pick[i]] = v
    target = np.zeros((B, M, C + 1), np.float32)
    if not empty_target:
        target[..., :C] = (rng.uniform(size=(B, M, C)) < 0.3) * rng.choice([1.0, 0.5, -2.0], size=(B, M, C))
        target[..., C] = target[..., :C].any(-1)
    else:
        target[..., C] = 1.0  # the any-object flag alone must not count
    return pred, target


@pytest.mark.parametrize("B, M, C, T", [(1, 300, 1, 1), (3, 37, 33, 16), (1, 5, 3, 2), (3, 1500, 13, 3)])
def test_confusion_counts(B, M, C, T):
    # M = 300: not a multiple of 256; 37 and 5: less than a wave; 3 x 1500 x 13 = 58500 elements: four chunks, the last partial
    from pyrapose_amd import ops
    thr = [0.5] if T == 1 else sorted(set(np.round(np.linspace(0.0, 0.9375, T), 4).tolist()))
    assert len(thr) == T
    pred, target = confusion_case(B * 1000 + C, B, M, C, thr)
    want = MN.mask_confusion(pred, target, thr)
    assert want.sum() > 0 and (T == 1 or (want[0] != want[-1]).any())
    got = ops.mask_confusion(ctx(), dev(pred, np.float32), dev(target, np.float32), thr)
    same_bytes(got, want, "counts")
    same_bytes(ops.mask_confusion(ctx(), dev(pred, np.float32), dev(target, np.float32), thr), want, "counts, second call")


def test_confusion_empty_target_and_scores():
    from pyrapose_amd.utils import mask_eval
    pred, target = confusion_case(7, 2, 70, 4, [0.5], empty_target=True)
    want = MN.mask_confusion(pred, target, [0.25, 0.5])
    assert want[..., 0].sum() == 0 and want[..., 2].sum() == 0 and want[..., 1].sum() > 0
    got = mask_eval.semantic_scores(pred, target, thresholds=(0.25, 0.5))
    same_bytes(got["counts"], want, "counts")
    iou, prec, rec, miou = MN.scores(want)
    for k, w in (("iou", iou), ("precision", prec), ("recall", rec), ("miou", miou)):
        same_bytes(got[k], w, k)
    pred, target = confusion_case(8, 1, 70, 4, [0.5])
    got = mask_eval.semantic_scores(dev(pred, np.float32), dev(target, np.float32))
    iou, prec, rec, miou = MN.scores(MN.mask_confusion(pred, target, [0.5]))
    assert miou[0] > 0
    for k, w in (("iou", iou), ("precision", prec), ("recall", rec), ("miou", miou)):
        same_bytes(got[k], w, k)


# ---- pp_mask_pack -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W", [(1, 1), (7, 9), (8, 8), (5, 13), (37, 29), (40, 52)])
def test_pack(H, W):
    # H W = 1, 63, 64, 65, 37 x 29 = 1073 (17 words, 49 bits in the last), 2080 (more words than the workgroup's 4 waves x 8)
    from pyrapose_amd import ops
    rng = np.random.default_rng(H * 100 + W)
    masks = (rng.uniform(size=(6, H, W)) < 0.5).astype(np.uint8) * rng.integers(1, 256, size=(6, H, W)).astype(np.uint8)
    masks[0] = 0                    # empty
    masks[1] = 255                  # full: the tail bits of the last word must still be zero
    masks[2] = 0
    masks[2].reshape(-1)[-1] = 7    # only the last pixel
    masks[3] = 0
    masks[3].reshape(-1)[0] = 1     # only the first
    want = MN.mask_pack(masks)
    tail = (H * W) % 64
    if tail:
        assert int(want[0][1, -1]) == (1 << tail) - 1
    got = ops.mask_pack(ctx(), dev(masks, np.uint8))
    for g, w, k in zip(got, want, ("words", "area", "word_range")):
        same_bytes(g, w, k)
    assert got[2][0].tolist() == [0, 0] and got[1][1].item() == H * W


# ---- pp_mask_iou_pairs ------------------------------------------------------------------------------------------------------
def iou_case(seed, B, D, n_gt, H=11, W=23, pad_image=None):
    """253 pixels = 4 words; special pairs in image 0 when it has room: identical masks, two empty masks, disjoint word ranges"""
    rng = np.random.default_rng(seed)
    G = int(np.sum(n_gt))
    det = (rng.uniform(size=(B, D, H, W)) < 0.4).astype(np.uint8)
    gt = (rng.uniform(size=(G, H, W)) < 0.4).astype(np.uint8) * 200
    labels = rng.integers(0, 3, size=(B, D)).astype(np.int32)
    labels[rng.uniform(size=(B, D)) < 0.2] = -1
    if pad_image is not None:
        labels[pad_image] = -1
    offs = np.zeros(B + 1, np.int32)
    offs[1:] = np.cumsum(n_gt)
    if n_gt[0] >= 3 and D >= 3:
        labels[0, :3] = 0
        det[0, 0] = gt[0] != 0                       # identical: exactly 1.0
        det[0, 1] = 0
        gt[1] = 0                                    # two empty masks: 0.0
        det[0, 2] = 0
        det[0, 2].reshape(-1)[:40] = 1               # word 0 only
        gt[2] = 0
        gt[2].reshape(-1)[200:] = 1                  # word 3 only: the ranges do not overlap
    return det, gt, labels, offs


@pytest.mark.parametrize("D, n_gt, pad_image", [(3, [3, 0, 5], None), (4, [4, 4], 1), (5, [5, 3, 9, 0], 2), (9, [1], None)])
def test_iou_pairs(D, n_gt, pad_image):
    # D and ng below, at and above the 4 x 4 tile; an image without ground truth; an image whose slots are all padding
    from pyrapose_amd import ops
    B = len(n_gt)
    det, gt, labels, offs = iou_case(D * 10 + B, B, D, n_gt, pad_image=pad_image)
    H, W = det.shape[2:]
    pd, pg = MN.mask_pack(det.reshape(B * D, H, W)), MN.mask_pack(gt)
    want_iou, want_inter, want_po = MN.mask_iou_pairs(pd, pg, offs, D, labels)
    if n_gt[0] >= 3 and D >= 3:
        ng = n_gt[0]
        assert want_iou[0 * ng + 0] == 1.0 and want_iou[1 * ng + 1] == 0.0 and want_iou[2 * ng + 2] == 0.0
        assert pd[2][2, 1] <= pg[2][2, 0]
    assert (want_iou > 0).any()
    gd, gg = ops.mask_pack(ctx(), dev(det.reshape(B * D, H, W), np.uint8)), ops.mask_pack(ctx(), dev(gt, np.uint8))
    import torch
    iou = ops.mask_iou_pairs(ctx(), gd, gg, dev(offs, np.int32), (H, W), D, det_labels=dev(labels, np.int32), want_inter=True)
    same_bytes(iou[0], want_iou, "iou")
    same_bytes(iou[2], want_inter, "inter")
    assert np.array_equal(iou[1], want_po)
    # without labels every slot is read
    want_all = MN.mask_iou_pairs(pd, pg, offs, D)[0]
    got_all, _po = ops.mask_iou_pairs(ctx(), gd, gg, dev(offs, np.int32), (H, W), D)
    same_bytes(got_all, want_all, "iou without labels")
    assert torch.is_tensor(got_all)


def test_mask_iou_host_path_equals_the_pixel_loop():
    from pyrapose_amd.utils import mask_eval
    det, gt, _labels, offs = iou_case(3, 2, 3, [2, 3], H=6, W=13)
    got = mask_eval.mask_iou(det, gt, offs)
    assert [g.shape for g in got] == [(3, 2), (3, 3)]
    for b in range(2):
        for d in range(3):
            for g in range(offs[b + 1] - offs[b]):
                assert got[b][d, g] == MN.brute_iou(det[b, d], gt[offs[b] + g])


# ---- pp_det_match_iou -------------------------------------------------------------------------------------------------------
def match_case(seed, B, D, n_gt, n_class=3, ignore=False):
    """an IoU matrix from a few values (equal IoUs are common, some exactly at a threshold) and scores from a small set"""
    rng = np.random.default_rng(seed)
    G = int(np.sum(n_gt))
    offs = np.zeros(B + 1, np.int32)
    offs[1:] = np.cumsum(n_gt)
    iou = rng.choice([0.0, 0.25, 0.5, 0.5, 0.625, 0.75, 1.0], size=D * G)
    scores = rng.integers(1, 5, size=(B, D)) / 4.0
    labels = rng.integers(0, n_class, size=(B, D)).astype(np.int32)
    labels[rng.uniform(size=(B, D)) < 0.15] = -1
    gt_labels = rng.integers(0, n_class, size=G).astype(np.int32)
    gt_ignore = (rng.uniform(size=G) < 0.3).astype(np.uint8) if ignore else None
    return iou, scores, labels, gt_labels, offs, gt_ignore


@pytest.mark.parametrize("rule, ignore, T", [("reference", False, 1), ("coco", True, 1), ("coco", True, 16), ("reference", False, 16)])
def test_match_on_an_iou_matrix(rule, ignore, T):
    from pyrapose_amd import ops
    thr = [0.5] if T == 1 else list(np.linspace(0.05, 0.8, 16))
    iou, scores, labels, gt_labels, offs, gt_ignore = match_case(T + len(rule), 4, 70, [0, 5, 66, 1], ignore=ignore)
    want = MN.det_match_iou(iou, scores, labels, gt_labels, offs, 3, thr, rule, gt_ignore)
    assert (want[0] >= 0).any() and (not ignore or want[1].any())
    got = ops.det_match_iou(ctx(), dev(iou, np.float64), dev(scores, np.float64), dev(labels, np.int32), dev(gt_labels, np.int32),
                            dev(offs, np.int32), 3, thr, rule=rule, gt_ignore=None if gt_ignore is None else dev(gt_ignore, np.uint8))
    for g, w, k in zip(got, want, ("match", "det_ignored", "npos")):
        same_bytes(g, w, (k, rule))


def test_rectangle_masks_match_as_their_boxes_and_the_whole_chain():
    import torch
    from pyrapose_amd import ops
    from pyrapose_amd.utils import mask_eval
    case = rect_case()
    B, D = case["det_scores"].shape
    H, W = case["H"], case["W"]
    thr = list(np.linspace(0.5, 0.95, 10))
    want = mask_chain_np(case, thr, "coco", "101")
    c = ctx()
    gd = ops.mask_pack(c, dev(case["det_masks"].reshape(B * D, H, W), np.uint8))
    gg = ops.mask_pack(c, dev(case["gt_masks"], np.uint8))
    labels, scores = dev(case["det_labels"], np.int32), dev(case["det_scores"], np.float64)
    gt_labels, offs, ign = dev(case["gt_labels"], np.int32), dev(case["gt_offsets"], np.int32), dev(case["gt_ignore"], np.uint8)
    iou, _po = ops.mask_iou_pairs(c, gd, gg, offs, (H, W), D, det_labels=labels)
    same_bytes(iou, want["iou"], "iou")
    from_masks = ops.det_match_iou(c, iou, scores, labels, gt_labels, offs, case["n_class"], thr, rule="coco", gt_ignore=ign)
    from_boxes = ops.det_match(c, dev(case["det_boxes"], np.float64), scores, labels, dev(case["gt_boxes"], np.float64), gt_labels, offs,
                               case["n_class"], thr, rule="coco", gt_ignore=ign)
    for a, b, k in zip(from_masks, from_boxes, ("match", "det_ignored", "npos")):
        assert torch.equal(a, b), k
        same_bytes(a, want[k], k)
    # the host path, from arrays and from device tensors, against the restatement and against the box chain's restatement
    boxes = DN.evaluate(case["det_boxes"], case["det_scores"], case["det_labels"], case["gt_boxes"], case["gt_labels"], case["gt_offsets"],
                        case["n_class"], thr, "coco", "101", case["gt_ignore"])
    for masks_in in ((case["det_masks"], case["gt_masks"]), (dev(case["det_masks"], np.uint8), dev(case["gt_masks"], np.uint8))):
        res = mask_eval.evaluate_masks(masks_in[0], case["det_scores"], case["det_labels"], masks_in[1], case["gt_labels"],
                                       case["gt_offsets"], ignore=case["gt_ignore"], num_classes=case["n_class"])
        for k in ("ap", "recall_final", "npos"):
            same_bytes(res[k], want[k], k)
            same_bytes(res[k], boxes[k], k + " (boxes)")
        have = want["npos"] > 0
        assert res["AP"] == float(want["ap"][:, have].mean()) and res["AP50"] == float(want["ap"][0, have].mean())
    ref = mask_eval.evaluate_masks(case["det_masks"], case["det_scores"], case["det_labels"], case["gt_masks"], case["gt_labels"],
                                   case["gt_offsets"], rule="reference", num_classes=case["n_class"])
    same_bytes(ref["ap"], mask_chain_np(case, [0.5], "reference", "area")["ap"], "ap (reference rule)")


# ---- pp_mask_rle / pp_mask_from_rle -----------------------------------------------------------------------------------------
def rle_masks():
    """13 x 17 fixture masks (first / last pixel set, all 0, all 1, single pixels, both checkerboards) and 21 x 31 = 651 pixels
    (both sides odd, so a checkerboard alternates in either order): more than two steps of the workgroup, with boundaries at
    the wave and step edges"""
    small = golden()["masks"]
    H, W = 21, 31
    rng = np.random.default_rng(11)
    board = (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(np.uint8)
    edges = np.zeros(H * W, np.uint8)
    edges[[63, 64, 255, 256, 257, 511, 512, 599]] = 1
    big = np.stack([board, 1 - board, edges.reshape(H, W), (rng.uniform(size=(H, W)) < 0.5).astype(np.uint8), np.zeros((H, W), np.uint8),
                    np.ones((H, W), np.uint8)])
    return small, big


@pytest.mark.parametrize("order", ["row", "column"])
def test_rle_and_back(order):
    from pyrapose_amd import ops
    for masks in rle_masks():
        want_offs, want_counts = MN.mask_rle(masks, order)
        assert int(np.diff(want_offs).max()) == masks.shape[1] * masks.shape[2] + 1  # the checkerboard that starts with 1
        offs, counts = ops.mask_rle(ctx(), dev(masks * 9, np.uint8), order=order)
        assert np.array_equal(offs, want_offs)
        same_bytes(counts, want_counts, "counts")
        back = ops.mask_from_rle(ctx(), offs, counts, masks.shape[1:], order=order)
        same_bytes(back, masks * 255, "decoded")
        back = ops.mask_from_rle(ctx(), want_offs, want_counts, masks.shape[1:], order=order)  # from host arrays
        same_bytes(back, masks * 255, "decoded from host arrays")


def test_rle_capacity_is_never_exceeded_silently():
    import ctypes
    import torch
    from pyrapose_amd import _lib, ops
    masks = rle_masks()[0]
    want_offs, want_counts = MN.mask_rle(masks, "row")
    total = int(want_offs[-1])
    with pytest.raises(ValueError, match="capacity"):
        ops.mask_rle(ctx(), dev(masks, np.uint8), capacity=total - 1)
    offs, counts = ops.mask_rle(ctx(), dev(masks, np.uint8), capacity=total)
    same_bytes(counts, want_counts, "counts at the exact capacity")
    # at the C ABI: the error code, the offsets reported on both sides, and nothing written to counts
    m = dev(masks, np.uint8)
    N, H, W = masks.shape
    nbytes = _lib.lib.pp_mask_rle_workspace_bytes(N)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    out = torch.full((total,), -7, dtype=torch.int32, device="cuda")
    offs_d = torch.zeros((N + 1,), dtype=torch.int32, device="cuda")
    host = np.zeros(N + 1, np.int32)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _lib.lib.pp_mask_rle(ctx().handle, N, H, W, 0, ptr(m), ptr(ws), nbytes, 10, ptr(offs_d), host.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                              ptr(out))
    assert rc == -1 and np.array_equal(host, want_offs) and np.array_equal(offs_d.cpu().numpy(), want_offs)
    assert (out == -7).all()
    # several masks of the most runs, the capacity left to the wrapper
    big = np.tile(rle_masks()[1][1:2], (3, 1, 1))
    offs, counts = ops.mask_rle(ctx(), dev(big, np.uint8))
    same_bytes(counts, MN.mask_rle(big, "row")[1], "counts")


def test_rle_strings_and_coco_dicts():
    from pyrapose_amd.utils import mask_eval
    g = golden()
    for m, s in zip(g["masks"], g["strings"]):
        assert mask_eval.rle_encode(m) == str(s)
    m = rle_masks()[1][3]
    rle = mask_eval.to_coco_rle(m)
    assert rle["size"] == [21, 31] and rle["counts"] == MN.rle_counts(m, "column") and all(isinstance(c, int) for c in rle["counts"])
    assert np.array_equal(mask_eval.from_coco_rle(rle), m * 255)
    assert np.array_equal(mask_eval.decode_rle(MN.rle_counts(m, "row"), (21, 31), order="row"), m * 255)
    with pytest.raises(ValueError, match="add up"):
        mask_eval.from_coco_rle({"size": [21, 31], "counts": rle["counts"][:-1]})


# ---- the evaluation loop's opt-in mask metrics ------------------------------------------------------------------------------
def test_mask_metrics_of_the_evaluation_loop():
    from pyrapose_amd.utils import eval_pose
    Cn, N, M = 3, 200, 192
    rng = np.random.default_rng(9)
    outputs = [rng.uniform(0, 1, (1, M, Cn)).astype(np.float32) for _ in range(3)]
    targets = [np.concatenate([(rng.uniform(size=(M, Cn)) < 0.3), np.ones((M, 1))], 1).astype(np.float32) for _ in range(3)]
    targets[1][:, :Cn] = 0  # an all-empty target

    class Gen(object):
        def size(self): return 4
        def load_image(self, i): return np.full((16, 16, 3), i, np.uint8)
        def preprocess_image(self, x): return x.astype(np.float32)
        def resize_image(self, x): return x, 1.0
        def load_annotations(self, i):  # image 3 has no annotation: it is not scored, nor is its mask
            return {"labels": np.zeros((0,)), "poses": np.zeros((0, 7))} if i == 3 else \
                {"labels": np.array([float(i % Cn)]), "poses": np.array([[0.0, 0.0, 800.0, 1.0, 0.0, 0.0, 0.0]])}

    def predict(x):  # no class gathers votes: the loop scores no pose, only the masks
        i = int(x[0, 0, 0, 0])
        return [np.zeros((1, N, 16), np.float32), np.full((1, N, Cn), 0.01, np.float32), outputs[i]]

    boxes, models, dia = np.zeros((Cn, 8, 3)), [None] * Cn, [0.1] * Cn
    K = np.array([[100.0, 0, 8], [0, 100.0, 8], [0, 0, 1]])
    kw = dict(generator=Gen(), predict_on_batch=predict, threeD_boxes=boxes, models=models, model_diameters=dia, load_depth=None, K=K)
    off = eval_pose.evaluate_pose_metrics(**kw)
    on = eval_pose.evaluate_pose_metrics(mask_metrics=dict(target=lambda i: targets[i], thresholds=(0.3, 0.5)), **kw)
    assert not any(k.startswith("mask_") for k in off) and set(on) - set(off) == {"mask_counts", "mask_iou", "mask_miou"}
    for k in off:
        assert np.array_equal(np.asarray(off[k]), np.asarray(on[k])), k
    want = sum(MN.mask_confusion(outputs[i], targets[i][None], [0.3, 0.5]) for i in range(3))
    same_bytes(on["mask_counts"], want, "mask_counts")
    iou, _p, _r, miou = MN.scores(want)
    same_bytes(on["mask_iou"], iou, "mask_iou")
    same_bytes(on["mask_miou"], miou, "mask_miou")
