"""Segmentation metrics, everything on the device (ops.mask_* / det_match_iou, csrc/mask_eval.hip):

* `semantic_scores`: IoU, precision and recall per class of the mask head's output against its training target.  The reference
  only thresholds that output at 0.5 and writes a picture (linemod_eval.py:336-369); scoring against the trained target means
  no resize rule is restated here.
* `mask_iou`, `evaluate_masks`: instance masks (utils.scene_gt's mask_visib of ground-truth or estimated poses,
  `masks_from_poses`) scored with COCO's mask AP as BOP's segmentation task does it: pack -> pairwise IoU -> matching on that
  IoU -> the detection chain's curves and integrals unchanged.
* `rle_encode` (the reference's annotation_scripts/misc.py:42-51, its exact string; pinned through tests/golden/mask_rle.npz),
  `to_coco_rle` / `from_coco_rle` (COCO's uncompressed dicts) and `decode_rle`.

Restated and unpinned: parity with pycocotools' maskUtils / evaluateImg and bop_toolkit, neither was at hand.  Out of scope:
pycocotools' compressed RLE string, crowd regions, area ranges."""
import numpy as np
import torch

from .. import ops
from .eval import COCO_IOU_THRESHOLDS, _dev


def _ctx(ctx):
    if ctx is None:
        from ..runtime import default_context
        ctx = default_context()
    return ctx, "cuda:%d" % ctx.device


def _ratio(num, den):
    """num / den as one rounded float64 quotient of the exact integers; 0.0 where den is 0"""
    num, den = num.astype(np.float64), den.astype(np.float64)
    return np.divide(num, den, out=np.zeros_like(num), where=den != 0)


def scores_from_counts(counts):
    """counts int64 [T,C,3] (tp, fp, fn) -> dict(iou [T,C] = tp / (tp + fp + fn), precision = tp / (tp + fp), recall = tp /
    (tp + fn), each 0.0 where its denominator is 0; miou [T]: the mean of iou over the classes with tp + fn > 0 at that
    threshold -- the classes present in the target --, 0.0 when there is none)."""
    counts = np.asarray(counts, np.int64)
    tp, fp, fn = counts[..., 0], counts[..., 1], counts[..., 2]
    iou = _ratio(tp, tp + fp + fn)
    have = (tp + fn) > 0
    miou = np.array([iou[t, have[t]].mean() if have[t].any() else 0.0 for t in range(iou.shape[0])], np.float64)
    return dict(iou=iou, precision=_ratio(tp, tp + fp), recall=_ratio(tp, tp + fn), miou=miou)


def semantic_scores(pred, target, thresholds=(0.5,), ctx=None):
    """The mask head scored against its training target: pred [B,M,C] (the mask output's sigmoid values) and target [B,M,C+1]
    (as ops.anchor_targets writes it), arrays or tensors -> dict(counts int64 [T,C,3] (tp, fp, fn), iou [T,C], precision,
    recall, miou [T], thresholds).  One pass on the device (ops.mask_confusion), the quotients on the host."""
    ctx, dev = _ctx(ctx)
    counts = ops.mask_confusion(ctx, _dev(pred, torch.float32, dev), _dev(target, torch.float32, dev), thresholds).cpu().numpy()
    return dict(scores_from_counts(counts), counts=counts, thresholds=np.asarray(thresholds, np.float64).reshape(-1))


def _mask_inputs(det_masks, gt_masks, gt_offsets, dev):
    det_masks = _dev(det_masks, torch.uint8, dev)  # (a device tensor of the right type stays where it is)
    gt_masks = _dev(gt_masks, torch.uint8, dev)
    if det_masks.dim() != 4 or gt_masks.dim() != 3 or tuple(gt_masks.shape[1:]) != tuple(det_masks.shape[2:]):
        raise ValueError("mask_eval: det_masks must be [B,D,H,W] and gt_masks [G,H,W] of the same H, W, got %s and %s" %
                         (list(det_masks.shape), list(gt_masks.shape)))
    return det_masks, gt_masks, _dev(gt_offsets, torch.int32, dev).reshape(-1)


def _pair_iou(ctx, det_masks, gt_masks, gt_offsets, det_labels=None, want_inter=False):
    B, D, H, W = (int(s) for s in det_masks.shape)
    return ops.mask_iou_pairs(ctx, ops.mask_pack(ctx, det_masks.reshape(B * D, H, W)), ops.mask_pack(ctx, gt_masks), gt_offsets, (H, W), D,
                              det_labels=det_labels, want_inter=want_inter)


def mask_iou(det_masks, gt_masks, gt_offsets, ctx=None):
    """IoU of every detection mask with every ground-truth mask of its image: det_masks [B,D,H,W] uint8 (non-zero = set), gt_masks
    [G,H,W], gt_offsets [B+1]; arrays or device tensors -> a list of B float64 arrays [D,ng_b].  0.0 where both masks are empty."""
    ctx, dev = _ctx(ctx)
    det_masks, gt_masks, gt_offsets = _mask_inputs(det_masks, gt_masks, gt_offsets, dev)
    D = int(det_masks.shape[1])
    iou, pair_offsets = _pair_iou(ctx, det_masks, gt_masks, gt_offsets)
    iou = iou.cpu().numpy()
    return [iou[pair_offsets[b]:pair_offsets[b + 1]].reshape(D, -1) for b in range(len(pair_offsets) - 1)]


def evaluate_masks(det_masks, det_scores, det_labels, gt_masks, gt_labels, gt_offsets, rule="coco", iou_thresholds=None, ignore=None,
                   num_classes=None, integration=None, ctx=None):
    """Average precision of instance masks, utils.eval.evaluate_detections with the IoU of masks in place of boxes.  det_masks
    [B,D,H,W] uint8 (non-zero = set), det_scores [B,D], det_labels [B,D] (-1 = padding: that slot's mask is not read); gt_masks
    [G,H,W], gt_labels [G], gt_offsets [B+1]; arrays or device tensors -- masks already on the device are not copied to the host.
    rule, iou_thresholds, ignore (e.g. utils.eval.bop_ignore(visib_fract)), num_classes, integration: as evaluate_detections
    -> its dict: ap [T,C], recall_final [T,C], npos [C], iou_thresholds, AP, AP50, AP75."""
    if rule not in ops.DET_RULES:
        raise ValueError("evaluate_masks: unknown rule %r (reference | coco)" % (rule,))
    if iou_thresholds is None:
        iou_thresholds = COCO_IOU_THRESHOLDS if rule == "coco" else (0.5,)
    thr = np.asarray(iou_thresholds, np.float64).reshape(-1)
    integration = integration or ("101" if rule == "coco" else "area")
    ctx, dev = _ctx(ctx)
    det_masks, gt_masks, gt_offsets = _mask_inputs(det_masks, gt_masks, gt_offsets, dev)
    B, D = int(det_masks.shape[0]), int(det_masks.shape[1])
    scores, labels = _dev(det_scores, torch.float64, dev).reshape(B, D), _dev(det_labels, torch.int32, dev).reshape(B, D)
    gt_labels = _dev(gt_labels, torch.int32, dev).reshape(-1)
    ignore = None if ignore is None else _dev(ignore, torch.uint8, dev).reshape(-1)
    if num_classes is None:
        num_classes = 1 + max(int(labels.max()) if labels.numel() else 0, int(gt_labels.max()) if gt_labels.numel() else 0)
    iou, _pair_offsets = _pair_iou(ctx, det_masks, gt_masks, gt_offsets, det_labels=labels)
    match, det_ignored, npos = ops.det_match_iou(ctx, iou, scores, labels, gt_labels, gt_offsets, num_classes, thr, rule=rule,
                                                 gt_ignore=ignore)
    order, class_offsets = ops.det_order(scores, labels, num_classes)
    _tp, _fp, recall, prec_env = ops.det_pr_curve(ctx, order, class_offsets, match, det_ignored, npos, check=False)
    ap, recall_final = ops.det_ap(ctx, class_offsets, npos, recall, prec_env, integration=integration, check=False)
    ap, recall_final, npos = ap.cpu().numpy(), recall_final.cpu().numpy(), npos.cpu().numpy()
    have = npos > 0

    def mean_at(value):
        t = np.nonzero(np.isclose(thr, value, rtol=0, atol=1e-9))[0]
        return float(ap[t[0], have].mean()) if t.size and have.any() else None

    return dict(ap=ap, recall_final=recall_final, npos=npos, iou_thresholds=thr, AP=float(ap[:, have].mean()) if have.any() else None,
                AP50=mean_at(0.5), AP75=mean_at(0.75))


def masks_from_poses(scenes, models, K, label_of, depth=None, im_size=None, max_instances=None, **scene_kw):
    """Estimated (or ground-truth) poses to visible masks in evaluate_masks' layout, through utils.scene_gt.scene_gt_info.
    scenes: per image a list of instances (dicts with 'obj_id', 'R', 't', optionally 'score'); models: obj_id -> model dict;
    label_of: obj_id -> class label (a dict or a callable); depth / im_size / **scene_kw: as scene_gt_info.
    -> dict(masks uint8 [B,D,h,w] on the device (D = max_instances, default the largest scene, at least 1; unused slots zero),
    scores float64 [B,D] (the instances' 'score', 1.0 where absent), labels int32 [B,D] (-1 = padding), offsets int32 [B+1],
    visib_fract [n]): masks.reshape(-1, h, w)[labels.reshape(-1) >= 0] with offsets is the packed layout of ground truth."""
    from .scene_gt import scene_gt_info
    scenes = [list(s) for s in scenes]
    gt = scene_gt_info(scenes, models, K, depth=depth, im_size=im_size, masks=True, **scene_kw)
    B = len(scenes)
    counts = [len(s) for s in scenes]
    D = int(max_instances) if max_instances is not None else max(counts + [1])
    if max(counts + [0]) > D:
        raise ValueError("masks_from_poses: a scene has %d instances, max_instances is %d" % (max(counts), D))
    h, w = (int(v) for v in gt.id_images.shape[-2:])
    masks = torch.zeros((B, D, h, w), dtype=torch.uint8, device="cuda")
    scores, labels = np.zeros((B, D), np.float64), np.full((B, D), -1, np.int32)
    lookup = label_of if callable(label_of) else label_of.__getitem__
    for b, instances in enumerate(scenes):
        if instances:
            masks[b, :len(instances)] = torch.as_tensor(gt.mask_visib[b]).to("cuda")
        for d, inst in enumerate(instances):
            scores[b, d], labels[b, d] = float(inst.get("score", 1.0)), int(lookup(inst["obj_id"]))
    offsets = np.zeros(B + 1, np.int32)
    offsets[1:] = np.cumsum(counts)
    visib = np.array([row["visib_fract"] for rows in gt.info for row in rows], np.float64)
    return dict(masks=masks, scores=scores, labels=labels, offsets=offsets, visib_fract=visib)


def _runs(img, order, ctx=None):
    """one image [H,W] (array or tensor, non-zero = set) -> (its COCO counts as a numpy int64 array, (H, W))"""
    ctx, dev = _ctx(ctx)
    m = torch.as_tensor(img)
    if m.dim() != 2:
        raise ValueError("mask_eval: a mask is a 2-D image, got shape %s" % (list(m.shape),))
    m = (m != 0).to(device=dev, dtype=torch.uint8).contiguous()
    _offs, counts = ops.mask_rle(ctx, m[None], order=order)
    return counts.cpu().numpy().astype(np.int64), (int(m.shape[0]), int(m.shape[1]))


def rle_encode(img, ctx=None):
    """The reference's rle_encode (annotation_scripts/misc.py:42-51) with its signature and its exact string: img 1 - mask,
    0 - background (flattened row-major) -> 'start length start length ...' with 1-based starts of the runs of set pixels.
    The runs come from the device (ops.mask_rle, row order); the string is derived from COCO's counts on the host."""
    counts, _shape = _runs(img, "row", ctx)
    ends = np.cumsum(counts)
    starts = ends[0:-1:2] + 1          # a set run begins after every even-numbered (zero) run that is followed by one
    lengths = counts[1::2]
    out = np.empty(2 * lengths.size, np.int64)
    out[0::2], out[1::2] = starts[:lengths.size], lengths
    return " ".join(str(x) for x in out)


def to_coco_rle(img, ctx=None):
    """COCO's uncompressed RLE of one mask [H,W]: {'size': [H, W], 'counts': [...]}, column-major, starting with the zero run."""
    counts, (H, W) = _runs(img, "column", ctx)
    return {"size": [H, W], "counts": [int(c) for c in counts]}


def decode_rle(counts, shape, order="column", ctx=None):
    """Run lengths (COCO's counts: alternating, the zero run first) of one mask back to a uint8 image [H,W] of 0 / 255 on the
    host; order 'column' (COCO) or 'row'.  Counts that do not add up to H * W raise ValueError."""
    ctx, _dev_name = _ctx(ctx)
    counts = np.asarray(counts, np.int64).reshape(-1)
    return ops.mask_from_rle(ctx, np.array([0, counts.size], np.int64), counts, shape, order=order)[0].cpu().numpy()


def from_coco_rle(rle, ctx=None):
    """{'size': [H, W], 'counts': [...]} (uncompressed) -> uint8 [H,W] of 0 / 255"""
    if not isinstance(rle.get("counts"), (list, tuple, np.ndarray)):
        raise ValueError("from_coco_rle: only the uncompressed form (counts as a list) is supported")
    return decode_rle(rle["counts"], rle["size"], "column", ctx)
