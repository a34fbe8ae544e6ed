"""2-D detection average precision with the reference's names (utils/eval.py): `_compute_ap`, `evaluate` -- the per-class
VOC-style AP behind the 'mAP' of callbacks.Evaluate -- and, beyond the reference, `evaluate_detections` (the array-level entry,
also COCO AP at IoU 0.50:0.05:0.95 with ignored ground truth, which is BOP's detection score) and `bop_ignore`.

All matching and curve arithmetic runs on the device (ops.det_match / det_order / det_pr_curve / det_ap, csrc/det_eval.hip).
What is pinned: rule 'reference' with integration 'area' reproduces the reference's `evaluate` (tests/golden/detection_ap.npz).
What is restated and unpinned: rule 'coco' and integration '101' follow pycocotools' evaluateImg / accumulate without crowd
and area ranges; pycocotools was not at hand to compare with."""
import numpy as np
import torch

from .. import ops

COCO_IOU_THRESHOLDS = tuple(np.linspace(0.5, 0.95, 10))  # cocoeval.py Params.iouThrs


def _compute_ap(recall, precision):
    """utils/eval.py:29-55 on the host, for callers that hold curves: the area under the precision envelope."""
    mrec = np.concatenate(([0.], np.asarray(recall, np.float64).reshape(-1), [1.]))
    mpre = np.concatenate(([0.], np.asarray(precision, np.float64).reshape(-1), [0.]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def bop_ignore(visib_fract, min_visib=0.1):
    """The ignore flags of BOP's detection task from utils.scene_gt's `visib_fract`: instances less visible than min_visib."""
    return (torch.as_tensor(visib_fract) < min_visib).to(torch.uint8)


def _dev(a, dtype, device):
    return torch.as_tensor(a).to(device=device, dtype=dtype).contiguous()


def evaluate_detections(detections, annotations, rule="coco", iou_thresholds=None, ignore=None, num_classes=None, integration=None,
                        ctx=None):
    """Average precision of a set of detections against ground truth, everything on the device.
    detections = (boxes [B,D,4], scores [B,D], labels [B,D], -1 = padding) as layers.FilterDetections returns them; annotations =
    (gt_boxes [G,4], gt_labels [G], gt_offsets [B+1]); arrays or tensors.  rule 'coco' (default thresholds 0.50:0.05:0.95,
    integration '101', `ignore` [G] flags, e.g. bop_ignore(...)) or 'reference' (default threshold 0.5, integration 'area', no
    ignore).  -> dict: ap [T,C], recall_final [T,C], npos [C] (numpy), iou_thresholds, AP (mean of ap over the classes with
    ground truth and all thresholds), AP50, AP75 (that mean at the one threshold; None when it is not among them)."""
    if rule not in ops.DET_RULES:
        raise ValueError("evaluate_detections: unknown rule %r (reference | coco)" % (rule,))
    if iou_thresholds is None:
        iou_thresholds = COCO_IOU_THRESHOLDS if rule == "coco" else (0.5,)
    thr = np.asarray(iou_thresholds, np.float64).reshape(-1)
    integration = integration or ("101" if rule == "coco" else "area")
    if ctx is None:
        from ..runtime import default_context
        ctx = default_context()
    dev = "cuda:%d" % ctx.device
    boxes, scores, labels = detections
    gt_boxes, gt_labels, gt_offsets = annotations
    boxes, scores, labels = _dev(boxes, torch.float64, dev), _dev(scores, torch.float64, dev), _dev(labels, torch.int32, dev)
    gt_boxes = _dev(gt_boxes, torch.float64, dev).reshape(-1, 4)
    gt_labels, gt_offsets = _dev(gt_labels, torch.int32, dev).reshape(-1), _dev(gt_offsets, torch.int32, dev).reshape(-1)
    ignore = None if ignore is None else _dev(ignore, torch.uint8, dev).reshape(-1)
    if num_classes is None:
        num_classes = 1 + max(int(labels.max()) if labels.numel() else 0, int(gt_labels.max()) if gt_labels.numel() else 0)
    match, det_ignored, npos = ops.det_match(ctx, boxes, scores, labels, gt_boxes, gt_labels, gt_offsets, num_classes, thr, rule=rule,
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


def evaluate(generator, model, iou_threshold=0.5, score_threshold=0.05, max_detections=100, save_path=None, ctx=None):
    """utils/eval.py:147-235: {label: (average_precision, num_annotations)} of `model` over `generator`, for every label the
    generator has; (0, 0) for a label without annotations.  The generator is read as the reference reads it (size, num_classes,
    has_label, load_image, preprocess_image, resize_image, load_annotations), model.predict_on_batch(...)[:3] are boxes, scores,
    labels; per image the detections above score_threshold, best max_detections first.  The images' detections are gathered
    into one padded batch; matching, curves and the integral run on the device (evaluate_detections, rule 'reference').
    Equal scores keep their input order here (the reference's argsort leaves them undefined).  Drawing is not part of this
    loop: save_path other than None raises NotImplementedError; visualization.save_detection_images writes those images."""
    if save_path is not None:
        raise NotImplementedError("evaluate: save_path (drawing detections) is not implemented here: "
                                  "utils.visualization.save_detection_images(generator, model, save_path) writes the images")
    n_img, n_class, cap = generator.size(), generator.num_classes(), int(max_detections)
    boxes = np.zeros((n_img, cap, 4), np.float64)
    scores = np.zeros((n_img, cap), np.float64)
    labels = np.full((n_img, cap), -1, np.int32)
    gt_boxes, gt_labels, gt_offsets = [], [], [0]
    for i in range(n_img):
        raw_image = generator.load_image(i)
        image = generator.preprocess_image(raw_image.copy())
        image, scale = generator.resize_image(image)
        out = model.predict_on_batch(np.expand_dims(image, axis=0))[:3]
        b, s, l = (np.asarray(o.cpu() if torch.is_tensor(o) else o) for o in out)
        b = b.astype(np.float64) / scale
        idx = np.where(s[0, :] > score_threshold)[0]
        idx = idx[np.argsort(-s[0][idx], kind="stable")[:cap]]
        n = idx.size
        boxes[i, :n], scores[i, :n], labels[i, :n] = b[0, idx, :4], s[0, idx], l[0, idx]
        ann = generator.load_annotations(i)
        gt_boxes.append(np.asarray(ann["bboxes"], np.float64).reshape(-1, 4))
        gt_labels.append(np.asarray(ann["labels"]).reshape(-1).astype(np.int32))
        gt_offsets.append(gt_offsets[-1] + gt_labels[-1].size)
    labels[(labels >= n_class)] = -1  # (a label the generator does not know is scored nowhere, as in the reference's per-label loop)
    gt_boxes = np.concatenate(gt_boxes) if gt_boxes else np.zeros((0, 4))
    gt_labels = np.concatenate(gt_labels) if gt_labels else np.zeros((0,), np.int32)
    res = evaluate_detections((boxes, scores, labels), (gt_boxes, gt_labels, np.asarray(gt_offsets, np.int32)), rule="reference",
                              iou_thresholds=(iou_threshold,), num_classes=n_class, ctx=ctx)
    average_precisions = {}
    for label in range(n_class):
        if not generator.has_label(label):
            continue
        n = int(res["npos"][label])
        average_precisions[label] = (float(res["ap"][0, label]), float(n)) if n else (0, 0)
    return average_precisions
