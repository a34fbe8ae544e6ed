"""Connected components on the device (ops.cc_label / ops.cc_select, csrc/cc.hip): from the mask head's class planes, or from
an id image, to instance labels, per-component statistics and instance masks.

* `label_masks`: planes -> labels numbered as scipy.ndimage.label numbers them, counts, stats, sums.
* `select_components`: the largest (or best-weighted) components per plane as slot tables and masks.
* `largest_component`, `remove_small`: the two clean-ups of a class mask before it goes into a cloud.
* `instances_from_mask_output`: the mask head's sigmoid output to scored instance masks in the layout
  utils.mask_eval.evaluate_masks takes:

      inst = instances_from_mask_output(pred, (h, w))
      evaluate_masks(inst["det_masks"], inst["det_scores"], inst["det_labels"], gt_masks, gt_labels, gt_offsets)

What the reference's area clustering (encode_area, annotate_val_LineMOD.py:88-130) hands to a PCL binary; its point-cloud
smoothness condition is not restated.  The numbering is scipy's (pinned in tests/test_cc_cpu.py); parity with
cv2.connectedComponents is unpinned.  Nothing here waits for the device: rankings are torch sorts on the stats tensors."""
import torch

from .. import ops
from ._host import to_device

_WEIGHT_ONE = 65535  # the integer weight of a sigmoid value of 1.0


def _ctx(ctx):
    if ctx is None:
        from ..runtime import default_context
        ctx = default_context()
    return ctx


def _planes(masks, name="masks"):
    """[..., H, W] array or tensor -> (uint8 cuda planes [N,H,W], the input's shape)"""
    masks = to_device(masks, torch.uint8)
    if masks.dim() < 2:
        raise ValueError("components: %s must be [..., H, W], got %s" % (name, list(masks.shape)))
    shape = tuple(masks.shape)
    return masks.reshape((-1,) + shape[-2:]), shape


def label_masks(masks, connectivity=8, mode="binary", weight=None, max_components=256, ctx=None):
    """masks uint8 [N,H,W] (or one [H,W]), weight int32 of the same shape or None; arrays or device tensors -> the dict of
    ops.cc_label on the device: labels int32 [N,H,W], counts int32 [N], stats int32 [N,M,6] (area, x_min, y_min, x_max, y_max,
    value), sums int64 [N,M,3] (sum_x, sum_y, sum_w), error int32 [1] (0 unless a kernel loop reached its bound)."""
    planes, _ = _planes(masks)
    if weight is not None:
        weight = to_device(weight, torch.int32, tuple(planes.shape))
    return ops.cc_label(_ctx(ctx), planes, connectivity, mode, weight, max_components)


def _rank(result, min_area, order):
    """-> (valid bool [N,M], order int64 [N,M]: the rows of each plane, the kept ones first, best first, ties by label)"""
    stats, sums = result["stats"], result["sums"]
    area = stats[:, :, 0].to(torch.int64)
    valid = area >= max(int(min_area), 1)
    if order == "area":
        key = area.to(torch.float64)  # (exact: an area is below 2^31)
    elif order == "weight":
        key = sums[:, :, 2].to(torch.float64) / area.clamp(min=1).to(torch.float64)
    else:
        raise ValueError("select_components: order %r, need area | weight" % (order,))
    key = torch.where(valid, key, torch.full_like(key, -1.0))
    return valid, torch.sort(key, dim=1, descending=True, stable=True).indices


def select_components(result, min_area=1, keep=None, order="area", ctx=None):
    """result: the dict of label_masks.  Per plane the `keep` (None: M) best components among the first M with area >=
    min_area: order 'area' the largest first, 'weight' the largest sum_w / area (a float64 quotient of the exact integers)
    first, ties by the smaller label -> (slot_plane int32 [N*K], slot_label int32 [N*K], masks uint8 [N*K,H,W]), plane i in
    the slots i K .. i K + K - 1, unused slots (-1, 0) with a zero mask.  No host synchronisation."""
    stats = result["stats"]
    N, M = int(stats.shape[0]), int(stats.shape[1])
    K = M if keep is None else min(int(keep), M)
    if K < 1:
        raise ValueError("select_components: keep must be at least 1, got %r" % (keep,))
    valid, idx = _rank(result, min_area, order)
    idx = idx[:, :K]
    ok = torch.gather(valid, 1, idx)
    plane = torch.arange(N, device=stats.device, dtype=torch.int32)[:, None].expand(N, K)
    slot_plane = torch.where(ok, plane, torch.full_like(plane, -1)).reshape(-1).contiguous()
    slot_label = torch.where(ok, (idx + 1).to(torch.int32), torch.zeros_like(plane)).reshape(-1).contiguous()
    return slot_plane, slot_label, ops.cc_select(_ctx(ctx), result["labels"], slot_plane, slot_label)


def largest_component(masks, connectivity=8, mode="binary", max_components=256, ctx=None):
    """masks [..., H, W] -> uint8 of the same shape, 1 on the largest component of each plane (the smaller label among equals;
    among its first max_components components), 0 elsewhere."""
    planes, shape = _planes(masks)
    result = ops.cc_label(_ctx(ctx), planes, connectivity, mode, None, max_components)
    return select_components(result, 1, 1, "area", ctx)[2].reshape(shape)


def remove_small(masks, min_area, connectivity=8, mode="binary", max_components=256, ctx=None):
    """masks [..., H, W] -> uint8 of the same shape: the pixels of components with area >= min_area keep their byte, the
    others become 0.  Components past the first max_components of a plane are never kept.  The keep table is looked up per
    pixel with a torch gather on the labels."""
    planes, shape = _planes(masks)
    result = ops.cc_label(_ctx(ctx), planes, connectivity, mode, None, max_components)
    N, M = int(result["stats"].shape[0]), int(result["stats"].shape[1])
    keep = torch.zeros((N, M + 2), dtype=torch.bool, device=planes.device)  # entry 0: background, entry M + 1: beyond M
    keep[:, 1:M + 1] = result["stats"][:, :, 0] >= max(int(min_area), 1)
    kept = torch.gather(keep, 1, result["labels"].reshape(N, -1).clamp(max=M + 1).to(torch.int64))
    return torch.where(kept.reshape(planes.shape), planes, torch.zeros_like(planes)).reshape(shape)


def instances_from_mask_output(pred, mask_hw, threshold=0.5, connectivity=8, min_area=4, max_instances=8, max_components=256, ctx=None):
    """The mask head's output to scored instance masks.  pred [B,h*w,C] or [B,h,w,C] float32: its sigmoid values, mask_hw =
    (h, w).  The planes are pred > threshold, one per image and class; a component of at least min_area pixels (among the first
    max_components of its plane) is an instance of that class with the score sum_w / (65535 area), one float64 quotient of
    exact integers, sum_w the sum of floor(pred 65535 + 0.5) (in float64) over its pixels.  Per image the max_instances best:
    score descending, then class ascending, then label ascending -> dict: det_masks uint8 [B,D,h,w], det_scores float64 [B,D],
    det_labels int32 [B,D] (-1 = padding: score 0, zero mask and box), boxes int32 [B,D,4] (x_min, y_min, x_max, y_max,
    inclusive).  No host synchronisation."""
    ctx = _ctx(ctx)
    h, w = int(mask_hw[0]), int(mask_hw[1])
    pred = to_device(pred, torch.float32)
    if pred.dim() not in (3, 4) or pred.numel() == 0 or pred.numel() % (pred.shape[0] * pred.shape[-1] * h * w):
        raise ValueError("instances_from_mask_output: pred must be [B,h*w,C] or [B,h,w,C] with (h, w) = %s, got %s" % ((h, w), list(pred.shape)))
    B, C, D = int(pred.shape[0]), int(pred.shape[-1]), int(max_instances)
    if D < 1:
        raise ValueError("instances_from_mask_output: max_instances must be at least 1")
    pred = pred.reshape(B, h, w, C).permute(0, 3, 1, 2)
    planes = (pred > threshold).to(torch.uint8).reshape(B * C, h, w).contiguous()
    weight = torch.floor(pred.to(torch.float64) * float(_WEIGHT_ONE) + 0.5).to(torch.int32).reshape(B * C, h, w).contiguous()
    result = ops.cc_label(ctx, planes, connectivity, "binary", weight, max_components)
    M = int(result["stats"].shape[1])
    stats, sums = result["stats"].reshape(B, C * M, 6), result["sums"].reshape(B, C * M, 3)
    area = stats[:, :, 0].to(torch.int64)
    valid = area >= max(int(min_area), 1)
    score = sums[:, :, 2].to(torch.float64) / (area.clamp(min=1) * _WEIGHT_ONE).to(torch.float64)
    score = torch.where(valid, score, torch.full_like(score, -1.0))
    # row c M + k of an image is class c, label k + 1: a stable sort leaves equal scores in class, then label order
    idx = torch.sort(score, dim=1, descending=True, stable=True).indices[:, :D]
    if idx.shape[1] < D:
        idx = torch.cat([idx, idx.new_zeros((B, D - idx.shape[1]))], dim=1)
        ok = torch.cat([torch.gather(valid, 1, idx[:, :C * M]), valid.new_zeros((B, D - C * M))], dim=1)
    else:
        ok = torch.gather(valid, 1, idx)
    cls, lab = (idx // M).to(torch.int32), (idx % M + 1).to(torch.int32)
    image = torch.arange(B, device=pred.device, dtype=torch.int32)[:, None]
    slot_plane = torch.where(ok, image * C + cls, torch.full_like(cls, -1)).reshape(-1).contiguous()
    slot_label = torch.where(ok, lab, torch.zeros_like(lab)).reshape(-1).contiguous()
    masks = ops.cc_select(ctx, result["labels"], slot_plane, slot_label).reshape(B, D, h, w)
    boxes = torch.gather(stats[:, :, 1:5], 1, idx[:, :, None].expand(B, D, 4))
    return dict(det_masks=masks, det_scores=torch.where(ok, torch.gather(score, 1, idx), torch.zeros_like(ok, dtype=torch.float64)),
                det_labels=torch.where(ok, cls, torch.full_like(cls, -1)),
                boxes=torch.where(ok[:, :, None], boxes, torch.zeros_like(boxes)).contiguous(), error=result["error"])
