"""Plain numpy-and-loops restatement of pp_cc_label / pp_cc_select (csrc/cc.hip, the rule in include/pyrapose_hip.h) and of the
instance ordering of utils.components.instances_from_mask_output.  Labelling is a breadth-first search started from every
unlabelled foreground pixel in raster order, so component k is the k-th one met: scipy.ndimage.label's numbering, which
tests/test_cc_cpu.py pins.  Integers only."""
from collections import deque

import numpy as np

MODES = ("binary", "value")
N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def label_plane(plane, connectivity=8, mode="binary"):
    """uint8 [H,W] -> (labels int32 [H,W], n)"""
    assert connectivity in (4, 8) and mode in MODES
    plane = np.asarray(plane, np.uint8)
    H, W = plane.shape
    v = plane if mode == "value" else (plane != 0).astype(np.uint8)
    labels = np.zeros((H, W), np.int32)
    steps = N8 if connectivity == 8 else N4
    n = 0
    for y in range(H):
        for x in range(W):
            if v[y, x] == 0 or labels[y, x]:
                continue
            n += 1
            labels[y, x] = n
            todo = deque([(y, x)])
            while todo:
                cy, cx = todo.popleft()
                for dy, dx in steps:
                    qy, qx = cy + dy, cx + dx
                    if 0 <= qy < H and 0 <= qx < W and labels[qy, qx] == 0 and v[qy, qx] == v[y, x]:
                        labels[qy, qx] = n
                        todo.append((qy, qx))
    return labels, n


def cc_label(planes, connectivity=8, mode="binary", weight=None, max_components=256):
    """uint8 [N,H,W] (+ int32 weight) -> dict(labels int32 [N,H,W], counts int32 [N], stats int32 [N,M,6], sums int64 [N,M,3])"""
    planes = np.asarray(planes, np.uint8)
    N, H, W = planes.shape
    M = int(max_components)
    assert 1 <= M <= 65535
    labels = np.zeros((N, H, W), np.int32)
    counts = np.zeros((N,), np.int32)
    stats = np.zeros((N, M, 6), np.int32)
    sums = np.zeros((N, M, 3), np.int64)
    for i in range(N):
        labels[i], n = label_plane(planes[i], connectivity, mode)
        counts[i] = n
        for k in range(min(n, M)):
            ys, xs = np.nonzero(labels[i] == k + 1)
            value = int(planes[i][ys[0], xs[0]]) if mode == "value" else 1
            stats[i, k] = (len(ys), xs.min(), ys.min(), xs.max(), ys.max(), value)
            sw = 0 if weight is None else int(np.asarray(weight)[i][ys, xs].astype(np.int64).sum())
            sums[i, k] = (int(xs.astype(np.int64).sum()), int(ys.astype(np.int64).sum()), sw)
    return dict(labels=labels, counts=counts, stats=stats, sums=sums)


def cc_select(labels, slot_plane, slot_label):
    labels = np.asarray(labels, np.int32)
    N, H, W = labels.shape
    masks = np.zeros((len(slot_plane), H, W), np.uint8)
    for s, (p, l) in enumerate(zip(slot_plane, slot_label)):
        if 0 <= p < N and l > 0:
            masks[s] = labels[p] == l
    return masks


def select_components(result, min_area=1, keep=None, order="area"):
    """-> (slot_plane int32 [N*K], slot_label int32 [N*K], masks uint8 [N*K,H,W]), K = keep or M.  Per plane the components of
    the first M with area >= min_area, the largest area (order 'weight': the largest sum_w / area as a float64 quotient) first,
    ties by the smaller label; unused slots are (-1, 0)."""
    stats, sums, labels = result["stats"], result["sums"], result["labels"]
    N, M = stats.shape[:2]
    K = M if keep is None else min(int(keep), M)
    slot_plane = np.full((N, K), -1, np.int32)
    slot_label = np.zeros((N, K), np.int32)
    for i in range(N):
        cand = []
        for k in range(M):
            area = int(stats[i, k, 0])
            if area >= max(int(min_area), 1):
                key = area if order == "area" else np.float64(sums[i, k, 2]) / np.float64(area)
                cand.append((-key, k + 1))
        cand.sort()
        for j, (_, lab) in enumerate(cand[:K]):
            slot_plane[i, j], slot_label[i, j] = i, lab
    return slot_plane.reshape(-1), slot_label.reshape(-1), cc_select(labels, slot_plane.reshape(-1), slot_label.reshape(-1))


def largest_component(masks, connectivity=8, mode="binary"):
    masks = np.asarray(masks, np.uint8)
    shape = masks.shape
    planes = masks.reshape((-1,) + shape[-2:])
    out = np.zeros_like(planes)
    for i, p in enumerate(planes):
        labels, n = label_plane(p, connectivity, mode)
        if n:
            areas = np.bincount(labels.ravel(), minlength=n + 1)[1:]
            out[i] = labels == 1 + int(np.argmax(areas))  # argmax: the first, i.e. the smaller label, among equals
    return out.reshape(shape)


def remove_small(masks, min_area, connectivity=8, mode="binary", max_components=256):
    """pixels of the components among the first M with area >= min_area keep their byte, all others become 0"""
    masks = np.asarray(masks, np.uint8)
    shape = masks.shape
    planes = masks.reshape((-1,) + shape[-2:])
    out = np.zeros_like(planes)
    for i, p in enumerate(planes):
        labels, n = label_plane(p, connectivity, mode)
        areas = np.bincount(labels.ravel(), minlength=n + 1)
        for k in range(1, min(n, max_components) + 1):
            if areas[k] >= min_area:
                out[i][labels == k] = p[labels == k]
    return out.reshape(shape)


def instances_from_mask_output(pred, mask_hw, threshold=0.5, connectivity=8, min_area=4, max_instances=8, max_components=256):
    """pred float32 [B,h*w,C] or [B,h,w,C] -> dict(det_masks uint8 [B,D,h,w], det_scores float64 [B,D], det_labels int32 [B,D],
    boxes int32 [B,D,4] = (x_min, y_min, x_max, y_max) inclusive); padding: label -1, score 0, zero mask and box."""
    h, w = mask_hw
    pred = np.asarray(pred, np.float32)
    B, C = pred.shape[0], pred.shape[-1]
    pred = pred.reshape(B, h, w, C)
    D = int(max_instances)
    planes = (pred > np.float32(threshold)).astype(np.uint8).transpose(0, 3, 1, 2).reshape(B * C, h, w)
    weight = np.floor(pred.astype(np.float64) * 65535.0 + 0.5).astype(np.int32).transpose(0, 3, 1, 2).reshape(B * C, h, w)
    res = cc_label(planes, connectivity, "binary", weight, max_components)
    det_masks = np.zeros((B, D, h, w), np.uint8)
    det_scores = np.zeros((B, D), np.float64)
    det_labels = np.full((B, D), -1, np.int32)
    boxes = np.zeros((B, D, 4), np.int32)
    for b in range(B):
        cand = []
        for c in range(C):
            for k in range(max_components):
                area = int(res["stats"][b * C + c, k, 0])
                if area >= max(int(min_area), 1):
                    score = np.float64(res["sums"][b * C + c, k, 2]) / np.float64(65535 * area)
                    cand.append((-score, c, k + 1))
        cand.sort()
        for j, (neg, c, lab) in enumerate(cand[:D]):
            det_masks[b, j] = res["labels"][b * C + c] == lab
            det_scores[b, j], det_labels[b, j] = -neg, c
            boxes[b, j] = res["stats"][b * C + c, lab - 1, 1:5]
    return dict(det_masks=det_masks, det_scores=det_scores, det_labels=det_labels, boxes=boxes)


# ---- the fixed cases shared by the CPU and the GPU tests ----

def random_plane(rng, H, W, density):
    return (rng.random((H, W)) < density).astype(np.uint8) * 255


def diagonal(n=64):
    """a one-pixel diagonal through the corner where four 32 x 32 tiles meet"""
    p = np.zeros((n, n), np.uint8)
    p[np.arange(n), np.arange(n)] = 1
    return p


def serpentine(H=96, W=96):
    """a one-pixel-wide path: every other row full, joined at alternating ends"""
    p = np.zeros((H, W), np.uint8)
    p[0::2, :] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        p[y, W - 1 if k % 2 == 0 else 0] = 1
    return p


def u_shape(H=70, W=70):
    """two arms that join only in the last tile row"""
    p = np.zeros((H, W), np.uint8)
    p[2:H - 1, 5] = 1
    p[2:H - 1, W - 4] = 1
    p[H - 2, 5:W - 3] = 1
    return p


def checkerboard(n=33):
    yy, xx = np.mgrid[0:n, 0:n]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def late_tile_first(H=40, W=70):
    """two components whose first pixels lie in different tiles; the tile further on (x >= 32) holds the earlier raster index"""
    p = np.zeros((H, W), np.uint8)
    p[1:4, 40:45] = 1   # first pixel (1, 40): tile column 1
    p[2:6, 3:9] = 1     # first pixel (2, 3): tile column 0
    return p


def rectangles(same):
    p = np.zeros((40, 70), np.uint8)
    p[5:30, 10:35] = 7
    p[12:38, 35:60] = 7 if same else 9
    return p


def discs():
    """an id image of three overlapping discs (the first flattened to semi-axes 30 x 7.5, so that a disc can cut it): the middle
    one, drawn last, is wider than the first is high and splits it in two"""
    yy, xx = np.mgrid[0:48, 0:80]
    p = np.zeros((48, 80), np.uint8)
    p[16 * (yy - 24) ** 2 + (xx - 34) ** 2 <= 30 ** 2] = 1
    p[(yy - 22) ** 2 + (xx - 64) ** 2 <= 14 ** 2] = 2
    p[(yy - 24) ** 2 + (xx - 34) ** 2 <= 10 ** 2] = 3
    return p
