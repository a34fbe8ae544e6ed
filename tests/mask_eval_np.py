"""numpy restatement of the segmentation-metric entry points (csrc/mask_eval.hip, pp_det_match_iou in csrc/det_eval.hip;
include/pyrapose_hip.h states the rules), with plain loops and sums.  Everything is integer work plus single float64 quotients,
so the device results are compared byte for byte.  The matching is det_eval_np.det_match itself, its two IoU functions
replaced by a look-up in the pair matrix."""
import numpy as np

import det_eval_np as DN

TILE_DET, TILE_GT = 4, 4  # pp_mask_iou_pairs' tile: the tests sit on both sides of it


def mask_confusion(pred, target, thresholds):
    """pred [B,M,C] float32, target [B,M,C+1] float32 -> counts int64 [T,C,3] (tp, fp, fn)"""
    pred, target = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    C = pred.shape[-1]
    p = pred.reshape(-1, C).astype(np.float64)
    s = target.reshape(-1, C + 1)[:, :C] != 0
    counts = np.zeros((len(thresholds), C, 3), np.int64)
    for t, thr in enumerate(thresholds):
        with np.errstate(invalid="ignore"):
            on = p > np.float64(thr)  # NaN compares false
        for c in range(C):
            counts[t, c] = (np.count_nonzero(on[:, c] & s[:, c]), np.count_nonzero(on[:, c] & ~s[:, c]), np.count_nonzero(~on[:, c] & s[:, c]))
    return counts


def mask_pack(masks):
    """[N,H,W] uint8 -> (words uint64 [N,ceil(HW/64)], area int64 [N], word_range int32 [N,2])"""
    masks = np.asarray(masks)
    N, HW = masks.shape[0], masks.shape[1] * masks.shape[2]
    n_word = (HW + 63) // 64
    words = np.zeros((N, n_word), np.uint64)
    area, rng = np.zeros(N, np.int64), np.zeros((N, 2), np.int32)
    for n in range(N):
        flat = masks[n].reshape(-1) != 0
        for k in range(n_word):
            w = 0
            for i, v in enumerate(flat[64 * k:64 * k + 64]):
                if v:
                    w |= 1 << i
            words[n, k] = w
        area[n] = int(flat.sum())
        full = np.nonzero(words[n])[0]
        if full.size:
            rng[n] = (full[0], full[-1] + 1)
    return words, area, rng


def popcount(w):
    return bin(int(w)).count("1")


def mask_iou_pairs(det_packed, gt_packed, gt_offsets, D, det_labels=None):
    """-> (iou float64 [D*G], inter int64 [D*G], pair_offsets int64 [B+1]); a slot with a label < 0 is padding: zeros"""
    dw, da, dr = det_packed
    gw, ga, gr = gt_packed
    gt_offsets = np.asarray(gt_offsets, np.int64)
    B, G = len(gt_offsets) - 1, gw.shape[0]
    iou, inter = np.zeros(D * G, np.float64), np.zeros(D * G, np.int64)
    pair_offsets = gt_offsets * D
    for b in range(B):
        g0, ng = int(gt_offsets[b]), int(gt_offsets[b + 1] - gt_offsets[b])
        for d in range(D):
            s = b * D + d
            if det_labels is not None and det_labels[b][d] < 0:
                continue
            for g in range(ng):
                lo, hi = max(dr[s, 0], gr[g0 + g, 0]), min(dr[s, 1], gr[g0 + g, 1])
                i = sum(popcount(dw[s, k] & gw[g0 + g, k]) for k in range(lo, hi))
                u = int(da[s]) + int(ga[g0 + g]) - i
                at = int(pair_offsets[b]) + d * ng + g
                inter[at] = i
                iou[at] = np.float64(i) / np.float64(u) if u > 0 else 0.0
    return iou, inter, pair_offsets


def brute_iou(a, b):
    """pixel loop over two [H,W] masks"""
    i = u = 0
    for y in range(a.shape[0]):
        for x in range(a.shape[1]):
            p, q = a[y, x] != 0, b[y, x] != 0
            i += int(p and q)
            u += int(p or q)
    return i / u if u else 0.0


def det_match_iou(iou, det_scores, det_labels, gt_labels, gt_offsets, n_class, thresholds, rule, gt_ignore=None):
    """det_eval_np.det_match on the pair matrix `iou` (mask_iou_pairs' layout): the boxes handed to it carry indices, and its
    two IoU functions look the pair up"""
    det_scores = np.asarray(det_scores, np.float64)
    B, D = det_scores.shape
    gt_offsets = np.asarray(gt_offsets, np.int64)
    G = int(gt_offsets[-1])
    image_of = np.repeat(np.arange(B), np.diff(gt_offsets))
    det_boxes = np.zeros((B, D, 4))
    det_boxes[:, :, 0], det_boxes[:, :, 1] = np.arange(B)[:, None], np.arange(D)[None, :]
    gt_boxes = np.zeros((G, 4))
    gt_boxes[:, 0] = np.arange(G)

    def lookup(d, g):
        b, slot = int(d[0]), int(d[1])
        g0, ng = int(gt_offsets[b]), int(gt_offsets[b + 1] - gt_offsets[b])
        out = np.zeros(len(g), np.float64)
        for j, row in enumerate(np.asarray(g).reshape(-1, 4)):
            gg = int(row[0])
            assert image_of[gg] == b
            out[j] = iou[D * g0 + slot * ng + (gg - g0)]
        return out

    saved = DN.iou_plus1, DN.iou_plain
    DN.iou_plus1 = DN.iou_plain = lookup
    try:
        return DN.det_match(det_boxes, det_scores, det_labels, gt_boxes, gt_labels, gt_offsets, n_class, thresholds, rule, gt_ignore)
    finally:
        DN.iou_plus1, DN.iou_plain = saved


def rle_counts(mask, order):
    """one [H,W] mask -> COCO's uncompressed counts (a list): alternating run lengths, the zero run first, in row-major
    ('row') or column-major ('column') order"""
    flat = (np.asarray(mask) != 0).reshape(-1) if order == "row" else (np.asarray(mask) != 0).T.reshape(-1)
    counts, run, cur = [], 0, False
    for v in flat:
        if bool(v) != cur:
            counts.append(run)
            run, cur = 0, bool(v)
        run += 1
    counts.append(run)
    return counts


def mask_rle(masks, order):
    """[N,H,W] -> (run_offsets int64 [N+1], counts int32)"""
    runs = [rle_counts(m, order) for m in masks]
    offs = np.zeros(len(runs) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in runs])
    return offs, np.asarray([c for r in runs for c in r], np.int32)


def mask_from_rle(counts, shape, order):
    """counts of one mask -> uint8 [H,W] of 0 / 255"""
    H, W = shape
    flat, v = [], 0
    for c in counts:
        flat += [v] * int(c)
        v = 255 - v
    assert len(flat) == H * W
    a = np.asarray(flat, np.uint8)
    return a.reshape(H, W) if order == "row" else a.reshape(W, H).T.copy()


def rle_string(mask):
    """the reference's rle_encode string from the row-major counts: 1-based starts and lengths of the set runs"""
    counts = rle_counts(mask, "row")
    out, pos = [], 0
    for i, c in enumerate(counts):
        if i % 2:
            out += [pos + 1, c]
        pos += c
    return " ".join(str(x) for x in out)


def scores(counts):
    """counts [T,C,3] -> (iou, precision, recall [T,C], miou [T]): single quotients, 0.0 on an empty denominator; miou over
    the classes with tp + fn > 0"""
    T, C = counts.shape[:2]
    iou, prec, rec, miou = np.zeros((T, C)), np.zeros((T, C)), np.zeros((T, C)), np.zeros(T)
    for t in range(T):
        have = []
        for c in range(C):
            tp, fp, fn = (int(v) for v in counts[t, c])
            iou[t, c] = tp / (tp + fp + fn) if tp + fp + fn else 0.0
            prec[t, c] = tp / (tp + fp) if tp + fp else 0.0
            rec[t, c] = tp / (tp + fn) if tp + fn else 0.0
            if tp + fn > 0:
                have.append(iou[t, c])
        miou[t] = np.mean(have) if have else 0.0
    return iou, prec, rec, miou


def rect_masks(boxes, H, W):
    """integer corner boxes [n,4] (x1, y1, x2, y2) -> filled rectangles [n,H,W] uint8 covering x1 <= x < x2, y1 <= y < y2: the
    mask's area is (x2 - x1)(y2 - y1), the box's area under iou_plain, and so is every intersection"""
    boxes = np.asarray(boxes).reshape(-1, 4).astype(np.int64)
    m = np.zeros((boxes.shape[0], H, W), np.uint8)
    for n, (x1, y1, x2, y2) in enumerate(boxes):
        m[n, max(y1, 0):max(y2, 0), max(x1, 0):max(x2, 0)] = 1
    return m
