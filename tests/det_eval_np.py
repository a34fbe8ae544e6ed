"""float64 numpy restatement of the detection-metric entry points (csrc/det_eval.hip, include/pyrapose_hip.h), written from the
rules stated there: both matching rules (the reference's utils/eval.py:187-211 and pycocotools' evaluateImg without crowd), the
true / false positive scans with the precision envelope, and both integrations -- the sums in the kernel's documented order, so
the device results can be compared bit for bit.  numpy's elementwise float64 operations round each product, quotient and sum on
its own, as the kernels (compiled without FMA contraction) do."""
import numpy as np

EPS = np.finfo(np.float64).eps
AP_THREADS = 256  # workgroup of det_ap_kernel: contiguous per-thread partials, then a halving tree


def iou_plus1(d, g):
    """compute_overlap.pyx with the detection d [4] as the `boxes` row and g [n,4] as `query_boxes` -> [n]"""
    g = np.asarray(g, np.float64).reshape(-1, 4)
    area = (g[:, 2] - g[:, 0] + 1) * (g[:, 3] - g[:, 1] + 1)
    iw = np.minimum(d[2], g[:, 2]) - np.maximum(d[0], g[:, 0]) + 1
    ih = np.minimum(d[3], g[:, 3]) - np.maximum(d[1], g[:, 1]) + 1
    ua = (d[2] - d[0] + 1) * (d[3] - d[1] + 1) + area - iw * ih
    with np.errstate(all="ignore"):
        return np.where((iw > 0) & (ih > 0), iw * ih / ua, 0.0)


def iou_plain(d, g):
    """pycocotools' bbIou without crowd, on corner boxes: no '+1'"""
    g = np.asarray(g, np.float64).reshape(-1, 4)
    area = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    iw = np.minimum(d[2], g[:, 2]) - np.maximum(d[0], g[:, 0])
    ih = np.minimum(d[3], g[:, 3]) - np.maximum(d[1], g[:, 1])
    i = iw * ih
    u = (d[2] - d[0]) * (d[3] - d[1]) + area - i
    with np.errstate(all="ignore"):
        return np.where((iw > 0) & (ih > 0), i / u, 0.0)


def score_order(scores, valid):
    """slots of the valid detections in descending score, equal scores by the lower slot"""
    slots = np.nonzero(valid)[0]
    return slots[np.argsort(-(scores[slots] + 0.0), kind="stable")]


def det_match(det_boxes, det_scores, det_labels, gt_boxes, gt_labels, gt_offsets, n_class, thresholds, rule, gt_ignore=None):
    """-> (match int32 [T,B,D], det_ignored uint8 [T,B,D], npos int32 [C])"""
    det_boxes, det_scores = np.asarray(det_boxes, np.float64), np.asarray(det_scores, np.float64)
    gt_boxes = np.asarray(gt_boxes, np.float64).reshape(-1, 4)
    B, D = det_scores.shape
    T, G = len(thresholds), gt_boxes.shape[0]
    ignore = np.zeros(G, bool) if gt_ignore is None else np.asarray(gt_ignore) != 0
    assert rule in ("reference", "coco") and (rule == "coco" or gt_ignore is None)
    match = np.full((T, B, D), -1, np.int32)
    ign = np.zeros((T, B, D), np.uint8)
    npos = np.array([np.count_nonzero((np.asarray(gt_labels) == c) & ~ignore) for c in range(n_class)], np.int32)
    for b in range(B):
        g0, g1 = int(gt_offsets[b]), int(gt_offsets[b + 1])
        labels_g, ignore_g = np.asarray(gt_labels[g0:g1]), ignore[g0:g1]
        valid = (det_labels[b] >= 0) & (det_labels[b] < n_class)
        order = score_order(det_scores[b], valid)
        iou = {}
        for d in order:  # the overlaps do not depend on the threshold
            own = np.nonzero(labels_g == det_labels[b, d])[0]
            iou[d] = (own, (iou_plus1 if rule == "reference" else iou_plain)(det_boxes[b, d], gt_boxes[g0:g1][own]))
        for t, thr in enumerate(thresholds):
            taken = np.zeros(g1 - g0, bool)
            for d in order:
                own, v = iou[d]
                if own.size == 0:
                    continue
                if rule == "reference":
                    k = int(np.argmax(v))  # first maximum, taken or not
                    if v[k] >= thr and not taken[own[k]]:
                        taken[own[k]] = True
                        match[t, b, d] = g0 + own[k]
                else:
                    floor, m = min(thr, 1 - 1e-10), -1
                    visit = [k for k in range(own.size) if not ignore_g[own[k]]] + [k for k in range(own.size) if ignore_g[own[k]]]
                    for k in visit:
                        if taken[own[k]]:
                            continue
                        if m > -1 and not ignore_g[own[m]] and ignore_g[own[k]]:
                            break
                        if v[k] < floor:
                            continue
                        floor, m = v[k], k
                    if m > -1:
                        taken[own[m]] = True
                        match[t, b, d] = g0 + own[m]
                        ign[t, b, d] = 1 if ignore_g[own[m]] else 0
    return match, ign, npos


def det_order(det_scores, det_labels, n_class):
    """class-major, then descending score, then ascending flat slot -> (order int32 [N], class_offsets int32 [C+1])"""
    s, l = np.asarray(det_scores, np.float64).reshape(-1), np.asarray(det_labels).reshape(-1)
    parts = [score_order(s, l == c) for c in range(n_class)]
    offsets = np.zeros(n_class + 1, np.int32)
    offsets[1:] = np.cumsum([p.size for p in parts])
    return (np.concatenate(parts) if parts else np.zeros(0)).astype(np.int32), offsets


def pr_curve(order, class_offsets, match, det_ignored, npos):
    """-> (tp int32 [T,N], fp int32 [T,N], recall [T,N], prec_env [T,N])"""
    T, N = match.shape[0], order.shape[0]
    m, ig = match.reshape(T, -1), det_ignored.reshape(T, -1)
    tp, fp = np.zeros((T, N), np.int32), np.zeros((T, N), np.int32)
    recall, env = np.zeros((T, N)), np.zeros((T, N))
    for c in range(len(npos)):
        lo, hi = int(class_offsets[c]), int(class_offsets[c + 1])
        if hi <= lo:
            continue
        seg = order[lo:hi]
        for t in range(T):
            keep = ig[t, seg] == 0
            a = np.cumsum(keep & (m[t, seg] >= 0), dtype=np.int32)
            f = np.cumsum(keep & (m[t, seg] < 0), dtype=np.int32)
            tp[t, lo:hi], fp[t, lo:hi] = a, f
            ad = a.astype(np.float64)
            recall[t, lo:hi] = ad / float(npos[c]) if npos[c] > 0 else 0.0
            prec = ad / np.maximum(ad + f.astype(np.float64), EPS)
            env[t, lo:hi] = np.maximum(np.maximum.accumulate(prec[::-1])[::-1], 0.0)
    return tp, fp, recall, env


def ap_area(rec, env):
    """_compute_ap's sum in the kernel's order: AP_THREADS contiguous partials, each added in ascending index onto 0.0, folded
    by the halving tree p[k] += p[k + s], s = 128 .. 1"""
    n = rec.shape[0]
    per = -(-n // AP_THREADS)
    prev = np.concatenate([[0.0], rec[:-1]])
    part = np.zeros(AP_THREADS)
    for k in range(AP_THREADS):
        s = 0.0
        for j in range(min(k * per, n), min((k + 1) * per, n)):
            if rec[j] != prev[j]:
                s = s + (rec[j] - prev[j]) * env[j]
        part[k] = s
    s = AP_THREADS // 2
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def ap_101(rec, env):
    """COCO accumulate: searchsorted-left at np.linspace(0, 1, 101), the 101 values added in index order, / 101"""
    n = rec.shape[0]
    idx = np.searchsorted(rec, np.linspace(0.0, 1.0, 101), side="left")
    s = 0.0
    for i in idx:
        s = s + (env[i] if i < n else 0.0)
    return s / 101.0


def det_ap(class_offsets, npos, recall, prec_env, integration):
    """-> (ap [T,C], recall_final [T,C])"""
    T, C = recall.shape[0], len(npos)
    ap, rf = np.zeros((T, C)), np.zeros((T, C))
    for c in range(C):
        lo, hi = int(class_offsets[c]), int(class_offsets[c + 1])
        for t in range(T):
            if npos[c] <= 0:
                ap[t, c] = rf[t, c] = 0.0 if integration == "area" else -1.0
                continue
            rec, env = recall[t, lo:hi], prec_env[t, lo:hi]
            ap[t, c] = ap_area(rec, env) if integration == "area" else ap_101(rec, env)
            rf[t, c] = rec[-1] if hi > lo else 0.0
    return ap, rf


def evaluate(det_boxes, det_scores, det_labels, gt_boxes, gt_labels, gt_offsets, n_class, thresholds, rule, integration, gt_ignore=None):
    """the whole chain -> dict(match, det_ignored, npos, order, class_offsets, tp, fp, recall, prec_env, ap, recall_final)"""
    match, ign, npos = det_match(det_boxes, det_scores, det_labels, gt_boxes, gt_labels, gt_offsets, n_class, thresholds, rule, gt_ignore)
    order, offs = det_order(det_scores, det_labels, n_class)
    tp, fp, recall, env = pr_curve(order, offs, match, ign, npos)
    ap, rf = det_ap(offs, npos, recall, env, integration)
    return dict(match=match, det_ignored=ign, npos=npos, order=order, class_offsets=offs, tp=tp, fp=fp, recall=recall, prec_env=env,
                ap=ap, recall_final=rf)


class FakeGenerator(object):
    """The generator surface utils/eval.py reads, over stored annotations: image i is a [2,2,3] array holding i; resize_image
    reports `scale` (the model's boxes are in the resized image, evaluate divides them by it)."""

    def __init__(self, gt_boxes, gt_labels, gt_offsets, has_label, scale):
        self.gt_boxes, self.gt_labels, self.gt_offsets = np.asarray(gt_boxes, np.float64), np.asarray(gt_labels), np.asarray(gt_offsets)
        self.has, self.scale = np.asarray(has_label).astype(bool), float(scale)

    def size(self):
        return len(self.gt_offsets) - 1

    def num_classes(self):
        return len(self.has)

    def has_label(self, label):
        return bool(self.has[label])

    def label_to_name(self, label):
        return "class%d" % label

    def load_image(self, i):
        return np.full((2, 2, 3), float(i))

    def preprocess_image(self, image):
        return image

    def resize_image(self, image):
        return image, self.scale

    def load_annotations(self, i):
        lo, hi = int(self.gt_offsets[i]), int(self.gt_offsets[i + 1])
        return {"bboxes": self.gt_boxes[lo:hi].copy(), "labels": self.gt_labels[lo:hi].copy()}


class FakeModel(object):
    """predict_on_batch of a stored raw output: boxes [B,N,4] float64 (in the resized image), scores [B,N], labels [B,N]"""

    def __init__(self, boxes, scores, labels):
        self.boxes, self.scores, self.labels = boxes, scores, labels

    def predict_on_batch(self, x):
        i = int(x[0, 0, 0, 0])
        return [self.boxes[i:i + 1].copy(), self.scores[i:i + 1].copy(), self.labels[i:i + 1].copy(), None]
