"""numpy restatement of pp_vote_cluster (pyrapose_amd/csrc/cluster.hip; semantics in include/pyrapose_hip.h) and the scene
builders of its tests.  The step has no counterpart in the reference, which assumes one object per class per image
(utils/tless_eval.py:378): the restatement is the specification, the kernel must agree with it exactly.

float32 where the kernel is float32 (vote boxes by min / max, the score compare), float64 for the IoU with every product and
sum rounded on its own (numpy never contracts them)."""
import numpy as np

from tests.test_oracle_pnp import BOX, K4, make_votes  # noqa: F401  (BOX and K4 are re-exported to the tests)


def vote_boxes(votes16):
    """[k,16] float32 corner votes -> ([k,4] float32 (x1, y1, x2, y2), valid [k]: every corner finite)"""
    v = np.asarray(votes16, np.float32).reshape(-1, 8, 2)
    valid = np.isfinite(v).all((1, 2))
    with np.errstate(invalid="ignore"):
        box = np.concatenate([v.min(1), v.max(1)], 1).astype(np.float32)
    return box, valid


def iou(a, b):
    """IoU of box a [4] with boxes b [k,4], float64, no '+1' convention"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64).reshape(-1, 4)
    w = np.maximum(0.0, np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]))
    h = np.maximum(0.0, np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]))
    inter = w * h
    ua = ((a[2] - a[0]) * (a[3] - a[1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) - inter
    out = np.zeros_like(inter)
    np.divide(inter, ua, out=out, where=ua > 0)
    return out


def cluster_cell(boxes, valid, score, iou_thr, min_votes, max_instances, max_rounds):
    """one (image, class): boxes [k,4] float32, valid [k], score [k] float32 in list (ascending anchor) order ->
    (inst [k], list of leader positions of the kept clusters)"""
    k = len(score)
    state = np.where(valid, -2, -1).astype(np.int32)  # -2 unassigned, -1 out, >= 0 instance
    score = np.asarray(score, np.float32)
    leaders, rounds = [], 0
    while rounds < max_rounds and len(leaders) < max_instances:
        un = np.nonzero(state == -2)[0]
        if len(un) == 0:
            break
        rounds += 1
        lv = int(un[np.argmax(score[un])])  # first maximum: ties go to the lowest position = lowest anchor
        members = un[(iou(boxes[lv], boxes[un]) > iou_thr) | (un == lv)]
        if len(members) >= min_votes:
            state[members] = len(leaders)
            leaders.append(lv)
        else:
            state[members] = -1
    state[state == -2] = -1
    assert k == len(state)
    return state, leaders


def vote_cluster(boxes3d, scores, idx, counts, iou_thr=0.5, min_votes=10, max_instances=8, max_rounds=None):
    """boxes3d [B,N,16] float32, scores [B,N,C] float32, idx [B,C,cap] int32, counts [B,C] int32 -> the six outputs of
    pp_vote_cluster: inst, order [B,C,cap], inst_offsets [B,C,max_instances+1], n_inst [B,C], leader [B,C,max_instances] int32,
    inst_box [B,C,max_instances,4] float32"""
    boxes3d, scores = np.asarray(boxes3d, np.float32), np.asarray(scores, np.float32)
    B, C, cap = idx.shape
    mi = int(max_instances)
    mr = 4 * mi if max_rounds is None else int(max_rounds)
    inst = np.full((B, C, cap), -1, np.int32)
    order = np.full((B, C, cap), -1, np.int32)
    offs = np.zeros((B, C, mi + 1), np.int32)
    n_inst = np.zeros((B, C), np.int32)
    leader = np.full((B, C, mi), -1, np.int32)
    inst_box = np.zeros((B, C, mi, 4), np.float32)
    for b in range(B):
        for c in range(C):
            cnt = min(int(counts[b, c]), cap)
            if cnt <= 0:
                continue
            a = idx[b, c, :cnt]
            bx, valid = vote_boxes(boxes3d[b, a])
            state, leaders = cluster_cell(bx, valid, scores[b, a, c], iou_thr, min_votes, mi, mr)
            inst[b, c, :cnt] = state
            pos = 0
            for k, lv in enumerate(leaders):
                mem = a[state == k]
                offs[b, c, k] = pos
                order[b, c, pos:pos + len(mem)] = mem
                pos += len(mem)
                leader[b, c, k] = a[lv]
                inst_box[b, c, k] = bx[lv]
            offs[b, c, len(leaders):] = pos
            n_inst[b, c] = len(leaders)
    return inst, order, offs, n_inst, leader, inst_box


def threshold_compact(scores, thr=0.5, cap=None):
    """np.where per (image, class) in the layout of pp_score_threshold_compact"""
    B, N, C = scores.shape
    cap = int(cap or N)
    idx = np.full((B, C, cap), -1, np.int32)
    cnt = np.zeros((B, C), np.int32)
    for b in range(B):
        for c in range(C):
            hit = np.nonzero(scores[b, :, c] > np.float32(thr))[0]
            cnt[b, c] = len(hit)
            idx[b, c, :min(len(hit), cap)] = hit[:cap]
    return idx, cnt


# ---------------------------------------------------------------------------------------------------------------- scenes
def base_uv(rng):
    """the 8 projected cuboid corners [8,2] of one random pose of make_votes"""
    return make_votes(rng, 1, 0.0, 0.0)[3].reshape(8, 2)


def uv_box(uv):
    uv = np.asarray(uv).reshape(-1, 2)
    return np.array([uv[:, 0].min(), uv[:, 1].min(), uv[:, 0].max(), uv[:, 1].max()])


def votes_about(rng, uv, k, centre=None, noise=1.0):
    """k votes [k,16] around the corner set uv, moved so that its box centre lies at `centre` (pixels)"""
    uv = np.asarray(uv, np.float64).reshape(8, 2)
    if centre is not None:
        x1, y1, x2, y2 = uv_box(uv)
        uv = uv + (np.asarray(centre, np.float64) - np.array([(x1 + x2) / 2, (y1 + y2) / 2]))
    return (uv[None] + rng.normal(scale=noise, size=(k, 8, 2))).reshape(k, 16)


class Scene(object):
    """network outputs under construction: background boxes uniform in the image with scores below the threshold"""

    def __init__(self, rng, B, N, C):
        self.rng, self.N = rng, N
        self.boxes3d = rng.uniform(0, 600, size=(B, N, 16)).astype(np.float32)
        self.scores = rng.uniform(0.0, 0.3, size=(B, N, C)).astype(np.float32)
        self.free = [list(rng.permutation(N)) for _ in range(B)]

    def put(self, b, c, votes16, score=None):
        """place votes on unused anchors of image b (ascending), scores uniform in (0.55, 0.99) unless given; -> the anchors"""
        k = len(votes16)
        anchors = np.sort(np.array([self.free[b].pop() for _ in range(k)]))
        self.boxes3d[b, anchors] = np.asarray(votes16, np.float32)
        self.scores[b, anchors, c] = self.rng.uniform(0.55, 0.99, size=k).astype(np.float32) if score is None else np.asarray(score, np.float32)
        return anchors


def mixed_scene(seed=0):
    """B = 2, C = 3, N = 600: the cells of the exact-agreement test (for iou 0.5, min_votes 10, max_instances 2).
    -> (boxes3d, scores, expected n_inst [2,3])"""
    rng = np.random.default_rng(seed)
    sc = Scene(rng, 2, 600, 3)
    # (0, 0): two separated instances, 40 + 25 votes, scores quantised to 0.05 so that the best score is shared (the tie rule)
    q = lambda k: (np.round(rng.uniform(0.6, 0.95, size=k) * 20) / 20).astype(np.float32)
    uv = base_uv(rng)
    sc.put(0, 0, votes_about(rng, uv, 40, (150, 150)), q(40))
    sc.put(0, 0, votes_about(rng, base_uv(rng), 25, (450, 330)), q(25))
    # (0, 1): two instances of one corner set, the second shifted by 0.538 of the box width: IoU about 0.3 between their boxes
    x1, _y1, x2, _y2 = uv_box(uv)
    sc.put(0, 1, votes_about(rng, uv, 30, (300, 120)))
    sc.put(0, 1, votes_about(rng, uv, 20, (300 + 0.538 * (x2 - x1), 120)))
    # (0, 2): one instance, one of its votes with a NaN corner
    v = votes_about(rng, base_uv(rng), 22, (120, 380))
    v[7, 5] = np.nan
    sc.put(0, 2, v)
    # (1, 0): no vote.  (1, 1): six votes, below min_votes
    sc.put(1, 1, votes_about(rng, base_uv(rng), 6, (200, 200)))
    # (1, 2): three instances, more than max_instances = 2
    for k, centre in ((15, (100, 100)), (14, (320, 240)), (13, (520, 380))):
        sc.put(1, 2, votes_about(rng, base_uv(rng), k, centre))
    return sc.boxes3d, sc.scores, np.array([[2, 2, 1], [0, 0, 2]], np.int32)


def large_scene(seed=1):
    """B = 1, C = 1, N = 3000: 2500 votes in three instances (1200 + 800 + 500) -> (boxes3d, scores, expected counts)"""
    rng = np.random.default_rng(seed)
    sc = Scene(rng, 1, 3000, 1)
    for k, centre in ((1200, (110, 120)), (800, (330, 250)), (500, (530, 370))):
        sc.put(0, 0, votes_about(rng, base_uv(rng), k, centre))
    return sc.boxes3d, sc.scores, (1200, 800, 500)


def separated_poses(rng, n, k, noise, outlier_frac, max_draws=2000):
    """n draws of make_votes(rng, k, noise, outlier_frac) whose noise-free vote boxes lie at least a box width (or a box height)
    apart, centre to centre, and so do not overlap: draws that come closer to an accepted one are thrown away.
    -> list of (R, t, votes [k,16], clean [k])"""
    out = []
    for _ in range(max_draws):
        R, t, _obj, img, clean = make_votes(rng, k, noise, outlier_frac)
        box = uv_box(img.reshape(k, 8, 2)[clean[::8]].mean(0))
        ok = True
        for o in out:
            dx = abs((box[0] + box[2]) - (o[4][0] + o[4][2])) / 2
            dy = abs((box[1] + box[3]) - (o[4][1] + o[4][3])) / 2
            ok = ok and (dx >= max(box[2] - box[0], o[4][2] - o[4][0]) or dy >= max(box[3] - box[1], o[4][3] - o[4][1]))
        if ok:
            out.append((R, t, img.reshape(k, 16), clean[::8], box))
        if len(out) == n:
            return [o[:4] for o in out]
    raise RuntimeError("separated_poses: no %d separated poses in %d draws" % (n, max_draws))


def two_instance_scene(seed=3, N=2000, k=40, noise=1.0, outlier_frac=0.2):
    """B = 1, C = 2: class 0 holds two poses a box width apart, class 1 one pose; every pose k votes of make_votes.
    -> (boxes3d, scores, truth: list of (cls, R, t, anchors, clean) in (class, first anchor-independent) creation order)"""
    rng = np.random.default_rng(seed)
    sc = Scene(rng, 1, N, 2)
    poses = separated_poses(rng, 3, k, noise, outlier_frac)
    truth = []
    for cls, (R, t, votes, clean) in zip((0, 0, 1), poses):
        truth.append((cls, R, t, sc.put(0, cls, votes), clean))
    return sc.boxes3d, sc.scores, truth


def single_instance_scene(seed=4, N=1500):
    """B = 2, C = 3: every (image, class) holds one pose of 30 votes with 1 px noise and no outlier: one cluster takes them all"""
    rng = np.random.default_rng(seed)
    sc = Scene(rng, 2, N, 3)
    for b in range(2):
        for (R, t, votes, _clean), c in zip(separated_poses(rng, 3, 30, 1.0, 0.0), range(3)):
            sc.put(b, c, votes)
    return sc.boxes3d, sc.scores
