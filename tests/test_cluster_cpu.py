"""CPU: the restatement of pp_vote_cluster (tests/cluster_np.py) on cases small enough to check by hand, the scenes of the
GPU tests against the instance counts those tests expect, and eval_pose.match_instances."""
import numpy as np

from tests import cluster_np as CN


def sq(x, y, s=10.0):
    """a vote whose 8 corners span the square [x, x + s] x [y, y + s]"""
    c = [(x, y), (x + s, y), (x, y + s), (x + s, y + s)]
    return np.array(c + c, np.float32).reshape(16)


def run(votes, scores, **kw):
    """one image, one class, every vote listed -> the six outputs of the cell"""
    votes = np.stack(votes)[None].astype(np.float32)
    scores = np.asarray(scores, np.float32).reshape(1, -1, 1)
    k = votes.shape[1]
    idx = np.arange(k, dtype=np.int32).reshape(1, 1, k)
    out = CN.vote_cluster(votes, scores, idx, np.array([[k]], np.int32), **kw)
    return [o[0, 0] for o in out]


def test_iou_by_hand():
    a = [0, 0, 10, 10]
    # shifted by 2 in x: inter 80, union 120; by 5: 50 / 150; disjoint; identical; degenerate (zero area twice)
    got = CN.iou(a, [[2, 0, 12, 10], [5, 0, 15, 10], [20, 0, 30, 10], [0, 0, 10, 10]])
    assert np.array_equal(got, np.array([80.0 / 120.0, 50.0 / 150.0, 0.0, 1.0]))
    assert CN.iou([1, 1, 1, 1], [[1, 1, 1, 1]])[0] == 0.0
    box, valid = CN.vote_boxes(np.stack([sq(3, 4), sq(0, 0)]))
    assert box.dtype == np.float32 and np.array_equal(box, [[3, 4, 13, 14], [0, 0, 10, 10]]) and valid.all()


def test_two_clusters_and_the_tie_rule():
    # votes 0, 1, 2 overlap (IoU 2/3 with their neighbour), votes 3, 4 sit apart; votes 1 and 3 share the best score: vote 1
    # (the lower anchor) leads first.  IoU(1, 0) = IoU(1, 2) = 2/3 > 0.5 -> {0, 1, 2}; then 3 leads {3, 4}
    votes = [sq(0, 0), sq(2, 0), sq(4, 0), sq(50, 0), sq(52, 0)]
    inst, order, offs, n_inst, leader, box = run(votes, [0.7, 0.9, 0.6, 0.9, 0.8], iou_thr=0.5, min_votes=2, max_instances=3)
    assert inst.tolist() == [0, 0, 0, 1, 1] and n_inst == 2
    assert order.tolist() == [0, 1, 2, 3, 4] and offs.tolist() == [0, 3, 5, 5]
    assert leader.tolist() == [1, 3, -1]
    assert np.array_equal(box, np.array([[2, 0, 12, 10], [50, 0, 60, 10], [0, 0, 0, 0]], np.float32))
    # led by vote 0 instead, vote 2 (IoU(0, 2) = 60 / 140 < 0.5) stays out and forms the third cluster alone
    inst, order, offs, n_inst, leader, _ = run(votes, [0.95, 0.9, 0.6, 0.9, 0.8], iou_thr=0.5, min_votes=1, max_instances=3)
    assert inst.tolist() == [0, 0, 2, 1, 1] and order.tolist() == [0, 1, 3, 4, 2] and offs.tolist() == [0, 2, 4, 5]
    assert leader.tolist() == [0, 3, 2]


def test_a_dropped_cluster_consumes_its_votes():
    # vote 4 has the best score and only vote 3 near it: a cluster of 2 < min_votes = 3 is dropped and both stay
    # consumed (vote 3 never leads a round of its own); the next leader (vote 1) keeps {0, 1, 2} as instance 0
    votes = [sq(0, 0), sq(2, 0), sq(4, 0), sq(50, 0), sq(52, 0)]
    inst, order, offs, n_inst, leader, _ = run(votes, [0.7, 0.8, 0.6, 0.75, 0.9], iou_thr=0.5, min_votes=3, max_instances=2)
    assert inst.tolist() == [0, 0, 0, -1, -1] and n_inst == 1
    assert order.tolist() == [0, 1, 2, -1, -1] and offs.tolist() == [0, 3, 3] and leader.tolist() == [1, -1]


def test_max_instances_and_max_rounds_stop():
    votes = [sq(0, 0), sq(1, 0), sq(40, 0), sq(41, 0), sq(80, 0), sq(81, 0)]
    scores = [0.9, 0.8, 0.7, 0.6, 0.95, 0.5]
    inst, order, offs, n_inst, leader, _ = run(votes, scores, iou_thr=0.5, min_votes=2, max_instances=2)
    assert inst.tolist() == [1, 1, -1, -1, 0, 0] and n_inst == 2 and leader.tolist() == [4, 0]
    assert order.tolist() == [4, 5, 0, 1, -1, -1] and offs.tolist() == [0, 2, 4]
    # one leader only: the best cluster, everything else unassigned -> -1
    inst, _, offs, n_inst, _, _ = run(votes, scores, iou_thr=0.5, min_votes=2, max_instances=3, max_rounds=1)
    assert inst.tolist() == [-1, -1, -1, -1, 0, 0] and n_inst == 1 and offs.tolist() == [0, 2, 2, 2]
    # rounds are counted in leaders, kept or not: with min_votes = 3 both rounds drop their cluster
    inst, _, _, n_inst, _, _ = run(votes, scores, iou_thr=0.5, min_votes=3, max_instances=3, max_rounds=2)
    assert inst.tolist() == [-1] * 6 and n_inst == 0


def test_an_invalid_vote_never_leads_and_never_joins():
    bad = sq(0, 0)
    bad[3] = np.inf
    votes = [sq(0, 0), bad, sq(1, 0), sq(2, 0)]
    inst, order, offs, n_inst, leader, _ = run(votes, [0.6, 0.99, 0.7, 0.8], iou_thr=0.5, min_votes=2, max_instances=2)
    assert inst.tolist() == [0, -1, 0, 0] and order.tolist() == [0, 2, 3, -1] and leader.tolist() == [3, -1] and n_inst == 1
    bad[3] = np.nan
    assert run([bad, bad], [0.9, 0.9], min_votes=1)[0].tolist() == [-1, -1]


def test_scenes_of_the_gpu_tests_cluster_as_expected():
    """the instance counts the GPU tests assert, settled here with the restatement alone"""
    b3, sc, want = CN.mixed_scene()
    for cap in (None, 128):
        idx, cnt = CN.threshold_compact(sc, 0.5, cap)
        assert cnt.tolist() == [[65, 50, 22], [0, 6, 42]]
        inst, order, offs, n_inst, leader, box = CN.vote_cluster(b3, sc, idx, cnt, 0.5, 10, 2)
        assert np.array_equal(n_inst, want)
        assert offs[0, 0].tolist() in ([0, 40, 65], [0, 25, 65]) and offs[0, 1].tolist() in ([0, 30, 50], [0, 20, 50])
        assert offs[0, 2].tolist() == [0, 21, 21] and (inst[0, 2, :22] == -1).sum() == 1      # the NaN vote
        assert 0.2 < CN.iou(box[0, 1, 0], box[0, 1, 1:2])[0] < 0.4
        # the tie rule is in play: the best score of cell (0, 0) is shared, and the leader is the lowest anchor that has it
        s = sc[0, idx[0, 0, :65], 0]
        assert (s == s.max()).sum() > 1 and leader[0, 0, 0] == idx[0, 0, :65][np.argmax(s)]
        assert sorted(np.diff(offs[1, 2]).tolist()) in ([13, 14], [13, 15], [14, 15])
    b3, sc, sizes = CN.large_scene()
    idx, cnt = CN.threshold_compact(sc)
    assert cnt[0, 0] == 2500
    offs = CN.vote_cluster(b3, sc, idx, cnt, 0.5, 10, 8)[2][0, 0]
    assert sorted(np.diff(offs[:4]).tolist()) == sorted(sizes) and offs[3] == offs[-1] == 2500
    b3, sc, truth = CN.two_instance_scene()
    idx, cnt = CN.threshold_compact(sc)
    assert cnt.tolist() == [[80, 40]]
    inst, order, offs, n_inst, _, _ = CN.vote_cluster(b3, sc, idx, cnt, 0.5, 10, 8)
    assert n_inst.tolist() == [[2, 1]]
    for cls, _R, _t, anchors, clean in truth:  # every cluster: all clean votes of one pose and nothing of another
        sets = [set(order[0, cls, offs[0, cls, k]:offs[0, cls, k + 1]].tolist()) for k in range(n_inst[0, cls])]
        assert sum(set(anchors[clean].tolist()) <= s <= set(anchors.tolist()) for s in sets) == 1
    b3, sc = CN.single_instance_scene()
    idx, cnt = CN.threshold_compact(sc)
    inst, order, offs, n_inst, _, _ = CN.vote_cluster(b3, sc, idx, cnt, 0.5, 10, 8)
    assert (cnt == 30).all() and (n_inst == 1).all() and (offs[:, :, 1] == 30).all()
    assert np.array_equal(order[:, :, :30], idx[:, :, :30])


def test_match_instances():
    from pyrapose_amd.utils.eval_pose import match_instances
    gt = np.array([[0.0, 0, 1], [1.0, 0, 1]])
    # crossing: detection 0 is annotation 1 and the reverse
    assert match_instances([[1.0, 0, 1.02], [0.0, 0, 1.01]], gt) == [(1, 0), (0, 1)]
    # greedy by ascending error: (1, 0) at 0.1 goes first, detection 0 takes what is left although annotation 0 is nearer
    assert match_instances([[0.2, 0, 1], [0.1, 0, 1]], gt) == [(1, 0), (0, 1)]
    # more detections than annotations, and the reverse: each side once
    assert match_instances([[0.5, 0, 1], [0.0, 0, 1.1], [1.0, 0.05, 1]], gt) == [(2, 1), (1, 0)]
    assert match_instances([[1.0, 0, 1.2]], gt) == [(0, 1)]
    # ties: (detection, annotation) index order
    assert match_instances([[0.5, 0, 1], [0.5, 0, 1]], gt) == [(0, 0), (1, 1)]
    assert match_instances(np.zeros((0, 3)), gt) == [] and match_instances(gt, []) == [] and match_instances([], []) == []
