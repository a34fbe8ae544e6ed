"""GPU: the detection-metric entry points (pp_det_match, pp_det_pr_curve, pp_det_ap; csrc/det_eval.hip) against the numpy
restatement tests/det_eval_np.py.  Every comparison of match, det_ignored, npos, tp, fp, recall, prec_env and ap is bit for bit:
the restatement runs the same rules and the sums in the kernel's documented order.  Shapes are the smallest at which each
mechanism can go wrong (wave width 64, scan chunk 256, the limits 1024).  End to end: utils.eval.evaluate_detections / evaluate
and callbacks.Evaluate against the reference's own numbers in tests/golden/detection_ap.npz."""
import ctypes
import os

import numpy as np
import pytest

import det_eval_np as DN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(bits(got), bits(want)), what


def gpu_match(case, thresholds, rule):
    from pyrapose_amd import ops
    ig = case.get("gt_ignore")
    return ops.det_match(ctx(), dev(case["det_boxes"], np.float64), dev(case["det_scores"], np.float64), dev(case["det_labels"], np.int32),
                         dev(case["gt_boxes"].reshape(-1, 4), np.float64), dev(case["gt_labels"], np.int32),
                         dev(case["gt_offsets"], np.int32), case["n_class"], thresholds, rule=rule,
                         gt_ignore=None if ig is None else dev(ig, np.uint8))


def gpu_chain(case, thresholds, rule, integration):
    from pyrapose_amd import ops
    match, ign, npos = gpu_match(case, thresholds, rule)
    order, offs = ops.det_order(dev(case["det_scores"], np.float64), dev(case["det_labels"], np.int32), case["n_class"])
    tp, fp, recall, env = ops.det_pr_curve(ctx(), order, offs, match, ign, npos)
    ap, rf = ops.det_ap(ctx(), offs, npos, recall, env, integration)
    return dict(match=match, det_ignored=ign, npos=npos, order=order, class_offsets=offs, tp=tp, fp=fp, recall=recall, prec_env=env, ap=ap,
                recall_final=rf)


def check_chain(case, thresholds, rule, integration):
    want = DN.evaluate(case["det_boxes"], case["det_scores"], case["det_labels"], case["gt_boxes"], case["gt_labels"], case["gt_offsets"],
                       case["n_class"], list(thresholds), rule, integration, case.get("gt_ignore"))
    got = gpu_chain(case, thresholds, rule, integration)
    for k in ("match", "det_ignored", "npos", "order", "class_offsets", "tp", "fp", "recall", "prec_env", "ap", "recall_final"):
        same_bits(got[k], want[k], (k, rule, integration))
    return got, want


def random_case(seed, D, n_valid, n_gt, n_class=3, ignore=False, n_scores=40):
    """B = len(n_gt) images of D slots; n_valid[b] of them hold a detection, at random slots (padding -1 anywhere); integer
    boxes on a coarse grid and scores from a small set, so equal IoUs and equal scores are common"""
    rng = np.random.default_rng(seed)
    B = len(n_gt)
    det_boxes = np.zeros((B, D, 4))
    det_scores = np.zeros((B, D))
    det_labels = np.full((B, D), -1, np.int32)
    gt_boxes, gt_labels = [], []
    for b in range(B):
        xy = rng.integers(0, 12, size=(n_gt[b], 2)) * 8.0
        g = np.concatenate([xy, xy + rng.integers(1, 5, size=(n_gt[b], 2)) * 8.0], axis=1)
        gt_boxes.append(g)
        gt_labels.append(rng.integers(0, n_class, size=n_gt[b]).astype(np.int32))
        slots = np.sort(rng.permutation(D)[:n_valid[b]])
        for d in slots:
            if n_gt[b] and rng.uniform() < 0.7:
                j = rng.integers(0, n_gt[b])
                det_boxes[b, d] = g[j] + rng.integers(-1, 2, size=4) * 4.0
                det_labels[b, d] = gt_labels[-1][j] if rng.uniform() < 0.8 else rng.integers(0, n_class)
            else:
                p = rng.integers(0, 12, size=2) * 8.0
                det_boxes[b, d] = np.concatenate([p, p + rng.integers(1, 5, size=2) * 8.0])
                det_labels[b, d] = rng.integers(0, n_class)
            det_scores[b, d] = rng.integers(1, n_scores + 1) / float(n_scores)
    offs = np.zeros(B + 1, np.int32)
    offs[1:] = np.cumsum(n_gt)
    case = dict(det_boxes=det_boxes, det_scores=det_scores, det_labels=det_labels, gt_boxes=np.concatenate(gt_boxes).reshape(-1, 4),
                gt_labels=np.concatenate(gt_labels), gt_offsets=offs, n_class=n_class)
    if ignore:
        case["gt_ignore"] = (rng.uniform(size=int(offs[-1])) < 0.3).astype(np.uint8)
    return case


RULES = [("reference", "area", False), ("coco", "101", True), ("coco", "area", False)]


@pytest.mark.parametrize("rule, integration, ignore", RULES)
def test_detections_per_image_at_the_wave_edges(rule, integration, ignore):
    # 0, 1, 63, 64, 65 detections in rows of 65 slots (so the shorter rows have padding in their middle), 7 ground truths each
    case = random_case(1, 65, [0, 1, 63, 64, 65], [7, 7, 7, 7, 7], ignore=ignore)
    assert (case["det_labels"][2, :40] == -1).any() and (case["det_labels"][2, 40:] >= 0).any()
    check_chain(case, [0.3, 0.5], rule, integration)


@pytest.mark.parametrize("rule, integration, ignore", RULES)
def test_ground_truth_per_image_at_the_wave_edges(rule, integration, ignore):
    case = random_case(2, 48, [48, 48, 48, 48, 30], [0, 1, 64, 65, 130], ignore=ignore)
    check_chain(case, [0.25, 0.5, 0.75], rule, integration)


@pytest.mark.parametrize("rule, ignore", [("reference", False), ("coco", True)])
def test_the_limits(rule, ignore):
    from pyrapose_amd import ops
    case = random_case(3, ops.DET_MAX_DET, [ops.DET_MAX_DET, 5], [ops.DET_MAX_GT, 3], n_class=4, ignore=ignore, n_scores=300)
    want = DN.det_match(case["det_boxes"], case["det_scores"], case["det_labels"], case["gt_boxes"], case["gt_labels"], case["gt_offsets"],
                        4, [0.5], rule, case.get("gt_ignore"))
    got = gpu_match(case, [0.5], rule)
    for g, w, k in zip(got, want, ("match", "det_ignored", "npos")):
        same_bits(g, w, (k, rule))
    assert (want[0] >= 0).sum() > 100


def test_class_in_detections_only_and_in_ground_truth_only():
    case = random_case(4, 20, [20, 20], [6, 6], n_class=2)
    case["n_class"] = 4
    case["det_labels"][case["det_labels"] == 1] = 2   # class 2: detections, no ground truth
    case["gt_labels"][case["gt_labels"] == 1] = 3     # class 3: ground truth, no detections
    for rule, integration in (("reference", "area"), ("coco", "101")):
        got, want = check_chain(case, [0.5], rule, integration)
        assert want["npos"][2] == 0 and want["npos"][3] > 0 and want["class_offsets"][3] == want["class_offsets"][4]
        assert want["ap"][0, 2] == (0.0 if integration == "area" else -1.0) and want["ap"][0, 3] == 0.0


@pytest.mark.parametrize("rule, ignore", [("reference", False), ("coco", True)])
def test_sixteen_thresholds_equal_sixteen_launches(rule, ignore):
    case = random_case(5, 70, [70, 33, 0, 64], [9, 70, 4, 0], ignore=ignore)
    thr = np.linspace(0.2, 0.95, 16)
    m16, i16, n16 = gpu_match(case, thr, rule)
    want = DN.det_match(case["det_boxes"], case["det_scores"], case["det_labels"], case["gt_boxes"], case["gt_labels"], case["gt_offsets"],
                        3, list(thr), rule, case.get("gt_ignore"))
    same_bits(m16, want[0], "match")
    same_bits(i16, want[1], "det_ignored")
    assert len(set(m16[t].cpu().numpy().tobytes() for t in range(16))) > 4  # the thresholds do differ in outcome
    for t in range(16):
        m1, i1, n1 = gpu_match(case, [thr[t]], rule)
        same_bits(m1[0], m16[t].cpu().numpy(), ("match", t))
        same_bits(i1[0], i16[t].cpu().numpy(), ("det_ignored", t))
        same_bits(n1, n16.cpu().numpy(), "npos")


def tiny(det, gt, n_class=1, gt_ignore=None):
    """one image: det = [(box, score, label)], gt = [(box, label)]"""
    case = dict(det_boxes=np.array([[d[0] for d in det]], np.float64).reshape(1, len(det), 4),
                det_scores=np.array([[d[1] for d in det]], np.float64), det_labels=np.array([[d[2] for d in det]], np.int32),
                gt_boxes=np.array([g[0] for g in gt], np.float64).reshape(-1, 4), gt_labels=np.array([g[1] for g in gt], np.int32),
                gt_offsets=np.array([0, len(gt)], np.int32), n_class=n_class)
    if gt_ignore is not None:
        case["gt_ignore"] = np.array(gt_ignore, np.uint8)
    return case


def test_ties():
    box = [10, 10, 50, 50]
    case = tiny([(box, 0.9, 0)], [(box, 0), (box, 0)])
    assert gpu_match(case, [0.5], "reference")[0].cpu().numpy().ravel().tolist() == [0]  # np.argmax: the first maximum
    assert gpu_match(case, [0.5], "coco")[0].cpu().numpy().ravel().tolist() == [1]       # pycocotools: the later one
    # equal scores: the lower slot goes first and takes the only ground truth
    case = tiny([([10, 10, 50, 52], 0.7, 0), (box, 0.7, 0), (box, 0.2, 0)], [(box, 0)])
    for rule in ("reference", "coco"):
        assert gpu_match(case, [0.5], rule)[0].cpu().numpy().ravel().tolist() == [0, -1, -1]
        check_chain(case, [0.5], rule, "area")


def test_iou_exactly_at_the_threshold():
    case = tiny([([0, 0, 9, 9], 0.9, 0)], [([0, 0, 9, 19], 0)])      # "+1": 100 / 200
    assert DN.iou_plus1(case["det_boxes"][0, 0], case["gt_boxes"])[0] == 0.5
    assert gpu_match(case, [0.5], "reference")[0].cpu().numpy().ravel().tolist() == [0]
    case = tiny([([0, 0, 10, 10], 0.9, 0)], [([0, 0, 10, 20], 0)])   # plain: 100 / 200
    assert DN.iou_plain(case["det_boxes"][0, 0], case["gt_boxes"])[0] == 0.5
    assert gpu_match(case, [0.5], "coco")[0].cpu().numpy().ravel().tolist() == [0]
    m = gpu_match(case, [0.5, 0.5000000000000001], "coco")[0].cpu().numpy()
    assert m[:, 0, 0].tolist() == [0, -1]


def test_the_case_that_separates_the_rules():
    A, Bx = [0, 0, 100, 100], [0, 65, 100, 165]
    case = tiny([(A, 0.9, 0), ([0, 30, 100, 130], 0.8, 0)], [(A, 0), (Bx, 0)])
    for f in (DN.iou_plus1, DN.iou_plain):  # the second detection's best ground truth is A, its second best is above 0.4
        v = f(case["det_boxes"][0, 1], case["gt_boxes"])
        assert v[0] > v[1] > 0.4
    assert gpu_match(case, [0.4], "reference")[0].cpu().numpy().ravel().tolist() == [0, -1]  # no second choice: false positive
    assert gpu_match(case, [0.4], "coco")[0].cpu().numpy().ravel().tolist() == [0, 1]
    check_chain(case, [0.4], "reference", "area")
    check_chain(case, [0.4], "coco", "101")


def test_ignored_ground_truth():
    from pyrapose_amd import _lib, ops
    A, Bx = [0, 0, 100, 100], [200, 0, 300, 100]
    # detection 0 reaches only the ignored B; detection 1 overlaps A (not ignored, lower IoU) and the ignored A2 (IoU 1)
    A2 = [0, 0, 100, 90]
    case = tiny([(Bx, 0.9, 0), (A2, 0.8, 0), ([500, 500, 600, 600], 0.7, 0)], [(A, 0), (A2, 0), (Bx, 0)], gt_ignore=[0, 1, 1])
    got, want = check_chain(case, [0.5], "coco", "101")
    assert want["match"].ravel().tolist() == [2, 0, -1] and want["det_ignored"].ravel().tolist() == [1, 0, 0]
    assert want["npos"].tolist() == [1]
    # the ignored detection counts nowhere: tp / fp in score order are (0,0), (1,0), (1,1)
    assert want["tp"].ravel().tolist() == [0, 1, 1] and want["fp"].ravel().tolist() == [0, 0, 1]
    with pytest.raises(ValueError):
        gpu_match(case, [0.5], "reference")
    # and the C ABI itself: PP_ERR_ARG, a host check
    d = {k: dev(case[k], t) for k, t in (("det_boxes", np.float64), ("det_scores", np.float64), ("det_labels", np.int32),
                                         ("gt_boxes", np.float64), ("gt_labels", np.int32), ("gt_ignore", np.uint8), ("gt_offsets", np.int32))}
    import torch
    out = [torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.uint8, device="cuda"),
           torch.zeros(1, dtype=torch.int32, device="cuda")]
    thr = (ctypes.c_double * 1)(0.5)
    host = (ctypes.c_int * 2)(0, 3)
    p = ops._ptr
    rc = _lib.lib.pp_det_match(ctx().handle, 1, 3, 3, 1, p(d["det_boxes"]), p(d["det_scores"]), p(d["det_labels"]), p(d["gt_boxes"]),
                               p(d["gt_labels"]), p(d["gt_ignore"]), host, p(d["gt_offsets"]), 1, thr, ops.DET_RULES["reference"],
                               p(out[0]), p(out[1]), p(out[2]))
    assert rc == -1


@pytest.mark.parametrize("rule, ignore", [("reference", False), ("coco", True)])
def test_batch_independence(rule, ignore):
    case = random_case(6, 66, [40, 66, 10, 50, 66], [5, 66, 0, 20, 3], ignore=ignore)
    thr = [0.3, 0.5, 0.7]
    m5, i5, _ = gpu_match(case, thr, rule)
    lo, hi = case["gt_offsets"][3], case["gt_offsets"][4]
    alone = dict(det_boxes=case["det_boxes"][3:4], det_scores=case["det_scores"][3:4], det_labels=case["det_labels"][3:4],
                 gt_boxes=case["gt_boxes"][lo:hi], gt_labels=case["gt_labels"][lo:hi], gt_offsets=np.array([0, hi - lo], np.int32), n_class=3)
    if ignore:
        alone["gt_ignore"] = case["gt_ignore"][lo:hi]
    m1, i1, _ = gpu_match(alone, thr, rule)
    m5 = m5.cpu().numpy()[:, 3]
    same_bits(m1[:, 0], np.where(m5 >= 0, m5 - lo, -1).astype(np.int32), "match")  # (global indices shift with the batch)
    same_bits(i1[:, 0], i5.cpu().numpy()[:, 3], "det_ignored")
    assert (m5 >= 0).any()


@pytest.mark.parametrize("integration", ["area", "101"])
def test_curves_at_the_scan_chunk_edges(integration):
    from pyrapose_amd import ops
    chunk = ops.DET_SCAN_CHUNK
    # segment lengths 0, 1, one chunk, one chunk + 1, three chunks + 7; then a class whose detections are all ignored and a
    # class without ground truth
    lengths = [0, 1, chunk, chunk + 1, 3 * chunk + 7, 40, 30]
    rng = np.random.default_rng(7)
    N, T, C = sum(lengths), 2, len(lengths)
    offs = np.zeros(C + 1, np.int32)
    offs[1:] = np.cumsum(lengths)
    order = np.concatenate([offs[c] + rng.permutation(lengths[c]) for c in range(C)]).astype(np.int32)  # any slots: a permutation
    match = np.where(rng.uniform(size=(T, 1, N)) < 0.4, rng.integers(0, 1000, size=(T, 1, N)), -1).astype(np.int32)
    ign = (rng.uniform(size=(T, 1, N)) < 0.15).astype(np.uint8)
    ign[:, 0, offs[5]:offs[6]] = 1
    npos = np.array([3, 2, 200, 150, 500, 9, 0], np.int32)
    want_curves = DN.pr_curve(order, offs, match, ign, npos)
    want_ap = DN.det_ap(offs, npos, want_curves[2], want_curves[3], integration)
    o, f, m, i, n = dev(order, np.int32), dev(offs, np.int32), dev(match, np.int32), dev(ign, np.uint8), dev(npos, np.int32)
    got = ops.det_pr_curve(ctx(), o, f, m, i, n)
    for g, w, k in zip(got, want_curves, ("tp", "fp", "recall", "prec_env")):
        same_bits(g, w, k)
    ap, rf = ops.det_ap(ctx(), f, n, got[2], got[3], integration)
    same_bits(ap, want_ap[0], "ap")
    same_bits(rf, want_ap[1], "recall_final")
    none = 0.0 if integration == "area" else -1.0
    assert (want_ap[0][:, 6] == none).all() and (want_ap[0][:, 5] == 0.0).all() and (want_ap[0][:, 0] == 0.0).all()
    assert (want_curves[0][:, offs[5]:offs[6]] == 0).all() and (want_ap[0][:, 4] > 0).all()
    # the envelope does rise somewhere across a chunk border, and the ordered sum differs from numpy's pairwise one somewhere
    prec = want_curves[0] / np.maximum(want_curves[0] + want_curves[1], DN.EPS)
    assert (want_curves[3][:, offs[4]:offs[5]] > prec[:, offs[4]:offs[5]]).any()


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "detection_ap.npz"))


def test_evaluate_detections_reproduces_the_reference(fixture):
    from pyrapose_amd.utils.eval import evaluate_detections
    z = fixture
    C = len(z["has_label"])
    res = evaluate_detections((z["det_boxes"], z["det_scores"], z["det_labels"]), (z["gt_boxes"], z["gt_labels"], z["gt_offsets"]),
                              rule="reference", iou_thresholds=[float(z["iou_threshold"])], num_classes=C)
    assert res["ap"].shape == (1, C)
    for l, ap_ref, num_ref in zip(z["labels"], z["ap"], z["num_annotations"]):
        n = int((z["det_labels"] == l).sum())
        assert float(res["npos"][l]) == num_ref
        assert abs(res["ap"][0, l] - ap_ref) <= n * 2.0 ** -52  # the bound derived in test_det_eval_cpu.py
    # the COCO side of the same inputs, against the restatement (pycocotools itself is unpinned)
    ig = (np.arange(len(z["gt_labels"])) % 5 == 0).astype(np.uint8)
    res = evaluate_detections((z["det_boxes"], z["det_scores"], z["det_labels"]), (z["gt_boxes"], z["gt_labels"], z["gt_offsets"]),
                              ignore=ig, num_classes=C)
    want = DN.evaluate(z["det_boxes"], z["det_scores"], z["det_labels"], z["gt_boxes"], z["gt_labels"], z["gt_offsets"], C,
                       list(np.linspace(0.5, 0.95, 10)), "coco", "101", ig)
    same_bits(res["ap"], want["ap"], "ap")
    same_bits(res["npos"], want["npos"], "npos")
    have = want["npos"] > 0
    assert res["AP"] == float(want["ap"][:, have].mean()) and res["AP50"] == float(want["ap"][0, have].mean())
    assert res["AP75"] == float(want["ap"][5, have].mean())


def test_evaluate_and_callback_on_the_fixture(fixture):
    from pyrapose_amd import callbacks
    from pyrapose_amd.utils.eval import evaluate
    z = fixture
    gen = DN.FakeGenerator(z["gt_boxes"], z["gt_labels"], z["gt_offsets"], z["has_label"], float(z["scale"]))
    model = DN.FakeModel(z["raw_boxes"], z["raw_scores"], z["raw_labels"])
    kw = dict(iou_threshold=float(z["iou_threshold"]), score_threshold=float(z["score_threshold"]), max_detections=int(z["max_detections"]))
    res = evaluate(gen, model, **kw)
    assert sorted(res) == [int(l) for l in z["labels"]]
    for l, ap_ref, num_ref in zip(z["labels"], z["ap"], z["num_annotations"]):
        n = int((z["det_labels"] == l).sum())
        assert res[int(l)][1] == num_ref and abs(res[int(l)][0] - ap_ref) <= n * 2.0 ** -52
    cb = callbacks.Evaluate(gen, verbose=0, **kw)
    cb.set_model(model)
    logs = {}
    cb.on_epoch_end(0, logs)
    n_all = int((z["det_labels"] >= 0).sum())  # every class within its n 2^-52, the mean of them within their sum
    assert abs(logs["mAP"] - z["ap"].sum() / (z["num_annotations"] > 0).sum()) <= n_all * 2.0 ** -52 and cb.mean_ap == logs["mAP"]


def test_argument_errors_are_host_checks():
    import torch
    from pyrapose_amd import ops
    case = random_case(8, 8, [8, 8], [3, 3])

    def bad(thr=(0.5,), **change):
        c = dict(case, **change)
        with pytest.raises(ValueError):
            gpu_match(c, list(thr), "reference")

    bad(thr=())
    bad(thr=np.linspace(0.1, 0.9, 17))
    bad(thr=(0.5, 0.5))
    bad(thr=(0.6, 0.5))
    lab = case["det_labels"].copy()
    lab[0, 0] = 3
    bad(det_labels=lab)
    bad(gt_labels=np.array([0, 1, 3, 0, 1, 2], np.int32))
    bad(gt_offsets=np.array([0, 4, 3], np.int32))   # not monotone
    bad(gt_offsets=np.array([0, 3, 5], np.int32))   # does not end at G
    D = ops.DET_MAX_DET + 1
    bad(det_boxes=np.zeros((2, D, 4)), det_scores=np.zeros((2, D)), det_labels=np.full((2, D), -1, np.int32))
    G = ops.DET_MAX_GT + 1
    bad(gt_boxes=np.zeros((G + 1, 4)), gt_labels=np.zeros(G + 1, np.int32), gt_offsets=np.array([0, G, G + 1], np.int32))
    with pytest.raises(ValueError):
        gpu_match(case, [0.5], "voc")
    # the curve entry points: offsets that do not rise, an unknown integration
    m, i, n = gpu_match(case, [0.5], "reference")
    order, offs = ops.det_order(dev(case["det_scores"], np.float64), dev(case["det_labels"], np.int32), 3)
    wrong = offs.clone()
    wrong[1], wrong[2] = offs[2] + 1, offs[1]
    with pytest.raises(ValueError):
        ops.det_pr_curve(ctx(), order, wrong, m, i, n)
    tp, fp, rec, env = ops.det_pr_curve(ctx(), order, offs, m, i, n)
    with pytest.raises(ValueError):
        ops.det_ap(ctx(), wrong, n, rec, env)
    with pytest.raises(ValueError):
        ops.det_ap(ctx(), offs, n, rec, env, integration="11")
    with pytest.raises(ValueError):
        ops.det_pr_curve(ctx(), order, offs, m.to(torch.int64), i, n)
