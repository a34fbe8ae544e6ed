"""GPU: filter_sort_kernel / filter_nms_kernel / filter_topk_kernel (csrc/detect.hip) against oracle/detect_np.py, which
tests/test_oracle_detect.py pins to hand tables.  Bar: all four outputs bit-equal -- the IoU is op-by-op float32 on both
sides (-ffp-contract=off), everything else is ordering.

The kernels are called through the C ABI with a ZEROED workspace: a key of 0 is the best possible key (highest score, anchor 0),
so a sort that read workspace it had not written (a missing sentinel) would put it first instead of getting lucky with what
the allocator last held there.

Most cases are built from pairwise disjoint boxes (a grid of 8 x 8 boxes on a 10-px pitch), where NMS keeps every candidate and
the survivor count is known by hand; a "shadow" of a grid box is the same box moved by 1 px (intersection 8 x 7 = 56, union
128 - 56 = 72, IoU 0.78): it overlaps its own cell's box only."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = np.float32
TOPK_STATIC_LDS = 264      # .group_segment_fixed_size of filter_topk_kernel in the gfx950 code object (s_off[65], padded)


@pytest.fixture(scope="module")
def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


def grid_boxes(n, cols=20, pitch=10, side=8):
    i = np.arange(n)
    y0, x0 = (i // cols) * pitch, (i % cols) * pitch
    return np.stack([y0, x0, y0 + side, x0 + side], axis=1).astype(F)


def shadows(boxes):
    return boxes + F([0, 1, 0, 1])


def boxes3d_of(boxes, seed=0):
    """distinct rows, so that a wrong gather cannot hide"""
    return np.random.default_rng(seed).uniform(0, 640, size=(len(boxes), 16)).astype(F)


def run_batch(ctx, boxes, boxes3d, scores, score_thr, iou_thr, max_det):
    """[B,N,4], [B,N,16], [B,N,C] numpy -> four numpy outputs through pp_filter_detections_batch (pp_filter_detections when the
    arrays carry no batch axis), workspace zeroed"""
    from pyrapose_amd._lib import check, lib
    single = scores.ndim == 2
    Bn = 1 if single else scores.shape[0]
    N, Cc = scores.shape[-2:]
    d = [torch.from_numpy(np.ascontiguousarray(a, F)).cuda() for a in (boxes, boxes3d, scores)]
    ws = torch.zeros((Bn * lib.pp_filter_workspace_bytes(N, Cc, max_det) + 8,), dtype=torch.uint8, device="cuda")
    lead = () if single else (Bn,)
    out = [torch.empty(lead + (max_det,) + tail, dtype=dt, device="cuda")
           for tail, dt in (((4,), torch.float32), ((16,), torch.float32), ((), torch.float32), ((), torch.int32))]
    p = [C.c_void_p(t.data_ptr()) for t in d + [ws] + out]
    if single:
        rc = lib.pp_filter_detections(ctx.handle, N, Cc, p[0], p[1], p[2], score_thr, iou_thr, max_det, *p[3:])
    else:
        rc = lib.pp_filter_detections_batch(ctx.handle, Bn, N, Cc, p[0], p[1], p[2], score_thr, iou_thr, max_det, *p[3:])
    check(rc, ctx.handle, "pp_filter_detections")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def same_bits(got, want):
    return all(g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def check_vs_oracle(ctx, boxes, boxes3d, scores, score_thr, iou_thr, max_det):
    from oracle import detect_np as D
    got = run_batch(ctx, boxes, boxes3d, scores, score_thr, iou_thr, max_det)
    want = D.filter_detections(boxes, boxes3d, scores, score_thr, max_det, iou_thr)
    assert same_bits(got, want), [int((g != w).sum()) for g, w in zip(got, want)]
    return got


@pytest.mark.parametrize("n_boxes", [255, 256, 257, 320])
def test_survivor_counts_around_the_workgroup_width(ctx, n_boxes):
    """filter_nms_kernel compares a candidate with the kept boxes 256 at a time: one class, more than 256 survivors"""
    rng = np.random.default_rng(n_boxes)
    boxes = grid_boxes(n_boxes)
    order = rng.permutation(n_boxes)                     # order[r] = the anchor with the r-th highest score
    sc = np.empty((n_boxes, 1), F)
    sc[order, 0] = F(0.9) - F(0.001) * np.arange(n_boxes, dtype=F)   # strictly decreasing: steps of 0.001 near 0.9, ulp 6e-8
    assert np.all(np.diff(sc[order, 0]) < 0)
    b3 = boxes3d_of(boxes)
    keep = min(n_boxes, 300)
    ob, o3, osc, ol = check_vs_oracle(ctx, boxes, b3, sc, 0.05, 0.5, 300)
    assert np.array_equal(ob[:keep], boxes[order[:keep]]) and np.array_equal(o3[:keep], b3[order[:keep]])   # by hand: all survive
    assert np.all(ol[:keep] == 0) and np.all(ol[keep:] == -1) and np.all(osc[keep:] == -1)
    # one shadow per cell, scored just below its own box and above the next one: visited right after its suppressor, which
    # sits at kept index r -- for r >= 256 only the second trip of the compare loop sees it
    boxes2 = np.concatenate([boxes, shadows(boxes)])
    sc2 = np.concatenate([sc, sc - F(0.0005)])
    s = np.sort(np.concatenate([sc[:, 0], sc2[n_boxes:, 0]]))
    assert np.all(np.diff(s) > 0)
    b3 = boxes3d_of(boxes2)
    ob, o3, osc, ol = check_vs_oracle(ctx, boxes2, b3, sc2, 0.05, 0.5, 300)
    assert np.array_equal(ob[:keep], boxes[order[:keep]]) and np.array_equal(osc[:keep], sc[order[:keep], 0])   # no shadow survives
    assert np.all(ol[keep:] == -1)


def _two_class_case():
    """40 cells, a box and its shadow in each; class 0 sees all 80 anchors, class 1 the anchors of 25 cells"""
    rng = np.random.default_rng(40)
    g = grid_boxes(40)
    boxes = np.concatenate([g, shadows(g)])
    sc = rng.uniform(0.1, 1.0, size=(80, 2)).astype(F)   # either of a cell's two may win
    cells = rng.permutation(40)[:15]
    sc[cells, 1] = 0.0
    sc[cells + 40, 1] = 0.0
    return boxes, boxes3d_of(boxes), sc                  # survivors by hand: 40 in class 0, 25 in class 1


@pytest.mark.parametrize("max_det", [1, 24, 25, 26, 39, 40, 41, 64, 65, 66, 1024])
def test_max_det_edges(ctx, max_det):
    """max_det against the survivors: 40 in class 0, 25 in class 1, 65 in all -- one below, equal, one above; 1; the host's limit"""
    boxes, b3, sc = _two_class_case()
    ob, o3, osc, ol = check_vs_oracle(ctx, boxes, b3, sc, 0.05, 0.5, max_det)
    n0, n1 = min(40, max_det), min(25, max_det)
    keep = min(n0 + n1, max_det)
    assert int((ol >= 0).sum()) == keep and np.all(ol[keep:] == -1)
    assert np.all(np.diff(osc[:keep]) <= 0)
    if max_det >= 65:
        assert int((ol == 0).sum()) == 40 and int((ol == 1).sum()) == 25


def test_size_limits_of_the_host_check(ctx):
    from pyrapose_amd import ops
    rng = np.random.default_rng(3)
    N = 50
    boxes = grid_boxes(N)
    b3 = boxes3d_of(boxes)
    dev = lambda a: torch.from_numpy(a).cuda()
    for n_class, max_det in ((1, 1025), (65, 8), (16, 1024)):      # max_det, classes, classes * max_det = 16384 keys > 64 KiB
        sc = rng.uniform(0.1, 1, size=(N, n_class)).astype(F)
        with pytest.raises(ValueError):
            ops.filter_detections(ctx, dev(boxes), dev(b3), dev(sc), 0.05, 0.5, max_det)
    sc = rng.uniform(0.1, 1, size=(N, 64)).astype(F)
    ob, o3, osc, ol = check_vs_oracle(ctx, boxes, b3, sc, 0.05, 0.5, 8)   # 64 classes x 8 = 512 keys
    assert np.all(ol >= 0)
    via_ops = ops.filter_detections(ctx, dev(boxes), dev(b3), dev(sc), 0.05, 0.5, 8)
    assert same_bits([t.cpu().numpy() for t in via_ops], [ob, o3, osc, ol])


SORT_CASES = [(1, 0), (1, 1), (2, 1), (2, 2), (100, 0), (100, 1), (100, 2), (100, 63), (100, 64), (100, 65), (64, 64),
              (1000, 1000), (1024, 1023), (1024, 1024), (1025, 1), (1025, 1024), (1025, 1025)]


@pytest.mark.parametrize("n,n_cand", SORT_CASES)
def test_sort_lengths(ctx, n, n_cand):
    """candidate counts on and beside a power of two (the bitonic length and its sentinels), n a power of two with every anchor a
    candidate (no sentinel at all), n = 1, n below and just past one 1024-thread compaction pass"""
    rng = np.random.default_rng(1000 * n + n_cand)
    boxes = grid_boxes(n, cols=40)
    b3 = boxes3d_of(boxes)
    sc = rng.uniform(0.0, 0.04, size=(n, 2)).astype(F)
    for c in range(2):
        # (1025, 1): the lone candidate is the anchor that only the second pass reads
        cand = np.array([n - 1]) if (n_cand == 1 and n > 1) else rng.permutation(n)[:n_cand]
        sc[cand, c] = rng.uniform(0.06, 1.0, size=len(cand)).astype(F)
    max_det = 300
    ob, o3, osc, ol = check_vs_oracle(ctx, boxes, b3, sc, 0.05, 0.5, max_det)
    assert int((ol >= 0).sum()) == min(2 * min(n_cand, max_det), max_det)


def test_threshold_and_ties(ctx):
    thr = F(0.05)
    g = grid_boxes(16)
    boxes = np.concatenate([g, F([[200, 0, 210, 10], [200, 0, 210, 5]])])      # 16, 17: IoU exactly 0.5
    b3 = boxes3d_of(boxes)
    sc = np.zeros((18, 3), F)
    sc[0:6, 0] = 0.5                         # a run of equal scores in one class: index order
    sc[6, 0] = thr                           # equal to the threshold: out
    sc[7, 0] = np.nextafter(thr, F(1))       # one ulp above: in
    sc[8, 0] = np.nan                        # NaN > thr is false: never a candidate
    sc[9, 0] = 0.75
    sc[[3, 9, 12], 1] = [0.5, 0.75, 0.5]     # equal scores across classes: class first, then selection order
    sc[8, 1] = -np.nan
    sc[16, 2], sc[17, 2] = 0.9, 0.8          # IoU 0.5 is not > 0.5: both stay
    ob, o3, osc, ol = check_vs_oracle(ctx, boxes, b3, sc, float(thr), 0.5, 32)
    # by hand: positions class 0 -> 9, 0..5, 7; class 1 -> 9, 3, 12; class 2 -> 16, 17
    anchors = [16, 17, 9, 9, 0, 1, 2, 3, 4, 5, 3, 12, 7]
    labels = [2, 2, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0]
    assert list(ol[:13]) == labels and np.array_equal(ob[:13], boxes[anchors]) and np.all(ol[13:] == -1)
    assert osc[12] == np.nextafter(thr, F(1))
    # at iou_thr just below 0.5 the pair loses its second box
    ob, o3, osc, ol = check_vs_oracle(ctx, boxes, b3, sc, float(thr), 0.49, 32)
    assert list(ol[:2]) == [2, 0] and int((ol >= 0).sum()) == 12


def test_degenerate_boxes(ctx):
    """zero-area boxes (IoU 0 with everything: never suppress, never suppressed) and boxes with reversed corners"""
    rng = np.random.default_rng(17)
    N = 400
    ctr = rng.uniform(20, 120, size=(N, 2)); wh = rng.uniform(10, 60, size=(N, 2))
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], axis=1).astype(F)
    boxes[::5] = boxes[::5][:, [2, 3, 0, 1]]             # both corners swapped
    boxes[1::7] = boxes[1::7][:, [0, 3, 2, 1]]           # x corners swapped
    boxes[2::9, 2] = boxes[2::9, 0]                      # zero height
    boxes[3::13, 3] = boxes[3::13, 1]                    # zero width
    boxes[4::31, 2:] = boxes[4::31, :2]                  # a point
    sc = (rng.uniform(0, 1, size=(N, 3)) ** 2).astype(F)
    check_vs_oracle(ctx, boxes, boxes3d_of(boxes), sc, 0.05, 0.5, 300)


def test_all_classes_empty(ctx):
    boxes = grid_boxes(70)
    sc = np.full((70, 3), 0.05, F)                       # all equal to the threshold
    for out in run_batch(ctx, boxes, boxes3d_of(boxes), sc, 0.05, 0.5, 20):
        assert np.all(out == -1)


def test_batch_of_unequal_images_vs_oracle(ctx):
    """one pp_filter_detections_batch call over images with 0, 1 and many candidates (and a class that is empty in one image
    only); every image against the oracle"""
    from oracle import detect_np as D
    rng = np.random.default_rng(23)
    B, N, Cc = 4, 500, 3
    ctr = rng.uniform(20, 200, size=(B, N, 2)); wh = rng.uniform(10, 60, size=(B, N, 2))
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], axis=-1).astype(F)
    b3 = rng.uniform(0, 640, size=(B, N, 16)).astype(F)
    sc = (rng.uniform(0, 1, size=(B, N, Cc)) ** 3).astype(F)
    sc[0] = 0.01                                         # no candidate
    sc[1] = 0.01
    sc[1, 321, 2] = 0.5                                  # one candidate
    sc[3, :, 1] = 0.0                                    # many, class 1 empty
    got = run_batch(ctx, boxes, b3, sc, 0.05, 0.5, 100)
    for b in range(B):
        want = D.filter_detections(boxes[b], b3[b], sc[b], 0.05, 100, 0.5)
        assert same_bits([g[b] for g in got], want), b
    assert np.all(got[3][0] == -1) and int((got[3][1] >= 0).sum()) == 1 and int((got[3][2] >= 0).sum()) > 1
    assert not np.any(got[3][3] == 1)


def test_signed_zero_scores_tie(ctx):
    """-0.0f == +0.0f, so scores [-0, +0, -0, +0] above a negative threshold are four equal scores: index order.  The scores
    are compared with ==, not as bits: the kernel canonicalises the zero in its sort key and may return +0 for a -0."""
    from oracle import detect_np as D
    boxes = grid_boxes(4)
    b3 = boxes3d_of(boxes)
    sc = F([-0.0, 0.0, -0.0, 0.0]).reshape(4, 1)
    for max_det in (4, 3, 8):
        ob, o3, osc, ol = run_batch(ctx, boxes, b3, sc, -1.0, 0.5, max_det)
        wb, w3, wsc, wl = D.filter_detections(boxes, b3, sc, -1.0, max_det, 0.5)
        assert same_bits([ob, o3, ol], [wb, w3, wl])
        assert np.array_equal(osc, wsc)
        k = min(4, max_det)
        assert np.array_equal(ob[:k], boxes[:k])         # by hand: anchors 0, 1, 2, 3
    # mixed with other scores, in two classes, and through the cross-class top-k
    boxes = grid_boxes(12)
    b3 = boxes3d_of(boxes)
    sc = np.zeros((12, 2), F)
    sc[:, 0] = F([0.0, -0.0, 0.5, -0.0, 0.0, -0.25, 0.0, -0.0, 0.0, 0.25, -0.0, 0.0])
    sc[:, 1] = -sc[:, 0]
    ob, o3, osc, ol = run_batch(ctx, boxes, b3, sc, -1.0, 0.5, 24)
    wb, w3, wsc, wl = D.filter_detections(boxes, b3, sc, -1.0, 24, 0.5)
    assert same_bits([ob, o3, ol], [wb, w3, wl]) and np.array_equal(osc, wsc)


def test_topk_at_its_lds_limit(ctx):
    """8 classes x max_det 1024 with more than 4096 survivors: filter_topk_kernel sorts 8192 keys = 65 536 bytes of dynamic LDS
    beside its static LDS.  The device's per-workgroup limit is read first, so no launch is issued that is expected to fail."""
    limit = torch.cuda.get_device_properties(0).shared_memory_per_block
    print("LDS per workgroup: %d bytes; top-k stage at its limit: %d + %d" % (limit, 65536, TOPK_STATIC_LDS))
    assert 65536 + TOPK_STATIC_LDS <= limit
    rng = np.random.default_rng(8)
    N, Cc = 560, 8
    boxes = grid_boxes(N, cols=28)
    b3 = boxes3d_of(boxes)
    sc = rng.uniform(0.06, 1.0, size=(N, Cc)).astype(F)
    sc[rng.permutation(N)[:40], 5] = 0.0                 # unequal classes: 7 x 560 + 520 = 4440 survivors, all disjoint
    ob, o3, osc, ol = check_vs_oracle(ctx, boxes, b3, sc, 0.05, 0.5, 1024)
    top = np.sort(sc[sc > F(0.05)])[::-1][:1024]
    assert np.array_equal(osc, top) and np.all(ol >= 0)  # by hand: every candidate survives, so the 1024 best scores of all
