"""GPU: pp_cc_label / pp_cc_select (csrc/cc.hip, ops.cc_label / cc_select, utils.components) against the numpy restatement
tests/cc_np.py -- every output byte for byte -- at the edges of the 32 x 32 tiles, across their seams and corners, through the
numbering scan, the cap M, value mode, weights, the batch, and the host helpers up to evaluate_masks.  The error word is
checked to be clear after every call."""
import numpy as np
import pytest
import torch

from tests import cc_np as R
from tests.test_cc_cpu import mask_output

pytestmark = pytest.mark.gpu

KEYS = ("labels", "counts", "stats", "sums")
DTYPES = dict(labels=torch.int32, counts=torch.int32, stats=torch.int32, sums=torch.int64)


def device(planes, conn=8, mode="binary", weight=None, M=256):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    p = torch.from_numpy(np.ascontiguousarray(planes)).cuda()
    w = None if weight is None else torch.from_numpy(np.ascontiguousarray(weight, np.int32)).cuda()
    out = ops.cc_label(default_context(), p, conn, mode, w, M)
    assert int(out["error"].item()) == 0
    for k in KEYS:
        assert out[k].dtype == DTYPES[k]
    return {k: out[k].cpu().numpy() for k in KEYS}, out


def check(planes, conn=8, mode="binary", weight=None, M=256):
    planes = np.asarray(planes, np.uint8)
    planes = planes[None] if planes.ndim == 2 else planes
    want = R.cc_label(planes, conn, mode, weight, M)
    got, _ = device(planes, conn, mode, weight, M)
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), "%s: %d values differ" % (k, int((got[k] != want[k]).sum()))
    return want


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 70), (70, 1), (31, 31), (32, 32), (33, 33), (65, 34)])
def test_tile_edges(H, W, conn):
    rng = np.random.default_rng(H * 100 + W)
    check(np.stack([R.random_plane(rng, H, W, d) for d in (0.3, 0.6, 0.9)]), conn, M=1024)


@pytest.mark.parametrize("conn", [4, 8])
def test_seams(conn):
    assert check(R.diagonal(), conn)["counts"][0] == (64 if conn == 4 else 1)
    assert check(R.serpentine(), conn)["counts"][0] == 1
    assert check(R.u_shape(), conn)["counts"][0] == 1
    assert check(R.checkerboard(), conn, M=600)["counts"][0] == (545 if conn == 4 else 1)
    assert check(R.diagonal()[:, ::-1], conn)["counts"][0] == (64 if conn == 4 else 1)  # the other diagonal of the corner


def test_numbering_across_tiles():
    want = check(R.late_tile_first())
    assert want["labels"][0, 1, 40] == 1 and want["labels"][0, 2, 3] == 2


@pytest.mark.parametrize("conn", [4, 8])
def test_empty_full_and_batch(conn):
    rng = np.random.default_rng(9)
    H, W = 65, 34
    planes = np.stack([np.zeros((H, W), np.uint8), R.random_plane(rng, H, W, 0.3), R.random_plane(rng, H, W, 0.6),
                       R.random_plane(rng, H, W, 0.9), np.full((H, W), 200, np.uint8)])
    want = check(planes, conn, M=512)
    assert want["counts"][0] == 0 and want["counts"][4] == 1 and want["stats"][4, 0].tolist() == [H * W, 0, 0, W - 1, H - 1, 1]
    for i in range(5):  # one at a time: the same bytes
        got, _ = device(planes[i:i + 1], conn, M=512)
        for k in KEYS:
            assert np.array_equal(got[k][0], want[k][i]), (i, k)


def test_cap():
    want = check(R.checkerboard(), 4, M=16)
    assert want["counts"][0] == 545 and want["labels"].max() == 545 and want["stats"].shape == (1, 16, 6) and want["stats"][0, :, 0].all()
    check(np.stack([R.checkerboard(), R.checkerboard()[::-1] * 0, R.checkerboard()]), 4, M=1)


@pytest.mark.parametrize("conn", [4, 8])
def test_value_mode(conn):
    assert check(R.rectangles(False), conn, "value")["counts"][0] == 2
    assert check(R.rectangles(True), conn, "value")["counts"][0] == 1
    assert check(R.rectangles(False), conn, "binary")["counts"][0] == 1
    want = check(R.discs(), conn, "value")
    assert want["counts"][0] == 4 and sorted(want["stats"][0, :4, 5].tolist()) == [1, 1, 2, 3]
    rng = np.random.default_rng(13)
    check(rng.integers(0, 4, (3, 65, 34)).astype(np.uint8), conn, "value", M=2048)


def test_weights():
    rng = np.random.default_rng(17)
    H, W = 65, 34
    planes = np.stack([R.random_plane(rng, H, W, 0.6), np.ones((H, W), np.uint8)])
    weight = rng.integers(0, 65536, (2, H, W)).astype(np.int32)
    weight[1] = 65535
    want = check(planes, 8, weight=weight)
    assert want["sums"].dtype == np.int64 and want["sums"][1, 0, 2] == H * W * 65535
    _, out = device(planes, 8, weight=weight)
    assert out["sums"].dtype == torch.int64


@pytest.mark.parametrize("W", [33, 64])
def test_select(W):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    rng = np.random.default_rng(W)
    planes = np.stack([R.random_plane(rng, 21, W, 0.4), R.random_plane(rng, 21, W, 0.5), np.zeros((21, W), np.uint8)])
    want = R.cc_label(planes)
    _, out = device(planes)
    n0, n1 = int(want["counts"][0]), int(want["counts"][1])
    plane = np.array([0, 0, 1, -1, 1, 0, 1, 2, 0, 7], np.int32)     # a repeat, padding both ways, beyond the count, past the planes
    label = np.array([1, 1, n1, 3, 0, n0 + 1, -2, 1, n0, 1], np.int32)
    masks = ops.cc_select(default_context(), out["labels"], torch.from_numpy(plane).cuda(), torch.from_numpy(label).cuda())
    ref = R.cc_select(want["labels"], plane, label)
    assert masks.dtype == torch.uint8 and np.array_equal(masks.cpu().numpy(), ref)
    assert ref[0].any() and ref[2].any() and ref[8].any() and not ref[[3, 4, 5, 6, 7, 9]].any()


def test_host_helpers():
    from pyrapose_amd.utils import components as Cm
    rng = np.random.default_rng(21)
    planes = np.stack([R.random_plane(rng, 65, 34, 0.3), R.random_plane(rng, 65, 34, 0.6), np.zeros((65, 34), np.uint8), R.u_shape()[:65, :34]])
    assert np.array_equal(Cm.largest_component(planes).cpu().numpy(), R.largest_component(planes))
    assert np.array_equal(Cm.largest_component(planes[1], connectivity=4).cpu().numpy(), R.largest_component(planes[1], 4))
    for min_area in (1, 3, 40):
        assert np.array_equal(Cm.remove_small(planes, min_area).cpu().numpy(), R.remove_small(planes, min_area))
    assert np.array_equal(Cm.remove_small(planes[1], 2, max_components=8).cpu().numpy(), R.remove_small(planes[1], 2, max_components=8))
    ids = rng.integers(0, 3, (2, 20, 33)).astype(np.uint8)
    assert np.array_equal(Cm.remove_small(ids, 4, mode="value").cpu().numpy(), R.remove_small(ids, 4, mode="value"))
    weight = rng.integers(0, 65536, planes.shape).astype(np.int32)
    res = Cm.label_masks(planes, weight=weight, max_components=64)
    assert int(res["error"].item()) == 0
    host = R.cc_label(planes, weight=weight, max_components=64)
    for order, min_area, keep in (("area", 1, 3), ("weight", 2, 5), ("area", 30, None)):
        sp, sl, masks = Cm.select_components(res, min_area, keep, order)
        wp, wl, wm = R.select_components(host, min_area, keep, order)
        assert sp.dtype == sl.dtype == torch.int32 and np.array_equal(sp.cpu().numpy(), wp) and np.array_equal(sl.cpu().numpy(), wl)
        assert np.array_equal(masks.cpu().numpy(), wm)


def test_instances_from_mask_output():
    from pyrapose_amd.utils import components as Cm
    from pyrapose_amd.utils.mask_eval import evaluate_masks
    pred, (h, w) = mask_output()
    want = R.instances_from_mask_output(pred, (h, w), max_instances=4)
    for p in (pred, pred.reshape(2, h, w, 3)):
        got = Cm.instances_from_mask_output(p, (h, w), max_instances=4)
        assert int(got["error"].item()) == 0
        assert got["det_scores"].dtype == torch.float64 and got["det_labels"].dtype == torch.int32 and got["det_masks"].dtype == torch.uint8
        for k in ("det_masks", "det_scores", "det_labels", "boxes"):
            assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert want["det_labels"][0].tolist() == [2, 0, 1, 1] and want["det_labels"][1].tolist() == [0, -1, -1, -1]
    # the same instances as ground truth: every one is matched at every threshold
    live = want["det_labels"] >= 0
    gt_masks, gt_labels = want["det_masks"][live], want["det_labels"][live]
    gt_offsets = np.concatenate([[0], np.cumsum(live.sum(axis=1))]).astype(np.int32)
    res = evaluate_masks(got["det_masks"], got["det_scores"], got["det_labels"], gt_masks, gt_labels, gt_offsets)
    assert res["AP"] == 1.0 and res["AP50"] == 1.0
    # more slots than candidates
    wide = Cm.instances_from_mask_output(pred, (h, w), max_instances=8, max_components=2)
    ref = R.instances_from_mask_output(pred, (h, w), max_instances=8, max_components=2)
    for k in ("det_masks", "det_scores", "det_labels", "boxes"):
        assert np.array_equal(wide[k].cpu().numpy(), ref[k]), k
