"""CPU (no GPU): the numpy restatement of pp_cc_label / pp_cc_select (tests/cc_np.py) against scipy.ndimage -- labels and
numbering against label, boxes against find_objects, areas and sums against sum --, its value mode against "label every byte on
its own, merge, renumber by first pixel", the host-side orderings, the C ABI of the two entry points and the argument refusals
of their wrappers that need no device.  The device side is tests/test_gpu_cc.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from tests import cc_np as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCT = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}

FIXED = [np.zeros((1, 1), np.uint8), np.ones((1, 1), np.uint8), np.ones((1, 70), np.uint8), np.ones((70, 1), np.uint8),
         np.zeros((33, 33), np.uint8), np.ones((33, 33), np.uint8), R.diagonal(), R.serpentine(), R.u_shape(), R.checkerboard(),
         R.late_tile_first(), R.rectangles(True), R.rectangles(False), R.discs()]


def random_cases():
    rng = np.random.default_rng(7)
    cases = []
    for size in list(range(1, 41, 3)) + [31, 32, 33]:
        for density in (0.0, 0.1, 0.3, 0.45, 0.6, 0.75, 0.9, 1.0):
            cases.append(R.random_plane(rng, size, int(rng.integers(1, 41)), density))
    return cases


def against_scipy(plane, conn):
    res = R.cc_label(plane[None], conn, "binary", max_components=2048)
    want, n = ndimage.label(plane != 0, structure=STRUCT[conn])
    assert res["counts"][0] == n and np.array_equal(res["labels"][0], want), (plane.shape, conn)
    idx = np.arange(1, n + 1)
    yy, xx = np.mgrid[0:plane.shape[0], 0:plane.shape[1]]
    boxes = ndimage.find_objects(want)
    assert np.array_equal(res["stats"][0, :n, 0], np.asarray(ndimage.sum(np.ones_like(want), want, idx), np.int64).reshape(-1))
    for k, sl in enumerate(boxes):
        assert res["stats"][0, k, 1:5].tolist() == [sl[1].start, sl[0].start, sl[1].stop - 1, sl[0].stop - 1]
    assert np.array_equal(res["sums"][0, :n, 0], np.asarray(ndimage.sum(xx, want, idx), np.int64).reshape(-1))
    assert np.array_equal(res["sums"][0, :n, 1], np.asarray(ndimage.sum(yy, want, idx), np.int64).reshape(-1))
    assert (res["stats"][0, :n, 5] == 1).all() and not res["stats"][0, n:].any() and not res["sums"][0, n:].any()
    return n


@pytest.mark.parametrize("conn", [4, 8])
def test_restatement_equals_scipy_on_random_planes(conn):
    for plane in random_cases():
        against_scipy(plane, conn)


@pytest.mark.parametrize("conn", [4, 8])
def test_restatement_equals_scipy_on_the_fixed_cases(conn):
    counts = [against_scipy(p, conn) for p in FIXED]
    assert counts[6] == (64 if conn == 4 else 1)          # the diagonal through the four-tile corner
    assert counts[7] == 1 and counts[8] == 1              # serpentine, U
    assert counts[9] == (545 if conn == 4 else 1)         # 33 x 33 checkerboard
    assert counts[10] == 2


def test_late_tile_holds_the_first_component():
    labels = R.cc_label(R.late_tile_first()[None])["labels"][0]
    assert labels[1, 40] == 1 and labels[2, 3] == 2


def value_by_bytes(plane, conn):
    """label each distinct byte on its own, merge, renumber by first pixel"""
    merged = np.zeros(plane.shape, np.int64)
    total = 0
    for b in np.unique(plane[plane != 0]):
        lab, n = ndimage.label(plane == b, structure=STRUCT[conn])
        merged[lab > 0] = lab[lab > 0] + total
        total += n
    flat = merged.ravel()
    firsts = sorted(int(np.argmax(flat == k)) for k in range(1, total + 1))
    out = np.zeros_like(flat)
    for new, p in enumerate(firsts):
        out[flat == flat[p]] = new + 1
    return out.reshape(plane.shape), total


@pytest.mark.parametrize("conn", [4, 8])
def test_value_mode(conn):
    rng = np.random.default_rng(11)
    planes = [R.rectangles(True), R.rectangles(False), R.discs()] + [rng.integers(0, 4, (h, w)).astype(np.uint8) for h, w in ((9, 13), (34, 33), (40, 7))]
    for p in planes:
        res = R.cc_label(p[None], conn, "value", max_components=2048)
        want, n = value_by_bytes(p, conn)
        assert res["counts"][0] == n and np.array_equal(res["labels"][0], want)
        for k in range(n):
            assert (p[want == k + 1] == res["stats"][0, k, 5]).all()
    assert R.cc_label(R.rectangles(True)[None], conn, "value")["counts"][0] == 1
    assert R.cc_label(R.rectangles(False)[None], conn, "value")["counts"][0] == 2
    assert R.cc_label(R.rectangles(False)[None], conn, "binary")["counts"][0] == 1
    d = R.cc_label(R.discs()[None], conn, "value")
    assert d["counts"][0] == 4 and sorted(d["stats"][0, :4, 5].tolist()) == [1, 1, 2, 3]  # the first disc is cut in two


def test_cap_weights_and_select():
    board = R.checkerboard()
    res = R.cc_label(board[None], 4, max_components=16)
    full = R.cc_label(board[None], 4, max_components=600)
    assert res["counts"][0] == 545 and res["labels"].max() == 545 and res["stats"].shape == (1, 16, 6)
    assert np.array_equal(res["stats"][0], full["stats"][0, :16]) and np.array_equal(res["sums"][0], full["sums"][0, :16])
    rng = np.random.default_rng(3)
    plane = np.ones((65, 34), np.uint8)
    wgt = np.full((1, 65, 34), 65535, np.int32)
    s = R.cc_label(plane[None], 8, weight=wgt)["sums"]
    assert s.dtype == np.int64 and s[0, 0].tolist() == [65 * 34 * 33 // 2, 34 * 65 * 64 // 2, 65 * 34 * 65535]
    labels = R.cc_label(R.random_plane(rng, 20, 33, 0.5)[None])["labels"]
    m = R.cc_select(labels, [0, 0, -1, 0, 0, 5], [2, 2, 1, 0, 10 ** 6, 1])
    assert np.array_equal(m[0], labels[0] == 2) and np.array_equal(m[0], m[1]) and m[0].any() and not m[2:].any() and m.dtype == np.uint8


def test_host_orderings():
    p = np.zeros((12, 16), np.uint8)
    p[0:2, 0:2] = 1      # label 1, area 4
    p[0:3, 5:8] = 1      # label 2, area 9
    p[6:9, 0:3] = 1      # label 3, area 9: the tie goes to label 2
    p[10, 10] = 1        # label 4, area 1
    res = R.cc_label(p[None])
    sp, sl, masks = R.select_components(res, min_area=2, keep=3)
    assert sp.tolist() == [0, 0, 0] and sl.tolist() == [2, 3, 1] and masks.sum(axis=(1, 2)).tolist() == [9, 9, 4]
    sp, sl, _ = R.select_components(res, min_area=5, keep=3)
    assert sp.tolist() == [0, 0, -1] and sl.tolist() == [2, 3, 0]
    assert np.array_equal(R.largest_component(p), R.cc_label(p[None])["labels"][0] == 2)
    assert R.remove_small(p, 5).sum() == 18 and R.remove_small(p, 1).sum() == p.sum() and not R.remove_small(p, 10).any()
    pred, (h, w) = mask_output()
    inst = R.instances_from_mask_output(pred, (h, w), max_instances=4)
    # image 0: class 1 holds two blobs with the same score as class 0's blob: class, then label decide
    assert inst["det_labels"][0].tolist() == [2, 0, 1, 1] and inst["det_scores"][0, 1] == inst["det_scores"][0, 2] == inst["det_scores"][0, 3]
    assert inst["det_labels"][1].tolist() == [0, -1, -1, -1] and not inst["det_masks"][1, 1:].any()
    assert inst["boxes"][0, 2].tolist() == [1, 1, 3, 3] and inst["boxes"][0, 3].tolist() == [10, 6, 12, 9]


def mask_output():
    """a seeded 2 x (12 x 16) x 3 prediction: image 0 has one blob of class 0, two of class 1 (all three score 0.75 exactly
    as weights) and a better one of class 2; image 1 one blob of class 0 and a speck below min_area"""
    h, w = 12, 16
    rng = np.random.default_rng(5)
    pred = (rng.random((2, h, w, 3)) * 0.3).astype(np.float32)
    pred[0, 2:5, 2:6, 0] = 0.75
    pred[0, 1:4, 1:4, 1] = 0.75
    pred[0, 6:10, 10:13, 1] = 0.75
    pred[0, 7:11, 2:7, 2] = 0.9
    pred[1, 3:8, 4:9, 0] = 0.8
    pred[1, 10, 14, 2] = 0.99
    return pred.reshape(2, h * w, 3), (h, w)


def test_entry_points_declared_and_exported():
    from pyrapose_amd import _lib
    src = open(os.path.join(ROOT, "include", "pyrapose_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_arg in (("pp_cc_label", 15), ("pp_cc_select", 9)):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.EXPORTS and hasattr(_lib.lib, name)
        fn = getattr(_lib.lib, name)
        decl = re.search(r"int %s\((.*?)\);" % name, code, flags=re.S).group(1).split(",")
        assert len(fn.argtypes) == len(decl) == n_arg and fn.restype == C.c_int
        kinds = ["p" if "*" in a else "z" if "size_t" in a else "i" for a in decl]
        assert [{C.c_void_p: "p", C.c_int: "i", C.c_size_t: "z"}[t] for t in fn.argtypes] == kinds
    # host-side refusals need no device: a NULL context first, as everywhere
    assert _lib.lib.pp_cc_label(None, 1, 8, 8, None, 8, 0, None, 16, None, 0, None, None, None, None) == -4
    assert _lib.lib.pp_cc_select(None, 1, 8, 8, None, 0, None, None, None) == -4
    from pyrapose_amd import ops
    k = open(os.path.join(ROOT, "pyrapose_amd", "csrc", "cc.hip")).read()
    consts = {n: int(v) for n, v in re.findall(r"#define CC_([A-Z_]+) (\d+)\b", k)}
    assert consts["TILE"] == ops.CC_TILE and consts["MAX_COMPONENTS"] == ops.CC_MAX_COMPONENTS
    assert {consts["ERR_TILE"], consts["ERR_CHASE"], consts["ERR_UNION"]} == set(ops.CC_ERRORS)
    modes = {n: int(v) for n, v in re.findall(r"#define PP_CC_([A-Z]+) (\d+)", code)}
    assert [modes[m.upper()] for m in ops.CC_MODES] == [0, 1] and ops.CC_MODES == R.MODES
    assert ops.cc_workspace_bytes(1, 1, 1) == 768 and ops.cc_workspace_bytes(5, 65, 34) == 256 + 2 * 44288


def test_every_while_is_counted():
    """the contract of cc.hip: every `while` counts its steps against a bound and reports through the error word"""
    k = open(os.path.join(ROOT, "pyrapose_amd", "csrc", "cc.hip")).read()
    code = re.sub(r"//[^\n]*", "", k)
    loops = [m.start() for m in re.finditer(r"\bwhile\s*\(", code)]
    assert len(loops) == 2
    for at in loops:
        body = code[at:at + 400]
        assert "> bound" in body and "atomicOr(err" in body
    assert "hipStreamSynchronize" not in code and "hipDeviceSynchronize" not in code and "hipMemcpy" not in code


def test_argument_errors_need_no_device():
    import torch
    from pyrapose_amd import ops
    from pyrapose_amd.utils import components
    host = torch.zeros((1, 8, 8), dtype=torch.uint8)
    for kw, word in ((dict(connectivity=6), "connectivity"), (dict(connectivity="8"), "connectivity"), (dict(mode="label"), "mode"),
                     (dict(max_components=0), "max_components"), (dict(max_components=65536), "max_components"),
                     (dict(max_components=2.5), "max_components")):
        with pytest.raises(ValueError, match=word):
            ops.cc_label(None, host, **kw)
    for planes in (None, np.zeros((1, 8, 8), np.uint8), host):  # not a device tensor
        with pytest.raises(ValueError, match="planes"):
            ops.cc_label(None, planes)
    for labels in (None, np.zeros((1, 8, 8), np.int32), torch.zeros((1, 8, 8), dtype=torch.int32)):
        with pytest.raises(ValueError, match="labels"):
            ops.cc_select(None, labels, None, None)
    with pytest.raises(ValueError, match="order"):
        components.select_components(dict(stats=torch.zeros((1, 4, 6), dtype=torch.int32), sums=torch.zeros((1, 4, 3), dtype=torch.int64)),
                                     order="score")
