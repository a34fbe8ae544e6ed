"""CPU (no GPU): the numpy restatement of pp_draw_overlay_u8 (tests/overlay_np.py) against the properties that pin its rule; the
host side of the overlays -- the 8 x 8 font, the generated colours, OverlayList's packing, png_lite -- and the C ABI of the entry
point.  The device side is tests/test_gpu_overlay.py.  OpenCV is not a dependency: parity with cv2's lines and text is not pinned.

The five functions of the reference's visualization.py are device-only here (there is no host fallback), so what is checked
without a device is their packing, and that they write the drawn batch back into the caller's array: draw_batch is replaced by
the restatement for that."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pyrapose_amd.utils import colors, font8, png_lite
from pyrapose_amd.utils import visualization as V
from tests import overlay_np as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHITE = O.pack_color((255, 255, 255))


def rec(kind, a0, a1, a2, a3, size, colour=WHITE):
    return np.array([kind, a0, a1, a2, a3, size, colour, 0], np.int64)


def seg(x0, y0, x1, y1, t):
    return O.cover_image(rec(O.SEGMENT, x0, y0, x1, y1, t), 48, 56)


def eight_connected(mask):
    """is the set one 8-connected component?"""
    todo = [tuple(np.argwhere(mask)[0])]
    seen = {todo[0]}
    while todo:
        y, x = todo.pop()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                q = (y + dy, x + dx)
                if 0 <= q[0] < mask.shape[0] and 0 <= q[1] < mask.shape[1] and mask[q] and q not in seen:
                    seen.add(q)
                    todo.append(q)
    return len(seen) == int(mask.sum())


@pytest.mark.parametrize("t", [1, 3, 5, 7])
def test_axis_aligned_segments_are_t_thick_between_their_ends(t):
    h = seg(10, 20, 40, 20, t)
    assert (h[:, 10:41].sum(axis=0) == t).all() and h[20 - t // 2:20 + t // 2 + 1, 10:41].all()
    v = seg(25, 8, 25, 39, t)
    assert (v[8:40, :].sum(axis=1) == t).all() and v[8:40, 25 - t // 2:25 + t // 2 + 1].all()
    # the caps: what lies beyond the end points is the half disc of diameter t there, nothing more
    yy, xx = np.mgrid[0:48, 0:56]
    disc0 = 4 * ((xx - 10) ** 2 + (yy - 20) ** 2) <= t * t
    assert np.array_equal(h[:, :10], disc0[:, :10]) and not h[:, 41 + t // 2:].any()
    assert h.sum() == 31 * t + 2 * disc0[:, :10].sum()


@pytest.mark.parametrize("ends", [(5, 5, 50, 9), (5, 40, 9, 3), (3, 3, 44, 44), (50, 2, 4, 45), (20, 20, 21, 20)])
@pytest.mark.parametrize("t", [1, 2, 3, 8])
def test_segments_swap_connect_and_hold_their_ends(ends, t):
    x0, y0, x1, y1 = ends
    m = seg(x0, y0, x1, y1, t)
    assert np.array_equal(m, seg(x1, y1, x0, y0, t))
    assert m[y0, x0] and m[y1, x1] and eight_connected(m)


def test_degenerate_segment_is_the_disc():
    yy, xx = np.mgrid[0:48, 0:56]
    for t in (1, 2, 3, 7, 8, 64):
        assert np.array_equal(seg(30, 22, 30, 22, t), 4 * ((xx - 30) ** 2 + (yy - 22) ** 2) <= t * t), t
    assert seg(30, 22, 30, 22, 7).sum() == 37  # |w|^2 <= 12: what cv2.circle(radius 3, filled) stands for here


def test_segment_arithmetic_fits_its_types():
    """the bound the kernel relies on, at the extreme coordinates: 4 cross^2 < 2^61 and every 32-bit term below 2^31"""
    x, y = np.array([0, 8191, 0, 8191]), np.array([0, 0, 8191, 8191])
    worst = 0
    for x0, y0, x1, y1 in ((-8192, -8192, 8192, 8192), (8192, -8192, -8192, 8192), (-8192, 8192, 8192, 8191), (8192, 8192, -8192, -8192)):
        dx, dy, wx, wy = x1 - x0, y1 - y0, x - x0, y - y0
        for term in (dx * dx + dy * dy, abs(wx * dx + wy * dy).max(), (wx * wx + wy * wy).max(), ((x - x1) ** 2 + (y - y1) ** 2).max()):
            assert int(term) < 2 ** 31
        worst = max(worst, int((4 * (dx * wy - dy * wx) ** 2).max()))
    assert 2 ** 57 < worst < 2 ** 61
    # and the restatement answers there: the far corner pixel lies on the diagonal, its neighbour row does not at t = 1
    m = O.cover(rec(O.SEGMENT, -8192, -8192, 8192, 8192, 1), np.array([8191, 8191]), np.array([8191, 8190]))
    assert m.tolist() == [True, False]


def test_alpha_is_identity_store_and_rounded_blend():
    rng = np.random.default_rng(0)
    px = rng.integers(0, 256, (50, 3)).astype(np.uint8)
    assert np.array_equal(O.paint(px, O.pack_color((9, 200, 77), 0)), px)
    assert (O.paint(px, O.pack_color((9, 200, 77), 255)) == np.array([9, 200, 77])).all()
    half = O.paint(px, O.pack_color((9, 200, 77), 100)).astype(np.int64)
    exact = (100 * np.array([9, 200, 77]) + 155 * px.astype(np.int64)) / 255.0
    assert (np.abs(half - exact) <= 0.5 + 1e-9).all()
    assert O.pack_color((1, 2, 3), 255) < 0 and O.pack_color((1, 2, 3), 127) == 0x7F030201


def test_invalid_records_paint_nothing():
    image = np.random.default_rng(1).integers(0, 256, (20, 24, 3)).astype(np.uint8)
    bad = [rec(3, 0, 0, 10, 10, 2), rec(-1, 0, 0, 10, 10, 2), rec(O.SEGMENT, 0, 0, 10, 10, 0), rec(O.SEGMENT, 0, 0, 10, 10, 65),
           rec(O.SEGMENT, 0, 0, 8193, 10, 2), rec(O.SEGMENT, 0, -8193, 10, 10, 2), rec(O.GLYPH, 2, 2, -1, -1, 0),
           rec(O.GLYPH, 2, 2, -1, -1, 5), rec(O.GLYPH, 2, 2, -1, -1, 1 | 3 << 8), rec(O.GLYPH, 2, 2, -1, -1, 1 | 1 << 16),
           rec(O.GLYPH, 8193, 2, -1, -1, 1)]
    assert np.array_equal(O.draw_image(image, np.stack(bad)), image)
    good = [rec(O.SEGMENT, 0, 0, 8192, 10, 64), rec(O.GLYPH, 2, 2, -1, -1, 4 | 2 << 8), rec(O.FILL_RECT, 2 ** 31 - 1, 5, -2 ** 31, 5, 99)]
    for r in good:
        assert O.cover_image(r, 20, 24).any()
    assert O.cover_image(good[2], 20, 24).sum() == 24  # reversed, far outside: the whole row 5


def test_glyph_cells_scale_and_dilate():
    lo, hi = 1 | 1 << 9, -(1 << 31)  # cells (0,0), (1,1) and (7,7)
    m = O.cover_image(rec(O.GLYPH, 3, 2, lo, hi, 1), 16, 16)
    assert sorted(map(tuple, np.argwhere(m))) == [(2, 3), (3, 4), (9, 10)]
    m3 = O.cover_image(rec(O.GLYPH, 3, 2, lo, hi, 3), 40, 40)
    assert m3.sum() == 27 and m3[2:5, 3:6].all() and m3[5:8, 6:9].all() and m3[23:26, 24:27].all()
    d = O.cover_image(rec(O.GLYPH, 3, 2, 1, 0, 2 | 2 << 8), 16, 16)  # one 2 x 2 cell grown by 2 all round: 6 x 6, cut at the top
    assert d.sum() == 6 * 6 and d[0:6, 1:7].all()
    # dilation reaches out of the cell grid, and in from a cell that lies outside the image
    e = O.cover_image(rec(O.GLYPH, -1, -1, 1, 0, 1 | 1 << 8), 8, 8)
    assert sorted(map(tuple, np.argwhere(e))) == [(0, 0)]


def test_outline_is_an_inner_contour():
    ids = np.zeros((20, 24), np.uint8)
    ids[5:12, 6:15] = 3
    one = O.outline_mask(ids, 1)
    border = np.zeros_like(one)
    border[5:12, 6:15] = True
    border[6:11, 7:14] = False
    assert np.array_equal(one, border)
    for w in (1, 2, 4):
        assert not (O.outline_mask(ids, w) & (ids == 0)).any()  # a subset of the fill
    assert np.array_equal(O.outline_mask(ids, 4), ids != 0)       # 7 rows: every pixel is within 4 of the rim
    # a rectangle in the image's corner has no contour along the image's border
    ids = np.zeros((20, 24), np.uint8)
    ids[0:6, 0:8] = 9
    want = np.zeros((20, 24), bool)
    want[5, 0:8] = True
    want[0:6, 7] = True
    assert np.array_equal(O.outline_mask(ids, 1), want)
    # two labels that touch outline each other; palette entry 0 is never drawn
    ids[0:6, 8:12] = 4
    assert O.outline_mask(ids, 1)[0:5, 8].all() and O.outline_mask(ids, 1)[0:5, 7].all()
    image = np.full((20, 24, 3), 50, np.uint8)
    pal = np.array([O.pack_color((1, 2, 3))] + [O.pack_color((k, k, 255 - k)) for k in range(1, 256)], np.int64)
    out = O.draw_image(image, np.zeros((0, 8), np.int64), ids, pal, fill=True, outline=0)
    assert (out[ids == 0] == 50).all() and (out[ids == 9] == (9, 9, 246)).all() and (out[ids == 4] == (4, 4, 251)).all()


def test_batch_offsets_and_order():
    images = np.zeros((3, 6, 7, 3), np.uint8)
    prims = np.stack([rec(O.FILL_RECT, 0, 0, 6, 5, 0, O.pack_color((10, 0, 0))), rec(O.FILL_RECT, 1, 1, 2, 2, 0, O.pack_color((20, 0, 0))),
                      rec(O.FILL_RECT, 0, 0, 0, 0, 0, O.pack_color((30, 0, 0)))])
    out = O.draw_overlay(images, prims, [0, 2, 2, 3])
    assert out[0, 0, 0, 0] == 10 and out[0, 1, 1, 0] == 20 and not out[1].any() and out[2, 0, 0, 0] == 30 and out[2].sum() == 30
    assert O.draw_overlay(images, prims[[1, 0]], [0, 2, 2, 2])[0, 1, 1, 0] == 10  # later over earlier


def test_font():
    assert len(font8.REQUIRED) == 10 + 26 + 26 + 13 and set(font8.REQUIRED) == set(font8.GLYPHS)
    words = [font8.glyph(ch) for ch in font8.REQUIRED]
    assert len(set(words)) == len(words) and font8.BOX not in words
    for ch, v in zip(font8.REQUIRED, words):
        assert 0 <= v < 1 << 64
        assert (v != 0) == (ch != " "), ch                       # the space is blank, nothing else is
        assert not any(v >> (8 * r + 7) & 1 for r in range(8)), ch  # column 7 is blank in every glyph
    assert font8.glyph("~") == font8.BOX == font8.glyph("é")
    assert font8.render("L") == ["#.......", "#.......", "#.......", "#.......", "#.......", "#.......", "#####...", "........"]
    lo, hi = font8.glyph_words("=")
    assert (lo & 0xFFFFFFFF) | (hi & 0xFFFFFFFF) << 32 == font8.glyph("=") and -2 ** 31 <= lo < 2 ** 31 and -2 ** 31 <= hi < 2 ** 31


def test_label_colors():
    cols = [colors.label_color(k) for k in range(360)]
    assert len(set(cols)) == 360 and colors.label_color(0) == (255, 0, 0)
    for c in cols:
        assert max(c) == 255 and min(c) == 0 and all(isinstance(v, int) for v in c)  # full saturation and value
    with pytest.raises(ValueError):
        colors.label_color(-1)
    pal = V.pack_palette(None, 96)
    assert pal.dtype == np.int32 and pal.shape == (256,) and (pal.view(np.uint32) >> 24 == 96).all()
    assert V.pack_palette()[1] == V.pack_color(colors.label_color(0), 255)
    with pytest.raises(ValueError):
        V.pack_palette(np.zeros((255, 3)))


def test_overlay_list_packs_by_image_in_order():
    ov = V.OverlayList(3)
    ov.fill_rect(2, (1, 2), (3, 4), (1, 2, 3))
    ov.segment(0, (0.5, 1.5), (2.5, 3.5), (9, 8, 7), thickness=5, alpha=128)   # half to even: 0, 2, 2, 4
    ov.disc(2, (10, 11), (4, 5, 6))
    ov.box(0, (1, 2, 30, 40), (0, 255, 0))
    prims, off = ov.pack()
    assert prims.dtype == np.int32 and prims.shape == (7, 8) and off.dtype == np.int32 and off.tolist() == [0, 5, 5, 7] and len(ov) == 7
    assert prims[0].tolist() == [O.SEGMENT, 0, 2, 2, 4, 5, O.pack_color((9, 8, 7), 128), 0]
    assert prims[1:5, 1:5].tolist() == [[1, 2, 30, 2], [30, 2, 30, 40], [30, 40, 1, 40], [1, 40, 1, 2]] and (prims[1:5, 5] == 2).all()
    assert prims[5].tolist() == [O.FILL_RECT, 1, 2, 3, 4, 0, O.pack_color((1, 2, 3)), 0]
    assert prims[6].tolist() == [O.SEGMENT, 10, 11, 10, 11, 7, O.pack_color((4, 5, 6)), 0]
    empty = V.OverlayList(2).pack()
    assert empty[0].shape == (0, 8) and empty[1].tolist() == [0, 0, 0]
    for bad in (lambda: ov.segment(0, (0, 0), (1, 1), (0, 0, 0), thickness=65), lambda: ov.segment(0, (0, 0), (1, 1), (0, 0, 256)),
                lambda: ov.text(0, (0, 0), "a", (0, 0, 0), scale=5), lambda: ov.segment(3, (0, 0), (1, 1), (0, 0, 0)), lambda: V.OverlayList(0)):
        with pytest.raises((ValueError, IndexError)):
            bad()


def test_box3d_edges_pose_axes_and_dropped():
    ov = V.OverlayList(1)
    corners = np.arange(16, dtype=np.float64) * 10
    ov.box3d(0, corners, (255, 0, 0))
    prims, _ = ov.pack()
    # linemod_eval.py:554-595: corner pairs 0-1, 1-2, 2-3, 3-0, 0-4, 1-5, 2-6, 3-7, 4-5, 5-6, 6-7, 7-4
    order = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 4), (1, 5), (2, 6), (3, 7), (4, 5), (5, 6), (6, 7), (7, 4)]
    assert prims[:, 1:5].tolist() == [[20 * a, 20 * a + 10, 20 * b, 20 * b + 10] for a, b in order] and (prims[:, 5] == 2).all()
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    box = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float64) * 0.05
    ov = V.OverlayList(1)
    ov.pose(0, np.eye(3), [0.0, 0.0, 1.0], K, box, (0, 204, 0))
    prims, _ = ov.pack()
    uv = box[:, :2] * 500.0 / (box[:, 2:3] + 1.0) + [320, 240]
    assert len(prims) == 12 and ov.dropped == 0 and prims[0, 1:5].tolist() == np.rint(np.concatenate([uv[0], uv[1]])).astype(int).tolist()
    ov.pose(0, np.eye(3), [0.0, 0.0, 0.02], K, box, (0, 204, 0))  # the four near corners are behind the camera: 8 edges have no image
    assert ov.dropped == 8 and len(ov) == 16
    ov.segment(0, (0, 0), (9000, 0), (1, 1, 1))
    ov.segment(0, (np.inf, 0), (1, 0), (1, 1, 1))
    ov.fill_rect(0, (0, -8193), (1, 1), (1, 1, 1))
    assert ov.dropped == 11 and len(ov) == 16
    ov = V.OverlayList(1)
    ov.axes(0, np.eye(3), [0.0, 0.0, 1000.0], K)
    prims, _ = ov.pack()
    assert prims[:, 1:5].tolist() == [[320, 240, 370, 240], [320, 240, 320, 290], [320, 240, 320, 240]] and (prims[:, 5] == 3).all()
    assert prims[:, 6].tolist() == [O.pack_color(c) for c in ((255, 0, 0), (0, 255, 0), (0, 0, 255))]


def test_text_and_caption_records():
    ov = V.OverlayList(1)
    ov.text(0, (10, 30), "a b", (1, 2, 3), scale=2, halo=(9, 9, 9))
    prims, _ = ov.pack()
    # halo pass first (dilate 1), then the text; the space has no record; the baseline row 30 is the last pixel row of cell row 6
    assert prims[:, 0].tolist() == [O.GLYPH] * 4 and prims[:, 5].tolist() == [2 | 1 << 8] * 2 + [2] * 2
    assert prims[:, 1].tolist() == [10, 10 + 2 * 2 * font8.ADVANCE] * 2 and (prims[:, 2] == 30 - 13).all()
    assert prims[:, 6].tolist() == [O.pack_color((9, 9, 9))] * 2 + [O.pack_color((1, 2, 3))] * 2
    assert tuple(prims[0, 3:5]) == font8.glyph_words("a") and tuple(prims[1, 3:5]) == font8.glyph_words("b")
    covered = O.cover_image(prims[2].astype(np.int64), 40, 40)
    assert covered[30].any() and not covered[31:].any()  # 'a' stands on the baseline
    ov = V.OverlayList(1)
    ov.caption(0, (20.4, 50.6, 80, 90), "x")
    prims, _ = ov.pack()
    assert prims[:, 1:3].tolist() == [[20, 41 - 6]] * 2 and prims[:, 6].tolist() == [O.pack_color((0, 0, 0)), O.pack_color((255, 255, 255))]


def restated_draw_batch(images, overlay, ids=None, palette=None, fill_alpha=None, outline=0, ctx=None):
    prims, off = overlay.pack()
    return O.draw_overlay(images, prims, off)


def test_reference_functions_pack_and_write_back(monkeypatch):
    monkeypatch.setattr(V, "draw_batch", restated_draw_batch)
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (60, 80, 3)).astype(np.uint8)
    boxes = np.array([[10.2, 20.7, 40, 50], [30, 25, 70, 55], [5, 5, 20, 20]])
    scores, labels = np.array([0.9, 0.4, 0.87]), np.array([1, 2, 0])
    name = lambda l: "obj%d" % int(l)

    def expect(build):
        ov = V.OverlayList(1)
        build(ov)
        return O.draw_overlay(base[None], *ov.pack())[0]

    image = base.copy()
    assert V.draw_box(image, boxes[0], (0, 0, 255)) is None
    assert not np.array_equal(image, base) and np.array_equal(image, expect(lambda ov: ov.box(0, boxes[0], (0, 0, 255))))
    image = base.copy()
    V.draw_boxes(image, boxes, (7, 8, 9), thickness=3)
    assert np.array_equal(image, expect(lambda ov: [ov.box(0, b, (7, 8, 9), 3) for b in boxes]))
    image = base.copy()
    V.draw_caption(image, boxes[1], "cap")
    assert np.array_equal(image, expect(lambda ov: ov.caption(0, boxes[1], "cap")))

    def detections(ov):  # score > 0.5 only, box then caption, 'name: 0.87'
        for k in (0, 2):
            ov.box(0, boxes[k], colors.label_color(labels[k]))
            ov.caption(0, boxes[k], "obj%d: %s" % (labels[k], ("0.90", "", "0.87")[k]))
    image = base.copy()
    V.draw_detections(image, boxes, scores, labels, label_to_name=name)
    assert np.array_equal(image, expect(detections))

    def annotations(ov):  # caption then box, green
        for k in range(3):
            ov.caption(0, boxes[k], "obj%d" % labels[k])
            ov.box(0, boxes[k], (0, 255, 0))
    image = base.copy()
    V.draw_annotations(image, dict(bboxes=boxes, labels=labels), label_to_name=name)
    assert np.array_equal(image, expect(annotations))
    image2 = base.copy()
    V.draw_annotations(image2, np.concatenate([boxes, labels[:, None]], axis=1), label_to_name=name)
    assert np.array_equal(image2, image)
    with pytest.raises(ValueError):
        V.draw_box(base.astype(np.float32), boxes[0], (0, 0, 255))


def test_png_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    for shape in ((1, 1), (7, 13), (5, 9, 3), (480, 640, 3)):
        a = rng.integers(0, 256, shape).astype(np.uint8)
        path = str(tmp_path / "a.png")
        png_lite.write_png(path, a)
        b = png_lite.read_png(path)
        assert b.dtype == np.uint8 and np.array_equal(a, b), shape
    data = png_lite.encode_png(a)
    with pytest.raises(ValueError):
        png_lite.decode_png(data[:40] + bytes([data[40] ^ 1]) + data[41:])  # a flipped bit: the CRC notices
    with pytest.raises(ValueError):
        png_lite.decode_png(b"not a png")
    for bad in (np.zeros((4, 4), np.uint16), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError):
            png_lite.encode_png(bad)


def test_png_and_pil_read_each_other(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    smooth = (np.add.outer(np.arange(37), np.arange(53)) * 3 % 256).astype(np.uint8)  # makes PIL's encoder pick its filters
    for a in (rng.integers(0, 256, (21, 34, 3)).astype(np.uint8), rng.integers(0, 256, (21, 34)).astype(np.uint8), smooth,
              np.stack([smooth, smooth.T[:37, :37].repeat(2, 1)[:, :53], 255 - smooth], axis=2)):
        path = str(tmp_path / "ours.png")
        png_lite.write_png(path, a)
        with Image.open(path) as im:
            assert np.array_equal(np.asarray(im), a)
        theirs = str(tmp_path / "pil.png")
        Image.fromarray(a).save(theirs)
        assert np.array_equal(png_lite.read_png(theirs), a)


def test_entry_point_declared_and_exported():
    from pyrapose_amd import _lib
    src = open(os.path.join(ROOT, "include", "pyrapose_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    name = "pp_draw_overlay_u8"
    assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.EXPORTS and hasattr(_lib.lib, name)
    fn = _lib.lib.pp_draw_overlay_u8
    decl = re.search(r"int pp_draw_overlay_u8\((.*?)\);", code, flags=re.S).group(1)
    assert len(fn.argtypes) == len(decl.split(",")) == 13 and fn.restype == C.c_int
    kinds = ["p" if "*" in a else "i" for a in decl.split(",")]
    assert [{C.c_void_p: "p", C.c_int: "i"}[t] for t in fn.argtypes] == kinds
    # host-side refusals need no device: a NULL context first, as everywhere
    assert fn(None, 1, 8, 8, None, None, None, None, 0, None, None, 0, 1) == -4
    from pyrapose_amd import ops
    k = open(os.path.join(ROOT, "pyrapose_amd", "csrc", "overlay.hip")).read()
    consts = {n: int(v) for n, v in re.findall(r"#define OV_([A-Z_]+) (\d+)\b", k)}
    assert consts["TILE"] == ops.OVERLAY_TILE and consts["CHUNK"] == ops.OVERLAY_CHUNK and consts["MAX_SIDE"] == ops.OVERLAY_MAX_SIDE == O.MAX_SIDE
    assert consts["MAX_COORD"] == ops.OVERLAY_MAX_COORD == O.MAX_COORD == V.MAX_COORD and consts["HALO"] == ops.OVERLAY_MAX_OUTLINE == O.MAX_OUTLINE
    assert consts["MAX_THICK"] == ops.OVERLAY_MAX_THICK == O.MAX_THICK == V.MAX_THICK and consts["MAX_SCALE"] == ops.OVERLAY_MAX_SCALE == O.MAX_SCALE
    assert consts["MAX_DILATE"] == ops.OVERLAY_MAX_DILATE == O.MAX_DILATE
    assert (consts["SEGMENT"], consts["GLYPH"], consts["FILL_RECT"]) == (O.SEGMENT, O.GLYPH, O.FILL_RECT) == (V.SEGMENT, V.GLYPH, V.FILL_RECT)


def test_argument_errors_need_no_device():
    from pyrapose_amd import ops
    with pytest.raises(ValueError):
        ops.draw_overlay(None, np.zeros((1, 8, 8, 3), np.uint8), None, None)  # not a device tensor
    with pytest.raises(ValueError):
        ops.draw_overlay(None, None, None, None)


def test_evaluate_still_refuses_save_path():
    from pyrapose_amd.utils.eval import evaluate
    with pytest.raises(NotImplementedError, match="save_detection_images"):
        evaluate(None, None, save_path="somewhere")
