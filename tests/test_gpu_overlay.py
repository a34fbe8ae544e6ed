"""GPU: pp_draw_overlay_u8 (csrc/overlay.hip, ops.draw_overlay, utils.visualization) against its numpy restatement
tests/overlay_np.py -- every output byte for byte -- at the edges of its 32 x 32 tiles, of the 4-pixel spans a thread owns, of
the 64-lane ballots and the 256-record chunks of the list walk, and of the id layer's halo; then end to end from an OverlayList
through draw_batch, the reference's in-place functions, and the PNGs of save_detection_images and evaluate_pose_metrics(draw=)."""
import os

import numpy as np
import pytest
import torch

from pyrapose_amd.utils import font8
from pyrapose_amd.utils import visualization as V
from tests import overlay_np as O

pytestmark = pytest.mark.gpu

T = 32  # ops.OVERLAY_TILE (asserted in tests/test_overlay_cpu.py against the kernel's define)
SIZES = [(1, 1, 1), (1, 64, 32), (1, 33, 31), (3, 70, 45)]  # (B, W, H): one pixel, exact tiles, ragged both ways, a batch


def col(rng, alpha=None):
    return O.pack_color(rng.integers(0, 256, 3), int(rng.integers(0, 256)) if alpha is None else alpha)


def rec(kind, a0, a1, a2, a3, size, colour):
    return [kind, a0, a1, a2, a3, size, colour, 0]


def background(rng, B, H, W):
    return rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)


def device(images, prims, offsets, ids=None, palette=None, fill=False, outline=0, in_place=False):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    img = torch.from_numpy(np.ascontiguousarray(images)).cuda()
    p = torch.from_numpy(np.asarray(prims, np.int64).reshape(-1, 8).astype(np.int32)).cuda()
    o = torch.from_numpy(np.asarray(offsets, np.int32)).cuda()
    i = None if ids is None else torch.from_numpy(np.ascontiguousarray(ids)).cuda()
    pal = None if palette is None else torch.from_numpy(np.asarray(palette, np.int64).astype(np.uint32).view(np.int32)).cuda()
    out = ops.draw_overlay(default_context(), img, p, o, i, pal, fill, outline, out=img if in_place else None)
    assert out.dtype == torch.uint8 and tuple(out.shape) == images.shape and (out.data_ptr() == img.data_ptr()) == in_place
    if not in_place:
        assert np.array_equal(img.cpu().numpy(), images)  # the input is left alone
    return out.cpu().numpy()


def check(images, prims, offsets, **kw):
    want = O.draw_overlay(images, prims, offsets, **kw)
    got = device(images, prims, offsets, **kw)
    assert got.dtype == want.dtype and np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    return want


def spread(per_image):
    """lists of records per image -> (prims, offsets)"""
    off = np.cumsum([0] + [len(p) for p in per_image])
    flat = [r for p in per_image for r in p]
    return np.asarray(flat, np.int64).reshape(-1, 8), off


def segments(rng, W, H):
    s = []
    for t in (1, 2, 3, 64):
        # across the seams at x = 32 and y = 32: shallow, steep, both diagonals
        s += [(2, 29, W + 5, 35, t), (29, -3, 35, H + 4, t), (20, 20, 44, 44, t), (44, 20, 20, 44, t)]
    for t in (1, 3):
        # an end point outside on each side, wholly outside on each side, and the far corners of the coordinate range
        s += [(-9, 5, 6, 8, t), (W - 4, 3, W + 11, 9, t), (7, -6, 3, 4, t), (5, H - 3, 9, H + 8, t),
              (-40, 3, -5, 9, t), (W + 3, 0, W + 30, H, t), (0, -20, W, -4, t), (0, H + 3, W, H + 9, t),
              (-8192, -8192, 8192, 8192, t), (8192, -8192, -8192, 8192, t), (-8192, H // 2, 8192, H // 2 + 1, t), (8192, 8192, 8100, 8100, t)]
    s += [(T, T, T, T, t) for t in (1, 2, 7, 9)]             # discs centred on a tile corner
    s += [(T - 1, T - 1, T - 1, T - 1, 64), (0, 0, 0, 0, 5)]
    return [rec(O.SEGMENT, *v, col(rng)) for v in s]


@pytest.mark.parametrize("B,W,H", SIZES)
def test_segments(B, W, H):
    rng = np.random.default_rng(W * 100 + H)
    images = background(rng, B, H, W)
    per_image = [segments(rng, W, H) for _ in range(B)]
    if B == 3:
        per_image[1] = []  # the middle image's list is empty: offsets[1] == offsets[2]
    prims, off = spread(per_image)
    want = check(images, prims, off)
    if B == 3:
        assert np.array_equal(want[1], images[1]) and not np.array_equal(want[0], images[0])


def test_one_segment_at_a_time_over_the_seams():
    """each on its own (opaque on black), so that a wrong pixel is not painted over by a later record"""
    rng = np.random.default_rng(2)
    W, H = 70, 45
    recs = [r for r in segments(rng, W, H) if r[5] in (1, 2, 3)][:40]
    images = np.zeros((len(recs), H, W, 3), np.uint8)
    for r in recs:
        r[6] = O.pack_color((255, 128, 1))
    prims, off = spread([[r] for r in recs])
    check(images, prims, off)


@pytest.mark.parametrize("n", [64, 65, 255, 256, 257, 600])
def test_order_across_waves_and_chunks(n):
    """n records that all cover the block around the tile corner (33..38, 30..34), distinct colours, mixed alpha: the last
    writer and the whole blend chain; then the same list with every other record made invalid (compaction over gaps)"""
    rng = np.random.default_rng(n)
    W, H = 70, 45
    images = background(rng, 2, H, W)
    recs = []
    for k in range(n):
        c = O.pack_color(((k * 7) % 256, (k * 13 + 5) % 256, k % 256), (255, 40, 128, 200, 0)[k % 5] if k % 11 else 255)
        kind = k % 3
        if kind == O.SEGMENT:
            recs.append(rec(O.SEGMENT, 30 + k % 5, 29 + k % 3, 41 - k % 4, 36 - k % 2, 9, c))
        elif kind == O.GLYPH:
            recs.append(rec(O.GLYPH, 29 + k % 2, 27, -1, -1, 2, c))  # all 64 cells, 16 x 16 pixels
        else:
            recs.append(rec(O.FILL_RECT, 33 - k % 4, 30 - k % 3, 38 + k % 6, 34 + k % 2, 0, c))
    holes = [list(r) for r in recs]
    for k in range(0, n, 2):
        holes[k][0] = 7 if k % 4 else -1                 # an unknown kind ...
        if k % 6 == 0:
            holes[k] = rec(O.SEGMENT, 30, 30, 40, 36, 65, holes[k][6])  # ... or a field out of range
    prims, off = spread([recs, holes])
    want = check(images, prims, off)
    assert (want[:, 30:35, 33:39] != images[:, 30:35, 33:39]).any(axis=(1, 2, 3)).all()
    last = recs[-1]
    if (last[6] >> 24) & 255 == 255:
        assert (want[0, 32, 35] == [last[6] & 255, (last[6] >> 8) & 255, (last[6] >> 16) & 255]).all()


def test_glyphs():
    rng = np.random.default_rng(5)
    W, H = 70, 45
    one, last, full = (1, 0), (0, -(1 << 31)), (-1, -1)
    per_image = []
    for scale in (1, 4):
        for dilate in (0, 1, 2):
            size = scale | dilate << 8
            recs = [rec(O.GLYPH, T - 3 * scale, T - 5 * scale, *font8.glyph_words("R"), size, col(rng)),   # a cell astride the seams
                    rec(O.GLYPH, -3 * scale, 8, *font8.glyph_words("g"), size, col(rng)),                   # cut by each border
                    rec(O.GLYPH, W - 4 * scale, 3, *font8.glyph_words("%"), size, col(rng)),
                    rec(O.GLYPH, 12, -4 * scale, *font8.glyph_words("W"), size, col(rng)),
                    rec(O.GLYPH, 40, H - 3 * scale, *font8.glyph_words("8"), size, col(rng)),
                    rec(O.GLYPH, 50, 20, *one, size, col(rng)), rec(O.GLYPH, 20 - 7 * scale, 30 - 7 * scale, *last, size, col(rng)),
                    rec(O.GLYPH, -1 - 8 * scale, -1 - 8 * scale, *last, size, col(rng)),   # bit 63 just outside: only its dilation shows
                    rec(O.GLYPH, W, H, *one, size, col(rng)), rec(O.GLYPH, 8192, -8192, *full, size, col(rng)),
                    rec(O.GLYPH, T - 8 * scale, 2, *full, size, col(rng, 255))]
            per_image.append(recs)
    prims, off = spread(per_image)
    images = background(rng, len(per_image), H, W)
    want = check(images, prims, off)
    assert (want[0, 2:10, T - 8:T] == want[0, 2, T - 8]).all()  # the full bitmap at scale 1: an 8 x 8 block, ending at the seam
    single = np.zeros((2, 9, 9, 3), np.uint8)
    white = O.pack_color((255, 255, 255))
    got = check(single, [rec(O.GLYPH, 0, 0, *one, 1, white), rec(O.GLYPH, 1, 1, *last, 1, white)], [0, 1, 2])
    assert got[0, 0, 0, 0] == 255 and got[0].sum() == 3 * 255 and got[1, 8, 8, 0] == 255 and got[1].sum() == 3 * 255


@pytest.mark.parametrize("B,W,H", SIZES)
def test_fill_rects(B, W, H):
    rng = np.random.default_rng(7 + W)
    images = background(rng, B, H, W)
    recs = [rec(O.FILL_RECT, 0, 0, W - 1, H - 1, 0, col(rng, 90)),                   # the whole image
            rec(O.FILL_RECT, W - 2, H - 2, 1, 1, 5, col(rng)),                       # reversed corners
            rec(O.FILL_RECT, W // 2, H // 2, W // 2, H // 2, 0, col(rng, 255)),      # one pixel
            rec(O.FILL_RECT, 2 ** 31 - 1, 3, -2 ** 31, 3, 0, col(rng)),              # any int32
            rec(O.FILL_RECT, 31, 31, 32, 32, 0, col(rng, 255)), rec(O.FILL_RECT, -5, -5, -1, H, 0, col(rng, 255))]
    prims, off = spread([recs if b != 1 else recs[:1] for b in range(B)])
    check(images, prims, off)


def label_image(rng, B, H, W):
    ids = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        ids[b, H // 3:H // 3 + 9, max(W // 2 - 6, 0):W // 2 + 7] = 3           # a blob over the seam x = 32 ...
        ids[b, H // 3 + 2:H // 3 + 6, W // 2 + 7:W // 2 + 14] = 200            # ... touched by another label
        ids[b, 0:5, 0:7] = 9                                                  # in the corner: the image border
        ids[b, H - 3:, W // 4:] = 255                                         # along the bottom and right borders
        yy, xx = np.mgrid[0:H, 0:W]
        ids[b][(xx - W + 12) ** 2 + (yy - 14) ** 2 <= 49] = 17                # a disc
        ids[b][rng.random((H, W)) < 0.01] = 77                               # single pixels
    return ids


@pytest.mark.parametrize("B,W,H", SIZES)
@pytest.mark.parametrize("fill,outline", [(True, 0), (False, 1), (False, 4), (True, 1), (True, 4), (False, 0)])
def test_id_layer(B, W, H, fill, outline):
    rng = np.random.default_rng(11 + W)
    images = background(rng, B, H, W)
    ids = label_image(rng, B, H, W)
    palette = np.array([col(rng, 255)] + [col(rng, (255, 120)[k % 2]) for k in range(1, 256)], np.int64)
    none = np.zeros((0, 8), np.int64)
    want = check(images, none, np.zeros(B + 1, np.int32), ids=ids, palette=palette, fill=fill, outline=outline)
    assert np.array_equal(want[ids == 0], images[ids == 0])  # palette entry 0 is never drawn
    if B == 3:  # the id layer, then primitives over it
        prims, off = spread([segments(rng, W, H)[:8], [], [rec(O.FILL_RECT, 0, 0, W, H, 0, col(rng, 60))]])
        check(images, prims, off, ids=ids, palette=palette, fill=fill, outline=outline)


def test_in_place_is_the_same():
    rng = np.random.default_rng(13)
    B, W, H = 3, 70, 45
    images = background(rng, B, H, W)
    ids = label_image(rng, B, H, W)
    palette = np.array([col(rng, 150) for _ in range(256)], np.int64)
    prims, off = spread([segments(rng, W, H), [], segments(rng, W, H)[:5]])
    apart = device(images, prims, off, ids=ids, palette=palette, fill=True, outline=2)
    same = device(images, prims, off, ids=ids, palette=palette, fill=True, outline=2, in_place=True)
    assert np.array_equal(apart, same) and np.array_equal(apart, O.draw_overlay(images, prims, off, ids, palette, True, 2))
    # an odd width and a view that starts at an odd byte: the twelve-byte spans fall back to bytes, to the same result
    odd = background(rng, 1, 9, 37)
    prims, off = spread([segments(rng, 37, 9)[:12]])
    check(odd, prims, off)


def test_argument_errors():
    from pyrapose_amd import _lib, ops
    from pyrapose_amd.runtime import default_context
    ctx = default_context()
    img = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    prims = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    off = torch.zeros((3,), dtype=torch.int32, device="cuda")
    ids = torch.zeros((2, 8, 8), dtype=torch.uint8, device="cuda")
    pal = torch.zeros((256,), dtype=torch.int32, device="cuda")
    for bad in (lambda: ops.draw_overlay(ctx, img.float(), prims, off), lambda: ops.draw_overlay(ctx, img[..., :2], prims, off),
                lambda: ops.draw_overlay(ctx, img, prims[:, :7], off), lambda: ops.draw_overlay(ctx, img, prims, off[:2]),
                lambda: ops.draw_overlay(ctx, img, prims.cpu(), off), lambda: ops.draw_overlay(ctx, img, prims, off, ids=ids),
                lambda: ops.draw_overlay(ctx, img, prims, off, ids=ids[:, :7], palette=pal),
                lambda: ops.draw_overlay(ctx, img, prims, off, ids=ids, palette=pal, outline=5),
                lambda: ops.draw_overlay(ctx, img, prims, off, fill=True), lambda: ops.draw_overlay(ctx, img, prims, off, out=img[:1]),
                lambda: ops.draw_overlay(ctx, img[:1], prims, off[:2], out=img.view(-1)[3:3 + 192].view(1, 8, 8, 3))):
        with pytest.raises(ValueError):
            bad()
    fn, p = _lib.lib.pp_draw_overlay_u8, lambda t: t.data_ptr()
    ok = (ctx.handle, 2, 8, 8, p(img), p(img), p(prims), p(off), 1, p(ids), p(pal), 3, 2)
    assert fn(*ok) == 0

    def with_(**kw):
        names = ("ctx", "B", "H", "W", "images", "out", "prims", "offsets", "n", "ids", "palette", "mode", "width")
        return [kw.get(k, v) for k, v in zip(names, ok)]
    for kw in (dict(B=0), dict(H=0), dict(W=8193), dict(H=8193), dict(n=-1), dict(n=(1 << 24) + 1), dict(images=None), dict(out=None),
               dict(offsets=None), dict(prims=None), dict(palette=None), dict(width=0), dict(width=5), dict(mode=4), dict(mode=-1)):
        assert fn(*with_(**kw)) == -1, kw
    assert fn(*with_(prims=None, n=0)) == 0 and fn(*with_(width=9, mode=1)) == 0 and fn(*with_(ids=None, palette=None, width=0)) == 0
    torch.cuda.synchronize()


def test_draw_batch_end_to_end(tmp_path):
    rng = np.random.default_rng(17)
    W, H = 96, 80
    images = background(rng, 2, H, W)
    K = np.array([[120.0, 0, 48], [0, 120.0, 40], [0, 0, 1]])
    box = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float64) * [0.05, 0.04, 0.03]
    c, s = np.cos(0.5), np.sin(0.5)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    ov = V.OverlayList(2)
    ov.box(0, (10.4, 22.5, 60, 70), (0, 255, 0))
    ov.caption(0, (10.4, 22.5, 60, 70), "obj_01: 0.87")
    ov.box(1, (-5, 30, 99, 85), (255, 0, 255), thickness=3)
    ov.caption(1, (40, 9, 99, 85), "Top (cut)")
    ov.pose(0, R, [0.01, 0.0, 0.2], K, box, (0, 204, 0))
    ov.pose(1, R.T, [0.0, 0.01, 0.02], K, box, (255, 0, 0))  # partly behind the camera
    ov.axes(0, R, [0.01, 0.0, 0.2], K, length=0.06)
    ov.text(1, (3, 60), "k=12 #3", (255, 255, 0), scale=2, halo=(0, 0, 0))
    ov.disc(1, (70.5, 20.2), (13, 243, 207))
    ov.fill_rect(1, (80, 60), (90, 70), (0, 0, 255), alpha=100)
    assert ov.dropped > 0
    prims, off = ov.pack()
    want = O.draw_overlay(images, prims, off)
    got = V.draw_batch(images, ov)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(V.draw_batch(torch.from_numpy(images).cuda(), (prims, off)).cpu().numpy(), want)
    assert not np.array_equal(want[0], images[0]) and not np.array_equal(want[1], images[1])
    # the id layer through draw_batch and draw_mask_output, with the generated palette
    ids = label_image(rng, 2, H, W)
    pal = V.pack_palette(None, 96).view(np.uint32).astype(np.int64)
    assert np.array_equal(V.draw_batch(images, ov, ids, fill_alpha=96, outline=2).cpu().numpy(), O.draw_overlay(images, prims, off, ids, pal, True, 2))
    pal = V.pack_palette(None, 128).view(np.uint32).astype(np.int64)
    none = np.zeros((0, 8), np.int64)
    assert np.array_equal(V.draw_mask_output(images, ids).cpu().numpy(), O.draw_overlay(images, none, [0, 0, 0], ids, pal, True, 1))
    # the reference's functions change the caller's image in place
    image = images[0].copy()
    V.draw_detections(image, np.array([[10.4, 22.5, 60, 70], [1, 1, 5, 5]]), np.array([0.87, 0.2]), np.array([1, 0]), label_to_name=lambda l: "obj_%02d" % l)
    one = V.OverlayList(1)
    V._add_detections(one, 0, np.array([[10.4, 22.5, 60, 70]]), np.array([0.87]), np.array([1]), label_to_name=lambda l: "obj_%02d" % l)
    assert len(one) == 4 + 2 * len("obj_01:0.87") and np.array_equal(image, O.draw_overlay(images[:1], *one.pack())[0])
    # and a picture written and read back
    V.save_image(str(tmp_path / "o.png"), got[0], bgr=True)
    from pyrapose_amd.utils.png_lite import read_png
    assert np.array_equal(read_png(str(tmp_path / "o.png")), want[0][..., ::-1])


def test_save_detection_images_and_pose_draw(tmp_path):
    from pyrapose_amd.utils import eval_pose
    from pyrapose_amd.utils.png_lite import read_png
    rng = np.random.default_rng(19)
    H, W, Cn, N = 120, 160, 3, 300
    raw = background(rng, 2, H, W)
    boxes2d = np.array([[20.0, 30, 90, 100], [60, 20, 150, 110]])

    class Gen(object):
        def size(self): return 2
        def num_classes(self): return Cn
        def has_label(self, l): return True
        def label_to_name(self, l): return "class%d" % int(l)
        def load_image(self, i): return raw[i].copy()
        def preprocess_image(self, x): return x.astype(np.float32)
        def resize_image(self, x): return x, 0.5
        def load_annotations(self, i):
            return {"labels": np.array([float(i)]), "bboxes": boxes2d[i:i + 1], "poses": np.array([[10.0 * i, -5.0, 400.0, 1.0, 0, 0, 0]])}

    class Model(object):
        def predict_on_batch(self, x):
            b = np.tile(boxes2d[None] * 0.5, (1, 2, 1)).astype(np.float32)
            return [b, np.array([[0.93, 0.6, 0.3, 0.01]], np.float32), np.array([[1, 2, 0, 1]])]

    save = str(tmp_path / "det")
    assert V.save_detection_images(Gen(), Model(), save) == 2
    for i in range(2):
        ov = V.OverlayList(1)
        V._add_annotations(ov, 0, Gen().load_annotations(i), label_to_name=Gen().label_to_name)
        V._add_detections(ov, 0, boxes2d[[0, 1, 0]], np.array([0.93, 0.6, 0.3]), np.array([1, 2, 0]), label_to_name=Gen().label_to_name)
        want = O.draw_overlay(raw[i:i + 1], *ov.pack())[0]
        got = read_png(os.path.join(save, "%d.png" % i))
        assert got.shape == (H, W, 3) and np.array_equal(got, want[..., ::-1]) and not np.array_equal(want, raw[i])

    # evaluate_pose_metrics(draw=): the loop's own detections and annotations as wireframes, one PNG per scored image
    K = np.array([[200.0, 0, 80], [0, 200.0, 60], [0, 0, 1]])
    sizes = [(0.08, 0.06, 0.11), (0.064, 0.048, 0.088), (0.088, 0.066, 0.121)]
    from pyrapose_amd.utils.renderer import render
    from tests.render_np import box_mesh
    models = [box_mesh(*s) for s in sizes]
    cuboids = np.stack([m["pts"] for m in models])
    dia = [float(np.linalg.norm(np.asarray(s))) for s in sizes]

    def predict(x):
        i = int(round(float(x[0, 0, 0, 0]))) % 2
        Xc = cuboids[i] + np.array([0.01 * i, -0.005, 0.4])
        uv = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1)
        b3 = rng.uniform(0, 150, (1, N, 16)).astype(np.float32)
        sc = rng.uniform(0, 0.2, (1, N, Cn)).astype(np.float32)
        b3[0, :40] = (uv[None] + rng.normal(scale=0.05, size=(40, 8, 2))).reshape(40, 16)
        sc[0, :40, i] = 0.9
        return [b3, sc, np.zeros((1, 300, Cn), np.float32)]

    class PoseGen(Gen):
        def load_image(self, i):
            im = raw[i].copy()
            im[0, 0, 0] = i  # the image carries its index to `predict`
            return im
        def resize_image(self, x): return x, 1.0

    def load_depth(i):
        mm = dict(models[i], pts=models[i]["pts"] * 1000.0)
        return np.round(render(mm, (W, H), K, np.eye(3), np.array([10.0 * i, -5.0, 400.0]))).astype(np.uint16)

    kw = dict(generator=PoseGen(), predict_on_batch=predict, threeD_boxes=cuboids, models=models, model_diameters=dia, load_depth=load_depth, K=K)
    plain = eval_pose.evaluate_pose_metrics(**kw)
    save = str(tmp_path / "pose")
    drawn = eval_pose.evaluate_pose_metrics(draw=dict(save_path=save, every=1), **kw)
    assert plain["trueDets"].tolist() == drawn["trueDets"].tolist() == [0, 1, 1, 0] and sorted(os.listdir(save)) == ["0.png", "1.png"]
    for i in range(2):
        got = read_png(os.path.join(save, "%d.png" % i))[..., ::-1]
        src = PoseGen().load_image(i)
        gt = V.OverlayList(1)
        gt.pose(0, np.eye(3), np.array([10.0 * i, -5.0, 400.0]) * 0.001, K, cuboids[i], (255, 0, 0))
        only_gt = O.draw_overlay(src[None], *gt.pack())[0]
        changed = (got != src).any(axis=2)
        assert got.shape == src.shape and changed.any() and ((only_gt != src).any(axis=2) <= changed).all()
        assert (got[changed] == (0, 204, 0)).all(axis=1).any() and set(map(tuple, got[changed])) <= {(255, 0, 0), (0, 204, 0)}
    every = str(tmp_path / "every")
    eval_pose.evaluate_add(PoseGen(), predict, cuboids, [m["pts"] for m in models], dia, K, draw=dict(save_path=every, every=2))
    assert os.listdir(every) == ["0.png"]
    with pytest.raises(ValueError):
        eval_pose.evaluate_add(PoseGen(), predict, cuboids, [m["pts"] for m in models], dia, K, draw=dict(every=2))
