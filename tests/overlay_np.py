"""numpy restatement of pp_draw_overlay_u8 (csrc/overlay.hip), written from the rule in include/pyrapose_hip.h: the records are
painted one by one, each over its own bounding box, pixel tests in Python integers / int64 arrays; the id layer by a direct
search of every pixel's neighbourhood.  No tiles, no chunks, no compaction: what the device's output is held to, byte for byte."""
import numpy as np

SEGMENT, GLYPH, FILL_RECT = 0, 1, 2
MAX_SIDE = 8192
MAX_COORD = 8192
MAX_THICK = 64
MAX_SCALE = 4
MAX_DILATE = 2
MAX_OUTLINE = 4


def pack_color(color, alpha=255):
    c0, c1, c2 = (int(v) for v in color)
    v = c0 | c1 << 8 | c2 << 16 | int(alpha) << 24
    return v - (1 << 32) if v >= 1 << 31 else v  # as int32


def paint(pixels, colour):
    """pixels uint8 [..., 3] painted with one packed colour -> uint8 [..., 3]"""
    colour = int(colour) & 0xFFFFFFFF
    A = colour >> 24
    c = np.array([(colour >> (8 * k)) & 255 for k in range(3)], np.int64)
    return ((A * c + (255 - A) * pixels.astype(np.int64) + 127) // 255).astype(np.uint8)


def record_valid(rec):
    kind, a0, a1, a2, a3, size = (int(v) for v in rec[:6])
    if kind == SEGMENT:
        return 1 <= size <= MAX_THICK and all(abs(v) <= MAX_COORD for v in (a0, a1, a2, a3))
    if kind == GLYPH:
        scale, dilate = size & 255, (size >> 8) & 255
        return (size >> 16) == 0 and 1 <= scale <= MAX_SCALE and dilate <= MAX_DILATE and abs(a0) <= MAX_COORD and abs(a1) <= MAX_COORD
    return kind == FILL_RECT


def record_box(rec):
    """inclusive (x0, y0, x1, y1) that holds every pixel the record can cover"""
    kind, a0, a1, a2, a3, size = (int(v) for v in rec[:6])
    if kind == SEGMENT:
        g = (size + 1) // 2
        return min(a0, a2) - g, min(a1, a3) - g, max(a0, a2) + g, max(a1, a3) + g
    if kind == GLYPH:
        scale, dilate = size & 255, (size >> 8) & 255
        return a0 - dilate, a1 - dilate, a0 + 8 * scale - 1 + dilate, a1 + 8 * scale - 1 + dilate
    return min(a0, a2), min(a1, a3), max(a0, a2), max(a1, a3)


def segment_cover(x, y, x0, y0, x1, y1, t):
    """int64 arrays x, y -> bool: 4 dist^2(pixel, segment) <= t^2"""
    dx, dy = x1 - x0, y1 - y0
    wx, wy = x - x0, y - y0
    L2 = dx * dx + dy * dy
    s = wx * dx + wy * dy
    cross = dx * wy - dy * wx
    head = 4 * (wx * wx + wy * wy) <= t * t
    tail = 4 * ((x - x1) ** 2 + (y - y1) ** 2) <= t * t
    body = 4 * cross * cross <= t * t * L2
    return np.where(s <= 0, head, np.where(s >= L2, tail, body))


def glyph_cover(x, y, x0, y0, bits, scale, dilate):
    cover = np.zeros(x.shape, bool)
    for oy in range(-dilate, dilate + 1):
        for ox in range(-dilate, dilate + 1):
            col, row = (x + ox - x0) // scale, (y + oy - y0) // scale  # floor division
            inside = (col >= 0) & (col < 8) & (row >= 0) & (row < 8)
            bit = 8 * np.clip(row, 0, 7) + np.clip(col, 0, 7)
            cover |= inside & (((bits >> bit.astype(np.uint64)) & np.uint64(1)) != 0)
    return cover


def cover(rec, x, y):
    """does record `rec` cover the pixels (x, y) (int64 arrays)?  An invalid record covers nothing."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    if not record_valid(rec):
        return np.zeros(x.shape, bool)
    kind, a0, a1, a2, a3, size = (int(v) for v in rec[:6])
    if kind == SEGMENT:
        return segment_cover(x, y, a0, a1, a2, a3, size)
    if kind == GLYPH:
        bits = np.uint64((a2 & 0xFFFFFFFF) | (a3 & 0xFFFFFFFF) << 32)
        return glyph_cover(x, y, a0, a1, bits, size & 255, (size >> 8) & 255)
    bx0, by0, bx1, by1 = record_box(rec)
    return (x >= bx0) & (x <= bx1) & (y >= by0) & (y <= by1)


def cover_image(rec, H, W):
    """bool [H,W]: the pixels of an H x W image that `rec` covers, tested over its bounding box only"""
    out = np.zeros((H, W), bool)
    if not record_valid(rec):
        return out
    bx0, by0, bx1, by1 = record_box(rec)
    bx0, by0, bx1, by1 = max(bx0, 0), max(by0, 0), min(bx1, W - 1), min(by1, H - 1)
    if bx0 > bx1 or by0 > by1:
        return out
    y, x = np.mgrid[by0:by1 + 1, bx0:bx1 + 1]
    out[by0:by1 + 1, bx0:bx1 + 1] = cover(rec, x, y)
    return out


def outline_mask(ids, width):
    """bool [H,W]: labelled pixels with a pixel of another id (0 included) within chessboard distance width, inside the image"""
    H, W = ids.shape
    edge = np.zeros((H, W), bool)
    for dy in range(-width, width + 1):
        for dx in range(-width, width + 1):
            ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if ys >= ye or xs >= xe:
                continue
            edge[ys:ye, xs:xe] |= ids[ys:ye, xs:xe] != ids[ys + dy:ye + dy, xs + dx:xe + dx]
    return edge & (ids != 0)


def draw_image(image, prims, ids=None, palette=None, fill=False, outline=0):
    """one image uint8 [H,W,3] and its own records int32 [n,8] -> a new uint8 [H,W,3]"""
    out = np.array(image, np.uint8, copy=True)
    H, W = out.shape[:2]
    if ids is not None and (fill or outline):
        for passes, mask in ((fill, ids != 0), (outline, outline_mask(ids, outline) if outline else None)):
            if not passes:
                continue
            for L in np.unique(ids[mask]):
                m = mask & (ids == L)
                out[m] = paint(out[m], palette[int(L)])
    for rec in np.asarray(prims, np.int64).reshape(-1, 8):
        m = cover_image(rec, H, W)
        out[m] = paint(out[m], rec[6])
    return out


def draw_overlay(images, prims, image_offsets, ids=None, palette=None, fill=False, outline=0):
    """the batch: images uint8 [B,H,W,3], prims int32 [n,8], image_offsets [B+1] -> uint8 [B,H,W,3]"""
    images = np.asarray(images, np.uint8)
    prims = np.asarray(prims, np.int64).reshape(-1, 8)
    n = len(prims)
    out = np.empty_like(images)
    for b in range(len(images)):
        begin = min(max(int(image_offsets[b]), 0), n)
        end = min(max(int(image_offsets[b + 1]), begin), n)
        out[b] = draw_image(images[b], prims[begin:end], None if ids is None else ids[b], palette, fill, outline)
    return out
