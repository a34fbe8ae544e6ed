"""float64 numpy restatement of the layered depth-hole filling (csrc/depth_inpaint.hip, pp_depth_inpaint of
include/pyrapose_hip.h), written as plain loops: the same operations in the same order, so that the device's outputs are its
bits.  The method is the project's own (the reference calls cv2.inpaint, which is not a dependency):

  L      the chessboard distance from a pixel to the nearest known (non-hole) pixel of its image, 0 on known pixels.  Pixels
         outside the image do not exist.  An image without a known pixel: L = NO_LAYER everywhere, the image is returned as it
         came, counts (H W, 0, 0).
  fill   v = depth on known pixels, 0 on holes.  For k = 1, 2, ... (k <= max_dist where max_dist > 0) every pixel p with L(p) = k:
         v(p) = (sum w v(q)) / (sum w) over the q of the (2 radius + 1)^2 window inside the image with L(q) < k, in row-major
         order, w = 1.0 / float((dx^2 + dy^2) (1 + L(q))).  Layer k reads layers < k only.
  rescale  ((v - min v) / (max v - min v)) max(depth) per image; unchanged where max v = min v."""
import numpy as np

NO_LAYER = 65535
MAX_RADIUS = 8
OUTPUTS = ("filled_f32", "filled_f64", "layer", "counts")


def holes_of(depth, hole_mask=None):
    return np.asarray(depth) == 0 if hole_mask is None else np.asarray(hole_mask) != 0


def layer_map(hole):
    """hole bool [H,W] -> int64 [H,W]: per row the distance along the row to the nearest known pixel, then per column
    min over y' of max(|y - y'|, that distance in row y').  NO_LAYER everywhere without a known pixel."""
    hole = np.asarray(hole, bool)
    H, W = hole.shape
    if hole.all():
        return np.full((H, W), NO_LAYER, np.int64)
    g = np.full((H, W), NO_LAYER, np.int64)
    for y in range(H):
        last = None
        for x in range(W):  # the nearest known pixel on the left ...
            last = x if not hole[y, x] else last
            if last is not None:
                g[y, x] = x - last
        last = None
        for x in range(W - 1, -1, -1):  # ... and on the right
            last = x if not hole[y, x] else last
            if last is not None:
                g[y, x] = min(g[y, x], last - x)
    L = np.empty((H, W), np.int64)
    rows = np.arange(H)
    for y in range(H):  # (integers: the whole row of pixels at once)
        L[y] = np.maximum(np.abs(rows - y)[:, None], g).min(axis=0)
    return L


def fill(depth, L, radius, max_dist=0):
    """depth [H,W], its layer map -> float64 [H,W], layer by layer"""
    H, W = L.shape
    v = np.where(L == 0, np.asarray(depth, np.float64), 0.0)
    top = int(L.max())
    if max_dist > 0:
        top = min(top, int(max_dist))
    for k in range(1, top + 1):
        new = {}
        for y in range(H):
            for x in range(W):
                if L[y, x] != k:
                    continue
                num, den = 0.0, 0.0
                for qy in range(max(y - radius, 0), min(y + radius, H - 1) + 1):
                    for qx in range(max(x - radius, 0), min(x + radius, W - 1) + 1):
                        lq = int(L[qy, qx])
                        if lq >= k:
                            continue
                        dx, dy = qx - x, qy - y
                        w = 1.0 / float((dx * dx + dy * dy) * (1 + lq))
                        num = num + w * float(v[qy, qx])
                        den = den + w
                new[y, x] = num / den
        for (y, x), val in new.items():  # (layer k read nothing of layer k)
            v[y, x] = val
    return v


def depth_inpaint(depth, hole_mask=None, radius=5, max_dist=0, rescale=False):
    """one image: depth [H,W] (float32 values), hole_mask [H,W] or None -> dict of OUTPUTS"""
    depth = np.ascontiguousarray(depth, np.float32)
    assert depth.ndim == 2 and 1 <= radius <= MAX_RADIUS and max_dist >= 0
    hole = holes_of(depth, hole_mask)
    H, W = depth.shape
    L = layer_map(hole)
    if hole.all():
        v = depth.astype(np.float64)
        counts = (H * W, 0, 0)
    else:
        v = fill(depth, L, int(radius), int(max_dist))
        to_fill = (L >= 1) & ((L <= max_dist) if max_dist > 0 else True)
        counts = (int(hole.sum()), int(to_fill.sum()), int(L.max()))
        if rescale:
            lo, hi, top = v.min(), v.max(), np.float64(depth.max())
            if hi > lo:
                v = ((v - lo) / (hi - lo)) * top
    return {"filled_f32": v.astype(np.float32), "filled_f64": v, "layer": L.astype(np.uint16), "counts": np.array(counts, np.int32)}


def depth_inpaint_batch(depth, hole_mask=None, radius=5, max_dist=0, rescale=False):
    """depth [n,H,W] -> dict of OUTPUTS stacked over the images"""
    each = [depth_inpaint(d, None if hole_mask is None else hole_mask[i], radius, max_dist, rescale) for i, d in enumerate(depth)]
    return {k: np.stack([e[k] for e in each]) for k in OUTPUTS}
