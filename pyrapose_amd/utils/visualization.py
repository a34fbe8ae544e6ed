"""Evaluation overlays: the reference's utils/visualization.py (draw_box, draw_boxes, draw_caption, draw_detections,
draw_annotations, same signatures, the image changed in place), the 3-D box wireframes and voted corners of its pose loops
(linemod_eval.py:537-620), draw_axis of its annotation scripts (annotation_scripts/misc.py:8) and the mask head's output as a
picture (linemod_eval.py:343-369), on one device pass: ops.draw_overlay paints an ordered list of primitives and an id layer over
a batch of uint8 images.  This module is the host side: OverlayList turns boxes, text, poses and axes into that list.

The line, text and contour rules are the project's own (include/pyrapose_hip.h): exact integer coverage of thick segments with
round caps, an 8 x 8 bitmap font (utils/font8.py), an inner contour of id regions.  They are not OpenCV's Bresenham or
anti-aliased lines (the reference passes LINE_AA to cv2.rectangle; nothing here is anti-aliased) nor its Hershey text, and OpenCV
is not a dependency: what is drawn and where follows the reference, parity of pixels with cv2 is not pinned.  Colours go by
channel index, as in cv2: on a BGR image (255, 0, 0) is blue.  There is no host fallback: drawing needs the device."""
import os

import numpy as np

from . import font8
from .colors import id_palette, label_color

SEGMENT, GLYPH, FILL_RECT = 0, 1, 2
MAX_COORD = 8192
MAX_THICK = 64
MAX_SCALE = 4
DISC_DIAMETER = 7  # cv2.circle(..., 3, ..., -2): radius 3 around the centre pixel
BOX3D_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (0, 4), (1, 5), (2, 6), (3, 7), (4, 5), (5, 6), (6, 7), (7, 4))  # linemod_eval.py:554-595
AXIS_COLORS = ((255, 0, 0), (0, 255, 0), (0, 0, 255))  # x, y, z as draw_axis has them


def pack_color(color, alpha=255):
    """three channel values 0..255 and an alpha -> c0 | c1 << 8 | c2 << 16 | A << 24 as an int32 value"""
    c = [int(v) for v in np.asarray(color).reshape(-1)]
    alpha = int(alpha)
    if len(c) != 3 or any(v < 0 or v > 255 for v in c) or not 0 <= alpha <= 255:
        raise ValueError("a colour is three values 0..255 and an alpha 0..255, got %r, %r" % (color, alpha))
    v = c[0] | c[1] << 8 | c[2] << 16 | alpha << 24
    return v - (1 << 32) if v >= 1 << 31 else v


def pack_palette(palette=None, alpha=None):
    """None (the generated id palette), [256,3] / [256,4] channel values, or [256] packed colours -> int32 [256] packed;
    alpha other than None replaces every entry's A."""
    p = np.asarray(id_palette() if palette is None else palette)
    if p.shape == (256,):
        out = p.astype(np.int64) & 0xFFFFFFFF
    elif p.shape in ((256, 3), (256, 4)):
        if (p < 0).any() or (p > 255).any():
            raise ValueError("palette: channel values are 0..255")
        p = p.astype(np.int64)
        out = p[:, 0] | p[:, 1] << 8 | p[:, 2] << 16 | (p[:, 3] if p.shape[1] == 4 else 255) << 24
    else:
        raise ValueError("palette: need [256,3], [256,4] or [256] packed colours, got %s" % (p.shape,))
    if alpha is not None:
        if not 0 <= int(alpha) <= 255:
            raise ValueError("palette: alpha 0..255, got %r" % (alpha,))
        out = (out & 0xFFFFFF) | int(alpha) << 24
    return out.astype(np.uint32).view(np.int32)


class OverlayList:
    """The primitives of n_images images, in drawing order per image.  Coordinates are pixels as floats or integers, rounded
    half to even.  (The reference truncates to uint16, which wraps negatives round to 65535: that is not reproduced.)  A
    record with a non-finite coordinate or one beyond +-8192 is left out and counted in .dropped -- a box corner behind the
    camera, for instance."""

    def __init__(self, n_images):
        if int(n_images) < 1:
            raise ValueError("OverlayList: at least one image")
        self._records = [[] for _ in range(int(n_images))]
        self.dropped = 0

    def __len__(self):
        return sum(len(r) for r in self._records)

    def _add(self, i, kind, coords, extra, size, color, alpha):
        c = np.asarray(coords, np.float64).reshape(-1)
        colour = pack_color(color, alpha)
        records = self._records[i]  # (an IndexError for an image the list does not have)
        if not np.isfinite(c).all():
            self.dropped += 1
            return
        c = np.rint(c)
        if (np.abs(c) > MAX_COORD).any():
            self.dropped += 1
            return
        a = [int(v) for v in c] + list(extra)
        records.append((kind, a[0], a[1], a[2], a[3], int(size), colour, 0))

    def segment(self, i, p0, p1, color, thickness=2, alpha=255):
        if not 1 <= int(thickness) <= MAX_THICK:
            raise ValueError("segment: thickness 1..%d, got %r" % (MAX_THICK, thickness))
        self._add(i, SEGMENT, [p0[0], p0[1], p1[0], p1[1]], (), thickness, color, alpha)

    def disc(self, i, center, color, diameter=DISC_DIAMETER, alpha=255):
        """a filled disc: the pixels whose squared distance to the centre is at most diameter^2 / 4"""
        self.segment(i, center, center, color, diameter, alpha)

    def fill_rect(self, i, p0, p1, color, alpha=255):
        self._add(i, FILL_RECT, [p0[0], p0[1], p1[0], p1[1]], (), 0, color, alpha)

    def box(self, i, xyxy, color, thickness=2):
        x1, y1, x2, y2 = (float(v) for v in np.asarray(xyxy).reshape(-1)[:4])
        for p0, p1 in (((x1, y1), (x2, y1)), ((x2, y1), (x2, y2)), ((x2, y2), (x1, y2)), ((x1, y2), (x1, y1))):
            self.segment(i, p0, p1, color, thickness)

    def text(self, i, xy_bottom_left, string, color, scale=1, halo=None, alpha=255):
        """`string` in the 8 x 8 font with its baseline's left end at xy_bottom_left (as cv2.putText places its origin), the
        cells scale x scale pixels; halo: a colour in which every glyph is painted first, grown by one pixel all round"""
        if not 1 <= int(scale) <= MAX_SCALE:
            raise ValueError("text: scale 1..%d, got %r" % (MAX_SCALE, scale))
        scale = int(scale)
        x, y = float(xy_bottom_left[0]), float(xy_bottom_left[1]) - (font8.BASELINE * scale - 1)
        for dilate, col in ((1, halo), (0, color)):
            if col is None:
                continue
            for k, ch in enumerate(str(string)):
                lo, hi = font8.glyph_words(ch)
                if lo == 0 and hi == 0:
                    continue  # a space paints nothing
                self._add(i, GLYPH, [x + k * font8.ADVANCE * scale, y], (lo, hi), scale | dilate << 8, col, alpha)

    def caption(self, i, box, string):
        """the reference's draw_caption: white text with a black rim, its baseline 10 pixels above the box's top-left corner"""
        b = np.asarray(box, np.float64).reshape(-1)
        self.text(i, (b[0], b[1] - 10), string, (255, 255, 255), 1, halo=(0, 0, 0))

    def box3d(self, i, corners16, color, thickness=2):
        """the wireframe of a projected cuboid: corners16 = 8 (x, y) pairs, the twelve edges in the reference's order"""
        c = np.asarray(corners16, np.float64).reshape(8, 2)
        for a, b in BOX3D_EDGES:
            self.segment(i, c[a], c[b], color, thickness)

    def pose(self, i, R, t, K, box8x3, color, thickness=2):
        """the cuboid box8x3 [8,3] under the pose (R, t), projected with K in float64 (toPix_array); a corner at or behind the
        camera plane has no image: its edges are dropped"""
        self.box3d(i, project(box8x3, R, t, K), color, thickness)

    def axes(self, i, R, t, K, length=100.0, thickness=3):
        """the object frame's axes from its origin, `length` model units long, x, y, z in draw_axis's colours"""
        p = project(np.array([[length, 0, 0], [0, length, 0], [0, 0, length], [0, 0, 0]], np.float64), R, t, K)
        for k in range(3):
            self.segment(i, p[3], p[k], AXIS_COLORS[k], thickness)

    def pack(self):
        """-> (prims int32 [n,8], image_offsets int32 [B+1]): grouped by image, in the order they were added within one"""
        offsets = np.zeros(len(self._records) + 1, np.int32)
        offsets[1:] = np.cumsum([len(r) for r in self._records])
        flat = [rec for r in self._records for rec in r]
        return np.asarray(flat, np.int64).reshape(-1, 8).astype(np.int32), offsets


def project(points, R, t, K):
    """points [n,3] under (R, t) through K -> pixel coordinates float64 [n,2]; NaN where z <= 0"""
    X = np.asarray(points, np.float64).reshape(-1, 3) @ np.asarray(R, np.float64).reshape(3, 3).T + np.asarray(t, np.float64).reshape(1, 3)
    K = np.asarray(K, np.float64).reshape(3, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(X[:, 2] > 0, X[:, 2], np.nan)
        return np.stack([X[:, 0] * K[0, 0] / z + K[0, 2], X[:, 1] * K[1, 1] / z + K[1, 2]], axis=1)


def draw_batch(images, overlay, ids=None, palette=None, fill_alpha=None, outline=0, ctx=None):
    """images uint8 [B,H,W,3] (numpy or a device tensor) with overlay (an OverlayList of B images, a (prims, image_offsets)
    pair, or None) and optionally an id layer: ids uint8 [B,H,W], palette as pack_palette takes it (None: the generated one),
    fill_alpha None (no fill) or 0..255 (labelled pixels are filled, every palette entry's alpha replaced by it), outline 0..4
    the width of the regions' inner contour (painted after the fill with the same entry, so it shows denser on it)
    -> a new device uint8 tensor [B,H,W,3]."""
    import torch

    from .. import ops
    from ._host import to_device
    if ctx is None:
        from ..runtime import default_context
        ctx = default_context()
    if not torch.is_tensor(images) and np.asarray(images).dtype != np.uint8:
        raise ValueError("draw_batch: images must be uint8, got %s" % np.asarray(images).dtype)
    img = to_device(images, torch.uint8)
    if img.dim() != 4:
        raise ValueError("draw_batch: images must be [B,H,W,3], got %s" % (list(img.shape),))
    B = int(img.shape[0])
    if overlay is None:
        prims, offsets = np.zeros((0, 8), np.int32), np.zeros(B + 1, np.int32)
    else:
        prims, offsets = overlay.pack() if isinstance(overlay, OverlayList) else overlay
    if len(offsets) != B + 1:
        raise ValueError("draw_batch: the overlay is of %d images, the batch of %d" % (len(offsets) - 1, B))
    pal = None
    if ids is not None:
        ids = to_device(ids, torch.uint8)
        pal = to_device(pack_palette(palette, fill_alpha), torch.int32)
    return ops.draw_overlay(ctx, img, to_device(prims, torch.int32, (-1, 8)), to_device(offsets, torch.int32), ids, pal,
                            fill=fill_alpha is not None and ids is not None, outline=outline if ids is not None else 0)


def _to_numpy(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _in_place(image, overlay):
    """one numpy image [H,W,3] drawn on the device and written back into the caller's array, as cv2's functions do"""
    if not isinstance(image, np.ndarray) or image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("need a uint8 numpy image [H,W,3], got %s" % (getattr(image, "shape", type(image).__name__),))
    image[...] = _to_numpy(draw_batch(np.ascontiguousarray(image)[None], overlay))[0]


def _add_detections(overlay, i, boxes, scores, labels, color=None, label_to_name=None, score_threshold=0.5):
    boxes, scores, labels = np.asarray(boxes), np.asarray(scores), np.asarray(labels)
    for k in np.where(scores > score_threshold)[0]:
        overlay.box(i, boxes[k, :4], color if color is not None else label_color(int(labels[k])))
        name = label_to_name(labels[k]) if label_to_name else labels[k]
        overlay.caption(i, boxes[k, :4], "%s: %.2f" % (name, scores[k]))


def _add_annotations(overlay, i, annotations, color=(0, 255, 0), label_to_name=None):
    if isinstance(annotations, np.ndarray):
        annotations = {"bboxes": annotations[:, :4], "labels": annotations[:, 4]}
    boxes, labels = np.asarray(annotations["bboxes"]).reshape(-1, 4), np.asarray(annotations["labels"]).reshape(-1)
    if len(boxes) != len(labels):
        raise ValueError("annotations: %d boxes, %d labels" % (len(boxes), len(labels)))
    for box, label in zip(boxes, labels):
        overlay.caption(i, box, "%s" % (label_to_name(label) if label_to_name else label))
        overlay.box(i, box, color if color is not None else label_color(int(label)))


def draw_box(image, box, color, thickness=2):
    """a box (x1, y1, x2, y2) on `image`, in place"""
    ov = OverlayList(1)
    ov.box(0, box, color, thickness)
    _in_place(image, ov)


def draw_caption(image, box, caption):
    """`caption` above the box (x1, y1, x2, y2) on `image`, in place"""
    ov = OverlayList(1)
    ov.caption(0, box, caption)
    _in_place(image, ov)


def draw_boxes(image, boxes, color, thickness=2):
    """the boxes [N,4] on `image`, in place"""
    ov = OverlayList(1)
    for b in boxes:
        ov.box(0, b, color, thickness)
    _in_place(image, ov)


def draw_detections(image, boxes, scores, labels, color=None, label_to_name=None, score_threshold=0.5):
    """the detections with scores > score_threshold on `image`, in place: per detection its box (color, or label_color of its
    label) and then its caption 'name: 0.87'"""
    ov = OverlayList(1)
    _add_detections(ov, 0, boxes, scores, labels, color, label_to_name, score_threshold)
    _in_place(image, ov)


def draw_annotations(image, annotations, color=(0, 255, 0), label_to_name=None):
    """annotations ([N,5] rows (x1, y1, x2, y2, label), or a dict of bboxes [N,4] and labels [N]) on `image`, in place: per
    annotation its caption and then its box"""
    ov = OverlayList(1)
    _add_annotations(ov, 0, annotations, color, label_to_name)
    _in_place(image, ov)


def pose_overlay(n_images, detections, annotations, threeD_boxes, K, gt_color=(255, 0, 0), est_color=(0, 204, 0), corners=None):
    """the OverlayList of draw_poses"""
    ov = OverlayList(n_images)
    boxes = np.asarray(threeD_boxes, np.float64)
    for i in range(n_images):
        Ki = np.asarray(K, np.float64)
        Ki = Ki[i] if Ki.ndim == 3 else Ki
        for cls, R, t in annotations[i]:
            ov.pose(i, R, t, Ki, boxes[int(cls)], gt_color)
        for d in detections[i]:
            ov.pose(i, d["R"], d["t"], Ki, boxes[int(d["cls"])], est_color)
        if corners is not None and corners[i] is not None:
            for k, p in enumerate(np.asarray(corners[i], np.float64).reshape(-1, 2)):
                ov.disc(i, p, label_color(k % 8))
    return ov


def draw_poses(images, detections, annotations, threeD_boxes, K, gt_color=(255, 0, 0), est_color=(0, 204, 0), corners=None):
    """Per image the ground-truth and then the estimated cuboid wireframes (linemod_eval.py:537-595): images uint8 [B,H,W,3];
    detections[i]: dicts with cls, R, t (pose_decode.poses_from_outputs); annotations[i]: (cls, R, t) triples; threeD_boxes
    [C,8,3] in the unit of t; K 3x3 or [B,3,3]; corners[i]: None or [n,2] pixel positions drawn as discs of diameter 7, corner
    k of a cuboid in label_color(k % 8) (the voted corners, :613-620) -> device uint8 [B,H,W,3]."""
    return draw_batch(images, pose_overlay(len(images), detections, annotations, threeD_boxes, K, gt_color, est_color, corners))


def draw_mask_output(images, mask_ids, palette=None, fill_alpha=128, outline=1, ctx=None):
    """the id layer alone: mask_ids uint8 [B,H,W] -- the mask head's arg-max image (0 = background, k = class k - 1) or
    scene_gt_info's instance ids -- over images uint8 [B,H,W,3] -> device uint8 [B,H,W,3]"""
    return draw_batch(images, None, mask_ids, palette, fill_alpha, outline, ctx)


def _as_u8(image):
    a = np.asarray(image)
    return a if a.dtype == np.uint8 else np.clip(np.rint(a.astype(np.float64)), 0, 255).astype(np.uint8)


def save_image(path, image, bgr=True):
    """a device or host uint8 image [H,W,3] as a PNG; bgr: the channels are in cv2's order, as the reference's generators load"""
    from .png_lite import write_png
    a = _to_numpy(image)
    write_png(path, np.ascontiguousarray(a[..., ::-1] if bgr else a))


def save_detection_images(generator, model, save_path, score_threshold=0.05, max_detections=100, ctx=None, bgr=True):
    """What the reference's _get_detections does when save_path is set (utils/eval.py:62-108): per image the annotations, then
    the detections above score_threshold (best max_detections first; of these draw_detections shows the ones above its own
    0.5), drawn on the raw image and written to save_path/{i}.png.  One device pass per image.  -> the number of images."""
    import torch
    os.makedirs(save_path, exist_ok=True)
    names = getattr(generator, "label_to_name", None)
    for i in range(generator.size()):
        raw = generator.load_image(i)
        image = generator.preprocess_image(raw.copy())
        image, scale = generator.resize_image(image)
        out = model.predict_on_batch(np.expand_dims(image, axis=0))[:3]
        b, s, l = (np.asarray(o.cpu() if torch.is_tensor(o) else o) for o in out)
        b = b.astype(np.float64) / scale
        idx = np.where(s[0, :] > score_threshold)[0]
        idx = idx[np.argsort(-s[0][idx], kind="stable")[:int(max_detections)]]
        ov = OverlayList(1)
        _add_annotations(ov, 0, generator.load_annotations(i), label_to_name=names)
        _add_detections(ov, 0, b[0, idx, :4], s[0, idx], l[0, idx], label_to_name=names)
        save_image(os.path.join(save_path, "%d.png" % i), draw_batch(_as_u8(raw)[None], ov, ctx=ctx)[0], bgr)
    return generator.size()


def save_pose_image(draw, index, raw_image, dets, anno, threeD_boxes, K, gt_translation_scale):
    """The opt-in `draw` of eval_pose.evaluate_add / evaluate_pose_metrics for one scored image: draw = dict(save_path, every=1,
    bgr=True); the wireframes of every annotation and of every kept detection on the raw image -> save_path/{index}.png, for
    every `every`-th image index.  -> the path written, or None."""
    from .eval_pose import quat2mat
    unknown = set(draw) - {"save_path", "every", "bgr"}
    if unknown or "save_path" not in draw:
        raise ValueError("draw: a dict of save_path and optionally every, bgr; got keys %s" % sorted(draw))
    if index % max(int(draw.get("every", 1)), 1) != 0:
        return None
    os.makedirs(draw["save_path"], exist_ok=True)
    gt = []
    for label, pose in zip(anno["labels"], anno["poses"]):
        pose = np.asarray(pose, np.float64)
        gt.append((int(label), quat2mat(pose[3:]), pose[:3] * gt_translation_scale))
    path = os.path.join(draw["save_path"], "%d.png" % index)
    save_image(path, draw_poses(_as_u8(raw_image)[None], [dets], [gt], threeD_boxes, K)[0], draw.get("bgr", True))
    return path
