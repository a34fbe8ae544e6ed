"""Normal images from depth maps on the device: the reference's get_normal (annotation_scripts/Augmentations.py:394-467, the
same function copied into annotate_val_LineMOD.py, annotate_val_LM_BOP.py, annotate_val_LMO_BOP.py, annotate_val_YCBV_BOP.py,
prepare_val_LineMOD_RGB.py, augment_syn_LineMOD.py and augment_syn_Tless.py), which turns a depth image into the surface-normal
image the reference writes as every sample's _dep.png and also returns the smoothed depth (csrc/depth_image.hip).

What is and is not the reference's:
  * fy is accepted and ignored, as the reference ignores it: both image axes are scaled by 1 / fx.
  * The arithmetic is float64 from the first filter tap on, but the depth goes to the device as float32, the type of the sensor's
    and the renderer's depth: integer depths in millimetres pass unchanged, a float64 depth off the float32 grid is rounded once.
  * The depth must be finite and >= 0.  NaN is not handled.
  * An image whose smoothed depth is all zero, or whose scaled normal image is all zero, makes the reference divide by zero under
    for_vis=False; here its uint8 image and its scaled depth are all zero.
  * The reference's int16 pixel table wraps beyond +-32767 pixels from the principal point; here it does not.
  * The three-value variants of augment_syn_LineMOD.py / augment_syn_Tless.py (cv2.inpaint) are not covered.
Pinned to the reference's own function by tests/golden/depth_normals.npz, at every pixel whose smoothed depth is not exactly 0."""
import numpy as np
import torch

from .. import ops
from ..runtime import default_context
from ._host import per_pose, to_device


def _intrinsics(K_or_intrinsics, n):
    """one 3x3 K, [n,3,3], one (fx, cx, cy) or [n,3] of them -> float64 [n,3] = (fx, cx, cy)"""
    a = np.asarray(K_or_intrinsics.cpu() if torch.is_tensor(K_or_intrinsics) else K_or_intrinsics, np.float64)
    if a.shape in ((3, 3), (n, 3, 3)):  # (with n = 3 a [3,3] is one camera matrix)
        K = per_pose(a, n, (3, 3))
        intr = np.stack([K[:, 0, 0], K[:, 0, 2], K[:, 1, 2]], axis=1)
    elif a.shape in ((3,), (n, 3)):
        intr = np.ascontiguousarray(per_pose(a, n, (3,)))
    else:
        raise ValueError("need K 3x3 or [%d,3,3], or (fx, cx, cy) as [3] or [%d,3], got %s" % (n, n, a.shape))
    if not np.isfinite(intr).all() or (intr[:, 0] == 0).any():
        raise ValueError("intrinsics must be finite with fx != 0")
    return np.ascontiguousarray(intr)


def _depth_stack(depth):
    """[n,H,W] array or tensor -> cuda float32 [n,H,W]"""
    if len(depth.shape) != 3:
        raise ValueError("depth must be [n,H,W], got %s" % (tuple(depth.shape),))
    if depth.shape[0] < 1 or depth.shape[1] < 3 or depth.shape[2] < 3:
        raise ValueError("depth needs n >= 1 images of at least 3 x 3 pixels, got %s" % (tuple(depth.shape),))
    if not torch.is_tensor(depth) and np.asarray(depth).dtype.kind not in "fiu":
        raise ValueError("depth must be a real numeric array, got %s" % np.asarray(depth).dtype)
    return to_device(depth, torch.float32)


def normals_from_depth_batch(depth, K_or_intrinsics, for_vis=True, signed=False, ctx=None):
    """get_normal on n depth images in one call: depth [n,H,W], a numpy array or a tensor (host or device; converted to
    float32), K_or_intrinsics one 3x3 camera matrix or [n,3,3], or (fx, cx, cy) as [3] or [n,3]
    -> (normals, depth_smoothed) as cuda tensors:
       for_vis=True   float64 [n,H,W,3] |unit normal|, float64 [n,H,W] smoothed depth
       for_vis=False  uint8 [n,H,W,3] the reference's _dep image, float64 [n,H,W] smoothed depth / its per-image maximum
    signed=True (for_vis=True only) returns the unit normals before the absolute value instead, zero where the reference's
    are zero.  A 3x3 K with n = 3 is read as one camera matrix, never as three (fx, cx, cy) rows.

    The renderers' depth goes straight in -- render_depth_batch's device tensor, and the scene depth that
    scene_gt.scene_gt_info composes for the scenes scene_gt.render_scenes draws:
        depth = render_depth_batch(model, (640, 480), K, R, t)                        # cuda float32 [n,480,640]
        normals, smoothed = normals_from_depth_batch(depth, K)
        images, info = scene_gt.render_scenes(scenes, models, K, (640, 480))          # the samples' _rgb
        gt = scene_gt.scene_gt_info(scenes, models, K, im_size=(640, 480))            # .depth: float32 [S,480,640], composed
        dep_png, _ = normals_from_depth_batch(gt.depth, K, for_vis=False)             # the samples' _dep: uint8 [S,480,640,3]"""
    if signed and not for_vis:
        raise ValueError("normals_from_depth_batch: signed=True goes with for_vis=True (the uint8 image has no sign)")
    d = _depth_stack(depth)
    intr = to_device(_intrinsics(K_or_intrinsics, int(d.shape[0])))
    first = "signed" if signed else ("normals" if for_vis else "normals_u8")
    out = ops.depth_normals(ctx or default_context(), d, intr, bool(for_vis), (first, "depth"))
    return out[first], out["depth"]


def get_normal(depth_refine, fx=-1, fy=-1, cx=-1, cy=-1, for_vis=True):
    """The reference's get_normal, signature and return pair: depth_refine [H,W] (numpy) -> (normals [H,W,3] float64, smoothed
    depth [H,W] float64) for for_vis=True, (normal image [H,W,3] uint8, smoothed depth / its maximum) for for_vis=False, numpy
    arrays.  fy is ignored, as the reference ignores it.  A drop-in for the annotation scripts' own copy."""
    depth = np.asarray(depth_refine)
    if depth.ndim != 2:
        raise ValueError("get_normal: depth_refine must be [H,W], got %s" % (depth.shape,))
    n, d = normals_from_depth_batch(depth[None], np.array([fx, cx, cy], np.float64), for_vis=for_vis)
    return n[0].cpu().numpy(), d[0].cpu().numpy()
