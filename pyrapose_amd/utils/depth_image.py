"""Depth images on the device: the reference's augmentDepth, hole filling and get_normal, the steps between a depth render (or a
sensor's depth frame) and the surface-normal image the reference writes as every sample's _dep.png.

get_normal (annotation_scripts/Augmentations.py:394-467, the same function copied into annotate_val_LineMOD.py,
annotate_val_LM_BOP.py, annotate_val_LMO_BOP.py, annotate_val_YCBV_BOP.py, prepare_val_LineMOD_RGB.py, augment_syn_LineMOD.py
and augment_syn_Tless.py) turns a depth image into the normal image and also returns the smoothed depth (csrc/depth_image.hip).

What is and is not the reference's:
  * fy is accepted and ignored, as the reference ignores it: both image axes are scaled by 1 / fx.
  * The arithmetic is float64 from the first filter tap on, but the depth goes to the device as float32, the type of the sensor's
    and the renderer's depth: integer depths in millimetres pass unchanged, a float64 depth off the float32 grid is rounded once.
  * The depth must be finite and >= 0.  NaN is not handled.
  * An image whose smoothed depth is all zero, or whose scaled normal image is all zero, makes the reference divide by zero under
    for_vis=False; here its uint8 image and its scaled depth are all zero.
  * The reference's int16 pixel table wraps beyond +-32767 pixels from the principal point; here it does not.
  * The three-value variants (annotate_val_LineMOD.py:202-, augment_syn_LineMOD.py:425-, augment_syn_Tless.py:363- and the other
    annotate_* / prepare_* copies), which fill the depth holes first and return the filled depth as a third value, are
    get_normal_inpaint and normals_from_depth_batch(inpaint=...), with the hole filling described below in place of cv2.inpaint.
Pinned to the reference's own function by tests/golden/depth_normals.npz, at every pixel whose smoothed depth is not exactly 0.

augmentDepth (annotation_scripts/Augmentations.py:10-134; augment_syn_LineMOD.py:273-418 and augment_syn_Tless.py:219-356 with
their `method` switch) makes a perfect rendered depth map look like a Kinect frame (csrc/depth_aug.hip): shadow holes from the
opened and median-filtered foreground mask, a half-resolution blur, quantisation to the sensor's depth resolution with
depth-proportional Gaussian noise, and a fractal-simplex-noise warp of pixel positions and depth.  The per-image parameters are
drawn on the host (sample_depth_programs), the pixels are done on the device (augment_depth_batch), bit for bit the numpy
restatement tests/depth_aug_np.py.

What is and is not the reference's there:
  * The simplex noise is the project's own (Gustavson's 3-D simplex noise with an integer hash, csrc/depth_aug.hip):
    pyfastnoisesimd's bits cannot be had, so a seed does not give the reference's field, only one of the same kind.
  * The standard normals of the sensor noise are supplied as a field z (torch.randn on the device by default) instead of being
    drawn inside: the result is q + (q depthNoise) z, what np.random.normal(loc=q, scale=q depthNoise) computes from its normals.
  * The arithmetic after the mask is float64, where cv2 computes float32 images in float32.
  * The image size is taken from the depth map; the fixed 640 x 480 of the T-LESS copy is not assumed.
  * cv2 is restated from its documented rules (morphologyEx's default border, resize INTER_LINEAR, GaussianBlur's
    BORDER_REFLECT_101 and getGaussianKernel) and not pinned; the majority filter is pinned to scipy.signal.medfilt2d and the
    opening to scipy.ndimage's grey erosion and dilation.
  * obj_mask is accepted and ignored, as the reference ignores it.

Hole filling (csrc/depth_inpaint.hip, inpaint_depth_batch): where the reference calls cv2.inpaint(depth, depth == 0, 5,
cv2.INPAINT_NS) and stretches the result back to [0, max depth] (annotate_val_LineMOD.py:206-219), holes (depth = 0: the
shadows augmentDepth cuts, the missing returns of a real sensor) are filled here layer by layer from their rim inwards, bit for
bit the numpy restatement tests/depth_inpaint_np.py.

What is and is not the reference's there:
  * The fill rule is the project's own, not OpenCV's Navier-Stokes fast marching: a hole pixel at chessboard distance k from the
    nearest known pixel is the mean of the pixels of lower layers in its (2 radius + 1)^2 window, weighted by
    1 / (squared distance x (1 + layer)).  Of the same kind (values propagate inwards from the rim), order-free and
    bit-reproducible, which a priority queue is not.  The reference's inPaiDia = 5 is radius = 5.
  * The arithmetic is float64, where cv2.inpaint computes a float32 image in float32.
  * Parity with cv2.inpaint is not pinned: OpenCV is not a dependency of this project or of its tests.  The layer map is pinned
    to scipy.ndimage.distance_transform_cdt(metric='chessboard').
  * An image without a known pixel is returned as it came; where the filled image is constant the rescaling leaves it alone (the
    reference divides by zero).  NaN depth is not handled."""
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


def inpaint_depth_batch(depth, hole_mask=None, radius=5, max_dist=0, rescale=False, ctx=None):
    """Fill the holes of n depth images in one call: depth [n,H,W] (array or tensor, host or device; converted to float32),
    hole_mask [n,H,W] (non-zero = hole; None means depth == 0), radius 1..ops.DEPTH_INPAINT_MAX_RADIUS of the window (the
    reference's inPaiDia), max_dist the deepest layer that is filled, in pixels from the nearest known pixel (0: every hole, however
    large -- an empty background is then filled too; give a limit to keep it empty), rescale=True the reference's stretch of the
    filled image to [0, max depth] -> cuda float32 [n,H,W], ready for normals_from_depth_batch.
    One call takes at most 65535 images and fewer than 2^31 pixels (pp_depth_inpaint's limits; ValueError beyond them) and does
    not split a larger batch itself: the images are independent, so call it on slices of the batch and concatenate."""
    if not 1 <= int(radius) <= ops.DEPTH_INPAINT_MAX_RADIUS or not 0 <= int(max_dist) <= ops.DEPTH_INPAINT_MAX_DIST:
        raise ValueError("inpaint_depth_batch: radius must be 1..%d and max_dist 0..%d, got %r and %r" %
                         (ops.DEPTH_INPAINT_MAX_RADIUS, ops.DEPTH_INPAINT_MAX_DIST, radius, max_dist))
    depth = depth if torch.is_tensor(depth) else np.asarray(depth)  # (a nested list has no shape to check)
    if hole_mask is not None:
        hole_mask = hole_mask if torch.is_tensor(hole_mask) else np.asarray(hole_mask)
        if tuple(hole_mask.shape) != tuple(depth.shape):
            raise ValueError("hole_mask must be %s like depth, got %s" % (tuple(depth.shape), tuple(hole_mask.shape)))
    d = _depth_stack(depth)
    m = None
    if hole_mask is not None:
        m = hole_mask if torch.is_tensor(hole_mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(hole_mask) != 0))
        m = (m.to(device="cuda") != 0).to(torch.uint8).contiguous()
    return ops.depth_inpaint(ctx or default_context(), d, m, int(radius), int(max_dist), bool(rescale), ("filled_f32",))["filled_f32"]


def normals_from_depth_batch(depth, K_or_intrinsics, for_vis=True, signed=False, ctx=None, inpaint=None):
    """get_normal on n depth images in one call: depth [n,H,W], a numpy array or a tensor (host or device; converted to
    float32), K_or_intrinsics one 3x3 camera matrix or [n,3,3], or (fx, cx, cy) as [3] or [n,3]
    -> (normals, depth_smoothed) as cuda tensors:
       for_vis=True   float64 [n,H,W,3] |unit normal|, float64 [n,H,W] smoothed depth
       for_vis=False  uint8 [n,H,W,3] the reference's _dep image, float64 [n,H,W] smoothed depth / its per-image maximum
    signed=True (for_vis=True only) returns the unit normals before the absolute value instead, zero where the reference's
    are zero.  A 3x3 K with n = 3 is read as one camera matrix, never as three (fx, cx, cy) rows.
    inpaint=dict(radius=5, ...) (the keywords of inpaint_depth_batch; an empty dict for its defaults) fills the depth holes first
    and returns (normals, depth_smoothed, filled depth as cuda float32 [n,H,W]), the three values of the reference's later
    get_normal; inpaint=None is the two-value call, untouched.

    The renderers' depth goes straight in -- render_depth_batch's device tensor, and the scene depth that
    scene_gt.scene_gt_info composes for the scenes scene_gt.render_scenes draws:
        depth = render_depth_batch(model, (640, 480), K, R, t)                        # cuda float32 [n,480,640]
        normals, smoothed = normals_from_depth_batch(depth, K)
        images, info = scene_gt.render_scenes(scenes, models, K, (640, 480))          # the samples' _rgb
        gt = scene_gt.scene_gt_info(scenes, models, K, im_size=(640, 480))            # .depth: float32 [S,480,640], composed
        programs = sample_depth_programs(np.random.default_rng(0), len(scenes))       # host: one parameter row per image
        noisy = augment_depth_batch(gt.depth, None, programs)                         # the Kinect look: float32 [S,480,640]
        filled = inpaint_depth_batch(noisy, radius=5, rescale=True)                   # its shadow holes closed: float32 [S,480,640]
        dep_png, _ = normals_from_depth_batch(filled, K, for_vis=False)               # the samples' _dep: uint8 [S,480,640,3]
    (the last two lines in one: normals_from_depth_batch(noisy, K, for_vis=False, inpaint=dict(radius=5, rescale=True)))"""
    if signed and not for_vis:
        raise ValueError("normals_from_depth_batch: signed=True goes with for_vis=True (the uint8 image has no sign)")
    if inpaint is not None:
        filled = inpaint_depth_batch(depth, ctx=ctx, **dict(inpaint))
        return normals_from_depth_batch(filled, K_or_intrinsics, for_vis, signed, ctx) + (filled,)
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


def get_normal_inpaint(depth_refine, fx=-1, fy=-1, cx=-1, cy=-1, for_vis=True):
    """The reference's later get_normal (annotate_val_LineMOD.py:202-, augment_syn_LineMOD.py:425-), signature and return triple:
    the holes (depth == 0) filled with radius 5 and the filled image stretched to [0, max depth], then get_normal on it
    -> (normals, smoothed depth, filled depth [H,W] float32) as numpy arrays; the first two as get_normal returns them."""
    depth = np.asarray(depth_refine)
    if depth.ndim != 2:
        raise ValueError("get_normal_inpaint: depth_refine must be [H,W], got %s" % (depth.shape,))
    n, d, filled = normals_from_depth_batch(depth[None], np.array([fx, cx, cy], np.float64), for_vis=for_vis,
                                            inpaint=dict(radius=5, rescale=True))
    return n[0].cpu().numpy(), d[0].cpu().numpy(), filled[0].cpu().numpy()


def _program_row(k_open, k_med, k_blur, blur_sigma, depth_noise, method, freq, octaves, w_xy, w_z, seed):
    """one parameter row of pp_depth_augment with the reference's constants: lacunarity 2.1, gain 0.45, the jitter ranges
    (0.001, 0.01), (0.001, 0.01) and (0.01, 0.1); method 0 | 1 | 2 = both stages | sensor only | simplex only"""
    if int(method) not in (0, 1, 2):
        raise ValueError("method must be 0 (both stages), 1 (sensor only) or 2 (simplex only), got %r" % (method,))
    row = np.zeros(ops.DEPTH_AUG_P, np.float64)
    at = {k: v[0] for k, v in ops.DEPTH_AUG_PARAMS.items()}
    row[at["k_open"]], row[at["k_med"]], row[at["k_blur"]] = int(k_open), int(k_med), int(k_blur)
    row[at["blur_taps"]:at["blur_taps"] + int(k_blur)] = ops.depth_aug_blur_taps(k_blur, blur_sigma)
    row[at["depth_noise"]] = depth_noise
    row[at["sensor"]], row[at["simplex"]] = ((1, 1), (1, 0), (0, 1))[int(method)]
    row[at["freq"]], row[at["octaves"]], row[at["lacunarity"]], row[at["gain"]] = freq, int(octaves), 2.1, 0.45
    row[at["w_xy"]], row[at["w_z"]] = w_xy, w_z
    row[at["jitter_lo"]:at["jitter_lo"] + 3] = 0.001, 0.001, 0.01
    row[at["jitter_hi"]:at["jitter_hi"] + 3] = 0.01, 0.01, 0.1
    row[at["seed"]] = int(seed)
    return row


def sample_depth_programs(rng, n, method=0, shadowClK=None, shadowMK=None, blurK=None, blurS=None, depthNoise=None):
    """The reference's draws for n images, on the host, from a numpy Generator -> float64 [n, ops.DEPTH_AUG_P], one parameter
    row of pp_depth_augment per image: the three kernel sizes uniformly from {3, 5, 7}, blurS ~ U(0, 1.5), depthNoise ~
    U(0.002, 0.004), a seed below 2^31, freq ~ U(0.05, 0.2), octaves from {4, 8}, Wxy from {1..4} ({2..4} for method 2),
    Wz ~ U(1e-4, 4e-3).  method 0 | 1 | 2 = both stages | sensor only | simplex only.  A value given for one of the five
    arguments the reference's augment_syn_* scripts draw themselves replaces that draw (the draw is still made, so the other
    values do not depend on it)."""
    rows = []
    for _ in range(int(n)):
        k_open, k_med, k_blur = (int(v) for v in rng.choice([3, 5, 7], size=3))
        sigma, noise = rng.uniform(0.0, 1.5), rng.uniform(0.002, 0.004)
        seed = int(rng.integers(0, 2 ** 31))
        freq = rng.uniform(0.05, 0.2)
        octaves = int(rng.choice([4, 8]))
        w_xy = int(rng.integers(2, 5)) if int(method) == 2 else int(rng.integers(1, 5))
        w_z = rng.uniform(0.0001, 0.004)
        rows.append(_program_row(k_open if shadowClK is None else shadowClK, k_med if shadowMK is None else shadowMK,
                                 k_blur if blurK is None else blurK, sigma if blurS is None else blurS,
                                 noise if depthNoise is None else depthNoise, method, freq, octaves, float(w_xy), w_z, seed))
    return np.stack(rows) if rows else np.zeros((0, ops.DEPTH_AUG_P), np.float64)


def augment_depth_batch(depth, mask, programs, z=None, generator=None, ctx=None):
    """augmentDepth on n depth images in one call: depth [n,H,W] (array or tensor, host or device; converted to float32,
    millimetres), mask [n,H,W] (non-zero = foreground; None means depth > 0), programs float64 [n, ops.DEPTH_AUG_P] from
    sample_depth_programs, z [n,h2,w2] the standard normals of the sensor noise (h2, w2 = ops.depth_aug_half_size of H, W;
    None: torch.randn on the device, from `generator` when given; not drawn when no image has the sensor stage)
    -> cuda float32 [n,H,W], ready for normals_from_depth_batch."""
    if len(depth.shape) != 3 or depth.shape[0] < 1 or depth.shape[1] < 8 or depth.shape[2] < 8:
        raise ValueError("depth must be [n,H,W] with n >= 1 images of at least 8 x 8 pixels, got %s" % (tuple(depth.shape),))
    d = _depth_stack(depth)
    n, H, W = (int(v) for v in d.shape)
    if mask is None:
        m = (d > 0).to(torch.uint8)
    else:
        if tuple(mask.shape) != (n, H, W):
            raise ValueError("mask must be %s like depth, got %s" % ((n, H, W), tuple(mask.shape)))
        m = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0))
        m = (m.to(device="cuda") != 0).to(torch.uint8).contiguous()
    programs = np.ascontiguousarray(programs, np.float64)
    if programs.shape != (n, ops.DEPTH_AUG_P):
        raise ValueError("programs must be [%d,%d] (sample_depth_programs), got %s" % (n, ops.DEPTH_AUG_P, programs.shape))
    h2, w2 = ops.depth_aug_half_size(H), ops.depth_aug_half_size(W)
    if z is not None:
        if tuple(z.shape) != (n, h2, w2):
            raise ValueError("z must be %s, got %s" % ((n, h2, w2), tuple(z.shape)))
        z = to_device(z, torch.float32)
    elif programs[:, ops.DEPTH_AUG_PARAMS["sensor"][0]].any():
        z = torch.randn((n, h2, w2), dtype=torch.float32, device="cuda", generator=generator)
    return ops.depth_augment(ctx or default_context(), d, m, programs, z, ("depth_f32",))["depth_f32"]


def augmentDepth(depth, obj_mask, mask_ori, shadowClK=None, shadowMK=None, blurK=None, blurS=None, depthNoise=None, method=0, rng=None):
    """The reference's augmentDepth, both signatures: (depth, obj_mask, mask_ori) of Augmentations.py, which draws every
    parameter itself, and (depth, obj_mask, mask_ori, shadowClK, shadowMK, blurK, blurS, depthNoise, method) of
    augment_syn_LineMOD.py / augment_syn_Tless.py, which is given five of them and the method switch.  depth [H,W] (numpy,
    millimetres), mask_ori [H,W] (> 0 = foreground), obj_mask ignored as in the reference -> the augmented depth [H,W] float64
    (numpy).  The remaining parameters are drawn from `rng` (a numpy Generator; a fresh one by default).  A drop-in for the
    annotation scripts' own copy."""
    depth = np.asarray(depth)
    if depth.ndim != 2:
        raise ValueError("augmentDepth: depth must be [H,W], got %s" % (depth.shape,))
    rng = np.random.default_rng() if rng is None else rng
    programs = sample_depth_programs(rng, 1, method, shadowClK, shadowMK, blurK, blurS, depthNoise)
    h2, w2 = ops.depth_aug_half_size(depth.shape[0]), ops.depth_aug_half_size(depth.shape[1])
    z = rng.standard_normal((1, h2, w2), dtype=np.float32)
    out = augment_depth_batch(depth[None], (np.asarray(mask_ori) > 0)[None], programs, z=z)
    return out[0].cpu().numpy().astype(np.float64)
