"""Scene ground truth from meshes and poses on the device: what the training path reads besides the image and what the
reference takes from disk -- annotation_scripts/annotate_BOP.py:363-378, 420, 461-471 reads mask_visib/*.png and
scene_gt_info.json, which bop_toolkit's calc_gt_masks / calc_gt_info wrote beforehand with an OpenGL renderer.  Here every
mesh is rendered once at all its poses (utils.renderer.render_depth_batch) and one pass over the renders (pp_scene_gt_info,
csrc/scene_gt.hip) gives the instance-id image, both masks, both boxes, the three pixel counts and the visible fraction of every
instance, against the sensor depth or, for a synthetic scene, against the depth composed from the instances themselves.
Parity with bop_toolkit is unpinned: its definitions are restated (tests/scene_gt_np.py)."""
import collections

import numpy as np
import torch

from .. import ops
from ..runtime import default_context
from ._host import k4, per_pose, to_device

EXTENTS = ("image", "bop")
SceneGroundTruth = collections.namedtuple("SceneGroundTruth", "info id_images depth mask_full mask_visib")
InstancePlan = collections.namedtuple("InstancePlan", "scene_offsets scene_of obj_ids R t groups order")


def plan_instances(scenes):
    """scenes: a list (one entry per image) of lists of instances, each a dict with 'obj_id' and the pose as 'R' / 't' or BOP's
    'cam_R_m2c' / 'cam_t_m2c' -> InstancePlan: the instances flattened in scene order (scene_offsets int32 [S+1], scene_of
    [n], obj_ids [n], R [n,3,3], t [n,3]); groups: obj_id -> the flat indices of its instances, in the order the ids first
    appear; order int64 [n]: with the groups rendered one after the other and concatenated, row order[i] is instance i."""
    offsets, scene_of, obj_ids, Rs, ts = [0], [], [], [], []
    for s, instances in enumerate(scenes):
        for inst in instances:
            try:
                obj_id = inst["obj_id"]
                R = inst["R"] if "R" in inst else inst["cam_R_m2c"]
                t = inst["t"] if "t" in inst else inst["cam_t_m2c"]
            except (KeyError, TypeError):
                raise ValueError("scene_gt_info: an instance is a dict with 'obj_id', 'R' and 't' (or 'cam_R_m2c' / 'cam_t_m2c')")
            R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
            if R.size != 9 or t.size != 3:
                raise ValueError("scene_gt_info: scene %d: R must hold 9 values and t 3" % s)
            scene_of.append(s)
            obj_ids.append(obj_id)
            Rs.append(R.reshape(3, 3))
            ts.append(t.reshape(3))
        if len(scene_of) - offsets[-1] > ops.SCENE_GT_MAX_INSTANCES:
            raise ValueError("scene_gt_info: scene %d has %d instances, the uint8 id image holds %d" %
                             (s, len(scene_of) - offsets[-1], ops.SCENE_GT_MAX_INSTANCES))
        offsets.append(len(scene_of))
    groups = collections.OrderedDict()
    for i, obj_id in enumerate(obj_ids):
        groups.setdefault(obj_id, []).append(i)
    order = np.empty(len(obj_ids), np.int64)
    if obj_ids:
        order[np.concatenate(list(groups.values()))] = np.arange(len(obj_ids))
    return InstancePlan(np.asarray(offsets, np.int32), np.asarray(scene_of, np.int64), obj_ids, np.reshape(Rs, (-1, 3, 3)),
                        np.reshape(ts, (-1, 3)), groups, order)


def _scene_depth(depth, n_scene, im_size):
    """depth None, [h,w] or [n_scene,h,w] and im_size (w, h) or None -> (depth as float32 or None, w, h)"""
    if depth is not None:
        if not torch.is_tensor(depth):
            depth = np.asarray(depth)
            if depth.dtype != np.float32:
                depth = depth.astype(np.float32)  # (uint16 sensor depth converts exactly)
        if depth.ndim not in (2, 3) or (depth.ndim == 3 and depth.shape[0] != n_scene):
            raise ValueError("scene_gt_info: depth must be [h,w] or [%d,h,w], got %s" % (n_scene, tuple(depth.shape)))
        h, w = (int(v) for v in depth.shape[-2:])
        if im_size is not None and tuple(int(v) for v in im_size) != (w, h):
            raise ValueError("scene_gt_info: im_size %s is not the size of depth (%d, %d)" % (tuple(im_size), w, h))
        return depth, w, h
    if im_size is None:
        raise ValueError("scene_gt_info: without depth, give im_size = (w, h)")
    w, h = (int(v) for v in im_size)
    if w < 1 or h < 1:
        raise ValueError("scene_gt_info: im_size must be positive, got %s" % (tuple(im_size),))
    return None, w, h


def _info(plan, out):
    """the counts and boxes of ops.scene_gt_info -> per scene a list of dicts with the keys of BOP's scene_gt_info.json"""
    counts, box_obj, box_visib = (a.cpu().numpy() for a in (out.px_count, out.bbox_obj, out.bbox_visib))
    info = []
    for s in range(len(plan.scene_offsets) - 1):
        rows = []
        for i in range(plan.scene_offsets[s], plan.scene_offsets[s + 1]):
            n_all, n_valid, n_visib = (int(v) for v in counts[i])
            rows.append({"bbox_obj": [int(v) for v in box_obj[i]], "bbox_visib": [int(v) for v in box_visib[i]], "px_count_all": n_all,
                         "px_count_valid": n_valid, "px_count_visib": n_visib, "visib_fract": n_visib / float(n_all) if n_all > 0 else 0.0})
        info.append(rows)
    return info


def scene_gt_info(scenes, models, K, depth=None, im_size=None, delta=15.0, extent="image", masks=False, clip_near=100,
                  clip_far=10000):
    """Ground truth of S images from the meshes and poses of their instances.  scenes: see plan_instances; models: obj_id ->
    model dict ('pts', 'faces': utils.ply_loader); K 3x3 or [S,3,3]; depth: the sensor depth [h,w] (shared) or [S,h,w] in the
    unit of the poses, None for a synthetic scene (the scene depth is then composed from the instances and returned; im_size =
    (w, h) is needed); delta: BOP's visibility tolerance in that unit.  extent 'image': the instances are rendered at the image
    size, so px_count_all and bbox_obj cover what lies inside the image.  extent 'bop': they are rendered on a 3 x 3 canvas
    with the principal point moved by (w, h), as calc_gt_info does, so px_count_all and bbox_obj include what falls outside
    the image (bbox_obj may be negative); this renders and reads nine times the pixels.
    -> SceneGroundTruth(info, id_images, depth, mask_full, mask_visib): info: per scene a list of dicts with the keys of BOP's
    scene_gt_info.json (bbox_obj, bbox_visib as [x, y, w, h], px_count_all, px_count_valid, px_count_visib, visib_fract =
    visib / all, 0.0 when all is 0); id_images uint8 [S,h,w] (1-based index within the scene of the last instance visible at
    the pixel, 0 = none); depth float32 [S,h,w], the composed scene depth (None when depth was given); mask_full / mask_visib:
    with masks, per scene a uint8 array [n_s,h,w] of 0 / 255 (None otherwise)."""
    from .renderer import render_depth_batch
    if extent not in EXTENTS:
        raise ValueError("scene_gt_info: unknown extent %r (image | bop)" % (extent,))
    if not float(delta) >= 0.0:
        raise ValueError("scene_gt_info: delta must not be negative, got %r" % (delta,))
    scenes = list(scenes)
    S = len(scenes)
    if S < 1:
        raise ValueError("scene_gt_info: no scenes")
    plan = plan_instances(scenes)
    missing = [o for o in plan.groups if o not in models]
    if missing:
        raise ValueError("scene_gt_info: no model for obj_id %s" % ", ".join(repr(o) for o in missing))
    depth, w, h = _scene_depth(depth, S, im_size)
    Ks = per_pose(K, S, (3, 3))
    n = len(plan.obj_ids)
    empty = np.zeros((S, h, w), np.uint8)
    if n == 0:  # nothing to render: empty id images, and an empty synthetic depth
        return SceneGroundTruth([[] for _ in scenes], empty, None if depth is not None else empty.astype(np.float32),
                                [empty[:0]] * S if masks else None, [empty[:0]] * S if masks else None)
    ctx = default_context()
    K_inst = Ks[plan.scene_of]
    if extent == "bop":
        window, canvas, K_render = (w, h, w, h), (3 * w, 3 * h), K_inst.copy()
        K_render[:, 0, 2] += w
        K_render[:, 1, 2] += h
    else:
        window, canvas, K_render = None, (w, h), K_inst
    renders = [render_depth_batch(models[o], canvas, K_render[idx], plan.R[idx], plan.t[idx], clip_near, clip_far, ctx)
               for o, idx in plan.groups.items()]
    stack = torch.cat(renders)[torch.from_numpy(plan.order).to(renders[0].device)] if len(renders) > 1 else renders[0]
    out = ops.scene_gt_info(ctx, stack, plan.scene_offsets, to_device(k4(K_inst, n)), None if depth is None else to_device(depth, torch.float32),
                            delta, window, masks)
    info = _info(plan, out)
    per_scene = lambda m: [m[plan.scene_offsets[s]:plan.scene_offsets[s + 1]] for s in range(S)]
    return SceneGroundTruth(info, out.id_image.cpu().numpy(), None if out.scene_depth is None else out.scene_depth.cpu().numpy(),
                            per_scene(out.mask_full.cpu().numpy()) if masks else None,
                            per_scene(out.mask_visib.cpu().numpy()) if masks else None)


def _background(background, S, h, w):
    """None, three values 0 ... 255 or uint8 images [h,w,3] / [S,h,w,3] (RGB) -> what ops.scene_compose takes"""
    if background is None:
        return (0, 0, 0)
    if not torch.is_tensor(background):
        background = np.asarray(background)
        if background.ndim == 1:
            return background
        if background.dtype != np.uint8:
            raise ValueError("render_scenes: a background image must be uint8, got %s" % background.dtype)
    if background.ndim == 3:
        background = background[None].expand(S, -1, -1, -1) if torch.is_tensor(background) else np.broadcast_to(background, (S,) + background.shape)
    if tuple(background.shape) != (S, h, w, 3):
        raise ValueError("render_scenes: background must be [%d,%d,3] or [%d,%d,%d,3], got %s" % (h, w, S, h, w, tuple(background.shape)))
    return to_device(background, torch.uint8)


def render_scenes(scenes, models, K, im_size, background=None, channel_order="bgr", **shading):
    """Synthetic images of S scenes from the meshes and poses of their instances, with their ground truth.  scenes, models, K:
    see scene_gt_info (models also carry 'colors' / 'normals' or, textured, 'texture' / 'texture_uv', each model its own, and
    a scene may mix both kinds: utils.renderer.render_rgbd_batch); im_size (w, h); background:
    None (black), three values 0 ... 255, or uint8 images [h,w,3] (shared) / [S,h,w,3], RGB, host or device; channel_order of
    the images 'bgr' (what engine.forward_u8 and the device augmentation take) or 'rgb'; **shading: shading, ambient_weight,
    light_cam_pos, surf_color, tex_filter, tex_wrap of render_rgbd_batch, and delta, clip_near, clip_far of scene_gt_info.  Every mesh is rendered
    once at all its poses (colour and depth in one pass), scene_gt_info(extent='image') runs on the depth renders against the
    depth composed from them, and its id image selects each pixel's instance colour (pp_scene_compose_u8).
    -> (images uint8 [S,h,w,3] on the device, info: as scene_gt_info's)."""
    from .renderer import render_rgbd_batch
    if channel_order not in ops.CHANNEL_ORDERS:
        raise ValueError("render_scenes: unknown channel order %r (rgb | bgr)" % (channel_order,))
    delta, clip_near, clip_far = shading.pop("delta", 15.0), shading.pop("clip_near", 100), shading.pop("clip_far", 10000)
    unknown = sorted(set(shading) - {"shading", "ambient_weight", "light_cam_pos", "surf_color", "tex_filter", "tex_wrap"})
    if unknown:
        raise TypeError("render_scenes: unexpected argument %s" % ", ".join(unknown))
    if not float(delta) >= 0.0:
        raise ValueError("render_scenes: delta must not be negative, got %r" % (delta,))
    scenes = list(scenes)
    S = len(scenes)
    if S < 1:
        raise ValueError("render_scenes: no scenes")
    plan = plan_instances(scenes)
    missing = [o for o in plan.groups if o not in models]
    if missing:
        raise ValueError("render_scenes: no model for obj_id %s" % ", ".join(repr(o) for o in missing))
    _, w, h = _scene_depth(None, S, im_size)
    Ks = per_pose(K, S, (3, 3))
    background = _background(background, S, h, w)
    n = len(plan.obj_ids)
    ctx = default_context()
    if n == 0:  # nothing to render: the background alone (one empty stand-in instance, no id refers to it)
        ids, colors = torch.zeros((S, h, w), dtype=torch.uint8, device="cuda"), torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
        offsets = np.zeros(S + 1, np.int32)
        offsets[-1] = 1
        return ops.scene_compose(ctx, ids, colors, offsets, background, channel_order), [[] for _ in scenes]
    K_inst = Ks[plan.scene_of]
    renders = [render_rgbd_batch(models[o], (w, h), K_inst[idx], plan.R[idx], plan.t[idx], clip_near, clip_far, ctx=ctx, **shading)
               for o, idx in plan.groups.items()]
    depth, rgb = (r[0][k] if len(r) == 1 else torch.cat([x[k] for x in r])[torch.from_numpy(plan.order).to(r[0][k].device)]
                  for r, k in ((renders, "depth"), (renders, "rgb")))
    out = ops.scene_gt_info(ctx, depth, plan.scene_offsets, to_device(k4(K_inst, n)), None, delta)
    return ops.scene_compose(ctx, out.id_image, rgb, plan.scene_offsets, background, channel_order), _info(plan, out)


def annotations_from_scene(info, id_row, skip=()):
    """The fields of the reference's per-object annotation that come from the ground-truth pass (annotate_BOP.py:363-378, 420,
    461-471), for one scene: info: that scene's list from scene_gt_info; id_row: the obj_id of each of its instances, in
    instance order; skip: obj_ids left out of the annotations (the reference's specific_object_set / per-dataset exclusions).
    -> a list of dicts with category_id, bbox (= bbox_visib), area (bbox w * h), mask_id and feature_visibility (=
    visib_fract).  mask_id is the instance's 1-based position in the scene, the value the id image carries for it: a skipped
    instance keeps its number, as in the reference, where the counter runs before the exclusions."""
    id_row = list(id_row)
    if len(id_row) != len(info):
        raise ValueError("annotations_from_scene: %d ids for %d instances" % (len(id_row), len(info)))
    out = []
    for i, (obj_id, gt) in enumerate(zip(id_row, info)):
        if obj_id in skip:
            continue
        bbox = [int(v) for v in gt["bbox_visib"]]
        out.append({"category_id": obj_id, "bbox": bbox, "area": bbox[2] * bbox[3], "mask_id": i + 1,
                    "feature_visibility": float(gt["visib_fract"])})
    return out
