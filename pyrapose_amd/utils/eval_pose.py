"""Pose evaluation loop: the arithmetic of utils/linemod_eval.py:evaluate_linemod (263-660) -- and of its siblings
occlusion_eval.py / ycbv_eval.py / tless_eval.py, which differ in the vote threshold and the class tables -- without the file
loaders, progress bars and OpenCV drawing around it.  Per image: network outputs -> per-class votes (score > threshold, at
least `min_votes`) -> RANSAC-PnP on the 8 cuboid corners -> ADD (ADD-S for the symmetric classes) against the ground
truth pose -> "true pose" when the error is below 10 % of the model diameter (:525-531).  Counters and rates as at :259-262
and :639-660 (index = class id + 1, as there)."""
import numpy as np

from . import pose_decode, pose_error


def quat2mat(q):
    """unit quaternion (w, x, y, z) -> rotation matrix; what the reference gets from transforms3d.quaternions.quat2mat
    (linemod_eval.py:511) for the normalised quaternions of its annotations."""
    w, x, y, z = [float(v) for v in q]
    n = w * w + x * x + y * y + z * z
    if n < 1e-12:
        return np.eye(3)
    s = 2.0 / n
    X, Y, Z = x * s, y * s, z * s
    wX, wY, wZ, xX, xY, xZ, yY, yZ, zZ = w * X, w * Y, w * Z, x * X, x * Y, x * Z, y * Y, y * Z, z * Z
    return np.array([[1.0 - (yY + zZ), xY - wZ, xZ + wY], [xY + wZ, 1.0 - (xX + zZ), yZ - wX], [xZ - wY, yZ + wX, 1.0 - (xX + yY)]])


def match_instances(t_est, t_gt):
    """Detections to annotations of one class, one to one: all pairwise translation errors |t_est[i] - t_gt[j]|, assigned
    greedily by ascending error (ties in (detection, annotation) index order), each side used once.  t_est [n,3], t_gt [m,3]
    -> list of (detection, annotation) pairs in the order they were assigned, min(n, m) long.  The reference has no such step:
    it scores against the first annotation of the class (tless_eval.py:378)."""
    a = np.asarray(t_est, np.float64).reshape(-1, 3)
    g = np.asarray(t_gt, np.float64).reshape(-1, 3)
    if len(a) == 0 or len(g) == 0:
        return []
    err = np.linalg.norm(a[:, None, :] - g[None, :, :], axis=2)
    used_d, used_g, pairs = set(), set(), []
    for flat in np.argsort(err.reshape(-1), kind="stable"):                  # stable: ties stay in (i, j) order
        i, j = divmod(int(flat), len(g))
        if i in used_d or j in used_g:
            continue
        used_d.add(i)
        used_g.add(j)
        pairs.append((i, j))
    return pairs


def _class_pairs(group, cls, labels, anno, gt_translation_scale, instances):
    """(detection, annotation index) pairs of one class: every detection against the first annotation of the class (the
    reference, instances=None), or match_instances over all its annotations, in detection order"""
    if instances is None:
        return [(d, labels.index(cls)) for d in group]
    gts = [gi for gi, lab in enumerate(labels) if lab == cls]
    t_gt = [np.asarray(anno["poses"][gi], np.float64)[:3] * gt_translation_scale for gi in gts]
    return [(group[i], gts[j]) for i, j in sorted(match_instances([d["t"] for d in group], t_gt))]


def _refine(dets, refine, depth, mask_out, K, models):
    """the opt-in ICP step (utils.icp.refine_poses with the keyword arguments in `refine`) on the detections of one image"""
    from . import icp
    kw = dict(refine)
    models = kw.pop("models", models)
    m = mask_out.cpu().numpy() if hasattr(mask_out, "cpu") else np.asarray(mask_out)
    return icp.refine_poses(dets, depth, m[0], K, models, **kw)


def _scored_images(generator, predict_on_batch, decode_kw, K, refine, load_depth, models, gt_translation_scale, instances,
                   depth_always=False, draw=None):
    """The per-image loop of evaluate_add and evaluate_pose_metrics, once.  Per image with at least one label: predict, decode
    (pose_decode.poses_from_outputs with threeD_boxes and the keywords of `decode_kw`, its seed plus the image index), keep the
    detections of annotated classes (the reference only scores those, linemod_eval.py:327-329), optionally refine them, and
    pair them per class with annotations (_class_pairs).  K: 3x3 intrinsics or a callable index -> 3x3.
    load_depth: None, or index -> depth image, called once per image where a detection survived the class filter (with
    depth_always: on every labelled image, and `refine` then also sees an empty detection list, as evaluate_add has it).
    Yields (index, labels, anno, Kc, depth or None, mask, pairs_by_class) for every such image, pairs_by_class =
    [(cls, [(det, annotation index), ...])] with classes ascending and no empty class.
    draw: None, or dict(save_path, every=1, bgr=True): every such image (every `every`-th index) is also written to
    save_path/{index}.png with the cuboid wireframes of its annotations and of the detections that are scored
    (visualization.save_pose_image, one device pass); what is yielded does not change."""
    kw = dict(decode_kw)
    threeD_boxes, seed = kw.pop("threeD_boxes"), kw.pop("seed")
    for index in range(generator.size()):
        raw_image = generator.load_image(index)
        image = generator.preprocess_image(raw_image.copy() if draw is not None else raw_image)
        image, _scale = generator.resize_image(image)
        anno = generator.load_annotations(index)
        if len(anno["labels"]) < 1:
            continue
        labels = [int(l) for l in anno["labels"]]
        Kc = np.asarray(K(index) if callable(K) else K, np.float64).reshape(3, 3)
        boxes3D, scores, mask = predict_on_batch(np.expand_dims(image, axis=0))
        poses = pose_decode.poses_from_outputs(boxes3D, scores, threeD_boxes, Kc, seed=seed + index, instances=instances, **kw)
        dets = [d for d in poses if d["cls"] in labels]
        if refine is not None and load_depth is None:
            raise ValueError("refine needs load_depth")
        depth = None
        if load_depth is not None and (dets or depth_always):
            depth = np.asarray(load_depth(index))
            if refine is not None:
                dets = _refine(dets, refine, depth, mask, Kc, models)
        pairs_by_class = []
        for cls in sorted(set(d["cls"] for d in dets)):
            pairs = _class_pairs([d for d in dets if d["cls"] == cls], cls, labels, anno, gt_translation_scale, instances)
            if pairs:
                pairs_by_class.append((cls, pairs))
        if draw is not None:
            from . import visualization
            visualization.save_pose_image(draw, index, raw_image, dets, anno, threeD_boxes, Kc, gt_translation_scale)
        yield index, labels, anno, Kc, depth, mask, pairs_by_class


def evaluate_add(generator, predict_on_batch, threeD_boxes, model_points, model_diameters, K=None, threshold=0.5, min_votes=10,
                 symmetric_classes=(), gt_translation_scale=0.001, seed=0, refine=None, load_depth=None, weighting=None,
                 instances=None, draw=None):
    """generator: load_image / preprocess_image / resize_image / load_annotations / size() (preprocessing/generator.py);
    predict_on_batch: the prediction model's method (x [1,H,W,3] -> [boxes3D, scores, mask]);
    threeD_boxes [C,8,3], model_points: list of [n_c,3], model_diameters [C] -- all in the unit of the estimated translation
    (the reference works in metres and scales the annotation's millimetres by 0.001, :516);
    K: 3x3 intrinsics (default: LineMOD, :423); symmetric_classes: 0-based class ids scored with ADD-S (the reference's
    cls == 10 or 11, 1-based, :525).  refine: None, or the keyword arguments of utils.icp.refine_poses (plus optionally
    'models': meshes to refine against, default model_points): the detections of each image are then refined against
    load_depth(index) (millimetres) inside the network's mask output before scoring, and each error tuple gains (refined,
    fitness).  weighting: None, 'corners' or 'scores' -- the uncertainty-weighted refinement of
    pose_decode.poses_from_outputs on every RANSAC pose (before the optional ICP).  instances: None (one pose per class, scored
    against the first annotation of the class, as the reference does), or the dict of poses_from_outputs: poses are decoded per
    object instance, matched per class to all annotations of that class (match_instances), every matched pair is scored as the
    single pair is otherwise, trueDets counts matched pairs and each error tuple gains (instance, gt).  draw: None, or dict(save_path, every=1): one
    overlay PNG per scored image (_scored_images); nothing else changes.  Returns dict(allPoses, trueDets, truePoses, recall, detections, recall_all, detections_all, errors) with the
    reference's 1-based class indexing."""
    C = len(model_diameters)
    if K is None:
        K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    allPoses, truePoses, trueDets = (np.zeros((C + 1,), np.uint32) for _ in range(3))
    errors = []
    decode_kw = dict(threeD_boxes=threeD_boxes, threshold=threshold, min_votes=min_votes, seed=seed, weighting=weighting)
    # depth only serves the refinement here, which runs on every labelled image
    for index, labels, anno, _Kc, _depth, _mask, pairs_by_class in _scored_images(
            generator, predict_on_batch, decode_kw, K, refine, load_depth if refine is not None else None, model_points,
            gt_translation_scale, instances, depth_always=True, draw=draw):
        for lab in labels:
            allPoses[lab + 1] += 1
        for cls, pairs in pairs_by_class:
            for det, gi in pairs:
                trueDets[cls + 1] += 1
                pose = np.asarray(anno["poses"][gi], np.float64)
                R_gt, t_gt = quat2mat(pose[3:]), pose[:3] * gt_translation_scale
                fn = pose_error.adi if cls in symmetric_classes else pose_error.add
                err = fn(det["R"], det["t"].reshape(3, 1), R_gt, t_gt.reshape(3, 1), model_points[cls])
                errors.append((index, cls, float(err)) if refine is None else (index, cls, float(err), det["refined"], det["fitness"]))
                if instances is not None:
                    errors[-1] = errors[-1] + (det["instance"], gi)
                if det["ok"] and err < model_diameters[cls] * 0.1:
                    truePoses[cls + 1] += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        recall = np.nan_to_num(truePoses / allPoses.astype(np.float64))
        detections = np.nan_to_num(trueDets / allPoses.astype(np.float64))
    seen = max(int((allPoses[1:] > 0).sum()), 1)
    return dict(allPoses=allPoses, trueDets=trueDets, truePoses=truePoses, recall=recall, detections=detections,
                recall_all=float(recall[1:].sum() / seen), detections_all=float(detections[1:].sum() / seen), errors=errors)


ADD_FRACTIONS = tuple(round(0.05 * k, 2) for k in range(1, 20))  # tless_eval.py:665-725: 0.05 ... 0.95 x diameter
# BOP's thresholds of correctness (BOP Challenge 2019 on): MSSD < f x diameter, MSPD < p x (image width / 640) pixels
BOP_FRACTIONS = tuple(round(0.05 * k, 2) for k in range(1, 11))
BOP_PIXELS = tuple(5 * k for k in range(1, 11))


def evaluate_pose_metrics(generator, predict_on_batch, threeD_boxes, models, model_diameters, load_depth, K, threshold=0.5, min_votes=10,
                          delta=0.3, tau=20.0, vsd_threshold=0.3, cost_type="step", symmetric_classes=(), gt_translation_scale=0.001,
                          depth_scale=1000.0, seed=0, refine=None, weighting=None, instances=None, symmetries=None, bop_vsd=None,
                          mask_metrics=None, draw=None):
    """The metric block of tless_eval.py:470-725 (also in occlusion_eval.py / ycbv_eval.py / homebrewed_eval.py) on top of the
    loop of evaluate_add: per detected, annotated class, the rotation / translation errors re / te (correct when re < 5 deg
    and te < 0.05), the reprojection error (< 5 px), VSD against the image's depth (< vsd_threshold) and ADD (ADI for
    symmetric_classes) against 0.05 ... 0.95 x the model diameter.

    models: per class a load_ply dict ('pts' [n,3] and 'faces' [m,3]) in the unit of the estimated translation (metres, as
    model_vsd at tless_eval.py:77); load_depth(index): the scene's depth image [h,w] in millimetres (uint16 or float);
    K: 3x3 intrinsics or a callable index -> 3x3; depth_scale: model / translation unit -> depth unit (VSD runs in
    millimetres with delta / tau as the reference passes them, 0.3 / 20).  One launch per metric per (image, class).
    refine: None, or the keyword arguments of utils.icp.refine_poses: the detections of each image are then refined against
    its depth inside the network's mask output before scoring, and each error dict gains 'refined' and 'fitness'.
    weighting: as in evaluate_add.  instances: as in evaluate_add (None: today's one pose per class against the first
    annotation of the class); with a dict each error dict gains 'instance' and 'gt' (the annotation index).
    symmetries: None (nothing below is computed or returned), or per class None (no symmetry), a list from
    utils.symmetry.get_symmetry_transformations or an (S_R, S_t) pair: BOP's MSSD and MSPD (pose_error.mssd / mspd, one launch
    each per (image, class), MSSD in the unit of the model) are scored too.  Each error dict gains 'mssd', 'mspd' and
    'sym_mssd', 'sym_mspd' (the symmetry that attains each); the result gains mssd_less / mspd_less [10, C+1] (ok detections
    with MSSD < BOP_FRACTIONS x the model diameter, MSPD < BOP_PIXELS x depth image width / 640 pixels), their _rate arrays,
    ar_mssd / ar_mspd [C+1] (the mean of the rates over the ten thresholds) and bop_fractions / bop_pixels.
    bop_vsd: None (nothing below is computed or returned), or a dict of delta (15.0, depth units), visib_mode ('bop19') and
    cost_type ('step'): BOP's VSD over its tolerance range, taus = BOP_FRACTIONS x the model diameter x depth_scale, in one
    launch per (image, class) on the two renders the single-tau VSD uses (pose_error.vsd_multi_from_depth).  Each error dict
    gains 'vsd_bop' (ten values) and 'visib_fract' (the visible fraction of the annotation); the result gains vsd_bop_less
    [10 taus, 10 thresholds, C+1] (ok detections with vsd_bop < BOP_FRACTIONS as thresholds of correctness), vsd_bop_less_rate
    and ar_vsd [C+1], its mean over both axes; with symmetries also ar = (ar_vsd + ar_mssd + ar_mspd) / 3, BOP's average recall.
    mask_metrics: None (nothing below is computed or returned), or a dict of target (index -> the image's mask training target
    [M,C+1] or [1,M,C+1] as ops.anchor_targets writes it, an array or a device tensor) and optionally thresholds ((0.5,)): the
    mask output of every scored image is counted against its target on the device (utils.mask_eval.semantic_scores' pass); the
    result gains mask_counts [T,C,3] (tp, fp, fn over all scored images), mask_iou [T,C] and mask_miou [T].
    Annotations are not dropped from allPoses by their visible fraction (BOP keeps those of at least 10 %): filter in the
    generator, on scene_gt_info.json or on pose_error.visib_fract_batch.
    draw: None, or dict(save_path, every=1): one overlay PNG per scored image (_scored_images); nothing else changes.
    Returns dict(allPoses, trueDets, less5, rep_less5, vsd_less_t, add_less [len(ADD_FRACTIONS), C+1], add_fractions, the
    matching rates (counter / allPoses) and errors: one dict per scored detection); index = class id + 1 as in evaluate_add."""
    C = len(model_diameters)
    counters = ("allPoses", "trueDets", "less5", "rep_less5", "vsd_less_t")
    out = {k: np.zeros((C + 1,), np.uint32) for k in counters}
    add_less = np.zeros((len(ADD_FRACTIONS), C + 1), np.uint32)
    errors = []
    if symmetries is not None:
        from .symmetry import stack_symmetries
        if len(symmetries) != C:
            raise ValueError("symmetries: need one entry per class (%d), got %d" % (C, len(symmetries)))
        symmetries = [stack_symmetries(s) for s in symmetries]
        mssd_less = np.zeros((len(BOP_FRACTIONS), C + 1), np.uint32)
        mspd_less = np.zeros((len(BOP_PIXELS), C + 1), np.uint32)
    if bop_vsd is not None:
        unknown = set(bop_vsd) - {"delta", "visib_mode", "cost_type"}
        if unknown:
            raise ValueError("bop_vsd: unknown keys %s (delta | visib_mode | cost_type)" % sorted(unknown))
        bop_vsd = dict(dict(delta=15.0, visib_mode="bop19", cost_type="step"), **bop_vsd)
        vsd_bop_less = np.zeros((len(BOP_FRACTIONS), len(BOP_FRACTIONS), C + 1), np.uint32)
    if mask_metrics is not None:
        from . import mask_eval
        unknown = set(mask_metrics) - {"target", "thresholds"}
        if unknown or not callable(mask_metrics.get("target")):
            raise ValueError("mask_metrics: a dict of target (a callable index -> target) and optionally thresholds, got keys %s" %
                             sorted(mask_metrics))
        mask_thresholds = tuple(mask_metrics.get("thresholds", (0.5,)))
        mask_counts = None
    decode_kw = dict(threeD_boxes=threeD_boxes, threshold=threshold, min_votes=min_votes, seed=seed, weighting=weighting)
    refine = None if refine is None else dict(refine, depth_scale=depth_scale)
    for index, labels, anno, Kc, depth, mask_out, pairs_by_class in _scored_images(
            generator, predict_on_batch, decode_kw, K, refine, load_depth, models, gt_translation_scale, instances, draw=draw):
        for lab in labels:
            out["allPoses"][lab + 1] += 1
        if mask_metrics is not None:
            import torch
            pred = torch.as_tensor(mask_out)
            target = torch.as_tensor(mask_metrics["target"](index))
            c = mask_eval.semantic_scores(pred.reshape(1, -1, pred.shape[-1]), target.reshape(1, -1, target.shape[-1]), mask_thresholds)["counts"]
            mask_counts = c if mask_counts is None else mask_counts + c
        for cls, pairs in pairs_by_class:
            group = [d for d, _gi in pairs]
            gt = [np.asarray(anno["poses"][gi], np.float64) for _d, gi in pairs]
            R_est = np.stack([d["R"] for d in group])
            t_est = np.stack([np.asarray(d["t"], np.float64).reshape(3) for d in group])
            R_g, t_g = np.stack([quat2mat(p[3:]) for p in gt]), np.stack([p[:3] * gt_translation_scale for p in gt])
            model = models[cls]
            rd = pose_error.re_batch(R_g, R_est)                                 # re(R_gt, R_est) as at tless_eval.py:470
            xyz = pose_error.te_batch(t_g, t_est)
            rep = pose_error.reproj_batch(Kc, R_est, t_est, R_g, t_g, model["pts"])
            mm = dict(model, pts=np.asarray(model["pts"], np.float64) * depth_scale)
            if bop_vsd is None:
                e_vsd = pose_error.vsd_batch(R_est, t_est * depth_scale, R_g, t_g * depth_scale, mm, depth, Kc, delta, tau, cost_type)
            else:  # the two renders of vsd_batch, made once for both VSD launches
                d_est, d_gt, Ks = pose_error.render_pairs(R_est, t_est * depth_scale, R_g, t_g * depth_scale, mm, depth, Kc)
                e_vsd = pose_error.vsd_from_depth(depth, d_est, d_gt, Ks, delta, tau, cost_type)
                taus = np.array(BOP_FRACTIONS) * model_diameters[cls] * depth_scale
                e_bop, _inter, _uni, n_vis, n_px = pose_error.vsd_multi_from_depth(
                    depth, d_est, d_gt, Ks, bop_vsd["delta"], taus, bop_vsd["cost_type"], bop_vsd["visib_mode"], return_counts=True)
            e_add = pose_error.add_batch(R_est, t_est, R_g, t_g, model["pts"], symmetric=cls in symmetric_classes)
            if symmetries is not None:
                e_mssd, s_mssd = pose_error.mssd_batch(R_est, t_est, R_g, t_g, model["pts"], symmetries[cls], return_sym=True)
                e_mspd, s_mspd = pose_error.mspd_batch(R_est, t_est, R_g, t_g, Kc, model["pts"], symmetries[cls], return_sym=True)
                width = np.shape(depth)[1]
            for k, d in enumerate(group):
                out["trueDets"][cls + 1] += 1
                errors.append(dict(image=index, cls=cls, ok=d["ok"], re=float(rd[k]), te=float(xyz[k]), reproj=float(rep[k]),
                                   vsd=float(e_vsd[k]), add=float(e_add[k])))
                if refine is not None:
                    errors[-1].update(refined=d["refined"], fitness=d["fitness"])
                if instances is not None:
                    errors[-1].update(instance=d["instance"], gt=pairs[k][1])
                if symmetries is not None:
                    errors[-1].update(mssd=float(e_mssd[k]), mspd=float(e_mspd[k]), sym_mssd=int(s_mssd[k]), sym_mspd=int(s_mspd[k]))
                if bop_vsd is not None:
                    errors[-1].update(vsd_bop=e_bop[k].tolist(), visib_fract=float(n_vis[k]) / float(n_px[k]) if n_px[k] > 0 else 0.0)
                if not d["ok"]:
                    continue
                out["less5"][cls + 1] += bool(rd[k] < 5.0 and xyz[k] < 0.05)
                out["rep_less5"][cls + 1] += bool(rep[k] < 5.0)
                out["vsd_less_t"][cls + 1] += bool(e_vsd[k] < vsd_threshold)
                for j, f in enumerate(ADD_FRACTIONS):
                    add_less[j, cls + 1] += bool(e_add[k] < model_diameters[cls] * f)
                if symmetries is not None:
                    for j, f in enumerate(BOP_FRACTIONS):
                        mssd_less[j, cls + 1] += bool(e_mssd[k] < f * model_diameters[cls])
                    for j, p in enumerate(BOP_PIXELS):
                        mspd_less[j, cls + 1] += bool(e_mspd[k] < p * width / 640.0)
                if bop_vsd is not None:
                    vsd_bop_less[:, :, cls + 1] += e_bop[k][:, None] < np.array(BOP_FRACTIONS)[None, :]
    all_f = out["allPoses"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in counters[1:]:
            out[k + "_rate"] = np.nan_to_num(out[k] / all_f)
        out["add_less_rate"] = np.nan_to_num(add_less / all_f[None])
        if symmetries is not None:
            out.update(mssd_less=mssd_less, mspd_less=mspd_less, mssd_less_rate=np.nan_to_num(mssd_less / all_f[None]),
                       mspd_less_rate=np.nan_to_num(mspd_less / all_f[None]), bop_fractions=np.array(BOP_FRACTIONS),
                       bop_pixels=np.array(BOP_PIXELS, np.float64))
            out.update(ar_mssd=out["mssd_less_rate"].mean(axis=0), ar_mspd=out["mspd_less_rate"].mean(axis=0))
        if bop_vsd is not None:
            out.update(vsd_bop_less=vsd_bop_less, vsd_bop_less_rate=np.nan_to_num(vsd_bop_less / all_f[None, None]),
                       bop_fractions=np.array(BOP_FRACTIONS))
            out["ar_vsd"] = out["vsd_bop_less_rate"].mean(axis=(0, 1))
            if symmetries is not None:
                out["ar"] = (out["ar_vsd"] + out["ar_mssd"] + out["ar_mspd"]) / 3.0
    if mask_metrics is not None and mask_counts is not None:
        scored = mask_eval.scores_from_counts(mask_counts)
        out.update(mask_counts=mask_counts, mask_iou=scored["iou"], mask_miou=scored["miou"])
    out.update(add_less=add_less, add_fractions=np.array(ADD_FRACTIONS), errors=errors)
    return out
