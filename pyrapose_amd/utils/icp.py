"""ICP refinement of estimated poses against scene depth, on the device (csrc/icp.hip): the block of
PyraPose_ROS_wrapper/scripts/pyrapose_node.py:run_estimation (:662-756; the same block at utils/ycbv_eval.py:424-526, 812-896,
and the get_evaluation* helpers of tless_eval.py:23-65 / occlusion_eval.py / linemod_eval.py / homebrewed_eval.py), which runs
on the CPU through Open3D and OpenCV there.

    mask (> 0.5 on the P3 grid, PIL-nearest upsampled) -> create_point_cloud of the masked depth -> voxel_down_sample 5 mm
    -> model at the PnP guess, faces turned away from the camera dropped -> scene gated to guess z +- 75 mm (fewer than 50
    points, or the scene median more than 75 mm from the guess: the model is moved onto the scene mean instead)
    -> estimate_normals (radius 10, max_nn 10) -> 100 iterations of point-to-plane ICP.

Deliberate deviations (also in DESIGN.md §7b):
  * Model normals come from the mesh faces (uniform surface samples carrying their face's normal by its winding, turned
    outward by the sign of the signed volume, averaged per voxel, i.e. area-weighted), not from estimate_normals on the model
    cloud: the reference's PCA normals are unoriented, so its
    back-face cull (normal[2] < 0) keeps either side at random.  A model given as points only gets PCA normals turned away
    from its centroid.
  * cv2.ppf_match_3d_ICP (Picky ICP, 4 pyramid levels, OpenCV internals) is replaced by Open3D-style point-to-plane ICP.
  * The default max_correspondence_distance is 10 mm: two voxels, about the 5-15 mm / 2-5 degree error of a good PnP pose on
    a 50-150 mm object; the commented-out Open3D call of the reference (:734) uses 5 mm at 5 mm voxels, which loses most
    correspondences of such a start.
  * In the fallback the reference sets the guess translation to the scene mean while it moves the model by (scene mean -
    model mean); here the translation moves by (scene mean - model mean), so the model's mean lands on the scene mean.
  * Voxel output order is ascending voxel key (Open3D's hash order is not reproducible).
Parity is unpinned: Open3D and OpenCV are not available and the reference ships no fixture; the contract is kept, the estimator
is this library's own, pinned to its numpy restatement (tests/icp_np.py) and to analytic and rendered scenes."""
import numpy as np
import torch

from .. import ops
from ..runtime import default_context
from ._host import k4, pack_ragged, to_device
from .anchors import guess_shapes


class RegistrationResult(object):
    """Open3D's registration result fields: transformation (4x4), fitness, inlier_rmse, correspondence_set [k,2] (source,
    target); plus iterations (updates applied) and status ('ok', 'too_few_correspondences', 'singular')."""

    def __init__(self, transformation, fitness, inlier_rmse, iterations, status, correspondence_set):
        self.transformation = transformation
        self.fitness = fitness
        self.inlier_rmse = inlier_rmse
        self.iterations = iterations
        self.status = status
        self.correspondence_set = correspondence_set

    def __repr__(self):
        return "RegistrationResult(fitness=%.6g, inlier_rmse=%.6g, iterations=%d, status=%s)" % (
            self.fitness, self.inlier_rmse, self.iterations, self.status)


def _points(a, what):
    p = a if torch.is_tensor(a) else np.asarray(a, np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("%s must be [n,3], got %s" % (what, tuple(p.shape)))
    return p


def create_point_cloud(depth, fx, fy, cx, cy, ds):
    """pyrapose_node.py:170-189: [rows*cols, 3] float64 (numpy), point (r, c) = ((c - cx) z / fx, (r - cy) z / fy, z) with
    z = depth * ds, the whole row NaN where z == 0 (:186) and NaN wherever the caller put NaN into depth."""
    d = np.asarray(depth)
    if d.ndim != 2:
        raise ValueError("create_point_cloud: depth must be [rows, cols]")
    return ops.cloud_from_depth(default_context(), to_device(d, torch.float32), fx, fy, cx, cy, ds, dense=True).cpu().numpy()


def _mask_grid(mask, shape):
    """mask [mh,mw] (bool / uint8 / scores thresholded by the caller) -> (uint8 grid, row index map [h], col index map [w])"""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("mask must be 2-D, got %s" % (m.shape,))
    h, w = shape
    mh, mw = m.shape
    rows = np.arange(h, dtype=np.int32) if mh == h else ops.pil_nearest_index(mh, h)
    cols = np.arange(w, dtype=np.int32) if mw == w else ops.pil_nearest_index(mw, w)
    return (m != 0).astype(np.uint8), rows, cols


def cloud_from_depth(depth, K, mask=None, ds=1.0, ctx=None):
    """The compacted device form: cuda float64 [n,3] of the pixels with finite, non-zero depth * ds whose mask cell is set, in
    row-major pixel order.  mask: None, [h,w], or a coarse grid [mh,mw] upsampled PIL-nearest (ops.pil_nearest_index)."""
    ctx = ctx or default_context()
    d = depth if torch.is_tensor(depth) else np.asarray(depth)
    if d.ndim != 2:
        raise ValueError("cloud_from_depth: depth must be [h,w]")
    fx, fy, cx, cy = k4(K)
    dt = to_device(d, torch.float32)
    if mask is None:
        return ops.cloud_from_depth(ctx, dt, fx, fy, cx, cy, ds)[0]
    g, rows, cols = _mask_grid(mask, tuple(d.shape))
    return ops.cloud_from_depth(ctx, dt, fx, fy, cx, cy, ds, to_device(g, torch.uint8), to_device(rows, torch.int32), to_device(cols, torch.int32))[0]


def voxel_down_sample(points, voxel_size, normals=None, ctx=None):
    """Open3D voxel_down_sample: the mean of the points of each voxel (normals averaged and renormalised), ascending voxel key
    order.  Returns cuda float64 [m,3], or ([m,3], [m,3]) with normals."""
    if not voxel_size > 0:
        raise ValueError("voxel_down_sample: voxel_size must be positive")
    p = to_device(_points(points, "points"))
    n = to_device(_points(normals, "normals")) if normals is not None else None
    out, out_n = ops.voxel_down_sample(ctx or default_context(), p, float(voxel_size), n)
    return (out, out_n) if normals is not None else out


def estimate_normals(points, radius, max_nn, ctx=None):
    """Open3D estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)): cuda float64 [n,3], toward the camera at the origin,
    zero for points with fewer than 3 neighbours."""
    return ops.estimate_normals(ctx or default_context(), to_device(_points(points, "points")), float(radius), int(max_nn))


def registration_icp_batch(problems, max_correspondence_distance, estimation="point_to_plane", max_iteration=30,
                           relative_fitness=1e-6, relative_rmse=1e-6, ctx=None):
    """problems: list of dicts (source [n,3], target [m,3], optional init 4x4 and target_normals [m,3]); one launch sequence
    for all of them.  Returns one RegistrationResult per problem."""
    if estimation not in ops.ICP_MODES:
        raise ValueError("registration_icp: unknown estimation %r" % (estimation,))
    if not problems:
        return []
    src, tgt, nrm, init = [], [], [], []
    for pr in problems:
        s, t = _points(pr["source"], "source"), _points(pr["target"], "target")
        T = np.asarray(pr.get("init", np.eye(4)), np.float64)
        if T.shape != (4, 4):
            raise ValueError("registration_icp: init must be 4x4")
        src.append(to_device(s))
        tgt.append(to_device(t))
        init.append(T)
        if estimation == "point_to_plane":
            if pr.get("target_normals") is None:
                raise ValueError("registration_icp: point_to_plane needs target_normals")
            nn = _points(pr["target_normals"], "target_normals")
            if nn.shape[0] != t.shape[0]:
                raise ValueError("registration_icp: target_normals must match the target points")
            nrm.append(to_device(nn))
    (so, src), (to, tgt) = pack_ragged(src), pack_ragged(tgt)
    R, t, fit, rmse, iters, status, corr = ops.icp(
        ctx or default_context(), to_device(so, torch.int32), to_device(to, torch.int32), src, tgt, to_device(np.stack(init)),
        float(max_correspondence_distance), int(max_iteration), float(relative_fitness), float(relative_rmse), estimation,
        torch.cat(nrm) if nrm else None)
    R, t, fit, rmse = R.cpu().numpy(), t.cpu().numpy(), fit.cpu().numpy(), rmse.cpu().numpy()
    iters, status, corr = iters.cpu().numpy(), status.cpu().numpy(), corr.cpu().numpy()
    out = []
    for p in range(len(problems)):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R[p], t[p]
        c = corr[so[p]:so[p + 1]]
        cs = np.stack([np.nonzero(c >= 0)[0], c[c >= 0]], 1).astype(np.int64)
        out.append(RegistrationResult(T, float(fit[p]), float(rmse[p]), int(iters[p]), ops.ICP_STATUS[int(status[p])], cs))
    return out


def registration_icp(source, target, max_correspondence_distance, init=np.eye(4), estimation="point_to_plane", max_iteration=30,
                     relative_fitness=1e-6, relative_rmse=1e-6, target_normals=None, ctx=None):
    """Open3D registration_icp(source, target, max_correspondence_distance, init, estimation,
    ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)) -> RegistrationResult."""
    return registration_icp_batch([dict(source=source, target=target, init=init, target_normals=target_normals)],
                                  max_correspondence_distance, estimation, max_iteration, relative_fitness, relative_rmse, ctx)[0]


def _mesh_samples(pts, faces, spacing):
    """uniform samples of every triangle (barycentric grid, edges <= spacing) with the triangle's unit normal by its winding,
    all flipped when the mesh's signed volume is negative (inward winding)"""
    P = pts[faces]                                                      # [m,3,3]
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    if np.einsum("ij,ij->", P[:, 0], n) < 0:
        n = -n
    ln = np.linalg.norm(n, axis=1)
    keep = ln > 0
    P, n = P[keep], n[keep] / ln[keep, None]
    edge = np.max(np.linalg.norm(P - np.roll(P, 1, axis=1), axis=2), axis=1)
    k = np.maximum(np.ceil(edge / spacing).astype(np.int64), 1)
    S, N = [], []
    for kk in np.unique(k):
        sel = k == kk
        i, j = np.meshgrid(np.arange(kk + 1), np.arange(kk + 1), indexing="ij")
        ok = i + j <= kk
        a, b = i[ok] / float(kk), j[ok] / float(kk)
        c = 1.0 - a - b
        Q = P[sel]
        S.append((a[None, :, None] * Q[:, None, 0] + b[None, :, None] * Q[:, None, 1] + c[None, :, None] * Q[:, None, 2]).reshape(-1, 3))
        N.append(np.repeat(n[sel], len(a), axis=0))
    return np.concatenate(S), np.concatenate(N)


def model_cloud(model, voxel_size, scale=1000.0, ctx=None):
    """The source cloud of a model (dict with 'pts' [n,3] and optionally 'faces' [m,3], or a point array), in depth units:
    (points [k,3], outward normals [k,3]) as cuda float64, voxel down-sampled."""
    ctx = ctx or default_context()
    pts = np.asarray(model["pts"] if isinstance(model, dict) else model, np.float64) * scale
    if pts.ndim != 2 or pts.shape[1] != 3 or len(pts) < 3:
        raise ValueError("model points must be [n,3] with n >= 3")
    faces = model.get("faces") if isinstance(model, dict) else None
    if faces is not None and len(faces):
        S, N = _mesh_samples(pts, np.asarray(faces, np.int64), 0.5 * voxel_size)
        p, n = ops.voxel_down_sample(ctx, to_device(S), float(voxel_size), to_device(N))
        return p, n
    p = ops.voxel_down_sample(ctx, to_device(pts), float(voxel_size))[0]
    n = ops.estimate_normals(ctx, p, 2.0 * voxel_size, 30)
    out = p - p.mean(0, keepdim=True)
    n = torch.where(((n * out).sum(1, keepdim=True) < 0), -n, n)
    return p, n


def refine_poses(dets, depth, mask_scores, K, models, mask_threshold=0.5, min_mask_pixels=3000, voxel_size=5.0, normal_radius=10.0,
                 normal_max_nn=10, z_gate=75.0, min_gate_points=50, max_correspondence_distance=10.0, max_iteration=100,
                 relative_fitness=1e-6, relative_rmse=1e-6, depth_scale=1000.0, ctx=None, box_margin=8.0):
    """Refine the PnP poses of one image against its depth (pyrapose_node.py:662-756).  dets: dicts of
    pose_decode.poses_from_outputs (cls, R, t in model units = metres); depth [h,w] in depth units (millimetres); mask_scores the
    mask output of predict_on_batch for this image, [h/8 * w/8, C] (or [1, ., C]); K 3x3; models: per class a load_ply dict
    ('pts' in metres, 'faces') or a point array; depth_scale: model unit -> depth unit.  All detections run in one ICP batch.
    Returns new dicts: the input's keys with R / t replaced by the refined pose, plus refined, fitness, inlier_rmse and
    iterations.  A detection whose upsampled mask has at most min_mask_pixels pixels, whose scene is empty, or whose ICP fails
    keeps its input pose with refined=False.
    A detection that carries a 'box' key (x1, y1, x2, y2 in pixels: the per-instance detections of
    poses_from_outputs(instances=...)) has its class mask restricted, before the min_mask_pixels test and the cloud cut, to the
    P3 cells whose pixel footprint intersects the box grown by box_margin pixels (default 8: one cell) -- several objects of
    one class share a mask channel, and the median, the gate and the ICP target must see one of them.  The library's own
    step; detections without 'box' behave as before."""
    ctx = ctx or default_context()
    d = np.asarray(depth)
    if d.ndim != 2:
        raise ValueError("refine_poses: depth must be [h,w]")
    h, w = d.shape
    fx, fy, cx, cy = k4(K)
    ms = np.asarray(mask_scores.cpu() if torch.is_tensor(mask_scores) else mask_scores, np.float32)
    if ms.ndim == 3 and ms.shape[0] == 1:
        ms = ms[0]
    mh, mw = (int(v) for v in guess_shapes((h, w), [3])[0])
    if ms.ndim != 2 or ms.shape[0] != mh * mw:
        raise ValueError("refine_poses: mask_scores must be [%d, C] for a %dx%d depth image, got %s" % (mh * mw, h, w, ms.shape))
    for name, v in (("voxel_size", voxel_size), ("normal_radius", normal_radius), ("z_gate", z_gate), ("depth_scale", depth_scale),
                    ("max_correspondence_distance", max_correspondence_distance)):
        if not v > 0:
            raise ValueError("refine_poses: %s must be positive" % name)
    if not box_margin >= 0:
        raise ValueError("refine_poses: box_margin must be >= 0")
    for det in dets:
        if det.get("box") is not None and (np.asarray(det["box"]).size != 4 or not np.isfinite(np.asarray(det["box"], np.float64)).all()):
            raise ValueError("refine_poses: box must be four finite numbers (x1, y1, x2, y2)")
        if not 0 <= int(det["cls"]) < ms.shape[1] or int(det["cls"]) >= len(models):
            raise ValueError("refine_poses: class %r has no mask channel or no model" % (det["cls"],))
        if np.asarray(det["R"]).shape != (3, 3) or np.asarray(det["t"]).size != 3:
            raise ValueError("refine_poses: each detection needs R 3x3 and t [3]")
        tt = np.asarray(det["t"], np.float64).reshape(3) * depth_scale
        if not np.isfinite(tt).all() or np.linalg.norm(tt) > 1.0e5:
            raise ValueError("refine_poses: a translation beyond 100 m at depth_scale %g: t must be in model units (metres)" % depth_scale)
    for m in set(int(det["cls"]) for det in dets):
        pts = np.asarray(models[m]["pts"] if isinstance(models[m], dict) else models[m], np.float64)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("refine_poses: model %d points must be [n,3]" % m)
        if np.ptp(pts, axis=0).max() * depth_scale > 10000.0:
            raise ValueError("refine_poses: model %d is larger than 10 m at depth_scale %g: model points must be in metres" % (m, depth_scale))
    rows, cols = ops.pil_nearest_index(mh, h), ops.pil_nearest_index(mw, w)
    rcount, ccount = np.bincount(rows, minlength=mh), np.bincount(cols, minlength=mw)
    dt = to_device(d, torch.float32)
    rows_d, cols_d = to_device(rows, torch.int32), to_device(cols, torch.int32)
    cache = {}
    problems, owners = [], []
    out = [dict(det, refined=False, fitness=0.0, inlier_rmse=0.0, iterations=0) for det in dets]
    for k, det in enumerate(dets):
        cls = int(det["cls"])
        grid = (ms[:, cls] > mask_threshold).reshape(mh, mw)
        if det.get("box") is not None:
            x1, y1, x2, y2 = (float(v) for v in np.asarray(det["box"], np.float64).reshape(4))
            # pixel p covers [p, p + 1]; a cell is kept when one of its pixels touches the grown box
            py, px = np.arange(h), np.arange(w)
            row_hit = np.bincount(rows, weights=((py + 1 >= y1 - box_margin) & (py <= y2 + box_margin)), minlength=mh) > 0
            col_hit = np.bincount(cols, weights=((px + 1 >= x1 - box_margin) & (px <= x2 + box_margin)), minlength=mw) > 0
            grid = grid & row_hit[:, None] & col_hit[None, :]
        if float(rcount @ grid.astype(np.float64) @ ccount) <= min_mask_pixels:
            continue
        scene, _ = ops.cloud_from_depth(ctx, dt, fx, fy, cx, cy, 1.0, to_device(grid, torch.uint8), rows_d, cols_d)
        if scene.shape[0] < 3:
            continue
        scene = ops.voxel_down_sample(ctx, scene, float(voxel_size))[0]
        if cls not in cache:
            cache[cls] = model_cloud(models[cls], voxel_size, depth_scale, ctx)
        mp, mn = cache[cls]
        R = to_device(det["R"])
        t = to_device(np.asarray(det["t"], np.float64).reshape(3) * depth_scale)
        front = (mn @ R.T)[:, 2] < 0                                       # model points facing the camera (:686-693)
        src = mp[front]
        if src.shape[0] < 6:
            continue
        cam = src @ R.T + t
        z = scene[:, 2]
        gated = scene[(z > t[2] - z_gate) & (z < t[2] + z_gate)]
        median = torch.quantile(scene, 0.5, dim=0)                          # np.median (:698)
        far = float(torch.linalg.norm(median - t)) > z_gate
        if gated.shape[0] < min_gate_points or far:                         # :716-726
            centre = gated.mean(0) if (gated.shape[0] > min_gate_points and far) else median
            t = t + (centre - cam.mean(0))
            target = scene
        else:
            target = gated
        nrm = ops.estimate_normals(ctx, target, float(normal_radius), int(normal_max_nn))
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = np.asarray(det["R"], np.float64), t.cpu().numpy()
        problems.append(dict(source=src, target=target, init=T, target_normals=nrm))
        owners.append(k)
    if problems:
        res = registration_icp_batch(problems, max_correspondence_distance, "point_to_plane", max_iteration, relative_fitness,
                                     relative_rmse, ctx)
        for k, r in zip(owners, res):
            out[k].update(fitness=r.fitness, inlier_rmse=r.inlier_rmse, iterations=r.iterations)
            if r.status == "ok" and r.fitness > 0:
                out[k].update(R=r.transformation[:3, :3].copy(), t=r.transformation[:3, 3] / depth_scale, refined=True)
    return out


def refine_pose(R, t, depth, mask, K, model, **kwargs):
    """One pose: R 3x3, t [3] (metres), depth [h,w] (millimetres), mask [h/8, w/8] scores of the class (or [h/8 * w/8]), K 3x3,
    model as in refine_poses -> (R, t, info dict with refined, fitness, inlier_rmse, iterations)."""
    m = np.asarray(mask, np.float32).reshape(-1, 1)
    r = refine_poses([dict(cls=0, R=np.asarray(R, np.float64), t=np.asarray(t, np.float64).reshape(3))], depth, m, K, [model], **kwargs)[0]
    return r["R"], r["t"], {k: r[k] for k in ("refined", "fitness", "inlier_rmse", "iterations")}
