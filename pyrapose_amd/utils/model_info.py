"""Model geometry from a mesh's points: what the training and evaluation paths otherwise read from a BOP dataset's
models_info.yml / .json (annotation_scripts/annotate_BOP.py:186-219) or from the reference's offline FPS.py (features.json),
so that a mesh outside any dataset can be trained on and evaluated:
  diameter (model_diameters of evaluate_add / evaluate_pose_metrics / PoseEvaluation, the taus of bop_vsd), min_* / size_*,
  threeD_boxes [C,8,3] (poses_from_outputs, target assignment; hard-coded by hand at render_custom_from_mesh.py:120-190),
  control points by greedy farthest-point sampling (FPS.py:37-99).
The all-pairs arithmetic runs on the device in float64 (csrc/model_info.hip); boxes are plain numpy.  bop_toolkit's
misc.calc_pts_diameter and FPS.py are restated, not run: parity with either is unpinned (tests/model_info_np.py holds the
restatements the kernels are bit-identical to)."""
import json
import math
import os
import warnings

import numpy as np
import torch

from .. import ops
from ..runtime import default_context
from ._host import pack_ragged, to_device


def _pts(model):
    """load_ply's dict, a path to a .ply or an [n,3] array -> float64 [n,3], n >= 1"""
    if isinstance(model, (str, os.PathLike)):
        from .ply_loader import load_ply
        model = load_ply(model)
    pts = np.asarray(model["pts"] if isinstance(model, dict) else model, np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError("a model's points must be n x 3 with n >= 1, got %s" % (pts.shape,))
    return pts


def pts_diameter(pts, return_pair=False):
    """The largest distance between two points of pts [n,3]: float; with return_pair also (i, j), i <= j, the pair that attains
    it (the lowest i, then the lowest j).  One launch over all pairs in float64; the root is taken here, as calc_pts_diameter
    takes it after its max."""
    d2, pair = ops.pts_diameter(default_context(), to_device(_pts(pts)))
    d = math.sqrt(float(d2.cpu()[0]))
    if not return_pair:
        return d
    i, j = (int(v) for v in pair.cpu())
    return d, (i, j)


def calc_pts_diameter(pts):
    """bop_toolkit_lib.misc.calc_pts_diameter: the diameter of a set of 3D points."""
    return pts_diameter(pts)


def model_info(model, symmetries=None):
    """One entry of a BOP models_info.json from a model (load_ply's dict, a path or an [n,3] array): diameter, min_x, min_y,
    min_z, size_x, size_y, size_z as floats; min and max are exact, size = max - min in float64.  symmetries: None (no
    symmetry keys), True or a dict of find_symmetries' keywords: the entry then also holds what find_symmetries(model) finds,
    'symmetries_discrete' and / or 'symmetries_continuous'."""
    if isinstance(model, (str, os.PathLike)):
        from .ply_loader import load_ply
        model = load_ply(model)
    pts = to_device(_pts(model))
    lo, hi = pts.min(dim=0).values.cpu().numpy(), pts.max(dim=0).values.cpu().numpy()
    d2, _ = ops.pts_diameter(default_context(), pts)
    info = {"diameter": math.sqrt(float(d2.cpu()[0]))}
    for a, axis in enumerate("xyz"):
        info["min_" + axis] = float(lo[a])
        info["size_" + axis] = float(hi[a] - lo[a])
    if symmetries is not None and symmetries is not False:
        info.update(find_symmetries(model, **({} if symmetries is True else dict(symmetries))))
    return info


def models_info(models, symmetries=None):
    """{int id: model or path} -> {int id: model_info(model, symmetries)}, the shape utils.symmetry.load_models_info returns.
    Without symmetries there are no symmetry entries: get_symmetry_transformations gives the identity for each."""
    return {int(k): model_info(m, symmetries) for k, m in models.items()}


def symmetric_ids(info):
    """The sorted int ids of a models_info dict that have any symmetry entry: the list a caller turns into the
    symmetric_classes= of evaluate_add / evaluate_pose_metrics (ADD-S instead of ADD)."""
    return sorted(int(k) for k, v in info.items() if v.get("symmetries_discrete") or v.get("symmetries_continuous"))


# ---- symmetries ---------------------------------------------------------------------------------------------------------
# A symmetry of a point set is a rigid transformation that moves the set onto itself.  The score of a candidate S is the
# one-sided Hausdorff distance of S(model) to the model, max_i min_j |S p_i - p_j| (pp_sym_hausdorff_f64: all candidates of a
# step in one launch), taken in both directions: the larger of S and of its inverse.

_PHI = (math.sqrt(5.0) - 1.0) / 2.0   # the golden ratio conjugate: its multiples stay away from every fraction of small order
_SWEEP_STOP = 1e-4                    # rad: the bracketing of a swept axis ends below this step


def _device_scorer(src, tgt, S_R, S_t):
    d2, arg = ops.sym_hausdorff(default_context(), to_device(src), None if tgt is None else to_device(tgt), to_device(S_R), to_device(S_t))
    return d2.cpu().numpy(), arg.cpu().numpy()


def _device_diameter(pts):
    return math.sqrt(float(ops.pts_diameter(default_context(), to_device(pts))[0].cpu()[0]))


def symmetry_residuals(model, syms, target=None, _scorer=None):
    """How far each transformation of a symmetry set moves a model off itself (or off `target`), in model units: float64 [K],
    per transformation the larger of the two one-sided Hausdorff distances, of S(model) to the target and of S^-1(model) to
    it.  model / target: load_ply's dict, a path or an [n,3] array (the points as they are, no resampling); syms: a list from
    utils.symmetry.get_symmetry_transformations or an (S_R [K,3,3], S_t [K,3]) pair.  The inverses ride in the same launch as K
    further candidates.  This is also the check of a dataset's declared symmetries against its mesh: a declared
    transformation whose residual is far above the mesh's sampling distance does not hold for that mesh."""
    from .symmetry import stack_symmetries
    S_R, S_t = stack_symmetries(syms)
    inv_R = np.ascontiguousarray(S_R.transpose(0, 2, 1))
    inv_t = -np.einsum("kij,kj->ki", inv_R, S_t)
    K = S_R.shape[0]
    d2, _ = (_scorer or _device_scorer)(_pts(model), None if target is None else _pts(target), np.concatenate([S_R, inv_R]),
                                        np.concatenate([S_t, inv_t]))
    return np.sqrt(np.maximum(d2[:K], d2[K:]))


def _rotation_angle(A, B):
    """the angle of the rotation that takes A to B"""
    return math.acos(min(1.0, max(-1.0, (float(np.trace(A.T.dot(B))) - 1.0) / 2.0)))


def _merge_axes(axes, eps=1e-9):
    """unit axes in order, a and -a (and repeats) merged: the first of each line stays"""
    out = []
    for a in axes:
        a = np.asarray(a, np.float64).reshape(3)
        n = np.linalg.norm(a)
        if not n > 0.0:
            raise ValueError("find_symmetries: an axis must not be zero")
        a = a / n
        if all(abs(float(a.dot(b))) < 1.0 - eps for b in out):
            out.append(a)
    return out


def _perpendicular(a):
    """(u, v): a right-handed orthonormal pair perpendicular to the unit axis a; u lies along a coordinate axis when a does"""
    e = np.zeros(3)
    e[int(np.argmin(np.abs(a)))] = 1.0
    u = e - a * float(a.dot(e))
    u /= np.linalg.norm(u)
    return u, np.cross(a, u)


def _close_group(elements, merge, max_group):
    """Rotations composed until closed: the given ones first, in order, then the products as they arise; an element within
    `merge` rad of the identity or of an earlier element is dropped; at most max_group elements."""
    group = []
    for R in elements:
        if _rotation_angle(np.eye(3), R) >= merge and all(_rotation_angle(G, R) >= merge for G in group):
            group.append(R)
    done = 0
    while done < len(group) and len(group) < max_group:
        new = group[done]
        done += 1
        for other in list(group):
            for P in (new.dot(other), other.dot(new)):
                if len(group) < max_group and _rotation_angle(np.eye(3), P) >= merge and all(_rotation_angle(G, P) >= merge for G in group):
                    group.append(P)
    return group


def find_symmetries(model, tol=0.01, orders=(2, 3, 4, 5, 6, 8), axes=None, center=None, n_probe=8, n_sweep=180, sample=0.02,
                    max_group=120, return_residuals=False, _scorer=None, _diameter=None):
    """The rotational symmetries of a model, in the form of a BOP models_info entry: a dict that holds 'symmetries_discrete'
    (each 16 numbers, a row-major 4x4) and / or 'symmetries_continuous' ({'axis': [3], 'offset': [3]}); a key is absent when
    its list is empty, so an asymmetric model gives {}.  utils.symmetry.get_symmetry_transformations consumes the result
    unchanged.  return_residuals adds 'residuals_discrete' / 'residuals_continuous': the residual of every returned element
    (for an axis: its worst probe) as a fraction of the diameter.

    Points: an [n,3] array or a model without faces is used as it is; a model with faces is sampled uniformly on its surface
    (utils.icp.model_cloud with voxel_size = sample * diameter).  The cloud is both source and target.  A sampled cloud is one
    mean per voxel of an axis-aligned grid, which no rotation keeps: a true symmetry of the mesh leaves a residual of up to
    about (1 + sqrt 3) * sample of the diameter (a voxel's diagonal plus a mean's distance off the surface), so for a mesh
    with faces tol must exceed that -- the defaults (0.02, 0.01) do not, and a warning says so: pass e.g. sample=0.01,
    tol=0.03, or the mesh's vertices as an array when they are dense and regular.
    Centre: `center`, by default the mean of the cloud (float64) -- every exact symmetry of the cloud keeps it.  Every
    candidate is a rotation R about an axis through the centre c: S = (R, c - R c).
    Accept: symmetry_residuals(S) <= tol * diameter (the diameter of the cloud, ops.pts_diameter).
    Candidate axes: `axes`, the coordinate axes and the three eigenvectors of the cloud's covariance, a and -a merged; per
    axis the rotations by 2 pi / n, n in `orders`.  An axis is continuous when the rotations by 2 pi phi i, i = 1..n_probe,
    all pass (phi the golden ratio conjugate: no finite order passes them by accident).
    Perpendicular sweep: for every accepted axis the 2-fold rotations about n_sweep axes perpendicular to it, evenly spaced
    over pi, are scored; the local minima of the residual that a passing axis within half a sweep step could explain
    (residual <= (tol + pi / n_sweep) * diameter: half a step of axis error turns a point by a full step) are refined by
    bracketing the angle, all minima in one launch per round, to below 1e-4 rad, then put to the accept rule.  This finds the
    in-plane axes of an eigen-plane that has no preferred direction (a square or hexagonal section, any rotated model).
    Closure: BOP lists every non-identity element of the group, so the accepted discrete elements are composed until closed
    (elements within 3 tol rad of one another count as one; at most max_group), all scored in one more launch and kept only
    when they pass.  With a continuous axis the discrete rotations about it are dropped -- it generates them -- and of the
    2-fold rotations perpendicular to it the first in candidate order stays.

    Limits.  A cloud whose covariance is isotropic (cube, tetrahedron, sphere) has arbitrary eigenvectors: its axes are found
    only when they are coordinate axes, are given in `axes`, or arise by closure.  Reflections are not looked for (BOP's
    symmetries are proper rotations).  The default tol was chosen on synthetic shapes (point grids of boxes, prisms and
    cylinders: true elements score below 1e-15 of the diameter, the nearest false candidate 0.039); how it fits scanned
    meshes, whose symmetric parts differ by scanning noise, is unmeasured -- look at return_residuals and set tol.  Parity with
    any dataset's hand-annotated symmetries is unpinned: no dataset was at hand."""
    from .symmetry import _rotation
    score, diameter_of = _scorer or _device_scorer, _diameter or _device_diameter
    if isinstance(model, (str, os.PathLike)):
        from .ply_loader import load_ply
        model = load_ply(model)
    pts = _pts(model)
    faces = model.get("faces") if isinstance(model, dict) else None
    if faces is not None and len(faces):
        from .icp import model_cloud
        if float(tol) < (1.0 + math.sqrt(3.0)) * float(sample):
            warnings.warn("find_symmetries: tol = %g is below the sampled cloud's own residual bound (1 + sqrt 3) * sample = %g: a true "
                          "symmetry of the mesh may not pass; lower sample or raise tol" % (tol, (1.0 + math.sqrt(3.0)) * float(sample)))
        pts = model_cloud(model, voxel_size=float(sample) * diameter_of(pts), scale=1.0)[0].cpu().numpy().astype(np.float64)
    pts = np.ascontiguousarray(pts)
    c = pts.mean(axis=0) if center is None else np.asarray(center, np.float64).reshape(3)
    diameter = diameter_of(pts)
    if not diameter > 0.0:
        return {}
    limit = float(tol) * diameter
    merge = max(3.0 * float(tol), 10.0 * _SWEEP_STOP)

    def residuals(rotations):
        """rotations about the centre -> their residuals in model units, one launch"""
        S_R = np.stack(rotations)
        return symmetry_residuals(pts, (S_R, c - np.einsum("kij,j->ki", S_R, c)), _scorer=score)

    # 1. the candidate axes, each with its finite orders and its probes of a continuous symmetry
    centred = pts - c
    cand_axes = _merge_axes(list(axes if axes is not None else ()) + list(np.eye(3)) + list(np.linalg.eigh(centred.T.dot(centred))[1].T))
    orders = [int(n) for n in orders]
    angles = [2.0 * math.pi / n for n in orders] + [2.0 * math.pi * _PHI * i for i in range(1, int(n_probe) + 1)]
    res = residuals([_rotation(w, a) for a in cand_axes for w in angles]).reshape(len(cand_axes), len(angles))
    discrete, continuous, accepted_axes = [], [], []   # rotations; (axis, residual); axes that take a sweep
    for a, r in zip(cand_axes, res):
        if n_probe > 0 and (r[len(orders):] <= limit).all():
            # (an eigenvector of a sampled cloud is a coordinate axis only nearly: axes within `merge` rad are one, the first stays)
            if all(abs(float(a.dot(b))) < math.cos(merge) for b, _ in continuous):
                continuous.append((a, float(r[len(orders):].max())))
                accepted_axes.append(a)
            continue
        passed = [w for w, v in zip(angles[:len(orders)], r) if v <= limit]
        discrete += [_rotation(w, a) for w in passed]
        if passed:
            accepted_axes.append(a)

    # 2. 2-fold axes perpendicular to every accepted axis: sweep, local minima, bracketing
    if accepted_axes and n_sweep > 0:
        step = math.pi / int(n_sweep)
        frames = [_perpendicular(a) for a in accepted_axes]
        flip = lambda f, th: _rotation(math.pi, math.cos(th) * frames[f][0] + math.sin(th) * frames[f][1])
        r = residuals([flip(f, step * i) for f in range(len(frames)) for i in range(int(n_sweep))]).reshape(len(frames), int(n_sweep))
        minima = []   # [frame, angle, residual]
        for f in range(len(frames)):
            for i in range(int(n_sweep)):
                if r[f, i] <= r[f, i - 1] and r[f, i] <= r[f, (i + 1) % int(n_sweep)] and r[f, i] <= limit + step * diameter:
                    minima.append([f, step * i, float(r[f, i])])
        h = 0.5 * step
        while minima and h >= 0.5 * _SWEEP_STOP:
            side = residuals([flip(f, th + s * h) for f, th, _ in minima for s in (-1.0, 1.0)]).reshape(len(minima), 2)
            for mnm, (lo, hi) in zip(minima, side):
                if lo < mnm[2] and lo <= hi:
                    mnm[1], mnm[2] = mnm[1] - h, float(lo)
                elif hi < mnm[2]:
                    mnm[1], mnm[2] = mnm[1] + h, float(hi)
            h *= 0.5
        discrete += [flip(f, th) for f, th, v in minima if v <= limit]

    # 3. what a continuous axis generates goes; of the flips perpendicular to it the first stays
    for a, _ in continuous:
        kept, have_flip = [], False
        for R in discrete:
            Ra = R.dot(a)
            if np.linalg.norm(Ra - a) < merge:
                continue
            if np.linalg.norm(Ra + a) < merge:
                if have_flip:
                    continue
                have_flip = True
            kept.append(R)
        discrete = kept

    # 4. closure, every element scored once more
    group = _close_group(discrete, merge, int(max_group))
    out = {}
    if group:
        r = residuals(group)
        keep = [k for k in range(len(group)) if r[k] <= limit]
        if keep:
            M = np.tile(np.eye(4), (len(keep), 1, 1))
            for row, k in enumerate(keep):
                M[row, :3, :3] = group[k]
                M[row, :3, 3] = c - group[k].dot(c)
            out["symmetries_discrete"] = [m.reshape(-1).tolist() for m in M]
            if return_residuals:
                out["residuals_discrete"] = [float(r[k] / diameter) for k in keep]
    if continuous:
        out["symmetries_continuous"] = [{"axis": a.tolist(), "offset": c.tolist()} for a, _ in continuous]
        if return_residuals:
            out["residuals_continuous"] = [v / diameter for _, v in continuous]
    return out


def save_models_info(path, info):
    """Writes info as a BOP models_info.json (string keys); utils.symmetry.load_models_info reads it back equal."""
    with open(path, "w") as f:
        json.dump({str(int(k)): v for k, v in info.items()}, f, indent=2, sort_keys=True)
        f.write("\n")


# the reference's corner order: per corner and axis, whether it takes min + size (True) or min
_CORNER_IS_MAX = np.array([[1, 1, 1], [1, 1, 0], [1, 0, 0], [1, 0, 1], [0, 1, 1], [0, 1, 0], [0, 0, 0], [0, 0, 1]], bool)


def threeD_boxes(info, n_classes=None, scale=1.0):
    """The 8 box corners per class the reference builds from models_info (annotate_BOP.py:198-219, same corner order), at
    index int(key): float32 [C,8,3], C = n_classes or the largest key + 1, rows without an entry zero.  scale is the reference's
    `fac` (0.001: millimetres to metres), applied as annotate_synthetic_LineMOD_train.py:38-44 applies it: min * scale and
    size * scale + min * scale."""
    keys = [int(k) for k in info]
    if not keys or min(keys) < 0:
        raise ValueError("threeD_boxes: need at least one entry and keys >= 0")
    C = max(keys) + 1 if n_classes is None else int(n_classes)
    if C <= max(keys):
        raise ValueError("threeD_boxes: key %d does not fit %d classes" % (max(keys), C))
    boxes = np.zeros((C, 8, 3), np.float32)
    for key, value in info.items():
        lo = np.array([value["min_" + a] for a in "xyz"], np.float64) * scale
        hi = np.array([value["size_" + a] for a in "xyz"], np.float64) * scale + lo
        boxes[int(key)] = np.where(_CORNER_IS_MAX, hi, lo)
    return boxes


def _fps_min_dist(pts):
    """FPS.py:49-59: (x_dim + y_dim + z_dim) / 7"""
    dim = pts.max(axis=0) - pts.min(axis=0)
    return (dim[0] + dim[1] + dim[2]) / 7


def _farthest(pts_list, k, rule, start, min_dist):
    """k picks from each of the point sets in ONE launch -> int64 [M,k]; start / min_dist: None or one value per set"""
    if rule not in ops.FPS_RULES:
        raise ValueError("farthest_points: unknown rule %r (min | sum)" % (rule,))
    k = int(k)
    if k < 1:
        raise ValueError("farthest_points: k must be at least 1, got %d" % k)
    for p in pts_list:
        if rule == "min" and k > p.shape[0]:
            raise ValueError("farthest_points: rule 'min' picks k = %d distinct points, the model has %d" % (k, p.shape[0]))
    if start is not None:
        for s, p in zip(start, pts_list):
            if not 0 <= int(s) < p.shape[0]:
                raise ValueError("farthest_points: start %d is not a point of a model of %d" % (int(s), p.shape[0]))
        start = to_device(np.asarray([int(s) for s in start], np.int32), torch.int32)
    if rule == "sum":
        md = [_fps_min_dist(p) for p in pts_list] if min_dist is None else [float(v) for v in min_dist]
        min_dist = to_device(np.asarray(md, np.float64))
    elif min_dist is not None:
        raise ValueError("farthest_points: min_dist belongs to rule 'sum'; rule 'min' blocks no point")
    offsets, flat = pack_ragged(pts_list)
    index = ops.farthest_points(default_context(), to_device(flat), offsets, k, rule, min_dist, start)
    return index.cpu().numpy().astype(np.int64)


def farthest_points(pts, k, rule="min", start=None, min_dist=None):
    """Greedy farthest-point sampling of k points of pts [n,3] on the device -> (index int64 [k], points float64 [k,3] =
    pts[index]).  start: the first pick, None = the point of largest norm (the first of equals).  rule 'min': each further pick
    maximises the smallest squared distance to the points chosen so far (k <= n).  rule 'sum': the reference's FPS.py -- it
    maximises the sum of distances to the chosen points, each rounded to float32 as FPS.py's control_points are, and scores a
    point 0 once a chosen point is nearer than min_dist (None: FPS.py's (x_dim + y_dim + z_dim) / 7).  The lowest index wins
    ties."""
    pts = _pts(pts)
    index = _farthest([pts], k, rule, None if start is None else [start], None if min_dist is None else [min_dist])[0]
    return index, pts[index]


def control_points(models, k, rule="sum"):
    """The features.json dict of FPS.py:96-99 for {id: model or path}: {id: k points as lists of float32 values}, all models in
    one launch.  The key is the caller's id (the reference's mesh_name[-6:-4] is file-name glue)."""
    keys = list(models)
    pts_list = [_pts(models[key]) for key in keys]
    index = _farthest(pts_list, k, rule, None, None)
    return {key: p[i].astype(np.float32).tolist() for key, p, i in zip(keys, pts_list, index)}
