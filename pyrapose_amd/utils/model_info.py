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


def model_info(model):
    """One entry of a BOP models_info.json from a model (load_ply's dict, a path or an [n,3] array): diameter, min_x, min_y,
    min_z, size_x, size_y, size_z as floats; min and max are exact, size = max - min in float64."""
    pts = to_device(_pts(model))
    lo, hi = pts.min(dim=0).values.cpu().numpy(), pts.max(dim=0).values.cpu().numpy()
    d2, _ = ops.pts_diameter(default_context(), pts)
    info = {"diameter": math.sqrt(float(d2.cpu()[0]))}
    for a, axis in enumerate("xyz"):
        info["min_" + axis] = float(lo[a])
        info["size_" + axis] = float(hi[a] - lo[a])
    return info


def models_info(models):
    """{int id: model or path} -> {int id: model_info(model)}, the shape utils.symmetry.load_models_info returns (no symmetry
    entries: get_symmetry_transformations gives the identity for each)."""
    return {int(k): model_info(m) for k, m in models.items()}


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
