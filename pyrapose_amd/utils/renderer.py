"""Depth rendering of a triangle mesh on the device, in place of the OpenGL depth pass of utils/hodan_renderer.py that the
reference's vsd() calls as render(model, im_size, K, R, t, clip_near=100, clip_far=10000, mode='depth')
(utils/pose_error.py:124-128).  Pixel (r, c) holds the camera-frame Z of the nearest surface point through (c + 0.5, r + 0.5)
in OpenCV pixel coordinates, 0 where the mesh does not cover it (csrc/render.hip).  Only mode='depth' exists."""
import numpy as np
import torch

from .. import ops
from ..runtime import default_context
from ._host import k4, to_device


def _mesh(model):
    pts = np.asarray(model["pts"], np.float64)
    faces = np.asarray(model["faces"])
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError("model['pts'] must be n x 3")
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError("model['faces'] must be m x 3 (triangles only)")
    fi = faces.astype(np.int64)
    if not np.array_equal(fi, faces) or fi.min() < 0 or fi.max() >= pts.shape[0]:
        raise ValueError("model['faces'] must hold vertex indices in [0, %d)" % pts.shape[0])
    return pts, fi.astype(np.int32)


def render_depth_batch(model, im_size, K, R, t, clip_near=100, clip_far=10000, ctx=None):
    """n poses of one mesh in one launch: model dict ('pts' [n_v,3], 'faces' [n_f,3]), im_size (w, h), K 3x3 or [n,3,3],
    R [n,3,3], t [n,3] (the unit of pts) -> cuda float32 tensor [n, h, w]."""
    w, h = (int(v) for v in im_size)
    pts, faces = _mesh(model)
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    n = R.shape[0]
    return ops.render_depth(ctx or default_context(), to_device(pts), to_device(faces, torch.int32), to_device(R), to_device(t, shape=(n, 3)),
                            to_device(k4(K, n)), w, h, float(clip_near), float(clip_far))


def render(model, im_size, K, R, t, clip_near=100, clip_far=10000, mode="depth", ambient_weight=0.5, surf_color=None,
           shading="phong"):
    """One depth image [h, w] float32 (numpy), im_size = (w, h); the signature vsd() calls.  The colour arguments of the
    reference's renderer are accepted for signature compatibility and must stay at their defaults: RGB is not rendered."""
    if mode != "depth":
        raise ValueError("render: only mode='depth' is implemented (got %r)" % (mode,))
    return render_depth_batch(model, im_size, K, R, t, clip_near, clip_far)[0].cpu().numpy()
