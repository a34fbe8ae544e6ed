"""Mirror of the pose-error functions the evaluation loops call (utils/pose_error.py:43-75, 105-275;
utils/linemod_eval.py:525-531, tless_eval.py:470-471, 651-662): same names, arguments and float return values, computed by the
HIP kernels (ADD / ADI / reproj in csrc/pose.hip, VSD in csrc/vsd.hip on depth images from utils.renderer); re / te and
depth_im_to_dist_im stay on the host in numpy.  mssd / mspd are BOP's symmetry-aware errors (bop_toolkit_lib.pose_error), also
in csrc/pose.hip, over the symmetry sets of utils/symmetry.py; vsd_multi_* score VSD at up to 16 misalignment tolerances in one
pass with BOP 2019's visibility rule (AR_VSD), and visib_fract_batch gives the visible fraction of an annotation."""
import math

import numpy as np
import torch

from .. import ops
from ..runtime import default_context
from ._host import k4, per_pose, to_device


def transform_pts_Rt(pts, R, t):
    """pose_error.py:64-75 (host: a 3x3 product is not worth a launch)."""
    pts = np.asarray(pts)
    assert pts.shape[1] == 3
    return (np.asarray(R).dot(pts.T) + np.asarray(t).reshape((3, 1))).T


def _one(R_est, t_est, R_gt, t_gt, pts, symmetric):
    pts = np.asarray(pts)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("pts must be n x 3")
    out = ops.pose_errors(default_context(), to_device(pts), to_device(R_est, shape=(1, 3, 3)), to_device(t_est, shape=(1, 3)),
                          to_device(R_gt, shape=(1, 3, 3)), to_device(t_gt, shape=(1, 3)), symmetric)
    return float(out.cpu()[0])


def add(R_est, t_est, R_gt, t_gt, pts):
    """Average Distance of Model Points (pose_error.py:210-228)."""
    return _one(R_est, t_est, R_gt, t_gt, pts, False)


def adi(R_est, t_est, R_gt, t_gt, pts):
    """Average Distance to the nearest model point, for objects with indistinguishable views (pose_error.py:231-246)."""
    return _one(R_est, t_est, R_gt, t_gt, pts, True)


def add_batch(R_est, t_est, R_gt, t_gt, pts, symmetric=False):
    """n poses of one object in one launch: R_* [n,3,3], t_* [n,3] -> float64 [n]."""
    return ops.pose_errors(default_context(), to_device(pts), to_device(R_est), to_device(t_est, shape=(-1, 3)), to_device(R_gt),
                           to_device(t_gt, shape=(-1, 3)), symmetric).cpu().numpy()


def _poses(R_est, t_est, R_gt, t_gt):
    R_est = np.asarray(R_est, np.float64).reshape(-1, 3, 3)
    n = R_est.shape[0]
    return (R_est, np.asarray(t_est, np.float64).reshape(n, 3), np.asarray(R_gt, np.float64).reshape(n, 3, 3),
            np.asarray(t_gt, np.float64).reshape(n, 3))


def reproj_batch(K, R_est, t_est, R_gt, t_gt, pts):
    """reproj() of n poses of one object in one launch: K 3x3 or [n,3,3], R_* [n,3,3], t_* [n,3] -> float64 [n] (pixels).
    Projections are rounded to float32 and the norm is taken in float32 as the reference does; the mean is summed in float64,
    so values agree with the reference's float32 mean within 1e-5 relative."""
    pts = np.asarray(pts, np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError("pts must be n x 3")
    R_est, t_est, R_gt, t_gt = _poses(R_est, t_est, R_gt, t_gt)
    poses = [to_device(a) for a in (per_pose(K, R_est.shape[0], (3, 3)), R_est, t_est, R_gt, t_gt)]
    return ops.pose_reproj(default_context(), to_device(pts), *poses).cpu().numpy()


def reproj(K, R_est, t_est, R_gt, t_gt, pts):
    """Mean 2-D reprojection error in pixels (pose_error.py:179-207)."""
    return float(reproj_batch(K, R_est, t_est, R_gt, t_gt, pts)[0])


def _sym_batch(op, R_est, t_est, R_gt, t_gt, pts, syms, K, return_sym):
    from .symmetry import stack_symmetries
    pts = np.asarray(pts, np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError("pts must be n x 3")
    S_R, S_t = stack_symmetries(syms)
    R_est, t_est, R_gt, t_gt = _poses(R_est, t_est, R_gt, t_gt)
    poses = [to_device(a) for a in (R_est, t_est, R_gt, t_gt)]
    if K is not None:
        poses.insert(0, to_device(per_pose(K, R_est.shape[0], (3, 3))))
    err, sym = op(default_context(), to_device(pts), to_device(S_R), to_device(S_t), *poses, best_sym=return_sym)
    return (err.cpu().numpy(), sym.cpu().numpy()) if return_sym else err.cpu().numpy()


def mssd_batch(R_est, t_est, R_gt, t_gt, pts, syms, return_sym=False):
    """mssd() of n poses of one object in one launch: R_* [n,3,3], t_* [n,3], syms: a list from
    utils.symmetry.get_symmetry_transformations, an (S_R, S_t) pair or None (the identity) -> float64 [n]; with return_sym also
    int32 [n], the index of the symmetry that attains each minimum (the lowest on ties)."""
    return _sym_batch(ops.pose_mssd, R_est, t_est, R_gt, t_gt, pts, syms, None, return_sym)


def mspd_batch(R_est, t_est, R_gt, t_gt, K, pts, syms, return_sym=False):
    """mspd() of n poses of one object in one launch: K 3x3 or [n,3,3], the rest as mssd_batch -> float64 [n] (pixels)."""
    return _sym_batch(ops.pose_mspd, R_est, t_est, R_gt, t_gt, pts, syms, K, return_sym)


def mssd(R_est, t_est, R_gt, t_gt, pts, syms):
    """Maximum Symmetry-Aware Surface Distance (bop_toolkit_lib.pose_error.mssd, its argument order; parity with bop_toolkit
    unpinned): min over the symmetry transformations S of max over the model points of |P_est x - P_gt S x|."""
    return float(mssd_batch(R_est, t_est, R_gt, t_gt, pts, syms)[0])


def mspd(R_est, t_est, R_gt, t_gt, K, pts, syms):
    """Maximum Symmetry-Aware Projection Distance in pixels (bop_toolkit_lib.pose_error.mspd, its argument order; parity with
    bop_toolkit unpinned): as mssd() between the projections with K, in float64."""
    return float(mspd_batch(R_est, t_est, R_gt, t_gt, K, pts, syms)[0])


def re(R_est, R_gt):
    """Rotational error in degrees (pose_error.py:249-262): the angle of R_est inv(R_gt), its cosine clipped to [-1, 1]."""
    R_est, R_gt = np.asarray(R_est), np.asarray(R_gt)
    if not R_est.shape == R_gt.shape == (3, 3):
        raise ValueError("re: R_est and R_gt must be 3 x 3")
    c = 0.5 * (np.trace(R_est.dot(np.linalg.inv(R_gt))) - 1.0)
    c = min(1.0, max(-1.0, c))
    return 180.0 * math.acos(c) / np.pi


def te(t_est, t_gt):
    """Translational error (pose_error.py:265-275), in the unit of t."""
    t_est, t_gt = np.asarray(t_est), np.asarray(t_gt)
    if not t_est.size == t_gt.size == 3:
        raise ValueError("te: t_est and t_gt must hold 3 values")
    return float(np.linalg.norm(t_gt.reshape(3) - t_est.reshape(3)))


def re_batch(R_est, R_gt):
    """re() of n pose pairs: [n,3,3] x2 -> float64 [n] degrees (each value is what re() returns for that pair)."""
    R_est, R_gt = np.asarray(R_est).reshape(-1, 3, 3), np.asarray(R_gt).reshape(-1, 3, 3)
    return np.array([re(a, b) for a, b in zip(R_est, R_gt)], np.float64)


def te_batch(t_est, t_gt):
    """te() of n pose pairs: [n,3] x2 -> float64 [n]."""
    t_est, t_gt = np.asarray(t_est).reshape(-1, 3), np.asarray(t_gt).reshape(-1, 3)
    return np.array([te(a, b) for a, b in zip(t_est, t_gt)], np.float64)


def depth_im_to_dist_im(depth_im, K):
    """Depth image -> distance image (pose_error.py:43-61), host numpy: per pixel (x, y) the length of
    ((x - cx) d / fx, (y - cy) d / fy, d), 0 where d is 0."""
    d = np.asarray(depth_im)
    K = np.asarray(K, np.float64)
    h, w = d.shape
    xs = np.tile(np.arange(w), [h, 1])
    ys = np.tile(np.arange(h), [w, 1]).T
    X = np.multiply(xs - K[0, 2], d) * (1.0 / K[0, 0])
    Y = np.multiply(ys - K[1, 2], d) * (1.0 / K[1, 1])
    return np.linalg.norm(np.dstack((X, Y, d)), axis=2)


def vsd_from_depth(depth_test, depth_est, depth_gt, K, delta, tau, cost_type="step", return_counts=False):
    """VSD of n problems from depth images already rendered: depth_est / depth_gt [n,h,w] (numpy or cuda tensors),
    depth_test [h,w] shared by all of them or [n,h,w] (float32 or uint16), K 3x3 or [n,3,3] -> float64 [n]; with
    return_counts also the intersection and union pixel counts."""
    de, dg, dt = (to_device(a, torch.float32) for a in (depth_est, depth_gt, depth_test))
    if de.dim() == 2:
        de, dg = de[None], dg[None]
    if de.dim() != 3 or dg.shape != de.shape:
        raise ValueError("vsd: depth_est and depth_gt must be [n,h,w] of one shape")
    e, inter, uni = ops.vsd(default_context(), dt, de, dg, to_device(k4(K, de.shape[0])), delta, tau, cost_type)
    e = e.cpu().numpy()
    return (e, inter.cpu().numpy(), uni.cpu().numpy()) if return_counts else e


def render_pairs(R_est, t_est, R_gt, t_gt, model, depth_test, K, clip_near=100, clip_far=10000):
    """The two depth renderings VSD needs of each of n poses of one object, in one render launch at the size of depth_test
    ([h,w] or [n,h,w]) -> (depth_est, depth_gt: cuda float32 [n,h,w], K as float64 [n,3,3])."""
    from .renderer import render_depth_batch
    R_est, t_est, R_gt, t_gt = _poses(R_est, t_est, R_gt, t_gt)
    n = R_est.shape[0]
    h, w = np.shape(depth_test)[-2:]
    Ks = per_pose(K, n, (3, 3))
    depth = render_depth_batch(model, (w, h), np.concatenate([Ks, Ks]), np.concatenate([R_est, R_gt]), np.concatenate([t_est, t_gt]),
                               clip_near=clip_near, clip_far=clip_far)
    return depth[:n], depth[n:], Ks


def vsd_batch(R_est, t_est, R_gt, t_gt, model, depth_test, K, delta, tau, cost_type="step", clip_near=100, clip_far=10000,
              return_counts=False):
    """vsd() of n poses of one object: both depth renderings of every pose in one launch, then one VSD launch.  depth_test
    [h,w] (one scene) or [n,h,w]; K 3x3 or [n,3,3]; R_* [n,3,3], t_* [n,3] -> float64 [n]."""
    if cost_type not in ops.VSD_COSTS:
        raise ValueError("vsd: unknown pixel matching cost %r (step | tlinear)" % (cost_type,))
    depth_est, depth_gt, Ks = render_pairs(R_est, t_est, R_gt, t_gt, model, depth_test, K, clip_near, clip_far)
    return vsd_from_depth(depth_test, depth_est, depth_gt, Ks, delta, tau, cost_type, return_counts)


def vsd(R_est, t_est, R_gt, t_gt, model, depth_test, K, delta, tau, cost_type="step"):
    """Visible Surface Discrepancy (pose_error.py:105-176).  model: dict with 'pts' [n,3] and 'faces' [m,3] (utils.ply_loader);
    depth_test: the scene's depth image [h,w]; delta, tau in its unit (the reference calls it with 0.3 and 20, millimetres,
    and renders with clip_near=100, clip_far=10000)."""
    return float(vsd_batch(R_est, t_est, R_gt, t_gt, model, depth_test, K, delta, tau, cost_type)[0])


def vsd_multi_from_depth(depth_test, depth_est, depth_gt, K, delta, taus, cost_type="step", visib_mode="bop19", return_counts=False):
    """VSD of n problems at T misalignment tolerances (1 ... 16, positive, strictly increasing) from depth images already
    rendered, one pass over the pixels for all of them; arrays as in vsd_from_depth.  visib_mode 'bop18': the visibility rule
    of vsd(); 'bop19': BOP 2019's, under which a rendered pixel without sensor depth counts as visible -> float64 [n,T]; with
    return_counts also (intersection, union, visib_gt, px_gt), int64 [n] each: the last two are the pixels of the
    ground-truth visibility mask and of the ground-truth render."""
    de, dg, dt = (to_device(a, torch.float32) for a in (depth_est, depth_gt, depth_test))
    if de.dim() == 2:
        de, dg = de[None], dg[None]
    if de.dim() != 3 or dg.shape != de.shape:
        raise ValueError("vsd_multi: depth_est and depth_gt must be [n,h,w] of one shape")
    out = ops.vsd_multi(default_context(), dt, de, dg, to_device(k4(K, de.shape[0])), delta, taus, cost_type, visib_mode)
    e = out[0].cpu().numpy()
    return (e,) + tuple(c.cpu().numpy() for c in out[1:]) if return_counts else e


def vsd_multi_batch(R_est, t_est, R_gt, t_gt, model, depth_test, K, delta, taus, cost_type="step", visib_mode="bop19",
                    clip_near=100, clip_far=10000, return_counts=False):
    """vsd_batch at T tolerances: both depth renderings of every pose in one render launch, then one VSD launch for all taus
    -> float64 [n,T] (and the counts of vsd_multi_from_depth with return_counts)."""
    if cost_type not in ops.VSD_COSTS:
        raise ValueError("vsd_multi: unknown pixel matching cost %r (step | tlinear)" % (cost_type,))
    if visib_mode not in ops.VSD_VISIB:
        raise ValueError("vsd_multi: unknown visibility rule %r (bop18 | bop19)" % (visib_mode,))
    depth_est, depth_gt, Ks = render_pairs(R_est, t_est, R_gt, t_gt, model, depth_test, K, clip_near, clip_far)
    return vsd_multi_from_depth(depth_test, depth_est, depth_gt, Ks, delta, taus, cost_type, visib_mode, return_counts)


def visib_fract_batch(R_gt, t_gt, model, depth_test, K, delta=15.0, visib_mode="bop19", clip_near=100, clip_far=10000):
    """Visible fraction of n ground-truth poses of one object (what BOP's scene_gt_info.json calls visib_fract): pixels of the
    ground-truth visibility mask / pixels of the ground-truth render -> float64 [n], 0.0 where nothing is rendered.  One render
    launch and one VSD launch, the ground-truth render in both model slots."""
    from .renderer import render_depth_batch
    if visib_mode not in ops.VSD_VISIB:
        raise ValueError("visib_fract: unknown visibility rule %r (bop18 | bop19)" % (visib_mode,))
    R_gt = np.asarray(R_gt, np.float64).reshape(-1, 3, 3)
    n = R_gt.shape[0]
    t_gt = np.asarray(t_gt, np.float64).reshape(n, 3)
    h, w = np.shape(depth_test)[-2:]
    Ks = per_pose(K, n, (3, 3))
    depth = render_depth_batch(model, (w, h), Ks, R_gt, t_gt, clip_near=clip_near, clip_far=clip_far)
    _e, _inter, _uni, vis, px = vsd_multi_from_depth(depth_test, depth, depth, Ks, delta, [1.0], "step", visib_mode, True)
    return np.where(px > 0, vis / np.maximum(px, 1).astype(np.float64), 0.0)
