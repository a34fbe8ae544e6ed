"""Uncertainty-weighted PnP: the reference's uncertainty_pnp/un_pnp_utils.py (module name and signatures), on the device.

There the solver is a Ceres problem behind cffi (src/uncertainty_pnp.cpp) and cannot be built from the reference tree; here
it is csrc/wpnp.hip: the same cost function (residual W (proj(R x + t) - u) with the symmetric 2x2 weight W = [[wxx, wxy],
[wxy, wyy]]), this library's own Levenberg-Marquardt -- parity with Ceres unpinned, the cost and its minimum pinned
(DESIGN.md 7b).  Deviation: the reference seeds with cv2.solvePnP(P3P) on the four heaviest points (:27-31, :90-93); here
the seed is `init=(R, t)` or, when absent, utils.pnp.solve_pnp_batch(..., points_per_vote=0) on the points with a non-zero
weight.  pn == 4 returns the seed, as there (:33-37)."""
import numpy as np
import torch

from .. import ops
from ..runtime import default_context
from . import pnp
from ._host import k4, pack_ragged, to_device

STATUS_NAMES = ("converged", "max_iterations", "too_few", "singular", "behind")


def uncertainty_pnp_batch(problems, init=None, max_iterations=50, gradient_tol=1e-10, parameter_tol=1e-8, function_tol=1e-6,
                          seed=0, ctx=None):
    """problems: list of (points_2d [pn,2], weights_2d [pn,3] = wxx, wxy, wyy, points_3d [pn,3], camera_matrix 3x3);
    init: None or a list with one (R [3,3], t [3]) or None per problem.  ONE launch of the solver (plus one RANSAC launch for
    the problems without a seed).  -> list of dicts: R, t, cost, cost_init, iterations, status (ops.WPNP_*), pose_cov [6,6]
    in (rotation vector, translation) order, seeded (False when no seed was found: the pose is then the identity)."""
    if not problems:
        return []
    ctx = ctx or default_context()
    P = len(problems)
    init = list(init) if init is not None else [None] * P
    if len(init) != P:
        raise ValueError("uncertainty_pnp_batch: one init (or None) per problem")
    p2, w2, p3, Ks = [], [], [], []
    for pts2, wts, pts3, K in problems:
        pts2 = np.asarray(pts2, np.float64).reshape(-1, 2)
        wts, pts3 = np.asarray(wts, np.float64), np.asarray(pts3, np.float64).reshape(-1, 3)
        if wts.shape != (pts2.shape[0], 3) or pts3.shape[0] != pts2.shape[0]:
            raise ValueError("uncertainty_pnp_batch: need points_2d [pn,2], weights_2d [pn,3], points_3d [pn,3]")
        p2.append(pts2); w2.append(wts); p3.append(pts3); Ks.append(k4(K))
    need = [p for p in range(P) if init[p] is None]
    seeded = [True] * P
    if need:
        live = [(w2[p] != 0).any(1) for p in need]
        got = pnp.solve_pnp_batch([(p3[p][m], p2[p][m], problems[p][3]) for p, m in zip(need, live)],
                                  seed=seed, points_per_vote=0, ctx=ctx)
        for p, (ok, R, t, _inl) in zip(need, got):
            init[p], seeded[p] = (R, t), bool(ok)
    R0 = np.stack([np.asarray(i[0], np.float64).reshape(3, 3) for i in init])
    t0 = np.stack([np.asarray(i[1], np.float64).reshape(3) for i in init])
    offs, obj = pack_ragged(p3)
    r = ops.pnp_refine_weighted(ctx, to_device(offs, torch.int32), to_device(obj), to_device(np.concatenate(p2)), to_device(np.concatenate(w2)),
                                to_device(Ks), to_device(R0), to_device(t0), max_iterations, gradient_tol, parameter_tol, function_tol)
    r = {k: v.cpu().numpy() for k, v in r.items()}
    out = []
    for p in range(P):
        keep = len(p2[p]) == 4 or not seeded[p]  # un_pnp_utils.py:33-37: no other points, the seed is the answer
        out.append(dict(R=R0[p] if keep else r["R"][p], t=t0[p] if keep else r["t"][p], cost=float(r["cost_init" if keep else "cost_final"][p]),
                        cost_init=float(r["cost_init"][p]), iterations=int(r["iterations"][p]), status=int(r["status"][p]),
                        pose_cov=r["pose_cov"][p], seeded=seeded[p]))
    return out


def uncertainty_pnp(points_2d, weights_2d, points_3d, camera_matrix, init=None):
    """un_pnp_utils.py:6-57: points_2d [pn,2], weights_2d [pn,3] (wxx, wxy, wyy), points_3d [pn,3], camera_matrix [3,3]
    -> Rt [3,4]"""
    pn = points_2d.shape[0]
    assert points_3d.shape[0] == pn and pn >= 4
    r = uncertainty_pnp_batch([(points_2d, weights_2d, points_3d, camera_matrix)], None if init is None else [init])[0]
    return np.concatenate([r["R"], r["t"].reshape(3, 1)], axis=-1)


def weights_from_covars(covars):
    """the weight rule of uncertainty_pnp_v2 (un_pnp_utils.py:75-83, 103-104): [pn,2,2] -> [pn,3] = (w, 0, w) with
    w = 1 / lambda_max, 0 where covars[:, 0, 0] < 1e-5"""
    covars = np.asarray(covars, np.float64).reshape(-1, 2, 2)
    w = np.zeros(len(covars))
    for pi in range(len(covars)):
        if not covars[pi, 0, 0] < 1e-5:
            w[pi] = 1.0 / np.max(np.linalg.eigvals(covars[pi]).real)
    return np.stack([w, np.zeros_like(w), w], 1)


def uncertainty_pnp_v2(points_2d, covars, points_3d, camera_matrix, init=None):
    """un_pnp_utils.py:60-121: covars [pn,2,2] -> Rt [3,4]"""
    pn = points_2d.shape[0]
    assert points_3d.shape[0] == pn and pn >= 4 and covars.shape[0] == pn
    return uncertainty_pnp(points_2d, weights_from_covars(covars), points_3d, camera_matrix, init)
