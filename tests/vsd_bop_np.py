"""numpy restatement of VSD over a vector of misalignment tolerances (pp_vsd_multi_f64, csrc/vsd.hip), one problem at a
time: the distance images of depth_im_to_dist_im, both visibility rules ('bop18': the reference's estimate_visib_mask, a
pixel without sensor depth is never visible; 'bop19': BOP 2019's, a rendered pixel without sensor depth is visible), both
pixel costs and the pixel counts.  Written from the definitions; tests/test_vsd_bop_cpu.py pins it in mode 'bop18' to the
values the reference's own vsd() wrote into tests/golden/pose_metrics.npz before any kernel is compared with it."""
import numpy as np


def dist_im(depth, K):
    """depth image [h,w] -> distance from the camera centre per pixel, float64: |((c - cx) d / fx, (r - cy) d / fy, d)|, the
    squares summed x, y, z in order; 0 where d is 0"""
    d = np.asarray(depth).astype(np.float64)
    K = np.asarray(K, np.float64)
    h, w = d.shape
    c = np.arange(w, dtype=np.float64)[None, :]
    r = np.arange(h, dtype=np.float64)[:, None]
    X = ((c - K[0, 2]) * d) * (1.0 / K[0, 0])
    Y = ((r - K[1, 2]) * d) * (1.0 / K[1, 1])
    return np.sqrt((X * X + Y * Y) + d * d)


def visib_mask(d_test, d_model, delta, visib_mode):
    """the visibility test in float32, as both rules have it"""
    near = (d_model.astype(np.float32) - d_test.astype(np.float32)) <= np.float32(delta)
    if visib_mode == "bop18":
        return (d_test > 0) & (d_model > 0) & near
    if visib_mode == "bop19":
        return (d_model > 0) & (near | (d_test == 0))
    raise ValueError(visib_mode)


def vsd_multi_one(depth_test, depth_est, depth_gt, K, delta, taus, cost_type="step", visib_mode="bop19"):
    """-> (e float64 [T], |inter|, |union|, |visib_gt|, |d_gt > 0|)"""
    taus = np.asarray(taus, np.float64).reshape(-1)
    d_t, d_e, d_g = (dist_im(x, K) for x in (depth_test, depth_est, depth_gt))
    vg = visib_mask(d_t, d_g, delta, visib_mode)
    ve = visib_mask(d_t, d_e, delta, visib_mode) | (vg & (d_e > 0))
    inter, union = vg & ve, vg | ve
    n_inter, n_union = int(inter.sum()), int(union.sum())
    d = np.abs(d_g[inter] - d_e[inter])
    e = np.ones(len(taus), np.float64)
    for i, tau in enumerate(taus):
        if cost_type == "step":
            cost = int((d >= tau).sum())
        elif cost_type == "tlinear":
            cost = np.minimum(d * (1.0 / tau), 1.0).sum()
        else:
            raise ValueError(cost_type)
        if n_union > 0:
            e[i] = (cost + (n_union - n_inter)) / float(n_union)
    return e, n_inter, n_union, int(vg.sum()), int((d_g > 0).sum())


def vsd_multi(depth_test, depth_est, depth_gt, K, delta, taus, cost_type="step", visib_mode="bop19"):
    """n problems: depth_est / depth_gt [n,h,w], depth_test [h,w] or [n,h,w], K 3x3 -> (e [n,T], inter, union, visib_gt,
    px_gt: int64 [n])"""
    depth_test = np.asarray(depth_test)
    rows = [vsd_multi_one(depth_test if depth_test.ndim == 2 else depth_test[i], depth_est[i], depth_gt[i], K, delta, taus,
                          cost_type, visib_mode) for i in range(len(depth_est))]
    return (np.stack([r[0] for r in rows]),) + tuple(np.array([r[k] for r in rows], np.int64) for k in range(1, 5))
