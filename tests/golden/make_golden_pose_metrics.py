#!/usr/bin/env python3
"""Golden vectors for reproj / re / te / VSD (test infrastructure, runs ONLY in the build container).

Loads the reference's unmodified ``PyraPose/utils/pose_error.py`` as make_golden_pose.py does (empty ``cv2`` /
``transforms3d`` stubs; reproj, re, te, vsd and the helpers they call use neither) and injects the module-level ``render``
that its vsd() calls (pose_error.py:124-128, import commented out at :12) as the numpy restatement of the depth renderer
(tests/render_np.py).  Writes tests/golden/pose_metrics.npz: inputs, the injected depth images, the reference's reproj / re
/ te values, its vsd for both cost types and several delta / tau (an empty union and a scene depth shared by all poses
included), and the intersection / union pixel counts from its own visibility-mask functions.  Nothing under tests/ with
``-m gpu`` reads /root/reference.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import render_np as RN  # noqa: E402
from tests.golden.make_golden_pose import load_reference, rot  # noqa: E402


def perturb(rng, R, t, ang, dt):
    w = rng.standard_normal(3)
    w *= ang / np.linalg.norm(w)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    dR = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    return dR @ R, t + rng.standard_normal(3) * dt


def main():
    ref = load_reference()
    rendered = []

    def render(model, im_size, K, R, t, clip_near=100, clip_far=10000, mode="depth"):
        assert mode == "depth"
        d = RN.render_depth(model["pts"], model["faces"], K, R, t, im_size[0], im_size[1], clip_near, clip_far)
        rendered.append(d)
        return d

    ref.render = render
    rng = np.random.default_rng(2027)
    out = {}

    # ---- reproj / re / te: 24 pose pairs on a 500-point model (metres), LineMOD-like K
    pts = rng.standard_normal((500, 3)) * np.array([0.05, 0.03, 0.02])
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    R_gt = np.stack([rot(rng) for _ in range(24)])
    t_gt = rng.uniform(-0.1, 0.1, (24, 3)) + np.array([0, 0, 0.8])
    R_est, t_est = [], []
    for i in range(24):
        ang = [0.0, 0.01, 0.05, 0.08, 0.2, 1.5][i % 6]
        dt = [0.0, 0.002, 0.01, 0.04, 0.1, 0.03][i % 6]
        R, t = perturb(rng, R_gt[i], t_gt[i], ang, dt) if ang > 0 else (R_gt[i].copy(), t_gt[i].copy())
        R_est.append(R)
        t_est.append(t)
    R_est, t_est = np.stack(R_est), np.stack(t_est)
    out.update(rt_pts=pts, rt_K=K, rt_R_est=R_est, rt_t_est=t_est, rt_R_gt=R_gt, rt_t_gt=t_gt)
    out["rt_reproj"] = np.array([ref.reproj(K, R_est[i], t_est[i], R_gt[i], t_gt[i], pts) for i in range(24)], np.float64)
    out["rt_re"] = np.array([ref.re(R_est[i], R_gt[i]) for i in range(24)], np.float64)
    out["rt_te"] = np.array([ref.te(t_est[i], t_gt[i]) for i in range(24)], np.float64)

    # ---- VSD: an ellipsoid mesh in millimetres, 128 x 96 images; the last case at 720 x 540
    cases = []
    mesh = RN.sphere_mesh(40.0, 10, 16, scale=(1.0, 0.7, 0.5))
    Ks = np.array([[300.0, 0.0, 63.7], [0.0, 310.0, 47.2], [0.0, 0.0, 1.0]])
    Kl = np.array([[1075.65, 0.0, 360.0], [0.0, 1073.90, 270.0], [0.0, 0.0, 1.0]])
    for ci, (w, h, Kc, n, shared) in enumerate([(128, 96, Ks, 6, False), (128, 96, Ks, 5, True), (720, 540, Kl, 2, False)]):
        R_gt = np.stack([rot(rng) for _ in range(n)])
        t_gt = np.stack([np.array([rng.uniform(-20, 20), rng.uniform(-15, 15), rng.uniform(450, 600)]) for _ in range(n)])
        if shared:  # one scene: the same object pose, several estimates against one depth image
            R_gt[:] = R_gt[0]
            t_gt[:] = t_gt[0]
        R_est, t_est = [], []
        for i in range(n):
            ang, dt = [(0.0, 0.0), (0.02, 1.0), (0.1, 5.0), (0.4, 15.0), (0.05, 3.0), (0.0, 0.0)][i % 6]
            R, t = perturb(rng, R_gt[i], t_gt[i], ang, dt) if ang > 0 else (R_gt[i].copy(), t_gt[i].copy())
            if ci == 0 and i == 5:  # est and gt both off-screen: empty union, e = 1
                t = t_gt[i] + np.array([5000.0, 0.0, 0.0])
                t_gt[i] = t_gt[i] + np.array([-5000.0, 0.0, 0.0])
            R_est.append(R)
            t_est.append(t)
        R_est, t_est = np.stack(R_est), np.stack(t_est)
        # scene depth: the object at its gt pose, millimetre sensor noise, a background plane, an occluding band
        depth_test = []
        for i in range(1 if shared else n):
            d = RN.render_depth(mesh["pts"], mesh["faces"], Kc, R_gt[i], t_gt[i], w, h)
            d = np.where(d > 0, np.round(d + rng.normal(0, 0.5, d.shape)), 900.0)
            d[: h // 5, :] = np.where(rng.uniform(size=(h // 5, w)) < 0.5, 0.0, d[: h // 5, :])   # missing sensor values
            d[:, w // 2: w // 2 + w // 10] = np.minimum(d[:, w // 2: w // 2 + w // 10], 420.0)     # an occluder
            depth_test.append(d.astype(np.float32))
        depth_test = np.stack(depth_test)
        vals, inter, union, dest, dgt = [], [], [], [], []
        params = [("step", 0.3, 20.0), ("step", 15.0, 5.0), ("tlinear", 0.3, 20.0), ("tlinear", 15.0, 5.0)]
        for i in range(n):
            dt_i = depth_test[0 if shared else i]
            row = []
            for cost, delta, tau in params:
                rendered.clear()
                row.append(ref.vsd(R_est[i], t_est[i], R_gt[i], t_gt[i], mesh, dt_i, Kc, delta, tau, cost))
                de_i, dg_i = rendered
            dest.append(de_i)
            dgt.append(dg_i)
            vals.append(row)
            ci_, cu_ = [], []
            for _cost, delta, _tau in params:
                d_t, d_g, d_e = (ref.depth_im_to_dist_im(x, Kc) for x in (dt_i, dg_i, de_i))
                vg = ref.estimate_visib_mask_gt(d_t, d_g, delta)
                ve = ref.estimate_visib_mask_est(d_t, d_e, vg, delta)
                ci_.append(int(np.logical_and(vg, ve).sum()))
                cu_.append(int(np.logical_or(vg, ve).sum()))
            inter.append(ci_)
            union.append(cu_)
        p = "v%d_" % ci
        out.update({p + "K": Kc, p + "R_est": R_est, p + "t_est": t_est, p + "R_gt": R_gt, p + "t_gt": t_gt,
                    p + "depth_test": depth_test, p + "depth_est": np.stack(dest), p + "depth_gt": np.stack(dgt),
                    p + "vsd": np.array(vals, np.float64), p + "inter": np.array(inter, np.int64), p + "union": np.array(union, np.int64),
                    p + "wh": np.array([w, h]), p + "shared": np.array(shared)})
        cases.append(ci)
    out["vsd_cases"] = np.array(cases)
    out["vsd_cost"] = np.array([c for c, _, _ in params])
    out["vsd_delta"] = np.array([d for _, d, _ in params])
    out["vsd_tau"] = np.array([t for _, _, t in params])
    out["mesh_pts"] = mesh["pts"]
    out["mesh_faces"] = mesh["faces"]
    path = os.path.join(HERE, "pose_metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for c in cases:
        print(c, out["v%d_vsd" % c].round(4).tolist(), out["v%d_union" % c][:, 0].tolist())


if __name__ == "__main__":
    main()
