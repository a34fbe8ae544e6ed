"""CPU (no GPU): the numpy restatement of csrc/wpnp.hip (tests/wpnp_np.py) -- its cost against the reference functor
(uncertainty_pnp/src/uncertainty_pnp.cpp:17-33) written out directly, its Jacobian against central differences, its minimum
against scipy's MINPACK Levenberg-Marquardt, the effect of the weights on 200 heteroscedastic scenes, the vote statistics
against numpy's own -- and the C ABI of the new entry points (header declarations, .so exports, _lib.EXPORTS)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
from scipy.optimize import least_squares

from tests import wpnp_np as W
from tests.wpnp_scenes import BOX, K4A, corner_problem, rot_err_deg, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WPNP_ENTRIES = ["pp_vote_stats_workspace_bytes", "pp_vote_stats_f64", "pp_pnp_refine_weighted_workspace_bytes",
                "pp_pnp_refine_weighted_f64"]
N_SCENES = 200
UNIT = np.tile([1.0, 0.0, 1.0], (8, 1))


def functor(pose, x2d, x3d, w3, fx, fy, px, py):
    """uncertainty_pnp.cpp:17-33 for one correspondence: ceres::AngleAxisRotatePoint (Rodrigues' formula on the point), add t,
    project, multiply by W"""
    w, th2 = pose[:3], float(pose[:3] @ pose[:3])
    if th2 > np.finfo(float).eps:
        th = np.sqrt(th2)
        k = w / th
        p = x3d * np.cos(th) + np.cross(k, x3d) * np.sin(th) + k * float(k @ x3d) * (1.0 - np.cos(th))
    else:
        p = x3d + np.cross(w, x3d)
    p = p + pose[3:]
    dx, dy = fx * p[0] / p[2] + px - x2d[0], fy * p[1] / p[2] + py - x2d[1]
    return np.array([w3[0] * dx + w3[1] * dy, w3[1] * dx + w3[2] * dy])


def test_residual_equals_the_reference_functor():
    rng = np.random.default_rng(0)
    for s in range(20):
        sc = scene(s)
        obj, mu, wg = corner_problem(sc)
        wg = wg + rng.normal(scale=0.05, size=wg.shape)
        x = np.concatenate([W.so3_log(sc["R0"]), sc["t0"]])
        got, _z = W.residuals(x, obj, mu, wg, K4A)
        want = np.stack([functor(x, mu[i], obj[i], wg[i], *K4A) for i in range(8)])
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the rotation logarithm and Rodrigues are inverse to each other, also near 0 and near pi
    for w in ([1e-14, 0, 0], [0.3, -1.2, 0.5], [0, 0, np.pi - 1e-9], [np.pi, 0, 0], [1e-5, 2e-5, -1e-5]):
        w = np.asarray(w, np.float64)
        assert np.abs(W.rodrigues(W.so3_log(W.rodrigues(w))) - W.rodrigues(w)).max() < 1e-12


def test_analytic_jacobian_equals_central_differences():
    """Central differences with step h: a truncation error of h^2 / 6 |f'''| and a rounding error of (error of f) / h.  f is a
    weighted pixel difference: its terms are below 1000 px, the weights below 2 (= 1 / sigma_floor), a handful of roundings:
    error of f <= 8 * 1000 * eps.  The third derivative is of the order of the first over the square of the parameter's scale
    (1 rad for the rotation vector, the depth, >= 600, for t; taken as 10 x to cover the constants).  Steps: 1e-5 of the scale,
    i.e. h = 1e-5 (rotation) and h = 6e-3 (translation), the step actually realised in floating point taken as the divisor.
    Bound per column k: 8000 eps / h_k + 10 (h_k / scale_k)^2 max |J[:, k]|  (1.8e-7 + 1e-9 max|J| for the rotation columns
    whose entries are in the hundreds, 3e-10 + 1e-9 max|J| for the translation columns whose entries are below 1)."""
    eps = np.finfo(np.float64).eps
    for s in range(20):
        sc = scene(s)
        obj, mu, wg = corner_problem(sc)
        x = np.concatenate([W.so3_log(sc["R0"]), sc["t0"]])
        J = W.jacobian(x, obj, mu, wg, K4A).reshape(-1, 6)
        for k in range(6):
            scale = 1.0 if k < 3 else 600.0
            e = np.zeros(6)
            e[k] = 1e-5 * scale
            xp, xm = x + e, x - e
            num = (W.residuals(xp, obj, mu, wg, K4A)[0] - W.residuals(xm, obj, mu, wg, K4A)[0]).reshape(-1) / (xp[k] - xm[k])
            err, bound = np.abs(num - J[:, k]).max(), 8000.0 * eps / e[k] + 10.0 * 1e-10 * np.abs(J[:, k]).max()
            assert err <= bound, (s, k, err, bound)


def test_minimum_is_where_scipy_lands():
    """Yardstick: scipy.optimize.least_squares(method='lm'), MINPACK's Levenberg-Marquardt, given the same residual and
    the analytic Jacobian, all tolerances 1e-15.  Measured on the 200 scenes: worst |dR| 1.5e-9 (absolute), worst |dt| / depth
    4.4e-10 (a numerical Jacobian in scipy gave 1.7e-8 for both); asserted: 10 x the measured worst values."""
    worst_R = worst_t = 0.0
    for s in range(N_SCENES):
        sc = scene(s)
        obj, mu, wg = corner_problem(sc)
        mine = W.refine_weighted(obj, mu, wg, K4A, sc["R0"], sc["t0"], 100, 1e-15, 1e-15, 1e-15)
        assert mine["status"] == W.CONVERGED
        x0 = np.concatenate([W.so3_log(sc["R0"]), sc["t0"]])
        ref = least_squares(lambda x: W.residuals(x, obj, mu, wg, K4A)[0].reshape(-1), x0,
                            jac=lambda x: W.jacobian(x, obj, mu, wg, K4A).reshape(-1, 6), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        worst_R = max(worst_R, np.abs(W.rodrigues(ref.x[:3]) - mine["R"]).max())
        worst_t = max(worst_t, np.abs(ref.x[3:] - mine["t"]).max() / mine["t"][2])
    print("worst difference to scipy: R %.3g, t / depth %.3g" % (worst_R, worst_t))
    assert worst_R < 1.5e-8 and worst_t < 4.4e-9


def test_weights_improve_the_pose_and_cost_never_rises():
    ew, eu = [], []
    for s in range(N_SCENES):
        sc = scene(s)
        obj, mu, wg = corner_problem(sc)
        a = W.refine_weighted(obj, mu, wg, K4A, sc["R0"], sc["t0"])
        u = W.refine_weighted(obj, mu, UNIT, K4A, sc["R0"], sc["t0"])
        for r in (a, u):
            assert r["status"] == W.CONVERGED and r["cost_final"] <= r["cost_init"] and 2 <= r["iterations"] <= 8
        ew.append(rot_err_deg(a["R"], sc["R"]))
        eu.append(rot_err_deg(u["R"], sc["R"]))
    ew, eu = np.asarray(ew), np.asarray(eu)
    print("median rotation error: weighted %.3f deg, unweighted %.3f deg; weighted better in %.1f %%" %
          (np.median(ew), np.median(eu), 100.0 * (ew < eu).mean()))
    assert np.median(ew) < np.median(eu) and (ew < eu).mean() > 0.75


def test_vote_stats_against_numpy():
    rng = np.random.default_rng(3)
    ks = [40, 7, 1, 0, 13]
    offs = np.concatenate([[0], np.cumsum([8 * k for k in ks])])
    img = rng.normal(scale=4.0, size=(offs[-1], 2)) + 300.0
    score = rng.uniform(0.5, 1.0, offs[-1] // 8)
    mask = (rng.uniform(size=offs[-1]) < 0.8).astype(np.uint8)
    mask[offs[4] + 3::8] = 0
    mask[offs[4] + 3] = 1                                  # corner 3 of the last problem: one vote left
    img[offs[1] + 5: offs[2]: 8] = [100.0, 50.0]          # corner 5 of problem 1: identical votes
    for sc_, mk in ((None, None), (score, None), (None, mask), (score, mask)):
        for mode in (W.FULL, W.ISO):
            st = W.vote_stats(img, offs, 8, sc_, mk, mode, 0.5)
            for p, k in enumerate(ks):
                for j in range(8):
                    idx = offs[p] + np.arange(k) * 8 + j
                    w = np.ones(k) if sc_ is None else sc_[offs[p] // 8: offs[p] // 8 + k].copy()
                    if mk is not None:
                        w = w * mk[idx]
                    keep = w > 0
                    assert st["count"][p, j] == keep.sum()
                    if keep.sum() == 0:
                        assert not st["wgt"][p, j].any() and st["wsum"][p, j] == 0.0
                        continue
                    xy, w = img[idx][keep], w[keep]
                    np.testing.assert_allclose(st["mu"][p, j], np.average(xy, axis=0, weights=w), rtol=1e-13)
                    np.testing.assert_allclose(st["n_eff"][p, j], w.sum() ** 2 / (w * w).sum(), rtol=1e-13)
                    if keep.sum() < 2:
                        assert not st["wgt"][p, j].any()       # the count < 2 rule, both modes
                        continue
                    C = np.atleast_2d(np.cov(xy.T, aweights=w, ddof=0))
                    np.testing.assert_allclose(st["cov"][p, j], [C[0, 0], C[0, 1], C[1, 1]], rtol=1e-9, atol=1e-12)
                    wxx, wxy, wyy = st["wgt"][p, j]
                    if mode == W.ISO:
                        want = 0.0 if C[0, 0] < 1e-5 else 1.0 / np.linalg.eigvalsh(C).max()
                        np.testing.assert_allclose([wxx, wxy, wyy], [want, 0.0, want], rtol=1e-9)
                    else:
                        Wm = np.array([[wxx, wxy], [wxy, wyy]])
                        Cm = C / st["n_eff"][p, j] + 0.25 * np.eye(2)
                        assert np.abs(Wm @ Cm @ Wm - np.eye(2)).max() < 1e-12
    st = W.vote_stats(img, offs, 8, None, None, W.ISO, 0.5)
    assert not st["wgt"][1, 5].any() and st["wgt"][1, 4, 0] > 0.0   # cov_xx < 1e-5
    st = W.vote_stats(img, offs, 8, None, None, W.FULL, 0.5)
    np.testing.assert_allclose(st["wgt"][1, 5], [2.0, 0.0, 2.0], rtol=1e-12)   # identical votes: the floor alone, 1 / 0.5


def test_every_status_is_reached():
    sc = scene(0)
    obj, mu, wg = corner_problem(sc)
    ok = W.refine_weighted(obj, mu, wg, K4A, sc["R0"], sc["t0"])
    assert ok["status"] == W.CONVERGED and np.abs(ok["pose_cov"] - ok["pose_cov"].T).max() < 1e-9 * np.abs(ok["pose_cov"]).max()
    r = W.refine_weighted(obj, mu, wg, K4A, sc["R0"], sc["t0"], max_iterations=1, function_tol=0.0)
    assert r["status"] == W.MAX_ITER and r["iterations"] == 2 and r["cost_final"] < r["cost_init"]
    r = W.refine_weighted(obj, mu, wg, K4A, sc["R0"], sc["t0"], max_iterations=0)
    assert r["status"] == W.MAX_ITER and r["iterations"] == 1 and r["cost_final"] == r["cost_init"]
    two = wg.copy()
    two[2:] = 0.0
    for r in (W.refine_weighted(obj, mu, two, K4A, sc["R0"], sc["t0"]), W.refine_weighted(obj[:0], mu[:0], wg[:0], K4A, sc["R0"], sc["t0"])):
        assert r["status"] == W.TOO_FEW and r["iterations"] == 0 and np.array_equal(r["R"], sc["R0"]) and np.array_equal(r["t"], sc["t0"])
    r = W.refine_weighted(obj, mu, wg, K4A, sc["R0"], sc["t0"] * [1, 1, -1])
    assert r["status"] == W.BEHIND and np.array_equal(r["R"], sc["R0"]) and not r["pose_cov"].any()
    r = W.refine_weighted(obj, mu, wg * 1e160, K4A, sc["R0"], sc["t0"])          # the normal equations overflow
    assert r["status"] == W.SINGULAR and np.array_equal(r["t"], sc["t0"])
    assert W.ldlt_solve(-np.eye(6), np.ones(6)) is None
    H = np.diag([4.0, 1, 1, 1, 1, 1]) + 0.1
    np.testing.assert_allclose(W.ldlt_solve(H, np.arange(6.0)), np.linalg.solve(H, np.arange(6.0)), rtol=1e-12)
    np.testing.assert_allclose(W.pose_covariance(H), np.linalg.inv(H), rtol=1e-12)


def _header_functions():
    src = open(os.path.join(ROOT, "include", "pyrapose_hip.h")).read()
    return set(re.findall(r"\b(pp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))


def test_wpnp_entry_points_are_declared_and_exported():
    declared = _header_functions()
    for name in WPNP_ENTRIES:
        assert name in declared, name
    from pyrapose_amd import _lib
    assert set(WPNP_ENTRIES) <= set(_lib.EXPORTS)
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = set(line.split()[-1] for line in syms.splitlines() if line.strip())
    else:
        raw = ctypes.CDLL(_lib.LIB_PATH)
        exported = set(n for n in WPNP_ENTRIES if hasattr(raw, n))
    for name in WPNP_ENTRIES:
        assert name in exported, name
