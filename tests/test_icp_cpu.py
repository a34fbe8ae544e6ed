"""CPU (no GPU): the numpy restatement of csrc/icp.hip (tests/icp_np.py) on analytic cases, and the C ABI of the ICP entry
points (header declarations and .so exports)."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np

from tests import icp_np as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ICP_ENTRIES = ["pp_cloud_from_depth_workspace_bytes", "pp_cloud_from_depth_f64", "pp_voxel_workspace_bytes", "pp_voxel_keys_f64",
               "pp_voxel_means_f64", "pp_estimate_normals_workspace_bytes", "pp_estimate_normals_f64", "pp_icp_workspace_bytes", "pp_icp_f64"]


def rot(axis, deg):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    th = math.radians(deg)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def asymmetric_cloud(n=300, seed=0):
    """points on an ellipsoid (semi-axes 60 / 40 / 25 mm) with a bump, off its centre, and their exact outward normals"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    ax = np.array([60.0, 40.0, 25.0])
    p = u * ax
    nrm = p / ax ** 2
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    b = rng.normal(size=(n // 3, 3))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    bump = b * 15.0 + np.array([55.0, 20.0, 0.0])
    keep = np.linalg.norm((bump / ax), axis=1) > 1.0
    return np.concatenate([p, bump[keep]]) + np.array([10.0, -5.0, 3.0]), np.concatenate([nrm, b[keep]])


def test_known_transform_is_recovered_in_both_modes():
    src, n = asymmetric_cloud()
    R, t = rot([1.0, 2.0, 0.5], 3.0), np.array([6.0, -5.0, 6.0])   # 3 degrees, |t| = 9.8 mm
    tgt = src @ R.T + t
    tn = n @ R.T
    for mode in ("point_to_plane", "point_to_point"):
        r = I.registration_icp(src, tgt, np.eye(4), 30.0, max_iteration=60, relative_fitness=1e-12, relative_rmse=1e-12,
                               estimation=mode, tgt_normals=tn)
        assert r["status"] == I.OK and r["fitness"] == 1.0
        assert np.abs(r["R"] - R).max() < 1e-9 and np.abs(r["t"] - t).max() < 1e-9, mode
        assert r["inlier_rmse"] < 1e-9 and np.array_equal(r["corr"], np.arange(len(src)))


def test_euler_update_is_orthonormal():
    rng = np.random.default_rng(1)
    for _ in range(50):
        U = I.euler_update(rng.uniform(-0.5, 0.5, 3))
        assert np.abs(U @ U.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(U) - 1.0) < 1e-14
    a, b, g = 0.1, -0.2, 0.3
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(g), -math.sin(g), 0], [math.sin(g), math.cos(g), 0], [0, 0, 1]])
    assert np.abs(I.euler_update([a, b, g]) - Rz @ Ry @ Rx).max() < 1e-15


def test_voxel_means_equal_a_brute_force_dictionary():
    rng = np.random.default_rng(2)
    p = rng.uniform(-40, 40, (2000, 3)) + np.array([0.0, 0.0, 700.0])
    nrm = rng.normal(size=p.shape)
    v = 5.0
    out, on, keys = I.voxel_down_sample(p, v, nrm)
    lo = p.min(0) - v * 0.5
    groups = {}
    for i, q in enumerate(p):
        groups.setdefault(tuple(np.floor((q - lo) / v).astype(int)), []).append(i)
    assert len(groups) == len(out) and np.all(np.diff(keys) > 0)
    for k, (ix, members) in enumerate(sorted(groups.items())):
        assert keys[k] == (ix[0] << 42) | (ix[1] << 21) | ix[2]
        np.testing.assert_allclose(out[k], p[members].mean(0), rtol=0, atol=1e-12)
        s = nrm[members].sum(0)
        np.testing.assert_allclose(on[k], s / np.linalg.norm(s), rtol=0, atol=1e-12)


def test_plane_normals_face_the_camera():
    g = np.stack(np.meshgrid(np.arange(-50, 51, 5.0), np.arange(-40, 41, 5.0)), -1).reshape(-1, 2)
    flat = np.concatenate([g, np.full((len(g), 1), 600.0)], 1)
    N, nb = I.estimate_normals(flat, 10.0, 10)
    assert np.abs(N - [0.0, 0.0, -1.0]).max() < 1e-12
    assert all(3 <= len(j) <= 10 for j in nb)
    R = rot([1.0, 0.3, 0.0], 30.0)
    tilt = (flat - [0, 0, 600.0]) @ R.T + [0, 0, 600.0]
    N, _ = I.estimate_normals(tilt, 10.0, 10)
    want = R @ [0.0, 0.0, -1.0]
    assert np.abs(N - want).max() < 1e-9 and np.all(np.einsum("ij,ij->i", N, tilt) < 0)
    N, _ = I.estimate_normals(flat[::50], 10.0, 10)                # isolated points: fewer than 3 neighbours
    assert not N.any()


def test_stopping_rule():
    # nine points far apart: every point's partner is its nearest target, so one Kabsch step is exact and the second changes
    # nothing -- the pass after it meets both relative thresholds
    s = np.array([[0, 0, 0], [100, 0, 0], [0, 70, 0], [0, 0, 50], [100, 70, 0], [100, 0, 50], [0, 70, 50], [80, 60, 45], [30, 10, 60.0]])
    R, t = rot([0.0, 1.0, 1.0], 2.0), np.array([3.0, 1.0, -2.0])
    tgt = s @ R.T + t
    kw = dict(estimation="point_to_point", relative_fitness=1e-6, relative_rmse=1e-6)
    r = I.registration_icp(s, tgt, np.eye(4), 50.0, max_iteration=30, **kw)
    assert r["iterations"] == 2 and r["status"] == I.OK and r["fitness"] == 1.0 and r["inlier_rmse"] < 1e-12
    assert np.abs(r["R"] - R).max() < 1e-12
    assert I.registration_icp(s, tgt, np.eye(4), 50.0, max_iteration=1, **kw)["iterations"] == 1
    r0 = I.registration_icp(s, tgt, np.eye(4), 50.0, max_iteration=0, **kw)
    assert r0["iterations"] == 0 and np.array_equal(r0["R"], np.eye(3)) and r0["inlier_rmse"] > 1.0
    assert I.registration_icp(s, s, np.eye(4), 50.0, max_iteration=30, **kw)["iterations"] == 1   # already aligned
    # fewer than 3 / 6 correspondences: the status and the initial pose
    r = I.registration_icp(s[:2], tgt[:2], np.eye(4), 50.0, **kw)
    assert r["status"] == I.TOO_FEW and r["iterations"] == 0
    src, n = asymmetric_cloud(seed=3)
    r = I.registration_icp(src[:5], src[:5] + 1.0, np.eye(4), 50.0, estimation="point_to_plane", tgt_normals=n[:5])
    assert r["status"] == I.TOO_FEW and np.array_equal(r["t"], np.zeros(3))


def test_create_point_cloud_restatement_matches_the_reference_expressions():
    rng = np.random.default_rng(4)
    d = rng.uniform(300, 900, (6, 7)).astype(np.float32)
    d[1, 2] = 0.0
    d[3, 4] = np.nan
    got = I.create_point_cloud(d, 500.0, 510.0, 3.2, 2.7, 1.0)
    rows, cols = d.shape
    zP = d.reshape(-1).astype(np.float64)
    x, y = np.meshgrid(np.arange(cols), np.arange(rows), indexing="xy")
    want = np.transpose(np.array(((x.reshape(-1) - 3.2) * zP / 500.0, (y.reshape(-1) - 2.7) * zP / 510.0, zP)))
    want[want[:, 2] == 0] = np.nan
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[1 * cols + 2]).all() and np.isnan(got[3 * cols + 4]).all()


def _header_functions():
    src = open(os.path.join(ROOT, "include", "pyrapose_hip.h")).read()
    return set(re.findall(r"\b(pp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))


def test_icp_entry_points_are_declared_and_exported():
    declared = _header_functions()
    for name in ICP_ENTRIES:
        assert name in declared, name
    from pyrapose_amd import _lib
    assert set(ICP_ENTRIES) <= set(_lib.EXPORTS)
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = set(line.split()[-1] for line in syms.splitlines() if line.strip())
    else:
        raw = ctypes.CDLL(_lib.LIB_PATH)
        exported = set(n for n in ICP_ENTRIES if hasattr(raw, n))
    for name in ICP_ENTRIES:
        assert name in exported, name
