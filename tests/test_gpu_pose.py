"""GPU: pp_pose_add_f64 / pp_pose_adi_f64 through the C ABI against the reference's vectors and the oracle."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "pose_error.npz"))


@pytest.fixture(scope="module")
def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


def test_add_adi_match_reference_vectors(ctx):
    from pyrapose_amd import ops
    from pyrapose_amd.utils import pose_error as PE
    for c in G["cases"]:
        k = lambda n: G["c%d_%s" % (c, n)]
        dev = lambda n: torch.from_numpy(k(n)).cuda()
        for sym, key in ((False, "add"), (True, "adi")):
            got = ops.pose_errors(ctx, dev("pts"), dev("R_est"), dev("t_est"), dev("R_gt"), dev("t_gt"), sym).cpu().numpy()
            np.testing.assert_allclose(got, k(key), rtol=1e-12, atol=1e-15)
            # the evaluation decision (linemod_eval.py:530: err < 0.1 * diameter) for a sweep of diameters
            for dia in (0.05, 0.1, 0.2, 0.5, 1.0):
                assert np.array_equal(got < 0.1 * dia, k(key) < 0.1 * dia)
        # reference-named single-pose functions (numpy in, float out)
        assert abs(PE.add(k("R_est")[0], k("t_est")[0], k("R_gt")[0], k("t_gt")[0], k("pts")) - k("add")[0]) <= 1e-12 * max(k("add")[0], 1e-3)
        assert abs(PE.adi(k("R_est")[0], k("t_est")[0].reshape(3, 1), k("R_gt")[0], k("t_gt")[0].reshape(3, 1), k("pts")) - k("adi")[0]) <= 1e-12 * max(k("adi")[0], 1e-3)


def test_large_model_matches_oracle_and_is_deterministic(ctx):
    from oracle import pose_np as P
    from pyrapose_amd import ops
    rng = np.random.default_rng(3)
    pts = rng.standard_normal((5003, 3)) * 0.07
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    R_gt = np.stack([np.eye(3), q * np.sign(np.linalg.det(q))])
    R_est = np.stack([q * np.sign(np.linalg.det(q)), np.eye(3)])
    t_gt = rng.uniform(-0.1, 0.1, (2, 3)); t_est = t_gt + 0.01
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for sym, fn in ((False, P.add), (True, P.adi)):
        a = ops.pose_errors(ctx, dev(pts), dev(R_est), dev(t_est), dev(R_gt), dev(t_gt), sym)
        b = ops.pose_errors(ctx, dev(pts), dev(R_est), dev(t_est), dev(R_gt), dev(t_gt), sym)
        assert torch.equal(a, b)
        want = np.array([fn(R_est[i], t_est[i], R_gt[i], t_gt[i], pts) for i in range(2)])
        np.testing.assert_allclose(a.cpu().numpy(), want, rtol=1e-12)


def test_bad_arguments(ctx):
    from pyrapose_amd.utils import pose_error as PE
    with pytest.raises(ValueError):
        PE.add(np.eye(3), np.zeros(3), np.eye(3), np.zeros(3), np.zeros((4, 2)))


def _reproj_np(K, R_est, t_est, R_gt, t_gt, pts):
    """the reference's reproj (pose_error.py:179-207): float64 projections stored as float32 pixels, float32 norm; the mean is
    taken in float64 as the device does (utils.pose_error.reproj_batch)"""
    px = []
    for R, t in ((R_est, t_est), (R_gt, t_gt)):
        h = np.asarray(K, np.float64).dot((R.dot(pts.T) + t.reshape(3, 1)))
        px.append(np.stack([h[0] / h[2], h[1] / h[2]], 1).astype(np.float32))
    return float(np.linalg.norm(px[0] - px[1], axis=1).astype(np.float64).mean())


@pytest.mark.parametrize("n_pts", [1, 255, 256, 257, 513])  # below, at and past one 256-point tile; three tiles
def test_tile_sums_at_tile_boundaries(ctx, n_pts):
    """ADD / ADI / reproj with 3 poses at point counts around the shared 256-wide tile sum: against the float64 numpy
    expressions at the tolerances of the tests above (ADD / ADI) and of test_gpu_pose_metrics (reproj), twice with equal bits."""
    from oracle import pose_np as P
    from pyrapose_amd import ops
    rng = np.random.default_rng(100 + n_pts)
    pts = rng.standard_normal((n_pts, 3)) * np.array([0.05, 0.03, 0.02])
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    rots = []
    for _ in range(4):
        q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
        rots.append(q * np.sign(np.linalg.det(q)))
    R_gt = np.stack([np.eye(3), rots[0], rots[1]])
    R_est = np.stack([rots[2], rots[0], rots[3]])
    t_gt = rng.uniform(-0.1, 0.1, (3, 3)) + np.array([0.0, 0.0, 0.8])
    t_est = t_gt + np.array([[0.01, 0.01, 0.01], [0.002, -0.003, 0.01], [-0.02, 0.01, 0.04]])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for sym, fn in ((False, P.add), (True, P.adi)):
        a = ops.pose_errors(ctx, dev(pts), dev(R_est), dev(t_est), dev(R_gt), dev(t_gt), sym)
        b = ops.pose_errors(ctx, dev(pts), dev(R_est), dev(t_est), dev(R_gt), dev(t_gt), sym)
        assert torch.equal(a, b)
        want = np.array([fn(R_est[i], t_est[i], R_gt[i], t_gt[i], pts) for i in range(3)])
        np.testing.assert_allclose(a.cpu().numpy(), want, rtol=1e-12)
    K9 = np.repeat(K[None], 3, 0)
    a = ops.pose_reproj(ctx, dev(pts), dev(K9), dev(R_est), dev(t_est), dev(R_gt), dev(t_gt))
    b = ops.pose_reproj(ctx, dev(pts), dev(K9), dev(R_est), dev(t_est), dev(R_gt), dev(t_gt))
    assert torch.equal(a, b)
    want = np.array([_reproj_np(K, R_est[i], t_est[i], R_gt[i], t_gt[i], pts) for i in range(3)])
    np.testing.assert_allclose(a.cpu().numpy(), want, rtol=1e-5, atol=1e-6)
