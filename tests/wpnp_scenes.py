"""Seeded heteroscedastic scenes for the weighted-PnP tests: the cuboid and intrinsics of tests/test_oracle_pnp.py, k votes
per corner, every corner with its own anisotropic pixel noise (0.3-1 px along one axis, 2-8 px along the other, at a random
orientation) -- a corner the network pins down next to a corner whose votes smear along an edge."""
import numpy as np

from tests import wpnp_np as W
from tests.test_oracle_pnp import BOX, K4, project

K4A = np.asarray(K4, np.float64)


def rot_err_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))


def scene(seed, k=40, box=BOX):
    """-> dict(R, t truth; votes [k,8,2]; obj [8k,3]; img [8k,2]; R0, t0: a start 2 degrees / 1 % of the depth off)"""
    rng = np.random.default_rng(1000 + seed)
    R = W.rodrigues(rng.normal(size=3))
    t = np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(600, 1000)])
    uv = project(R, t, box)
    phi = rng.uniform(0, np.pi, 8)
    s_minor, s_major = rng.uniform(0.3, 1.0, 8), rng.uniform(2.0, 8.0, 8)
    e = rng.normal(size=(k, 8, 2)) * np.stack([s_major, s_minor], 1)[None]
    c, s = np.cos(phi), np.sin(phi)
    noise = np.stack([c * e[:, :, 0] - s * e[:, :, 1], s * e[:, :, 0] + c * e[:, :, 1]], 2)
    votes = uv[None] + noise
    ax = rng.normal(size=3)
    R0 = W.rodrigues(np.radians(2.0) * ax / np.linalg.norm(ax)) @ R
    t0 = t + 0.01 * t[2] * rng.uniform(-1, 1, 3)
    return dict(R=R, t=t, votes=votes, obj=np.tile(box, (k, 1)), img=votes.reshape(-1, 2), R0=R0, t0=t0)


def corner_problem(sc, mode=W.FULL, sigma_floor=0.5, scores=None):
    """votes aggregated per corner: (obj [8,3], mu [8,2], wgt [8,3]) from the restated vote_stats"""
    k = sc["votes"].shape[0]
    st = W.vote_stats(sc["img"], [0, 8 * k], 8, scores, None, mode, sigma_floor)
    return BOX.copy(), st["mu"][0], st["wgt"][0]


def vote_problem(seed, n):
    """the first n correspondences of scene(seed) with ceil(n / 8) votes, every vote whitened by its corner's covariance
    (W = (cov + 0.25 I)^(-1/2), the restated vote_stats with n_eff = 1) -> (obj [n,3], img [n,2], wgt [n,3], R0, t0)"""
    k = max((n + 7) // 8, 2)
    sc = scene(seed, k)
    st = W.vote_stats(sc["img"], [0, 8 * k], 8, None, None, W.FULL, 0.5)
    wc = np.stack([W.weight_from_cov(st["cov"][0, j], 1.0, W.FULL, 0.5) for j in range(8)])
    return sc["obj"][:n].copy(), sc["img"][:n].copy(), np.tile(wc, (k, 1))[:n].copy(), sc["R0"], sc["t0"]
