"""The designed inputs of tests/test_gpu_pnp_stages.py, built from fixed seeds, with their oracle results (oracle/pnp_np.py) computed
once per process.  tests/test_pnp_cases_cpu.py asserts on the CPU the margins that make the GPU comparisons meaningful (clean samples
well conditioned, ties exact and far ahead, no point on an inlier threshold); the GPU file compares the kernel with the same objects.

A case is one call of pp_pnp_ransac_f64: a batch of problems (obj [n,3], img [n,2], K4), iterations, seed, points per vote."""
import functools
from collections import namedtuple

import numpy as np

from oracle import pnp_np as P
from tests.test_oracle_pnp import BOX, K4, rot_err_deg  # noqa: F401  (re-exported)

Case = namedtuple("Case", "name problems iterations seed ppv reproj_error info")
Problem = namedtuple("Problem", "obj img K4")

K4_OTHER = (601.25, 588.5, 301.75, 259.125)       # differs from K4 in all four entries
MODEL_HALF = np.array([40.0, 30.0, 55.0])         # the model-sized box general object points are drawn from (BOX's half extents)
REPROJ = 5.0


def project(R, t, X, k4=K4):
    Xc = X @ R.T + t
    return np.stack([k4[0] * Xc[:, 0] / Xc[:, 2] + k4[2], k4[1] * Xc[:, 1] / Xc[:, 2] + k4[3]], axis=1)


def random_pose(rng):
    return P.so3_exp(rng.normal(size=3)), np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(600, 1100)])


def general_points(rng, n):
    return rng.uniform(-1, 1, size=(n, 3)) * MODEL_HALF


def vote_problem(rng, nv, noise, outlier_votes=(), k4=K4, vote_obj=BOX, leftover=0, pose=None):
    """nv votes of len(vote_obj) points under one pose: Gaussian pixel noise, +40 px noise on the outlier votes; `leftover` extra
    correspondences (inliers) after the last vote"""
    R, t = pose if pose is not None else random_pose(rng)
    ppv = len(vote_obj)
    img = np.repeat(project(R, t, vote_obj, k4)[None], nv, 0) + rng.normal(scale=noise, size=(nv, ppv, 2))
    for v in outlier_votes:
        img[v] += rng.normal(scale=40.0, size=(ppv, 2))
    obj, img = np.tile(vote_obj, (nv, 1)), img.reshape(-1, 2)
    if leftover:
        extra = general_points(rng, leftover)
        obj = np.concatenate([obj, extra])
        img = np.concatenate([img, project(R, t, extra, k4) + rng.normal(scale=noise, size=(leftover, 2))])
    return Problem(obj, img, k4), (R, t)


def clean_votes(rng, nv, vote_obj, k4=K4, pose=None):
    """exact projections + uniform noise of at most 1e-3 px, so that the votes give different, well-conditioned hypotheses"""
    R, t = pose if pose is not None else random_pose(rng)
    ppv = len(vote_obj)
    exact = np.repeat(project(R, t, vote_obj, k4)[None], nv, 0)
    img = exact + rng.uniform(-1e-3, 1e-3, size=(nv, ppv, 2))
    return Problem(np.tile(vote_obj, (nv, 1)), img.reshape(-1, 2), k4), (R, t), exact.reshape(-1, 2)


def empty_problem(k4=K4):
    return Problem(np.zeros((0, 3)), np.zeros((0, 2)), k4)


# ---- a. clean cases: every hypothesis is compared element by element ----

def _clean_ppv8():
    """6 cuboid votes, vote 2 collapsed to one object point (rms == 0: marked row); second problem: 5 points < 8 (every row marked)"""
    rng = np.random.default_rng(101)
    p0, pose, exact0 = clean_votes(rng, 6, BOX)
    obj, img = p0.obj.copy(), p0.img.copy()
    obj[16:24] = BOX[3]
    img[16:24] = exact0[16:24] = project(pose[0], pose[1], BOX[3:4])
    p1, _, exact1 = clean_votes(rng, 1, BOX)
    return Case("clean_ppv8", [Problem(obj, img, K4), Problem(p1.obj[:5], p1.img[:5], K4)], 20, 11, 8, REPROJ,
                {"exact": [exact0, exact1[:5]]})


def _clean_ppv6():
    rng = np.random.default_rng(102)
    p0, _, exact = clean_votes(rng, 5, general_points(rng, 6))
    return Case("clean_ppv6", [p0], 16, 12, 6, REPROJ, {"exact": [exact]})


def _clean_ppv16():
    rng = np.random.default_rng(103)
    p0, _, exact = clean_votes(rng, 4, np.concatenate([BOX, general_points(rng, 8)]))
    return Case("clean_ppv16", [p0], 12, 13, 16, REPROJ, {"exact": [exact]})


def _clean_ppv0():
    """general object points (no vote structure): six sampled points are neither coplanar nor repeated.  The camera stands 350 away:
    at 600 and more, six points of a model this size leave the depth of the oracle's own hypothesis looser than 1/100 of the bound"""
    rng = np.random.default_rng(104)
    R, t = random_pose(rng)
    t = np.array([0.3 * t[0], 0.3 * t[1], 350.0])
    obj = general_points(rng, 50)
    exact = project(R, t, obj)
    img = exact + rng.uniform(-1e-3, 1e-3, size=(50, 2))
    return Case("clean_ppv0", [Problem(obj, img, K4)], 24, 14, 0, REPROJ, {"exact": [exact]})


def _clean_iterations(iterations):
    """the stage-1 / stage-2 strides against `iterations`: vote 0 is an exact vote of another pose (it wins only when it is alone),
    votes 1..4 belong to the pose of the problem"""
    rng = np.random.default_rng(105)
    pa, pose_a, exact = clean_votes(rng, 5, BOX)
    pose_b = random_pose(rng)
    img = pa.img.copy()
    img[:8] = exact[:8] = project(pose_b[0], pose_b[1], BOX)
    return Case("iterations_%d" % iterations, [Problem(pa.obj, img, K4)], iterations, 15, 8, REPROJ,
                {"pose_a": pose_a, "pose_b": pose_b, "exact": [exact]})


ITERATION_COUNTS = (1, 3, 4, 5, 255, 256, 257)


# ---- b. vote schedule ----

def _schedule(seed):
    """problems 0, 1 and 3 hold the same 5 clean votes (problem 2 another 5), 40 iterations: rows 5.. repeat the rows of drawn votes"""
    rng = np.random.default_rng(106)
    p0, _, e0 = clean_votes(rng, 5, BOX)
    p2, _, e2 = clean_votes(rng, 5, BOX)
    return Case("schedule_seed%d" % seed, [p0, p0, p2, p0], 40, seed, 8, REPROJ, {"nv": 5, "same": (0, 1, 3), "exact": [e0, e0, e2, e0]})


SCHEDULE_SEEDS = (21, 22)


# ---- c. tie rule ----

TIES = {  # name: (iteration of A, iteration of B, the winner)
    "in_wave": (0, 4, "A"),               # wave 0 meets it = 0 then it = 4
    "lower_wave_first": (2, 1, "B"),      # it = 1 in wave 1, it = 2 in wave 2
    "higher_wave_lower_it": (1, 4, "A"),  # it = 4 in wave 0, it = 1 in wave 1
}


def _tie(name):
    """iterations = number of votes = 9.  Votes 0..4: one exact vote of pose A, one of pose B, three single-vote filler poses; votes
    5..8: two supporters of A and two of B -- eight copies of ONE corner's exact projection, so each adds 8 inliers to its pose and
    its own row is marked (rms == 0), never a rival.  A and B count 24, a filler 8."""
    it_a, it_b, _ = TIES[name]
    rng = np.random.default_rng(107)
    pose_a, pose_b = random_pose(rng), random_pose(rng)
    obj = np.tile(BOX, (9, 1))
    img = np.zeros((72, 2))
    for v in range(5):
        pose = pose_a if v == it_a else pose_b if v == it_b else random_pose(rng)
        img[8 * v:8 * v + 8] = project(pose[0], pose[1], BOX)
    for v, (pose, corner) in zip(range(5, 9), ((pose_a, 1), (pose_b, 6), (pose_a, 4), (pose_b, 2))):
        obj[8 * v:8 * v + 8] = BOX[corner]
        img[8 * v:8 * v + 8] = project(pose[0], pose[1], BOX[corner:corner + 1])
    return Case("tie_" + name, [Problem(obj, img, K4)], 9, 31, 8, REPROJ,
                {"A": pose_a, "B": pose_b, "it_a": it_a, "it_b": it_b, "exact": [img.copy()]})


# ---- d. strides ----

VOTE_COUNTS = (1, 7, 8, 9, 31, 32, 33, 65)     # n = 8 .. 520 around 64 and 256
UNSTRUCTURED_N = (6, 7, 63, 64, 65, 255, 256, 257)


def _votes(nv):
    """1 px noise, every fourth vote an outlier (vote 0 never); nv = 32 carries 3 leftover points: scored, never sampled"""
    rng = np.random.default_rng(200 + nv)
    p, pose = vote_problem(rng, nv, 1.0, outlier_votes=range(3, nv, 4), leftover=3 if nv == 32 else 0)
    return Case("votes_%d" % nv, [p], nv + 3, 41, 8, REPROJ, {"pose": pose})


def _unstructured(n):
    """general points, 0.5 px noise, every fifth correspondence 30 to 100 px off from n = 63 on"""
    rng = np.random.default_rng(300 + n)
    R, t = random_pose(rng)
    obj = general_points(rng, n)
    img = project(R, t, obj) + rng.normal(scale=0.5, size=(n, 2))
    bad = np.zeros(n, bool)
    if n >= 63:
        bad[rng.permutation(n)[:n // 5]] = True
        ang = rng.uniform(0, 2 * np.pi, size=int(bad.sum()))
        img[bad] += rng.uniform(30.0, 100.0, size=(int(bad.sum()), 1)) * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    return Case("unstructured_%d" % n, [Problem(obj, img, K4)], 24, 42, 0, REPROJ, {"pose": (R, t), "bad": bad})


# ---- e. batch layout ----

def _batch():
    rng = np.random.default_rng(108)
    normal, _ = vote_problem(rng, 9, 1.0, outlier_votes=(2, 5))
    short, _ = vote_problem(rng, 1, 0.5)
    other_k, _ = vote_problem(rng, 8, 1.0, outlier_votes=(4,), k4=K4_OTHER)
    few, _ = vote_problem(rng, 10, 1.0, outlier_votes=(0, 1, 3, 4, 5, 7, 9))
    problems = [normal, empty_problem(), Problem(short.obj[:5], short.img[:5], K4), other_k, few]
    return Case("batch", problems, 24, 51, 8, REPROJ, {"failed": (1, 2), "other_k": 3, "few": 4})


# ---- f. points behind the camera ----

def _behind():
    """64 scene-sized points around the camera: 48 in front (depth >= 150) with their projections + 0.2 px, 16 behind (depth <= -150)
    with arbitrary image points"""
    rng = np.random.default_rng(109)
    R = P.so3_exp(rng.normal(size=3))
    t = np.array([30.0, -20.0, 400.0])
    z = np.concatenate([rng.uniform(150.0, 900.0, size=48), rng.uniform(-900.0, -150.0, size=16)])
    Xc = np.stack([rng.uniform(-0.8, 0.8, size=64) * z, rng.uniform(-0.8, 0.8, size=64) * z, z], axis=1)   # camera frame
    obj = (Xc - t) @ R
    img = np.concatenate([project(R, t, obj[:48]) + rng.normal(scale=0.2, size=(48, 2)), rng.uniform(0, 600, size=(16, 2))])
    order = rng.permutation(64)
    behind = np.zeros(64, bool)
    behind[48:] = True
    return Case("behind", [Problem(obj[order], img[order], K4)], 48, 61, 0, REPROJ, {"pose": (R, t), "behind": behind[order]})


_BUILDERS = {"clean_ppv8": _clean_ppv8, "clean_ppv6": _clean_ppv6, "clean_ppv16": _clean_ppv16, "clean_ppv0": _clean_ppv0,
             "batch": _batch, "behind": _behind}
_BUILDERS.update({"iterations_%d" % k: functools.partial(_clean_iterations, k) for k in ITERATION_COUNTS})
_BUILDERS.update({"schedule_seed%d" % s: functools.partial(_schedule, s) for s in SCHEDULE_SEEDS})
_BUILDERS.update({"tie_" + k: functools.partial(_tie, k) for k in TIES})
_BUILDERS.update({"votes_%d" % k: functools.partial(_votes, k) for k in VOTE_COUNTS})
_BUILDERS.update({"unstructured_%d" % k: functools.partial(_unstructured, k) for k in UNSTRUCTURED_N})

CLEAN = ["clean_ppv8", "clean_ppv6", "clean_ppv16", "clean_ppv0"] + ["iterations_%d" % k for k in ITERATION_COUNTS] + \
        ["schedule_seed%d" % s for s in SCHEDULE_SEEDS] + ["tie_" + k for k in TIES]
TIE = ["tie_" + k for k in TIES]
FINAL = TIE + ["iterations_%d" % k for k in ITERATION_COUNTS] + ["votes_%d" % k for k in VOTE_COUNTS] + \
        ["unstructured_%d" % k for k in UNSTRUCTURED_N] + ["batch", "behind"]     # cases whose (ok, R, t, mask) is compared
ALL = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def oracle_stages(name, p):
    """(hypotheses [iterations,12], samples, counts [iterations]) of problem p of a case; read-only"""
    c = case(name)
    pr = c.problems[p]
    with np.errstate(all="ignore"):     # (a sample of outliers may overflow on its way to a marked row)
        hyps, samples = P.hypotheses(pr.obj, pr.img, pr.K4, c.iterations, c.seed, p, c.ppv)
        counts = P.score(hyps, pr.obj, pr.img, pr.K4, c.reproj_error)
    hyps.setflags(write=False); counts.setflags(write=False)
    return hyps, samples, counts


@functools.lru_cache(maxsize=None)
def oracle_final(name, p):
    """(ok, R, t, mask) of problem p of a case, solved alone with its own problem index and K4; read-only"""
    c = case(name)
    pr = c.problems[p]
    with np.errstate(all="ignore"):
        ok, R, t, mask = P.solve_pnp_ransac(pr.obj, pr.img, pr.K4, c.iterations, c.reproj_error, c.seed, p, c.ppv)
    for a in (R, t, mask):
        a.setflags(write=False)
    return ok, R, t, mask


def threshold_margins(R, t, pr, reproj_error):
    """(smallest |e / thr^2 - 1| over the points in front, smallest |depth - 1e-9|) under one pose; (inf, inf) without points"""
    if len(pr.obj) == 0:
        return np.inf, np.inf
    z = (pr.obj @ R.T + t)[:, 2]
    e, ok = P.reproj_sq(R, t, pr.obj, pr.img, pr.K4)
    rel = np.abs(e[ok] / reproj_error ** 2 - 1.0)
    return (rel.min() if rel.size else np.inf), np.abs(z - 1e-9).min()
