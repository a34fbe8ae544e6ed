"""GPU: pp_pnp_ransac_f64 stage by stage against oracle/pnp_np.py (hypotheses / score / winner / refine), on the designed inputs of
tests/pnp_cases.py whose margins tests/test_pnp_cases_cpu.py asserts on the CPU.  The entry point is called through the C ABI so that
the test owns the hypothesis workspace [n_problems][iterations][12] and every output buffer: each carries 64 spare elements and
starts filled with sentinel bytes.

Bounds are those of test_gpu_pnp.py::test_batch_matches_oracle: |dR| < 1e-8, |dt| < 1e-6, equal inlier sets -- for every hypothesis
of the clean cases as for final poses.  The vote schedule is checked bit for bit: a vote drawn again runs the same thread code on the
same inputs."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import pnp_np as P
from tests import pnp_cases as C

pytestmark = pytest.mark.gpu

SPARE = 64
SENT_F, SENT_I, SENT_B = -12345.678, -77, 0xA5
R_TOL, T_TOL = 1e-8, 1e-6


@pytest.fixture(scope="module")
def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


class Got(object):
    pass


def run_case(ctx, c):
    """one call of pp_pnp_ransac_f64 on a case; every buffer comes back whole, spare elements included"""
    from pyrapose_amd._lib import check, lib
    n_prob = len(c.problems)
    offs = np.concatenate([[0], np.cumsum([len(p.obj) for p in c.problems])]).astype(np.int32)
    N = int(offs[-1])
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    obj = dev(np.concatenate([p.obj for p in c.problems]).reshape(-1, 3), np.float64)
    img = dev(np.concatenate([p.img for p in c.problems]).reshape(-1, 2), np.float64)
    K4 = dev(np.array([p.K4 for p in c.problems]), np.float64)
    offsets = dev(offs, np.int32)
    ws_bytes = lib.pp_pnp_ransac_workspace_bytes(n_prob, c.iterations)
    assert ws_bytes == n_prob * c.iterations * 12 * 8
    full = lambda n, v, dt: torch.full((n + SPARE,), v, dtype=dt, device="cuda")
    ws = full(n_prob * c.iterations * 12, SENT_F, torch.float64)
    R, t = full(n_prob * 9, SENT_F, torch.float64), full(n_prob * 3, SENT_F, torch.float64)
    n_in, ok = full(n_prob, SENT_I, torch.int32), full(n_prob, SENT_I, torch.int32)
    mask = full(N, SENT_B, torch.uint8)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    check(lib.pp_pnp_ransac_f64(ctx.handle, n_prob, p(offsets), N, p(obj), p(img), p(K4), c.iterations, c.reproj_error, c.seed, c.ppv,
                                p(ws), p(R), p(t), p(n_in), p(mask), p(ok)), ctx.handle, "pp_pnp_ransac_f64")
    torch.cuda.synchronize()
    g = Got()
    g.offs, g.N, g.n_prob = offs, N, n_prob
    g.ws_all, g.R_all, g.t_all = ws.cpu().numpy(), R.cpu().numpy(), t.cpu().numpy()
    g.n_in_all, g.ok_all, g.mask_all = n_in.cpu().numpy(), ok.cpu().numpy(), mask.cpu().numpy()
    g.ws = g.ws_all[:n_prob * c.iterations * 12].reshape(n_prob, c.iterations, 12)
    g.R, g.t = g.R_all[:n_prob * 9].reshape(n_prob, 3, 3), g.t_all[:n_prob * 3].reshape(n_prob, 3)
    g.n_in, g.ok, g.mask = g.n_in_all[:n_prob], g.ok_all[:n_prob], g.mask_all[:N]
    return g


def assert_spare_untouched(g, c):
    assert np.all(g.ws_all[g.n_prob * c.iterations * 12:] == SENT_F)
    assert np.all(g.R_all[g.n_prob * 9:] == SENT_F) and np.all(g.t_all[g.n_prob * 3:] == SENT_F)
    assert np.all(g.n_in_all[g.n_prob:] == SENT_I) and np.all(g.ok_all[g.n_prob:] == SENT_I)
    assert np.all(g.mask_all[g.N:] == SENT_B)


def assert_hypotheses(g, c, p):
    """every workspace row of problem p against the oracle's; the marked rows are the same rows"""
    hyps, _, _ = C.oracle_stages(c.name, p)
    marked = np.isnan(hyps[:, 0])
    assert np.array_equal(np.isnan(g.ws[p, :, 0]), marked), (c.name, p, np.nonzero(np.isnan(g.ws[p, :, 0]) != marked)[0][:8])
    rows = ~marked
    if rows.any():
        assert np.isfinite(g.ws[p, rows]).all() and not np.any(g.ws[p, rows] == SENT_F)
        dR = np.abs(g.ws[p, rows, :9] - hyps[rows, :9]).max(axis=1)
        dt = np.abs(g.ws[p, rows, 9:] - hyps[rows, 9:]).max(axis=1)
        print("%s problem %d: %d rows, max |dR| %.3e, max |dt| %.3e" % (c.name, p, int(rows.sum()), dR.max(), dt.max()))
        assert dR.max() < R_TOL and dt.max() < T_TOL, (c.name, p, int(np.argmax(dR)), dR.max(), int(np.argmax(dt)), dt.max())


def assert_final(g, c, p):
    """(ok, R, t, n_inliers, mask) of problem p against the oracle run alone with its own problem index and K4"""
    ok, R, t, mask = C.oracle_final(c.name, p)
    m = g.mask[g.offs[p]:g.offs[p + 1]]
    assert g.ok[p] == int(ok), (c.name, p, g.ok[p], ok)
    if not ok and not mask.any() and np.array_equal(R, np.eye(3)):     # the failure path: exact values
        assert np.array_equal(g.R[p], np.eye(3)) and np.array_equal(g.t[p], np.zeros(3)) and g.n_in[p] == 0 and not m.any()
        return
    dR, dt = np.abs(g.R[p] - R).max(), np.abs(g.t[p] - t).max()
    print("%s problem %d: final |dR| %.3e, |dt| %.3e, %d inliers of %d" % (c.name, p, dR, dt, int(mask.sum()), len(mask)))
    assert dR < R_TOL and dt < T_TOL, (c.name, p, dR, dt)
    assert set(np.unique(m)) <= {0, 1} and np.array_equal(m.astype(bool), mask), (c.name, p, np.nonzero(m.astype(bool) != mask)[0][:8])
    assert g.n_in[p] == int(mask.sum())


# ---- a. hypotheses, element by element ----

@pytest.mark.parametrize("name", C.CLEAN)
def test_hypotheses_match_the_oracle(ctx, name):
    """points per vote 8, 6, 16 and 0; a vote collapsed to one object point and a problem with fewer points than a vote (marked rows);
    iterations around the 256 threads of stage 1"""
    c = C.case(name)
    g = run_case(ctx, c)
    assert_spare_untouched(g, c)
    for p in range(g.n_prob):
        assert_hypotheses(g, c, p)
    if name == "clean_ppv8":
        assert np.isnan(g.ws[1, :, 0]).all() and np.isnan(g.ws[0, 2, 0]) and not np.isnan(g.ws[0, :2, 0]).any()


# ---- b. vote schedule, without a tolerance ----

@pytest.mark.parametrize("seed", C.SCHEDULE_SEEDS)
def test_vote_schedule_bit_for_bit(ctx, seed):
    """every vote once, then the vote of draw(seed, problem, it, 0) % nv: rows it >= nv are copies, bit for bit, of the row of the vote
    they drew; problems 0, 1 and 3 hold the same data and differ in their schedules alone"""
    c = C.case("schedule_seed%d" % seed)
    nv, same = c.info["nv"], c.info["same"]
    g = run_case(ctx, c)
    bits = g.ws.view(np.int64)
    schedules = []
    for p in same:
        assert not np.isnan(g.ws[p]).any()
        assert np.array_equal(bits[p, :nv], bits[same[0], :nv])                      # votes 0 .. nv-1, whatever the problem index
        assert len({bits[p, v].tobytes() for v in range(nv)}) == nv
        want = [it if it < nv else int(P.draw(seed, p, it, 0) % nv) for it in range(c.iterations)]
        seen = [[v for v in range(nv) if np.array_equal(bits[p, it], bits[p, v])] for it in range(c.iterations)]
        assert seen == [[v] for v in want], (p, [(it, s, w) for it, (s, w) in enumerate(zip(seen, want)) if s != [w]][:6])
        schedules.append(tuple(want[nv:]))
    assert len(set(schedules)) == len(same)
    for p in range(g.n_prob):
        assert_hypotheses(g, c, p)


# ---- c. tie rule ----

@pytest.mark.parametrize("name", C.TIE)
def test_tie_goes_to_the_lower_iteration(ctx, name):
    """two hypotheses with 24 inliers each and different poses, every other at most 8: inside one wave, across waves with the lower
    wave holding the lower iteration, and across waves with the higher wave holding it"""
    c = C.case(name)
    _, _, want = C.TIES[name[len("tie_"):]]
    g = run_case(ctx, c)
    assert_hypotheses(g, c, 0)
    assert_final(g, c, 0)
    (Ra, _), (Rb, _) = c.info["A"], c.info["B"]
    err_a, err_b = C.rot_err_deg(g.R[0], Ra), C.rot_err_deg(g.R[0], Rb)
    assert (err_a < 0.1) == (want == "A") and (err_b < 0.1) == (want == "B"), (want, err_a, err_b)


# ---- d. strides ----

@pytest.mark.parametrize("name", ["votes_%d" % k for k in C.VOTE_COUNTS])
def test_vote_counts_around_the_strides(ctx, name):
    """n = 8 .. 520 against the 64 lanes of scoring and the 256 threads of refinement; 32 votes + 3 leftover points"""
    c = C.case(name)
    g = run_case(ctx, c)
    assert_spare_untouched(g, c)
    assert_final(g, c, 0)


@pytest.mark.parametrize("name", ["unstructured_%d" % k for k in C.UNSTRUCTURED_N])
def test_unstructured_sizes_around_the_strides(ctx, name):
    c = C.case(name)
    g = run_case(ctx, c)
    assert_spare_untouched(g, c)
    assert_final(g, c, 0)


@pytest.mark.parametrize("name", ["iterations_%d" % k for k in C.ITERATION_COUNTS])
def test_iteration_counts_around_the_strides(ctx, name):
    """iterations below the 4 waves of scoring and around the 256 threads of stage 1; with one iteration the vote of pose B is alone"""
    c = C.case(name)
    g = run_case(ctx, c)
    assert_final(g, c, 0)
    want = c.info["pose_b" if c.iterations == 1 else "pose_a"]
    assert C.rot_err_deg(g.R[0], want[0]) < 0.1


# ---- e. batch layout ----

def test_batch_layout_and_failure_stores(ctx):
    """a normal problem, one without points, one with 5 points < 8, one with its own K4 row, one with few inliers -- in one call, each
    against the oracle run alone; failed problems get exactly identity, zeros, zero mask bytes and ok = 0, and nothing is stored
    outside a problem's own slots"""
    c = C.case("batch")
    g = run_case(ctx, c)
    assert_spare_untouched(g, c)
    assert list(g.ok) == [1, 0, 0, 1, 1]
    for p in range(g.n_prob):
        assert_final(g, c, p)
    for p in c.info["failed"]:
        assert np.array_equal(g.R[p], np.eye(3)) and np.array_equal(g.t[p], np.zeros(3)) and g.n_in[p] == 0 and g.ok[p] == 0
        assert not g.mask[g.offs[p]:g.offs[p + 1]].any()
        assert np.isnan(g.ws[p, :, 0]).all()
    assert g.offs[1] == g.offs[2] and g.offs[3] - g.offs[2] == 5
    # the failed problem's neighbours keep their inliers up to its first and after its last byte
    assert g.mask[g.offs[2] - 1] == 1 and g.mask[g.offs[3]] == 1
    assert not np.any(g.mask == SENT_B) and not np.any(g.R == SENT_F) and not np.any(g.t == SENT_F)
    other = c.info["other_k"]
    assert np.abs(g.R[other] - C.oracle_final("batch", other)[1]).max() < R_TOL
    assert 20 <= g.n_in[c.info["few"]] <= 32


# ---- f. behind the camera ----

def test_points_behind_the_camera_are_outliers(ctx):
    c = C.case("behind")
    g = run_case(ctx, c)
    assert_spare_untouched(g, c)
    assert_final(g, c, 0)
    behind = c.info["behind"]
    assert g.ok[0] == 1 and not g.mask[behind].any() and g.mask[~behind].all() and g.n_in[0] == 48
