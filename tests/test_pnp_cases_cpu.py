"""Host-side ledger of tests/test_gpu_pnp_stages.py (no GPU): the conditions on the designed inputs of tests/pnp_cases.py under which
the kernel's comparison with oracle/pnp_np.py at |dR| < 1e-8, |dt| < 1e-6 and equal inlier sets says something about the kernel --
asserted through the oracle alone.  These are conditions on the inputs (seeds are chosen so that each holds), not measurements:

  clean cases   every oracle hypothesis moves by < 1e-10 in R and < 1e-8 in t (1/100 of the bounds) when the image points move by a
                relative 1e-13: a sample that is ill conditioned in the oracle itself would not test the kernel;
  tie cases     the two tied hypotheses count the same, at least 16 more than any other, their poses differ by > 1 degree, and the
                oracle's winner is the intended one;
  masks         under the oracle's final pose -- and under every hypothesis, whose counts decide the winner -- no squared error lies
                within a relative 1e-6 of reproj_error^2; under the final pose no depth within 1e-6 of the 1e-9 front test;
  unstructured  six sampled points are six different points and span space."""
import numpy as np
import pytest

from oracle import pnp_np as P
from tests import pnp_cases as C


def problems_of(names):
    return [(n, p) for n in names for p in range(len(C.case(n).problems))]


def test_every_case_is_in_a_group_and_has_the_sizes_it_names():
    assert set(C.ALL) == set(C.CLEAN) | set(C.FINAL)
    for nv in C.VOTE_COUNTS:
        c = C.case("votes_%d" % nv)
        assert len(c.problems[0].obj) == 8 * nv + (3 if nv == 32 else 0) and c.iterations > nv and c.ppv == 8
    assert [len(C.case("unstructured_%d" % n).problems[0].obj) for n in C.UNSTRUCTURED_N] == list(C.UNSTRUCTURED_N)
    assert [C.case("iterations_%d" % k).iterations for k in C.ITERATION_COUNTS] == [1, 3, 4, 5, 255, 256, 257]
    assert {C.case(n).ppv for n in C.CLEAN} == {8, 6, 16, 0}
    b = C.case("batch")
    assert [len(p.obj) for p in b.problems] == [72, 0, 5, 64, 80] and b.iterations > 10
    assert all(abs(a - o) > 1.0 for a, o in zip(b.problems[3].K4, b.problems[0].K4))


@pytest.mark.parametrize("name,p", problems_of(C.CLEAN))
def test_clean_hypotheses_are_well_conditioned(name, p):
    c = C.case(name)
    pr = c.problems[p]
    hyps, samples, _ = C.oracle_stages(name, p)
    assert np.abs(pr.img - c.info["exact"][p]).max() <= 1e-3            # exact projections, or noise of at most 1e-3 px
    rel = np.random.default_rng(7).choice([-1e-13, 1e-13], size=pr.img.shape)
    moved, samples2 = P.hypotheses(pr.obj, pr.img * (1.0 + rel), pr.K4, c.iterations, c.seed, p, c.ppv)
    assert samples2 == samples
    marked = np.isnan(hyps[:, 0])
    assert np.array_equal(marked, np.isnan(moved[:, 0])) and np.array_equal(np.isnan(hyps).all(axis=1), marked)
    if not marked.all():
        dR = np.abs(hyps[~marked, :9] - moved[~marked, :9]).max()
        dt = np.abs(hyps[~marked, 9:] - moved[~marked, 9:]).max()
        assert dR < 1e-10 and dt < 1e-8, (dR, dt)
        R = hyps[~marked, :9].reshape(-1, 3, 3)
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12


def test_clean_cases_mark_the_rows_they_are_meant_to():
    hyps, samples, _ = C.oracle_stages("clean_ppv8", 0)
    vote2 = np.array([s[0] == 16 for s in samples])
    assert vote2[2] and vote2.sum() >= 2                 # met again among the random draws
    assert np.array_equal(np.isnan(hyps[:, 0]), vote2)
    hyps, samples, counts = C.oracle_stages("clean_ppv8", 1)
    assert np.isnan(hyps).all() and samples == [None] * 20 and (counts == -1).all()
    for name in ("clean_ppv6", "clean_ppv16", "clean_ppv0"):
        hyps, samples, _ = C.oracle_stages(name, 0)
        assert not np.isnan(hyps).any()
        assert {len(s) for s in samples} == {C.case(name).ppv or 6}


@pytest.mark.parametrize("seed", C.SCHEDULE_SEEDS)
def test_schedule_case_tells_votes_problems_and_seeds_apart(seed):
    name = "schedule_seed%d" % seed
    c = C.case(name)
    nv = c.info["nv"]
    schedules = {}
    for p in c.info["same"]:
        assert all(np.array_equal(a, b) for a, b in zip(c.problems[p], c.problems[0]))
        hyps, samples, _ = C.oracle_stages(name, p)
        assert len({hyps[v].tobytes() for v in range(nv)}) == nv          # a row names its vote
        assert np.array_equal(hyps[:nv], C.oracle_stages(name, 0)[0][:nv])
        sched = [s[0] // 8 for s in samples]
        assert sched[:nv] == list(range(nv))
        assert sched[nv:] == [int(P.draw(seed, p, it, 0) % nv) for it in range(nv, c.iterations)]
        assert set(sched[nv:]) == set(range(nv))
        schedules[p] = tuple(sched)
    assert len(set(schedules.values())) == 3                              # the problem index reaches the key
    other = "schedule_seed%d" % [s for s in C.SCHEDULE_SEEDS if s != seed][0]
    assert [s[0] // 8 for s in C.oracle_stages(other, 0)[1]] != list(schedules[0])


@pytest.mark.parametrize("name", C.TIE)
def test_tie_cases_are_exact_ties_far_ahead(name):
    c = C.case(name)
    it_a, it_b, want = C.TIES[name[len("tie_"):]]
    assert c.iterations == len(c.problems[0].obj) // 8
    hyps, _, counts = C.oracle_stages(name, 0)
    assert counts[it_a] == counts[it_b] == 24
    others = np.delete(counts, [it_a, it_b])
    assert others.max() <= counts[it_a] - 16, counts
    (Ra, ta), (Rb, tb) = c.info["A"], c.info["B"]
    assert C.rot_err_deg(Ra, Rb) > 1.0
    assert C.rot_err_deg(hyps[it_a, :9].reshape(3, 3), Ra) < 1e-3 and C.rot_err_deg(hyps[it_b, :9].reshape(3, 3), Rb) < 1e-3
    assert P.winner(counts) == (it_a if want == "A" else it_b) == min(it_a, it_b)
    ok, R, t, mask = C.oracle_final(name, 0)
    Rw = Ra if want == "A" else Rb
    assert ok and mask.sum() == 24 and C.rot_err_deg(R, Rw) < 0.1 and C.rot_err_deg(R, Rb if want == "A" else Ra) > 1.0


@pytest.mark.parametrize("name,p", problems_of(C.FINAL))
def test_no_point_sits_on_an_inlier_threshold(name, p):
    c = C.case(name)
    pr = c.problems[p]
    ok, R, t, mask = C.oracle_final(name, p)
    rel, depth = C.threshold_margins(R, t, pr, c.reproj_error)
    assert rel > 1e-6 and depth > 1e-6, (rel, depth)
    hyps, _, counts = C.oracle_stages(name, p)
    for h in hyps[counts >= 0]:
        rel, _ = C.threshold_margins(h[:9].reshape(3, 3), h[9:], pr, c.reproj_error)
        assert rel > 1e-6, rel


@pytest.mark.parametrize("name", ["clean_ppv0", "behind"] + ["unstructured_%d" % n for n in C.UNSTRUCTURED_N])
def test_unstructured_samples_are_six_points_that_span_space(name):
    c = C.case(name)
    obj = c.problems[0].obj
    assert c.ppv == 0 and len({tuple(x) for x in obj}) == len(obj)
    _, samples, _ = C.oracle_stages(name, 0)
    for s in samples:
        assert len(set(s)) == 6 and min(s) >= 0 and max(s) < len(obj)
        X = obj[s] - obj[s].mean(axis=0)
        sv = np.linalg.svd(X, compute_uv=False)
        assert sv[2] > 0.02 * sv[0], (s, sv)


def test_final_cases_end_as_designed():
    for k in C.ITERATION_COUNTS:                                          # alone, the vote of pose B wins; from 3 on pose A
        name = "iterations_%d" % k
        ok, R, t, mask = C.oracle_final(name, 0)
        want = C.case(name).info["pose_b" if k == 1 else "pose_a"]
        assert ok and C.rot_err_deg(R, want[0]) < 0.1 and mask.sum() == (8 if k == 1 else 32)
    for nv in C.VOTE_COUNTS:
        name = "votes_%d" % nv
        ok, R, t, mask = C.oracle_final(name, 0)
        assert ok and C.rot_err_deg(R, C.case(name).info["pose"][0]) < 3.0
        if nv == 32:
            assert len(mask) == 259 and mask[256:].all()                  # the leftover points are scored
    for n in C.UNSTRUCTURED_N:
        name = "unstructured_%d" % n
        ok, R, t, mask = C.oracle_final(name, 0)
        bad = C.case(name).info["bad"]
        assert ok and not mask[bad].any() and mask[~bad].sum() >= 0.9 * (~bad).sum()
    b = C.case("batch")
    oks = [C.oracle_final("batch", p)[0] for p in range(5)]
    assert oks == [True, False, False, True, True]
    for p in b.info["failed"]:
        ok, R, t, mask = C.oracle_final("batch", p)
        assert np.array_equal(R, np.eye(3)) and not t.any() and not mask.any()
    assert C.oracle_final("batch", 0)[3][-1] and C.oracle_final("batch", 3)[3][0]      # inliers on either side of the 5-point problem
    few = C.oracle_final("batch", b.info["few"])[3]
    assert 20 <= few.sum() <= 32 and len(few) == 80                       # 3 clean votes of 10
    ok, R, t, mask = C.oracle_final("behind", 0)
    behind = C.case("behind").info["behind"]
    assert ok and behind.sum() == 16 and not mask[behind].any() and mask[~behind].all()
    assert ((C.case("behind").problems[0].obj @ R.T + t)[behind, 2] < -100.0).all()
