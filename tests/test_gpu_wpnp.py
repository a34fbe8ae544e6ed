"""GPU: csrc/wpnp.hip through the C ABI (ops.vote_stats / ops.pnp_refine_weighted) against its numpy restatement
(tests/wpnp_np.py) on a ragged batch that covers both kernel paths, bitwise batch independence, failure cases and argument
checks; the reference's un_pnp_utils signatures; the weighting option of pose_decode.poses_from_outputs / evaluate_add."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import wpnp_np as W  # noqa: E402
from tests.test_oracle_pnp import BOX, K4, project  # noqa: E402
from tests.wpnp_scenes import K4A, corner_problem, rot_err_deg, scene, vote_problem  # noqa: E402

# (correspondences, seeds): one wave per problem up to 64, one workgroup above (in registers up to 1024); the seeds are the
# ones whose restatement trace keeps every stopping test a factor 10 away from its threshold (searched on the CPU)
RAGGED = ((8, (0, 2, 3)), (9, (0, 2)), (64, (3, 4, 6)), (65, (0, 4, 5)), (320, (1, 2, 3)), (1600, (4, 7, 8)))
KMAT = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])


@pytest.fixture(scope="module")
def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


def ragged_batch():
    probs = [vote_problem(s, n) for n, seeds in RAGGED for s in seeds]
    o, i, w, R0, t0 = vote_problem(1, 24)
    probs.insert(4, (o[:0], i[:0], w[:0], R0, t0))          # an empty problem
    probs.insert(9, (o, i, np.zeros_like(w), R0, t0))       # a problem whose weights are all zero
    return probs


def dev(a, dt=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()


def run(ctx, probs, pose_cov=True, **kw):
    from pyrapose_amd import ops
    offs = np.concatenate([[0], np.cumsum([len(p[0]) for p in probs])]).astype(np.int32)
    cat = lambda k, w: np.concatenate([p[k].reshape(-1, w) for p in probs])
    r = ops.pnp_refine_weighted(ctx, dev(offs, torch.int32), dev(cat(0, 3)), dev(cat(1, 2)), dev(cat(2, 3)), dev(np.tile(K4A, (len(probs), 1))),
                                dev(np.stack([p[3] for p in probs])), dev(np.stack([p[4] for p in probs])), pose_cov=pose_cov, **kw)
    return {k: v.cpu().numpy() for k, v in r.items() if v is not None}


def test_ragged_batch_matches_the_restatement(ctx):
    probs = ragged_batch()
    tight = dict(max_iterations=100, gradient_tol=1e-15, parameter_tol=1e-15, function_tol=1e-15)
    got = run(ctx, probs, **tight)
    for p, (o, i, w, R0, t0) in enumerate(probs):
        want = W.refine_weighted(o, i, w, K4A, R0, t0, **tight)
        assert got["status"][p] == want["status"], p
        dR, dt = np.abs(got["R"][p] - want["R"]).max(), np.abs(got["t"][p] - want["t"]).max()
        print("problem %d (%d points): |dR| %.3g |dt| %.3g passes %d / %d" % (p, len(o), dR, dt, got["iterations"][p], want["iterations"]))
        assert dR < 1e-8 and dt < 1e-6, (p, dR, dt)
        assert np.abs(got["rvec"][p] - want["rvec"]).max() < 1e-8
        if want["status"] == W.CONVERGED:
            assert np.abs(got["pose_cov"][p] - want["pose_cov"]).max() <= 1e-6 * np.abs(want["pose_cov"]).max(), p
            assert np.abs(W.rodrigues(got["rvec"][p]) - got["R"][p]).max() < 1e-14
    # default tolerances: the same decisions wherever the restatement's trace keeps clear of every threshold
    got = run(ctx, probs)
    clear = 0
    for p, (o, i, w, R0, t0) in enumerate(probs):
        want = W.refine_weighted(o, i, w, K4A, R0, t0)
        if W.trace_is_clear(want["trace"]):
            clear += 1
            assert got["status"][p] == want["status"] and got["iterations"][p] == want["iterations"], (p, got["iterations"][p], want["iterations"])
        assert got["cost_final"][p] <= got["cost_init"][p]
    assert clear >= 0.75 * len(probs), clear


def test_bitwise_independent_of_batch_and_run(ctx):
    probs = ragged_batch()
    a, b = run(ctx, probs), run(ctx, probs)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for p, prob in enumerate(probs):
        alone = run(ctx, [prob])
        for k in a:
            assert np.array_equal(alone[k][0], a[k][p]), (p, k)
    assert "pose_cov" not in run(ctx, probs[:3], pose_cov=False)


def test_failure_cases_and_bad_arguments(ctx):
    from pyrapose_amd import ops
    o, i, w, R0, t0 = vote_problem(0, 8)
    two = w.copy()
    two[2:] = 0.0
    probs = [(o[:0], i[:0], w[:0], R0, t0), (o, i, two, R0, t0), (o, i, w, R0, t0 * [1, 1, -1]), (o, i, w * 1e160, R0, t0), (o, i, w, R0, t0)]
    o2, i2, w2, R2, t2 = vote_problem(4, 1600)
    probs += [(o2, i2, w2, R2, t2 * [1, 1, -1]), (o2, i2, w2 * 1e160, R2, t2)]
    got = run(ctx, probs)
    assert got["status"].tolist() == [W.TOO_FEW, W.TOO_FEW, W.BEHIND, W.SINGULAR, W.CONVERGED, W.BEHIND, W.SINGULAR]
    for p in (0, 1, 2, 3, 5, 6):
        assert np.array_equal(got["R"][p], probs[p][3]) and np.array_equal(got["t"][p], probs[p][4]) and not got["pose_cov"][p].any()
        assert got["cost_final"][p] == got["cost_init"][p]
        want = W.refine_weighted(*probs[p][:3], K4A, *probs[p][3:])
        assert got["iterations"][p] == want["iterations"] and np.abs(got["rvec"][p] - want["rvec"]).max() < 1e-12
    r = run(ctx, [probs[4]], max_iterations=1, function_tol=0.0)
    assert r["status"][0] == W.MAX_ITER and r["iterations"][0] == 2 and r["cost_final"][0] < r["cost_init"][0]
    r = run(ctx, [probs[4]], max_iterations=0)
    assert r["status"][0] == W.MAX_ITER and r["iterations"][0] == 1 and r["cost_final"][0] == r["cost_init"][0]
    good = [dev(np.array([0, 8], np.int32), torch.int32), dev(o), dev(i), dev(w), dev(K4A[None]), dev(R0[None]), dev(t0[None])]
    bad = {0: [dev(np.array([0, 9], np.int32), torch.int32), dev(np.array([1, 8], np.int32), torch.int32), dev(np.array([0, 9, 8], np.int32), torch.int32),
               dev(np.array([0, 8], np.int64), torch.int64), torch.tensor([0, 8], dtype=torch.int32)],
           1: [dev(o).float(), dev(o[:7]), torch.from_numpy(o)], 2: [dev(o)], 3: [dev(w[:, :2])], 4: [dev(K4A[None, :3])],
           5: [dev(R0)], 6: [dev(np.stack([t0, t0]))]}
    for k, alts in bad.items():
        for alt in alts:
            args = list(good)
            args[k] = alt
            with pytest.raises(ValueError):
                ops.pnp_refine_weighted(ctx, *args)
    for kw in (dict(max_iterations=-1), dict(gradient_tol=-1.0), dict(function_tol=float("nan"))):
        with pytest.raises(ValueError):
            ops.pnp_refine_weighted(ctx, *good, **kw)
    img = dev(np.zeros((16, 2)))
    for args, kw in (((dev(np.array([0, 12, 16], np.int32), torch.int32), img), {}), ((good[0], img), {}), ((good[0], img[:8]), dict(mode="huber")),
                     ((good[0], img[:8]), dict(sigma_floor=-1.0)), ((good[0], img[:8]), dict(points_per_vote=3)),
                     ((good[0], img[:8]), dict(vote_weight=dev(np.ones(2)))), ((good[0], img[:8]), dict(inlier_mask=dev(np.ones(8)))),
                     ((good[0], img[:8].float()), {})):
        with pytest.raises(ValueError):
            ops.vote_stats(ctx, *args, **kw)


def test_vote_stats_matches_the_restatement(ctx):
    from pyrapose_amd import ops
    rng = np.random.default_rng(3)
    ks = [40, 7, 1, 0, 13, 300]
    offs = np.concatenate([[0], np.cumsum([8 * k for k in ks])]).astype(np.int32)
    img = rng.normal(scale=4.0, size=(offs[-1], 2)) + 300.0
    score = rng.uniform(0.5, 1.0, offs[-1] // 8)
    mask = (rng.uniform(size=offs[-1]) < 0.8).astype(np.uint8)
    img[offs[1] + 5: offs[2]: 8] = [100.0, 50.0]
    for sc_, mk in ((None, None), (score, None), (None, mask), (score, mask)):
        for mode, name in ((W.FULL, "full"), (W.ISO, "iso")):
            want = W.vote_stats(img, offs, 8, sc_, mk, mode, 0.5)
            got = ops.vote_stats(ctx, dev(offs, torch.int32), dev(img), 8, None if sc_ is None else dev(sc_),
                                 None if mk is None else dev(mk, torch.uint8), name, 0.5)
            assert np.array_equal(got["count"].cpu().numpy(), want["count"])
            for k in ("wsum", "mu", "n_eff"):
                np.testing.assert_allclose(got[k].cpu().numpy(), want[k], rtol=1e-12, atol=0, err_msg=k)
            # second moments and what follows from them: 1e-12 relative to the variances (the xy term cancels)
            scale = np.abs(want["cov"]).max(-1, keepdims=True)
            # (+ 1e-18 px^2: identical votes leave second moments of the order of the mean's rounding squared, not zeros)
            assert (np.abs(got["cov"].cpu().numpy() - want["cov"]) <= 1e-12 * scale + 1e-18).all()
            wscale = np.abs(want["wgt"]).max(-1, keepdims=True)
            assert (np.abs(got["wgt"].cpu().numpy() - want["wgt"]) <= 1e-12 * wscale).all()


def test_reference_signatures(ctx):
    from pyrapose_amd.utils import un_pnp_utils as U
    sc = scene(5)
    uv = project(sc["R"], sc["t"], BOX)
    w = np.tile([1.0, 0.0, 1.0], (8, 1)) * np.linspace(0.5, 2.0, 8)[:, None]
    Rt = U.uncertainty_pnp(uv.astype(np.float64), w, BOX.astype(np.float32), KMAT, init=(sc["R0"], sc["t0"]))
    assert Rt.shape == (3, 4) and np.abs(Rt[:, :3] - sc["R"]).max() < 1e-9 and np.abs(Rt[:, 3] - sc["t"]).max() < 1e-9 * sc["t"][2]
    Rt = U.uncertainty_pnp(uv, w, BOX, KMAT)                                      # seeded by the RANSAC solver
    assert np.abs(Rt[:, :3] - sc["R"]).max() < 1e-9 and np.abs(Rt[:, 3] - sc["t"]).max() < 1e-9 * sc["t"][2]
    cov = np.tile(np.array([[2.0, 0.5], [0.5, 1.0]]), (8, 1, 1)) * np.linspace(1, 3, 8)[:, None, None]
    cov[3] = 0.0                                                                  # cov_xx < 1e-5: the point drops out
    Rt = U.uncertainty_pnp_v2(uv, cov, BOX, KMAT, init=(sc["R0"], sc["t0"]))
    assert Rt.shape == (3, 4) and np.abs(Rt[:, :3] - sc["R"]).max() < 1e-9
    wv2 = U.weights_from_covars(cov)
    assert wv2[3].tolist() == [0, 0, 0] and np.isclose(wv2[0, 0], 1.0 / np.linalg.eigvalsh(cov[0]).max()) and not wv2[:, 1].any()
    Rt = U.uncertainty_pnp(uv[:4], w[:4], BOX[:4], KMAT, init=(sc["R0"], sc["t0"]))  # pn == 4: the seed
    assert np.array_equal(Rt[:, :3], sc["R0"]) and np.array_equal(Rt[:, 3], sc["t0"])
    out = U.uncertainty_pnp_batch([(uv, w, BOX, KMAT)] * 3, init=[(sc["R0"], sc["t0"])] * 3)
    assert len(out) == 3 and all(o["status"] == W.CONVERGED and o["pose_cov"].shape == (6, 6) and o["cost"] < 1e-12 for o in out)
    assert U.uncertainty_pnp_batch([]) == []


def scripted_outputs(rng):
    """like test_poses_from_prediction_outputs, the votes of every corner with their own anisotropic noise"""
    B, N, C = 4, 3000, 3
    boxes3D = rng.uniform(0, 600, size=(B, N, 16)).astype(np.float32)
    scores = rng.uniform(0.0, 0.3, size=(B, N, C)).astype(np.float32)
    corners = np.stack([BOX, BOX * 0.7, BOX * np.array([1.2, 0.8, 1.0])])
    truth = {}
    for n_, (b, c, k) in enumerate((b, c, 40) for b in range(B) for c in range(C)):
        sc = scene(1100 + n_, k, corners[c])
        anchors = np.sort(rng.choice(N, size=k, replace=False))
        boxes3D[b, anchors] = sc["votes"].reshape(k, 16).astype(np.float32)
        scores[b, anchors, c] = rng.uniform(0.55, 0.99, size=k).astype(np.float32)
        truth[(b, c)] = (sc["R"], sc["t"])
    return boxes3D, scores, corners, truth


def test_poses_from_outputs_weighting(ctx):
    from pyrapose_amd.utils import pose_decode
    boxes3D, scores, corners, truth = scripted_outputs(np.random.default_rng(8))
    base = pose_decode.poses_from_outputs(boxes3D, scores, corners, KMAT, seed=3, ctx=ctx)
    none = pose_decode.poses_from_outputs(boxes3D, scores, corners, KMAT, seed=3, ctx=ctx, weighting=None)
    assert len(base) == 12
    for a, b in zip(base, none):
        assert sorted(a) == sorted(b) == ["R", "cls", "image", "inliers", "ok", "t", "votes"]
        assert all(np.array_equal(a[k], b[k]) for k in a)
    cor = pose_decode.poses_from_outputs(boxes3D, scores, corners, KMAT, seed=3, ctx=ctx, weighting="corners")
    e_ref, e_ran = [], []
    for a, o in zip(base, cor):
        R, t = truth[(o["image"], o["cls"])]
        assert o["ok"] and o["refine_status"] == W.CONVERGED and np.array_equal(o["R_ransac"], a["R"]) and np.array_equal(o["t_ransac"], a["t"])
        assert np.array_equal(o["inliers"], a["inliers"]) and o["cost"] <= o["cost_ransac"] and o["pose_cov"].shape == (6, 6)
        e_ref.append(rot_err_deg(o["R"], R))
        e_ran.append(rot_err_deg(o["R_ransac"], R))
    print("median rotation error: refined %.3f deg, RANSAC %.3f deg" % (np.median(e_ref), np.median(e_ran)))
    assert np.median(e_ref) < np.median(e_ran)
    sco = pose_decode.poses_from_outputs(boxes3D, scores, corners, KMAT, seed=3, ctx=ctx, weighting="scores")
    for a, o in zip(base, sco):
        assert o["refine_status"] in (W.CONVERGED, W.MAX_ITER) and o["cost"] <= o["cost_ransac"]
        # the cost of the RANSAC pose under the same weights, recomputed on the host
        k = len(a["votes"])
        s = np.repeat(scores[o["image"], a["votes"], o["cls"]].astype(np.float64), 8)
        m = np.zeros(8 * k)
        m[a["inliers"]] = 1.0
        wgt = np.stack([s * m, np.zeros(8 * k), s * m], 1)
        x = np.concatenate([W.so3_log(a["R"]), a["t"]])
        img = boxes3D[o["image"], a["votes"]].astype(np.float64).reshape(-1, 2)
        c0 = W.evaluate(x, np.tile(corners[o["cls"]], (k, 1)), img, wgt, K4A)[0]
        assert abs(c0 - o["cost_ransac"]) <= 1e-9 * c0 and o["cost"] <= c0 * (1 + 1e-12)
    with pytest.raises(ValueError):
        pose_decode.poses_from_outputs(boxes3D, scores, corners, KMAT, ctx=ctx, weighting="votes")
    assert pose_decode.poses_from_outputs(boxes3D, scores, corners, KMAT, threshold=0.995, ctx=ctx, weighting="corners") == []


def test_evaluate_add_with_weighting_reproduces_the_counters(ctx):
    """the scripted network of test_gpu_pnp.test_evaluate_add_loop_on_a_scripted_network through weighting='corners'"""
    from oracle import pnp_np as P
    from pyrapose_amd.utils import eval_pose
    rng = np.random.default_rng(12)
    C, N, H, Wd = 3, 2000, 480, 640
    boxes = np.stack([BOX, BOX * 0.8, BOX * 1.1]) * 0.001
    pts = [rng.uniform(-1, 1, (300, 3)) * np.abs(b).max(0) for b in boxes]
    dia = [float(np.linalg.norm(b.max(0) - b.min(0))) for b in boxes]

    def axis_angle_to_quat(w):
        th = np.linalg.norm(w)
        return np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * w / th])

    cases = []
    for lab, kind in ((0, "good"), (1, "wrong"), (2, "few"), (1, "good")):
        w = rng.normal(size=3)
        t = np.array([rng.uniform(-100, 100), rng.uniform(-80, 80), rng.uniform(600, 1000)])
        cases.append((lab, axis_angle_to_quat(w), t, kind))

    class Gen(object):
        def size(self): return len(cases)
        def load_image(self, i): return np.full((H, Wd, 3), i, np.uint8)
        def preprocess_image(self, x): return x.astype(np.float32)
        def resize_image(self, x): return x, 1.0
        def load_annotations(self, i):
            lab, q, t, _ = cases[i]
            return {"labels": np.array([float(lab)]), "poses": np.array([np.concatenate([t, q])])}

    def predict(x):
        i = int(x[0, 0, 0, 0])
        lab, q, t, kind = cases[i]
        R = eval_pose.quat2mat(q)
        if kind == "wrong":
            R = P.so3_exp(np.array([0.0, 0.0, 1.2])) @ R
        k = 5 if kind == "few" else 40
        uv = project(R, t * 0.001, boxes[lab])
        b3 = rng.uniform(0, 600, (1, N, 16)).astype(np.float32)
        sc = rng.uniform(0, 0.2, (1, N, C)).astype(np.float32)
        anchors = np.sort(rng.choice(N, k, replace=False))
        b3[0, anchors] = (uv[None] + rng.normal(scale=0.8, size=(k, 8, 2))).reshape(k, 16)
        sc[0, anchors, lab] = 0.9
        return [b3, sc, np.zeros((1, 4800, C), np.float32)]

    for weighting in ("corners", "scores"):
        out = eval_pose.evaluate_add(Gen(), predict, boxes, pts, dia, symmetric_classes=(2,), weighting=weighting)
        assert out["allPoses"].tolist() == [0, 1, 2, 1]
        assert out["trueDets"].tolist() == [0, 1, 2, 0] and out["truePoses"].tolist() == [0, 1, 1, 0]
        assert abs(out["recall_all"] - 0.5) < 1e-12 and len(out["errors"]) == 3
