"""GPU: BOP's symmetry-aware pose errors MSSD / MSPD (pp_pose_mssd_f64 / pp_pose_mspd_f64, ops.pose_mssd / pose_mspd,
utils.pose_error.mssd / mspd) against the float64 numpy restatement tests/pose_sym_np.py -- bit for bit: the same IEEE
operations in the same order, maxima and minima exact -- their identities, and utils.eval_pose.evaluate_pose_metrics with
symmetry sets on the scripted network of tests/test_gpu_pose_metrics.py."""
import numpy as np
import pytest
import torch

from tests import pose_sym_np as SN
from tests import render_np as RN

pytestmark = pytest.mark.gpu

N_SYM = (1, 2, 7, 8, 9, 17)          # around the kernel's chunk of 8 symmetries
N_POSE = (1, 3)
# (ranges, offset): n_pts = ranges * ops.POSE_SYM_RANGE + offset -- around the tile of 256 threads and around one range
N_PTS = [(0, 1), (0, 255), (0, 256), (0, 257), (0, 1500), (1, -1), (1, 0), (1, 1)]
K = SN.K_LINEMOD


def both(pts, S_R, S_t, R_est, t_est, R_gt, t_gt):
    """(mssd, its symmetry, mspd, its symmetry) from the device and from the restatement"""
    from pyrapose_amd.utils import pose_error as PE
    syms = (S_R, S_t)
    got = PE.mssd_batch(R_est, t_est, R_gt, t_gt, pts, syms, return_sym=True) + PE.mspd_batch(R_est, t_est, R_gt, t_gt, K, pts, syms, return_sym=True)
    want = SN.mssd_np(pts, S_R, S_t, R_est, t_est, R_gt, t_gt) + SN.mspd_np(pts, S_R, S_t, K, R_est, t_est, R_gt, t_gt)
    return got, want


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("mssd", "sym_mssd", "mspd", "sym_mspd")):
        print(what, name, "device", g, "restatement", w)
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g, w), (what, name, g, w)


def on_symmetry(R_gt, t_gt, S_R, S_t, k):
    """the ground truth composed with symmetry k on the host (BLAS): an estimate whose best symmetry is k"""
    return R_gt @ S_R[k], (R_gt @ S_t[k].reshape(3, 1)).reshape(-1, 3) + t_gt


@pytest.mark.parametrize("ranges,offset", N_PTS)
def test_both_metrics_equal_the_restatement_bit_for_bit(ranges, offset):
    from pyrapose_amd import ops
    assert ops.POSE_SYM_CHUNK == 8
    n_pts = ranges * ops.POSE_SYM_RANGE + offset
    rng = np.random.default_rng(1000 * ranges + offset)
    for n_pose in N_POSE:
        pts, R_est, t_est, R_gt, t_gt = SN.scene(rng, n_pose, n_pts)
        for n_sym in N_SYM:
            S_R, S_t = SN.random_symmetries(rng, n_sym)
            k = n_sym - 1
            R_est[0], t_est[0] = [a[0] for a in on_symmetry(R_gt[:1], t_gt[:1], S_R, S_t, k)]   # pose 0: the last symmetry wins
            R_est[0] = SN.axis_angle([0.0, 0.01, 0.0]) @ R_est[0]
            got, want = both(pts, S_R, S_t, R_est, t_est, R_gt, t_gt)
            assert_same(got, want, "n_pts %d n_sym %d n_pose %d" % (n_pts, n_sym, n_pose))
            assert want[1][0] == k and (want[0] > 0).all() and (want[2] > 0).all()


def test_more_symmetries_than_threads_of_the_finishing_workgroup():
    rng = np.random.default_rng(7)
    pts, R_est, t_est, R_gt, t_gt = SN.scene(rng, 2, 300)
    S_R, S_t = SN.random_symmetries(rng, 300)
    R_est[1], t_est[1] = [a[0] for a in on_symmetry(R_gt[1:], t_gt[1:], S_R, S_t, 270)]
    got, want = both(pts, S_R, S_t, R_est, t_est, R_gt, t_gt)
    assert_same(got, want, "n_sym 300")
    assert got[1].tolist() == [0, 270] and got[3].tolist() == [0, 270]


def test_identity_set_is_the_plain_maximum_and_bounds_add():
    from pyrapose_amd.utils import pose_error as PE
    rng = np.random.default_rng(11)
    pts, R_est, t_est, R_gt, t_gt = SN.scene(rng, 3, 700)
    d = np.stack([np.linalg.norm(np.stack(SN.rigid(R_est[i], t_est[i], pts)) - np.stack(SN.rigid(R_gt[i], t_gt[i], pts)), axis=0).max()
                  for i in range(3)])
    for syms in (None, [], SN.random_symmetries(rng, 1)):
        e, s = PE.mssd_batch(R_est, t_est, R_gt, t_gt, pts, syms, return_sym=True)
        assert np.array_equal(e, SN.mssd_np(pts, np.eye(3)[None], np.zeros((1, 3)), R_est, t_est, R_gt, t_gt)[0]) and s.tolist() == [0, 0, 0]
        np.testing.assert_allclose(e, d, rtol=1e-12)           # (np.linalg.norm sums the squares in its own order)
        assert (e >= PE.add_batch(R_est, t_est, R_gt, t_gt, pts)).all()


def test_estimate_equal_to_ground_truth_is_exactly_zero():
    from pyrapose_amd.utils import pose_error as PE
    rng = np.random.default_rng(12)
    pts, _R, _t, R_gt, t_gt = SN.scene(rng, 3, 400)
    syms = SN.random_symmetries(rng, 9)
    for e, s in (PE.mssd_batch(R_gt, t_gt, R_gt, t_gt, pts, syms, return_sym=True), PE.mspd_batch(R_gt, t_gt, R_gt, t_gt, K, pts, syms, return_sym=True)):
        assert np.array_equal(e, np.zeros(3)) and s.tolist() == [0, 0, 0]


@pytest.mark.parametrize("k", [1, 7, 8, 16])
def test_estimate_on_symmetry_k_is_found(k):
    from pyrapose_amd.utils import pose_error as PE
    rng = np.random.default_rng(20 + k)
    pts, _R, _t, R_gt, t_gt = SN.scene(rng, 3, 900)
    S_R, S_t = SN.random_symmetries(rng, 17)
    R_est, t_est = on_symmetry(R_gt, t_gt, S_R, S_t, k)
    diameter = np.linalg.norm(pts[:, None] - pts[None], axis=2).max()
    e3, s3 = PE.mssd_batch(R_est, t_est, R_gt, t_gt, pts, (S_R, S_t), return_sym=True)
    e2, s2 = PE.mspd_batch(R_est, t_est, R_gt, t_gt, K, pts, (S_R, S_t), return_sym=True)
    print("on symmetry", k, "mssd", e3, "mspd", e2, "diameter", diameter)
    assert s3.tolist() == [k] * 3 and s2.tolist() == [k] * 3
    # composed once with BLAS and once on the device: rounding of coordinates of about 1e3 mm, some 1e-13 mm; a pixel is
    # f / z <= 572 / 400 = 1.4 times that
    assert (e3 <= 1e-9 * diameter).all() and (e2 <= 1e-9 * diameter).all()


def test_duplicated_symmetry_reports_the_lower_index():
    from pyrapose_amd.utils import pose_error as PE
    rng = np.random.default_rng(31)
    pts, _R, _t, R_gt, t_gt = SN.scene(rng, 2, 300)
    S_R, S_t = SN.random_symmetries(rng, 20)
    k = 3
    for later in (5, 12, 19):                                        # in the same chunk of 8 symmetries, and in later ones
        D_R, D_t = S_R.copy(), S_t.copy()
        D_R[later], D_t[later] = S_R[k], S_t[k]
        R_est, t_est = on_symmetry(R_gt, t_gt, D_R, D_t, k)
        R_est = np.stack([SN.axis_angle([0.02, 0.0, 0.01]) @ R for R in R_est])
        got, want = both(pts, D_R, D_t, R_est, t_est, R_gt, t_gt)
        assert_same(got, want, "duplicate at %d" % later)
        per = SN.per_symmetry(pts, D_R, D_t, R_est[0], t_est[0], R_gt[0], t_gt[0])
        assert per[k] == per[later] == per.min()
        assert got[1].tolist() == [k, k] and got[3].tolist() == [k, k]
    # the identity twice
    D_R, D_t = np.stack([np.eye(3)] * 3), np.zeros((3, 3))
    e, s = PE.mssd_batch(R_gt, t_gt + 1.0, R_gt, t_gt, pts, (D_R, D_t), return_sym=True)
    assert s.tolist() == [0, 0] and (e > 0).all()


def test_more_symmetries_never_raise_the_error():
    from pyrapose_amd.utils import pose_error as PE
    rng = np.random.default_rng(41)
    pts, R_est, t_est, R_gt, t_gt = SN.scene(rng, 3, 500)
    S_R, S_t = SN.random_symmetries(rng, 17)
    S_R[5], S_t[5] = SN.axis_angle([0.0, 0.0, 0.03]), np.array([0.5, 0.0, 0.0])   # near the identity: it can win
    R_est[1], t_est[1] = [a[0] for a in on_symmetry(R_gt[1:2], t_gt[1:2], S_R, S_t, 5)]
    for n in (2, 8, 17):
        assert (PE.mssd_batch(R_est, t_est, R_gt, t_gt, pts, (S_R[:n], S_t[:n])) <= PE.mssd_batch(R_est, t_est, R_gt, t_gt, pts, (S_R[:1], S_t[:1]))).all()
        assert (PE.mspd_batch(R_est, t_est, R_gt, t_gt, K, pts, (S_R[:n], S_t[:n])) <= PE.mspd_batch(R_est, t_est, R_gt, t_gt, K, pts, (S_R[:1], S_t[:1]))).all()
    assert PE.mssd_batch(R_est, t_est, R_gt, t_gt, pts, (S_R, S_t))[1] < 0.01 * PE.mssd_batch(R_est, t_est, R_gt, t_gt, pts, None)[1]


def test_flipped_symmetric_cuboid():
    from pyrapose_amd.utils import pose_error as PE
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations
    g = np.linspace(-1.0, 1.0, 7)
    pts = np.array([[x, y, z] for x in g for y in g for z in g if max(abs(x), abs(y), abs(z)) == 1.0]) * np.array([40.0, 25.0, 60.0])
    diameter = 2.0 * np.linalg.norm([40.0, 25.0, 60.0])
    half_turn = np.diag([-1.0, -1.0, 1.0, 1.0])                     # about the cuboid's z axis
    syms = get_symmetry_transformations({"diameter": diameter, "symmetries_discrete": [half_turn.reshape(-1).tolist()]})
    R_gt, t_gt = SN.random_rotation(np.random.default_rng(51)), np.array([30.0, -20.0, 700.0])
    R_est = R_gt @ half_turn[:3, :3]                                # the object turned by 180 degrees about its own z axis
    plain = PE.mssd(R_est, t_gt, R_gt, t_gt, pts, None)
    sym = PE.mssd_batch(R_est, t_gt, R_gt, t_gt, pts, syms, return_sym=True)
    print("flipped cuboid: mssd identity", plain, "with the half-turn", sym, "diameter", diameter)
    assert plain > 0.5 * diameter
    assert sym[0][0] < 1e-9 * diameter and sym[1][0] == 1
    assert PE.mspd(R_est, t_gt, R_gt, t_gt, K, pts, syms) < 1e-9 * diameter < 5.0 < PE.mspd(R_est, t_gt, R_gt, t_gt, K, pts, None)
    assert PE.adi(R_est, t_gt, R_gt, t_gt, pts) < 1e-9 * diameter   # ADD-S agrees here; it is the non-symmetric flips it forgives


def test_ops_without_best_sym_and_bad_arguments():
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    ctx = default_context()
    rng = np.random.default_rng(61)
    pts, R_est, t_est, R_gt, t_gt = SN.scene(rng, 3, 300)
    S_R, S_t = SN.random_symmetries(rng, 9)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    p, sr, st, re_, te_, rg, tg = (dev(a) for a in (pts, S_R, S_t, R_est, t_est, R_gt, t_gt))
    k9 = dev(np.broadcast_to(K, (3, 3, 3)))
    e3, s3 = ops.pose_mssd(ctx, p, sr, st, re_, te_, rg, tg)
    e2, s2 = ops.pose_mspd(ctx, p, sr, st, k9, re_, te_, rg, tg)
    assert e3.is_cuda and e3.dtype == torch.float64 and s3.dtype == torch.int32 and tuple(s3.shape) == (3,)
    n3, none3 = ops.pose_mssd(ctx, p, sr, st, re_, te_, rg, tg, best_sym=False)        # best_sym = NULL
    n2, none2 = ops.pose_mspd(ctx, p, sr, st, k9, re_, te_, rg, tg, best_sym=False)
    assert none3 is None and none2 is None and torch.equal(n3, e3) and torch.equal(n2, e2)
    want = SN.mssd_np(pts, S_R, S_t, R_est, t_est, R_gt, t_gt)
    assert np.array_equal(e3.cpu().numpy(), want[0]) and np.array_equal(s3.cpu().numpy(), want[1])
    with pytest.raises(ValueError):                                  # n_sym = 0
        ops.pose_mssd(ctx, p, sr[:0], st[:0], re_, te_, rg, tg)
    with pytest.raises(ValueError):
        ops.pose_mspd(ctx, p, sr[:0], st[:0], k9, re_, te_, rg, tg)
    with pytest.raises(ValueError):                                  # S_R and S_t of different lengths
        ops.pose_mssd(ctx, p, sr, st[:8], re_, te_, rg, tg)
    with pytest.raises(ValueError):
        ops.pose_mspd(ctx, p, sr[:8], st, k9, re_, te_, rg, tg)
    with pytest.raises(ValueError):                                  # a host tensor
        ops.pose_mssd(ctx, p.cpu(), sr, st, re_, te_, rg, tg)
    with pytest.raises(ValueError):
        ops.pose_mspd(ctx, p, sr, st, k9.cpu(), re_, te_, rg, tg)
    with pytest.raises(ValueError):                                  # float32
        ops.pose_mssd(ctx, p.float(), sr, st, re_, te_, rg, tg)
    with pytest.raises(ValueError):                                  # no poses, no points
        ops.pose_mssd(ctx, p, sr, st, re_[:0], te_[:0], rg[:0], tg[:0])
    with pytest.raises(ValueError):
        ops.pose_mssd(ctx, p[:0], sr, st, re_, te_, rg, tg)
    torch.cuda.synchronize()


def test_single_pose_forms_equal_the_batch():
    from pyrapose_amd.utils import mspd, mssd, pose_error as PE
    assert mssd is PE.mssd and mspd is PE.mspd
    rng = np.random.default_rng(71)
    pts, R_est, t_est, R_gt, t_gt = SN.scene(rng, 3, 300)
    S_R, S_t = SN.random_symmetries(rng, 9)
    syms = [{"R": S_R[s], "t": S_t[s].reshape(3, 1)} for s in range(9)]    # the list form
    e3 = PE.mssd_batch(R_est, t_est, R_gt, t_gt, pts, (S_R, S_t))
    e2 = PE.mspd_batch(R_est, t_est, R_gt, t_gt, K, pts, (S_R, S_t))
    for i in range(3):
        one3 = PE.mssd(R_est[i], t_est[i].reshape(3, 1), R_gt[i], t_gt[i].reshape(3, 1), pts, syms)
        one2 = PE.mspd(R_est[i], t_est[i].reshape(3, 1), R_gt[i], t_gt[i].reshape(3, 1), K, pts, syms)
        assert isinstance(one3, float) and isinstance(one2, float) and one3 == e3[i] and one2 == e2[i]


# ---- evaluate_pose_metrics on the scripted network of tests/test_gpu_pose_metrics.py (the same fixtures, rebuilt here) ----
Cn, N, H, W = 3, 2000, 480, 640
SIZES = [(0.08, 0.06, 0.11), (0.064, 0.048, 0.088), (0.088, 0.066, 0.121)]    # metres
RESULT_KEYS = {"allPoses", "trueDets", "less5", "rep_less5", "vsd_less_t", "trueDets_rate", "less5_rate", "rep_less5_rate",
               "vsd_less_t_rate", "add_less_rate", "add_less", "add_fractions", "errors"}
ERROR_KEYS = {"image", "cls", "ok", "re", "te", "reproj", "vsd", "add"}
SYM_RESULT_KEYS = {"mssd_less", "mspd_less", "mssd_less_rate", "mspd_less_rate", "ar_mssd", "ar_mspd", "bop_fractions", "bop_pixels"}
SYM_ERROR_KEYS = {"mssd", "mspd", "sym_mssd", "sym_mspd"}


def scripted_evaluation(**kw):
    from pyrapose_amd.utils import eval_pose
    from pyrapose_amd.utils.renderer import render
    rng = np.random.default_rng(5)
    models = [RN.box_mesh(*s) for s in SIZES]
    boxes = np.stack([m["pts"] for m in models])
    dia = [float(np.linalg.norm(np.asarray(s))) for s in SIZES]

    def axis_angle(w):
        th = np.linalg.norm(w)
        k = w / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx, np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * k])

    cases = []  # (label, gt R, gt quaternion, gt t [mm], what the network votes for)
    for lab, kind in ((0, "good"), (1, "wrong"), (2, "good"), (1, "shifted")):
        R, q = axis_angle(rng.normal(size=3))
        t = np.array([rng.uniform(-60, 60), rng.uniform(-40, 40), rng.uniform(600, 900)])
        cases.append((lab, R, q, t, kind))

    class Gen(object):
        def size(self): return len(cases)
        def load_image(self, i): return np.full((H, W, 3), i, np.uint8)
        def preprocess_image(self, x): return x.astype(np.float32)
        def resize_image(self, x): return x, 1.0
        def load_annotations(self, i):
            lab, _R, q, t, _ = cases[i]
            return {"labels": np.array([float(lab)]), "poses": np.array([np.concatenate([t, q])])}

    def load_depth(i):  # the scene: the object at its ground-truth pose, millimetres, as uint16 sensor depth
        lab, _R, q, t, _ = cases[i]
        mm = dict(models[lab], pts=models[lab]["pts"] * 1000.0)
        return np.round(render(mm, (W, H), K, eval_pose.quat2mat(q), t)).astype(np.uint16)

    def predict(x):
        i = int(x[0, 0, 0, 0])
        lab, _R, q, t, kind = cases[i]
        R, tt = eval_pose.quat2mat(q), t * 0.001
        if kind == "wrong":
            R = axis_angle(np.array([0.0, 0.0, 1.2]))[0] @ R
        if kind == "shifted":
            tt = tt + np.array([0.0, 0.0, 0.25])                    # 25 cm deeper: every metric but the rotation fails
        Xc = boxes[lab] @ R.T + tt
        uv = np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1)
        b3 = rng.uniform(0, 600, (1, N, 16)).astype(np.float32)
        sc = rng.uniform(0, 0.2, (1, N, Cn)).astype(np.float32)
        anchors = np.sort(rng.choice(N, 40, replace=False))
        b3[0, anchors] = (uv[None] + rng.normal(scale=0.05, size=(40, 8, 2))).reshape(40, 16)
        sc[0, anchors, lab] = 0.9
        return [b3, sc, np.zeros((1, 4800, Cn), np.float32)]

    out = eval_pose.evaluate_pose_metrics(Gen(), predict, boxes, models, dia, load_depth, K, symmetric_classes=(2,), **kw)
    return out, dia


def test_evaluate_pose_metrics_without_symmetries_keeps_its_keys():
    out, _dia = scripted_evaluation()
    assert set(out) == RESULT_KEYS
    assert len(out["errors"]) == 4 and all(set(e) == ERROR_KEYS for e in out["errors"])
    assert out["allPoses"].tolist() == [0, 1, 2, 1] and out["less5"].tolist() == [0, 1, 0, 1]   # as the parent commit counts


def test_evaluate_pose_metrics_with_symmetry_sets():
    from pyrapose_amd.utils import eval_pose
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations
    half_turn = np.diag([-1.0, -1.0, 1.0, 1.0]).reshape(-1).tolist()
    S = get_symmetry_transformations({"symmetries_discrete": [half_turn]})
    symmetries = [None, (np.stack([s["R"] for s in S]), np.stack([s["t"].reshape(3) for s in S])), S]
    out, dia = scripted_evaluation(symmetries=symmetries)
    assert set(out) == RESULT_KEYS | SYM_RESULT_KEYS
    assert len(out["errors"]) == 4 and all(set(e) == ERROR_KEYS | SYM_ERROR_KEYS for e in out["errors"])
    assert eval_pose.BOP_FRACTIONS == (0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5)
    assert eval_pose.BOP_PIXELS == (5, 10, 15, 20, 25, 30, 35, 40, 45, 50)
    assert np.array_equal(out["bop_fractions"], eval_pose.BOP_FRACTIONS) and np.array_equal(out["bop_pixels"], eval_pose.BOP_PIXELS)
    for key in ("mssd_less", "mspd_less"):
        assert out[key].shape == (10, Cn + 1) and out[key].dtype == np.uint32
        assert (np.diff(out[key].astype(np.int64), axis=0) >= 0).all()                 # monotone along the thresholds
    want3, want2 = np.zeros((10, Cn + 1), np.uint32), np.zeros((10, Cn + 1), np.uint32)
    for e in out["errors"]:
        print(e)
        assert e["sym_mssd"] in (0, 1) and e["sym_mspd"] in (0, 1) and (e["cls"] != 0 or e["sym_mssd"] == e["sym_mspd"] == 0)
        if e["ok"]:
            for j in range(10):
                want3[j, e["cls"] + 1] += bool(e["mssd"] < eval_pose.BOP_FRACTIONS[j] * dia[e["cls"]])
                want2[j, e["cls"] + 1] += bool(e["mspd"] < eval_pose.BOP_PIXELS[j] * W / 640.0)
    assert np.array_equal(out["mssd_less"], want3) and np.array_equal(out["mspd_less"], want2)
    all_f = out["allPoses"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rate3, rate2 = np.nan_to_num(want3 / all_f[None]), np.nan_to_num(want2 / all_f[None])
    assert np.array_equal(out["mssd_less_rate"], rate3) and np.array_equal(out["mspd_less_rate"], rate2)
    assert out["ar_mssd"].shape == (Cn + 1,) and np.array_equal(out["ar_mssd"], rate3.mean(axis=0))
    assert np.array_equal(out["ar_mspd"], rate2.mean(axis=0))
    # the good poses are within 5 % of the diameter and 5 px, the wrong and the shifted one of class 1 are not
    assert out["mssd_less"][0].tolist() == [0, 1, 0, 1] and out["mspd_less"][0].tolist() == [0, 1, 0, 1]
    assert out["ar_mssd"][1] == 1.0 and out["ar_mssd"][0] == 0.0
    errs = {(e["image"], e["cls"]): e for e in out["errors"]}
    assert errs[(0, 0)]["mssd"] >= errs[(0, 0)]["add"] and errs[(3, 1)]["mssd"] > 0.2
    # the other keys are what they are without symmetries
    assert out["less5"].tolist() == [0, 1, 0, 1] and out["rep_less5"].tolist() == [0, 1, 0, 1] and out["vsd_less_t"].tolist() == [0, 1, 0, 1]
    with pytest.raises(ValueError):
        scripted_evaluation(symmetries=[None])
