"""GPU: VSD over a range of misalignment tolerances in one pass (pp_vsd_multi_f64 through ops.vsd_multi and
utils.pose_error.vsd_multi_* / visib_fract_batch) against the reference's vectors (tests/golden/pose_metrics.npz), the
single-tau kernel pp_vsd_f64 and the numpy restatement tests/vsd_bop_np.py (pinned to the reference by
tests/test_vsd_bop_cpu.py), and the AR_VSD / AR counters of utils.eval_pose.evaluate_pose_metrics on a scripted network.
The 'step' cost is compared exactly; 'tlinear' within rtol 1e-12, the tolerance of the golden VSD test (float64 sums in
another order than numpy's)."""
import os

import numpy as np
import pytest
import torch

from tests import render_np as RN
from tests import vsd_bop_np as VN

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "pose_metrics.npz"))
BOP_TAUS_90 = [round(0.05 * k, 2) * 90.0 for k in range(1, 11)]       # BOP's ten tolerances of a 90 mm object


def golden_case(c):
    g = lambda k: G["v%d_%s" % (c, k)]
    dt = g("depth_test")
    return (dt[0] if bool(g("shared")) else dt), g("depth_est"), g("depth_gt"), g("K"), g


def same_cost(got, want, cost):
    if cost == "step":
        assert np.array_equal(got, want), (got, want)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def test_reference_vectors_at_two_taus():
    from pyrapose_amd.utils import pose_error as PE
    # golden columns: (step, 0.3, 20), (step, 15, 5), (tlinear, 0.3, 20), (tlinear, 15, 5)
    column = {(str(c), float(d)): (j, float(t)) for j, (c, d, t) in enumerate(zip(G["vsd_cost"], G["vsd_delta"], G["vsd_tau"]))}
    for c in (0, 1, 2):
        dt, de, dg, K, g = golden_case(c)
        assert (c != 1 or dt.ndim == 2) and (c != 2 or dt.shape[-2:] == (540, 720))
        for cost in ("step", "tlinear"):
            for delta in (0.3, 15.0):
                j, tau = column[(cost, delta)]
                e, inter, uni, vis, px = PE.vsd_multi_from_depth(dt, de, dg, K, delta, [5.0, 20.0], cost, "bop18", return_counts=True)
                assert e.shape == (len(de), 2) and e.dtype == np.float64
                same_cost(e[:, [5.0, 20.0].index(tau)], g("vsd")[:, j], cost)
                assert np.array_equal(inter, g("inter")[:, j]) and np.array_equal(uni, g("union")[:, j])
                assert np.array_equal(px, (dg > 0).sum(axis=(1, 2))) and (inter <= vis).all() and (vis <= px).all()
                if c == 0:
                    assert uni[5] == 0 and e[5].tolist() == [1.0, 1.0]               # the empty union: 1.0 at every tau


@pytest.mark.parametrize("cost", ["step", "tlinear"])
def test_columns_carry_the_bits_of_the_single_tau_kernel(cost):
    from pyrapose_amd.utils import pose_error as PE
    for c in (0, 1, 2):
        dt, de, dg, K, _g = golden_case(c)
        e, inter, uni, _vis, _px = PE.vsd_multi_from_depth(dt, de, dg, K, 15.0, BOP_TAUS_90, cost, "bop18", return_counts=True)
        assert e.shape == (len(de), 10)
        for t, tau in enumerate(BOP_TAUS_90):
            one, i1, u1 = PE.vsd_from_depth(dt, de, dg, K, 15.0, tau, cost, return_counts=True)
            same_cost(e[:, t], one, cost)
            assert np.array_equal(inter, i1) and np.array_equal(uni, u1)
        assert (np.diff(e, axis=1) <= 0).all() and (e[:, 0] > e[:, -1]).any()        # the taus do separate the poses


def test_bop19_visibility_against_the_restatement():
    from pyrapose_amd.utils import pose_error as PE
    _dt, de, dg, K, _g = golden_case(0)
    dt = G["v0_depth_test"].copy()
    rows, cols = np.indices(dt.shape[1:])
    dt[(dg > 0) & ((rows + cols) % 4 == 0)[None]] = 0.0                  # missing sensor depth inside every on-screen silhouette
    got = PE.vsd_multi_from_depth(dt, de, dg, K, 15.0, BOP_TAUS_90, "step", "bop19", return_counts=True)
    want = VN.vsd_multi(dt, de, dg, K, 15.0, BOP_TAUS_90, "step", "bop19")
    for a, b in zip(got, want):
        assert np.array_equal(a, b), (a, b)
    old = PE.vsd_multi_from_depth(dt, de, dg, K, 15.0, BOP_TAUS_90, "step", "bop18", return_counts=True)
    on_screen = got[4] > 0
    assert on_screen.tolist() == [True] * 5 + [False]
    # the two rules differ on every on-screen problem: the holes join visib_gt and the union
    assert (got[3][on_screen] > old[3][on_screen]).all() and (got[2][on_screen] > old[2][on_screen]).all()
    assert not np.array_equal(got[0][on_screen], old[0][on_screen])
    assert got[0][5].tolist() == [1.0] * 10


def random_triples(seed, n, h, w):
    rng = np.random.default_rng(seed)
    dg = rng.uniform(400.0, 600.0, (n, h, w))
    de = dg + rng.uniform(-60.0, 60.0, (n, h, w))
    dt = np.round(dg + rng.uniform(-30.0, 30.0, (n, h, w)))
    out = [np.where(rng.uniform(size=(n, h, w)) < 0.3, 0.0, d).astype(np.float32) for d in (dt, de, dg)]
    K = np.array([[31.0, 0.0, w / 2 - 0.3], [0.0, 29.5, h / 2 + 0.2], [0.0, 0.0, 1.0]])
    return out[0], out[1], out[2], K


@pytest.mark.parametrize("hw", [(29, 37), (3, 5)])             # 1073 pixels: one full block of 1024 and a tail of 49; 15: under a wave
@pytest.mark.parametrize("n_tau", [1, 7, 16])
def test_block_edges_on_random_depth(hw, n_tau):
    from pyrapose_amd.utils import pose_error as PE
    dt, de, dg, K = random_triples(11 + n_tau, 3, *hw)
    taus = np.linspace(3.0, 48.0, 16)[:n_tau]
    for cost in ("step", "tlinear"):
        for mode in ("bop18", "bop19"):
            got = PE.vsd_multi_from_depth(dt, de, dg, K, 15.0, taus, cost, mode, return_counts=True)
            want = VN.vsd_multi(dt, de, dg, K, 15.0, taus, cost, mode)
            same_cost(got[0], want[0], cost)
            for a, b in zip(got[1:], want[1:]):
                assert a.dtype == np.int64 and np.array_equal(a, b), (cost, mode, a, b)
            assert (got[2] > 0).all() and (got[1] < got[2]).all() and (got[3] < got[4]).all()     # no degenerate mask
        if n_tau == 1:                                                        # the single-tau entry point, same bits
            one, i1, u1 = PE.vsd_from_depth(dt, de, dg, K, 15.0, float(taus[0]), cost, return_counts=True)
            got = PE.vsd_multi_from_depth(dt, de, dg, K, 15.0, taus, cost, "bop18", return_counts=True)
            same_cost(got[0][:, 0], one, cost)
            assert np.array_equal(got[1], i1) and np.array_equal(got[2], u1)
    # one scene depth shared by the problems
    got = PE.vsd_multi_from_depth(dt[1], de, dg, K, 15.0, taus, "step", "bop19", return_counts=True)
    want = VN.vsd_multi(dt[1], de, dg, K, 15.0, taus, "step", "bop19")
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_tlinear_is_bit_identical_run_to_run():
    from pyrapose_amd.utils import pose_error as PE
    dt, de, dg, K, _g = golden_case(2)
    a = PE.vsd_multi_from_depth(dt, de, dg, K, 15.0, BOP_TAUS_90, "tlinear", "bop19")
    b = PE.vsd_multi_from_depth(dt, de, dg, K, 15.0, BOP_TAUS_90, "tlinear", "bop19")
    assert a.shape == (2, 10) and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert ((a > 0) & (a < 1)).any()


def test_visible_fraction():
    from pyrapose_amd.utils import pose_error as PE
    from pyrapose_amd.utils.renderer import render_depth_batch
    mesh = RN.box_mesh(80.0, 60.0, 110.0)
    K = np.array([[300.0, 0.0, 64.0], [0.0, 300.0, 48.0], [0.0, 0.0, 1.0]])
    c, s = np.cos(0.4), np.sin(0.4)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    t = np.array([[3.0, -2.0, 600.0], [5000.0, 0.0, 600.0]])                # on screen, off screen
    Rs = np.repeat(R[None], 2, 0)
    depth = render_depth_batch(mesh, (128, 96), K, Rs, t).cpu().numpy()
    assert (depth[0] > 0).sum() > 300 and (depth[1] > 0).sum() == 0
    plane = np.where(depth[0] > 0, np.round(depth[0]), 2000.0).astype(np.float32)       # the box in front of a far plane
    free = PE.visib_fract_batch(Rs, t, mesh, plane, K)
    assert free.dtype == np.float64 and free.tolist() == [1.0, 0.0]
    cols = np.flatnonzero((depth[0] > 0).any(axis=0))
    band = slice(int(cols[len(cols) // 4]), int(cols[len(cols) // 2]))          # a quarter of the silhouette's columns
    occluded = plane.copy()
    occluded[:, band] = 300.0                                                   # an occluder in front of the box
    _e, _i, _u, vis, px = VN.vsd_multi(occluded, depth, depth, K, 15.0, [1.0], "step", "bop19")
    got = PE.visib_fract_batch(Rs, t, mesh, occluded, K)
    assert got[0] == vis[0] / px[0] and 0.0 < got[0] < 1.0 and got[1] == 0.0
    assert vis[0] == (depth[0] > 0).sum() - (depth[0][:, band] > 0).sum()
    # without sensor depth in the band the two rules part: 'bop19' sees the box there, 'bop18' does not
    occluded[:, band] = 0.0
    assert PE.visib_fract_batch(Rs, t, mesh, occluded, K)[0] == 1.0
    assert PE.visib_fract_batch(Rs, t, mesh, occluded, K, visib_mode="bop18")[0] == got[0]


def test_refused_arguments_leave_the_context_usable():
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    from pyrapose_amd.utils import pose_error as PE
    dt, de, dg, K = random_triples(3, 2, 8, 8)
    want = VN.vsd_multi(dt, de, dg, K, 15.0, [5.0, 20.0], "step", "bop19")[0]

    def refused(**kw):
        args = dict(depth_test=dt, depth_est=de, depth_gt=dg, K=K, delta=15.0, taus=[5.0, 20.0], cost_type="step", visib_mode="bop19")
        args.update(kw)
        with pytest.raises(ValueError):
            PE.vsd_multi_from_depth(**args)
        assert np.array_equal(PE.vsd_multi_from_depth(dt, de, dg, K, 15.0, [5.0, 20.0]), want)      # the next valid call works

    refused(taus=[])
    refused(taus=list(np.arange(1.0, 18.0)))
    refused(taus=[5.0, 5.0])
    refused(taus=[20.0, 5.0])
    refused(taus=[0.0, 5.0])
    refused(taus=[float("nan")])
    refused(cost_type="quadratic")
    refused(visib_mode="bop20")
    refused(depth_gt=np.zeros((2, 8, 9), np.float32))
    refused(depth_test=np.zeros((3, 8, 8), np.float32))
    with pytest.raises(ValueError):
        PE.vsd_multi_batch(np.eye(3), [0, 0, 500], np.eye(3), [0, 0, 500], RN.box_mesh(1, 1, 1), dt[0], K, 15.0, [5.0], visib_mode="x")
    with pytest.raises(ValueError):
        PE.visib_fract_batch(np.eye(3), [0, 0, 500], RN.box_mesh(1, 1, 1), dt[0], K, visib_mode="x")
    with pytest.raises(ValueError):  # no problems
        ops.vsd_multi(default_context(), torch.zeros((8, 8), device="cuda"), torch.zeros((0, 8, 8), device="cuda"),
                      torch.zeros((0, 8, 8), device="cuda"), torch.zeros((0, 4), dtype=torch.float64, device="cuda"), 15.0, [5.0])
    assert ops.VSD_VISIB == {"bop18": 0, "bop19": 1}


def test_vsd_multi_batch_renders_and_scores_in_one_call():
    from pyrapose_amd.utils import pose_error as PE
    mesh = {"pts": G["mesh_pts"], "faces": G["mesh_faces"]}
    g = lambda k: G["v1_" + k]
    scene = g("depth_test")[0]
    e, inter, uni, vis, px = PE.vsd_multi_batch(g("R_est"), g("t_est"), g("R_gt"), g("t_gt"), mesh, scene, g("K"), 15.0, BOP_TAUS_90,
                                                visib_mode="bop18", return_counts=True)
    assert e.shape == (5, 10)
    for t in (0, 9):                                                             # the same renders through the single-tau path
        assert np.array_equal(e[:, t], PE.vsd_batch(g("R_est"), g("t_est"), g("R_gt"), g("t_gt"), mesh, scene, g("K"), 15.0, BOP_TAUS_90[t]))
    assert e[0].tolist() == [0.0] * 10 and (px > 300).all() and (vis < px).all()  # estimate 0 is the ground truth; the occluder hides a part


# ---- evaluate_pose_metrics on a scripted network, as tests/test_gpu_pose_metrics.py builds it, at 128 x 96 ------------------
Cn, N, H, W = 3, 2000, 96, 128
K_EVAL = np.array([[114.48228, 0.0, 65.05222], [0.0, 114.714086, 48.409798], [0.0, 0.0, 1.0]])
SIZES = [(0.08, 0.06, 0.11), (0.064, 0.048, 0.088), (0.088, 0.066, 0.121)]    # metres


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

    cases = []  # (label, gt quaternion, gt t [mm], what the network votes for)
    for lab, kind in ((0, "good"), (1, "wrong"), (2, "good"), (1, "shifted")):
        _R, q = axis_angle(rng.normal(size=3))
        t = np.array([rng.uniform(-60, 60), rng.uniform(-40, 40), rng.uniform(600, 900)])
        cases.append((lab, q, t, kind))

    class Gen(object):
        def size(self): return len(cases)
        def load_image(self, i): return np.full((H, W, 3), i, np.uint8)
        def preprocess_image(self, x): return x.astype(np.float32)
        def resize_image(self, x): return x, 1.0
        def load_annotations(self, i):
            lab, q, t, _ = cases[i]
            return {"labels": np.array([float(lab)]), "poses": np.array([np.concatenate([t, q])])}

    def load_depth(i):  # the scene: the object at its ground-truth pose, millimetres, as uint16 sensor depth
        lab, q, t, _ = cases[i]
        mm = dict(models[lab], pts=models[lab]["pts"] * 1000.0)
        return np.round(render(mm, (W, H), K_EVAL, eval_pose.quat2mat(q), t)).astype(np.uint16)

    def predict(x):
        i = int(x[0, 0, 0, 0])
        lab, q, t, kind = cases[i]
        R, tt = eval_pose.quat2mat(q), t * 0.001
        if kind == "wrong":
            R = axis_angle(np.array([0.0, 0.0, 1.2]))[0] @ R
        if kind == "shifted":
            tt = tt + np.array([0.0, 0.0, 0.25])                    # 25 cm deeper: every depth difference is past the largest tau
        Xc = boxes[lab] @ R.T + tt
        uv = np.stack([K_EVAL[0, 0] * Xc[:, 0] / Xc[:, 2] + K_EVAL[0, 2], K_EVAL[1, 1] * Xc[:, 1] / Xc[:, 2] + K_EVAL[1, 2]], 1)
        b3 = rng.uniform(0, 120, (1, N, 16)).astype(np.float32)
        sc = rng.uniform(0, 0.2, (1, N, Cn)).astype(np.float32)
        anchors = np.sort(rng.choice(N, 40, replace=False))
        # votes exact to float32: the good poses then render the silhouette of the ground truth pixel for pixel
        b3[0, anchors] = np.repeat(uv[None], 40, 0).reshape(40, 16)
        sc[0, anchors, lab] = 0.9
        return [b3, sc, np.zeros((1, 192, Cn), np.float32)]

    out = eval_pose.evaluate_pose_metrics(Gen(), predict, boxes, models, dia, load_depth, K_EVAL, symmetric_classes=(2,), **kw)
    return out, dia


def same_value(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(same_value(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_evaluation_loop_counts_ar_vsd_and_ar():
    from pyrapose_amd.utils import eval_pose
    plain, dia = scripted_evaluation()
    none, _ = scripted_evaluation(bop_vsd=None)
    assert set(none) == set(plain) and same_value(none, plain)
    assert not {"vsd_bop_less", "ar_vsd", "ar"} & set(plain) and all("vsd_bop" not in e for e in plain["errors"])

    symmetries = [None, None, None]
    out, _ = scripted_evaluation(bop_vsd={}, symmetries=symmetries)
    assert set(out) - set(plain) == {"vsd_bop_less", "vsd_bop_less_rate", "ar_vsd", "ar", "bop_fractions", "bop_pixels", "mssd_less",
                                     "mspd_less", "mssd_less_rate", "mspd_less_rate", "ar_mssd", "ar_mspd"}
    assert len(out["errors"]) == 4
    fr = np.array(eval_pose.BOP_FRACTIONS)
    want = np.zeros((10, 10, Cn + 1), np.uint32)
    for e in out["errors"]:
        print(e["image"], e["cls"], e["ok"], e["vsd"], e["visib_fract"], e["vsd_bop"])
        assert len(e["vsd_bop"]) == 10 and (np.diff(e["vsd_bop"]) <= 0).all()
        if e["ok"]:
            want[:, :, e["cls"] + 1] += np.asarray(e["vsd_bop"])[:, None] < fr[None, :]
    assert out["vsd_bop_less"].dtype == np.uint32 and np.array_equal(out["vsd_bop_less"], want)
    all_f = out["allPoses"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rate = np.nan_to_num(want / all_f[None, None])
    assert np.array_equal(out["vsd_bop_less_rate"], rate)
    assert out["ar_vsd"].shape == (Cn + 1,) and np.array_equal(out["ar_vsd"], rate.mean(axis=(0, 1)))
    assert np.array_equal(out["ar"], (out["ar_vsd"] + out["ar_mssd"] + out["ar_mspd"]) / 3.0)
    errs = {(e["image"], e["cls"]): e for e in out["errors"]}
    assert all(e["ok"] for e in out["errors"])
    assert errs[(0, 0)]["vsd_bop"] == [0.0] * 10 and errs[(2, 2)]["vsd_bop"] == [0.0] * 10       # the perfect detections
    assert errs[(3, 1)]["vsd_bop"] == [1.0] * 10                                                 # 25 cm off in depth
    assert errs[(1, 1)]["vsd_bop"][0] > 0.3
    assert all(e["visib_fract"] == 1.0 for e in out["errors"])                                   # nothing occludes the scenes
    assert out["ar_vsd"][1] == 1.0 and out["ar_vsd"][3] == 1.0 and out["ar_vsd"][0] == 0.0 and out["ar_vsd"][2] < 0.5
    # the keys from before are what they are without bop_vsd: the single-tau VSD runs on the shared renders
    for k in plain:
        if k != "errors":
            assert same_value(out[k], plain[k]), k
    for e, p in zip(out["errors"], plain["errors"]):
        assert all(same_value(e[k], p[k]) for k in p)
    # without symmetries there is ar_vsd and no ar; an unknown setting is refused
    only, _ = scripted_evaluation(bop_vsd=dict(cost_type="tlinear", visib_mode="bop18", delta=10.0))
    assert "ar_vsd" in only and "ar" not in only and "ar_mssd" not in only
    assert errs[(0, 0)]["vsd"] == only["errors"][0]["vsd"]
    with pytest.raises(ValueError):
        scripted_evaluation(bop_vsd=dict(tau=20.0))
