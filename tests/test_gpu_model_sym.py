"""GPU: the symmetry score on the device (pp_sym_hausdorff_f64, ops.sym_hausdorff) against its float64 numpy restatement
tests/model_sym_np.py -- bit for bit, dtype and shape included: the same IEEE operations in the same order, maxima and minima
exact, ties to the lowest index -- at the edges of the source tile, the target tile and the candidate chunk; then
utils.model_info.find_symmetries / symmetry_residuals / model_info(symmetries=...) end to end on the device and into MSSD."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import model_sym_np as SN

pytestmark = pytest.mark.gpu

CENTRE = np.array([1000.0, 1000.0, 1000.0])


def sizes():
    from pyrapose_amd import ops
    T = ops.DIAMETER_TILE
    return [1, 2, T - 1, T, T + 1, 2 * T + 1]


def cand_counts():
    from pyrapose_amd import ops
    c = ops.SYM_HD_CHUNK
    return [1, c - 1, c, c + 1, 2 * c + 1]


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))          # a copy: the shared clouds are read-only, some views reversed
    return (t if dtype is None else t.to(dtype)).cuda()


def device_score(src, tgt, S_R, S_t):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    d2, arg = ops.sym_hausdorff(default_context(), dev(src), None if tgt is None else dev(tgt), dev(S_R), dev(S_t))
    return d2.cpu().numpy(), arg.cpu().numpy()


def assert_same(got, want, what):
    print(what, "device", got[0][:4], got[1][:4].tolist(), "restatement", want[0][:4], want[1][:4].tolist())
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, got, want)


def candidates(rng, K, src):
    """K rigid transformations: random rotations with small shifts; the LAST one carries the source's first point onto the
    origin, where no target is -- a target tail entry read as a zero point would win that candidate's minima by a factor ~1e6"""
    S_R = np.stack([SN.rot(rng.normal(size=3), rng.uniform(0.0, math.pi)) for _ in range(K)])
    S_t = np.stack([CENTRE - R.dot(CENTRE) + rng.uniform(-0.2, 0.2, size=3) for R in S_R])
    S_R[-1] = np.eye(3)
    S_t[-1] = -src[0]
    return S_R, S_t


@pytest.fixture(scope="module")
def clouds():
    """per size one random cloud of extent 1 around (1000, 1000, 1000): a source tail lane taken for a zero point would win the
    maximum by a factor ~3e6; shared by the tests, never written to"""
    rng = np.random.default_rng(11)
    out = {n: CENTRE + rng.uniform(-0.5, 0.5, size=(n, 3)) for n in sizes()}
    for a in out.values():
        a.flags.writeable = False
    return out


@pytest.mark.parametrize("n_tgt", sizes())
@pytest.mark.parametrize("n_src", sizes())
def test_sizes_around_the_tiles_equal_the_restatement(clouds, n_src, n_tgt):
    from pyrapose_amd import ops
    rng = np.random.default_rng(1000 * n_src + n_tgt)
    src, tgt = clouds[n_src], clouds[n_tgt][::-1]
    S_R, S_t = candidates(rng, ops.SYM_HD_CHUNK + 1, src)
    want = SN.sym_hausdorff_np(src, tgt, S_R, S_t)
    assert_same(device_score(src, tgt, S_R, S_t), want, "n_src %d n_tgt %d" % (n_src, n_tgt))
    assert want[0][-1] > 1e6 and (want[0][:-1] < 10.0).all()       # (the test's own construction: nobody is at the origin)


@pytest.mark.parametrize("K", cand_counts())
def test_candidate_counts_around_the_chunk(clouds, K):
    from pyrapose_amd import ops
    T = ops.DIAMETER_TILE
    rng = np.random.default_rng(K)
    src, tgt = clouds[2 * T + 1], clouds[T + 1]
    S_R, S_t = candidates(rng, K, src)
    want = SN.sym_hausdorff_np(src, tgt, S_R, S_t)
    got = device_score(src, tgt, S_R, S_t)
    assert_same(got, want, "K %d" % K)
    assert got[0].shape == (K,) and got[1].shape == (K, 2)
    # every candidate on its own gives what it gives in the launch
    for k in sorted({0, K - 1}):
        one = device_score(src, tgt, S_R[k:k + 1], S_t[k:k + 1])
        assert np.array_equal(one[0], got[0][k:k + 1]) and np.array_equal(one[1], got[1][k:k + 1])


def test_ties_go_to_the_lowest_index():
    """integer coordinates keep the ties exact: the farthest source point three times (two tiles apart), its nearest target
    twice -- the lowest i wins the maximum, the lowest j its minimum; under a quarter turn about z as well"""
    from pyrapose_amd import ops
    T = ops.DIAMETER_TILE
    rng = np.random.default_rng(5)
    n, m = 2 * T + 40, T + 30
    src = rng.integers(-2, 3, size=(n, 3)).astype(np.float64)
    tgt = rng.integers(-2, 3, size=(m, 3)).astype(np.float64)
    src[[T - 3, 7, 2 * T + 9]] = (9.0, 0.0, 0.0)
    tgt[[T + 5, 12]] = (4.0, 0.0, 0.0)                     # the nearest to (9, 0, 0): 25 away, twice
    quarter = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    S_R, S_t = np.stack([np.eye(3), quarter.T]), np.zeros((2, 3))
    want = SN.sym_hausdorff_np(src, tgt, S_R, S_t)
    assert want[0][0] == 25.0 and want[1][0].tolist() == [7, 12]   # (the test's own construction)
    assert_same(device_score(src, tgt, S_R, S_t), want, "ties")
    # every target the same point: each minimum ties over all j
    same = np.tile([[1.0, 2.0, 3.0]], (T + 2, 1))
    want = SN.sym_hausdorff_np(src, same, S_R, S_t)
    assert want[1][:, 1].tolist() == [0, 0]
    assert_same(device_score(src, same, S_R, S_t), want, "one target point repeated")


def test_no_target_means_the_source_and_a_second_call_gives_the_same_bits(clouds):
    from pyrapose_amd import ops
    T = ops.DIAMETER_TILE
    rng = np.random.default_rng(3)
    src = clouds[2 * T + 1]
    S_R, S_t = candidates(rng, 2 * ops.SYM_HD_CHUNK + 1, src)
    first = device_score(src, None, S_R, S_t)
    assert_same(first, SN.sym_hausdorff_np(src, None, S_R, S_t), "tgt None")
    assert_same(device_score(src, src.copy(), S_R, S_t), first, "the source passed twice")
    assert_same(device_score(src, None, S_R, S_t), first, "second call")
    ident = device_score(src, None, np.eye(3)[None], np.zeros((1, 3)))
    assert ident[0].tolist() == [0.0] and ident[1].tolist() == [[0, 0]]


def test_argument_errors():
    from pyrapose_amd import _lib, ops
    from pyrapose_amd.runtime import default_context
    ctx = default_context()
    p, R, t = dev(np.zeros((4, 3))), dev(np.eye(3)[None]), dev(np.zeros((1, 3)))
    for bad in (lambda: ops.sym_hausdorff(ctx, p[:0], None, R, t), lambda: ops.sym_hausdorff(ctx, p, p[:0], R, t),
                lambda: ops.sym_hausdorff(ctx, p, None, R[:0], t[:0]), lambda: ops.sym_hausdorff(ctx, p, None, R, dev(np.zeros((2, 3)))),
                lambda: ops.sym_hausdorff(ctx, p.float(), None, R, t), lambda: ops.sym_hausdorff(ctx, p.cpu(), None, R, t),
                lambda: ops.sym_hausdorff(ctx, p, None, dev(np.zeros((1, 9))), t)):
        with pytest.raises(ValueError):
            bad()
    lib, h = _lib.lib, ctx.handle
    ptr = lambda x: C.c_void_p(x.data_ptr())
    assert lib.pp_sym_hausdorff_workspace_bytes(0, 1) == 0 and lib.pp_sym_hausdorff_workspace_bytes(4, 0) == 0
    assert lib.pp_sym_hausdorff_workspace_bytes((1 << 24) + 1, 1) == 0 and lib.pp_sym_hausdorff_workspace_bytes(4, ops.SYM_HD_MAX_CAND + 1) == 0
    need = lib.pp_sym_hausdorff_workspace_bytes(4, 1)
    assert need >= 12
    ws, d2, arg = torch.empty(need, dtype=torch.uint8, device="cuda"), torch.full((1,), -7.0, dtype=torch.float64, device="cuda"), \
        torch.full((1, 2), -7, dtype=torch.int32, device="cuda")
    call = lambda n_src=4, src=p, n_tgt=4, tgt=p, K=1, SR=R, St=t, w=ws, nb=need, o=d2, a=arg: lib.pp_sym_hausdorff_f64(
        h, n_src, ptr(src) if src is not None else None, n_tgt, ptr(tgt) if tgt is not None else None, K, ptr(SR) if SR is not None else None,
        ptr(St) if St is not None else None, ptr(w) if w is not None else None, nb, ptr(o) if o is not None else None,
        ptr(a) if a is not None else None)
    SHAPE, ARG = -2, -1                                               # PP_ERR_SHAPE, PP_ERR_ARG
    for kw in (dict(n_src=0), dict(n_tgt=0), dict(K=0), dict(n_src=(1 << 24) + 1), dict(n_tgt=(1 << 24) + 1), dict(K=ops.SYM_HD_MAX_CAND + 1)):
        rc = call(**kw)
        msg = lib.pp_last_error_string(h).decode()
        print(kw, rc, msg)
        assert rc == SHAPE and ("16777216" in msg or "65535" in msg)    # the limits are stated
    for kw in (dict(src=None), dict(tgt=None), dict(SR=None), dict(St=None), dict(w=None), dict(o=None), dict(a=None), dict(nb=need - 1)):
        rc = call(**kw)
        print(kw, rc, lib.pp_last_error_string(h).decode())
        assert rc == ARG
    torch.cuda.synchronize()
    assert d2.cpu().tolist() == [-7.0] and arg.cpu().tolist() == [[-7, -7]]   # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert d2.cpu().tolist() == [0.0] and arg.cpu().tolist() == [[0, 0]]


# ---- find_symmetries end to end on the device ---------------------------------------------------------------------------

TOL = 0.01


def shapes():
    """name -> (points in the axis-aligned placement, expected group, continuous axis, count where not the whole group)"""
    heights5, heights9 = [-1.0, -0.5, 0.0, 0.5, 1.0], [0.25 * k - 1.0 for k in range(9)]
    flips = [SN.rot(a, math.pi) for a in np.eye(3)]
    return {"box_2x2x3": (SN.box_grid(2.0, 2.0, 3.0, 0.25), SN.dihedral(4), None, None),
            "box_2x3x4": (SN.box_grid(2.0, 3.0, 4.0, 0.25), flips, None, None),
            "hexagonal_prism": (SN.hex_prism(7, heights5), SN.dihedral(6), None, None),
            "cylinder": (SN.cylinder(180, heights9), SN.dihedral(180)[179:], np.array([0.0, 0.0, 1.0]), 1),
            "cut_box": (SN.cut_box(0.25), [], None, None)}


@pytest.fixture(scope="module")
def found():
    """find_symmetries(tol = 0.01) on the device, once per shape and placement: name -> (points, result, Q)"""
    from pyrapose_amd.utils.model_info import find_symmetries
    out = {}
    for name, (pts, _, _, _) in shapes().items():
        for Q, tag in ((np.eye(3), ""),) + (((SN.fixed_rotation(), "_rotated"),) if name == "box_2x2x3" else ()):
            p = pts.dot(Q.T) + SN.OFFSET
            out[name + tag] = (p, find_symmetries(p, tol=TOL, return_residuals=True), Q)
    return out


@pytest.mark.parametrize("name", ["box_2x2x3", "box_2x2x3_rotated", "box_2x3x4", "hexagonal_prism", "cylinder", "cut_box"])
def test_find_symmetries_finds_the_group(found, name):
    pts, result, Q = found[name]
    _, expected, axis, count = shapes()[name.replace("_rotated", "")]
    print(name, len(pts), "points; residuals / diameter", result.get("residuals_discrete"), result.get("residuals_continuous"))
    if name == "cut_box":
        assert result == {}
        return
    SN.check_result(result, pts, expected, TOL, Q, continuous_axis=axis, count=count)
    assert all(r <= TOL for r in result.get("residuals_discrete", []) + result.get("residuals_continuous", []))


def test_symmetry_residuals_on_the_device_is_the_restatement(found):
    from pyrapose_amd.utils.model_info import symmetry_residuals
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations
    pts, result, _ = found["box_2x2x3_rotated"]
    syms = get_symmetry_transformations(result)
    got, want = symmetry_residuals(pts, syms), symmetry_residuals(pts, syms, _scorer=SN.scorer)
    print("residuals of the found set", got)
    assert got.dtype == np.float64 and got.shape == (8,) and np.array_equal(got, want)


@pytest.mark.parametrize("name", ["box_2x2x3_rotated", "hexagonal_prism", "cylinder"])
def test_found_symmetries_make_mssd_symmetry_aware(found, name):
    """a pose moved by a found element scores <= tol * diameter with the found set, and more than that without it"""
    from pyrapose_amd.utils import pose_error as PE
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations
    pts, result, _ = found[name]
    diameter = SN.diameter_of(pts)
    syms = get_symmetry_transformations(result)
    M = np.asarray(result["symmetries_discrete"][-1]).reshape(4, 4)
    R_gt, t_gt = SN.rot((0.3, -1.0, 0.5), 1.1), np.array([10.0, -20.0, 700.0])
    R_est, t_est = R_gt.dot(M[:3, :3]), R_gt.dot(M[:3, 3]) + t_gt
    with_set = PE.mssd_batch(R_est[None], t_est[None], R_gt[None], t_gt[None], pts, syms)
    without = PE.mssd_batch(R_est[None], t_est[None], R_gt[None], t_gt[None], pts, None)
    e_with, e_without = float(np.asarray(with_set[0]).reshape(-1)[0]), float(np.asarray(without[0]).reshape(-1)[0])
    print(name, "mssd with the found set", e_with, "without", e_without, "tol * diameter", TOL * diameter)
    assert e_with <= TOL * diameter < e_without


def test_model_info_writes_symmetries_that_load_back(found, tmp_path):
    from pyrapose_amd.utils import model_info as MI
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations, load_models_info
    models = {3: found["box_2x3x4"][0], 8: found["cut_box"][0], 11: {"pts": found["cylinder"][0]}}
    plain = MI.models_info(models)
    assert all(sorted(v) == ["diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z"] for v in plain.values())
    info = MI.models_info(models, symmetries=True)
    assert MI.symmetric_ids(info) == [3, 11] and info[8] == plain[8]
    assert info[3]["symmetries_discrete"] == found["box_2x3x4"][1]["symmetries_discrete"]
    assert info[11]["symmetries_continuous"] == found["cylinder"][1]["symmetries_continuous"]
    assert MI.model_info(models[3], symmetries=dict(orders=(3, 5), n_sweep=0)) == plain[3]      # keywords reach find_symmetries
    path = str(tmp_path / "models_info.json")
    MI.save_models_info(path, info)
    back = load_models_info(path)
    assert back == info
    assert [len(get_symmetry_transformations(back[k])) for k in (3, 8, 11)] == [4, 1, 630]


def test_a_mesh_is_sampled_on_its_surface():
    """a model with faces goes through icp.model_cloud: a 2 x 3 x 4 box of 8 vertices and 12 triangles has the three half
    turns.  The cloud is one mean per voxel of 0.01 diameter: a moved point (itself up to a voxel off the surface at an edge)
    lands within a voxel diagonal of the mean of the voxel it falls in, 0.01 (1 + sqrt 3) = 0.027 of the diameter, inside
    tol = 0.05; the nearest false candidate, the quarter turn about z, leaves a corner 0.5 = 0.093 of the diameter off."""
    from pyrapose_amd.utils.model_info import find_symmetries
    v = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.5, 1.5) for z in (-2.0, 2.0)]) + SN.OFFSET
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])
    with pytest.warns(UserWarning, match="below the sampled cloud's own residual bound"):
        find_symmetries({"pts": v, "faces": faces})           # the defaults: tol 0.01 under (1 + sqrt 3) * sample 0.02
    got = find_symmetries({"pts": v, "faces": faces}, tol=0.05, sample=0.01, return_residuals=True)
    print("sampled box", got.get("residuals_discrete"))
    found_R = [np.asarray(m).reshape(4, 4)[:3, :3] for m in got.get("symmetries_discrete", [])]
    flips = [SN.rot(a, math.pi) for a in np.eye(3)]
    assert len(found_R) == 3 and all(min(SN.angle_between(E, R) for E in flips) <= 3 * 0.05 for R in found_R)
