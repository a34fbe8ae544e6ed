"""CPU: the host logic of utils.model_info.find_symmetries / symmetry_residuals driven by the numpy restatement of the device
score (tests/model_sym_np.py) -- the shapes of tests/test_gpu_model_sym.py at coarser spacing: the groups found, closure, the
merge of a and -a, the continuous rule, BOP's format, the models_info.json round trip and symmetric_ids.  No device here: the
scorer and the diameter are passed in; model_info itself is looked at through stand-ins for the two device ops."""
import math

import numpy as np
import pytest

from tests import model_sym_np as SN

CPU = dict(_scorer=SN.scorer, _diameter=SN.diameter_of)


def find(pts, **kw):
    from pyrapose_amd.utils.model_info import find_symmetries
    return find_symmetries(pts, **{**CPU, "n_sweep": 36, **kw})


def test_restatement_tie_rules_and_tails():
    """integer coordinates: duplicated source points tie the maximum (lowest i), duplicated targets tie a minimum (lowest j)"""
    src = np.array([[0, 0, 0], [5, 0, 0], [1, 0, 0], [5, 0, 0]], np.float64)
    tgt = np.array([[1, 0, 0], [2, 0, 0], [2, 0, 0], [0, 0, 0]], np.float64)
    d2, arg = SN.sym_hausdorff_np(src, tgt, np.eye(3)[None], np.zeros((1, 3)))
    assert d2.dtype == np.float64 and arg.dtype == np.int32 and d2.tolist() == [9.0] and arg.tolist() == [[1, 1]]
    d2, arg = SN.sym_hausdorff_np(src, None, np.eye(3)[None], np.array([[1.0, 0.0, 0.0]]))
    assert d2.tolist() == [1.0] and arg.tolist() == [[1, 1]]      # 6 is 1 from the first 5; 0 + 1 and 1 + 1 = 2 tie at 1 later
    blocked = SN.sym_hausdorff_np(src, tgt, np.eye(3)[None], np.zeros((1, 3)), block=3)
    assert blocked[0].tolist() == [9.0] and blocked[1].tolist() == [[1, 1]]


@pytest.mark.parametrize("rotated", [False, True])
def test_square_box_has_seven_elements(rotated):
    """2 x 2 x 3: 4-fold about z, 2-fold about x, y; the diagonals by the sweep or by closure.  Rotated: no axis is a coordinate
    axis and the x / y eigen-plane has no preferred direction -- the sweep and its refinement find the in-plane axes."""
    Q = SN.fixed_rotation() if rotated else np.eye(3)
    pts = SN.box_grid(2.0, 2.0, 3.0, 0.5).dot(Q.T) + SN.OFFSET
    SN.check_result(find(pts), pts, SN.dihedral(4), 0.01, Q)


def test_closure_alone_completes_the_group():
    """without the sweep, the 4-fold and 2-fold about z and the 2-folds about x and y are what the candidate axes give: their
    products supply the quarter turn back and both diagonals"""
    pts = SN.box_grid(2.0, 2.0, 3.0, 0.5) + SN.OFFSET
    SN.check_result(find(pts, n_sweep=0), pts, SN.dihedral(4), 0.01)
    # closure capped: nothing past max_group elements is composed, what is there still passes
    few = find(pts, n_sweep=0, max_group=4)
    assert len(few["symmetries_discrete"]) == 4


def test_plain_box_has_three_and_a_or_minus_a_is_one_axis():
    pts = SN.box_grid(2.0, 3.0, 4.0, 0.5) + SN.OFFSET
    flips = [SN.rot(a, math.pi) for a in np.eye(3)]
    SN.check_result(find(pts), pts, flips, 0.01)
    # -x, x again and a scaled z from the caller add nothing
    SN.check_result(find(pts, axes=[(-1.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 0.0, -3.0)]), pts, flips, 0.01)
    from pyrapose_amd.utils.model_info import _merge_axes
    merged = _merge_axes([(2, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -3, 0), (1, 0, 0), (0, 0, 1)])
    assert np.array_equal(merged, np.eye(3))               # the first of each line stays, normalised
    with pytest.raises(ValueError):
        _merge_axes([(0, 0, 0)])


def test_hexagonal_prism_has_eleven():
    pts = SN.hex_prism(3, [-1.0, 0.0, 1.0]) + SN.OFFSET
    SN.check_result(find(pts), pts, SN.dihedral(6), 0.01)


def test_an_axis_off_the_candidates_comes_from_the_caller():
    """a tetrahedron's covariance is isotropic (the stated limit): rotated off the coordinate axes nothing is found; one 3-fold
    and one 2-fold axis from the caller generate all 11 non-identity elements by closure"""
    Q = SN.fixed_rotation()
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
    edge = [v[a] + (v[b] - v[a]) * m / 4.0 for a in range(4) for b in range(a + 1, 4) for m in range(1, 4)]
    pts = np.concatenate([v, edge]).dot(Q.T) + SN.OFFSET
    group = [SN.rot(v[k], s * 2 * math.pi / 3) for k in range(4) for s in (1, 2)] + [SN.rot(a, math.pi) for a in np.eye(3)]
    got = find(pts, axes=[Q.dot(v[0]), Q.dot((0.0, 0.0, 1.0))])
    SN.check_result(got, pts, group, 0.01, Q, count=11)


def test_cylinder_is_one_continuous_axis_and_one_flip():
    """90 points per ring: an arbitrary turn leaves every point within half a spacing of another, 0.0156 of the diameter (the
    180-point ring of the device test reaches 0.0048), so tol = 0.02 here"""
    per_ring = 90
    for Q in (np.eye(3), SN.fixed_rotation()):
        pts = SN.cylinder(per_ring, [-0.5, 0.0, 0.5]).dot(Q.T) + SN.OFFSET
        got = find(pts, tol=0.02, return_residuals=True)
        SN.check_result(got, pts, SN.dihedral(per_ring)[per_ring - 1:], 0.02, Q, continuous_axis=np.array([0.0, 0.0, 1.0]), count=1)
        assert len(got["residuals_continuous"]) == 1 and 0.0 < got["residuals_continuous"][0] <= 0.02
        assert len(got["residuals_discrete"]) == 1 and 0.0 <= got["residuals_discrete"][0] <= 0.02
    # an axis 1e-3 rad off z (what an eigenvector of a resampled cloud is) passes as well: still one continuous axis, the first
    pts = SN.cylinder(per_ring, [-0.5, 0.0, 0.5]) + SN.OFFSET
    got = find(pts, tol=0.02, axes=[(1e-3, 0.0, 1.0)])
    assert len(got["symmetries_continuous"]) == 1 and got["symmetries_continuous"][0]["axis"][0] > 0.0
    assert len(got["symmetries_discrete"]) == 1
    # without probes no axis is called continuous: the finite orders that divide 90 remain, closed into D_30 (orders 2, 3, 5, 6)
    pts = SN.cylinder(per_ring, [-0.5, 0.0, 0.5]) + SN.OFFSET
    assert "symmetries_continuous" not in find(pts, n_probe=0, tol=0.001)


def test_asymmetric_model_gives_an_empty_dict():
    assert find(SN.cut_box(0.5) + SN.OFFSET) == {}
    assert find(np.zeros((3, 3))) == {}                    # no extent: nothing to ask


def test_symmetry_residuals_scores_declared_symmetries():
    from pyrapose_amd.utils.model_info import symmetry_residuals
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations
    pts = SN.box_grid(2.0, 3.0, 4.0, 0.5) + SN.OFFSET
    c = pts.mean(axis=0)
    good, bad = SN.rot((0, 0, 1), math.pi), SN.rot((0, 0, 1), math.pi / 2)
    as4x4 = lambda R: np.block([[R, (c - R.dot(c))[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]]).reshape(-1).tolist()
    syms = get_symmetry_transformations({"symmetries_discrete": [as4x4(good), as4x4(bad)]})
    r = symmetry_residuals(pts, syms, _scorer=SN.scorer)
    print("declared symmetries of the 2 x 3 x 4 box: residuals", r)
    assert r.shape == (3,) and r.dtype == np.float64
    assert r[0] == 0.0 and r[1] < 1e-14 and r[2] >= 0.5 - 1e-12    # the quarter turn swaps the 2 and 3 sides: a corner lands 0.5 off
    # the (S_R, S_t) form; a target: a source that lacks a point still lands on the full set, the full set misses a lacking one
    pair = (np.stack([good]), np.stack([c - good.dot(c)]))
    assert symmetry_residuals(pts, pair, _scorer=SN.scorer)[0] == r[1]
    assert symmetry_residuals(pts[:-1], pair, target=pts, _scorer=SN.scorer)[0] < 1e-14
    assert symmetry_residuals(pts, pair, target=pts[1:], _scorer=SN.scorer)[0] >= 0.5 - 1e-12   # one grid spacing, rounded
    # both directions count: a third of a turn forward and back about z differ when the target is not the source
    third = SN.rot((0, 0, 1), 2 * math.pi / 3)
    tri = np.array([[1.0, 0.0, 0.0], [-0.5, math.sqrt(0.75), 0.0], [-0.5, -math.sqrt(0.75), 0.0], [0.0, 0.0, 1.0]])
    tgt = np.concatenate([tri, [tri[0] * 2.0]])
    src = np.concatenate([tri, [third.T.dot(tri[0] * 2.0)]])   # lands on the extra target under `third`, far off under its inverse
    S = (np.stack([third]), np.zeros((1, 3)))
    fwd = math.sqrt(SN.sym_hausdorff_np(src, tgt, *S)[0][0])
    back = symmetry_residuals(src, S, target=tgt, _scorer=SN.scorer)[0]    # the extra point lands at radius 2 over a corner at 1
    assert fwd < 1e-14 and abs(back - 1.0) < 1e-12


def test_format_round_trip_and_symmetric_ids(tmp_path):
    from pyrapose_amd.utils import model_info as MI
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations, load_models_info
    box = SN.box_grid(2.0, 2.0, 3.0, 0.5) + SN.OFFSET
    cyl = SN.cylinder(90, [-0.5, 0.0, 0.5]) + SN.OFFSET
    info = {1: dict(diameter=SN.diameter_of(box), **find(box)),
            2: dict(diameter=SN.diameter_of(cyl), **find(cyl, tol=0.02)),
            5: dict(diameter=1.0, **find(SN.cut_box(0.5)))}
    for M in info[1]["symmetries_discrete"]:
        assert isinstance(M, list) and len(M) == 16 and all(type(v) is float for v in M) and M[12:] == [0.0, 0.0, 0.0, 1.0]
    entry = info[2]["symmetries_continuous"][0]
    assert sorted(entry) == ["axis", "offset"] and all(len(entry[k]) == 3 and all(type(v) is float for v in entry[k]) for k in entry)
    assert sorted(info[5]) == ["diameter"]
    assert MI.symmetric_ids(info) == [1, 2] and MI.symmetric_ids({"7": info[2], "3": info[5], 4: info[1]}) == [4, 7]
    path = str(tmp_path / "models_info.json")
    MI.save_models_info(path, info)
    back = load_models_info(path)
    assert back == info
    syms = get_symmetry_transformations(back[1])
    assert len(syms) == 8 and np.array_equal(syms[0]["R"], np.eye(3))
    assert np.array_equal(syms[3]["R"], np.asarray(info[1]["symmetries_discrete"][2]).reshape(4, 4)[:3, :3])
    assert len(get_symmetry_transformations(back[2])) == 2 * 315
    assert get_symmetry_transformations(back[5])[0]["t"].shape == (3, 1) and len(get_symmetry_transformations(back[5])) == 1


def test_model_info_keeps_its_keys_and_merges_what_is_found(monkeypatch):
    """model_info(model) without `symmetries` returns exactly today's keys; with it, the found keys are merged.  The two device
    ops are stood in for by numpy here (the device path: tests/test_gpu_model_sym.py)."""
    import torch
    from pyrapose_amd.utils import model_info as MI
    monkeypatch.setattr(MI, "to_device", lambda a, *args, **kw: torch.as_tensor(np.asarray(a)))
    monkeypatch.setattr(MI, "default_context", lambda: None)
    monkeypatch.setattr(MI.ops, "pts_diameter", lambda ctx, p: (torch.tensor([SN.diameter_of(p.numpy()) ** 2]), None))
    monkeypatch.setattr(MI.ops, "sym_hausdorff", lambda ctx, s, t, R, T: tuple(
        torch.from_numpy(a) for a in SN.sym_hausdorff_np(s.numpy(), None if t is None else t.numpy(), R.numpy(), T.numpy())))
    pts = SN.box_grid(2.0, 3.0, 4.0, 1.0) + SN.OFFSET
    plain = MI.model_info(pts)
    assert sorted(plain) == ["diameter", "min_x", "min_y", "min_z", "size_x", "size_y", "size_z"]
    assert MI.model_info(pts, symmetries=None) == plain and MI.models_info({"4": pts}) == {4: plain}
    with_sym = MI.model_info(pts, symmetries=dict(n_sweep=12))
    assert sorted(with_sym) == sorted(list(plain) + ["symmetries_discrete"]) and len(with_sym["symmetries_discrete"]) == 3
    assert {k: with_sym[k] for k in plain} == plain
    both = MI.models_info({4: pts, 9: SN.cut_box(1.0)}, symmetries=dict(n_sweep=12))
    assert MI.symmetric_ids(both) == [4] and sorted(both[9]) == sorted(plain)
