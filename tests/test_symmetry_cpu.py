"""CPU (no GPU): the symmetry sets of utils/symmetry.py (BOP's get_symmetry_transformations restated) and the numpy
restatement of MSSD / MSPD (tests/pose_sym_np.py) against the two formulas in the matrix form bop_toolkit writes them in."""
import json
import math

import numpy as np
import pytest

from tests import pose_sym_np as SN

HALF_TURN_Z = [-1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
CASES = [  # (model_info, step, expected count)
    ({"diameter": 100.0}, 0.01, 1),
    ({"diameter": 100.0, "symmetries_discrete": [HALF_TURN_Z]}, 0.01, 2),
    ({"diameter": 100.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, 0.01, 315),
    ({"diameter": 100.0, "symmetries_discrete": [[1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, -1.0, 0, 0, 0, 0, 1.0]],
      "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, 0.01, 630),
    ({"diameter": 100.0, "symmetries_continuous": [{"axis": [1, 2, -0.5], "offset": [3.0, -4.0, 5.0]}]}, 0.5, 7),
]


@pytest.mark.parametrize("info,step,count", CASES)
def test_count_identity_first_and_rigid(info, step, count):
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations, stack_symmetries
    syms = get_symmetry_transformations(info, step)
    n_disc = len(info.get("symmetries_discrete", ()))
    n_cont = int(math.ceil(math.pi / step)) if "symmetries_continuous" in info else 0
    assert len(syms) == count == (1 + n_disc) * max(1, n_cont)
    assert np.array_equal(syms[0]["R"], np.eye(3)) and np.array_equal(syms[0]["t"], np.zeros((3, 1)))
    for s in syms:
        assert s["R"].shape == (3, 3) and s["t"].shape == (3, 1) and s["R"].dtype == s["t"].dtype == np.float64
        assert np.abs(s["R"].T @ s["R"] - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(s["R"]) - 1.0) <= 1e-12
    S_R, S_t = stack_symmetries(syms)
    assert S_R.shape == (count, 3, 3) and S_t.shape == (count, 3) and S_R.dtype == S_t.dtype == np.float64
    assert S_R.flags.c_contiguous and S_t.flags.c_contiguous
    assert np.array_equal(S_R[-1], syms[-1]["R"]) and np.array_equal(S_t[-1], syms[-1]["t"].reshape(3))


def test_default_step_and_stack_of_nothing():
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations, stack_symmetries
    assert len(get_symmetry_transformations(CASES[2][0])) == 315
    for nothing in (None, []):
        S_R, S_t = stack_symmetries(nothing)
        assert np.array_equal(S_R, np.eye(3)[None]) and np.array_equal(S_t, np.zeros((1, 3)))
    pair = SN.random_symmetries(np.random.default_rng(0), 4)
    S_R, S_t = stack_symmetries(pair)
    assert np.array_equal(S_R, pair[0]) and np.array_equal(S_t, pair[1])
    with pytest.raises(ValueError):
        stack_symmetries((pair[0], pair[1][:3]))


def test_continuous_symmetry_keeps_its_offset_point_fixed():
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations
    info = CASES[4][0]
    o = np.array(info["symmetries_continuous"][0]["offset"]).reshape(3, 1)
    a = np.array(info["symmetries_continuous"][0]["axis"], np.float64)
    syms = get_symmetry_transformations(info, 0.5)
    for i, s in enumerate(syms):
        assert np.abs(s["R"] @ o + s["t"] - o).max() <= 1e-12
        # a rotation by 2 pi i / 7 about the normalised axis: the axis is kept, the trace gives the angle
        assert np.abs(s["R"] @ a - a).max() <= 1e-12
        assert abs(np.trace(s["R"]) - (1.0 + 2.0 * math.cos(2.0 * math.pi * i / 7))) <= 1e-12


def test_discrete_half_turn_maps_an_off_centre_cube_onto_itself():
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations
    c = np.array([10.0, -20.0, 5.0])
    corners = c + np.array([[x, y, z] for x in (-7.0, 7.0) for y in (-7.0, 7.0) for z in (-7.0, 7.0)])
    R = np.diag([-1.0, -1.0, 1.0])                      # half-turn about the z direction through c: p -> R (p - c) + c
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, c - R @ c
    syms = get_symmetry_transformations({"diameter": 1.0, "symmetries_discrete": [M.reshape(-1).tolist()]})
    assert len(syms) == 2
    moved = corners @ syms[1]["R"].T + syms[1]["t"].reshape(3)
    as_set = lambda p: sorted(tuple(v) for v in np.round(p, 9).tolist())
    assert as_set(moved) == as_set(corners) and not np.allclose(moved, corners)


def test_combination_order_discrete_outer_continuous_inner():
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations
    info = dict(CASES[3][0], symmetries_continuous=[{"axis": [0, 0, 1], "offset": [1.0, 2.0, 3.0]}])
    syms = get_symmetry_transformations(info, 0.5)
    cont = get_symmetry_transformations({"symmetries_continuous": info["symmetries_continuous"]}, 0.5)
    d = np.array(info["symmetries_discrete"][0]).reshape(4, 4)
    assert len(syms) == 14 and len(cont) == 7
    for i in range(7):
        assert np.array_equal(syms[i]["R"], cont[i]["R"]) and np.allclose(syms[i]["t"], cont[i]["t"], atol=1e-15)
        np.testing.assert_allclose(syms[7 + i]["R"], cont[i]["R"] @ d[:3, :3], atol=1e-15)
        np.testing.assert_allclose(syms[7 + i]["t"], cont[i]["R"] @ d[:3, 3:] + cont[i]["t"], atol=1e-15)


def test_load_models_info_round_trip(tmp_path):
    from pyrapose_amd.utils.symmetry import get_symmetry_transformations, load_models_info
    info = {"1": {"diameter": 142.5, "min_x": -50.0, "size_x": 100.0},
            "5": {"diameter": 80.25, "symmetries_discrete": [HALF_TURN_Z]},
            "30": {"diameter": 63.5, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}
    path = tmp_path / "models_info.json"
    path.write_text(json.dumps(info))
    got = load_models_info(str(path))
    assert sorted(got) == [1, 5, 30] and all(isinstance(k, int) for k in got)
    assert got == {int(k): v for k, v in info.items()}
    assert [len(get_symmetry_transformations(got[k])) for k in (1, 5, 30)] == [1, 2, 315]


@pytest.mark.parametrize("n_sym", [1, 2, 9])
def test_restatement_agrees_with_the_blas_form(n_sym):
    rng = np.random.default_rng(100 + n_sym)
    pts, R_est, t_est, R_gt, t_gt = SN.scene(rng, 3, 500)
    S_R, S_t = SN.random_symmetries(rng, n_sym)
    syms = [{"R": S_R[s], "t": S_t[s].reshape(3, 1)} for s in range(n_sym)]
    e3, s3 = SN.mssd_np(pts, S_R, S_t, R_est, t_est, R_gt, t_gt)
    e2, s2 = SN.mspd_np(pts, S_R, S_t, SN.K_LINEMOD, R_est, t_est, R_gt, t_gt)
    assert e3.dtype == e2.dtype == np.float64 and s3.dtype == s2.dtype == np.int32
    for i in range(3):
        np.testing.assert_allclose(e3[i], SN.bop_blas_mssd(R_est[i], t_est[i], R_gt[i], t_gt[i], pts, syms), rtol=1e-12)
        np.testing.assert_allclose(e2[i], SN.bop_blas_mspd(R_est[i], t_est[i], R_gt[i], t_gt[i], SN.K_LINEMOD, pts, syms), rtol=1e-12)
    # the estimates are a few degrees off the ground truth, every other symmetry is a random pose: the identity wins
    assert s3.tolist() == [0, 0, 0] and s2.tolist() == [0, 0, 0] and (e3 > 1.0).all() and (e2 > 0.5).all()
