"""CPU: the host-array helpers the pose-tail modules of utils/ share (pyrapose_amd/utils/_host.py): k4, per_pose, pack_ragged.
to_device needs a device and is covered in tests/test_gpu_tail_args.py."""
import numpy as np
import pytest

from pyrapose_amd.utils._host import k4, pack_ragged, per_pose

K = np.array([[572.4, 0.0, 325.2], [0.0, 573.5, 242.0], [0.0, 0.0, 1.0]])


def test_k4_of_one_matrix_of_n_and_of_one_shared_by_n():
    assert k4(K) == (572.4, 573.5, 325.2, 242.0)
    assert k4(K.tolist()) == (572.4, 573.5, 325.2, 242.0)
    Ks = np.stack([K, 2.0 * K, 3.0 * K])
    got = k4(Ks, 3)
    assert got.dtype == np.float64 and got.shape == (3, 4)
    assert np.array_equal(got, np.outer([1.0, 2.0, 3.0], [572.4, 573.5, 325.2, 242.0]))
    shared = k4(K, 3)
    assert shared.dtype == np.float64 and np.array_equal(shared, np.tile([572.4, 573.5, 325.2, 242.0], (3, 1)))
    assert np.array_equal(k4(K.astype(np.float32), 2), np.tile(np.float32([572.4, 573.5, 325.2, 242.0]).astype(np.float64), (2, 1)))


@pytest.mark.parametrize("bad, n", [(K.reshape(9), None), (K[:2], None), (K[None], None), (np.stack([K, K]), None), (K.reshape(9), 3),
                                    (K[:2], 3), (np.stack([K, K]), 3), (K[None], 3), (np.zeros((3, 9)), 3), (np.zeros((3, 4, 4)), 3)])
def test_k4_of_a_wrong_shape_raises(bad, n):
    with pytest.raises(ValueError):
        k4(bad, n)


def test_per_pose_shared_and_one_each():
    a = np.arange(6).reshape(2, 3)
    got = per_pose(a, 4, (2, 3))
    assert got.dtype == np.float64 and got.shape == (4, 2, 3) and all(np.array_equal(row, a) for row in got)
    each = np.arange(24.0).reshape(4, 2, 3)
    assert np.array_equal(per_pose(each, 4, (2, 3)), each)
    assert np.array_equal(per_pose(a, 2, (3,)), a)  # n rows of shape (3,): one per pose
    for bad in (a.reshape(6), each[:3], each.reshape(4, 6)):
        with pytest.raises(ValueError):
            per_pose(bad, 4, (2, 3))


def test_pack_ragged_with_an_empty_middle_problem():
    rng = np.random.default_rng(0)
    arrays = [rng.standard_normal((3, 2)), np.zeros((0, 2)), rng.standard_normal((5, 2))]
    offsets, cat = pack_ragged(arrays)
    assert offsets.dtype == np.int32 and offsets.tolist() == [0, 3, 3, 8]
    assert cat.shape == (8, 2)
    for p, a in enumerate(arrays):
        assert np.array_equal(cat[offsets[p]:offsets[p + 1]], a)
    offsets, cat = pack_ragged([np.arange(4.0)])
    assert offsets.tolist() == [0, 4] and np.array_equal(cat, np.arange(4.0))
