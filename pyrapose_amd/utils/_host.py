"""Host arrays on their way to the device entry points: the conversions the pose-tail modules of utils/ share (pose_error,
renderer, pnp, un_pnp_utils, icp, pose_decode).  Shape errors are ValueError."""
import numpy as np
import torch

_NUMPY = {torch.float64: np.float64, torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}


def to_device(a, dtype=torch.float64, shape=None):
    """numpy array, list or tensor -> contiguous cuda tensor of `dtype` (reshaped to `shape` when given).  Host values are
    converted on the host; a tensor already on the device with that dtype and layout comes back as it is."""
    if not torch.is_tensor(a):
        a = np.asarray(a, _NUMPY[dtype], order="C")
        a = torch.from_numpy(a if a.flags.writeable else a.copy())  # broadcast views are read-only
    a = a.to(device="cuda", dtype=dtype)
    return (a if shape is None else a.reshape(shape)).contiguous()


def per_pose(a, n, shape):
    """one array of `shape` shared by all n poses, or one per pose -> float64 [n, *shape] (a read-only view when shared)"""
    a = np.asarray(a, np.float64)
    if a.shape == tuple(shape):
        return np.broadcast_to(a, (n,) + tuple(shape))
    if a.shape != (n,) + tuple(shape):
        raise ValueError("need %s or %s, got %s" % (tuple(shape), (n,) + tuple(shape), a.shape))
    return a


def k4(K, n=None):
    """camera matrix -> (fx, fy, cx, cy): of one 3x3 as a tuple; with n, of a 3x3 or an [n,3,3] as float64 [n,4]"""
    if n is None:
        K = np.asarray(K, np.float64)
        if K.shape != (3, 3):
            raise ValueError("K must be 3x3, got %s" % (K.shape,))
        return K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    K = per_pose(K, n, (3, 3))
    return np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], axis=1)


def pack_ragged(arrays):
    """a list of P arrays (or of P tensors) [n_i, ...] -> (offsets int32 [P+1] from 0 to sum n_i, their concatenation)"""
    offsets = np.zeros(len(arrays) + 1, np.int32)
    offsets[1:] = np.cumsum([len(a) for a in arrays])
    return offsets, (torch.cat(arrays) if torch.is_tensor(arrays[0]) else np.concatenate(arrays))
