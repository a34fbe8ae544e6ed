"""Symmetry sets of BOP object models: the `symmetries_discrete` / `symmetries_continuous` entries of a dataset's
models_info.json (the file annotation_scripts/annotate_BOP.py:221-230 reads) turned into the list of rigid transformations
that BOP's symmetry-aware pose errors MSSD / MSPD minimise over (utils.pose_error.mssd / mspd, csrc/pose.hip).  Host numpy:
a set is built once per object.  BOP's definition (bop_toolkit_lib.misc.get_symmetry_transformations) restated -- parity with
bop_toolkit unpinned: no BOP toolkit was at hand to compare against."""
import json
import math

import numpy as np


def load_models_info(path):
    """A BOP models_info.json -> dict keyed by int object id; the values are the file's dicts ('diameter', optionally
    'symmetries_discrete' and 'symmetries_continuous', the extents)."""
    with open(path, "r") as f:
        return {int(k): v for k, v in json.load(f).items()}


def _rotation(angle, axis):
    """Rodrigues: the rotation by `angle` about the normalised `axis`"""
    k = np.asarray(axis, np.float64).reshape(3)
    n = np.linalg.norm(k)
    if not n > 0.0:
        raise ValueError("symmetry axis must not be zero")
    k = k / n
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(angle) * Kx + (1.0 - math.cos(angle)) * Kx.dot(Kx)


def get_symmetry_transformations(model_info, max_sym_disc_step=0.01):
    """The symmetry transformations of one object: list of {'R': 3x3 float64, 't': 3x1 float64}, the identity first.
    Discrete symmetries: the identity, then each entry of model_info['symmetries_discrete'] (16 numbers, a row-major 4x4).
    Continuous symmetries ({'axis': a, 'offset': o}): n = ceil(pi / max_sym_disc_step) rotations by 2 pi i / n about the
    axis through o (R, -R o + o; 315 at the default step).  Result: the discrete list when there is no continuous symmetry;
    otherwise for every discrete d in order, and for it every continuous c in order, (c.R d.R, c.R d.t + c.t)."""
    disc = [{"R": np.eye(3), "t": np.zeros((3, 1))}]
    for sym in model_info.get("symmetries_discrete", ()):
        M = np.asarray(sym, np.float64).reshape(4, 4)
        disc.append({"R": M[:3, :3].copy(), "t": M[:3, 3].reshape(3, 1).copy()})
    cont = []
    for sym in model_info.get("symmetries_continuous", ()):
        axis = np.asarray(sym["axis"], np.float64).reshape(3)
        offset = np.asarray(sym["offset"], np.float64).reshape(3, 1)
        n = int(math.ceil(math.pi / max_sym_disc_step))
        for i in range(n):
            R = _rotation(2.0 * math.pi * i / n, axis)  # i = 0: exactly the identity
            cont.append({"R": R, "t": -R.dot(offset) + offset})
    if not cont:
        return disc
    return [{"R": c["R"].dot(d["R"]), "t": c["R"].dot(d["t"]) + c["t"]} for d in disc for c in cont]


def stack_symmetries(syms):
    """A list from get_symmetry_transformations -> (S_R [n_sym,3,3], S_t [n_sym,3]) contiguous float64, the form the ops take.
    None or an empty list: the single identity.  An (S_R, S_t) pair is checked and passed through."""
    if syms is None or (isinstance(syms, (list, tuple)) and len(syms) == 0):
        return np.eye(3)[None].copy(), np.zeros((1, 3))
    if isinstance(syms, tuple) and len(syms) == 2 and not isinstance(syms[0], dict):
        S_R, S_t = np.asarray(syms[0], np.float64), np.asarray(syms[1], np.float64)
        if S_R.ndim != 3 or S_R.shape[1:] != (3, 3) or S_R.shape[0] < 1 or S_t.size != 3 * S_R.shape[0]:
            raise ValueError("symmetries: need S_R [n_sym,3,3] and S_t [n_sym,3] with n_sym >= 1")
        return np.ascontiguousarray(S_R), np.ascontiguousarray(S_t.reshape(-1, 3))
    S_R = np.ascontiguousarray(np.stack([np.asarray(s["R"], np.float64).reshape(3, 3) for s in syms]))
    S_t = np.ascontiguousarray(np.stack([np.asarray(s["t"], np.float64).reshape(3) for s in syms]))
    return S_R, S_t
