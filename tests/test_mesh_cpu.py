"""CPU (no GPU): the numpy restatement of csrc/mesh.hip (tests/mesh_np.py) against closed forms -- cube, inward cube,
octahedron, tetrahedron, degenerate and out-of-range faces --, its sampler's statistics on a mesh of known area shares, the
margins the device tests rely on, the C ABI of the three entry points and the refusals that need no device.  The device side is
tests/test_gpu_mesh.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import mesh_np as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 3   # of the sampling statistics below: fixed after the restatement alone was seen to meet them (a condition on the inputs)


def geometry(p, f):
    g = R.face_geometry(p, f)
    t = g["totals"]
    return g, t[0] / 2.0, t[1] / 6.0, t[2:5] / (3.0 * t[0])


def test_unit_cube():
    p, f = R.cube()
    g, area, vol, cen = geometry(p, f)
    assert g["status"] == 0 and area == 6.0 and vol == 1.0 and np.array_equal(cen, [0.5, 0.5, 0.5])
    assert (g["area2"] == 1.0).all() and g["totals"][5] == 1.0 and not g["totals"][6:].any()
    vn, off, adj = R.vertex_normals(f, 8, g["normal"], g["totals"])
    assert np.allclose(np.linalg.norm(vn, axis=1), 1.0, rtol=0, atol=1e-15)
    assert (np.sign(vn) == np.sign(p - 0.5)).all()            # every corner's normal points into its own octant
    assert off[-1] == 36 and (np.diff(off) >= 3).all() and all((np.diff(adj[off[v]:off[v + 1]]) > 0).all() for v in range(8))


def test_inward_cube_is_flipped_by_outward():
    p, f = R.cube()
    pi, fi = R.cube(inward=True)
    g, gi = R.face_geometry(p, f), R.face_geometry(pi, fi)
    assert gi["totals"][1] / 6.0 == -1.0 and gi["totals"][0] == 12.0
    out = R.vertex_normals(f, 8, g["normal"], g["totals"])[0]
    raw = R.vertex_normals(fi, 8, gi["normal"], gi["totals"], outward=False)[0]
    fixed = R.vertex_normals(fi, 8, gi["normal"], gi["totals"], outward=True)[0]
    assert np.array_equal(fixed, -raw) and np.allclose(fixed, out, rtol=0, atol=1e-15)
    s = R.sample_surface(pi, fi, gi, 50, seed=1, outward=True)
    centre_to_point = s["points"] - 0.5
    assert ((s["normals"] * centre_to_point).sum(axis=1) > 0).all()
    assert np.array_equal(R.sample_surface(pi, fi, gi, 50, seed=1, outward=False)["normals"], -s["normals"])


def test_regular_octahedron_vertex_normals_are_the_axes():
    p, f = R.octahedron()
    g, area, vol, cen = geometry(p, f)
    assert vol == 4.0 / 3.0 and abs(area - 4.0 * math.sqrt(3.0)) < 1e-14 and np.abs(cen).max() < 1e-16
    vn, off, _ = R.vertex_normals(f, 6, g["normal"], g["totals"])
    assert np.array_equal(vn, p) and np.array_equal(np.diff(off), [4] * 6)


def test_tetrahedron():
    p, f = R.tetrahedron()
    g, area, vol, cen = geometry(p, f)
    assert vol == 1.0 / 6.0 and abs(area - (1.5 + math.sqrt(3.0) / 2.0)) < 1e-15
    assert np.array_equal(g["normal"][3], [1.0, 1.0, 1.0]) and np.array_equal(g["normal"][0], [0.0, 0.0, -1.0])
    vn = R.vertex_normals(f, 4, g["normal"], g["totals"])[0]
    assert np.allclose(vn[0], -np.ones(3) / math.sqrt(3.0), rtol=0, atol=1e-15)


def test_degenerate_and_out_of_range_faces_among_good_ones():
    p, f = R.cube()
    clean = R.face_geometry(p, f)
    f2 = np.concatenate([f[:5], [[0, 0, 3]], f[5:9], [[1, 8, 2]], [[-1, 2, 3]], f[9:]]).astype(np.int32)
    g = R.face_geometry(p, f2)
    assert g["status"] == 1 and g["totals"][0] == clean["totals"][0] and g["totals"][1] == clean["totals"][1]
    for k in (5, 10, 11):
        assert not g["normal"][k].any() and g["area2"][k] == 0.0
    vn, off, adj = R.vertex_normals(f2, 8, g["normal"], g["totals"])
    assert np.array_equal(vn, R.vertex_normals(f, 8, clean["normal"], clean["totals"])[0])
    assert off[-1] == 36 + 3 and (adj[off[-1]:] == -1).all() and len(adj) == 3 * len(f2)
    assert adj[off[0]:off[1]].tolist().count(5) == 2          # the degenerate face lists vertex 0 twice
    assert 10 not in adj and 11 not in adj                    # a face with a bad index is in no list
    s = R.sample_surface(p, f2, g, 500, seed=2)
    assert not np.isin(s["face"], [5, 10, 11]).any()
    none = R.face_geometry(p, np.array([[0, 0, 1], [2, 2, 2]], np.int32))
    assert none["status"] == 2
    z = R.sample_surface(p, [[0, 0, 1], [2, 2, 2]], none, 7, attr=np.ones((8, 2)))
    assert (z["face"] == -1).all() and not any(z[k].any() for k in ("points", "bary", "normals", "attr_out"))
    assert R.face_geometry(p, np.array([[0, 9, 1]], np.int32))["status"] == 3


def test_sums_run_in_the_stated_order():
    rng = np.random.default_rng(0)
    v = rng.uniform(0.0, 1.0, 2 * R.THREADS + 5)
    first = v[:R.THREADS].copy()
    s = R.THREADS // 2
    while s:
        first[:s] += first[s:2 * s]
        s >>= 1
    pad = np.zeros(R.THREADS)
    pad[:5] = v[2 * R.THREADS:]
    assert R.tree_sum(v[:R.THREADS]) == first[0] and R.tree_sum(v[:1]) == v[0]
    assert R.tree_sum(v) == (first[0] + R.tree_sum(v[R.THREADS:2 * R.THREADS])) + R.tree_sum(pad)


def share_deviations(mode, n=20000):
    p, f = R.ratio_mesh()
    g = R.face_geometry(p, f)
    s = R.sample_surface(p, f, g, n, seed=SEED, mode=mode, attr=p[:, :2])
    share = g["area2"] / g["area2"].sum()
    counts = np.bincount(s["face"], minlength=4)
    sigma = np.sqrt(n * share * (1.0 - share))
    return p, f, g, s, np.abs(counts - n * share), sigma


@pytest.mark.parametrize("mode", ["random", "weyl"])
def test_samples_follow_the_area_shares_and_lie_on_their_faces(mode):
    p, f, g, s, dev, sigma = share_deviations(mode)
    assert np.array_equal(g["area2"], [2.0, 4.0, 10.0, 100.0])
    assert (dev <= 5.0 * sigma).all(), (dev, sigma)
    a, b, c = s["bary"].T
    assert (np.abs(((a + b) + c) - 1.0) <= 2.0 * np.finfo(np.float64).eps).all() and s["bary"].min() >= 0.0
    unit = g["normal"][s["face"]] / g["area2"][s["face"]][:, None]
    dist = ((s["points"] - p[f[s["face"], 0]]) * unit).sum(axis=1)
    assert np.abs(dist).max() <= 1e-12
    assert np.array_equal(s["normals"], unit) and np.array_equal(s["attr_out"], s["points"][:, :2])
    again = R.sample_surface(p, f, g, 20000, seed=SEED, mode=mode)
    assert all(np.array_equal(again[k], s[k]) for k in ("points", "face", "bary"))
    other = R.sample_surface(p, f, g, 20000, seed=SEED + 1, mode=mode)
    assert not np.array_equal(other["points"], s["points"])


def test_weyl_shares_are_no_worse_than_random_ones():
    assert share_deviations("weyl")[4].max() <= share_deviations("random")[4].max()


def test_quantisation_rule():
    area2 = np.array([3.0, 3.0 * 2.0 ** -38, 3.0 * 2.0 ** -41, 0.0, 1.5])
    faces = np.array([[0, 1, 2]] * 4 + [[0, 1, 3]])
    q = R.quantise(faces, 3, area2, 3.0)
    assert q.tolist() == [3 << 38, 3, 0, 0, 0] and 2 ** 39 <= int(q[0]) < 2 ** 40   # the last face names vertex 3 of 3
    assert not R.quantise(faces, 4, area2, 0.0).any()
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF and int(R._mix(np.array([0], np.uint64))[0]) == R.splitmix64(0)


def test_even_samples_of_a_cube_span_its_diagonal():
    """the margin tests/test_gpu_mesh.py relies on: 8000 Weyl samples of the unit cube thinned to 2000 by farthest points hold
    a pair within 2 % of sqrt(3) apart -- here on the restatement alone, with the thinning restated by the min-distance rule"""
    p, f = R.cube()
    cand = R.sample_surface(p, f, R.face_geometry(p, f), 8000, seed=0, mode="weyl")["points"]
    chosen = [int(np.argmax((cand * cand).sum(axis=1)))]
    score = np.full(len(cand), np.inf)
    for _ in range(1999):
        d = cand - cand[chosen[-1]]
        score = np.minimum(score, (d * d).sum(axis=1))
        chosen.append(int(np.argmax(score)))
    pts = cand[chosen]
    best = max(float(np.sqrt(((pts - q) ** 2).sum(axis=1).max())) for q in pts)
    assert best <= math.sqrt(3.0) and math.sqrt(3.0) - best <= 0.02 * math.sqrt(3.0)   # (1.4 % at this seed)


def test_entry_points_declared_and_exported():
    from pyrapose_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "pyrapose_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    kind = {C.c_void_p: "p", C.c_int: "i", C.c_size_t: "z", C.c_ulonglong: "z"}   # (one 64-bit unsigned class to ctypes)
    for name, n_arg in (("pp_mesh_face_geometry_f64", 11), ("pp_mesh_vertex_normals_f64", 12), ("pp_mesh_sample_surface_f64", 21)):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.EXPORTS and hasattr(_lib.lib, name)
        fn = getattr(_lib.lib, name)
        decl = re.search(r"int %s\((.*?)\);" % name, code, flags=re.S).group(1).split(",")
        assert len(fn.argtypes) == len(decl) == n_arg and fn.restype == C.c_int
        kinds = ["p" if "*" in a else "z" if "size_t" in a or "unsigned long long" in a else "i" for a in decl]
        assert [kind[t] for t in fn.argtypes] == kinds
        ws = name.replace("_f64", "_workspace_bytes")
        assert re.search(r"size_t %s\(" % ws, code) and ws in _lib.EXPORTS and getattr(_lib.lib, ws).restype == C.c_size_t
    k = open(os.path.join(ROOT, "pyrapose_amd", "csrc", "mesh.hip")).read()
    consts = {n: eval(v) for n, v in re.findall(r"#define MESH_([A-Z_]+) (\d+|\(1 << \d+\))\s", k)}
    assert consts["THREADS"] == ops.MESH_THREADS == R.THREADS and consts["SCAN_CHUNK"] == ops.MESH_SCAN_CHUNK == R.SCAN_CHUNK
    assert consts["MAX_ELEMS"] == ops.MESH_MAX_ELEMS == R.MAX_ELEMS and consts["MAX_SAMPLES"] == ops.MESH_MAX_SAMPLES == R.MAX_SAMPLES
    assert consts["MAX_ATTR"] == ops.MESH_MAX_ATTR == R.MAX_ATTR and consts["Q_BITS"] == R.Q_BITS and ops.MESH_MODES == R.MODES
    mk = open(os.path.join(ROOT, "pyrapose_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bmesh\.hip\b", mk, flags=re.M) and "EXTRA_mesh := -ffp-contract=off" in mk
    # host-side refusals need no device: a NULL context first, as everywhere; the workspace sizes are plain host arithmetic
    L = _lib.lib
    assert L.pp_mesh_face_geometry_f64(None, 1, 1, None, None, None, 0, None, None, None, None) == -4
    assert L.pp_mesh_vertex_normals_f64(None, 1, 1, None, None, None, 1, None, 0, None, None, None) == -4
    assert L.pp_mesh_sample_surface_f64(None, 1, 1, None, None, None, None, None, 1, 0, 0, 1, 0, None, None, 0, None, None, None, None, None) == -4
    big = R.MAX_ELEMS
    assert L.pp_mesh_face_geometry_workspace_bytes(1) == 64 and L.pp_mesh_face_geometry_workspace_bytes(257) == 128
    assert L.pp_mesh_face_geometry_workspace_bytes(0) == 0 and L.pp_mesh_face_geometry_workspace_bytes(big + 1) == 0
    assert L.pp_mesh_face_geometry_workspace_bytes(big) == big // 256 * 64
    assert L.pp_mesh_vertex_normals_workspace_bytes(3, 1) == 2 * 256 + 12 and L.pp_mesh_vertex_normals_workspace_bytes(65, 10) == 2 * 512 + 120
    assert L.pp_mesh_vertex_normals_workspace_bytes(big + 1, 1) == 0 and L.pp_mesh_vertex_normals_workspace_bytes(1, 0) == 0
    assert L.pp_mesh_sample_surface_workspace_bytes(1) == 256 + 16 and L.pp_mesh_sample_surface_workspace_bytes(1025) == 8448 + 24
    assert L.pp_mesh_sample_surface_workspace_bytes(big + 1) == 0


def test_the_kernels_keep_their_contract():
    """mesh.hip: no float atomics, no host synchronisation, every loop a counted `for`"""
    k = open(os.path.join(ROOT, "pyrapose_amd", "csrc", "mesh.hip")).read()
    code = re.sub(r"//[^\n]*", "", k)
    assert not re.search(r"\bwhile\s*\(", code) and "goto" not in code
    for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "hipMalloc", "hipEventSynchronize"):
        assert word not in code
    atomics = re.findall(r"atomic\w+\(&(\w+)\[", code)
    assert sorted(set(atomics)) == ["counts", "cursor"] and len(re.findall(r"\batomic\w+\(", code)) == len(atomics) == 2
    assert re.search(r"int\* __restrict__ counts", code) and re.search(r"int\* __restrict__ cursor", code)   # integers both


def test_argument_errors_need_no_device():
    import torch
    from pyrapose_amd import ops
    from pyrapose_amd.utils import mesh
    host_p, host_f = torch.zeros((4, 3), dtype=torch.float64), torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(ValueError, match="pts"):
        ops.mesh_face_geometry(None, host_p, host_f)
    with pytest.raises(ValueError, match="pts"):
        ops.mesh_face_geometry(None, np.zeros((4, 3)), host_f)
    with pytest.raises(ValueError, match="faces"):
        ops.mesh_vertex_normals(None, 4, host_f, {})
    for kw, word in ((dict(mode="sobol"), "mode"), (dict(n_samples=0), "n_samples"), (dict(n_samples=2 ** 24 + 1), "n_samples"),
                     (dict(n_samples=2.5), "n_samples"), (dict(want=("points", "colour")), "want")):
        args = dict(n_samples=4)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            ops.mesh_sample_surface(None, host_p, host_f, {}, **args)
    with pytest.raises(ValueError, match="pts"):
        ops.mesh_sample_surface(None, host_p, host_f, {}, 4)
    for bad in (None, {}, dict(pts=np.zeros((4, 3))), dict(pts=np.zeros((4, 2)), faces=np.zeros((1, 3), int)),
                dict(pts=np.zeros((4, 3)), faces=np.zeros((0, 3), int)), dict(pts=np.zeros((4, 3)), faces=np.full((1, 3), 0.5))):
        with pytest.raises(ValueError):
            mesh.vertex_normals(bad)
    with pytest.raises(ValueError, match="mode"):
        mesh.sample_surface(dict(pts=np.zeros((4, 3)), faces=np.zeros((1, 3), int)), 5, mode="grid")
    with pytest.raises(ValueError, match="oversample"):
        mesh.sample_surface_even(dict(pts=np.zeros((4, 3)), faces=np.zeros((1, 3), int)), 5, oversample=0)


def test_with_normals_leaves_given_normals_alone():
    from pyrapose_amd.utils import mesh
    p, f = R.cube()
    given = np.full((8, 3), 7.0)
    model = dict(pts=p, faces=f, normals=given, colors=np.zeros((8, 3)))
    out = mesh.with_normals(model)                            # (no device is touched: the normals are there)
    assert out is not model and out["normals"] is given and sorted(out) == sorted(model) and out["pts"] is p
