"""GPU: csrc/mesh.hip bit for bit against its numpy restatement (tests/mesh_np.py) at the smallest shapes where each kernel can
go wrong -- W = ops.MESH_THREADS faces per chunk of the float sums, S = ops.MESH_SCAN_CHUNK quantised areas per workgroup of
the integer scan --, then the host path: with_normals into the phong renderer, model_points into pts_diameter."""
import math

import numpy as np
import pytest
import torch

from tests import mesh_np as R

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def same_bits(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype == np.float64:
        return np.array_equal(got.view(np.int64), want.view(np.int64))
    return np.array_equal(got, want)


def device_geometry(p, f):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    ctx = default_context()
    P, F = dev(p, np.float64), dev(f, np.int32)
    return ctx, P, F, ops.mesh_face_geometry(ctx, P, F)


def check_geometry(p, f, status=None):
    _, _, _, g = device_geometry(p, f)
    want = R.face_geometry(p, f)
    for k in ("normal", "area2", "totals"):
        assert same_bits(g[k], want[k]), (k, len(f))
    assert int(g["status"].cpu()[0]) == want["status"]
    if status is not None:
        assert want["status"] == status
    return want


def sizes():
    from pyrapose_amd import ops
    return ops.MESH_THREADS, ops.MESH_SCAN_CHUNK


# ---- face geometry ----------------------------------------------------------------------------------------------------------

def test_face_geometry_at_the_chunk_edges():
    W, S = sizes()
    assert (W, S) == (R.THREADS, R.SCAN_CHUNK)
    rng = np.random.default_rng(0)
    for n_f in (1, 2, W - 1, W, W + 1, 2 * W + 1, 3 * S + 1):
        p, f = R.soup(n_f, rng)                 # points near (1000, 1000, 1000): a tail lane read as a zero point would show
        want = check_geometry(p, f, status=0)
        assert want["totals"][0] > 0 and abs(want["totals"][2] / (3.0 * want["totals"][0]) - 1000.0) < 2.0
        p, f = R.strip(n_f, rng)                # shared vertices, alternating winding
        check_geometry(p, f, status=0)


def test_a_planted_largest_face_is_found_wherever_it_sits():
    W, _ = sizes()
    n_f = 2 * W + 1
    for at in (0, W - 1, W, n_f - 1):
        scale = np.ones(n_f)
        scale[at] = 64.0
        p, f = R.soup(n_f, np.random.default_rng(at), scale=scale)
        want = check_geometry(p, f, status=0)
        assert int(np.argmax(want["area2"])) == at and want["totals"][5] == want["area2"][at]


def test_degenerate_and_out_of_range_faces():
    W, _ = sizes()
    rng = np.random.default_rng(1)
    p, f = R.strip(W + 7, rng)
    f[3] = [5, 5, 6]                            # degenerate: zero area, in range
    check_geometry(p, f, status=0)
    f[W] = [0, len(p), 1]                       # one past the last vertex, in the second chunk
    f[W + 1] = [-1, 2, 3]
    f[9] = [2 ** 31 - 1, 0, 1]
    want = check_geometry(p, f, status=1)
    assert not want["normal"][[3, 9, W, W + 1]].any()
    check_geometry(p, np.array([[0, 0, 1], [2, 2, 2]], np.int32), status=2)
    check_geometry(p, np.array([[0, len(p), 1]], np.int32), status=3)
    check_geometry(np.zeros((1, 3)), np.zeros((1, 3), np.int32), status=2)


# ---- vertex normals and adjacency ---------------------------------------------------------------------------------------------

def valence_mesh(inward=False):
    """hubs of valence 1, 2, 63, 64, 65 and 2 W + 1, an isolated vertex, a face that lists a hub twice and one with a bad index"""
    W, _ = sizes()
    fans = [R.fan(v, offset=(3.0 * k, 1.0, 0.5), lift=0.25 + 0.1 * k) for k, v in enumerate((1, 2, 63, 64, 65, 2 * W + 1))]
    p, f = R.join(fans + [(np.array([[50.0, 50.0, 50.0]]), np.zeros((0, 3), np.int32))])
    hubs = np.cumsum([0] + [len(fp) for fp, _ in fans])[:-1]
    f = np.concatenate([f[:40], [[hubs[3], hubs[3], hubs[3] + 5]], f[40:], [[hubs[2], len(p), 1]], [[hubs[5], hubs[5] + 2, hubs[5]]]]).astype(np.int32)
    return p, (f[:, ::-1].copy() if inward else f), hubs


def device_vertex_normals(p, f, outward):
    from pyrapose_amd import ops
    ctx, P, F, g = device_geometry(p, f)
    return ops.mesh_vertex_normals(ctx, len(p), F, g, outward)


@pytest.mark.parametrize("inward", [False, True])
def test_vertex_normals_and_adjacency_over_the_valences(inward):
    W, _ = sizes()
    p, f, hubs = valence_mesh(inward)
    geom = R.face_geometry(p, f)
    for outward in (False, True):
        want = R.vertex_normals(f, len(p), geom["normal"], geom["totals"], outward)
        got = device_vertex_normals(p, f, outward)
        again = device_vertex_normals(p, f, outward)
        for k, name in enumerate(("vnormal", "adj_offsets", "adj_faces")):
            assert same_bits(got[k], want[k]), (name, outward)
            assert same_bits(again[k], got[k].cpu().numpy()), (name, "run to run")
    off, adj = want[1], want[2]
    val = np.diff(off)
    assert val[hubs].tolist() == [1, 2, 63, 64 + 2, 65, 2 * W + 1 + 2] and val[-1] == 0 and not want[0][-1].any()
    hub = adj[off[hubs[5]]:off[hubs[5] + 1]]
    assert (np.diff(hub) >= 0).all() and (np.diff(hub) == 0).sum() == 1          # ascending; the last face lists the hub twice
    assert off[-1] == 3 * (len(f) - 1) and (adj[off[-1]:] == -1).all()           # the face with a bad index is in no list


def test_both_windings_agree_under_outward():
    p, f = R.sphere(7, 9)
    out = device_vertex_normals(p, f, True)[0].cpu().numpy()
    flipped = device_vertex_normals(p, f[:, ::-1].copy(), True)[0].cpu().numpy()
    raw = device_vertex_normals(p, f[:, ::-1].copy(), False)[0].cpu().numpy()
    assert same_bits(raw, -flipped) and np.abs(out - flipped).max() < 1e-14 and ((out * p).sum(axis=1) > 0.9).all()


# ---- sampling -----------------------------------------------------------------------------------------------------------------

KEYS = ("points", "face", "bary", "normals", "attr_out")


def check_samples(p, f, n, seed, mode, attr=None, outward=True, want_keys=("points", "face", "bary", "normals")):
    from pyrapose_amd import ops
    ctx, P, F, g = device_geometry(p, f)
    geom = R.face_geometry(p, f)
    got = ops.mesh_sample_surface(ctx, P, F, g, n, seed, mode, outward, None if attr is None else dev(attr, np.float64), want_keys)
    want = R.sample_surface(p, f, geom, n, seed, mode, outward, attr)
    keys = tuple(want_keys) + (("attr_out",) if attr is not None else ())
    assert sorted(got) == sorted(keys)
    for k in keys:
        assert same_bits(got[k], want[k]), (k, n, seed, mode)
    return want, geom


def test_sample_counts_modes_and_seeds():
    W, _ = sizes()
    p, f = R.soup(37, np.random.default_rng(2), offset=(5.0, -3.0, 2.0))
    for n in (1, W - 1, W + 1, 2 * W + 1):
        for mode in ("random", "weyl"):
            for seed in (0, 2 ** 63 + 12345):
                check_samples(p, f, n, seed, mode)


def test_sample_zero_area_faces_and_tiny_faces():
    W, _ = sizes()
    rng = np.random.default_rng(3)
    p, f = R.soup(9, rng, offset=(0.0, 0.0, 0.0))
    for at in (0, 8):
        g = f.copy()
        g[at] = [g[at, 0], g[at, 0], g[at, 1]]
        want, _ = check_samples(p, g, 2 * W + 1, 5, "random")
        assert at not in want["face"] and len(np.unique(want["face"])) == 8
    none = np.repeat(f[:, :1], 3, axis=1)
    for mode in ("random", "weyl"):
        want, _ = check_samples(p, none, W + 1, 1, mode, attr=np.ones((len(p), 3)))
        assert (want["face"] == -1).all()
    scale = np.ones(40)
    scale[[0, 7, 39]] = 2.0 ** -23                 # areas 2^-46 of the others: their q is 0
    p, f = R.soup(40, rng, offset=(0.0, 0.0, 0.0), scale=scale)
    want, geom = check_samples(p, f, 2 * W + 1, 9, "weyl")
    q = R.quantise(f, len(p), geom["area2"], geom["totals"][5])
    assert (geom["area2"] > 0).all() and (q[[0, 7, 39]] == 0).all() and (q > 0).sum() == 37
    assert geom["area2"].max() / geom["area2"].min() > 2.0 ** 45 and not np.isin(want["face"], [0, 7, 39]).any()
    bad = f.copy()
    bad[5] = [0, len(p), 1]
    want, _ = check_samples(p, bad, W + 1, 9, "random")
    assert 5 not in want["face"]


def test_sample_at_the_scan_chunk_edges():
    W, S = sizes()
    rng = np.random.default_rng(4)
    for n_f in (S - 1, S, S + 1, 2 * S + 1):
        p, f = R.strip(n_f, rng, offset=(0.0, 0.0, 0.0))
        want, _ = check_samples(p, f, 2 * W + 1, n_f, "random")
        assert want["face"].max() >= n_f - 64 and want["face"].min() < 64   # both ends, so every chunk, are reached
    want, _ = check_samples(p, f, 2 * W + 1, 3, "weyl", outward=False)


def test_sample_attributes_and_skipped_outputs():
    W, _ = sizes()
    rng = np.random.default_rng(5)
    p, f = R.sphere(5, 6)
    inward = f[:, ::-1].copy()
    for n_attr in (1, 3, 8):
        check_samples(p, inward, W + 1, 7, "random", attr=rng.normal(size=(len(p), n_attr)))
    attr = rng.normal(size=(len(p), 2))
    for skip in range(4):
        keys = tuple(k for i, k in enumerate(KEYS[:4]) if i != skip)
        check_samples(p, f, W + 1, 8, "weyl", attr=attr, want_keys=keys)
        check_samples(p, f, W + 1, 8, "weyl", want_keys=(KEYS[skip],))
    check_samples(p, f, W + 1, 8, "random", attr=attr, want_keys=())


def test_entry_point_refusals_launch_nothing():
    from pyrapose_amd import _lib, ops
    from pyrapose_amd.runtime import default_context
    ctx = default_context()
    p, f = R.cube()
    _, P, F, g = device_geometry(p, f)
    L, h, big = _lib.lib, ctx.handle, R.MAX_ELEMS
    ptr = ops._ptr
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.zeros(64, dtype=torch.float64, device="cuda")
    geo = lambda n_v, n_f, nbytes, pts=P: L.pp_mesh_face_geometry_f64(h, n_v, n_f, ptr(pts), ptr(F), ptr(ws), nbytes, ptr(out), ptr(out), ptr(out), ptr(out))
    assert geo(0, 12, 4096) == geo(8, 0, 4096) == geo(big + 1, 12, 4096) == geo(8, big + 1, 4096) == -2      # PP_ERR_SHAPE
    assert geo(8, 12, 63) == geo(8, 12, 4096, None) == -1                                                     # PP_ERR_ARG
    vn = lambda n_v, n_f, nbytes, tot=g["totals"]: L.pp_mesh_vertex_normals_f64(h, n_v, n_f, ptr(F), ptr(g["normal"]), ptr(tot), 1, ptr(ws), nbytes,
                                                                                ptr(out), ptr(out), ptr(out))
    assert vn(0, 12, 4096) == vn(8, big + 1, 4096) == -2 and vn(8, 12, 2 * 256 + 143) == vn(8, 12, 4096, None) == -1
    sm = lambda n, mode=0, n_attr=0, attr_out=None, nbytes=4096, pts=P: L.pp_mesh_sample_surface_f64(
        h, 8, 12, ptr(pts), ptr(F), ptr(g["normal"]), ptr(g["area2"]), ptr(g["totals"]), n, 0, mode, 1, n_attr, None, ptr(ws), nbytes, ptr(out), None, None,
        None, ptr(attr_out))
    assert sm(0) == sm(2 ** 24 + 1) == sm(4, 0, 9, out) == sm(4, 0, 0, out) == -2
    assert sm(4, 2) == sm(4, 0, 2, out) == sm(4, nbytes=256 + 15) == sm(4, pts=None) == -1
    torch.cuda.synchronize()
    assert not out.any().item()                                                                                 # nothing was written


# ---- the host path --------------------------------------------------------------------------------------------------------------

def test_with_normals_feeds_the_phong_renderer():
    from pyrapose_amd.utils import mesh
    from pyrapose_amd.utils.renderer import render_rgbd_batch
    p, f = R.cube(side=100.0, origin=(-50.0, -50.0, -50.0))
    model = dict(pts=p, faces=f)
    K = np.array([[100.0, 0.0, 32.0], [0.0, 100.0, 24.0], [0.0, 0.0, 1.0]])
    c, s = math.cos(0.6), math.sin(0.6)
    Rm = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]).dot(np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]))[None]
    t = np.array([[0.0, 0.0, 400.0]])
    with pytest.raises(ValueError, match="normals"):
        render_rgbd_batch(model, (64, 48), K, Rm, t, shading="phong", outputs=("rgb_f32",))
    filled = mesh.with_normals(model)
    g = R.face_geometry(p, f)
    want_normals = R.vertex_normals(f, 8, g["normal"], g["totals"])[0]
    assert same_bits(filled["normals"], want_normals) and "normals" not in model
    got = render_rgbd_batch(filled, (64, 48), K, Rm, t, shading="phong", outputs=("rgb_f32",))["rgb_f32"]
    want = render_rgbd_batch(dict(model, normals=want_normals), (64, 48), K, Rm, t, shading="phong", outputs=("rgb_f32",))["rgb_f32"]
    assert got.shape == (1, 48, 64, 3) and torch.equal(got, want) and (got.amax(dim=3) > 0).float().mean().item() > 0.1


def test_model_points_give_a_cube_its_diameter():
    from pyrapose_amd.utils import mesh
    from pyrapose_amd.utils.model_info import pts_diameter
    p, f = R.cube()
    model = dict(pts=p, faces=f, colors=np.zeros((8, 3)))
    even = mesh.model_points(model, 2000)
    assert even["pts"].shape == (2000, 3) and "faces" not in even and "colors" not in even and len(model["pts"]) == 8
    # a blend of coordinates 1 is (a + b) + c: 1 to the 2 ulp of the weights' sum and the blend's own roundings, not exactly 1
    assert even["pts"].min() >= 0.0 and even["pts"].max() <= 1.0 + 4.0 * np.finfo(np.float64).eps
    d = pts_diameter(even)
    assert abs(d - math.sqrt(3.0)) <= 0.02 * math.sqrt(3.0)
    cand = R.sample_surface(p, f, R.face_geometry(p, f), 8000, seed=0, mode="weyl")["points"]
    assert same_bits(mesh.sample_surface(model, 8000, 0, "weyl")["points"], cand)
    assert abs(mesh.surface_area(model) - 6.0) == 0.0 and mesh.volume(model) == 1.0 and np.array_equal(mesh.centroid(model), [0.5] * 3)
    off, adj = mesh.adjacency(model)
    assert same_bits(off, R.adjacency(f, 8)[0]) and same_bits(adj, R.adjacency(f, 8)[1])
    unit, area2 = mesh.face_normals(model, unit=True)
    assert same_bits(area2, np.ones(12)) and np.abs(unit.cpu().numpy()).sum(axis=1).tolist() == [1.0] * 12
