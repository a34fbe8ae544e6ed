"""Geometry of a triangle mesh on the device (csrc/mesh.hip): face normals, surface area, volume and centroid, area-weighted
vertex normals with the vertex-to-face adjacency, and points drawn uniformly by area from the surface.  For the meshes users
bring themselves -- CAD exports with a few large triangles and no nx ny nz properties -- where a BOP scan's dense vertex set
cannot double as a point cloud:
  with_normals(model)      fills model['normals'], which render_rgbd_batch(shading='phong') asks for
  model_points(model, n)   replaces model['pts'] by n even surface samples, for the consumers that read the points as they are
                           (ADD / ADI / MSSD / MSPD, pts_diameter, farthest_points, sym_hausdorff)
Models are the dicts utils.ply_loader.load_ply returns ('pts' [n_v,3], 'faces' [n_f,3]); arrays or device tensors go in.
Nothing in the reference computes any of this (it reads normals from BOP's files and points from BOP's models) and neither
Open3D nor trimesh was at hand: the rules are this project's, restated in tests/mesh_np.py and unpinned.  Open3D's
compute_vertex_normals uses the same area weighting.  A face that names a vertex out of range counts as degenerate."""
import numpy as np
import torch

from .. import ops
from ..runtime import default_context
from ._host import to_device


def _mesh(model):
    """model dict -> (pts, faces) as they came, their shapes checked (no device is touched)"""
    if not isinstance(model, dict) or model.get("pts") is None or model.get("faces") is None:
        raise ValueError("a mesh is a dict with 'pts' [n_v,3] and 'faces' [n_f,3] (utils.ply_loader.load_ply)")
    pts, faces = model["pts"], model["faces"]
    for name, a in (("pts", pts), ("faces", faces)):
        shape = tuple(a.shape) if torch.is_tensor(a) else np.shape(a)
        if len(shape) != 2 or shape[1] != 3 or shape[0] < 1:
            raise ValueError("model[%r] must be n x 3 with n >= 1, got %s" % (name, shape))
    if not torch.is_tensor(faces):
        f = np.asarray(faces)
        if f.dtype.kind not in "iu" and not np.array_equal(f, np.floor(f)):
            raise ValueError("model['faces'] must hold integers")
    return pts, faces


def _geometry(model, ctx):
    """-> (ctx, pts cuda float64 [n_v,3], faces cuda int32 [n_f,3], ops.mesh_face_geometry's dict)"""
    pts, faces = _mesh(model)
    ctx = ctx or default_context()
    pts, faces = to_device(pts), to_device(faces, torch.int32)
    return ctx, pts, faces, ops.mesh_face_geometry(ctx, pts, faces)


def face_normals(model, unit=False, ctx=None):
    """(normal cuda float64 [n_f,3] = (p1 - p0) x (p2 - p0), area2 [n_f] = its length, twice the area); unit=True divides the
    normals by their lengths (a degenerate face keeps a zero normal)."""
    _, _, _, g = _geometry(model, ctx)
    if not unit:
        return g["normal"], g["area2"]
    l = g["area2"][:, None]
    return torch.where(l > 0, g["normal"] / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(g["normal"])), g["area2"]


def _totals(model, ctx):
    return _geometry(model, ctx)[3]["totals"].cpu().numpy()


def surface_area(model, ctx=None):
    """the mesh's area: float (half the device's sum of the cross products' lengths)"""
    return float(_totals(model, ctx)[0]) / 2.0


def volume(model, ctx=None):
    """the signed volume of a closed mesh: float, positive for outward winding (the device's sum of p0 . normal over 6)"""
    return float(_totals(model, ctx)[1]) / 6.0


def centroid(model, ctx=None):
    """the centroid of the surface, every face's centre weighted by its area: float64 [3]; ValueError for a mesh of no area"""
    t = _totals(model, ctx)
    if not t[0] > 0.0:
        raise ValueError("centroid: the mesh has no area")
    return t[2:5] / (3.0 * t[0])


def vertex_normals(model, outward=True, ctx=None):
    """cuda float64 [n_v,3]: per vertex the sum of its faces' unnormalised normals (area weighting), in ascending face index,
    over its length; zero for a vertex no face of any area touches.  outward: negated for a mesh wound inward."""
    ctx, pts, faces, g = _geometry(model, ctx)
    return ops.mesh_vertex_normals(ctx, int(pts.shape[0]), faces, g, outward)[0]


def adjacency(model, ctx=None):
    """(adj_offsets cuda int32 [n_v+1], adj_faces int32 [3 n_f]): vertex v belongs to the faces
    adj_faces[adj_offsets[v]:adj_offsets[v+1]], ascending, a face once per listing of v; -1 past adj_offsets[n_v]"""
    ctx, pts, faces, g = _geometry(model, ctx)
    return ops.mesh_vertex_normals(ctx, int(pts.shape[0]), faces, g, False)[1:]


def with_normals(model, outward=True, ctx=None):
    """a copy of the model with 'normals' (numpy float64 [n_v,3]) filled in from vertex_normals unless the model brings its own"""
    out = dict(model)
    if out.get("normals") is None:
        out["normals"] = vertex_normals(model, outward, ctx).cpu().numpy()
    return out


def sample_surface(model, n, seed=0, mode="random", normals=False, attrs=None, outward=True, ctx=None):
    """n points uniform by area: dict of cuda tensors 'points' float64 [n,3], 'face' int32 [n], 'bary' [n,3]; normals=True adds
    'normals' (each face's unit normal); attrs: a per-vertex table [n_v,k], k <= 8 (colours, UVs, vertex normals), blended
    like the points into 'attrs' [n,k] -- the caller normalises what has to stay of unit length.  mode 'random' | 'weyl' (a
    low-discrepancy choice of faces).  The same seed gives the same bits."""
    if mode not in ops.MESH_MODES:
        raise ValueError("sample_surface: mode %r, need random | weyl" % (mode,))
    ctx, pts, faces, g = _geometry(model, ctx)
    attr = None if attrs is None else to_device(attrs)
    want = ("points", "face", "bary") + (("normals",) if normals else ())
    out = ops.mesh_sample_surface(ctx, pts, faces, g, n, seed, mode, outward, attr, want)
    if attr is not None:
        out["attrs"] = out.pop("attr_out")
    return out


def sample_surface_even(model, n, oversample=4, seed=0, ctx=None):
    """n points spread evenly over the surface: cuda float64 [n,3].  oversample n Weyl samples, thinned to n by greedy
    farthest-point sampling (ops.farthest_points, rule 'min')."""
    n, k = int(n), int(oversample)
    if n < 1 or k < 1:
        raise ValueError("sample_surface_even: need n >= 1 and oversample >= 1, got %d and %d" % (n, k))
    ctx = ctx or default_context()
    cand = sample_surface(model, n * k, seed, "weyl", ctx=ctx)["points"]
    if k == 1:
        return cand
    index = ops.farthest_points(ctx, cand, [0, n * k], n, "min")
    return cand[index[0].long()]


def model_points(model, n, oversample=4, seed=0, ctx=None):
    """the model with 'pts' replaced by n even surface samples (numpy float64 [n,3]) and without the keys that went with the
    old vertices ('faces', 'normals', 'colors', 'texture_uv'): what the point-set consumers take"""
    out = {k: v for k, v in model.items() if k not in ("faces", "normals", "colors", "texture_uv")}
    out["pts"] = sample_surface_even(model, n, oversample, seed, ctx).cpu().numpy()
    return out
