"""GPU: the argument handling of the pose-tail wrappers in ops.py (pose_errors ... vote_cluster) and utils._host.to_device.
Every tensor argument may be a non-contiguous view (same outputs, bit for bit); a host tensor, a wrong dtype, a wrong trailing
dimension or a wrong leading count is a ValueError naming the wrapper and the argument, raised on the host before any launch.
Every bad case here is detectable from the tensors' metadata or (icp offsets) from a host copy: none reaches the library."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K4 = (572.4114, 573.57043, 325.2611, 242.04899)
BOX = np.array([[x, y, z] for x in (-40.0, 40.0) for y in (-30.0, 30.0) for z in (-55.0, 55.0)])


@pytest.fixture(scope="module")
def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def project(obj, R, t):
    cam = obj @ R.T + t
    return np.stack([K4[0] * cam[:, 0] / cam[:, 2] + K4[2], K4[1] * cam[:, 1] / cam[:, 2] + K4[3]], 1)


# ---- one smallest valid call per wrapper: name -> (call(ctx, args dict), args dict of cuda tensors in signature order,
#      the (argument, form) pairs that are no error because that dimension is free: it sets n / n_pts / N / P / h / w) ----

def _pose(with_K, with_sym, call):
    rng = np.random.default_rng(1)
    a = dict(pts=dev(rng.standard_normal((5, 3)) * 0.05))
    if with_sym:
        a.update(S_R=dev(np.stack([np.eye(3), np.diag([-1.0, -1.0, 1.0])])), S_t=dev(np.zeros((2, 3))))
    if with_K:
        a.update(K9=dev(np.tile(np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]]), (2, 1, 1))))
    R_gt = np.stack([rotation(rng), rotation(rng)])
    t_gt = rng.uniform(-0.1, 0.1, (2, 3)) + [0.0, 0.0, 0.8]
    a.update(R_est=dev(np.stack([rotation(rng), R_gt[1]])), t_est=dev(t_gt + 0.01), R_gt=dev(R_gt), t_gt=dev(t_gt))
    first = "K9" if with_K else "R_est"
    return call, a, {("pts", "lead"), ("S_R", "lead"), (first, "lead")}


def _render():
    from pyrapose_amd import ops
    a = dict(verts=dev([[-50.0, -50.0, 0.0], [50.0, -50.0, 0.0], [0.0, 60.0, 0.0]]), faces=dev([[0, 1, 2]], torch.int32),
             R=dev(np.eye(3)[None]), t=dev([[0.0, 0.0, 500.0]]), K4=dev([[100.0, 100.0, 8.0, 8.0]]))
    return (lambda ctx, a: ops.render_depth(ctx, a["verts"], a["faces"], a["R"], a["t"], a["K4"], 16, 16),
            a, {("verts", "lead"), ("faces", "lead"), ("R", "lead")})


def _vsd():
    from pyrapose_amd import ops
    rng = np.random.default_rng(2)
    d = rng.uniform(400.0, 600.0, (3, 2, 8, 8)).astype(np.float32)
    a = dict(depth_test=dev(d[0, 0], torch.float32), depth_est=dev(d[1], torch.float32), depth_gt=dev(d[2], torch.float32),
             K4=dev(np.tile(K4, (2, 1))))
    # depth_est sets n, h and w; a depth_test with one more row or column is named, with a leading 1 added it is not [n,h,w]
    return (lambda ctx, a: ops.vsd(ctx, a["depth_test"], a["depth_est"], a["depth_gt"], a["K4"], 15.0, 20.0),
            a, {("depth_est", "lead"), ("depth_est", "trail")})


def _pnp_problem():
    rng = np.random.default_rng(3)
    R, t = rotation(rng), np.array([10.0, -20.0, 700.0])
    obj = np.tile(BOX, (2, 1))
    img = project(obj, R, t) + rng.normal(0.0, 0.3, (16, 2))
    return obj, img, R, t


def _pnp_ransac():
    from pyrapose_amd import ops
    obj, img, _R, _t = _pnp_problem()
    a = dict(offsets=dev([0, 16], torch.int32), obj=dev(obj), img=dev(img), K4=dev([K4]))
    # offsets [P+1] set P: one more entry and K4 [P,4] is named; obj sets N
    return (lambda ctx, a: ops.pnp_ransac(ctx, a["offsets"], a["obj"], a["img"], a["K4"], 20, 5.0, 1, 8),
            a, {("offsets", "lead"), ("obj", "lead")})


def _cloud_from_depth():
    from pyrapose_amd import ops
    rng = np.random.default_rng(4)
    depth = rng.uniform(400.0, 600.0, (8, 8)).astype(np.float32)
    depth[2, 3] = 0.0
    mask = (rng.uniform(size=(4, 4)) < 0.7).astype(np.uint8)
    a = dict(depth=dev(depth, torch.float32), mask=dev(mask, torch.uint8), row_idx=dev(np.arange(8) // 2, torch.int32),
             col_idx=dev(np.arange(8) // 2, torch.int32))
    return (lambda ctx, a: ops.cloud_from_depth(ctx, a["depth"], *K4, 1.0, a["mask"], a["row_idx"], a["col_idx"]),
            a, {("depth", "lead"), ("depth", "trail"), ("mask", "lead"), ("mask", "trail")})


def _clouds():
    rng = np.random.default_rng(5)
    src = rng.uniform(-30.0, 30.0, (40, 3)) + [0.0, 0.0, 600.0]
    nrm = rng.standard_normal((40, 3))
    return src, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def _voxel():
    from pyrapose_amd import ops
    pts, nrm = _clouds()
    return (lambda ctx, a: ops.voxel_down_sample(ctx, a["pts"], 20.0, a["normals"]), dict(pts=dev(pts), normals=dev(nrm)), {("pts", "lead")})


def _normals():
    from pyrapose_amd import ops
    return (lambda ctx, a: ops.estimate_normals(ctx, a["pts"], 25.0, 10, return_neighbors=True), dict(pts=dev(_clouds()[0])), {("pts", "lead")})


def _icp(mode):
    from pyrapose_amd import ops
    tgt, nrm = _clouds()
    src = tgt + [0.5, -0.3, 0.8]
    a = dict(src_offsets=dev([0, 40], torch.int32), tgt_offsets=dev([0, 40], torch.int32), src=dev(src), tgt=dev(tgt), init=dev(np.eye(4)[None]))
    if mode == "point_to_plane":
        a.update(tgt_normals=dev(nrm))
    # src / tgt set Ns / Nt: with one more point the offsets no longer end at the count, which names the offsets
    return (lambda ctx, a: ops.icp(ctx, a["src_offsets"], a["tgt_offsets"], a["src"], a["tgt"], a["init"], 10.0, 5, 1e-6, 1e-6, mode,
                                   a.get("tgt_normals")), a, {("src", "lead"), ("tgt", "lead")})


def _vote_stats():
    from pyrapose_amd import ops
    _obj, img, _R, _t = _pnp_problem()
    a = dict(offsets=dev([0, 16], torch.int32), img=dev(img), vote_weight=dev([0.9, 0.6]), inlier_mask=dev(np.ones(16), torch.uint8))
    # img sets N: one more point and points_per_vote no longer divides it (no argument to name)
    return (lambda ctx, a: ops.vote_stats(ctx, a["offsets"], a["img"], 8, a["vote_weight"], a["inlier_mask"]),
            a, {("img", "lead")})


def _refine():
    from pyrapose_amd import ops
    obj, img, R, t = _pnp_problem()
    a = dict(offsets=dev([0, 16], torch.int32), obj=dev(obj), img=dev(img), wgt=dev(np.tile([1.0, 0.0, 1.0], (16, 1))), K4=dev([K4]),
             R_init=dev(R[None]), t_init=dev((t + [1.0, -1.0, 5.0])[None]))
    return (lambda ctx, a: ops.pnp_refine_weighted(ctx, a["offsets"], a["obj"], a["img"], a["wgt"], a["K4"], a["R_init"], a["t_init"]),
            a, {("obj", "lead")})


def _vote_cluster(ctx):
    from pyrapose_amd import ops
    rng = np.random.default_rng(6)
    centre = np.where(np.arange(32)[:, None] < 20, 100.0, 400.0) + rng.normal(0.0, 2.0, (32, 16))
    b3 = (centre + np.tile([-30.0, -30.0, 30.0, 30.0], 4)).astype(np.float32)[None]
    sc = rng.uniform(0.6, 0.9, (1, 32, 1)).astype(np.float32)
    a = dict(boxes3D=dev(b3, torch.float32), scores=dev(sc, torch.float32))
    a["idx"], a["cnt"] = ops.score_threshold_compact(ctx, a["scores"], 0.5)
    # scores sets B, N and C, idx sets cap
    return (lambda ctx, a: ops.vote_cluster(ctx, a["boxes3D"], a["scores"], a["idx"], a["cnt"], 0.5, 10, 4),
            a, {("scores", "lead"), ("scores", "trail"), ("idx", "trail")})


def make_case(name, ctx):
    from pyrapose_amd import ops
    if name == "pose_errors":
        return _pose(False, False, lambda ctx, a: (ops.pose_errors(ctx, *a.values()), ops.pose_errors(ctx, *a.values(), symmetric=True)))
    if name == "pose_reproj":
        return _pose(True, False, lambda ctx, a: ops.pose_reproj(ctx, *a.values()))
    if name == "pose_mssd":
        return _pose(False, True, lambda ctx, a: ops.pose_mssd(ctx, *a.values()))
    if name == "pose_mspd":
        return _pose(True, True, lambda ctx, a: ops.pose_mspd(ctx, *a.values()))
    if name.startswith("icp"):
        return _icp(name[4:])
    if name == "vote_cluster":
        return _vote_cluster(ctx)
    return {"render_depth": _render, "vsd": _vsd, "pnp_ransac": _pnp_ransac, "cloud_from_depth": _cloud_from_depth,
            "voxel_down_sample": _voxel, "estimate_normals": _normals, "vote_stats": _vote_stats, "pnp_refine_weighted": _refine}[name]()


CASES = ["pose_errors", "pose_reproj", "pose_mssd", "pose_mspd", "render_depth", "vsd", "pnp_ransac", "cloud_from_depth",
         "voxel_down_sample", "estimate_normals", "icp_point_to_point", "icp_point_to_plane", "vote_stats", "pnp_refine_weighted",
         "vote_cluster"]


def flat(out):
    """the tensors of a wrapper's result (a tensor, a tuple or a dict, None where an output is switched off) in a fixed order"""
    if out is None:
        return []
    if torch.is_tensor(out):
        return [out]
    return [t for o in ([out[k] for k in sorted(out)] if isinstance(out, dict) else out) for t in flat(o)]


def strided(t):
    """the same values as a view that is not contiguous: every second element of a buffer twice as long in the last dimension"""
    buf = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    view = buf[..., ::2]
    view.copy_(t)
    assert torch.equal(view, t) and (t.numel() == 1 or not view.is_contiguous())
    return view


def widen(t, dim):
    """one more entry along `dim` (a copy of the first)"""
    return torch.cat([t, t.narrow(dim, 0, 1)], dim).contiguous()


OTHER = {torch.float64: torch.float32, torch.float32: torch.float64, torch.int32: torch.int64, torch.uint8: torch.int32}
FORMS = {"host": lambda t: t.cpu(), "dtype": lambda t: t.to(OTHER[t.dtype]), "trail": lambda t: widen(t, t.dim() - 1),
         "lead": lambda t: widen(t, 0)}


# ---- a. to_device ----

def test_to_device():
    from pyrapose_amd.utils._host import to_device
    view = np.broadcast_to(np.arange(9.0).reshape(3, 3), (4, 3, 3))
    assert not view.flags.writeable
    lst = [[np.float32(1.5), np.float32(2.5)], [np.float32(3.5), np.float32(4.5)]]
    other = torch.arange(6, dtype=torch.int32, device="cuda").reshape(2, 3)
    for a, want in ((view, view), (lst, np.array(lst, np.float64)), (other, other.cpu().numpy().astype(np.float64)),
                    (other.t(), other.cpu().numpy().T.astype(np.float64)), (np.arange(12.0).reshape(3, 4).T, np.arange(12.0).reshape(3, 4).T)):
        for dtype in (torch.float64, torch.float32):
            got = to_device(a, dtype)
            assert got.is_cuda and got.dtype == dtype and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want)
    assert to_device(np.arange(6), torch.int32, shape=(-1, 3)).shape == (2, 3)
    assert to_device(np.array([True, False]), torch.uint8).tolist() == [1, 0]
    assert to_device(np.array([3, 65535], np.uint16), torch.float32).tolist() == [3.0, 65535.0]  # uint16 depth, host conversion
    ready = torch.arange(6.0, dtype=torch.float64, device="cuda").reshape(2, 3)
    assert to_device(ready).data_ptr() == ready.data_ptr()
    assert to_device(ready, shape=(3, 2)).data_ptr() == ready.data_ptr()
    assert to_device(ready.t()).data_ptr() != ready.data_ptr()


# ---- b. non-contiguous views of every tensor argument ----

@pytest.mark.parametrize("name", CASES)
def test_strided_arguments_give_equal_outputs(ctx, name):
    call, args, _free = make_case(name, ctx)
    want = flat(call(ctx, args))
    assert want and all(t.is_cuda for t in want)
    got = flat(call(ctx, {k: strided(t) for k, t in args.items()}))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w)
    again = flat(call(ctx, args))
    assert all(torch.equal(g, w) for g, w in zip(again, want))


# ---- c. one argument at a time made wrong ----

@pytest.mark.parametrize("name", CASES)
def test_each_wrong_argument_is_a_named_value_error(ctx, name):
    call, args, free = make_case(name, ctx)
    wrapper = name[:3] if name.startswith("icp") else name
    tried = 0
    for arg, t in args.items():
        for form, make in FORMS.items():
            if (arg, form) in free or (form == "trail" and t.dim() == 1):  # of one dimension, the trailing is the leading one
                continue
            with pytest.raises(ValueError) as e:
                call(ctx, dict(args, **{arg: make(t)}))
            msg = str(e.value)
            assert msg.startswith(wrapper + ":") and arg in msg, (arg, form, msg)
            tried += 1
    assert tried >= 2 * len(args)
    torch.cuda.synchronize()


def test_missing_and_non_tensor_arguments(ctx):
    from pyrapose_amd import ops
    call, args, _ = make_case("icp_point_to_plane", ctx)
    with pytest.raises(ValueError, match="icp: tgt_normals"):  # point_to_plane needs them
        call(ctx, {k: v for k, v in args.items() if k != "tgt_normals"})
    call, args, _ = make_case("cloud_from_depth", ctx)
    with pytest.raises(ValueError, match="cloud_from_depth: row_idx"):  # a mask needs its index maps
        call(ctx, dict(args, row_idx=None))
    call, args, _ = make_case("pose_errors", ctx)
    with pytest.raises(ValueError, match="pose_errors: R_gt"):
        call(ctx, dict(args, R_gt=args["R_gt"].cpu().numpy()))
    empty = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="voxel_down_sample: pts"):
        ops.voxel_down_sample(ctx, empty, 5.0)
    with pytest.raises(ValueError, match="estimate_normals: pts"):
        ops.estimate_normals(ctx, empty, 5.0, 10)


# ---- d. icp offsets, through the shared offsets check ----

@pytest.mark.parametrize("which", ["src_offsets", "tgt_offsets"])
@pytest.mark.parametrize("bad", [[1, 40], [0, 39], [0, 41], [0, 41, 40]])
def test_icp_offsets(ctx, which, bad):
    call, args, _ = make_case("icp_point_to_point", ctx)
    with pytest.raises(ValueError, match="icp: " + which):
        call(ctx, dict(args, **{which: dev(bad, torch.int32)}))
