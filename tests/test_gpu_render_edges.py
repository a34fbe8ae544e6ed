"""GPU: the three raster kernels of csrc/render.hip (depth, colour, textured colour -- one raster text, render_raster_tile.inc,
compiled three times) against the numpy restatement tests/render_rgb_np.py on the scenes of tests/render_cases.py, which reach
the raster phase's control-flow edges (tests/test_render_cases_cpu.py asserts that they do).  Every comparison is of all pixels
and bit for bit, depth as uint32 and triangle ids as int32: the image is a pure function of (triangle, pixel), and device and
restatement evaluate the same expressions in the same order.  Through ops.*: utils.renderer refuses the bad faces of scene I."""
import numpy as np
import pytest
import torch

from tests import render_cases as C

pytestmark = pytest.mark.gpu
SINGLE = sorted(n for n in C.SCENES if n != "G_scan_carry")


def dev(a, dt=torch.float64):
    return torch.as_tensor(np.array(a), dtype=dt).cuda()               # a copy: the scenes' arrays are read-only


def mesh_args(s, poses):
    poses = list(poses)
    K = s["K"]
    K4 = np.tile([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], (len(poses), 1))
    return dev(s["pts"]), dev(s["faces"], torch.int32), dev(s["R"][poses]), dev(s["t"][poses]), dev(K4), s["w"], s["h"]


def twice(call):
    """the op's outputs as numpy arrays, after a second run gave the same bytes"""
    a, b = call(), call()
    a, b = (({"depth": o} if torch.is_tensor(o) else o) for o in (a, b))
    a, b = ({k: v.cpu().numpy() for k, v in o.items()} for o in (a, b))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "%s differs between two runs" % k
    return a


def depth_pass(s, poses):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    return twice(lambda: ops.render_depth(default_context(), *mesh_args(s, poses), clip_near=s["near"], clip_far=s["far"]))["depth"]


def colour_pass(s, poses):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    return twice(lambda: ops.render_rgbd(default_context(), *mesh_args(s, poses), clip_near=s["near"], clip_far=s["far"], shading="flat",
                                         outputs=("depth", "tri_id")))


def textured_pass(s, poses):
    """flat shaded through a 2 x 2 texture: a colour output, so that the textured kernel is the one launched"""
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    rng = np.random.default_rng(106)
    uv, tex = dev(rng.uniform(size=(len(s["pts"]), 2))), dev(rng.integers(0, 256, size=(2, 2, 4)), torch.uint8)
    return twice(lambda: ops.render_rgbd_tex(default_context(), *mesh_args(s, poses), uv=uv, tex=tex, clip_near=s["near"], clip_far=s["far"],
                                             shading="flat", outputs=("rgb", "tri_id", "depth")))


def same_bits(name, pose, what, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, what, got.dtype, got.shape)
    g, w = (a.view(np.uint32 if a.dtype == np.float32 else np.int32) for a in (got, want))
    if not np.array_equal(g, w):
        rr, cc = np.nonzero(g != w)
        ids = C.restated(name, pose)[1]
        pytest.fail("%s pose %d, %s: %d of %d pixels differ; first at row %d, column %d: device %r, restatement %r (its triangle there: %d)"
                    % (name, pose, what, len(rr), g.size, rr[0], cc[0], got[rr[0], cc[0]], want[rr[0], cc[0]], ids[rr[0], cc[0]]))


def check(name, poses, depth=None, rgbd=None):
    for k, pose in enumerate(poses):
        want_depth, want_ids = C.restated(name, pose)
        if depth is not None:
            same_bits(name, pose, "depth pass", depth[k], want_depth)
        if rgbd is not None:
            same_bits(name, pose, "depth of the colour pass", rgbd["depth"][k], want_depth)
            same_bits(name, pose, "tri_id", rgbd["tri_id"][k], want_ids)


@pytest.mark.parametrize("name", SINGLE)
def test_depth_and_colour_pass_equal_the_restatement(name):
    s = C.scene(name)
    poses = range(len(s["R"]))
    check(name, poses, depth=depth_pass(s, poses), rgbd=colour_pass(s, poses))
    assert (C.restated(name)[1] >= 0).any()


@pytest.mark.parametrize("name", C.TEXTURED)
def test_textured_pass_equals_the_restatement(name):
    s = C.scene(name)
    out = textured_pass(s, [0])
    check(name, [0], rgbd=out)
    ids = C.restated(name)[1]
    assert out["rgb"].shape == (1,) + ids.shape + (3,) and out["rgb"].dtype == np.uint8 and not out["rgb"][0][ids < 0].any()


def test_batch_beyond_the_scans_first_chunk():
    s = C.scene("G_scan_carry")
    poses = range(C.G_POSES)
    depth, rgbd = depth_pass(s, poses), colour_pass(s, poses)
    check("G_scan_carry", poses, depth=depth, rgbd=rgbd)
    for i in C.G_ALONE:
        assert depth_pass(s, [i])[0].tobytes() == depth[i].tobytes(), i
        alone = colour_pass(s, [i])
        assert alone["depth"][0].tobytes() == rgbd["depth"][i].tobytes() and alone["tri_id"][0].tobytes() == rgbd["tri_id"][i].tobytes(), i
    assert all((rgbd["tri_id"][i] >= 0).sum() > 100 for i in C.G_ALONE) and not any(rgbd["tri_id"][i].max() >= 0 for i in C.G_OFF_SCREEN)


def test_too_many_bins_are_refused_before_anything_is_allocated():
    """65535 poses of 16384 x 16384 are 1.7e10 (pose, tile) bins, more than the int the scan takes; the outputs alone would be 70 TB"""
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    ctx, n = default_context(), 65535
    args = (dev(np.eye(3)), dev([[0, 1, 2]], torch.int32), dev(np.tile(np.eye(3), (n, 1, 1))), dev(np.zeros((n, 3))), dev(np.ones((n, 4))))
    for call in (lambda: ops.render_depth(ctx, *args, 16384, 16384),
                 lambda: ops.render_rgbd(ctx, *args, 16384, 16384, shading="flat", outputs=("depth",)),
                 lambda: ops.render_rgbd_tex(ctx, *args, 16384, 16384, shading="flat", outputs=("depth",))):
        with pytest.raises(ValueError, match="unsupported shape"):
            call()
    p = ops._ptr
    one = torch.zeros(1, dtype=torch.float32, device="cuda")
    assert ops.lib.pp_render_depth_f32(ctx.handle, n, 3, p(args[0]), 1, p(args[1]), p(args[2]), p(args[3]), p(args[4]), 16384, 16384, 100.0,
                                       10000.0, p(one), 4, p(one)) == -2
    assert "n_pose * tiles" in ops.lib.pp_last_error_string(ctx.handle).decode()
