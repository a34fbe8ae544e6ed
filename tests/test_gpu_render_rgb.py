"""GPU: the colour renderer pp_render_rgbd (csrc/render.hip) and the scene image pp_scene_compose_u8 (csrc/scene_gt.hip) through ops.render_rgbd,
utils.renderer.render_rgbd_batch / render_object and utils.scene_gt.render_scenes, against the numpy restatement
tests/render_rgb_np.py (pinned to closed forms by tests/test_render_rgb_cpu.py).  Depth is compared with the depth pass bit for
bit, colour with the restatement fed the device's own triangle ids, so that coverage differences cannot enter."""
import numpy as np
import pytest
import torch

from tests import render_np as RN
from tests import render_rgb_np as RR
from tests.test_gpu_scene_gt import BOX, MODELS, SCENES, TETRA
from tests.test_render_rgb_cpu import EYE, ORIGIN, centred_square

pytestmark = pytest.mark.gpu
W, H = 128, 96
K = np.array([[500.0, 0.0, 64.0], [0.0, 480.0, 48.0], [0.0, 0.0, 1.0]])
W2, H2 = 70, 45                                                        # no multiple of 32 or of 4
K2 = np.array([[150.0, 0.0, 35.3], [0.0, 150.0, 22.1], [0.0, 0.0, 1.0]])
NEAR, FAR = 10.0, 10000.0
LIGHTS = {"origin": (0.0, 0.0, 0.0), "offset": (200.0, -100.0, 0.0)}
ALL = ("rgb", "rgb_f32", "depth", "tri_id")


def rot(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def _scene():
    """the mesh and the 4 poses of test_gpu_render.test_matches_numpy_restatement (the last one a close-up: triangles far larger
    than a tile), with random vertex colours and noisy outward normals"""
    rng = np.random.default_rng(7)
    m = RN.sphere_mesh(40.0, 12, 18, scale=(1.0, 0.6, 0.8))
    smooth = m["pts"].copy()
    m["pts"] = m["pts"] + rng.normal(scale=1.5, size=m["pts"].shape)
    Rs = [rot(rng) for _ in range(4)]
    ts = [[rng.uniform(-20, 20), rng.uniform(-15, 15), rng.uniform(250, 600)] for _ in range(4)]
    ts[3] = [10.0, -5.0, 70.0]
    m["colors"] = rng.uniform(size=m["pts"].shape)
    m["normals"] = smooth + rng.normal(scale=4.0, size=smooth.shape)   # not unit length: the kernel normalises
    return m, np.stack(Rs), np.asarray(ts)


MESH, RS, TS = _scene()


def rgbd(model=MESH, R=RS, t=TS, K=K, w=W, h=H, outputs=ALL, **kw):
    from pyrapose_amd.utils.renderer import render_rgbd_batch
    kw.setdefault("clip_near", NEAR)
    kw.setdefault("clip_far", FAR)
    out = render_rgbd_batch(model, (w, h), K, np.asarray(R).reshape(-1, 3, 3), np.asarray(t).reshape(-1, 3), outputs=outputs, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def depth_pass(model=MESH, R=RS, t=TS, K=K, w=W, h=H):
    from pyrapose_amd.utils.renderer import render_depth_batch
    return render_depth_batch(model, (w, h), K, np.asarray(R).reshape(-1, 3, 3), np.asarray(t).reshape(-1, 3), NEAR, FAR).cpu().numpy()


@pytest.fixture(scope="module")
def full():
    """all four outputs of the 4 poses at 128 x 96, phong, defaults"""
    out = rgbd()
    for v in out.values():
        v.setflags(write=False)
    return out


def restated(i, ids, shading, ambient, light, K=K, bg=(0.0, 0.0, 0.0)):
    return RR.shade_rgb(MESH["pts"], MESH["faces"], MESH["colors"], MESH["normals"], K, RS[i], TS[i], ids, shading, ambient, light, bg)


@pytest.mark.parametrize("w,h,Kc", [(W, H, K), (W2, H2, K2)])
def test_depth_is_the_depth_pass_bit_for_bit(w, h, Kc):
    out = rgbd(K=Kc, w=w, h=h)
    want = depth_pass(K=Kc, w=w, h=h)
    assert out["depth"].dtype == np.float32 and out["depth"].shape == (4, h, w) and (want > 0).sum() > 1500
    assert np.array_equal(out["depth"].view(np.uint32), want.view(np.uint32))
    assert (want[3] > 0).mean() > 0.5                                  # the close-up fills the image: the big-triangle path
    assert out["rgb"].shape == (4, h, w, 3) and out["rgb"].dtype == np.uint8 and out["rgb_f32"].dtype == np.float32
    assert out["tri_id"].dtype == np.int32
    # each output asked for alone is the one of the joint call
    for name in ALL:
        alone = rgbd(K=Kc, w=w, h=h, outputs=(name,))
        assert list(alone) == [name] and alone[name].tobytes() == out[name].tobytes(), name


def test_triangle_ids_follow_the_tie_rule(full):
    ids, depth = full["tri_id"], full["depth"]
    assert np.array_equal(ids >= 0, depth > 0) and ids.max() < len(MESH["faces"]) and ids.min() == -1
    checked = 0
    for i in range(4):
        want_depth, want = RR.render_ids(MESH["pts"], MESH["faces"], K, RS[i], TS[i], W, H, NEAR, FAR)
        assert np.array_equal(ids[i], want), (i, int((ids[i] != want).sum()))                      # every pixel, edges included
        assert np.array_equal(depth[i].view(np.uint32), want_depth.view(np.uint32)), i
        assert np.array_equal(want, RR.smallest_id_at_depth(MESH["pts"], MESH["faces"], K, RS[i], TS[i], W, H, depth[i], NEAR, FAR)), i
        checked += int((want >= 0).sum())
    assert checked > 5000
    # a duplicated face, in both windings: the smaller index everywhere
    tri = {"pts": np.array([RR.unproject(10.25, 10.25, 500.0, K), RR.unproject(90.75, 20.25, 500.0, K), RR.unproject(40.25, 80.75, 650.0, K)])}
    for faces in ([[0, 1, 2], [0, 1, 2]], [[2, 1, 0], [2, 1, 0]]):
        out = rgbd(dict(tri, faces=np.array(faces)), EYE, ORIGIN, outputs=("depth", "tri_id"))
        want_depth, want_ids = RR.render_ids(tri["pts"], np.array(faces), K, EYE, ORIGIN, W, H, NEAR, FAR)
        assert (out["depth"][0] > 0).sum() > 1000 and np.all(out["tri_id"][0][out["depth"][0] > 0] == 0)
        assert np.array_equal(out["tri_id"][0], want_ids) and np.array_equal(out["depth"][0], want_depth)


@pytest.mark.parametrize("light", sorted(LIGHTS))
@pytest.mark.parametrize("shading", ["flat", "phong"])
def test_colour_equals_the_restatement_on_the_device_visibility(shading, light, full):
    for ambient in (0.0, 0.5, 1.0):
        out = rgbd(outputs=("rgb_f32", "tri_id"), shading=shading, ambient_weight=ambient, light_cam_pos=LIGHTS[light])
        assert np.array_equal(out["tri_id"], full["tri_id"])
        for i in range(4):
            want, _ = restated(i, out["tri_id"][i], shading, ambient, LIGHTS[light])
            got = out["rgb_f32"][i]
            differ = got != want
            print("%s %s ambient %.1f pose %d: %d of %d values differ, max |diff| %.3g" %
                  (shading, light, ambient, i, differ.sum(), differ.size, np.abs(got.astype(np.float64) - want).max()))
            assert np.array_equal(got, want), (shading, light, ambient, i)
        if ambient < 1.0:
            lit = out["rgb_f32"][out["tri_id"] >= 0]
            assert lit.min() >= 0.0 and lit.max() <= 1.0 and lit.std() > 0.05


def test_uint8_is_the_rounded_float_image(full):
    assert np.array_equal(full["rgb"], np.round(full["rgb_f32"] * np.float32(255)).astype(np.uint8))
    assert len(np.unique(full["rgb"])) > 100


def test_background_repeatability_and_an_empty_image(full):
    bg = (0.25, 0.5, 1.0)
    out = rgbd(bg_color=bg)
    empty = out["tri_id"] < 0
    assert 1000 < empty.sum() < empty.size - 1000
    assert np.all(out["rgb_f32"][empty] == np.array(bg, np.float32)) and np.all(out["rgb"][empty] == np.array([64, 128, 255], np.uint8))
    assert np.all(out["depth"][empty] == 0.0)
    for name in ALL:                                                   # the object's pixels do not depend on the background
        assert np.array_equal(out[name][~empty], full[name][~empty])
    again = rgbd(bg_color=bg)
    for name in ALL:
        assert again[name].tobytes() == out[name].tobytes(), name
    off = rgbd(R=EYE, t=[5000.0, 0.0, 500.0], bg_color=bg)
    assert np.all(off["tri_id"] == -1) and not off["depth"].any() and np.all(off["rgb"] == np.array([64, 128, 255], np.uint8))
    assert np.all(off["rgb_f32"] == np.array(bg, np.float32))


def test_analytic_scenes_on_the_device():
    m = centred_square(K, 500.0)
    inside = np.zeros((H, W), bool)
    inside[32:64, 44:84] = True                                        # pixel centres inside 64 +- 20.25 x 48 +- 15.75
    # full ambient light: exactly the colour, and its rounded bytes
    c = np.array([0.2, 0.6, 1.0])
    for shading, normals in (("flat", None), ("phong", np.tile([0.3, -0.2, -1.0], (4, 1)))):
        out = rgbd(dict(m, colors=np.tile(c, (4, 1)), normals=normals), EYE, ORIGIN, shading=shading, ambient_weight=1.0)
        assert np.array_equal(out["tri_id"][0] >= 0, inside)
        assert np.all(out["rgb_f32"][0][inside] == c.astype(np.float32)) and np.all(out["rgb"][0][inside] == np.array([51, 153, 255], np.uint8))
        assert np.all(out["depth"][0][inside] == np.float32(500.0))
    # phong with normals facing away: ambient light only
    c = np.array([0.5, 0.25, 0.75])
    away = dict(m, colors=np.tile(c, (4, 1)), normals=np.tile([0.0, 0.0, 1.0], (4, 1)))
    out = rgbd(away, EYE, ORIGIN, shading="phong", ambient_weight=0.5)
    assert np.all(out["rgb_f32"][0][inside] == (0.5 * c).astype(np.float32))
    # render_object: the reference's keys per mode, surf_color, a model without colours is grey
    from pyrapose_amd.utils.renderer import render_object
    both = render_object(away, (W, H), K, EYE, [0.0, 0.0, 0.0], clip_near=NEAR, ambient_weight=0.5)
    assert sorted(both) == ["depth", "rgb"] and both["rgb"].shape == (H, W, 3) and both["rgb"].dtype == np.uint8
    assert both["depth"].shape == (H, W) and both["depth"].dtype == np.float32 and np.array_equal(both["rgb"], out["rgb"][0])
    assert sorted(render_object(away, (W, H), K, EYE, ORIGIN, mode="rgb")) == ["rgb"]
    assert sorted(render_object(away, (W, H), K, EYE, ORIGIN, mode="depth")) == ["depth"]
    red = render_object(away, (W, H), K, EYE, ORIGIN, mode="rgb", surf_color=(1.0, 0.0, 0.0), ambient_weight=1.0)["rgb"]
    assert np.all(red[inside] == np.array([255, 0, 0], np.uint8))
    grey = render_object({"pts": m["pts"], "faces": m["faces"]}, (W, H), K, EYE, ORIGIN, mode="rgb", shading="flat", ambient_weight=1.0)["rgb"]
    assert np.all(grey[inside] == 128) and not grey[~inside].any()
    bytes_ = render_object(dict(m, colors=np.tile([51.0, 153.0, 255.0], (4, 1))), (W, H), K, EYE, ORIGIN, mode="rgb", shading="flat",
                           ambient_weight=1.0)["rgb"]
    assert np.all(bytes_[inside] == np.array([51, 153, 255], np.uint8))


def coloured_models():
    rng = np.random.default_rng(21)
    return {o: dict(m, colors=rng.uniform(size=m["pts"].shape)) for o, m in MODELS.items()}


def test_scene_images_are_composed_from_the_instances():
    """the two scenes of test_gpu_scene_gt.py (instances cut by the border, hidden, off screen, two visible on one pixel) with an
    empty scene between them, 70 x 45"""
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    from pyrapose_amd.utils import scene_gt as SG
    from pyrapose_amd.utils._host import k4, to_device
    from pyrapose_amd.utils.renderer import render_rgbd_batch
    scenes, models = [SCENES[0], [], SCENES[1]], coloured_models()
    rng = np.random.default_rng(22)
    bg = rng.integers(0, 256, size=(3, H2, W2, 3)).astype(np.uint8)
    kw = dict(shading="flat", ambient_weight=0.3, light_cam_pos=(100.0, -50.0, 0.0))
    images, info = SG.render_scenes(scenes, models, K2, (W2, H2), background=bg, channel_order="rgb", **kw)
    assert torch.is_tensor(images) and images.is_cuda and images.dtype == torch.uint8 and tuple(images.shape) == (3, H2, W2, 3)
    images = images.cpu().numpy()
    # the pieces, called directly
    plan = SG.plan_instances(scenes)
    assert plan.scene_offsets.tolist() == [0, 4, 4, 5] and list(plan.groups) == [BOX, TETRA]
    renders = [render_rgbd_batch(models[o], (W2, H2), K2, plan.R[idx], plan.t[idx], **kw) for o, idx in plan.groups.items()]
    order = torch.from_numpy(plan.order).cuda()
    depth, rgb = (torch.cat([r[k] for r in renders])[order] for k in ("depth", "rgb"))
    gt = ops.scene_gt_info(default_context(), depth, plan.scene_offsets, to_device(k4(K2, 5)))
    ids, rgb = gt.id_image.cpu().numpy(), rgb.cpu().numpy()
    assert sorted(np.unique(ids[0]).tolist()) == [0, 1, 3] and not ids[1].any() and np.unique(ids[2]).tolist() == [0, 1]
    assert np.array_equal(images, RR.compose(ids, rgb, plan.scene_offsets, bg, "rgb"))
    assert np.array_equal(images[ids == 0], bg[ids == 0]) and np.array_equal(images[1], bg[1])
    shown = (ids[0] == 3)
    assert shown.sum() > 5 and np.array_equal(images[0][shown], rgb[2][shown])          # the later of two visible instances
    assert info == SG.scene_gt_info(scenes, models, K2, None, (W2, H2)).info and [len(rows) for rows in info] == [4, 0, 1]
    # BGR (the default) is RGB reversed; one background image for all scenes; a constant; none
    assert np.array_equal(SG.render_scenes(scenes, models, K2, (W2, H2), background=bg, **kw)[0].cpu().numpy(), images[..., ::-1])
    shared = SG.render_scenes(scenes, models, K2, (W2, H2), background=torch.from_numpy(bg[1]).cuda(), channel_order="rgb", **kw)[0].cpu().numpy()
    assert np.array_equal(shared, RR.compose(ids, rgb, plan.scene_offsets, np.broadcast_to(bg[1], bg.shape), "rgb"))
    const = SG.render_scenes(scenes, models, K2, (W2, H2), background=(10, 20, 30), **kw)[0].cpu().numpy()
    assert np.array_equal(const, RR.compose(ids, rgb, plan.scene_offsets, (10, 20, 30), "bgr")) and np.all(const[1] == np.array([30, 20, 10], np.uint8))
    black = SG.render_scenes(scenes, models, K2, (W2, H2), channel_order="rgb", **kw)[0].cpu().numpy()
    assert np.array_equal(black, RR.compose(ids, rgb, plan.scene_offsets, (0, 0, 0), "rgb"))
    # no instance at all: the background
    nothing, no_info = SG.render_scenes([[], []], models, K2, (W2, H2), background=bg[:2], channel_order="rgb")
    assert np.array_equal(nothing.cpu().numpy(), bg[:2]) and no_info == [[], []]


def test_refused_arguments_launch_nothing(full):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    from pyrapose_amd.utils import scene_gt as SG
    from pyrapose_amd.utils.renderer import render as render_one
    from pyrapose_amd.utils.renderer import render_object, render_rgbd_batch
    ctx = default_context()
    args = (MESH, (W, H), K, RS, TS)
    no_normals = {k: v for k, v in MESH.items() if k != "normals"}
    refused = [lambda: render_rgbd_batch(no_normals, *args[1:], shading="phong"),
               lambda: render_rgbd_batch(dict(no_normals, texture_file="obj.png", texture_uv=np.zeros((len(MESH["pts"]), 2))), *args[1:], shading="flat"),
               lambda: render_rgbd_batch(dict(MESH, colors=MESH["colors"][:-1]), *args[1:]),
               lambda: render_rgbd_batch(dict(MESH, colors=MESH["colors"] * 300.0), *args[1:]),
               lambda: render_rgbd_batch(*args, outputs=()),
               lambda: render_rgbd_batch(*args, outputs=("rgb", "normals")),
               lambda: render_rgbd_batch(*args, shading="gouraud"),
               lambda: render_rgbd_batch(MESH, (0, H), K, RS, TS),
               lambda: render_rgbd_batch(MESH, (W, 0), K, RS, TS),
               lambda: render_rgbd_batch(*args, clip_near=500.0, clip_far=100.0),
               lambda: render_rgbd_batch(*args, ambient_weight=-0.5),
               lambda: render_rgbd_batch(*args, bg_color=(0.0, 2.0, 0.0)),
               lambda: render_rgbd_batch(*args, light_cam_pos=(0.0, float("inf"), 0.0)),
               lambda: render_object(MESH, (W, H), K, RS[0], TS[0], mode="rgbd"),
               lambda: render_one(MESH, (W, H), K, RS[0], TS[0], mode="rgb")]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d was not refused" % k)
    # a texture is no obstacle once surf_color says what to draw; flat shading needs no normals
    render_rgbd_batch(dict(no_normals, texture_file="obj.png"), *args[1:], shading="flat", surf_color=(0.2, 0.4, 0.6))
    # the raw wrapper: colours of another length, phong without normals, no output
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.asarray(a), dtype=dt).cuda()
    raw = (dev(MESH["pts"]), dev(MESH["faces"], torch.int32), dev(RS), dev(TS), dev(np.tile([500.0, 480.0, 64.0, 48.0], (4, 1))), W, H)
    with pytest.raises(ValueError):
        ops.render_rgbd(ctx, *raw, colors=dev(MESH["colors"][:-1]), normals=dev(MESH["normals"]))
    with pytest.raises(ValueError, match=r"pp_render_rgbd failed \(-1\)"):
        ops.render_rgbd(ctx, *raw, colors=dev(MESH["colors"]), shading="phong")
    with pytest.raises(ValueError, match=r"pp_render_rgbd failed \(-1\)"):
        ops.render_rgbd(ctx, *raw, shading="flat", outputs=("rgb",))                # a colour output without colours
    with pytest.raises(ValueError):
        ops.render_rgbd(ctx, *raw, colors=dev(MESH["colors"]), shading="flat", outputs=())
    assert ops.lib.pp_render_rgbd(ctx.handle, 4, 10, None, None, None, 5, None, None, None, None, W, H, 10.0, 100.0, 0, 0.5, None, None,
                                  None, 0, None, None, None, None) == -1            # nothing requested, nothing given
    assert ops.lib.pp_render_rgbd_workspace_bytes(0, 10, 5, W, H) == 0 and ops.lib.pp_render_rgbd_workspace_bytes(4, 10, 5, W, 20000) == 0
    assert ops.lib.pp_render_rgbd_workspace_bytes(4, 10, 5, W, H) > ops.lib.pp_render_workspace_bytes(4, 10, 5, W, H) > 0
    # compose: offsets that do not match the stack, a scene of more than 255 instances, an unknown channel order
    ids, colors = torch.zeros((2, 4, 5), dtype=torch.uint8).cuda(), torch.zeros((3, 4, 5, 3), dtype=torch.uint8).cuda()
    for offsets in ([0, 2, 4], [0, 3], [1, 2, 3], [0, 3, 2]):
        with pytest.raises(ValueError):
            ops.scene_compose(ctx, ids, colors, offsets)
    with pytest.raises(ValueError, match=r"pp_scene_compose_u8 failed \(-2\)"):
        ops.scene_compose(ctx, ids[:1], torch.zeros((256, 4, 5, 3), dtype=torch.uint8).cuda(), [0, 256])
    with pytest.raises(ValueError):
        ops.scene_compose(ctx, ids, colors, [0, 2, 3], channel_order="rgba")
    with pytest.raises(ValueError):
        ops.scene_compose(ctx, ids, colors, [0, 2, 3], background=(0, 0, 256))
    assert not ops.scene_compose(ctx, ids, colors, [0, 2, 3]).any()
    crowd = [[{"obj_id": TETRA, "R": np.eye(3), "t": [0.0, 0.0, 500.0]}] * 256]
    with pytest.raises(ValueError):
        SG.render_scenes(crowd, coloured_models(), K2, (W2, H2), shading="flat")
    with pytest.raises(ValueError):
        SG.render_scenes([SCENES[1]], coloured_models(), K2, (W2, H2), shading="flat", channel_order="gbr")
    with pytest.raises(ValueError):
        SG.render_scenes([SCENES[1]], coloured_models(), K2, (W2, H2), shading="flat", background=np.zeros((H2, W2 + 1, 3), np.uint8))
    with pytest.raises(ValueError):
        SG.render_scenes([SCENES[1]], coloured_models(), K2, (W2, H2), shading="phong")    # these models carry no normals
    # the next valid call works and repeats the bits
    assert rgbd()["rgb"].tobytes() == full["rgb"].tobytes()
