"""GPU: the textured colour pass pp_render_rgbd_tex (csrc/render.hip) through utils.renderer.render_rgbd_batch /
render_object and utils.scene_gt.render_scenes, against the numpy restatement tests/render_tex_np.py (pinned to closed forms by
tests/test_render_tex_cpu.py).  Colour is compared bit for bit with the restatement fed the device's own triangle ids, depth
and ids byte for byte with the untextured pass."""
import numpy as np
import pytest
import torch

from tests import render_rgb_np as RR
from tests import render_tex_np as RT
from tests.test_gpu_render_rgb import ALL, FAR, H2, K2, LIGHTS, MESH, NEAR, RS, TS, W2, H, K, W, coloured_models
from tests.test_gpu_scene_gt import BOX, MODELS, SCENES, TETRA
from tests.test_render_rgb_cpu import EYE, ORIGIN
from tests.test_render_tex_cpu import UNIT_UV, analytic_square, clamped_twice

pytestmark = pytest.mark.gpu
SIZES = [(W, H, K), (W2, H2, K2)]


def _textured():
    """the sphere of test_gpu_render_rgb.py with a 37 x 23 texture -- odd, not square, no power of two -- and UVs from a
    spherical parametrisation stretched over [-0.6, 1.7] x [-0.4, 1.5], so that a good share lies outside [0, 1]"""
    rng = np.random.default_rng(31)
    p = MESH["pts"] / np.linalg.norm(MESH["pts"], axis=1, keepdims=True)
    lon, lat = np.arctan2(p[:, 1], p[:, 0]) / (2.0 * np.pi) + 0.5, np.arccos(np.clip(p[:, 2], -1.0, 1.0)) / np.pi
    uv = np.stack([-0.6 + 2.3 * lon, -0.4 + 1.9 * lat], axis=1)
    tex = rng.integers(0, 256, size=(23, 37, 3)).astype(np.uint8)
    return dict({k: v for k, v in MESH.items() if k != "colors"}, texture_uv=uv, texture=tex)


TMESH = _textured()
PLAIN = {k: v for k, v in MESH.items()}                                # the same geometry with vertex colours


def rgbd(model=TMESH, R=RS, t=TS, K=K, w=W, h=H, outputs=ALL, **kw):
    from pyrapose_amd.utils.renderer import render_rgbd_batch
    kw.setdefault("clip_near", NEAR)
    kw.setdefault("clip_far", FAR)
    out = render_rgbd_batch(model, (w, h), K, np.asarray(R).reshape(-1, 3, 3), np.asarray(t).reshape(-1, 3), outputs=outputs, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("shading", ["flat", "phong"])
@pytest.mark.parametrize("wrap", RT.WRAPS)
@pytest.mark.parametrize("filter", RT.FILTERS)
def test_colour_equals_the_restatement_on_the_device_visibility(filter, wrap, shading):
    light = LIGHTS["offset"]
    textured = outside = 0
    values = set()
    for w, h, Kc in SIZES:
        for ambient in (0.0, 0.5, 1.0):
            out = rgbd(K=Kc, w=w, h=h, outputs=("rgb_f32", "tri_id"), shading=shading, ambient_weight=ambient, light_cam_pos=light,
                       tex_filter=filter, tex_wrap=wrap)
            for i in range(4):
                ids = out["tri_id"][i]
                want, _ = RT.shade_rgb_tex(TMESH["pts"], TMESH["faces"], TMESH["texture_uv"], TMESH["texture"], TMESH["normals"], Kc,
                                           RS[i], TS[i], ids, filter, wrap, shading, ambient, light)
                got = out["rgb_f32"][i]
                differ = got != want
                print("%s %s %s %dx%d ambient %.1f pose %d: %d of %d values differ, max |diff| %.3g" %
                      (filter, wrap, shading, w, h, ambient, i, differ.sum(), differ.size, np.abs(got.astype(np.float64) - want).max()))
                assert np.array_equal(got, want), (filter, wrap, shading, w, h, ambient, i)
                if ambient == 0.5:
                    coords = RT.interp_uv(TMESH["pts"], TMESH["faces"], TMESH["texture_uv"], Kc, RS[i], TS[i], ids)[ids >= 0]
                    textured += len(coords)
                    outside += int(((coords < 0.0) | (coords > 1.0)).any(axis=1).sum())
                    values.update(np.unique(got[ids >= 0]).tolist())
    # the test sees what it claims to see
    print("textured pixels %d, with a coordinate outside [0, 1] %d, distinct values %d" % (textured, outside, len(values)))
    assert textured > 5000 and outside > 0.1 * textured and len(values) > 100


@pytest.fixture(scope="module")
def joint():
    out = rgbd(tex_filter="bilinear", tex_wrap="repeat")
    for v in out.values():
        v.setflags(write=False)
    return out


def test_geometry_does_not_depend_on_texturing(joint):
    plain = rgbd(PLAIN)
    assert (plain["depth"] > 0).sum() > 5000
    for name in ("depth", "tri_id"):
        assert joint[name].tobytes() == plain[name].tobytes(), name
    assert not np.array_equal(joint["rgb"], plain["rgb"])
    assert np.array_equal(joint["rgb"], RR.to_u8(joint["rgb_f32"])) and len(np.unique(joint["rgb"])) > 100
    for name in ALL:                                                   # each output asked for alone is the one of the joint call
        alone = rgbd(outputs=(name,), tex_filter="bilinear", tex_wrap="repeat")
        assert list(alone) == [name] and alone[name].tobytes() == joint[name].tobytes(), name
    again = rgbd(tex_filter="bilinear", tex_wrap="repeat")
    for name in ALL:
        assert again[name].tobytes() == joint[name].tobytes(), name
    # the 70 x 45 image too, and a background colour where nothing is drawn
    small, small_plain = rgbd(K=K2, w=W2, h=H2, bg_color=(0.25, 0.5, 1.0)), rgbd(PLAIN, K=K2, w=W2, h=H2)
    for name in ("depth", "tri_id"):
        assert small[name].tobytes() == small_plain[name].tobytes(), name
    empty = small["tri_id"] < 0
    assert empty.sum() > 500 and np.all(small["rgb"][empty] == np.array([64, 128, 255], np.uint8)) and np.all(small["depth"][empty] == 0.0)
    # an RGBX texture, a float texture on the 1/255 grid and a device tensor are the same texture
    for same in (np.concatenate([TMESH["texture"], np.full((23, 37, 1), 3, np.uint8)], axis=2), TMESH["texture"].astype(np.float64) / 255.0,
                 (TMESH["texture"].astype(np.float32) / np.float32(255.0)), torch.from_numpy(TMESH["texture"]).cuda()):
        assert rgbd(outputs=("rgb",), texture=same, tex_filter="bilinear", tex_wrap="repeat")["rgb"].tobytes() == joint["rgb"].tobytes()


def test_analytic_scenes_on_the_device():
    m = analytic_square()
    rng = np.random.default_rng(11)
    tex = rng.integers(0, 256, size=(32, 40, 3)).astype(np.uint8)
    inside = np.zeros((H, W), bool)
    inside[32:64, 44:84] = True
    for uv, want in ((UNIT_UV, tex[::-1]), (UNIT_UV * [1.0, -1.0] + [0.0, 1.0], tex)):
        for filter in RT.FILTERS:
            for wrap in RT.WRAPS:
                out = rgbd(dict(m, texture_uv=uv, texture=tex), EYE, ORIGIN, shading="flat", ambient_weight=1.0, tex_filter=filter, tex_wrap=wrap)
                assert np.array_equal(out["tri_id"][0] >= 0, inside) and np.all(out["depth"][0][inside] == np.float32(500.0))
                assert np.array_equal(out["rgb"][0][32:64, 44:84], want), (filter, wrap)
                assert not out["rgb"][0][~inside].any()
    tex2 = rng.integers(0, 256, size=(16, 20, 3)).astype(np.uint8)
    twice = dict(m, texture_uv=UNIT_UV * 2.0, texture=tex2)
    for filter in RT.FILTERS:
        rep = rgbd(twice, EYE, ORIGIN, shading="flat", ambient_weight=1.0, tex_filter=filter, tex_wrap="repeat")["rgb"][0]
        assert np.array_equal(rep[32:64, 44:84], np.tile(tex2[::-1], (2, 2, 1))), filter
        cl = rgbd(twice, EYE, ORIGIN, shading="flat", ambient_weight=1.0, tex_filter=filter, tex_wrap="clamp")["rgb"][0]
        assert np.array_equal(cl[32:64, 44:84], clamped_twice(tex2)), filter
    # ambient light only (phong normals facing away): half the texel
    away = dict(m, texture_uv=UNIT_UV, texture=tex, normals=np.tile([0.0, 0.0, 1.0], (4, 1)))
    half = rgbd(away, EYE, ORIGIN, shading="phong", ambient_weight=0.5)["rgb_f32"][0]
    assert np.array_equal(half[32:64, 44:84], (0.5 * (tex[::-1].astype(np.float64) / 255.0)).astype(np.float32))


def test_render_object_and_scenes_with_textured_meshes():
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    from pyrapose_amd.utils import scene_gt as SG
    from pyrapose_amd.utils._host import k4, to_device
    from pyrapose_amd.utils.renderer import render_object, render_rgbd_batch
    want = rgbd(R=RS[:1], t=TS[:1])
    both = render_object(TMESH, (W, H), K, RS[0], TS[0], clip_near=NEAR, clip_far=FAR)
    assert sorted(both) == ["depth", "rgb"] and both["rgb"].shape == (H, W, 3) and both["rgb"].dtype == np.uint8
    assert both["depth"].dtype == np.float32 and np.array_equal(both["rgb"], want["rgb"][0]) and np.array_equal(both["depth"], want["depth"][0])
    assert sorted(render_object(TMESH, (W, H), K, RS[0], TS[0], mode="rgb", clip_near=NEAR)) == ["rgb"]
    assert sorted(render_object(TMESH, (W, H), K, RS[0], TS[0], mode="depth", clip_near=NEAR)) == ["depth"]
    # texture= serves a model that carries only its UVs; the keywords reach the sampler
    bare = {k: v for k, v in TMESH.items() if k != "texture"}
    kw = dict(mode="rgb", clip_near=NEAR, clip_far=FAR, tex_filter="bilinear", tex_wrap="repeat")
    passed = render_object(bare, (W, H), K, RS[0], TS[0], texture=TMESH["texture"], **kw)["rgb"]
    assert np.array_equal(passed, rgbd(R=RS[:1], t=TS[:1], tex_filter="bilinear", tex_wrap="repeat")["rgb"][0]) and not np.array_equal(passed, both["rgb"])
    # surf_color wins over the texture: the picture of the untextured mesh in that colour
    red = render_object(TMESH, (W, H), K, RS[0], TS[0], mode="rgb", clip_near=NEAR, clip_far=FAR, surf_color=(1.0, 0.2, 0.0))["rgb"]
    assert np.array_equal(red, rgbd(PLAIN, RS[:1], TS[:1], surf_color=(1.0, 0.2, 0.0))["rgb"][0]) and not np.array_equal(red, both["rgb"])
    # a scene set mixing a textured box and a vertex-coloured tetrahedron, as test_gpu_render_rgb.py composes it
    rng = np.random.default_rng(41)
    models = coloured_models()
    box = {k: v for k, v in models[BOX].items() if k != "colors"}
    models[BOX] = dict(box, texture_uv=rng.uniform(-0.5, 1.5, size=(len(box["pts"]), 2)), texture=rng.integers(0, 256, size=(9, 14, 3)).astype(np.uint8))
    scenes = [SCENES[0], [], SCENES[1]]
    bg = rng.integers(0, 256, size=(3, H2, W2, 3)).astype(np.uint8)
    kw = dict(shading="flat", ambient_weight=0.3, light_cam_pos=(100.0, -50.0, 0.0), tex_filter="bilinear", tex_wrap="repeat")
    images, info = SG.render_scenes(scenes, models, K2, (W2, H2), background=bg, channel_order="rgb", **kw)
    images = images.cpu().numpy()
    plan = SG.plan_instances(scenes)
    assert list(plan.groups) == [BOX, TETRA]
    renders = [render_rgbd_batch(models[o], (W2, H2), K2, plan.R[idx], plan.t[idx], **kw) for o, idx in plan.groups.items()]
    order = torch.from_numpy(plan.order).cuda()
    depth, rgb = (torch.cat([r[k] for r in renders])[order] for k in ("depth", "rgb"))
    gt = ops.scene_gt_info(default_context(), depth, plan.scene_offsets, to_device(k4(K2, 5)))
    ids, rgb = gt.id_image.cpu().numpy(), rgb.cpu().numpy()
    assert np.array_equal(images, RR.compose(ids, rgb, plan.scene_offsets, bg, "rgb")) and (ids > 0).any()
    assert info == SG.scene_gt_info(scenes, MODELS, K2, None, (W2, H2)).info
    # the box's pixels are the restatement's texture samples, and they differ from the picture of the vertex-coloured box
    idx = plan.groups[BOX]
    one = render_rgbd_batch(models[BOX], (W2, H2), K2, plan.R[idx], plan.t[idx], outputs=("rgb", "tri_id"), **kw)
    tri, got, seen = one["tri_id"].cpu().numpy(), one["rgb"].cpu().numpy(), 0
    for k, i in enumerate(idx):
        _, u8 = RT.shade_rgb_tex(models[BOX]["pts"], models[BOX]["faces"], models[BOX]["texture_uv"], models[BOX]["texture"], None, K2,
                                 plan.R[i], plan.t[i], tri[k], "bilinear", "repeat", "flat", 0.3, (100.0, -50.0, 0.0))
        assert np.array_equal(got[k], u8), k
        seen += int((tri[k] >= 0).sum())
    assert seen > 50
    plain_images, _ = SG.render_scenes(scenes, coloured_models(), K2, (W2, H2), background=bg, channel_order="rgb", **kw)
    assert not np.array_equal(plain_images.cpu().numpy(), images)


def test_refused_arguments_launch_nothing(joint):
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    from pyrapose_amd.utils import scene_gt as SG
    from pyrapose_amd.utils.renderer import render_object, render_rgbd_batch
    ctx = default_context()
    args = ((W, H), K, RS, TS)
    nv = len(TMESH["pts"])
    nan_uv = TMESH["texture_uv"].copy()
    nan_uv[5, 1] = np.nan
    inf_uv = TMESH["texture_uv"].copy()
    inf_uv[0, 0] = np.inf
    refused = [lambda: render_rgbd_batch(dict(TMESH, texture_uv=TMESH["texture_uv"][:-1]), *args),
               lambda: render_rgbd_batch(dict(TMESH, texture_uv=np.zeros((nv, 3))), *args),
               lambda: render_rgbd_batch(dict(TMESH, texture_uv=nan_uv), *args),
               lambda: render_rgbd_batch(dict(TMESH, texture_uv=inf_uv), *args),
               lambda: render_rgbd_batch({k: v for k, v in TMESH.items() if k != "texture_uv"}, *args),
               lambda: render_rgbd_batch(TMESH, *args, texture=TMESH["texture"].astype(np.int32)),
               lambda: render_rgbd_batch(TMESH, *args, texture=torch.from_numpy(TMESH["texture"]).cuda().float()),
               lambda: render_rgbd_batch(TMESH, *args, texture=TMESH["texture"][:, :, 0]),
               lambda: render_rgbd_batch(TMESH, *args, texture=TMESH["texture"][:, :, :2]),
               lambda: render_rgbd_batch(TMESH, *args, texture=TMESH["texture"][None]),
               lambda: render_rgbd_batch(TMESH, *args, texture=TMESH["texture"] / 256.0),
               lambda: render_rgbd_batch(TMESH, *args, texture=TMESH["texture"] * 1.0),
               lambda: render_rgbd_batch(TMESH, *args, tex_filter="trilinear"),
               lambda: render_rgbd_batch(TMESH, *args, tex_wrap="mirror"),
               lambda: render_rgbd_batch(PLAIN, *args, tex_filter="linear"),
               lambda: render_object(TMESH, (W, H), K, RS[0], TS[0], tex_wrap="mirrored_repeat"),
               lambda: SG.render_scenes([SCENES[1]], coloured_models(), K2, (W2, H2), shading="flat", tex_filter="cubic"),
               # what was refused before still is: a texture file without an image and without surf_color
               lambda: render_rgbd_batch(dict({k: v for k, v in TMESH.items() if k != "texture"}, texture_file="obj.png"), *args)]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d was not refused" % k)
    with pytest.raises(TypeError):
        SG.render_scenes([SCENES[1]], coloured_models(), K2, (W2, H2), shading="flat", texture=TMESH["texture"])
    # depth and ids alone need neither UVs nor a readable texture
    geometry = rgbd(dict(TMESH, texture_uv=None, texture="no image"), outputs=("depth", "tri_id"))
    assert geometry["depth"].tobytes() == joint["depth"].tobytes() and geometry["tri_id"].tobytes() == joint["tri_id"].tobytes()
    # the raw wrapper and the raw entry point
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.asarray(a), dtype=dt).cuda()
    raw = (dev(TMESH["pts"]), dev(TMESH["faces"], torch.int32), dev(RS), dev(TS), dev(np.tile([500.0, 480.0, 64.0, 48.0], (4, 1))), W, H)
    uv, tex = dev(TMESH["texture_uv"]), dev(np.concatenate([TMESH["texture"], np.zeros((23, 37, 1), np.uint8)], axis=2), torch.uint8)
    normals = dev(TMESH["normals"])
    for bad in (dict(uv=uv[:-1], tex=tex), dict(uv=uv, tex=tex[:, :, :3].contiguous()), dict(uv=uv, tex=tex.cpu()), dict(uv=uv, tex=tex.int()),
                dict(uv=uv, tex=tex, filter="cubic"), dict(uv=uv, tex=tex, wrap="mirror"), dict(uv=uv, tex=tex, outputs=()),
                dict(uv=uv, tex=tex[:, :0])):
        with pytest.raises(ValueError):
            ops.render_rgbd_tex(ctx, *raw, normals=normals, **bad)
    with pytest.raises(ValueError, match=r"pp_render_rgbd_tex failed \(-1\)"):
        ops.render_rgbd_tex(ctx, *raw, uv=uv, normals=normals, outputs=("rgb",))             # a colour output without a texture
    with pytest.raises(ValueError, match=r"pp_render_rgbd_tex failed \(-1\)"):
        ops.render_rgbd_tex(ctx, *raw, tex=tex, normals=normals, outputs=("rgb_f32",))       # ... without UVs
    with pytest.raises(ValueError, match=r"pp_render_rgbd_tex failed \(-1\)"):
        ops.render_rgbd_tex(ctx, *raw, uv=uv, tex=tex, shading="phong")                      # phong without normals
    lib = ops.lib
    light = bg = (ops.C.c_double * 3)(0.0, 0.0, 0.0)
    n, nt = 4, len(TMESH["faces"])
    nbytes = lib.pp_render_rgbd_tex_workspace_bytes(n, nv, nt, W, H, 37, 23)
    ws, rgb = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    p = ops._ptr
    call = lambda tex_ptr, tw, th, filter, wrap: lib.pp_render_rgbd_tex(
        ctx.handle, n, nv, p(raw[0]), p(uv), tex_ptr, tw, th, filter, wrap, p(normals), nt, p(raw[1]), p(raw[2]), p(raw[3]), p(raw[4]), W, H,
        NEAR, FAR, 1, 0.5, light, bg, p(ws), nbytes, None, None, None, p(rgb))
    assert call(None, 37, 23, 0, 0) == -1                                                     # a null tex and a colour output
    assert call(p(tex), 37, 23, 2, 0) == -1 and call(p(tex), 37, 23, 0, -1) == -1
    assert call(p(tex), 0, 23, 0, 0) == -2 and call(p(tex), 20000, 23, 0, 0) == -2 and call(p(tex), 16384, 16385, 0, 0) == -2
    torch.cuda.synchronize()
    assert not rgb.any()                                                                      # nothing was launched
    assert lib.pp_render_rgbd_tex_workspace_bytes(n, nv, nt, W, H, 0, 23) == 0 and lib.pp_render_rgbd_tex_workspace_bytes(n, nv, nt, W, H, 20000, 23) == 0
    assert nbytes == lib.pp_render_rgbd_workspace_bytes(n, nv, nt, W, H) > 0
    assert call(p(tex), 37, 23, 1, 1) == 0                                                    # the next valid call works and repeats the bits
    assert np.array_equal(rgb.cpu().numpy(), joint["rgb"])
