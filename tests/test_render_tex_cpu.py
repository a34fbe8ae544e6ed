"""CPU: the numpy restatement of the textured colour pass (tests/render_tex_np.py) against closed forms, so that the device
can be compared with the restatement alone; utils.ply_loader.load_ply(texture=True); the ABI of the two new entry points.
Texel values are exact where a sample falls on a texel centre (a weight of exactly 0 or 1); blends hold to float64
rounding, 1e-12 relative as in tests/test_render_rgb_cpu.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import render_rgb_np as RR
from tests import render_tex_np as RT
from tests.test_render_rgb_cpu import EYE, H, K, ORIGIN, RTOL, W, centred_square, rays, tilted_plane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEX_ENTRIES = ("pp_render_rgbd_tex_workspace_bytes", "pp_render_rgbd_tex")
UNIT_UV = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])   # for centred_square's corners: v = 0 at the image's top


def small_texture():
    """3 wide, 2 high, in file order: row 0 is the TOP row of the image, which is v = 1"""
    return np.array([[[10, 20, 30], [40, 50, 60], [70, 80, 90]],
                     [[110, 120, 130], [140, 150, 160], [170, 180, 190]]], np.uint8)


def test_a_texel_centres_give_the_texel_in_the_prescribed_orientation():
    tex = small_texture()
    for i in range(3):
        for j in range(2):                                             # GL texel (i, j): j = 0 is the file's bottom row
            u, v = (i + 0.5) / 3.0, (j + 0.5) / 2.0
            want = tex[1 - j, i].astype(np.float64) / 255.0
            for filter in RT.FILTERS:
                for wrap in RT.WRAPS:
                    got = RT.sample(tex, u, v, filter, wrap)
                    assert got.shape == (1, 3)
                    if filter == "nearest":
                        assert np.array_equal(got[0], want), (i, j, wrap)
                    else:
                        np.testing.assert_allclose(got[0], want, rtol=RTOL)
    # a fourth byte is ignored
    rgbx = np.concatenate([tex, np.full((2, 3, 1), 7, np.uint8)], axis=2)
    assert np.array_equal(RT.sample(rgbx, 0.4, 0.8, "bilinear", "repeat"), RT.sample(tex, 0.4, 0.8, "bilinear", "repeat"))


def test_b_blends_and_wrapping():
    tex = small_texture()
    c = lambda i, j: tex[1 - j, i].astype(np.float64) / 255.0
    # half way between the centres of texels (0, 0) and (1, 0), and of (1, 0) and (1, 1): their mean
    np.testing.assert_allclose(RT.sample(tex, 1.0 / 3.0, 0.25, "bilinear")[0], 0.5 * (c(0, 0) + c(1, 0)), rtol=RTOL)
    np.testing.assert_allclose(RT.sample(tex, 0.5, 0.5, "bilinear")[0], 0.5 * (c(1, 0) + c(1, 1)), rtol=RTOL)
    # the middle of four texels: their mean
    np.testing.assert_allclose(RT.sample(tex, 2.0 / 3.0, 0.5, "bilinear")[0], 0.25 * (c(1, 0) + c(2, 0) + c(1, 1) + c(2, 1)), rtol=RTOL)
    # u = -0.25: x = -0.75, nearest texel -1; bilinear between texels -2 and -1 with weight 0.75 on -1
    # u = 1.25: x = 3.75, nearest texel 3; bilinear between texels 3 and 4 with weight 0.25 on 4
    v = 0.25                                                           # the centre of GL row 0
    assert np.array_equal(RT.sample(tex, -0.25, v, "nearest", "clamp")[0], c(0, 0))
    assert np.array_equal(RT.sample(tex, -0.25, v, "nearest", "repeat")[0], c(2, 0))
    assert np.array_equal(RT.sample(tex, 1.25, v, "nearest", "clamp")[0], c(2, 0))
    assert np.array_equal(RT.sample(tex, 1.25, v, "nearest", "repeat")[0], c(0, 0))
    np.testing.assert_allclose(RT.sample(tex, -0.25, v, "bilinear", "clamp")[0], c(0, 0), rtol=RTOL)
    np.testing.assert_allclose(RT.sample(tex, -0.25, v, "bilinear", "repeat")[0], 0.25 * c(1, 0) + 0.75 * c(2, 0), rtol=RTOL)
    np.testing.assert_allclose(RT.sample(tex, 1.25, v, "bilinear", "clamp")[0], c(2, 0), rtol=RTOL)
    np.testing.assert_allclose(RT.sample(tex, 1.25, v, "bilinear", "repeat")[0], 0.75 * c(0, 0) + 0.25 * c(1, 0), rtol=RTOL)
    # the same in v: below the image the bottom row (clamp) or the top row (repeat)
    assert np.array_equal(RT.sample(tex, 0.5, -0.25, "nearest", "clamp")[0], c(1, 0))
    assert np.array_equal(RT.sample(tex, 0.5, -0.25, "nearest", "repeat")[0], c(1, 1))
    # repeat is periodic, far out and on the negative side; clamp saturates
    for filter in RT.FILTERS:
        base = RT.sample(tex, 0.3, 0.7, filter, "repeat")[0]
        for du, dv in ((1.0, 0.0), (-3.0, 2.0), (-1000.0, 1000.0)):
            np.testing.assert_allclose(RT.sample(tex, 0.3 + du, 0.7 + dv, filter, "repeat")[0], base, rtol=1e-9)
        assert np.array_equal(RT.sample(tex, 1e300, -1e300, filter, "clamp")[0], c(2, 0))
        assert np.array_equal(RT.sample(tex, 7.5e8, 0.25, filter, "clamp")[0], c(2, 0))
    # a coordinate that is no number takes GL texel (0, 0), whatever the other one is
    for filter in RT.FILTERS:
        for wrap in RT.WRAPS:
            for u, v in ((np.nan, 0.9), (0.9, np.inf), (-np.inf, np.nan), (1e308, 0.9)):
                assert np.array_equal(RT.sample(tex, u, v, filter, wrap)[0], c(0, 0)), (filter, wrap, u, v)
    # a 1 x 1 texture is one colour everywhere
    one = np.array([[[255, 0, 51]]], np.uint8)
    for filter in RT.FILTERS:
        for wrap in RT.WRAPS:
            np.testing.assert_allclose(RT.sample(one, [-0.3, 0.5, 7.2], [0.1, 2.5, -4.0], filter, wrap), np.tile([1.0, 0.0, 0.2], (3, 1)), rtol=RTOL)


def test_c_uv_is_interpolated_perspective_correctly():
    m = tilted_plane()                                                 # Z = 300 + 4 X, corners at u = -100 and 150
    A = np.array([[2e-3, 0.0, 5e-4], [-1e-3, 3e-3, 2e-4]])
    uv = m["pts"] @ A.T + np.array([0.4, 0.3])                         # affine in the surface point: what perspective-correct means
    _, ids = RR.render_ids(m["pts"], m["faces"], K, EYE, ORIGIN, W, H)
    assert np.all(ids >= 0)
    got = RT.interp_uv(m["pts"], m["faces"], uv, K, EYE, ORIGIN, ids)
    a, b = rays(K)
    Z = 300.0 / (1.0 - 4.0 * a)
    hit = np.stack([a * Z, b * Z, Z], axis=-1)
    want = hit @ A.T + np.array([0.4, 0.3])
    np.testing.assert_allclose(got, want, rtol=1e-11)
    # the midpoint of the tilted top edge on the screen (column 25 is u = 25.5, the edge runs from -100 to 150): the
    # perspective-correct coordinate is far from the screen-space mean of the two corners
    mid_u = 0.5 * (uv[0, 0] + uv[1, 0])                               # (u does not depend on Y here)
    assert abs(got[0, 25, 0] - want[0, 25, 0]) < 1e-12 and abs(got[0, 25, 0] - mid_u) > 0.1
    # and the texture follows it: a wide two-texel texture read with nearest flips where the correct u crosses a texel edge
    tex = np.array([[[255, 255, 255], [0, 0, 0]]], np.uint8)
    rgb, _ = RT.shade_rgb_tex(m["pts"], m["faces"], uv, tex, None, K, EYE, ORIGIN, ids, "nearest", "repeat", "flat", 1.0, dtype=np.float64)
    dark = (np.floor(want[..., 0] * 2.0) % 2) == 1
    edge = np.abs(want[..., 0] * 2.0 - np.round(want[..., 0] * 2.0)) < 1e-9
    assert 100 < dark.sum() < dark.size - 100
    assert np.array_equal(rgb[..., 0][~edge], np.where(dark, 0.0, 1.0)[~edge])


def analytic_square():
    """the fronto-parallel square whose corners project onto pixel edges: columns 44 ... 84, rows 32 ... 64 at Z = 500"""
    return centred_square(K, 500.0, 20.0, 16.0)


def test_d_the_analytic_scene_shows_the_texture_texel_for_pixel():
    """the unit square of UVs over 40 x 32 pixels with a 40 x 32 texture: pixel centres are texel centres.  v = 0 at the top
    of the square shows the image upside down (v = 0 is its bottom row); v = 1 at the top shows it as it is stored."""
    m = analytic_square()
    rng = np.random.default_rng(11)
    tex = rng.integers(0, 256, size=(32, 40, 3)).astype(np.uint8)
    _, ids = RR.render_ids(m["pts"], m["faces"], K, EYE, ORIGIN, W, H, 10.0, 10000.0)
    inside = np.zeros((H, W), bool)
    inside[32:64, 44:84] = True
    assert np.array_equal(ids >= 0, inside)
    for uv, want in ((UNIT_UV, tex[::-1]), (UNIT_UV * [1.0, -1.0] + [0.0, 1.0], tex)):
        for filter in RT.FILTERS:
            for wrap in RT.WRAPS:
                f32, u8 = RT.shade_rgb_tex(m["pts"], m["faces"], uv, tex, None, K, EYE, ORIGIN, ids, filter, wrap, "flat", 1.0)
                assert np.array_equal(u8[32:64, 44:84], want), (filter, wrap)
                assert not u8[~inside].any()
                if filter == "nearest":
                    assert np.array_equal(f32[32:64, 44:84], (want.astype(np.float64) / 255.0).astype(np.float32))
    # UVs (0, 0) ... (2, 2) with a 20 x 16 texture, so that pixel centres stay texel centres: repeat shows the texture twice in
    # each direction, clamp shows it once and smears its last column and its last GL row (the file's first)
    tex2 = rng.integers(0, 256, size=(16, 20, 3)).astype(np.uint8)
    up = tex2[::-1]
    for filter in RT.FILTERS:
        _, rep = RT.shade_rgb_tex(m["pts"], m["faces"], UNIT_UV * 2.0, tex2, None, K, EYE, ORIGIN, ids, filter, "repeat", "flat", 1.0)
        assert np.array_equal(rep[32:64, 44:84], np.tile(up, (2, 2, 1))), filter
        _, cl = RT.shade_rgb_tex(m["pts"], m["faces"], UNIT_UV * 2.0, tex2, None, K, EYE, ORIGIN, ids, filter, "clamp", "flat", 1.0)
        assert np.array_equal(cl[32:64, 44:84], clamped_twice(tex2)), filter


def clamped_twice(tex2):
    """what UVs (0, 0) ... (2, 2), v = 0 at the top, show of a texture under clamp, texel for pixel"""
    up = tex2[::-1]
    h, w = up.shape[:2]
    out = np.empty((2 * h, 2 * w, 3), np.uint8)
    out[:h, :w] = up
    out[:h, w:] = up[:, -1:]
    out[h:, :w] = up[-1:]
    out[h:, w:] = up[-1, -1]
    return out


def test_e_lighting_multiplies_the_texel():
    m = analytic_square()
    tex = np.random.default_rng(12).integers(0, 256, size=(32, 40, 3)).astype(np.uint8)
    _, ids = RR.render_ids(m["pts"], m["faces"], K, EYE, ORIGIN, W, H, 10.0, 10000.0)
    away = np.tile([0.0, 0.0, 1.0], (4, 1))                            # phong normals facing away: ambient light only
    f32, _ = RT.shade_rgb_tex(m["pts"], m["faces"], UNIT_UV, tex, away, K, EYE, ORIGIN, ids, "nearest", "clamp", "phong", 0.5)
    assert np.array_equal(f32[32:64, 44:84], (0.5 * (tex[::-1].astype(np.float64) / 255.0)).astype(np.float32))
    # the light factor is the one the vertex-colour restatement applies to a constant colour
    c = np.array([1.0, 0.5, 0.25])
    for shading, normals in (("flat", None), ("phong", np.tile([0.3, -0.2, -1.0], (4, 1)))):
        kw = dict(shading=shading, ambient_weight=0.0, light=(200.0, -100.0, 0.0))
        ref, _ = RR.shade_rgb(m["pts"], m["faces"], np.tile(c, (4, 1)), normals, K, EYE, ORIGIN, ids, dtype=np.float64, **kw)
        one = np.full((1, 1, 3), 255, np.uint8)
        got, _ = RT.shade_rgb_tex(m["pts"], m["faces"], UNIT_UV, one, normals, K, EYE, ORIGIN, ids, "bilinear", "repeat", dtype=np.float64, **kw)
        np.testing.assert_allclose(got[ids >= 0] * c, ref[ids >= 0], rtol=RTOL)
        assert got[ids >= 0].min() > 0.2 and got[ids >= 0].std() > 1e-4


PLY = """ply
format ascii 1.0
comment made by hand
%selement vertex 3
property float x
property float y
property float z
property float texture_u
property float texture_v
element face 1
property list uchar int vertex_indices
end_header
0 0 0 0 0
1 0 0 1 0
0 1 0 0 1
3 0 1 2
"""


def test_f_load_ply_reads_the_texture_beside_the_file(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from pyrapose_amd.utils.ply_loader import load_ply
    image = np.random.default_rng(13).integers(0, 256, size=(5, 7, 3)).astype(np.uint8)
    Image.fromarray(image).save(str(tmp_path / "obj_000001.png"))
    path = tmp_path / "obj_000001.ply"
    path.write_text(PLY % "comment TextureFile obj_000001.png\n")
    plain = load_ply(str(path))
    assert sorted(plain) == ["faces", "pts", "texture_uv"]             # the default is what it was: no texture keys
    assert np.array_equal(plain["texture_uv"], [[0, 0], [1, 0], [0, 1]]) and plain["pts"].dtype == np.float64
    m = load_ply(str(path), texture=True)
    assert sorted(m) == ["faces", "pts", "texture", "texture_file", "texture_uv"] and m["texture_file"] == "obj_000001.png"
    assert m["texture"].dtype == np.uint8 and np.array_equal(m["texture"], image)
    for k in plain:
        assert np.array_equal(plain[k], m[k])
    # an RGBA image is read as RGB
    Image.fromarray(np.concatenate([image, np.full((5, 7, 1), 9, np.uint8)], axis=2)).save(str(tmp_path / "rgba.png"))
    path.write_text(PLY % "comment TextureFile rgba.png\n")
    assert np.array_equal(load_ply(str(path), texture=True)["texture"], image)
    # no comment, or a file that is not there
    bare = tmp_path / "bare.ply"
    bare.write_text(PLY % "")
    assert sorted(load_ply(str(bare))) == ["faces", "pts", "texture_uv"]
    with pytest.raises(ValueError, match="TextureFile"):
        load_ply(str(bare), texture=True)
    path.write_text(PLY % "comment TextureFile missing.png\n")
    with pytest.raises(ValueError, match="missing.png"):
        load_ply(str(path), texture=True)
    assert sorted(load_ply(str(path))) == ["faces", "pts", "texture_uv"]


def test_g_texture_images_are_padded_exactly_or_refused():
    """the host conversion of utils.renderer up to the copy to the device: checked through its refusals here (no GPU)"""
    from pyrapose_amd.utils.renderer import texture_rgbx
    for bad in (np.zeros((4, 5), np.uint8), np.zeros((4, 5, 2), np.uint8), np.zeros((4, 5, 3), np.int32), np.zeros((0, 5, 3), np.uint8),
                np.full((4, 5, 3), 0.5), np.full((4, 5, 3), 1.5), np.full((4, 5, 3), np.nan), np.full((4, 5, 3), 0.5, np.float32)):
        with pytest.raises(ValueError):
            texture_rgbx(bad)


def test_h_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "pyrapose_hip.h")).read()
    declared = set(re.findall(r"\b(pp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    from pyrapose_amd import _lib
    for name in TEX_ENTRIES:
        assert name in declared and name in _lib.EXPORTS, name
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = set(line.split()[-1] for line in syms.splitlines() if line.strip())
    else:
        raw = ctypes.CDLL(_lib.LIB_PATH)
        exported = set(n for n in TEX_ENTRIES if hasattr(raw, n))
    for name in TEX_ENTRIES:
        assert name in exported, name
    assert "textures are not rendered" not in src
    # the shape rule needs no device: 0 bytes refuses the texture
    ws = _lib.lib.pp_render_rgbd_tex_workspace_bytes
    assert ws(4, 10, 5, 128, 96, 0, 23) == 0 and ws(4, 10, 5, 128, 96, 20000, 23) == 0 and ws(4, 10, 5, 128, 96, 37, 0) == 0
    assert ws(4, 10, 5, 128, 96, 16384, 16384) == ws(4, 10, 5, 128, 96, 37, 23) == _lib.lib.pp_render_rgbd_workspace_bytes(4, 10, 5, 128, 96) > 0
    assert ws(4, 10, 5, 128, 96, 16384, 16384 + 1) == 0 and ws(0, 10, 5, 128, 96, 37, 23) == 0
