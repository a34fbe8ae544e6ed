"""CPU: the numpy restatement of the colour renderer (tests/render_rgb_np.py) against closed forms, so that the device can be
compared with the restatement alone.  Corners sit on quarter pixels and project exactly, so a closed form holds to float64
rounding: 1e-12 relative, a few dozen operations at 1.1e-16 each.  Colours are looked at before their rounding to float32
(dtype=np.float64) and, where the expected value is exact, after it."""
import numpy as np

from tests import render_rgb_np as RR
from tests import scene_gt_np as SN

W, H = 128, 96
K = np.array([[500.0, 0.0, 64.0], [0.0, 480.0, 48.0], [0.0, 0.0, 1.0]])
KWIDE = np.array([[32.0, 0.0, 64.0], [0.0, 32.0, 48.0], [0.0, 0.0, 1.0]])   # 63 degrees to the image's left and right edges
EYE, ORIGIN = np.eye(3), np.zeros(3)
RTOL = 1e-12


def centred_square(K, Z, du=20.25, dv=15.75):
    """fronto-parallel, centred on the principal point: its corners are equally far from the camera"""
    cx, cy = K[0, 2], K[1, 2]
    return RR.quad([RR.unproject(cx - du, cy - dv, Z, K), RR.unproject(cx + du, cy - dv, Z, K), RR.unproject(cx + du, cy + dv, Z, K),
                    RR.unproject(cx - du, cy + dv, Z, K)])


def rays(K):
    cc, rr = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    return (cc - K[0, 2]) / K[0, 0], (rr - K[1, 2]) / K[1, 1]


def shade(m, colors, ids, K=K, normals=None, dtype=np.float64, **kw):
    return RR.shade_rgb(m["pts"], m["faces"], colors, normals, K, EYE, ORIGIN, ids, dtype=dtype, **kw)


def test_a_flat_square_lit_from_the_camera():
    c = np.array([0.9, 0.5, 0.3])
    for Kc, Z, some_unclamped in ((K, 500.0, False), (KWIDE, 512.0, True)):
        m = centred_square(Kc, Z, 40.25, 30.75)
        depth, ids = RR.render_ids(m["pts"], m["faces"], Kc, EYE, ORIGIN, W, H)
        assert (ids >= 0).sum() == 80 * 62 and np.array_equal(ids >= 0, depth > 0) and np.all(depth[ids >= 0] == np.float32(Z))
        got, _ = shade(m, np.tile(c, (4, 1)), ids, Kc, shading="flat", ambient_weight=0.2)
        a, b = rays(Kc)
        cos = 1.0 / np.sqrt(a * a + b * b + 1.0)                  # Z / |P| of the point on the pixel-centre ray
        want = np.minimum(0.2 + cos, 1.0)[..., None] * c
        inside = ids >= 0
        np.testing.assert_allclose(got[inside], want[inside], rtol=RTOL)
        assert ((0.2 + cos[inside] < 1.0).sum() > 500) == some_unclamped
        assert np.all(got[~inside] == 0.0)


def tilted_plane():
    corners = []
    for (u, v) in ((-100.0, -50.0), (150.0, -50.0), (150.0, 150.0), (-100.0, 150.0)):
        a = (u - K[0, 2]) / K[0, 0]
        Z = 300.0 / (1.0 - 4.0 * a)                                # the plane Z = 300 + 4 X
        corners.append([a * Z, (v - K[1, 2]) / K[1, 1] * Z, Z])
    return RR.quad(corners)


def test_b_colours_are_interpolated_perspective_correctly():
    m = tilted_plane()
    A = np.array([[4e-4, 1e-3, 2e-4], [-3e-4, 5e-4, 1e-4], [1e-4, -2e-3, -1e-4]])
    c0 = np.array([0.45, 0.5, 0.55])
    colors = m["pts"] @ A.T + c0
    assert colors.min() > 0.0 and colors.max() < 1.0
    depth, ids = RR.render_ids(m["pts"], m["faces"], K, EYE, ORIGIN, W, H)
    assert np.all(ids >= 0)
    got, _ = shade(m, colors, ids, shading="flat", ambient_weight=1.0)
    a, b = rays(K)
    Z = 300.0 / (1.0 - 4.0 * a)
    hit = np.stack([a * Z, b * Z, Z], axis=-1)
    want = hit @ A.T + c0
    np.testing.assert_allclose(got, want, rtol=RTOL)
    np.testing.assert_allclose(depth, Z, rtol=1e-6)
    # screen-linear interpolation of the corner colours is far off on this plane
    u = (np.arange(W) + 0.5 + 100.0) / 250.0
    linear = colors[0][None, :] + u[:, None] * (colors[1] - colors[0])[None, :]
    assert np.abs(linear[None, :, 0] - want[:, :, 0]).max() > 0.05


def test_c_flat_shading_does_not_depend_on_the_winding():
    m = centred_square(KWIDE, 512.0, 40.25, 30.75)
    rng = np.random.default_rng(3)
    colors = rng.uniform(size=(4, 3))
    kw = dict(shading="flat", ambient_weight=0.2, light=(200.0, -100.0, 0.0))
    _, ids = RR.render_ids(m["pts"], m["faces"], KWIDE, EYE, ORIGIN, W, H)
    a, _ = shade(m, colors, ids, KWIDE, **kw)
    rev = {"pts": m["pts"], "faces": m["faces"][:, ::-1].copy()}
    _, ids_rev = RR.render_ids(rev["pts"], rev["faces"], KWIDE, EYE, ORIGIN, W, H)
    b, _ = shade(rev, colors, ids_rev, KWIDE, **kw)
    assert np.array_equal(ids, ids_rev) and (ids >= 0).sum() == 80 * 62
    np.testing.assert_allclose(a, b, rtol=RTOL)
    lit = a[ids >= 0] / RR.shade_rgb(m["pts"], m["faces"], colors, None, KWIDE, EYE, ORIGIN, ids, "flat", 1.0, dtype=np.float64)[0][ids >= 0]
    assert lit.min() > 0.2 + 0.3 and lit.max() <= 1.0              # the diffuse term is there: the normal faces the viewer


def test_d_phong_normals_facing_away_get_ambient_light_only():
    m = centred_square(K, 500.0)
    c = np.array([0.5, 0.25, 0.75])
    away = np.tile([0.0, 0.0, 1.0], (4, 1))
    _, ids = RR.render_ids(m["pts"], m["faces"], K, EYE, ORIGIN, W, H)
    got, _ = shade(m, np.tile(c, (4, 1)), ids, normals=away, shading="phong", ambient_weight=0.5)
    np.testing.assert_allclose(got[ids >= 0], np.broadcast_to(0.5 * c, got[ids >= 0].shape), rtol=RTOL)
    got32, _ = shade(m, np.tile(c, (4, 1)), ids, normals=away, shading="phong", ambient_weight=0.5, dtype=np.float32)
    assert got32.dtype == np.float32 and np.all(got32[ids >= 0] == (0.5 * c).astype(np.float32))
    # towards the camera the same surface is fully lit
    lit, _ = shade(m, np.tile(c, (4, 1)), ids, normals=-away, shading="phong", ambient_weight=0.5)
    np.testing.assert_allclose(lit[ids >= 0], np.broadcast_to(c, lit[ids >= 0].shape), rtol=RTOL)


def test_e_full_ambient_light_gives_the_colour_and_its_rounded_bytes():
    m = centred_square(K, 500.0)
    c = np.array([0.2, 0.6, 1.0])
    _, ids = RR.render_ids(m["pts"], m["faces"], K, EYE, ORIGIN, W, H)
    for shading, normals in (("flat", None), ("phong", np.tile([0.3, -0.2, -1.0], (4, 1)))):
        f32, u8 = shade(m, np.tile(c, (4, 1)), ids, normals=normals, shading=shading, ambient_weight=1.0, dtype=np.float32,
                        bg_color=(0.0, 0.5, 1.0))
        assert np.all(f32[ids >= 0] == c.astype(np.float32))
        assert u8.dtype == np.uint8 and np.all(u8[ids >= 0] == np.array([51, 153, 255], np.uint8))
        assert np.all(f32[ids < 0] == np.array([0.0, 0.5, 1.0], np.float32)) and np.all(u8[ids < 0] == np.array([0, 128, 255], np.uint8))


def test_f_a_duplicated_face_shows_the_smaller_index():
    pts = np.array([RR.unproject(10.25, 10.25, 500.0, K), RR.unproject(90.75, 20.25, 500.0, K), RR.unproject(40.25, 80.75, 650.0, K)])
    for faces in ([[0, 1, 2], [0, 1, 2]], [[2, 1, 0], [2, 1, 0]]):
        depth, ids = RR.render_ids(pts, np.array(faces), K, EYE, ORIGIN, W, H)
        assert (depth > 0).sum() > 1000 and np.all(ids[depth > 0] == 0) and np.all(ids[depth == 0] == -1)
    # the nearer triangle wins whatever its index
    far = pts + np.array([0.0, 0.0, 100.0])
    for order in ((0, 1), (1, 0)):
        both = np.concatenate([pts, far])
        faces = np.array([[0, 1, 2], [3, 4, 5]])[list(order)]
        depth, ids = RR.render_ids(both, faces, K, EYE, ORIGIN, W, H)
        near_index = order.index(0)
        one, _ = RR.render_ids(pts, np.array([[0, 1, 2]]), K, EYE, ORIGIN, W, H)
        assert np.all(ids[one > 0] == near_index) and np.array_equal(depth[one > 0], one[one > 0])


def test_g_compose_selects_instance_colours_and_backgrounds():
    rng = np.random.default_rng(5)
    h, w = 5, 7
    # scene 0: instances 0 and 1 at the same depth on two pixels (the later one shows), 1 alone on a third; scene 1: empty;
    # scene 2: instance 2
    stack = np.zeros((3, h, w), np.float32)
    stack[0, 1, 1:3] = 400.0
    stack[1, 1, 1:4] = 400.0
    stack[0, 3, 5] = 500.0
    stack[2, 2, 2:6] = 450.0
    offsets = np.array([0, 2, 2, 3], np.int32)
    ids = SN.scene_gt(stack, offsets, K, None, 15.0)["id_image"]
    assert ids[0, 1].tolist() == [0, 2, 2, 2, 0, 0, 0] and ids[0, 3, 5] == 1 and not ids[1].any() and ids[2, 2].tolist() == [0, 0, 1, 1, 1, 1, 0]
    colors = rng.integers(0, 256, size=(3, h, w, 3)).astype(np.uint8)
    bg_image = rng.integers(0, 256, size=(3, h, w, 3)).astype(np.uint8)
    for bg in (bg_image, (10, 20, 30)):
        rgb = RR.compose(ids, colors, offsets, bg, "rgb")
        assert rgb.dtype == np.uint8 and rgb.shape == (3, h, w, 3)
        for s in range(3):
            for r in range(h):
                for c in range(w):
                    k = ids[s, r, c]
                    want = colors[offsets[s] + k - 1, r, c] if k else (bg_image[s, r, c] if bg is bg_image else np.array(bg, np.uint8))
                    assert np.array_equal(rgb[s, r, c], want)
        assert np.array_equal(RR.compose(ids, colors, offsets, bg, "bgr"), rgb[..., ::-1])
