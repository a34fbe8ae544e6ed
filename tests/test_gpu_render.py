"""GPU: the depth renderer pp_render_depth_f32 (csrc/render.hip) against the numpy restatement (tests/render_np.py) and
analytic scenes: half-pixel convention, perspective-correct depth, nearest surface, clipping, determinism, bad arguments."""
import numpy as np
import pytest
import torch

from tests import render_np as RN

pytestmark = pytest.mark.gpu
W, H = 128, 96
K = np.array([[500.0, 0.0, 64.0], [0.0, 480.0, 48.0], [0.0, 0.0, 1.0]])


def rot(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def render(model, R, t, K=K, w=W, h=H, near=100.0, far=10000.0):
    from pyrapose_amd.utils.renderer import render_depth_batch
    return render_depth_batch(model, (w, h), K, np.asarray(R).reshape(-1, 3, 3), np.asarray(t).reshape(-1, 3), near, far).cpu().numpy()


def quad(corners):
    """two triangles over four camera-frame corners given in order round the quad"""
    return {"pts": np.asarray(corners, np.float64), "faces": np.array([[0, 1, 2], [0, 2, 3]])}


def unproject(u, v, Z, K=K):
    return [(u - K[0, 2]) * Z / K[0, 0], (v - K[1, 2]) * Z / K[1, 1], Z]


def test_fronto_parallel_square_pins_the_half_pixel_convention():
    Z = 500.0
    u0, u1, v0, v1 = 10.25, 40.75, 20.25, 50.75
    m = quad([unproject(u0, v0, Z), unproject(u1, v0, Z), unproject(u1, v1, Z), unproject(u0, v1, Z)])
    d = render(m, np.eye(3), np.zeros(3))[0]
    cc, rr = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    inside = (cc > u0) & (cc < u1) & (rr > v0) & (rr < v1)       # pixel (r, c) samples (c + 0.5, r + 0.5)
    assert inside.sum() == 31 * 31
    assert np.array_equal(d > 0, inside)
    assert np.all(d[inside] == np.float32(Z))
    # the diagonal shared by the two triangles is drawn once, with no gap
    assert np.array_equal(d, RN.render_depth(m["pts"], m["faces"], K, np.eye(3), np.zeros(3), W, H))


def test_tilted_plane_is_perspective_correct():
    # plane Z = 300 + 4 X (strongly tilted), corners far outside the image so every pixel samples it
    corners = []
    for (u, v) in ((-100.0, -50.0), (150.0, -50.0), (150.0, 150.0), (-100.0, 150.0)):
        a = (u - K[0, 2]) / K[0, 0]
        Z = 300.0 / (1.0 - 4.0 * a)
        corners.append([a * Z, (v - K[1, 2]) / K[1, 1] * Z, Z])
    assert all(c[2] > 0 for c in corners)
    d = render(quad(corners), np.eye(3), np.zeros(3))[0]
    cc, rr = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    want = 300.0 / (1.0 - 4.0 * (cc - K[0, 2]) / K[0, 0])            # ray-plane depth
    assert np.all(d > 0)
    np.testing.assert_allclose(d, want, rtol=1e-5)
    # linear (screen-space) interpolation of Z would be off by far more than that here
    assert np.abs(d / want - 1).max() < 1e-5


def test_cube_front_face_wins():
    m = RN.box_mesh(100.0, 100.0, 100.0)
    for R in (np.eye(3), np.diag([1.0, -1.0, -1.0])):          # both windings of the front face
        d = render(m, R, [0.0, 0.0, 500.0])[0]
        assert np.all(d[40:56, 56:72] == np.float32(450.0))
        assert d.max() <= 450.0 + 1e-3 and d[d > 0].min() >= 450.0 - 1e-3


def test_clipping_behind_camera_and_empty():
    Z = 500.0
    m = quad([unproject(5.2, 5.2, Z), unproject(100.7, 5.2, Z), unproject(100.7, 80.7, Z), unproject(5.2, 80.7, Z)])
    assert (render(m, np.eye(3), np.zeros(3), near=499.0, far=501.0)[0] > 0).sum() == 96 * 76
    assert not render(m, np.eye(3), np.zeros(3), near=501.0, far=10000.0).any()
    assert not render(m, np.eye(3), np.zeros(3), near=100.0, far=499.0).any()
    # a slanted quad from Z = 300 to 900 cut by the near plane at 600: only what lies at Z >= 600 stays
    tilt = quad([[-100, -60, 300], [100, -60, 900], [100, 60, 900], [-100, 60, 300]])
    d = render(tilt, np.eye(3), np.zeros(3), near=600.0)[0]
    full = render(tilt, np.eye(3), np.zeros(3))[0]
    assert d.any() and (d[d > 0] >= 600.0).all() and np.array_equal(d > 0, full >= 600.0)
    # a vertex behind the camera skips the triangle (not clipped)
    behind = {"pts": np.array([[-50.0, -50.0, 500.0], [50.0, -50.0, 500.0], [0.0, 50.0, -10.0]]), "faces": np.array([[0, 1, 2]])}
    assert not render(behind, np.eye(3), np.zeros(3)).any()
    # off-screen pose and an object beyond the far plane: all zeros
    sph = RN.sphere_mesh(30.0, 6, 8)
    assert not render(sph, np.eye(3), [5000.0, 0.0, 500.0]).any()
    assert not render(sph, np.eye(3), [0.0, 0.0, 20000.0]).any()


def test_matches_numpy_restatement():
    rng = np.random.default_rng(7)
    m = RN.sphere_mesh(40.0, 12, 18, scale=(1.0, 0.6, 0.8))
    m["pts"] = m["pts"] + rng.normal(scale=1.5, size=m["pts"].shape)   # irregular, non-convex surface
    Rs = [rot(rng) for _ in range(4)]
    ts = [[rng.uniform(-20, 20), rng.uniform(-15, 15), rng.uniform(250, 600)] for _ in range(4)]
    ts[3] = [10.0, -5.0, 70.0]                                           # close-up: triangles far larger than a tile
    got = render(m, Rs, ts, near=10.0)
    for i in range(4):
        want = RN.render_depth(m["pts"], m["faces"], K, Rs[i], ts[i], W, H, 10.0, 10000.0)
        assert (want > 0).sum() > 200
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (i, int((got[i] != want).sum()))   # coverage and depth, every pixel


def test_full_size_batch_is_deterministic_and_equals_single_calls():
    rng = np.random.default_rng(11)
    m = RN.sphere_mesh(50.0, 24, 40)
    Kl = np.array([[1075.65, 0.0, 360.0], [0.0, 1073.9, 270.0], [0.0, 0.0, 1.0]])
    Rs = np.stack([rot(rng) for _ in range(5)])
    ts = np.stack([[rng.uniform(-80, 80), rng.uniform(-60, 60), rng.uniform(300, 900)] for _ in range(5)])
    a = render(m, Rs, ts, K=Kl, w=720, h=540)
    b = render(m, Rs, ts, K=Kl, w=720, h=540)
    assert a.shape == (5, 540, 720) and (a > 0).sum() > 10000
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for i in range(5):
        assert np.array_equal(render(m, Rs[i], ts[i], K=Kl, w=720, h=540)[0].view(np.uint32), a[i].view(np.uint32))
    # an odd image width: the right-hand tiles take the scalar stores
    Ko = np.array([[1075.65, 0.0, 166.0], [0.0, 1073.9, 125.0], [0.0, 0.0, 1.0]])
    c = render(m, Rs[0], ts[0], K=Ko, w=333, h=251)[0]
    want = RN.render_depth(m["pts"], m["faces"], Ko, Rs[0], ts[0], 333, 251)
    assert (want > 0).sum() > 1000
    assert np.array_equal(c.view(np.uint32), want.view(np.uint32)), int((c != want).sum())


def test_render_signature_and_bad_arguments():
    from pyrapose_amd import ops
    from pyrapose_amd.runtime import default_context
    from pyrapose_amd.utils.renderer import render as render_one
    m = RN.box_mesh(100.0, 100.0, 100.0)
    d = render_one(m, (W, H), K, np.eye(3), np.array([[0.0], [0.0], [500.0]]), clip_near=100, clip_far=10000, mode="depth")
    assert d.shape == (H, W) and d.dtype == np.float32 and d.max() == np.float32(450.0)
    with pytest.raises(ValueError):
        render_one(m, (W, H), K, np.eye(3), [0, 0, 500], mode="rgb")
    with pytest.raises(ValueError):
        render_one({"pts": m["pts"], "faces": np.array([[0, 1, 8]])}, (W, H), K, np.eye(3), [0, 0, 500])
    with pytest.raises(ValueError):
        render_one({"pts": m["pts"][:, :2], "faces": m["faces"]}, (W, H), K, np.eye(3), [0, 0, 500])
    ctx = default_context()
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.asarray(a), dtype=dt).cuda()
    args = (dev(m["pts"]), dev(m["faces"], torch.int32), dev(np.eye(3)[None]), dev([[0.0, 0.0, 500.0]]), dev([[500.0, 480.0, 64.0, 48.0]]))
    with pytest.raises(ValueError):
        ops.render_depth(ctx, *args, 0, H)
    with pytest.raises(ValueError):
        ops.render_depth(ctx, *args, W, H, clip_near=500.0, clip_far=100.0)
