"""Scenes that reach the control-flow edges of the tiled rasteriser (csrc/render.hip, render_raster_tile.inc), and a host census
of the binning decisions that says which edges a scene reaches (test infrastructure; no GPU, no torch).
tests/test_render_cases_cpu.py asserts every scene's claim, tests/test_gpu_render_edges.py compares the device with the
restatement tests/render_rgb_np.py bit for bit on them.  A scene is a dict: pts [n_v,3], faces [n_f,3], K 3x3, R [n,3,3],
t [n,3], w, h, near, far.  Screen positions are given as (u, v, Z) and unprojected, so vertices sit where a scene says."""
import numpy as np

from tests import render_np as RN
from tests.render_np import project
from tests.render_rgb_np import _setup, render_ids, unproject

# csrc/render.hip and csrc/pose_common.h
RT = 32                 # screen tile edge (pixels)
RASTER_THREADS = 256    # entries of a tile's list, and of the pose's big list, taken per chunk
RASTER_SMALL_PX = 64    # a larger per-tile box goes through the workgroup's queue
BIN_MAX_TILES = 4       # a triangle on more tiles goes to the pose's big list
SCAN_THREADS = 1024     # (pose, tile) bins the one-workgroup scan takes per chunk

EYE, ORIGIN = np.eye(3), np.zeros(3)


def pixel_box(V, w, h):
    """setup_triangle's pixel box (c0, c1, r0, r1), inclusive and clamped to the image, or None when it is empty"""
    xs, ys = [float(v[0]) for v in V], [float(v[1]) for v in V]
    c0 = max(int(np.ceil(min(max(min(xs) - 0.5, -1.0), float(w)))), 0)
    c1 = min(int(np.floor(min(max(max(xs) - 0.5, -1.0), float(w)))), w - 1)
    r0 = max(int(np.ceil(min(max(min(ys) - 0.5, -1.0), float(h)))), 0)
    r1 = min(int(np.floor(min(max(max(ys) - 0.5, -1.0), float(h)))), h - 1)
    return None if c0 > c1 or r0 > r1 else (c0, c1, r0, r1)


def census(pts, faces, K, R, t, w, h):
    """The binning of one pose as setup_triangle, render_bin_kernel and render_raster_tile.inc decide it -> dict:
      drawn      indices of the triangles that pass setup_triangle (valid indices, every Z > 0, an area, a box on the image)
      big        those on more than BIN_MAX_TILES tiles: the pose's big list (every one is queued in every tile it touches)
      tiles      {triangle: number of tiles its box touches} for the drawn ones
      list_len   [tiles_y, tiles_x] length of each tile's list
      entries    per list entry (triangle, tile row, tile column, pixels of the box clipped to the tile, queued) with
                 queued = pixels > RASTER_SMALL_PX: the workgroup's queue, otherwise the thread's own loop
      n_tiles    (pose, tile) bins of this pose"""
    x, y, iz = project(pts, np.asarray(K, np.float64), R, t)
    tiles_x, tiles_y = (w + RT - 1) // RT, (h + RT - 1) // RT
    out = {"drawn": [], "big": [], "tiles": {}, "list_len": np.zeros((tiles_y, tiles_x), np.int64), "entries": [],
           "n_tiles": tiles_x * tiles_y}
    for tri, f in enumerate(np.asarray(faces, np.int64)):
        T = _setup(x, y, iz, f)
        box = pixel_box(T[0], w, h) if T is not None else None
        if box is None:
            continue
        c0, c1, r0, r1 = box
        tc0, tc1, tr0, tr1 = c0 // RT, c1 // RT, r0 // RT, r1 // RT
        out["drawn"].append(tri)
        out["tiles"][tri] = (tc1 - tc0 + 1) * (tr1 - tr0 + 1)
        if out["tiles"][tri] > BIN_MAX_TILES:
            out["big"].append(tri)
            continue
        for ty in range(tr0, tr1 + 1):
            for tx in range(tc0, tc1 + 1):
                a0, a1 = max(c0, tx * RT), min(c1, tx * RT + RT - 1)
                b0, b1 = max(r0, ty * RT), min(r1, ty * RT + RT - 1)
                area = (a1 - a0 + 1) * (b1 - b0 + 1)
                out["list_len"][ty, tx] += 1
                out["entries"].append((tri, ty, tx, area, area > RASTER_SMALL_PX))
    return out


def n_bins(scene):
    return len(scene["R"]) * ((scene["w"] + RT - 1) // RT) * ((scene["h"] + RT - 1) // RT)


def make(pts, faces, K, w, h, R=EYE, t=ORIGIN, near=10.0, far=10000.0):
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    return {"pts": np.asarray(pts, np.float64), "faces": np.asarray(faces, np.int64), "K": np.asarray(K, np.float64), "R": R,
            "t": np.asarray(t, np.float64).reshape(len(R), 3), "w": w, "h": h, "near": float(near), "far": float(far)}


def soup(tris, K):
    """triangles given as three screen points (u, v, Z) each, no shared vertices -> pts [3 n,3], faces [n,3]"""
    pts = [unproject(u, v, Z, K) for tri in tris for (u, v, Z) in tri]
    return np.array(pts, np.float64), np.arange(len(pts)).reshape(-1, 3)


def box_tri(c0, r0, bw, bh, Z):
    """a right triangle whose pixel box is exactly columns c0 .. c0 + bw - 1, rows r0 .. r0 + bh - 1"""
    return [(c0 + 0.25, r0 + 0.25, Z), (c0 + bw + 0.25, r0 + 0.25, Z), (c0 + 0.25, r0 + bh + 0.25, Z)]


def camera(w, h, f=150.0):
    return np.array([[f, 0.0, w / 2 + 0.3], [0.0, f, h / 2 - 0.2], [0.0, 0.0, 1.0]])


# ---- A: a tile list longer than one chunk -------------------------------------------------------------------------------------
def grid(nx, ny, x0, x1, y0, y1, K, seed):
    """nx x ny quads (2 nx ny triangles) over the screen rectangle, the inner vertices jittered by 0.3 of the spacing, every
    vertex at a depth of its own in 400 .. 600"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1))
    u = u + rng.uniform(-0.3, 0.3, u.shape) * (x1 - x0) / nx
    v = v + rng.uniform(-0.3, 0.3, v.shape) * (y1 - y0) / ny
    Z = rng.uniform(400.0, 600.0, u.shape)
    pts = [unproject(a, b, z, K) for a, b, z in zip(u.ravel(), v.ravel(), Z.ravel())]
    faces = []
    for j in range(ny):
        for i in range(nx):
            a = j * (nx + 1) + i
            faces += [[a, a + 1, a + nx + 2], [a, a + nx + 2, a + nx + 1]]
    return np.array(pts), np.array(faces)


def long_list():
    """13 x 13 quads inside tile (0, 0) of 70 x 45: a list of 338 small triangles"""
    K = camera(70, 45)
    return make(*grid(13, 13, 2.0, 30.0, 2.0, 30.0, K, 101), K, 70, 45)


def long_list_on_seams():
    """22 x 20 quads round the corner (32, 32) of four tiles of 70 x 45, running off the bottom of the image"""
    K = camera(70, 45)
    return make(*grid(22, 20, 3.0, 61.0, 1.5, 47.0, K, 102), K, 70, 45)


# ---- B: a big list longer than one chunk --------------------------------------------------------------------------------------
B_TRIS = 320


def long_big_list():
    """320 triangles that cover all or nearly all of 96 x 96 (9 tiles).  Triangle i lies on a plane whose 1 / Z -- affine in
    screen space -- is the tangent at a point p_i of the image to the convex 1e-3 + 5e-10 |p - centre|^2, so the nearest
    surface at a pixel is the triangle whose p_i is closest: every triangle wins a cell of its own, with ties where cells meet."""
    rng = np.random.default_rng(103)
    K = camera(96, 96)
    centre, b = np.array([48.0, 48.0]), 5e-10                         # shallow: float32 depths tie along the cells' borders
    p = rng.uniform(2.0, 94.0, (B_TRIS, 2))
    tris = []
    for i in range(B_TRIS):
        corners = np.array([[-12.0, -12.0], [212.0, -12.0], [-12.0, 212.0]]) + rng.uniform(-20.0, 20.0, (3, 2))
        if i % 2:
            corners = corners[::-1]                                    # both windings
        g = 2.0 * b * (p[i] - centre)
        iz = 1e-3 + b * ((p[i] - centre) ** 2).sum() + (corners - p[i]) @ g
        tris.append([(q[0], q[1], 1.0 / z) for q, z in zip(corners, iz)])
    return make(*soup(tris, K), K, 96, 96)


# ---- C: the small / queued threshold ------------------------------------------------------------------------------------------
C_BOXES = {0: 64, 1: 64, 2: 65, 3: 66}        # triangle -> pixels of its box; triangle 4 straddles the seam at column 32
C_STRADDLER = 4


def small_queued_threshold():
    K = camera(96, 64)
    tris = [box_tri(3, 2, 8, 8, 500.0), box_tri(6, 12, 16, 4, 480.0), box_tri(8, 5, 13, 5, 520.0), box_tri(12, 9, 11, 6, 460.0),
            box_tri(28, 20, 13, 8, 500.0),      # columns 28 .. 40: 4 x 8 pixels in tile (0, 0), 9 x 8 in tile (0, 1)
            box_tri(40, 36, 8, 8, 500.0), box_tri(44, 40, 13, 5, 450.0)]     # the same two sizes in a lower tile, overlapping
    return make(*soup(tris, K), K, 96, 64)


# ---- D: the list / big threshold ----------------------------------------------------------------------------------------------
D_TILES = {0: 4, 1: 4, 2: 4, 3: 5, 4: 5, 5: 6}     # triangle -> tiles its box touches (2x2, 1x4, 4x1, 1x5, 5x1, 2x3)


def list_big_threshold():
    K = camera(160, 160)
    tris = [box_tri(20, 20, 21, 21, 500.0),     # columns and rows 20 .. 40: tiles 0 .. 1 both ways
            box_tri(10, 70, 111, 11, 480.0),    # columns 10 .. 120 (tiles 0 .. 3), rows 70 .. 80 (tile 2)
            box_tri(130, 10, 11, 111, 520.0),   # the same, upright
            box_tri(5, 100, 146, 11, 460.0),    # columns 5 .. 150 (tiles 0 .. 4), rows 100 .. 110 (tile 3)
            box_tri(70, 5, 11, 146, 540.0),     # the same, upright: crosses triangles 1 and 3
            box_tri(40, 120, 61, 21, 440.0)]    # columns 40 .. 100 (tiles 1 .. 3), rows 120 .. 140 (tiles 3 .. 4)
    return make(*soup(tris, K), K, 160, 160)


# ---- E: vertices and edges through pixel centres ------------------------------------------------------------------------------
E_K = np.array([[128.0, 0.0, 0.0], [0.0, 128.0, 0.0], [0.0, 0.0, 1.0]])     # at Z = 128 a vertex's screen position is its (X, Y)
E_RIM = [(0.5, 0.5), (32.5, 0.5), (63.5, 0.5), (63.5, 32.5), (63.5, 63.5), (32.5, 63.5), (0.5, 63.5), (0.5, 32.5)]


def fan(reverse_winding=False, reverse_order=False):
    """8 triangles round the hub (32.5, 32.5), a pixel centre at the corner of the four tiles of 64 x 64, the rim on the lines
    0.5 and 63.5: the spokes run through pixel centres, along rows, columns and diagonals.  All at Z = 128: every fragment ties."""
    pts = [[32.5, 32.5, 128.0]] + [[u, v, 128.0] for u, v in E_RIM]
    faces = np.array([[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)])
    if reverse_winding:
        faces = faces[:, ::-1]
    if reverse_order:
        faces = faces[::-1]
    return make(pts, faces, E_K, 64, 64)


# ---- F: image shapes ----------------------------------------------------------------------------------------------------------
F_SHAPES = [(w, 33) for w in (1, 3, 4, 31, 32, 33, 36, 70)] + [(36, h) for h in (1, 31, 32)]


def ellipsoid():
    """the perturbed ellipsoid of tests/test_gpu_render.py: irregular and non-convex"""
    rng = np.random.default_rng(7)
    m = RN.sphere_mesh(40.0, 12, 18, scale=(1.0, 0.6, 0.8))
    return m["pts"] + rng.normal(scale=1.5, size=m["pts"].shape), m["faces"]


def rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def image_shape(w, h):
    """the ellipsoid at least 44 pixels across, centred or, in a wide image, 20 pixels from the right-hand border: it fills the
    small images and is cut by the right-hand and the bottom border of every one"""
    pts, faces = ellipsoid()
    K = camera(w, h)
    return make(pts, faces, K, w, h, rotation(104), unproject(max(w / 2, w - 20.0) + 0.3, h / 2 - 0.4, 160.0, K))


# ---- G: the scan's second chunk -----------------------------------------------------------------------------------------------
G_POSES = 176                               # x 6 tiles = 1056 bins
G_SEAM = 170                                # its tiles 3 and 4 are bins 1023 and 1024, the last of the scan's first chunk and the next
G_OFF_SCREEN = (3, 100, 168, 174)
G_ALONE = (0, G_SEAM - 1, G_SEAM, G_SEAM + 1, G_POSES - 1)     # first, last, and round bin 1024: also rendered one by one


def scan_carry():
    """a small ellipsoid at 176 translations on 96 x 64; pose 170 sits on the seam of tiles (1, 0) and (1, 1)"""
    m = RN.sphere_mesh(30.0, 4, 6, scale=(1.0, 0.7, 0.85))
    K = camera(96, 64)
    i = np.arange(G_POSES)
    t = np.stack([-70.0 + 140.0 * ((i * 37) % G_POSES) / G_POSES, -40.0 + 80.0 * ((i * 59) % G_POSES) / G_POSES, 280.0 + 0.5 * i], axis=1)
    t[list(G_OFF_SCREEN), 0] = 4000.0
    t[G_SEAM] = unproject(32.0, 48.0, 300.0, K)
    return make(m["pts"], m["faces"], K, 96, 64, np.tile(rotation(105), (G_POSES, 1, 1)), t)


# ---- H: far coordinates -------------------------------------------------------------------------------------------------------
H_FAR = (1, 2, 3)        # drawn: one vertex about 1e6, 1e9, 1e12 pixels off the image
H_SKIPPED = (4, 5, 6)    # a projection beyond float32; a vertex at Z < 0; a vertex at Z = 0


def far_coordinates():
    K = camera(64, 48)
    tris = [box_tri(5, 30, 20, 12, 500.0),
            [(10.25, 4.25, 500.0), (10.25, 12.25, 500.0), (1e6, 8.0, 500.0)],
            [(60.25, 14.25, 450.0), (60.25, 22.25, 450.0), (-1e9, 18.0, 450.0)],
            [(30.25, 2.25, 550.0), (40.25, 2.25, 550.0), (35.0, 1e12, 550.0)],
            [(20.25, 24.25, 400.0), (20.25, 28.25, 400.0), (1e39, 26.0, 400.0)]]
    pts, faces = soup(tris, K)
    behind = [unproject(40.25, 30.25, 500.0, K), unproject(50.25, 30.25, 500.0, K), [0.0, 50.0, -10.0]]
    at_zero = [unproject(40.25, 36.25, 500.0, K), unproject(50.25, 36.25, 500.0, K), [0.0, 0.0, 0.0]]
    return make(np.concatenate([pts, behind, at_zero]), np.concatenate([faces, [[15, 16, 17], [18, 19, 20]]]), K, 64, 48)


# ---- I: faces the host wrappers refuse and the kernels skip --------------------------------------------------------------------
I_GOOD = (0, 3, 6, 8)
I_BAD = (1, 2, 4, 5, 7)


def bad_faces():
    K = camera(70, 45)
    tris = [box_tri(4, 4, 20, 14, 500.0), box_tri(30, 6, 24, 20, 450.0), box_tri(10, 20, 40, 20, 550.0), box_tri(40, 2, 28, 40, 600.0)]
    pts, _ = soup(tris, K)
    n = len(pts) + 3
    line = [unproject(u, 30.25, 400.0, K) for u in (5.25, 25.25, 50.25)]      # three points of one screen row: no area
    pts = np.concatenate([pts, line])
    faces = [[0, 1, 2], [-1, 1, 2], [3, 4, n], [3, 4, 5], [12, 13, 14], [6, 6, 7], [6, 7, 8], [0, n + 5, 1], [9, 10, 11]]
    return make(pts, faces, K, 70, 45)


# ---- J: depth ties and clip equality ------------------------------------------------------------------------------------------
def coplanar_overlap(swap=False):
    """two different triangles of the plane Z = 512 that overlap; with swap, in the other index order"""
    K = np.array([[128.0, 0.0, 32.0], [0.0, 128.0, 24.0], [0.0, 0.0, 1.0]])
    tris = [[(4.25, 4.25, 512.0), (50.25, 8.25, 512.0), (10.25, 40.25, 512.0)], [(58.75, 44.75, 512.0), (6.75, 30.75, 512.0), (44.75, 2.75, 512.0)]]
    return make(*soup(tris[::-1] if swap else tris, K), K, 64, 48)


J_NEAR, J_FAR = 128.0, 8192.0       # powers of two: 1 / Z and every product with it are exact, so the interpolated Z is Z


def clip_equality():
    """a fronto-parallel quad exactly at clip_near and another exactly at clip_far, side by side; both are kept"""
    K = np.array([[128.0, 0.0, 32.0], [0.0, 128.0, 24.0], [0.0, 0.0, 1.0]])
    quad = lambda u0, u1, Z: [[(u0, 5.25, Z), (u1, 5.25, Z), (u1, 40.75, Z)], [(u0, 5.25, Z), (u1, 40.75, Z), (u0, 40.75, Z)]]
    return make(*soup(quad(3.25, 28.75, J_NEAR) + quad(34.25, 60.75, J_FAR), K), K, 64, 48, near=J_NEAR, far=J_FAR)


SCENES = {"A_long_list": long_list, "A_long_list_on_seams": long_list_on_seams, "B_long_big_list": long_big_list,
          "C_small_queued_threshold": small_queued_threshold, "D_list_big_threshold": list_big_threshold,
          "E_fan": fan, "E_fan_reversed_winding": lambda: fan(reverse_winding=True), "E_fan_reversed_order": lambda: fan(reverse_order=True),
          "G_scan_carry": scan_carry, "H_far_coordinates": far_coordinates, "I_bad_faces": bad_faces,
          "J_coplanar_overlap": coplanar_overlap, "J_coplanar_overlap_swapped": lambda: coplanar_overlap(swap=True),
          "J_clip_equality": clip_equality}
SCENES.update({"F_%dx%d" % (w, h): (lambda w=w, h=h: image_shape(w, h)) for w, h in F_SHAPES})
TEXTURED = ("A_long_list", "A_long_list_on_seams", "B_long_big_list", "E_fan", "E_fan_reversed_winding", "E_fan_reversed_order")

_built = {}


def scene(name):
    """the scene, built once; its arrays are read-only"""
    if name not in _built:
        s = SCENES[name]()
        for v in s.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _built[name] = s
    return _built[name]


def scene_census(name, pose=0):
    s = scene(name)
    return census(s["pts"], s["faces"], s["K"], s["R"][pose], s["t"][pose], s["w"], s["h"])


def pose_args(s, pose=0):
    """what tests/render_rgb_np.py's fragments / render_ids take, of one pose of the scene"""
    return s["pts"], s["faces"], s["K"], s["R"][pose], s["t"][pose], s["w"], s["h"], s["near"], s["far"]


_restated = {}


def restated(name, pose=0):
    """(depth float32 [h,w], triangle id int32 [h,w]) of the restatement, computed once and read-only"""
    if (name, pose) not in _restated:
        depth, ids = render_ids(*pose_args(scene(name), pose))
        depth.setflags(write=False)
        ids.setflags(write=False)
        _restated[name, pose] = (depth, ids)
    return _restated[name, pose]
