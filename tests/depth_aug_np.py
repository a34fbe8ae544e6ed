"""float64 numpy restatement of pp_depth_augment (csrc/depth_aug.hip): the reference's augmentDepth
(annotation_scripts/Augmentations.py:10-134, augment_syn_LineMOD.py:273-418, augment_syn_Tless.py:219-356) with every operation
in the order the device takes it, so that the device outputs are these bits, and the host sampler of the per-image programs.
No torch, no device.

What is not the reference's: the simplex noise is the project's own (pyfastnoisesimd's bits cannot be had), the standard normals
come in as a field z, and everything after the mask is float64 where cv2 computes float32 images in float32.  cv2 itself is
restated from its documented rules (MORPH_OPEN with the default border, resize INTER_LINEAR, GaussianBlur with BORDER_REFLECT_101,
getGaussianKernel) and is not pinned; scipy's medfilt2d and grey morphology are (tests/test_depth_aug_cpu.py).

One parameter row per image, float64 [P] (the layout of include/pyrapose_hip.h):"""
import numpy as np

P_K_OPEN, P_K_MED, P_K_BLUR, P_TAPS = 0, 1, 2, 3          # taps: 7 slots, the first k_blur used, the others 0
P_DEPTH_NOISE, P_SENSOR, P_SIMPLEX = 10, 11, 12
P_FREQ, P_OCTAVES, P_LACUNARITY, P_GAIN, P_W_XY, P_W_Z = 13, 14, 15, 16, 17, 18
P_JITTER_LO, P_JITTER_HI, P_SEED = 19, 22, 25
P = 26
OUTPUTS = ("depth_f32", "depth_f64", "mask_u8", "half_f64", "sensor_f64")

NOISE_SCALE = 32.0
F3, G3 = 1.0 / 3.0, 1.0 / 6.0
G3_2, G3_3 = 2.0 * G3, 3.0 * G3
GRAD = np.array([[1, 1, 0], [-1, 1, 0], [1, -1, 0], [-1, -1, 0], [1, 0, 1], [-1, 0, 1], [1, 0, -1], [-1, 0, -1],
                 [0, 1, 1], [0, -1, 1], [0, 1, -1], [0, -1, -1]], np.float64)


def blur_taps(k, sigma):
    """cv2.getGaussianKernel(k, sigma) in float64: exp(-x^2 / (2 sigma^2)) over x = -(k-1)/2 .. (k-1)/2, divided by the sum;
    sigma <= 0 means 0.3 ((k - 1) 0.5 - 1) + 0.8"""
    k = int(k)
    sigma = float(sigma)
    if sigma <= 0:
        sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x = np.arange(k, dtype=np.float64) - (k - 1) // 2
    w = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return w / w.sum()


def make_program(k_open=3, k_med=3, k_blur=3, blur_sigma=1.0, depth_noise=0.003, method=0, freq=0.1, octaves=4, lacunarity=2.1,
                 gain=0.45, w_xy=2.0, w_z=0.002, jitter_lo=(0.001, 0.001, 0.01), jitter_hi=(0.01, 0.01, 0.1), seed=1):
    """one parameter row; method 0 | 1 | 2 = both stages | sensor only | simplex only"""
    row = np.zeros(P, np.float64)
    row[[P_K_OPEN, P_K_MED, P_K_BLUR]] = k_open, k_med, k_blur
    row[P_TAPS:P_TAPS + int(k_blur)] = blur_taps(k_blur, blur_sigma)
    row[P_DEPTH_NOISE] = depth_noise
    row[P_SENSOR], row[P_SIMPLEX] = {0: (1, 1), 1: (1, 0), 2: (0, 1)}[int(method)]
    row[[P_FREQ, P_OCTAVES, P_LACUNARITY, P_GAIN, P_W_XY, P_W_Z]] = freq, octaves, lacunarity, gain, w_xy, w_z
    row[P_JITTER_LO:P_JITTER_LO + 3] = jitter_lo
    row[P_JITTER_HI:P_JITTER_HI + 3] = jitter_hi
    row[P_SEED] = seed
    return row


def sample_programs(rng, n, method=0):
    """the reference's distributions, one row per image, drawn from a numpy Generator in a fixed order"""
    rows = []
    for _ in range(n):
        k_open, k_med, k_blur = (int(v) for v in rng.choice([3, 5, 7], size=3))
        sigma = rng.uniform(0.0, 1.5)
        noise = rng.uniform(0.002, 0.004)
        seed = int(rng.integers(0, 2 ** 31))
        freq = rng.uniform(0.05, 0.2)
        octaves = int(rng.choice([4, 8]))
        w_xy = int(rng.integers(2, 5)) if int(method) == 2 else int(rng.integers(1, 5))
        w_z = rng.uniform(0.0001, 0.004)
        rows.append(make_program(k_open, k_med, k_blur, sigma, noise, method, freq, octaves, 2.1, 0.45, float(w_xy), w_z, seed=seed))
    return np.stack(rows) if rows else np.zeros((0, P), np.float64)


# ---- launch A: shadow and halve ---------------------------------------------------------------------------------------------

def _box(m, k, pad, fold):
    """fold the k x k window of every pixel of m, padded with `pad`"""
    r = (int(k) - 1) // 2
    H, W = m.shape
    p = np.pad(m, r, mode="constant", constant_values=pad)
    out = None
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            win = p[dy:dy + H, dx:dx + W]
            out = win.copy() if out is None else fold(out, win)
    return out


def opening(m, k):
    """erode, then dilate, a 0/1 image with a k x k box; pixels outside the image take no part in either"""
    return _box(_box(m, k, 1, np.minimum), k, 0, np.maximum)


def majority(m, k):
    """(count of set pixels in the zero-padded k x k window) > k^2 / 2"""
    return (2 * _box(m.astype(np.int32), k, 0, np.add) > int(k) * int(k)).astype(np.uint8)


def shadow_mask(mask, k_open, k_med):
    """uint8 0/1 [H,W]"""
    m0 = (np.asarray(mask) != 0).astype(np.uint8)
    return majority(opening(m0, k_open), k_med)


def half_size(n):
    """cv2's cvRound(n / 2): half to even"""
    return int(np.rint(n / 2.0))


def halve(d1):
    H, W = d1.shape
    h2, w2 = half_size(H), half_size(W)
    r0, r1 = np.minimum(2 * np.arange(h2), H - 1), np.minimum(2 * np.arange(h2) + 1, H - 1)
    c0, c1 = np.minimum(2 * np.arange(w2), W - 1), np.minimum(2 * np.arange(w2) + 1, W - 1)
    assert r1.max() < H and c1.max() < W and 2 * (h2 - 1) <= H - 1 and 2 * (w2 - 1) <= W - 1
    a = 0.5 * d1[np.ix_(r0, c0)] + 0.5 * d1[np.ix_(r0, c1)]
    b = 0.5 * d1[np.ix_(r1, c0)] + 0.5 * d1[np.ix_(r1, c1)]
    return 0.5 * a + 0.5 * b


# ---- launch B: sensor -------------------------------------------------------------------------------------------------------

def reflect_101(j, n):
    """gfedcb|abcdefgh, mirrored again and again for a line shorter than the reach"""
    if n == 1:
        return np.zeros_like(j)
    p = 2 * (n - 1)
    m = np.mod(j, p)
    return np.where(m < n, m, p - m)


def _blur_axis1(a, w):
    k = len(w)
    r = (k - 1) // 2
    n = a.shape[1]
    idx = np.arange(n)
    acc = w[0] * a[:, reflect_101(idx - r, n)]
    for t in range(1, k):
        acc = acc + w[t] * a[:, reflect_101(idx - r + t, n)]
    return acc


def blur(d2, w):
    """along each row first (axis 1), then along each column"""
    return np.ascontiguousarray(_blur_axis1(_blur_axis1(d2, w).T, w).T)


def sensor(d2, row, z):
    t = (d2 / 1000.0) * 1.41421356
    res = t * t
    b = blur(d2, row[P_TAPS:P_TAPS + int(row[P_K_BLUR])])
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(res != 0, np.rint(b / res) * res, 0.0)
    return q + (q * row[P_DEPTH_NOISE]) * np.asarray(z, np.float32).astype(np.float64), res


# ---- launch C: up-sampling and simplex warp -----------------------------------------------------------------------------------

def _upsample_axis(n_out, n_in):
    f = (np.arange(n_out, dtype=np.float64) + 0.5) * (np.float64(n_in) / np.float64(n_out)) - 0.5
    s = np.floor(f)
    frac = f - s
    s = s.astype(np.int64)
    lo = s < 0
    hi = s >= n_in - 1
    s = np.where(lo, 0, np.where(hi, n_in - 1, s))
    frac = np.where(lo | hi, 0.0, frac)
    return s, np.minimum(s + 1, n_in - 1), frac


def upsample(s, H, W, ys=None, xs=None):
    """cv2.resize(s, (W, H)) INTER_LINEAR, at all pixels or at the pixel lists (ys, xs)"""
    h2, w2 = s.shape
    sy, sy1, fy = _upsample_axis(H, h2)
    sx, sx1, fx = _upsample_axis(W, w2)
    if ys is None:
        ys, xs = np.mgrid[0:H, 0:W]
    sy, sy1, fy, sx, sx1, fx = sy[ys], sy1[ys], fy[ys], sx[xs], sx1[xs], fx[xs]
    top = (1.0 - fx) * s[sy, sx] + fx * s[sy, sx1]
    bot = (1.0 - fx) * s[sy1, sx] + fx * s[sy1, sx1]
    return (1.0 - fy) * top + fy * bot


def splitmix64(x):
    """the published splitmix64 on a uint64 array (the mixer of csrc/splitmix.h)"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def jitter_u(seed, f, pixel):
    """u in [0, 1): (splitmix64(splitmix64(4 seed + f) + pixel index) >> 11) 2^-53"""
    with np.errstate(over="ignore"):
        key = splitmix64(np.array([4 * int(seed) + int(f)], np.uint64))[0] + np.asarray(pixel, np.uint64)
    return (splitmix64(key) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def grad_index(i, j, k, seed):
    """h = lo32(seed) ^ hi32(seed) ^ i 0x9E3779B1 ^ j 0x85EBCA77 ^ k 0xC2B2AE3D in uint32, murmur3's fmix32 of it, mod 12"""
    u = lambda a: (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32)
    s = int(seed)
    with np.errstate(over="ignore"):
        h = np.uint32((s ^ (s >> 32)) & 0xFFFFFFFF) ^ (u(i) * np.uint32(0x9E3779B1)) ^ (u(j) * np.uint32(0x85EBCA77)) ^ (u(k) * np.uint32(0xC2B2AE3D))
        h = h ^ (h >> np.uint32(16))
        h = h * np.uint32(0x85EBCA6B)
        h = h ^ (h >> np.uint32(13))
        h = h * np.uint32(0xC2B2AE35)
        h = h ^ (h >> np.uint32(16))
    return (h % np.uint32(12)).astype(np.int64)


def _corner(x, y, z, gi):
    t = ((0.6 - x * x) - y * y) - z * z
    g = GRAD[gi]
    dot = (g[..., 0] * x + g[..., 1] * y) + g[..., 2] * z
    t2 = t * t
    return np.where(t > 0, (t2 * t2) * dot, 0.0)


def simplex3(x, y, z, seed):
    """Gustavson's 3-D simplex noise: skew 1/3, unskew 1/6, corners ordered by comparing the offsets, fall-off 0.6 - |d|^2,
    t^4 (g . d), the 12 edge-midpoint gradients by grad_index, scale NOISE_SCALE"""
    s = ((x + y) + z) * F3
    fi, fj, fk = np.floor(x + s), np.floor(y + s), np.floor(z + s)
    i, j, k = fi.astype(np.int64), fj.astype(np.int64), fk.astype(np.int64)
    t = ((i + j) + k).astype(np.float64) * G3
    x0, y0, z0 = x - (fi - t), y - (fj - t), z - (fk - t)
    xy, yz, xz = x0 >= y0, y0 >= z0, x0 >= z0
    # the standard six orderings
    i1 = np.where(xy, np.where(yz | xz, 1, 0), 0)
    j1 = np.where(xy, 0, np.where(~yz, 0, 1))
    k1 = np.where(xy, np.where(yz | xz, 0, 1), np.where(~yz, 1, 0))
    i2 = np.where(xy, 1, np.where(~yz | ~xz, 0, 1))
    j2 = np.where(xy, np.where(yz, 1, 0), 1)
    k2 = np.where(xy, np.where(yz, 0, 1), np.where(~yz | ~xz, 1, 0))
    n = _corner(x0, y0, z0, grad_index(i, j, k, seed))
    n = n + _corner((x0 - i1) + G3, (y0 - j1) + G3, (z0 - k1) + G3, grad_index(i + i1, j + j1, k + k1, seed))
    n = n + _corner((x0 - i2) + G3_2, (y0 - j2) + G3_2, (z0 - k2) + G3_2, grad_index(i + i2, j + j2, k + k2, seed))
    n = n + _corner((x0 - 1.0) + G3_3, (y0 - 1.0) + G3_3, (z0 - 1.0) + G3_3, grad_index(i + 1, j + 1, k + 1, seed))
    return NOISE_SCALE * n


def fractal(px, py, pz, octaves, lacunarity, gain, seed):
    """sum_o gain^o N(p lacunarity^o; seed + o) / sum_o gain^o, the powers by repeated multiplication"""
    total, norm, amp, fo = 0.0, 0.0, 1.0, 1.0
    for o in range(int(octaves)):
        total = total + amp * simplex3(px * fo, py * fo, pz * fo, int(seed) + o)
        norm = norm + amp
        amp = amp * gain
        fo = fo * lacunarity
    return total / norm


def noise_fields(H, W, row):
    """V0, V1, V2 [H,W]: field f at (j_f, y, x) freq, j_f = lo + (hi - lo) u"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    pixel = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    freq, seed = row[P_FREQ], int(row[P_SEED])
    out = []
    for f in range(3):
        lo, hi = row[P_JITTER_LO + f], row[P_JITTER_HI + f]
        j = lo + (hi - lo) * jitter_u(seed, f, pixel)
        out.append(fractal(j * freq, y * freq, x * freq, row[P_OCTAVES], row[P_LACUNARITY], row[P_GAIN], seed))
    return out


def warp(D_at, H, W, row):
    """D_at(ys, xs) -> D at integer pixels; the simplex warp of launch C"""
    y, x = np.mgrid[0:H, 0:W]
    V0, V1, V2 = noise_fields(H, W, row)
    a = D_at(y, x) * 0.001
    fx = x.astype(np.float64) + (a * row[P_W_XY]) * V0
    fy = y.astype(np.float64) + (a * row[P_W_XY]) * V1
    fx = np.where(fx < 0, 0.0, np.where(fx > W - 1, np.float64(W - 1), fx)).astype(np.int64)
    fy = np.where(fy < 0, 0.0, np.where(fy > H - 1, np.float64(H - 1), fy)).astype(np.int64)
    out = D_at(fy, fx) + (a * row[P_W_Z]) * V2
    return np.where(out > 0, out, 0.0)


# ---- the whole thing --------------------------------------------------------------------------------------------------------

def depth_augment(depth, mask, row, z=None):
    """depth [H,W] float32, mask [H,W], row [P], z [h2,w2] float32 (needed when row's sensor is 1) -> dict of all OUTPUTS;
    half_f64 is zero and sensor_f64 is d1 for an image without the sensor stage"""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    row = np.asarray(row, np.float64)
    m = shadow_mask(mask, int(row[P_K_OPEN]), int(row[P_K_MED]))
    d1 = np.where(m != 0, depth.astype(np.float64), 0.0)
    h2, w2 = half_size(H), half_size(W)
    if row[P_SENSOR]:
        s, _ = sensor(halve(d1), row, z)
        D_at = lambda ys, xs: upsample(s, H, W, ys, xs)
    else:
        s = np.zeros((h2, w2), np.float64)
        D_at = lambda ys, xs: d1[ys, xs]
    y, x = np.mgrid[0:H, 0:W]
    D = D_at(y, x)
    out = warp(D_at, H, W, row) if row[P_SIMPLEX] else D
    return {"depth_f32": out.astype(np.float32), "depth_f64": out, "mask_u8": (m * np.uint8(255)).astype(np.uint8), "half_f64": s,
            "sensor_f64": D}


def depth_augment_batch(depth, mask, rows, z=None):
    outs = [depth_augment(depth[i], mask[i], rows[i], None if z is None else z[i]) for i in range(len(depth))]
    return {k: np.stack([o[k] for o in outs]) for k in OUTPUTS}
