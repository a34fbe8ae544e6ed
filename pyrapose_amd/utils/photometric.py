"""Host half of the photometric augmentation (utils/image.py:154-191 of the reference: the imgaug chain in front of
cv2.warpAffine): SAMPLING one ordered op list per image, BUILDING every table / tap array in float64, and PACKING a batch's
lists for ops.photo_augment_u8 (pyrapose_amd/csrc/photo.hip applies them; its header comment defines every op).

An op is a dict: kind in {"lut", "gray", "huesat", "blend", "conv", "median", "bilateral"} plus its data, and -- for what the
sampler drew -- name / group / params (the drawn numbers, for inspection and tests).

Parity with imgaug / OpenCV is UNPINNED (neither is installed, the reference has no fixture); the structure and the ranges are
the reference's.  Kernel sizes the reference's ranges allow to be even are handled the way imgaug handles them:
  AverageBlur  keeps an even k (cv2.blur, anchor k // 2: the window covers -k//2 .. k//2 - 1); here those k x k taps sit in
               a (k+1) x (k+1) array whose last row and column are zero;
  MedianBlur   and MotionBlur draw k in 3..7 and use k + 1 when k is even;
  BilateralBlur passes d to cv2.bilateralFilter, which uses radius max(d // 2, 1): d = 1, 2, 3 -> 3 x 3, 4, 5 -> 5 x 5, 6, 7 -> 7 x 7;
  GaussianBlur takes imgaug's own kernel size: int(max(3.3 sigma, 5)) for sigma < 3, plus one when even (5 or 7 here), and is
               skipped for sigma < 1e-3.
"""
import numpy as np

KINDS = {"lut": 1, "gray": 2, "huesat": 3, "blend": 4, "conv": 5, "median": 6, "bilateral": 7}
OP_DTYPE = np.dtype([("kind", "<i4"), ("k", "<i4"), ("off0", "<i4"), ("off1", "<i4"), ("f0", "<f4"), ("f1", "<f4")])
MASK_MAX = 32
MAX_OPS = 32


# ------------------------------------------------------------------------------------------------ tables
def _lut(fn, value):
    """3 x 256 uint8 (b, g, r): fn(i, v) in float64 on i = 0..255, rounded once; value: a scalar or one per channel"""
    v = np.broadcast_to(np.asarray(value, np.float64).reshape(-1, 1), (3, 1)) if np.ndim(value) else np.full((3, 1), float(value))
    i = np.arange(256, dtype=np.float64)[None, :]
    with np.errstate(over="ignore"):
        return np.clip(np.rint(fn(i, v)), 0, 255).astype(np.uint8)


def lut_identity():
    return np.tile(np.arange(256, dtype=np.uint8), (3, 1))


def lut_add(value):
    return _lut(lambda i, v: i + v, value)


def lut_multiply(mul):
    return _lut(lambda i, v: i * v, mul)


def lut_linear_contrast(alpha):
    """imgaug's convention: 127 + alpha (v - 127)"""
    return _lut(lambda i, v: 127.0 + v * (i - 127.0), alpha)


def lut_gamma(gamma):
    return _lut(lambda i, v: 255.0 * (i / 255.0) ** v, gamma)


def lut_sigmoid(gain, cutoff):
    g = np.broadcast_to(np.asarray(gain, np.float64).reshape(-1, 1), (3, 1)) if np.ndim(gain) else np.full((3, 1), float(gain))
    return _lut(lambda i, c: 255.0 / (1.0 + np.exp(g * (c - i / 255.0))), cutoff)


def lut_log(gain):
    return _lut(lambda i, v: 255.0 * v * np.log2(1.0 + i / 255.0), gain)


def compose_luts(first, second):
    """the table of `first` followed by `second` (exact: both map bytes to bytes)"""
    return np.stack([second[c][first[c]] for c in range(3)])


# ------------------------------------------------------------------------------------------------ taps
def gaussian_kernel_size(sigma):
    k = 3.3 * sigma if sigma < 3.0 else (2.9 * sigma if sigma < 5.0 else 2.6 * sigma)
    k = int(max(k, 5))
    return k + 1 if k % 2 == 0 else k


def gaussian_taps(sigma, k=None):
    """cv2.getGaussianKernel(k, sigma) x its transpose, in float64, as float32 taps"""
    k = gaussian_kernel_size(sigma) if k is None else int(k)
    x = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    g /= g.sum()
    return np.outer(g, g).astype(np.float32)


def average_taps(k):
    k = int(k)
    if k % 2 == 1:
        return np.full((k, k), 1.0 / (k * k), np.float32)
    t = np.zeros((k + 1, k + 1), np.float32)  # anchor k // 2: offsets -k/2 .. k/2 - 1
    t[:k, :k] = 1.0 / (k * k)
    return t


def motion_taps(k, angle, direction):
    """imgaug's MotionBlur kernel: a vertical line through the centre column weighted linspace(d, 1 - d) with
    d = (direction + 1) / 2, rotated by `angle` degrees (here: a bilinear inverse map about the centre), normalised to sum 1"""
    k = int(k)
    k = k + 1 if k % 2 == 0 else k
    d = (float(np.clip(direction, -1.0, 1.0)) + 1.0) / 2.0
    base = np.zeros((k, k), np.float64)
    base[:, k // 2] = np.linspace(d, 1.0 - d, num=k)
    c = (k - 1) / 2.0
    th = np.deg2rad(angle)
    yy, xx = np.mgrid[0:k, 0:k].astype(np.float64)
    sx = np.cos(th) * (xx - c) + np.sin(th) * (yy - c) + c
    sy = -np.sin(th) * (xx - c) + np.cos(th) * (yy - c) + c
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    fx, fy = sx - x0, sy - y0
    out = np.zeros((k, k), np.float64)
    for oy, wy in ((0, 1.0 - fy), (1, fy)):
        for ox, wx in ((0, 1.0 - fx), (1, fx)):
            yi, xi = y0 + oy, x0 + ox
            ok = (yi >= 0) & (yi < k) & (xi >= 0) & (xi < k)
            out += np.where(ok, base[np.clip(yi, 0, k - 1), np.clip(xi, 0, k - 1)], 0.0) * wy * wx
    s = out.sum()
    if s <= 0:
        out = base
        s = out.sum()
    return (out / s).astype(np.float32)


def bilateral_size(d):
    return 2 * max(int(d) // 2, 1) + 1


def bilateral_tables(d, sigma_color, sigma_space):
    """cv2.bilateralFilter's weights: space exp(-r^2 / (2 sigma_space^2)) inside the circle r <= radius (0 outside), colour
    exp(-i^2 / (2 sigma_color^2)) for i = |db|+|dg|+|dr| = 0..765"""
    k = bilateral_size(d)
    r = k // 2
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1].astype(np.float64)
    rr = np.sqrt(yy * yy + xx * xx)
    space = np.where(rr <= r, np.exp(-(rr * rr) / (2.0 * sigma_space * sigma_space)), 0.0).astype(np.float32)
    i = np.arange(766, dtype=np.float64)
    colour = np.exp(-(i * i) / (2.0 * sigma_color * sigma_color)).astype(np.float32)
    return space, colour


def frequency_noise_mask(rng, exponent, size):
    """the low-resolution alpha mask of FrequencyNoiseAlpha: white noise shaped by f^exponent in the frequency domain
    (numpy inverse FFT), stretched to [0, 1]; size x size, size <= 32"""
    size = int(size)
    assert 1 <= size <= MASK_MAX
    noise = rng.uniform(size=(size, size)) + 1j * rng.uniform(size=(size, size))
    f = np.fft.fftfreq(size)
    ff = np.sqrt(f[:, None] ** 2 + f[None, :] ** 2)
    scale = np.zeros_like(ff)
    scale[ff > 0] = ff[ff > 0] ** float(exponent)
    m = np.real(np.fft.ifft2(noise * scale))
    lo, hi = m.min(), m.max()
    m = (m - lo) / (hi - lo) if hi > lo else np.full_like(m, 0.5)
    return m.astype(np.float32)


# ------------------------------------------------------------------------------------------------ op constructors
def op_lut(table, **meta):
    table = np.ascontiguousarray(table, np.uint8)
    assert table.shape == (3, 256)
    return dict(kind="lut", table=table, **meta)


def op_gray(alpha, **meta):
    return dict(kind="gray", alpha=float(alpha), **meta)


def op_huesat(dh, ds, **meta):
    return dict(kind="huesat", dh=int(dh), ds=int(ds), **meta)


def op_blend(first, second, mask, **meta):
    return dict(kind="blend", first=np.ascontiguousarray(first, np.uint8), second=np.ascontiguousarray(second, np.uint8),
                mask=np.ascontiguousarray(mask, np.float32), **meta)


def op_conv(taps, **meta):
    return dict(kind="conv", taps=np.ascontiguousarray(taps, np.float32), **meta)


def op_median(k, **meta):
    return dict(kind="median", k=int(k), **meta)


def op_bilateral(space, colour, **meta):
    return dict(kind="bilateral", space=np.ascontiguousarray(space, np.float32), colour=np.ascontiguousarray(colour, np.float32), **meta)


# ------------------------------------------------------------------------------------------------ the sampler
def _maybe_per_channel(rng, draw):
    """imgaug's per_channel=0.5: with probability 0.5 one value per channel, else one for all"""
    if rng.uniform() < 0.5:
        return np.array([draw() for _ in range(3)])
    return draw()


def _some_of(rng, n_choices, lo=0, hi=2):
    n = int(rng.integers(lo, hi + 1))
    return sorted(rng.choice(n_choices, size=n, replace=False).tolist())


def _blur_op(rng, which):
    g = "blur"
    if which == 0:
        sigma = float(rng.uniform(0.0, 2.0))
        if sigma < 1e-3:
            return None
        return op_conv(gaussian_taps(sigma), name="gaussian", group=g, params=dict(sigma=sigma))
    if which == 1:
        k = int(rng.integers(3, 8))
        return op_conv(average_taps(k), name="average", group=g, params=dict(k=k))
    if which == 2:
        k = int(rng.integers(3, 8))
        return op_median(k + 1 if k % 2 == 0 else k, name="median", group=g, params=dict(k=k))
    if which == 3:
        d = int(rng.integers(1, 8))
        sc, ss = float(rng.uniform(10, 250)), float(rng.uniform(10, 250))  # imgaug's defaults for sigma_color / sigma_space
        return op_bilateral(*bilateral_tables(d, sc, ss), name="bilateral", group=g, params=dict(d=d, sigma_color=sc, sigma_space=ss))
    k = int(rng.integers(3, 8))
    angle, direction = float(rng.uniform(0, 360)), float(rng.uniform(-1, 1))
    return op_conv(motion_taps(k, angle, direction), name="motion", group=g, params=dict(k=k, angle=angle, direction=direction))


def _colour_op(rng, which):
    g = "colour"
    if which == 0:
        v = int(rng.integers(-15, 16))
        # imgaug: the value shifts S as it is and H scaled to the [0,180) range of uint8 HSV
        return op_huesat(int(np.rint(v * 180.0 / 255.0)), v, name="huesat", group=g, params=dict(value=v))
    a = float(rng.uniform(0.0, 0.2))
    return op_gray(a, name="grayscale", group=g, params=dict(alpha=a))


def _add(rng, g):
    v = _maybe_per_channel(rng, lambda: int(rng.integers(-10, 11)))
    return op_lut(lut_add(v), name="add", group=g, params=dict(value=v))


def _multiply(rng, g):
    v = _maybe_per_channel(rng, lambda: float(rng.uniform(0.75, 1.25)))
    return op_lut(lut_multiply(v), name="multiply", group=g, params=dict(mul=v))


def _linear(rng, g):
    v = _maybe_per_channel(rng, lambda: float(rng.uniform(0.7, 1.3)))
    return op_lut(lut_linear_contrast(v), name="linear", group=g, params=dict(alpha=v))


def _brightness_ops(rng, which):
    g = "brightness"
    if which == 0:
        return [_add(rng, g), _multiply(rng, g)]
    if which == 1:
        return [_add(rng, g)]
    if which == 2:
        return [_multiply(rng, g)]
    exponent = float(rng.uniform(-4.0, 0.0))
    size = int(rng.integers(4, 17))
    first, second = _multiply(rng, g), _linear(rng, g)
    return [op_blend(first["table"], second["table"], frequency_noise_mask(rng, exponent, size), name="freqnoise", group=g,
                     params=dict(exponent=exponent, size=size, mul=first["params"]["mul"], alpha=second["params"]["alpha"]))]


def _contrast_op(rng, which):
    g = "contrast"
    if which == 0:
        v = _maybe_per_channel(rng, lambda: float(rng.uniform(0.75, 1.25)))
        return op_lut(lut_gamma(v), name="gamma", group=g, params=dict(gamma=v))
    if which == 1:
        per = rng.uniform() < 0.5
        n = 3 if per else 1
        gain = np.array([float(rng.uniform(0.0, 10.0)) for _ in range(n)])
        cutoff = np.array([float(rng.uniform(0.25, 0.75)) for _ in range(n)])
        if not per:
            gain, cutoff = float(gain[0]), float(cutoff[0])
        return op_lut(lut_sigmoid(gain, cutoff), name="sigmoid", group=g, params=dict(gain=gain, cutoff=cutoff))
    if which == 2:
        v = _maybe_per_channel(rng, lambda: float(rng.uniform(0.75, 1.0)))
        return op_lut(lut_log(v), name="log", group=g, params=dict(gain=v))
    return _linear(rng, g)


def sample_chain(rng):
    """One image's op list, drawn with a numpy.random.Generator in the structure and ranges of the reference's chain:
    SomeOf(0-2) blurs, SomeOf(0-2) of hue/sat and grayscale, OneOf brightness, SomeOf(0-2) contrasts; the four groups in random
    order (iaa.Sequential(random_order=True)), the members of a SomeOf in listed order.  The same generator state gives the
    same list.  Each op carries name / group / params; ops of one group instance share `slot` (0..3: its place in the order)."""
    chain = []
    for slot, grp in enumerate(rng.permutation(4).tolist()):
        if grp == 0:
            ops = [_blur_op(rng, w) for w in _some_of(rng, 5)]
        elif grp == 1:
            ops = [_colour_op(rng, w) for w in _some_of(rng, 2)]
        elif grp == 2:
            ops = _brightness_ops(rng, int(rng.integers(0, 4)))
        else:
            ops = [_contrast_op(rng, w) for w in _some_of(rng, 4)]
        for op in ops:
            if op is not None:
                op["slot"] = slot
                chain.append(op)
    return chain


# ------------------------------------------------------------------------------------------------ packing
def fuse_luts(chain):
    """adjacent LUT ops composed into one table (exact)"""
    out = []
    for op in chain:
        if op["kind"] == "lut" and out and out[-1]["kind"] == "lut":
            out[-1] = op_lut(compose_luts(out[-1]["table"], op["table"]), name="fused")
        else:
            out.append(op)
    return out


class PhotoPrograms:
    """A batch's packed programs: op_offsets int32 [B+1], ops (OP_DTYPE records), pool uint8 (tables, taps, masks at 4-byte
    aligned offsets); chains: the fused op lists they were packed from."""

    def __init__(self, chains, op_offsets, ops, pool):
        self.chains, self.op_offsets, self.ops, self.pool = chains, op_offsets, ops, pool
        self._pinned = None

    def __len__(self):
        return len(self.chains)

    def n_ops(self):
        return np.diff(self.op_offsets)

    def pinned_pool(self):
        """the pool in page-locked memory from torch's host allocator (made once), for a non-blocking upload"""
        if self._pinned is None:
            import torch
            t = torch.from_numpy(self.pool if self.pool.size else np.zeros(4, np.uint8))
            self._pinned = t.pin_memory() if torch.cuda.is_available() else t
        return self._pinned


def _odd_square(a, what, kmax=7):
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] % 2 == 0 or a.shape[0] > kmax:
        raise ValueError("%s must be k x k with k odd and <= %d, got %s" % (what, kmax, a.shape))
    return a.shape[0]


def compile_chain(chains, fuse=True):
    """chains: one op list per image (sample_chain's, or hand-built with the op_* constructors) -> PhotoPrograms.
    Adjacent LUTs are fused; malformed ops raise ValueError."""
    fused, recs, blobs, offsets = [], [], [], [0]
    size = 0

    def put(arr):
        nonlocal size
        b = np.ascontiguousarray(arr).tobytes()
        b += b"\0" * (-len(b) % 4)
        off = size
        blobs.append(b)
        size += len(b)
        return off

    for chain in chains:
        chain = fuse_luts(chain) if fuse else list(chain)
        if len(chain) > MAX_OPS:
            raise ValueError("at most %d ops per image, got %d" % (MAX_OPS, len(chain)))
        for op in chain:
            kind = op.get("kind")
            if kind not in KINDS:
                raise ValueError("unknown op kind %r" % (kind,))
            k = off0 = off1 = 0
            f0 = f1 = 0.0
            if kind == "lut":
                if op["table"].shape != (3, 256) or op["table"].dtype != np.uint8:
                    raise ValueError("a LUT is 3 x 256 uint8")
                off0 = put(op["table"])
            elif kind == "gray":
                if not 0.0 <= op["alpha"] <= 1.0:
                    raise ValueError("grayscale alpha in [0, 1], got %r" % (op["alpha"],))
                f0 = op["alpha"]
            elif kind == "huesat":
                if abs(op["dh"]) > 180 or abs(op["ds"]) > 255:
                    raise ValueError("dh in [-180, 180], ds in [-255, 255]")
                f0, f1 = float(op["dh"]), float(op["ds"])
            elif kind == "blend":
                m = op["mask"]
                if op["first"].shape != (3, 256) or op["second"].shape != (3, 256):
                    raise ValueError("blend tables are 3 x 256 uint8")
                if m.ndim != 2 or not (1 <= m.shape[0] <= MASK_MAX and 1 <= m.shape[1] <= MASK_MAX):
                    raise ValueError("a blend mask is at most %d x %d, got %s" % (MASK_MAX, MASK_MAX, m.shape))
                off0 = put(np.concatenate([op["first"], op["second"]]))
                off1 = put(np.array(m.shape, "<i4"))
                put(m.astype("<f4"))
            elif kind == "conv":
                k = _odd_square(op["taps"], "conv taps")
                off0 = put(op["taps"])
            elif kind == "median":
                k = op["k"]
                if k not in (3, 5, 7):
                    raise ValueError("median k is 3, 5 or 7, got %r" % (k,))
            else:
                k = _odd_square(op["space"], "bilateral space weights")
                if op["colour"].shape != (766,):
                    raise ValueError("bilateral colour weights: 766 entries")
                off0, off1 = put(op["space"]), put(op["colour"])
            recs.append((KINDS[kind], k, off0, off1, f0, f1))
        fused.append(chain)
        offsets.append(len(recs))
    return PhotoPrograms(fused, np.asarray(offsets, np.int32), np.array(recs, OP_DTYPE).reshape(-1),
                         np.frombuffer(b"".join(blobs), np.uint8).copy())


def sample_programs(rng, batch):
    """`batch` sampled chains, compiled"""
    return compile_chain([sample_chain(rng) for _ in range(batch)])
