"""Numpy restatement of the photometric ops of pyrapose_amd/csrc/photo.hip: the same float32 expressions in the same order
(the header comment of photo.hip defines them), one op at a time on a [H,W,3] uint8 BGR image, rounded to uint8 after every
op.  The device result must equal this byte for byte."""
import numpy as np

F = np.float32


def u8(f):
    return np.clip(np.rint(f), F(0), F(255)).astype(np.uint8)


def lut(img, table):
    return np.stack([table[c][img[..., c]] for c in range(3)], axis=-1)


def gray(img, alpha):
    v = img.astype(F)
    b, g, r = v[..., 0], v[..., 1], v[..., 2]
    luma = (F(0.299) * r + F(0.587) * g) + F(0.114) * b
    a = F(alpha)
    return u8(v + a * (luma[..., None] - v))


def huesat(img, dh, ds):
    dh, ds = int(dh), int(ds)
    if dh == 0 and ds == 0:
        return img.copy()
    v = img.astype(F)
    b, g, r = v[..., 0], v[..., 1], v[..., 2]
    V = np.maximum(np.maximum(b, g), r)
    m = np.minimum(np.minimum(b, g), r)
    d = V - m
    with np.errstate(divide="ignore", invalid="ignore"):
        S = np.where(V > 0, np.rint((F(255) * d) / V), F(0)).astype(np.int32)
        h = np.where(d == 0, F(0),
                     np.where(V == r, (F(30) * (g - b)) / d,
                              np.where(V == g, F(60) + (F(30) * (b - r)) / d, F(120) + (F(30) * (r - g)) / d))).astype(F)
    h = np.where(h < 0, h + F(180), h).astype(F)
    Hq = np.rint(h).astype(np.int32)
    Hq = np.where(Hq >= 180, Hq - 180, Hq)
    H2 = (Hq + dh) % 180
    S2 = np.clip(S + ds, 0, 255)
    s = S2.astype(F) / F(255)
    hh = H2.astype(F) / F(30)
    i = np.floor(hh).astype(np.int32)
    f = hh - i.astype(F)
    p = V * (F(1) - s)
    q = V * (F(1) - s * f)
    t = V * (F(1) - s * (F(1) - f))
    ro = np.choose(np.minimum(i, 5), [V, q, p, p, t, V])
    go = np.choose(np.minimum(i, 5), [t, V, V, q, p, p])
    bo = np.choose(np.minimum(i, 5), [p, p, t, V, V, q])
    return np.stack([u8(bo), u8(go), u8(ro)], axis=-1)


def blend_alpha(H, W, mask):
    mask = np.asarray(mask, F)
    mh, mw = mask.shape

    def axis(n, mn):
        u = (np.arange(n).astype(F) + F(0.5)) * (F(mn) / F(n)) - F(0.5)
        u = np.clip(u, F(0), F(mn - 1)).astype(F)
        i0 = np.floor(u).astype(np.int32)
        return i0, np.minimum(i0 + 1, mn - 1), (u - i0.astype(F)).astype(F)

    y0, y1, fy = axis(H, mh)
    x0, x1, fx = axis(W, mw)
    fx, fy = fx[None, :], fy[:, None]
    top = mask[y0][:, x0] * (F(1) - fx) + mask[y0][:, x1] * fx
    bot = mask[y1][:, x0] * (F(1) - fx) + mask[y1][:, x1] * fx
    return (top * (F(1) - fy) + bot * fy).astype(F)


def blend(img, first, second, mask):
    a = blend_alpha(img.shape[0], img.shape[1], mask)[..., None]
    return u8(a * lut(img, first).astype(F) + (F(1) - a) * lut(img, second).astype(F))


def _windows(img, k, mode):
    r = k // 2
    H, W = img.shape[:2]
    p = np.pad(img, ((r, r), (r, r), (0, 0)), mode=mode)
    for dy in range(k):
        for dx in range(k):
            yield dy, dx, p[dy:dy + H, dx:dx + W]


def conv(img, taps):
    taps = np.asarray(taps, F)
    acc = np.zeros(img.shape, F)
    for dy, dx, win in _windows(img, taps.shape[0], "reflect"):
        acc = acc + taps[dy, dx] * win.astype(F)
    return u8(acc)


def median(img, k):
    stack = np.stack([win for _, _, win in _windows(img, k, "edge")], axis=0)
    return np.sort(stack, axis=0)[k * k // 2]


def bilateral(img, space, colour):
    space, colour = np.asarray(space, F), np.asarray(colour, F)
    ctr = img.astype(np.int32)
    num = np.zeros(img.shape, F)
    den = np.zeros(img.shape[:2], F)
    for dy, dx, win in _windows(img, space.shape[0], "reflect"):
        idx = np.abs(win.astype(np.int32) - ctr).sum(axis=-1)
        w = space[dy, dx] * colour[idx]
        num = num + w[..., None] * win.astype(F)
        den = den + w
    with np.errstate(divide="ignore", invalid="ignore"):
        out = u8(np.nan_to_num(num / den[..., None]))
    return np.where((den > 0)[..., None], out, img)


def apply_op(img, op):
    k = op["kind"]
    if k == "lut":
        return lut(img, op["table"])
    if k == "gray":
        return gray(img, op["alpha"])
    if k == "huesat":
        return huesat(img, op["dh"], op["ds"])
    if k == "blend":
        return blend(img, op["first"], op["second"], op["mask"])
    if k == "conv":
        return conv(img, op["taps"])
    if k == "median":
        return median(img, op["k"])
    if k == "bilateral":
        return bilateral(img, op["space"], op["colour"])
    raise ValueError("unknown op kind %r" % (k,))


def apply_chain(img, chain):
    for op in chain:
        img = apply_op(img, op)
    return img


def apply_batch(images, chains):
    return np.stack([apply_chain(im, ch) for im, ch in zip(images, chains)])
