"""Numpy restatement of the kernels between the convolutions of a training step: the pointwise / resampling ops and the stem
packers of pyrapose_amd/csrc/elementwise.hip, and the multi-tensor Adam of pyrapose_amd/csrc/optim.hip.  One function per
operation, written from the operation's definition (the header comments of the two files), not from the kernels' loops.
Where a float32 result depends on the order of its additions the function says which order it takes; everything else is
exact.  tests/test_pointwise_np_cpu.py pins these functions to closed forms."""
import collections

import numpy as np

F = np.float32


# ---- MaxPooling2D(3, strides=2, padding='same') ------------------------------------------------------------------------------
def tf_same(n, k=3, s=2):
    """(pad before, pad after, output extent) of TF 'same' padding"""
    out = -(-n // s)
    tot = max((out - 1) * s + k - n, 0)
    return tot // 2, tot - tot // 2, out


def maxpool3x3s2(x):
    """x [B,H,W,C] -> [B,ceil(H/2),ceil(W/2),C]; the padding never wins (identity -inf)"""
    x = np.asarray(x)
    B, H, W, C = x.shape
    pt, pb, oh = tf_same(H)
    pl, pr, ow = tf_same(W)
    xp = np.full((B, pt + H + pb + 2, pl + W + pr + 2, C), -np.inf, x.dtype)
    xp[:, pt:pt + H, pl:pl + W] = x
    out = np.full((B, oh, ow, C), -np.inf, x.dtype)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, xp[:, dy:dy + 2 * oh - 1:2, dx:dx + 2 * ow - 1:2])
    return out


# ---- UpsampleLike: tf.image.resize(NEAREST), TF 2.1 half-pixel centres ----------------------------------------------------------
def nn_index(n_in, n_out):
    """source index of every target index: min(floor((dst + 0.5) * in/out), in - 1), scale and product in float32"""
    scale = F(n_in) / F(n_out)
    i = np.floor((np.arange(n_out, dtype=F) + F(0.5)) * scale).astype(np.int64)
    return np.minimum(i, n_in - 1)


def upsample_add_fwd(src, th, tw, other=None):
    """src [B,sh,sw,C] gathered to [B,th,tw,C] (+ other): one addition per element, so exact in src's type"""
    src = np.asarray(src)
    iy, ix = nn_index(src.shape[1], th), nn_index(src.shape[2], tw)
    out = src[:, iy][:, :, ix]
    return out + other if other is not None else out.copy()


def upsample_add_bwd(dtarget, sh, sw, base=None, dtype=F):
    """the adjoint of the gather: dsrc[b,sy,sx] = base + sum of dtarget over the target pixels that read (sy, sx), accumulated in
    `dtype` in the order base, then target rows ascending, then target columns ascending"""
    g = np.asarray(dtarget).astype(dtype)
    B, th, tw, C = g.shape
    iy, ix = nn_index(sh, th), nn_index(sw, tw)
    acc = np.zeros((B, sh, sw, C), dtype) if base is None else np.asarray(base).astype(dtype).copy()
    # the index is monotone, so the target rows of one source row are consecutive; rank = position inside that run.  All target
    # pixels of one (row rank, column rank) hit distinct source pixels: one vector add per rank pair, ranks in row-major order
    ry = np.arange(th) - np.searchsorted(iy, iy, side="left")
    rx = np.arange(tw) - np.searchsorted(ix, ix, side="left")
    for a in range(int(ry.max()) + 1 if th else 0):
        ys = np.nonzero(ry == a)[0]
        for b in range(int(rx.max()) + 1 if tw else 0):
            xs = np.nonzero(rx == b)[0]
            acc[:, iy[ys][:, None], ix[xs][None, :]] += g[:, ys[:, None], xs[None, :]]
    return acc


def gather_matrix(n_in, n_out):
    """[n_out, n_in] 0/1 matrix of the 1-D nearest gather"""
    m = np.zeros((n_out, n_in))
    m[np.arange(n_out), nn_index(n_in, n_out)] = 1.0
    return m


# ---- stem input: RGB -> 4 channels inside a zero frame ---------------------------------------------------------------------------
def pack_rgb_padded(x3, Hp, Wp, pad):
    """x3 [B,H,W,3] float32 -> [B,Hp,Wp,4]: the image at (pad, pad), zeros in the margin and in channel 3"""
    x3 = np.asarray(x3, F)
    B, H, W, _ = x3.shape
    out = np.zeros((B, Hp, Wp, 4), F)
    out[:, pad:pad + H, pad:pad + W, :3] = x3
    return out


CAFFE_MEAN = (103.939, 116.779, 123.68)


def preprocess_caffe_u8_padded(u8, sizes_hw, Hp, Wp, pad):
    """u8 [B,H,W,3] uint8, sizes_hw = B (h, w): float32(u8) - mean inside each image's own h x w corner, zeros elsewhere (the
    batch padding is NOT mean-subtracted)"""
    u8 = np.asarray(u8)
    B = u8.shape[0]
    out = np.zeros((B, Hp, Wp, 4), F)
    for b, (h, w) in enumerate(sizes_hw):
        for c in range(3):
            out[b, pad:pad + h, pad:pad + w, c] = u8[b, :h, :w, c].astype(F) - F(CAFFE_MEAN[c])
    return out


# ---- keras 2.3.1 Adam with global-norm clipnorm, multi-tensor (optim.hip's header) -------------------------------------------------
Param = collections.namedtuple("Param", "offset count ld trainable scale_off l2")


def _scale_of(p, scales):
    return np.asarray(scales, np.float64)[p.scale_off + np.arange(p.count) % p.ld] if p.scale_off >= 0 else 1.0


def effective_grad(params, w, g, scales):
    """float64 [total]: g * scale[e % ld] + 2 * l2 * w on the trainable tensors, 0 elsewhere"""
    w, g = np.asarray(w, np.float64), np.asarray(g, np.float64)
    ge = np.zeros_like(w)
    for p in params:
        if p.trainable:
            sl = slice(p.offset, p.offset + p.count)
            ge[sl] = g[sl] * _scale_of(p, scales) + 2.0 * p.l2 * w[sl]
    return ge


def l2_penalty(params, w):
    """sum over the trainable tensors of l2 * w^2"""
    w = np.asarray(w, np.float64)
    return float(sum(p.l2 * (w[p.offset:p.offset + p.count] ** 2).sum() for p in params if p.trainable))


def adam_clipnorm_step(params, w, m, v, g, scales, lr, beta1, beta2, eps, clipnorm, step):
    """One step in float64.  Returns (w, w_eff, m, v, norm): new copies of the state, w_eff = w * scale (w where a tensor has no
    scale) on every listed tensor, frozen ones included, and the global norm of the effective gradient before the clip.
    Elements outside every tensor keep w, m, v and get w_eff = nan."""
    w, m, v = (np.array(a, np.float64) for a in (w, m, v))
    ge = effective_grad(params, w, g, scales)
    norm = float(np.sqrt((ge ** 2).sum()))
    if clipnorm > 0 and norm >= clipnorm:
        ge = ge * (clipnorm / norm)
    lr_t = lr * np.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
    w_eff = np.full_like(w, np.nan)
    for p in params:
        sl = slice(p.offset, p.offset + p.count)
        if p.trainable:
            m[sl] = beta1 * m[sl] + (1.0 - beta1) * ge[sl]
            v[sl] = beta2 * v[sl] + (1.0 - beta2) * ge[sl] ** 2
            w[sl] = w[sl] - lr_t * m[sl] / (np.sqrt(v[sl]) + eps)
        w_eff[sl] = w[sl] * _scale_of(p, scales)
    return w, w_eff, m, v, norm
