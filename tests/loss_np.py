"""Plain numpy references of the loss, count, head-export and P16-audit entry points (include/pyrapose_hip.h), written from the
header's contract and the formulas of the reference's losses.py (focal :22-68, orthogonal_l1 :321-408), not from the kernels.

Everything is vectorised numpy.  `dtype` is the arithmetic: float64 is the reference; float32 evaluates the SAME closed form in the
kernels' number format, which is how the GPU tests size their bounds (float32 against float64 on the test's own inputs; the device
is never asked).  tests/test_loss_np_cpu.py pins the float64 references against torch.autograd through oracle/model_torch.py.

Layout (the header's "row space"): a head tensor is level-major, [rows][ld]; level s holds n_img images of h[s] * w[s] cells, image
after image.  Keras concatenates the levels per image: y_true is (B, N, ...) with N = cells * A, anchor a of cell c at c * A + a.
"""
import numpy as np

# losses.py:338-361: edge feature k = (r[a] - r[b]) - (r[c] - r[d]) on the x coordinates; the y feature uses every index + 1
ORTH_QUADS = np.array([
    [0, 6, 2, 4],
    [0, 6, 8, 14],
    [0, 2, 6, 4],
    [0, 2, 8, 10],
    [0, 8, 2, 10],
    [0, 8, 6, 14],
    [12, 10, 14, 8],
    [12, 10, 4, 2],
    [12, 4, 10, 2],
    [12, 4, 14, 6],
    [12, 14, 4, 6],
    [12, 14, 10, 8],
], np.int64)
W_XY, W_ORTH = 0.8, 0.2   # losses.py:323-324


def n_rows(B, shapes):
    return B * sum(h * w for h, w in shapes)


def row_of(B, shapes):
    """int64 [B, cells]: the level-major row of (image b, global cell c) = row_begin[s] + b * hw[s] + (c - cell_off[s]),
    s = the level that cell c lies in."""
    hw = np.array([h * w for h, w in shapes], np.int64)
    cell_off = np.concatenate([[0], np.cumsum(hw)[:-1]])
    row_begin = np.concatenate([[0], np.cumsum(B * hw)[:-1]])
    out = np.empty((B, int(hw.sum())), np.int64)
    for s in range(len(shapes)):
        local = np.arange(hw[s])
        for b in range(B):
            out[b, cell_off[s]: cell_off[s] + hw[s]] = row_begin[s] + b * hw[s] + local
    return out


def to_keras(t, B, shapes, A, V):
    """[rows, ld] level-major -> (B, cells * A, V) in Keras order (columns >= A * V are not read)"""
    rmap = row_of(B, shapes)
    return t[rmap.reshape(-1), : A * V].reshape(B, rmap.shape[1] * A, V)


def from_keras(k, B, shapes, A, V, ld, dtype):
    """(B, cells * A, V) -> [rows, ld] level-major, zero in the padding columns"""
    rmap = row_of(B, shapes)
    out = np.zeros((n_rows(B, shapes), ld), dtype)
    out[rmap.reshape(-1), : A * V] = k.reshape(-1, A * V)
    return out


def focal_ref(logits, y_true, B, shapes, A, C, alpha, gamma, count, loss_weight, eps, one_minus_eps, dtype=np.float64):
    """-> (loss, dlogits [rows, ld]).  p = sigmoid(x); focal weight alpha_t * q^gamma, q = 1 - p where the label is 1 and p
    elsewhere; keras binary_crossentropy on clip(p, eps, one_minus_eps), whose derivative is zero outside the clip; anchors with
    state -1 contribute nothing; normaliser max(1, count); the gradient (not the loss) carries loss_weight."""
    f = np.dtype(dtype).type
    one = f(1)
    x = to_keras(logits, B, shapes, A, C).astype(dtype)
    y = np.asarray(y_true).astype(dtype)
    z, state = y[:, :, :C], y[:, :, C]
    keep = (state != -1)[:, :, None]
    x = np.where(keep, x, f(0))                      # ignored anchors are not read
    p = one / (one + np.exp(-x))
    pos = z == 1
    alpha_t = np.where(pos, f(alpha), one - f(alpha))
    q = np.where(pos, one - p, p)
    fw = alpha_t * q ** f(gamma)
    dfw = np.where(pos, -one, one) * alpha_t * f(gamma) * q ** (f(gamma) - one)      # d fw / d p
    lo, hi = f(eps), f(one_minus_eps)
    pc = np.clip(p, lo, hi)
    inside = (p >= lo) & (p <= hi)
    bce = -(z * np.log(pc) + (one - z) * np.log(one - pc))
    dbce = np.where(inside, -(z / pc) + (one - z) / (one - pc), f(0))                # d bce / d p
    norm = f(max(1, int(count)))
    loss = np.where(keep, fw * bce, f(0)).sum(dtype=dtype) / norm
    grad = np.where(keep, (dfw * bce + fw * dbce) * p * (one - p) / norm * f(loss_weight), f(0))
    return loss, from_keras(grad, B, shapes, A, C, logits.shape[1], dtype)


def orth_edges(v):
    """[..., 16] -> [..., 24]: x1, y1, ..., x12, y12 of losses.py:338-362"""
    out = []
    for a, b, c, d in ORTH_QUADS:
        for o in (0, 1):
            out.append((v[..., a + o] - v[..., b + o]) - (v[..., c + o] - v[..., d + o]))
    return np.stack(out, axis=-1)


def orth_l1_ref(pred, y_true, B, shapes, A, weight, sigma, count, loss_weight, dtype=np.float64):
    """-> (loss, dpred [rows, ld]).  On anchors with state 1: weight * (0.8 * smooth L1 (knee at 1 / sigma^2) + 0.2 * mean of the
    24 |edge difference|), summed and divided by max(1, count); the gradient (not the loss) carries loss_weight."""
    f = np.dtype(dtype).type
    y = np.asarray(y_true)
    pos = y[:, :, 16] == 1
    r = to_keras(pred, B, shapes, A, 16)[pos].astype(dtype)      # [P, 16]: only positives are read
    t = y[:, :, :16][pos].astype(dtype)
    s2 = f(sigma) * f(sigma)
    d = r - t
    ad = np.abs(d)
    quad = ad < f(1) / s2
    xy = np.where(quad, f(0.5) * s2 * ad * ad, ad - f(0.5) / s2)
    g = f(W_XY) * np.where(quad, s2 * d, np.sign(d))
    e = orth_edges(r) - orth_edges(t)
    sg = np.sign(e) * (f(W_ORTH) / f(24))
    for k, (ia, ib, ic, id_) in enumerate(ORTH_QUADS):           # d |e| / d r: +, -, -, + on the quadruple
        for o in (0, 1):
            g[:, ia + o] += sg[:, 2 * k + o]
            g[:, ib + o] -= sg[:, 2 * k + o]
            g[:, ic + o] -= sg[:, 2 * k + o]
            g[:, id_ + o] += sg[:, 2 * k + o]
    norm = f(max(1, int(count)))
    per_anchor = f(W_XY) * xy.sum(axis=1, dtype=dtype) + f(W_ORTH) * (np.abs(e).sum(axis=1, dtype=dtype) / f(24))
    loss = f(weight) * per_anchor.sum(dtype=dtype) / norm
    grad = np.zeros(pos.shape + (16,), dtype)
    grad[pos] = g * (f(weight) * f(loss_weight) / norm)
    return loss, from_keras(grad, B, shapes, A, 16, pred.shape[1], dtype)


def export_ref(src, B, shapes, A, V, apply_sigmoid, dtype=np.float64):
    """out[b][cell * A + a][v] = f(src[row(b, cell)][a * V + v]): (B, cells * A, V); identity keeps src's dtype and bits"""
    k = to_keras(src, B, shapes, A, V)
    if not apply_sigmoid:
        return k.copy()
    f = np.dtype(dtype).type
    return f(1) / (f(1) + np.exp(-k.astype(dtype)))


def count_ref(y_box, y_cls, y_mask, counts):
    """counts[0..2] + number of rows whose last column (the anchor state) is 1; a tensor that is None adds nothing"""
    out = np.array(counts, np.int64).copy()
    for i, y in enumerate((y_box, y_cls, y_mask)):
        if y is not None:
            out[i] += int((np.asarray(y)[..., -1] == 1).sum())
    return out


def p16_stats_ref(hi_halves, cols, within=None):
    """hi_halves uint16 [rows, ld] -> (elements, nonzero, clamped, subnormal, max_abs_bits) over columns < cols of the rows whose
    32-row block is flagged in `within` (None: every row).  With a = the half's 15 magnitude bits: clamped is a >= 0x7700
    (|h| >= 28 672), subnormal is 0 < a < 0x0400 (|h| < 2^-14)."""
    h = np.asarray(hi_halves)
    assert h.dtype == np.uint16 and h.ndim == 2
    rows = h.shape[0]
    sel = np.ones(rows, bool) if within is None else np.asarray(within)[np.arange(rows) >> 5] != 0
    a = (h[sel, :cols] & 0x7FFF).astype(np.int64)
    return (int(a.size), int((a != 0).sum()), int((a >= 0x7700).sum()), int(((a > 0) & (a < 0x0400)).sum()),
            int(a.max()) if a.size else 0)


def strict_measure(got, ref):
    """max |got - ref| / (|ref| + 1e-6 * max |ref|) over every element"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (np.abs(ref) + 1e-6 * np.abs(ref).max())).max())


def max_measure(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---- inputs shared by tests/test_loss_np_cpu.py and tests/test_gpu_losses.py -----------------------------------------------------
LAYOUT_B, LAYOUT_SHAPES = 3, [(5, 7), (3, 4), (2, 2), (1, 1)]
ORTH_MARGIN = 1e-3        # no smooth-L1 residual this close to 0 or to a knee, no edge term this close to 0
ORTH_KNEES = (1.0 / 9.0, 1.0 / 4.0)   # 1 / sigma^2 of the two sigmas the tests use (3 and 2): one draw serves both


def draw_states(rng, B, N):
    """about 10 % positives (1), 10 % ignored (-1), the rest background (0)"""
    return rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=(B, N), p=[0.1, 0.8, 0.1])


def focal_inputs(rng, B, shapes, A, C, ld, saturate=False):
    """-> (logits float32 [rows, ld] with NaN in the padding columns, y_true float32 (B, N, C + 1) with one label per positive).
    Logits: a mixture of N(-4.6, 2) (the prior of the head's bias), N(0, 3) and U(-12, 12), nothing beyond |x| = 12; saturate
    replaces 5 % by +-U(17.5, 30), so that no logit lies in 12 < |x| < 17.5 (where the float32 sigmoid crosses the clip bounds)."""
    rows, AC = n_rows(B, shapes), A * C
    N = rows // B * A
    comp = rng.integers(0, 3, size=(rows, AC))
    x = np.where(comp == 0, rng.normal(-4.6, 2.0, (rows, AC)), np.where(comp == 1, rng.normal(0.0, 3.0, (rows, AC)), 0.0))
    u = rng.uniform(-12.0, 12.0, (rows, AC))
    x = np.where((comp == 2) | (np.abs(x) > 12.0), u, x)
    if saturate:
        big = rng.uniform(17.5, 30.0, (rows, AC)) * rng.choice([-1.0, 1.0], size=(rows, AC))
        x = np.where(rng.uniform(size=(rows, AC)) < 0.05, big, x)
    x = x.astype(np.float32)
    assert not ((np.abs(x) > 12.0) & (np.abs(x) < 17.5)).any()
    logits = np.full((rows, ld), np.nan, np.float32)
    logits[:, :AC] = x
    y = np.zeros((B, N, C + 1), np.float32)
    y[:, :, C] = draw_states(rng, B, N)
    bi, ni = np.nonzero(y[:, :, C] == 1)
    y[bi, ni, rng.integers(0, C, size=len(bi))] = 1
    return logits, y


def orth_offenders(r, t):
    """bool [P]: rows [P, 16] of predictions / targets with a smooth-L1 residual d within ORTH_MARGIN of 0 or of a knee, an edge
    term within ORTH_MARGIN of 0, or a gradient element that nearly cancels: below a knee the element is
    0.8 sigma^2 d + n * 0.2 / 24 with an integer |n| <= 6, and float32 holds a sum within ORTH_MARGIN of zero to no relative
    accuracy that means anything (float64 on the float32 inputs)."""
    r, t = r.astype(np.float64), t.astype(np.float64)
    d = r - t
    ad = np.abs(d)
    bad = ad < ORTH_MARGIN
    for knee in ORTH_KNEES:
        bad |= np.abs(ad - knee) < ORTH_MARGIN
        v = W_XY / knee * d
        n = np.clip(np.rint(v * 24 / W_ORTH), -6, 6)
        bad |= (ad < knee) & (np.abs(v - n * W_ORTH / 24) < ORTH_MARGIN)
    e = np.abs(orth_edges(r) - orth_edges(t))
    return bad.any(axis=1) | (e < ORTH_MARGIN).any(axis=1)


def orth_inputs(rng, B, shapes, A, ld):
    """-> (pred float32 [rows, ld] with NaN in the padding columns, y_true float32 (B, N, 17)).  Residuals N(0, 0.3) put a good part
    on either side of both knees; positive anchors (the only ones the loss reads) that orth_offenders() flags are redrawn on the
    CPU until none is left."""
    rows = n_rows(B, shapes)
    N = rows // B * A
    y = np.zeros((B, N, 17), np.float32)
    y[:, :, 16] = draw_states(rng, B, N)
    t = rng.normal(0.0, 1.0, (B, N, 16)).astype(np.float32)
    r = (t + rng.normal(0.0, 0.3, (B, N, 16))).astype(np.float32)
    pos = np.nonzero((y[:, :, 16] == 1).reshape(-1))[0]
    tp, rp = t.reshape(-1, 16)[pos], r.reshape(-1, 16)[pos]
    for _ in range(200):
        bad = orth_offenders(rp, tp)
        if not bad.any():
            break
        n = int(bad.sum())
        tp[bad] = rng.normal(0.0, 1.0, (n, 16)).astype(np.float32)
        rp[bad] = (tp[bad] + rng.normal(0.0, 0.3, (n, 16))).astype(np.float32)
    assert not orth_offenders(rp, tp).any()
    t.reshape(-1, 16)[pos], r.reshape(-1, 16)[pos] = tp, rp
    y[:, :, :16] = t
    pred = np.full((rows, ld), np.nan, np.float32)
    pred[:, : A * 16] = from_keras(r, B, shapes, A, 16, A * 16, np.float32)
    return pred, y
