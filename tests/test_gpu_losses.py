"""GPU: the loss, count, head-export, ReLU and P16-audit entry points, element by element, against the float64 numpy references of
tests/loss_np.py (pinned on the CPU by tests/test_loss_np_cpu.py).

focal_kernel / orth_l1_kernel (csrc/losses.hip): every element of dlogits / dpred, the padding columns, the rows of ignored (and,
for the box loss, non-positive) anchors, and the loss increment; on a small multi-level geometry (3 images, 4 levels, A = 9; the
single-level A = 1 mask head; ld == A * 16 and the memset path ld > A * 16 of the box head) and on one geometry per kernel that
needs more workgroups than the launch's cap of 8 * n_cu, so the grid-stride loop runs.  Output buffers start as NaN, the padding
columns of the inputs hold NaN (they are not read), loss_sum starts non-zero (the contract is +=).

Clip bounds.  The kernel is Keras in float32: eps = float32(1e-7), 1 - eps = float32(1) - float32(1e-7) = 1 - 2^-23.  The
reference takes these two float32 values (promoted to float64).  They differ from the float64 oracle's 1 - 1e-7 by about 1 % of
the BCE on saturated negatives (-log(2^-23) = 15.94 against -log(1e-7) = 16.12).

Measures.  strict = max |got - ref| / (|ref| + 1e-6 max |ref|) over every element; maxrel = max |got - ref| / max |ref|; loss =
|got - ref| / |ref| of the increment of loss_sum.

Bounds.  None comes from a device.  Each test evaluates the SAME closed form in numpy float32 (loss_np, dtype=float32) on its own
inputs, measures that against the float64 reference, and allows 8 x the measured value: the margin is for the device's expf / logf
/ powf being a few ulp from numpy's and for the order of the float32 atomics.  Measured on the CPU with the seeds below (the
tests print the figures they run with):

    quantity                                          measured (float32 vs float64)     bound = 8 x
    focal main set, strict, every element of dlogits  1.7e-6 .. 3.1e-5                  1.4e-5 .. 2.5e-4
        (asserted < 1e-4 before it is used: the inputs, not the bound, give way if it is not)
    focal saturation set, maxrel of dlogits           7.6e-7 .. 1.6e-6                  6.1e-6 .. 1.3e-5
    focal, loss                                       1.7e-8 .. 6.9e-6                  + accumulator, see below
    orth_l1, strict, every element of dpred           4.1e-7 .. 3.3e-6                  3.3e-6 .. 2.7e-5
    orth_l1, loss                                     4e-9 .. 1.1e-7                    + accumulator, see below
    export, sigmoid, strict                           about 1.2e-7                      about 1e-6

The saturation set (5 % of the logits at +-U(17.5, 30)) is held to maxrel, not to strict: in float32 1 - p has no relative
accuracy there.  No logit lies in 12 < |x| < 17.5, where the float32 sigmoid crosses the clip bounds and kernel and reference may
legitimately take different branches.

The loss.  The float32 evaluation of a SUM lands where its rounding errors happen to cancel: 4e-6 of float64 on the focal main set,
but 2e-8 on a saturation set and 4e-9 for orth_l1, less than ANY float32 accumulator can show.  The increment is read off
loss_sum = init + loss, a float32 that each workgroup adds to once, and each add rounds by up to 2^-24 (|init| + |loss|), in an
order that changes from run to run.  So the bound on the increment is 8 x measured x |loss| + n_adds x 2^-24 x (|init| + |loss|),
n_adds = the workgroups of the launch (6 / 78 on the small geometries, the cap 8 * n_cu on the large ones: 5e-7 / 5e-6 / 1.2e-4 of
the loss).  The second term is format precision, fixed before any device ran; on the focal main set of the small geometries the
first one dominates.

orth_l1's inputs are conditioned, never its comparison: positive anchors are redrawn (on the CPU, until none is left) while a
smooth-L1 residual lies within 1e-3 of 0 or of a knee 1 / sigma^2, an edge term within 1e-3 of 0, or a gradient element
0.8 sigma^2 d + n 0.2 / 24 within 1e-3 of cancelling.  At least 20 % of the residuals lie on each side of the knee.
"""
import functools

import numpy as np
import pytest
import torch

from tests import loss_np as L

pytestmark = pytest.mark.gpu

MARGIN = 8.0
EPS32 = float(np.float32(1e-7))
ONE_MINUS_EPS32 = float(np.float32(1) - np.float32(1e-7))
FOCAL_PARAMS = [(0.25, 2.0), (0.4, 1.5), (0.1, 3.0)]
ORTH_PARAMS = [(0.125, 3.0), (0.3, 2.0)]
B, SHAPES = L.LAYOUT_B, L.LAYOUT_SHAPES
# needs rows * ld > 8 * n_cu * 256 (focal) / B * cells * A > 8 * n_cu * 256 (orth_l1); asserted on the device the test runs on
FOCAL_STRIDE = (2, [(40, 52), (20, 26), (10, 13), (5, 7), (3, 4)], 9, 13, 128)
ORTH_STRIDE = (1, [(250, 240)], 9, 144)
FOCAL_INIT, ORTH_INIT = 0.5, 0.03125


@pytest.fixture(scope="module")
def ctx():
    from pyrapose_amd import ops
    return ops.Context(0)


def f32(v):
    return float(np.float32(v))


def loss_bound(measured_rel, ref_loss, init, n_adds):
    """absolute bound on the increment of loss_sum: 8 x the measured float32 error of the closed form, plus the rounding of the
    float32 accumulator the increment is read through (module docstring)"""
    return MARGIN * measured_rel * abs(ref_loss) + n_adds * 2.0 ** -24 * (abs(init) + abs(ref_loss))


def cap_of(ctx):
    n_cu, _ = ctx.device_info()
    assert n_cu > 0
    return 8 * n_cu


@functools.lru_cache(maxsize=None)
def focal_case(B_, shapes, A, C, ld, saturate, seed):
    logits, y = L.focal_inputs(np.random.default_rng(seed), B_, list(shapes), A, C, ld, saturate=saturate)
    assert np.isnan(logits[:, A * C:]).all() and not np.isnan(logits[:, : A * C]).any()
    state = y[:, :, C]
    frac = [(state == v).mean() for v in (-1, 1)]
    assert all(0.04 < v < 0.2 for v in frac), frac
    assert ((y[:, :, :C] == 1).sum(axis=2) == (state == 1)).all()      # one label per positive, none elsewhere
    return logits, y, torch.from_numpy(logits).cuda(), torch.from_numpy(y).cuda()


@functools.lru_cache(maxsize=None)
def orth_case(B_, shapes, A, ld, seed):
    pred, y = L.orth_inputs(np.random.default_rng(seed), B_, list(shapes), A, ld)
    assert np.isnan(pred[:, A * 16:]).all() and not np.isnan(pred[:, : A * 16]).any()
    pos = y[:, :, 16] == 1
    r, t = L.to_keras(pred, B_, list(shapes), A, 16)[pos], y[:, :, :16][pos]
    assert pos.sum() > 0 and not L.orth_offenders(r, t).any()
    ad = np.abs(r.astype(np.float64) - t.astype(np.float64))
    for knee in L.ORTH_KNEES:
        below = (ad < knee).mean()
        assert 0.2 <= below <= 0.8, (knee, below)
    return pred, y, torch.from_numpy(pred).cuda(), torch.from_numpy(y).cuda()


def anchor_mask(flag_bn, B_, shapes, A, V, ld):
    """bool [rows, ld]: the elements of the anchors flagged in flag_bn (B, N)"""
    k = np.broadcast_to(flag_bn[:, :, None], flag_bn.shape + (V,))
    return L.from_keras(k, B_, shapes, A, V, ld, np.float32) != 0


def run_focal(ctx, case, geo, alpha, gamma, count, lw, want_loss=True, want_grad=True):
    from pyrapose_amd import ops
    B_, shapes, A, C, ld = geo
    rs = ops.RowSpace.make(B_, shapes)
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    loss = torch.tensor([FOCAL_INIT], dtype=torch.float32, device="cuda") if want_loss else None
    d = torch.full((L.n_rows(B_, shapes), ld), float("nan"), dtype=torch.float32, device="cuda") if want_grad else None
    ops.focal(ctx, rs, A, C, case[2], case[3], alpha, gamma, cnt, lw, loss, d)
    torch.cuda.synchronize()
    return (float(loss.cpu()[0].double()) - FOCAL_INIT if want_loss else None), (d.cpu().numpy() if want_grad else None)


def check_focal(ctx, geo, saturate, alpha, gamma, combos, seed):
    B_, shapes, A, C, ld = geo
    case = focal_case(B_, tuple(shapes), A, C, ld, saturate, seed)
    logits, y = case[0], case[1]
    state = y[:, :, C]
    true_count = int((state == 1).sum())
    ignored = anchor_mask(state == -1, B_, shapes, A, C, ld)
    assert ignored.any()
    alpha = f32(alpha)                                      # what the entry point is handed
    n_adds = min(-(-L.n_rows(B_, shapes) * ld // 256), cap_of(ctx))
    for count, lw in combos:
        count = true_count if count is None else count
        ref_loss, ref = L.focal_ref(logits, y, B_, shapes, A, C, alpha, gamma, count, lw, EPS32, ONE_MINUS_EPS32)
        r32_loss, r32 = L.focal_ref(logits, y, B_, shapes, A, C, alpha, gamma, count, lw, EPS32, ONE_MINUS_EPS32, dtype=np.float32)
        m_loss = abs(float(r32_loss) - ref_loss) / abs(ref_loss)
        tol_loss = loss_bound(m_loss, ref_loss, FOCAL_INIT, n_adds)
        m_grad = L.max_measure(r32, ref) if saturate else L.strict_measure(r32, ref)
        if not saturate:
            assert m_grad < 1e-4, m_grad                    # the condition on the inputs under which the strict measure is used
        got_loss, got = run_focal(ctx, case, geo, alpha, gamma, count, lw)
        e_grad = L.max_measure(got, ref) if saturate else L.strict_measure(got, ref)
        print("focal %s sat=%d a=%g g=%g count=%d lw=%g: %s float32 %.3g bound %.3g device %.3g | loss %.9g float32 %.3g bound(abs) %.3g "
              "device(abs) %.3g" % (shapes, saturate, alpha, gamma, count, lw, "maxrel" if saturate else "strict", m_grad, MARGIN * m_grad,
                                    e_grad, ref_loss, m_loss, tol_loss, abs(got_loss - ref_loss)))
        assert np.isfinite(got).all()
        assert (got[:, A * C:] == 0).all()
        assert (got[ignored] == 0).all()
        assert e_grad <= MARGIN * m_grad
        assert abs(got_loss - ref_loss) <= tol_loss
    # dlogits = NULL leaves the loss as it is (to the order of the atomics), loss_sum = NULL leaves the gradient bit for bit
    only_loss, _ = run_focal(ctx, case, geo, alpha, gamma, count, lw, want_grad=False)
    assert abs(only_loss - ref_loss) <= tol_loss
    _, only_grad = run_focal(ctx, case, geo, alpha, gamma, count, lw, want_loss=False)
    assert np.array_equal(only_grad, got)


ALL_COMBOS = [(None, 1.0), (None, 0.5), (0, 1.0), (0, 0.5)]     # (count: None = the true one, 0 = normaliser 1; loss_weight)
HEADS = {"cls": (B, SHAPES, 9, 13, 128), "mask": (B, [(5, 7)], 1, 13, 16)}


@pytest.mark.parametrize("saturate", [False, True], ids=["main", "saturated"])
@pytest.mark.parametrize("alpha,gamma", FOCAL_PARAMS)
@pytest.mark.parametrize("head", sorted(HEADS))
def test_focal_every_element_layout(ctx, head, alpha, gamma, saturate):
    check_focal(ctx, HEADS[head], saturate, alpha, gamma, ALL_COMBOS, seed=21)


@pytest.mark.parametrize("saturate", [False, True], ids=["main", "saturated"])
@pytest.mark.parametrize("alpha,gamma", FOCAL_PARAMS)
def test_focal_every_element_stride_loop(ctx, alpha, gamma, saturate):
    B_, shapes, A, C, ld = FOCAL_STRIDE
    assert L.n_rows(B_, shapes) * ld > cap_of(ctx) * 256
    check_focal(ctx, FOCAL_STRIDE, saturate, alpha, gamma, [(None, 1.0), (0, 0.5)], seed=22)


def run_orth(ctx, case, geo, weight, sigma, count, lw, want_loss=True, want_grad=True):
    from pyrapose_amd import ops
    B_, shapes, A, ld = geo
    rs = ops.RowSpace.make(B_, shapes)
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    loss = torch.tensor([ORTH_INIT], dtype=torch.float32, device="cuda") if want_loss else None
    d = torch.full((L.n_rows(B_, shapes), ld), float("nan"), dtype=torch.float32, device="cuda") if want_grad else None
    ops.orth_l1(ctx, rs, A, case[2], case[3], weight, sigma, cnt, lw, loss, d)
    torch.cuda.synchronize()
    return (float(loss.cpu()[0].double()) - ORTH_INIT if want_loss else None), (d.cpu().numpy() if want_grad else None)


def check_orth(ctx, geo, weight, sigma, combos, seed):
    B_, shapes, A, ld = geo
    case = orth_case(B_, tuple(shapes), A, ld, seed)
    pred, y = case[0], case[1]
    state = y[:, :, 16]
    true_count = int((state == 1).sum())
    not_positive = anchor_mask(state != 1, B_, shapes, A, 16, ld)
    assert not_positive.any() and (state == -1).any() and (state == 0).any()
    n_adds = min(-(-L.n_rows(B_, shapes) * A // 256), cap_of(ctx))
    weight = f32(weight)
    for count, lw in combos:
        count = true_count if count is None else count
        ref_loss, ref = L.orth_l1_ref(pred, y, B_, shapes, A, weight, sigma, count, lw)
        r32_loss, r32 = L.orth_l1_ref(pred, y, B_, shapes, A, weight, sigma, count, lw, dtype=np.float32)
        m_loss = abs(float(r32_loss) - ref_loss) / abs(ref_loss)
        tol_loss = loss_bound(m_loss, ref_loss, ORTH_INIT, n_adds)
        m_grad = L.strict_measure(r32, ref)
        got_loss, got = run_orth(ctx, case, geo, weight, sigma, count, lw)
        e_grad = L.strict_measure(got, ref)
        print("orth_l1 %s ld=%d w=%g s=%g count=%d lw=%g: strict float32 %.3g bound %.3g device %.3g | loss %.9g float32 %.3g bound(abs) %.3g "
              "device(abs) %.3g" % (shapes, ld, weight, sigma, count, lw, m_grad, MARGIN * m_grad, e_grad, ref_loss, m_loss, tol_loss,
                                    abs(got_loss - ref_loss)))
        assert np.isfinite(got).all()
        assert (got[:, A * 16:] == 0).all()
        assert (got[not_positive] == 0).all()
        assert e_grad <= MARGIN * m_grad
        assert abs(got_loss - ref_loss) <= tol_loss
    only_loss, _ = run_orth(ctx, case, geo, weight, sigma, count, lw, want_grad=False)
    assert abs(only_loss - ref_loss) <= tol_loss
    _, only_grad = run_orth(ctx, case, geo, weight, sigma, count, lw, want_loss=False)
    assert np.array_equal(only_grad, got)


@pytest.mark.parametrize("weight,sigma", ORTH_PARAMS)
@pytest.mark.parametrize("ld", [144, 160], ids=["ld144", "ld160-memset"])
def test_orth_l1_every_element_layout(ctx, ld, weight, sigma):
    check_orth(ctx, (B, SHAPES, 9, ld), weight, sigma, ALL_COMBOS, seed=23)


@pytest.mark.parametrize("weight,sigma,count,lw", [(0.125, 3.0, None, 1.0), (0.3, 2.0, 0, 0.5)])
def test_orth_l1_every_element_stride_loop(ctx, weight, sigma, count, lw):
    B_, shapes, A, ld = ORTH_STRIDE
    assert L.n_rows(B_, shapes) * A > cap_of(ctx) * 256
    check_orth(ctx, ORTH_STRIDE, weight, sigma, [(count, lw)], seed=24)


def test_count_positives_exact(ctx):
    """three tensors of different row counts and widths at once; only state == 1 (the LAST column) counts, a label of 1.0 in a
    non-positive row does not; counts are added to; a tensor that is None leaves its count alone; one tensor goes past the grid cap
    of 1024 workgroups x 256 rows"""
    from pyrapose_amd import ops
    rng = np.random.default_rng(25)

    def labelled(shape):
        y = np.zeros(shape, np.float32)
        y[:, :, -1] = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=shape[:2], p=[0.1, 0.8, 0.1])
        y[:, :, :-1] = (rng.uniform(size=(shape[0], shape[1], shape[2] - 1)) < 0.3)     # 1.0 labels in rows of every state
        return y

    y_box = rng.standard_normal((2, 1000, 17)).astype(np.float32)
    y_box[:, :, 16] = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=(2, 1000), p=[0.1, 0.8, 0.1])
    y_box[:, ::3, 15] = 1.0
    y_cls, y_mask, y_big = labelled((3, 701, 14)), labelled((2, 333, 6)), labelled((1, 300000, 2))
    assert y_big.shape[1] > 1024 * 256
    zeros = np.zeros((2, 500, 6), np.float32)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    for trio in [(y_box, y_cls, y_mask), (y_box, None, y_mask), (None, y_cls, zeros), (y_box, y_big, None), (None, None, y_big)]:
        init = [5, 60, 700]
        counts = torch.tensor(init + [9], dtype=torch.int32, device="cuda")
        ops.count_positives(ctx, *[dev(a) for a in trio], counts)
        want = L.count_ref(*trio, init)
        assert counts.cpu().numpy().tolist() == want.tolist() + [9], (counts.cpu().numpy(), want)
    assert L.count_ref(y_box, y_big, None, [0, 0, 0])[1] > 20000


@pytest.mark.parametrize("A,V,ld,sig", [(9, 16, 160, 0), (9, 13, 128, 1), (1, 16, 24, 0), (1, 13, 16, 1)])
def test_export_head_every_element(ctx, A, V, ld, sig):
    """identity bit for bit; sigmoid to 8 x the float32-numpy error (strict measure); every output element written; NaN in the
    padding columns of the source is not read"""
    from pyrapose_amd import ops
    rng = np.random.default_rng(26)
    rows, cells = L.n_rows(B, SHAPES), L.n_rows(1, SHAPES)
    src = np.full((rows, ld), np.nan, np.float32)
    src[:, : A * V] = rng.normal(0.0, 4.0, (rows, A * V)).astype(np.float32)
    out = torch.full((B, cells * A, V), float("nan"), dtype=torch.float32, device="cuda")
    ops.export_head(ctx, ops.RowSpace.make(B, SHAPES), A, V, torch.from_numpy(src).cuda(), sig, out)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    if not sig:
        assert np.array_equal(got.view(np.uint32), L.export_ref(src, B, SHAPES, A, V, False).view(np.uint32))
        return
    ref = L.export_ref(src, B, SHAPES, A, V, True)
    m = L.strict_measure(L.export_ref(src, B, SHAPES, A, V, True, dtype=np.float32), ref)
    e = L.strict_measure(got, ref)
    print("export sigmoid A=%d: strict float32 %.3g bound %.3g device %.3g" % (A, m, MARGIN * m, e))
    assert e <= MARGIN * m


@pytest.mark.parametrize("n", [4, 1020, 256 * 1024 + 12])
def test_relu_fwd_bit_exact(ctx, n):
    """pp_relu_fwd == np.maximum(x, 0) bit for bit, with -0.0, subnormals and infinities among the inputs; n % 4 == 0 is what the
    entry accepts, and n is no multiple of 256"""
    from pyrapose_amd import ops
    rng = np.random.default_rng(27)
    x = rng.standard_normal(n).astype(np.float32)
    special = np.array([-0.0, 0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, np.inf, -np.inf, 3.4e38, -3.4e38], np.float32)
    if n >= 1020:
        x[rng.choice(n, size=10 * 50, replace=False)] = np.tile(special, 50)
    else:
        x[:] = special[[0, 2, 3, 6]]
    assert n % 4 == 0 and n % 256 != 0
    y = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    ops.relu_fwd(ctx, torch.from_numpy(x).cuda(), y)
    want = np.maximum(x, np.float32(0))
    assert np.array_equal(y.cpu().numpy().view(np.uint32), want.view(np.uint32))
    if n == 1020:
        with pytest.raises(ValueError, match="multiple of 4"):
            ops.relu_fwd(ctx, torch.from_numpy(x[:1018].copy()).cuda(), y)


def test_planes_stats_exact(ctx):
    """pp_planes_stats on a P16 tensor with known populations: the five numbers equal the reference's count over the hi plane's
    halves AND what the construction says (so an encoder that did not clamp, or flushed a subnormal, shows too)"""
    from pyrapose_amd import ops
    p16 = ctx.twin(1)
    rng = np.random.default_rng(28)
    rows, ld = 100, 32
    n = rows * ld
    kind = rng.choice(5, size=n, p=[0.3, 0.4, 0.1, 0.1, 0.1])       # zero, ordinary, clamped, half-subnormal, flushed
    sign = rng.choice(np.array([-1.0, 1.0]), size=n)
    v = np.zeros(n, np.float64)
    v = np.where(kind == 1, rng.uniform(1e-3, 2000.0, n), v)
    v = np.where(kind == 2, rng.uniform(28672.0, 60000.0, n), v)
    v = np.where(kind == 3, rng.uniform(1e-7, 6.0e-5, n), v)        # inside (6e-8, 6.1e-5): below the smallest normal half 2^-14
    v = np.where(kind == 4, rng.uniform(1e-9, 2.9e-8, n), v)        # below 2^-25: the half is zero
    v = (v * sign).astype(np.float32)
    i_clamp = np.nonzero(kind == 2)[0]
    v[i_clamp[0]], v[i_clamp[1]], v[i_clamp[2]] = 28672.0, -70000.0, 1e9     # at the clamp exactly; above the largest half 65504
    x = v.reshape(rows, ld)
    kind = kind.reshape(rows, ld)
    hi, lo = ops.new_planes(rows, ld)
    ops.split_planes3(p16, torch.from_numpy(x).cuda(), hi, lo)
    halves = hi.contiguous().reshape(rows, ld).cpu().numpy().view(np.uint16)
    within = torch.tensor([1, 0, 1, 0], dtype=torch.uint8, device="cuda")       # rows 96..99 are a partial last block
    in_blocks = (np.arange(rows) >> 5) % 2 == 0

    def expected(sel_rows, cols):
        k = kind[sel_rows, :cols]
        return (k.size, int(((k >= 1) & (k <= 3)).sum()), int((k == 2).sum()), int((k == 3).sum()))

    total = np.zeros(5, np.int64)
    for cols, w, sel in [(ld, None, np.ones(rows, bool)), (16, None, np.ones(rows, bool)), (ld, within, in_blocks), (16, within, in_blocks)]:
        stats = torch.zeros(5, dtype=torch.int64, device="cuda")
        ops.planes_stats(p16, (hi, lo), cols, stats, within=w)
        got = tuple(stats.cpu().numpy().tolist())
        want = L.p16_stats_ref(halves, cols, None if w is None else w.cpu().numpy())
        assert got == want, (cols, got, want)
        assert got[:4] == expected(sel, cols), (cols, got, expected(sel, cols))
        assert got[4] == 0x7700                                     # 28 672: nothing is stored above the clamp
        # a second call adds to the four counters and keeps the maximum
        ops.planes_stats(p16, (hi, lo), 16, stats, within=within)
        again = L.p16_stats_ref(halves, 16, within.cpu().numpy())
        got2 = tuple(stats.cpu().numpy().tolist())
        assert got2 == tuple(a + b for a, b in zip(want[:4], again[:4])) + (max(want[4], again[4]),)
    # the maximum is kept across calls, not overwritten: a tensor of small values after a large one
    small = torch.full((32, 8), 0.5, dtype=torch.float32, device="cuda")
    shi, slo = ops.new_planes(32, 8)
    ops.split_planes3(p16, small, shi, slo)
    stats = torch.zeros(5, dtype=torch.int64, device="cuda")
    ops.planes_stats(p16, (hi, lo), ld, stats)
    ops.planes_stats(p16, (shi, slo), 8, stats)
    assert stats.cpu().numpy().tolist()[4] == 0x7700 and stats.cpu().numpy().tolist()[0] == n + 256
    # bf16 pairs keep the float32 range: the audit refuses a context in that format
    assert ctx.planes_fmt == 0
    with pytest.raises(ValueError, match="P16 context"):
        ops.planes_stats(ctx, (hi, lo), ld, torch.zeros(5, dtype=torch.int64, device="cuda"))
