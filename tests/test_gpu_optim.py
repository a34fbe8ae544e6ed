"""GPU: the multi-tensor Adam with global-norm clip of csrc/optim.hip (ops.Optimizer) against the float64 restatement of
tests/pointwise_np.py, on a tensor set chosen for the kernels' indexing: tensors of one element, of one chunk (1024 elements)
minus one, exactly one, plus one and of several chunks with a tail; a per-column scale whose period (48) does not divide the
chunk; an L2 tensor; frozen tensors with and without a scale; more than 1024 chunks for the stride loop of the final norm
kernel.  Three steps each, both clip branches and the disabled clip; w, w_eff, m, v, the norm and the L2 loss are all compared,
and the gaps between the tensors must stay as they were."""
import numpy as np
import pytest
import torch

from tests import pointwise_np as PN

pytestmark = pytest.mark.gpu

# the entry point takes its hyper-parameters as float32: the reference works in float64 on those same float32 values (1 - 0.999f
# is 1.3e-5 away from 0.001, which is more than the bound on v)
LR, B1, B2, EPS = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-7))
SENTINEL = {"w": 12345.5, "w_eff": -777.25, "m": 31.0, "v": 63.0}
L2_PRELOAD = 0.8125


@pytest.fixture(scope="module")
def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


def layout(specs):
    """specs: (count, ld, trainable, scale_off, l2) -> (params, total); every tensor starts on a multiple of 64 elements and has a
    gap of at least 64 before and behind it"""
    params, off = [], 64
    for (count, ld, trainable, scale_off, l2) in specs:
        params.append(PN.Param(off, count, ld, trainable, scale_off, l2))
        off = (off + count + 63) // 64 * 64 + 64
    return params, off


SMALL = [(1, 1, 1, -1, 0.0), (1023, 1023, 1, -1, 0.0), (1024, 64, 1, -1, 0.0), (1025, 1025, 1, -1, 0.0), (3 * 1024 + 5, 7, 1, -1, 0.0),
         (48 * 50, 48, 1, 0, 0.0),      # scaled: e % 48 across two chunk boundaries (1024 = 21 * 48 + 16)
         (2500, 100, 1, -1, 0.01),      # L2
         (16 * 70, 16, 0, 48, 0.0),     # frozen, scaled
         (1300, 13, 0, -1, 0.0)]        # frozen, unscaled
N_SCALES = 48 + 16
BIG = [(1024 * 1030 + 7, 1024, 1, -1, 0.0)]  # 1031 chunks: the final kernel's 1024 threads take a second trip


def descs_of(params):
    from pyrapose_amd._lib import ParamDesc
    out = []
    for p in params:
        d = ParamDesc()
        d.offset, d.count, d.ld, d.trainable, d.scale_off, d.l2 = p
        out.append(d)
    return out


def gaps_mask(params, total):
    mask = np.ones(total, bool)
    for p in params:
        mask[p.offset:p.offset + p.count] = False
    return mask


def initial_state(params, total, seed):
    rng = np.random.default_rng(seed)
    gaps = gaps_mask(params, total)
    w = rng.standard_normal(total).astype(np.float32)
    # (moments that are already under way: the decay terms count from the first step, and "unchanged" means something on the frozen tensors)
    m, v = (rng.standard_normal(total) * 0.01).astype(np.float32), rng.uniform(0.5e-4, 1.5e-4, total).astype(np.float32)
    w_eff = np.full(total, np.nan, np.float32)
    for name, a in (("w", w), ("w_eff", w_eff), ("m", m), ("v", v)):
        a[gaps] = SENTINEL[name]
    scales = rng.uniform(0.5, 1.5, N_SCALES).astype(np.float32)
    grads = []
    for _ in range(3):
        g = (rng.standard_normal(total) * 0.1).astype(np.float32)
        g[gaps] = np.nan  # a gradient read outside the tensors would poison the norm
        grads.append(g)
    return w, w_eff, m, v, scales, grads


def run_device(ctx, params, total, state, clipnorm, with_l2=True):
    """three steps on the device -> per step (w, w_eff, m, v, gnorm_sq, l2_loss, w before the step) as numpy"""
    from pyrapose_amd import ops
    w0, weff0, m0, v0, scales, grads = state
    w, weff, m, v = (torch.from_numpy(a.copy()).cuda() for a in (w0, weff0, m0, v0))
    sc = torch.from_numpy(scales).cuda()
    gn = torch.full((1,), float("nan"), device="cuda")
    opt = ops.Optimizer(ctx, descs_of(params), total)
    steps = []
    try:
        for step, g in enumerate(grads, 1):
            gd = torch.from_numpy(g).cuda()
            before = w.cpu().numpy()
            l2 = torch.full((1,), L2_PRELOAD, device="cuda") if with_l2 else None
            opt.grad_norm(w, gd, sc, gn, l2)
            opt.adam_step(w, weff, gd, sc, m, v, gn, LR, B1, B2, EPS, clipnorm, step)
            steps.append(tuple(t.cpu().numpy() for t in (w, weff, m, v, gn)) + (float(l2.cpu()) if with_l2 else None, before))
    finally:
        opt.close()
    return steps


def near(got, want, rtol, floor):
    """|got - want| <= rtol * |want| + floor, elementwise; returns the worst excess ratio for the message"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / (rtol * np.abs(want) + floor)).max()) if got.size else 0.0


def check_against_reference(params, total, state, steps, clipnorm):
    w0, weff0, m0, v0, scales, grads = state
    gaps = gaps_mask(params, total)
    wr, mr, vr = w0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    for step, (g, (w, weff, m, v, gn, l2, before)) in enumerate(zip(grads, steps), 1):
        wr, weffr, mr, vr, norm = PN.adam_clipnorm_step(params, wr, mr, vr, np.nan_to_num(g), scales, LR, B1, B2, EPS, clipnorm, step)
        assert clipnorm in (0, 1e-3, 1e3) and (norm >= 1e-3) and (norm < 1e3)  # 1e-3 clips, 1e3 does not
        assert abs(np.sqrt(float(gn[0])) - norm) < 1e-5 * norm, (step, float(gn[0]), norm)
        if l2 is not None:
            # the kernel's sum is over the w it read: the device's own weights before the step, in float64; += onto the preload
            want_l2 = L2_PRELOAD + PN.l2_penalty(params, before)
            assert abs(l2 - want_l2) < 1e-6 * want_l2, (step, l2, want_l2)
        for i, p in enumerate(params):
            sl = slice(p.offset, p.offset + p.count)
            what = (clipnorm, step, i, p)
            np.testing.assert_allclose(w[sl], wr[sl], rtol=2e-5, atol=2e-6, err_msg=str(what))
            np.testing.assert_allclose(weff[sl], weffr[sl], rtol=2e-5, atol=2e-6, err_msg=str(what))
            if p.trainable:
                for name, got, want in (("m", m[sl], mr[sl]), ("v", v[sl], vr[sl])):
                    worst = near(got, want, 1e-5, 1e-6 * np.abs(want).max())
                    assert worst <= 1.0, (name, what, worst)
            else:  # frozen: the state is bit-unchanged, w_eff is the one float32 product (or a copy)
                assert np.array_equal(w[sl], w0[sl]) and np.array_equal(m[sl], m0[sl]) and np.array_equal(v[sl], v0[sl]), what
                sc = scales[p.scale_off + np.arange(p.count) % p.ld] if p.scale_off >= 0 else np.float32(1)
                assert np.array_equal(weff[sl], w0[sl] * sc), what
        for name, got, init in (("w", w, w0), ("w_eff", weff, weff0), ("m", m, m0), ("v", v, v0)):
            assert np.array_equal(got[gaps].view(np.uint32), init[gaps].view(np.uint32)), (name, clipnorm, step)


@pytest.mark.parametrize("clipnorm", [1e-3, 1e3, 0.0], ids=["clip", "noclip", "off"])
def test_adam_tensor_set_vs_float64(ctx, clipnorm):
    params, total = layout(SMALL)
    state = initial_state(params, total, seed=51)
    steps = run_device(ctx, params, total, state, clipnorm)
    check_against_reference(params, total, state, steps, clipnorm)
    # the same run again gives the same bits (fixed-order reduction), and l2_loss = None changes nothing else
    again = run_device(ctx, params, total, state, clipnorm, with_l2=False)
    for a, b in zip(steps, again):
        for x, y in zip(a[:5], b[:5]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("clipnorm", [1e-3, 1e3, 0.0], ids=["clip", "noclip", "off"])
def test_adam_more_than_1024_chunks(ctx, clipnorm):
    params, total = layout(BIG)
    assert sum(-(-p.count // 1024) for p in params) > 1024
    state = initial_state(params, total, seed=52)
    steps = run_device(ctx, params, total, state, clipnorm)
    check_against_reference(params, total, state, steps, clipnorm)
    again = run_device(ctx, params, total, state, clipnorm)
    for a, b in zip(steps, again):
        for x, y in zip(a[:5], b[:5]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert a[5] == b[5]
