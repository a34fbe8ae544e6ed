"""GPU: the stride-2 data gradient with all parity classes in one launch (pp_conv2d_nhwc_bwd_data_s2_bf16x3, igemm3m_kernel).

One table, CASES.  Every case asserts its plan, runs the new entry point and
  1. compares dx byte for byte -- guard bands included -- with pp_conv2d_nhwc_bwd_data_bf16x3 on the same operands (the route of
     one launch per class plus class_fill_kernel: the same products in the same order, so nothing may differ);
  2. compares it with float64 under the per-kernel bound of tests/test_gpu_conv_tiles.py (1e-4 of the output's scale; its helpers).

Shapes are the smallest at which the route can go wrong: class grids of four different sizes (5x7, 6x5), classes without rows (H = 1;
a 1x1 input), a class below one tile, one row over a tile (65), classes that are exact multiples of the tile (16x16); a 1x1 kernel
(one class with a tap, three that only run the epilogue) and 3x3 with pad (0, 0) and (1, 1) (which class gets the four taps moves
with the padding); cin 64 and 160 (a column tail of 32 on either tile width; the weight split takes cin % 32 == 0 only, so the 144
of the 3D-box head's cout is not a cin any call can have), cout 32 and 48 (a reduction rounded up to 64).  No shape this small makes the
planner leave the 64 x 64 tile by itself, so the 64 x 128 cases set the per-launch hook PP_CONV3_TILE as tests/test_gpu_conv_tiles.py
does; either way the plan text is asserted before the launch.  Operand forms: all planes (both plane formats: the ctx fixture)
and all float32; addend absent / float32 / planes; ReLU source absent / its hi plane (float32 for the all-float32 form).

Then the refusals (PP_ERR_ARG before anything is launched) and one B = 1 training plan run with the merged route and, under
PP_CONV3_S2MERGED=0, with the per-class route in the same process: every gradient a stride-2 launch writes is bit-identical."""
import collections
import ctypes as C
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import test_gpu_conv_tiles as T
from tests.test_gpu_conv import _cat_rows
from tests.test_gpu_planes import planned

pytestmark = pytest.mark.gpu

# name; B images of H x W; cin, cout; k, pad (top = left); form "pp" (dy, dx planes) / "ff" (float32); addend None / "f32" / "planes";
# mask: ReLU source given; tile
Case = collections.namedtuple("Case", "name B H W cin cout k pad form addend mask tile")


def _cases():
    geos = [("5x7", 2, 5, 7), ("6x5", 2, 6, 5), ("h1", 2, 1, 9), ("one_cell", 3, 1, 1), ("m65", 1, 9, 25), ("exact", 2, 16, 16)]
    kernels = [(1, 0), (3, 0), (3, 1)]
    chans = [(64, 32), (160, 48)]
    eps = [(None, False), ("f32", True), ("planes", True), ("planes", False), ("f32", False), (None, True)]
    rows, i = [], 0
    for gi, (gname, B, H, W) in enumerate(geos):
        for ki, (k, pad) in enumerate(kernels):
            for form in ("pp", "ff"):
                cin, cout = chans[(gi + ki + (form == "ff")) % 2]
                addend, mask = eps[i % len(eps)]
                if form == "ff" and addend == "planes":
                    addend = "f32"
                tile = "64x128" if (gi + ki) % 2 else "64x64"
                rows.append(Case("%s_k%dp%d_%s_c%d_%s%s_%s" % (gname, k, pad, form, cin, addend or "noadd", "_mask" if mask else "", tile), B, H, W, cin, cout,
                                 k, pad, form, addend, mask, tile))
                i += 1
    # every epilogue form on the shape with four unequal classes, 1x1 (the classes without taps ARE the epilogue) and 3x3
    for k, pad in ((1, 0), (3, 1)):
        for form in ("pp", "ff"):
            for addend, mask in eps:
                if form == "ff" and addend == "planes":
                    continue
                name = "ep_5x7_k%d_%s_%s%s" % (k, form, addend or "noadd", "_mask" if mask else "")
                if not any(r.name.startswith(name) for r in rows):
                    rows.append(Case(name, 2, 5, 7, 160, 48, k, pad, form, addend, mask, "64x64"))
    return rows


CASES = _cases()
TILE_ENV = {"64x64": "1,1", "64x128": "1,2"}


@pytest.fixture(scope="module", params=[0, 1], ids=["bf16x3", "f16c8"])
def ctx(request):
    from pyrapose_amd.runtime import default_context
    T.FMT[0] = request.param
    return default_context().twin(request.param)


def _out_hw(c):
    return -(-c.H // 2), -(-c.W // 2)


def _desc(c):
    from pyrapose_amd import ops
    return ops.make_conv_desc(c.B, [(c.H, c.W)], [_out_hw(c)], c.cin, c.cout, c.k, 2, c.pad, c.pad, c.cin, (c.cout + 31) // 32 * 32, (c.cout + 15) // 16 * 16)


def _forms(c):
    from pyrapose_amd import ops
    return (ops.PLAN_PLANES_IN | ops.PLAN_PLANES_OUT) if c.form == "pp" else 0


def _f64_dgrad(c, w, gy):
    """float64 dx [B, H, W, cin] of the stride-2 conv (pad top / left, as much zero extension at the bottom / right as the output needs)"""
    oh, ow = _out_hw(c)
    x = torch.zeros((c.B, c.cin, c.H, c.W), dtype=torch.float64, requires_grad=True)
    pb, pr = (oh - 1) * 2 + c.k - c.H - c.pad, (ow - 1) * 2 + c.k - c.W - c.pad
    y = F.conv2d(F.pad(x, (c.pad, pr, c.pad, pb)), w.permute(3, 2, 0, 1), None, stride=2)
    assert y.shape[2:] == (oh, ow)
    gx, = torch.autograd.grad((y * gy.permute(0, 3, 1, 2)).sum(), [x])
    return gx.permute(0, 2, 3, 1).reshape(-1, c.cin)


def _operands(ctx, c):
    rng = np.random.default_rng([11, sum(map(ord, c.name))])
    oh, ow = _out_hw(c)
    rows_in = c.B * c.H * c.W
    w = torch.as_tensor(rng.standard_normal((c.k, c.k, c.cin, c.cout)) / np.sqrt(c.k * c.k * c.cin), dtype=torch.float64)
    gy64 = torch.as_tensor(rng.standard_normal((c.B, oh, ow, c.cout)), dtype=torch.float64)
    gy = _cat_rows([gy64], (c.cout + 31) // 32 * 32)
    add = torch.as_tensor(rng.standard_normal((rows_in, c.cin)), dtype=torch.float32).cuda()
    msk = torch.relu(torch.as_tensor(rng.standard_normal((rows_in, c.cin)), dtype=torch.float32)).cuda()
    return w, gy, T._split(ctx, gy), add, T._split(ctx, add), msk, T._split(ctx, msk)


def _call(fn, ctx, c, d, wdg, gy, gp, add, ap, msk, mp):
    out = T.Guarded(c.B * c.H * c.W, c.cin, 64, c.form == "ff", c.form == "pp")
    pp = c.form == "pp"
    fn(ctx, d, None if pp else gy, wdg[0], wdg[1], add if c.addend == "f32" else None, msk if (c.mask and not pp) else None, out.t,
       dy_planes=gp if pp else None, dx_planes=out.pl, addend_planes=ap if c.addend == "planes" else None,
       relu_src_hi=mp[0] if (c.mask and pp) else None)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_merged_launch_equals_the_class_launches_and_float64(ctx, c, monkeypatch):
    from pyrapose_amd import ops
    T._set_env(monkeypatch, {"PP_CONV3_TILE": TILE_ENV[c.tile]})
    d = _desc(c)
    # the plan of this very call: one launch at the case's tile, the classes that have rows, no fill
    new_plan, = planned(ctx, d, ops.PLAN_BWD_DATA_S2, _forms(c))
    n_cls = (1 if c.H == 1 else 2) * (1 if c.W == 1 else 2)
    assert new_plan.endswith(" igemm3f[stride-2 merged]") and ("tile %s," % c.tile) in new_plan and (" %d classes:" % n_cls) in new_plan, new_plan
    steps = [int(s) for s in re.findall(r"steps (\d+)", new_plan)]
    red = (c.cout + 31) // 32
    assert steps == sorted(steps, reverse=True), new_plan          # heaviest class first
    if c.k == 3 and n_cls == 4:
        assert steps == [4 * red, 2 * red, 2 * red, red], new_plan
    if c.k == 1:
        assert steps == [red] + [0] * (n_cls - 1), new_plan
    old_plan = planned(ctx, d, ops.PLAN_BWD_DATA, _forms(c))
    assert len(old_plan) == n_cls and all(("tile %s " % c.tile) in h for h in old_plan if "class_fill" not in h), old_plan
    w, gy, gp, add, ap, msk, mp = _operands(ctx, c)
    Wn = collections.namedtuple("Wn", "k cin cout")(c.k, c.cin, c.cout)
    _, wdg, _ = T._weights3(ctx, Wn, d, w.numpy())
    new = _call(ops.conv_bwd_data3_s2, ctx, c, d, wdg, gy, gp, add, ap, msk, mp)
    new.check(c.cin, "merged data gradient")
    old = _call(ops.conv_bwd_data3, ctx, c, d, wdg, gy, gp, add, ap, msk, mp)
    # 1. byte for byte, guard bands included
    if c.form == "ff":
        assert torch.equal(new.full.view(torch.int32), old.full.view(torch.int32)), c.name
    else:
        assert torch.equal(new.pfull[0], old.pfull[0]) and torch.equal(new.pfull[1], old.pfull[1]), c.name
    # 2. float64 on the operands as the launch reads them (a plane-stored operand IS the planes' value)
    pp = c.form == "pp"
    gv = (T._merged(gp) if pp else gy).double().cpu()[:, :c.cout].reshape(c.B, *_out_hw(c), c.cout)
    ref = _f64_dgrad(c, w, gv)
    if c.addend:
        ref = ref + (T._merged(ap) if c.addend == "planes" else add).double().cpu()
    if c.mask:
        ref = ref * (msk.cpu() > 0)
    got = T._merged(new.pl) if pp else new.t
    T._close(got.cpu(), ref, 1e-4, "%s vs float64" % c.name)


def test_refusals_come_before_any_launch(ctx):
    """stride 1, two levels, mixed operand forms, options that are not this call's: PP_ERR_ARG, and dx keeps its sentinel"""
    from pyrapose_amd import ops
    from pyrapose_amd._lib import lib
    PP_ERR_ARG = -1
    c = Case("refuse", 2, 6, 5, 64, 32, 1, 0, "pp", None, False, "64x64")
    w, gy, gp, add, ap, msk, mp = _operands(ctx, c)
    Wn = collections.namedtuple("Wn", "k cin cout")(c.k, c.cin, c.cout)
    s2 = _desc(c)
    _, wdg, _ = T._weights3(ctx, Wn, s2, w.numpy())
    s1 = ops.make_conv_desc(c.B, [(3, 3)], [(3, 3)], c.cin, c.cout, 1, 1, 0, 0, c.cin, 32, 32)                      # the rows of gy as a stride-1 conv
    two = ops.make_conv_desc(1, [(3, 3), (3, 3)], [(3, 3), (3, 3)], c.cin, c.cout, 1, 1, 0, 0, c.cin, 32, 32)       # ... as two levels
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    out = T.Guarded(c.B * c.H * c.W, c.cin, 64, True, True)

    def call(d, dy, dyp, dx, dxp, opts=None):
        rc = lib.pp_conv2d_nhwc_bwd_data_s2_bf16x3(ctx.handle, C.byref(d), P(dy), P(dyp[0] if dyp else None), P(dyp[1] if dyp else None), P(wdg[0]),
                                                   P(wdg[1]), None, 0, None, 0, P(dx), P(dxp[0] if dxp else None), P(dxp[1] if dxp else None), opts)
        torch.cuda.synchronize()
        return rc
    assert call(s1, None, gp, None, out.pl) == PP_ERR_ARG            # stride 1
    assert call(two, None, gp, None, out.pl) == PP_ERR_ARG           # two levels
    assert call(s2, gy, None, None, out.pl) == PP_ERR_ARG            # f32 in, planes out
    assert call(s2, None, gp, out.t, None) == PP_ERR_ARG             # planes in, f32 out
    assert call(s2, None, gp, out.t, out.pl) == PP_ERR_ARG           # both output forms
    flags = torch.zeros((64,), dtype=torch.uint8, device="cuda")
    lst = torch.zeros((64,), dtype=torch.int32, device="cuda")
    assert call(s2, None, gp, None, out.pl, ops._conv_opts(skip=(flags, lst))) == PP_ERR_ARG      # row-block skip: not an option of this call
    cap = ops.new_planes(gy.shape[0], gy.shape[1])
    assert call(s2, gy, None, out.t, None, ops._conv_opts(capture=cap)) == PP_ERR_ARG             # split capture: neither
    bits = out.full.view(torch.int32)
    assert bool((bits == T.NAN_BITS).all()) and all(bool((T._flat(p) == 0x7fc0).all()) for p in out.pfull)
    assert call(s2, None, gp, None, out.pl) == 0                     # and the call the route takes
    out2 = T.Guarded(c.B * c.H * c.W, c.cin, 64, True, False)
    assert call(s2, gy, None, out2.t, None) == 0


def test_training_plan_gradients_are_bit_identical_on_both_routes(monkeypatch):
    """B = 1 at 64 x 96 (the small training plan of the suite): the backward once with the merged route and once under
    PP_CONV3_S2MERGED=0, in one process; every gradient a stride-2 data-gradient launch writes is the same bytes"""
    from pyrapose_amd import arch
    from pyrapose_amd.engine import Engine
    from pyrapose_amd.runtime import default_context
    from tests.test_gpu_model import random_targets, synth_input
    B, H, W, Cn = 1, 64, 96, 5
    rng = np.random.default_rng(3)
    Wt = arch.init_weights(Cn, seed=0)
    x = synth_input(rng, B, H, W)
    grads, tg = {}, None
    for route, env in (("merged", None), ("classes", "0")):
        if env is None:
            monkeypatch.delenv("PP_CONV3_S2MERGED", raising=False)
        else:
            monkeypatch.setenv("PP_CONV3_S2MERGED", env)
        eng = Engine(default_context(), Cn, B, H, W, weights=Wt, train=True)
        if tg is None:
            tg = [torch.from_numpy(t).cuda() for t in random_targets(rng, B, eng.N, eng.M3, Cn)]
        eng.set_targets(*tg)
        eng.forward(torch.from_numpy(x).cuda())
        eng.loss_and_backward()
        torch.cuda.synchronize()
        assert eng._s2_grads and all(r == route for _, _, r in eng._s2_grads), [(n, r) for n, _, r in eng._s2_grads]
        grads[route] = [(n, [p.clone() for p in g.pl] if g.pl is not None else [g.t.clone()]) for n, g, _ in eng._s2_grads]
        eng.close()
    names = [n for n, _ in grads["merged"]]
    assert names == [n for n, _ in grads["classes"]]
    # the four stage entries of res4a / res5a and the two FPN down-convs (res3a's input is frozen)
    assert len(names) == 6, names
    for (n, a), (_, b) in zip(grads["merged"], grads["classes"]):
        for pa, pb in zip(a, b):
            assert torch.equal(pa, pb), n
