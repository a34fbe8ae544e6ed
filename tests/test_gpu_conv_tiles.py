"""GPU: every tile of the convolution kernels that a training step launches, against float64.

tests/test_gpu_conv.py and tests/test_gpu_planes.py run one CASES table whose row spaces are so small that the planner gives
every forward and data-gradient launch the 64 x 64 tile.  The product runs 128 x 128, 128 x 64, 64 x 128 and 256 x 128 tiles, many
with a reduction split.  This module holds ONE table, TABLE, of launches at those tiles; every row DECLARES the kernel family,
tile and split count it must get, and

    a case asserts its plan before it launches

(planned() of tests/test_gpu_planes.py: the plan of that exact call on this context): a mismatch is a failure, never a skip.  The
host-only ledger tests/test_conv_tile_cases_cpu.py checks the same declarations without a device and that the table covers every
plan signature pinned in tests/golden/conv_plans.txt.

Shapes are the smallest that hold a tile's edges: M = BM + 1 (a second row tile with one live row), M = 2 (BM - 2) + 1 (the two-row
overlap of the row-reuse tiles across three tiles), a level wider than BM - 2 (a row's +-1-row neighbours live in another tile),
image and level boundaries inside a tile, cout = 144 / 117 (ragged column tiles), cin = 96 (three 32-channel chunks), and for the
data gradient cout = 80 (the reduction rounded up to 96).  Only switches that are read at every launch are set.

Bounds (the suite's own): bf16x3 / P16 against float64 1e-4 of the output's max magnitude (dW 1e-4, bias gradient 5e-5); the same
entry point at the 64 x 64 tile -- same products, another f32 summation order -- 2e-6, or one remainder step of the plane format
(4e-5 / 8e-5) where the output is re-encoded into planes; the f32 kernels of conv.hip 2e-5 (dW 5e-5).  Outputs sit between guard
bands of BM rows filled with a sentinel that must come back bit-unchanged, and no live element may keep the sentinel."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_conv import _cat_rows, _device_weight, ref_conv, rel_err, tf_same
from tests.test_gpu_planes import planned

pytestmark = pytest.mark.gpu

# name; kind: "gemm" (bf16x3 forward / data gradient), "wgrad" (bf16x3 weight gradient), "f32" (conv.hip, no plan text);
# pass_: "fwd" / "dgrad" / "wgrad"; the descriptor: B images, levels, cin, cout, k, stride, pad ("same" or a number), ld_y (None: cout
# rounded up to 32); forms: operand forms, a subset of {"pin", "pout", "f32out", "capture", "list"} (no "pout" means f32 out);
# env: the per-launch switches; ws: scratch bytes; DECLARED: family, tile "BMxBN", splits (the number in the plan line's head)
Row = collections.namedtuple("Row", "name kind pass_ B shapes cin cout k stride pad ld_y forms env ws family tile splits")

TILE_ENV = {"64x64": "1,1", "64x128": "1,2", "128x64": "2,1", "128x128": "2,2", "256x128": "4,2"}
BIG_TILES = ("64x128", "128x64", "128x128", "256x128")
FORMS = {"ff": (), "pf": ("pin",), "fp": ("pout",), "pp": ("pin", "pout"), "cap": ("capture",)}
MB = 1 << 20


def _bm(tile):
    return int(tile.split("x")[0])


def _x_family(form, tile, splits=1):
    """family of a 3x3 stride-1 'same' launch: the 256-row tile has the row-reuse kernel for plane-stored operands without capture only"""
    if form == "cap":
        return "igemm3x[capture]" if _bm(tile) <= 128 else "igemm3f"
    pin, pout = "pin" in FORMS[form], "pout" in FORMS[form] and splits == 1   # split-K: partial sums to scratch, the finish writes planes
    if _bm(tile) == 256 and not pin:
        return "igemm3f"
    return "igemm3x[%s->%s]" % ("planes" if pin else "f32", "planes" if pout else "f32")


def _gemm_rows():
    rows = []

    def add(name, pass_, B, shapes, cin, cout, k, stride, pad, ld_y, form, tile, family, splits=1, ws=0):
        env = {"PP_CONV3_TILE": TILE_ENV[tile]}
        if splits > 1 or ws:
            env["PP_CONV3_SPLITS"] = str(splits)
        rows.append(Row("%s_%s_%s_%s%s" % (name, pass_, form, tile, "_split%d" % splits if splits > 1 else ""), "gemm", pass_, B, shapes, cin, cout, k, stride, pad, ld_y, FORMS[form], env, ws,
                        family, tile, splits))

    for tile in BIG_TILES:
        bm = _bm(tile)
        # ---- igemm3f: 1x1 stride 1 (M = BM + 1; levels inside a tile) and the 3x3 stride-2 forward (BM + 1 output rows)
        one = {64: [(5, 13)], 128: [(3, 43)], 256: [(16, 16), (1, 1)]}[bm]
        add("pw_m_plus1", "fwd", 1, one, 96, 117, 1, 1, 0, 128, "ff", tile, "igemm3f")
        add("pw_levels", "fwd", 2 if bm < 256 else 4, [(9, 12), (5, 6), (3, 3), (1, 1)], 64, 144, 1, 1, 0, 160, "pp", tile, "igemm3f")
        add("pw_levels", "dgrad", 2 if bm < 256 else 4, [(9, 12), (5, 6), (3, 3), (1, 1)], 160, 80, 1, 1, 0, 96, "pf", tile, "igemm3f")
        add("pw_m_plus1", "dgrad", 1, one, 96, 80, 1, 1, 0, 96, "fp", tile, "igemm3f")
        add("pw_images", "fwd", 7 if bm < 256 else 11, [(5, 5)], 32, 144, 1, 1, 0, 160, "fp", tile, "igemm3f")
        add("pw_images", "dgrad", 7 if bm < 256 else 11, [(5, 5)], 160, 144, 1, 1, 0, 160, "pp", tile, "igemm3f")
        s2_in = {64: (9, 25), 128: (5, 85), 256: (2, 513)}[bm]
        add("down_m_plus1", "fwd", 1, [s2_in], 96, 144, 3, 2, "same", 160, "pf", tile, "igemm3f")
        add("down_m_plus1", "fwd", 1, [s2_in], 64, 117, 3, 2, "same", 128, "ff", tile, "igemm3f")
        # ---- igemm3f[parity class]: the stride-2 data gradient, 1x1 and 3x3, odd extents (four unequal classes) and even ones
        n_odd, n_even = {64: (2, 2), 128: (2, 3), 256: (3, 6)}[bm]
        add("s2_3x3_odd", "dgrad", n_odd, [(17, 23)], 64, 80, 3, 2, "same", 96, "pp", tile, "igemm3f[parity class]")
        add("s2_3x3_even", "dgrad", n_even, [(12, 16)], 64, 80, 3, 2, "same", 96, "ff", tile, "igemm3f[parity class]")
        add("s2_1x1_odd", "dgrad", 2 * n_odd, [(9, 13)], 160, 80, 1, 2, 0, 96, "ff", tile, "igemm3f[parity class]")
        add("s2_1x1_even", "dgrad", n_even, [(12, 16)], 160, 80, 1, 2, 0, 96, "pp", tile, "igemm3f[parity class]")
        # ---- igemm3x (3x3 stride 1 "same"), every operand form, forward and data gradient
        three = {64: [(5, 25)], 128: [(11, 23)], 256: [(22, 23), (1, 3)]}[bm]          # M = 2 (BM - 2) + 1
        wide = [(3, {64: 66, 128: 130, 256: 258}[bm])]                                   # a level wider than BM - 2
        last1 = {64: [(7, 9), (1, 1)], 128: [(9, 14), (1, 1)], 256: [(15, 17), (1, 1)]}[bm]  # M = (BM - 2) + 1
        images = 7 if bm < 256 else 11
        levels = [(9, 12), (5, 6), (3, 3), (1, 1)]
        nl = 2 if bm < 256 else 4
        add("x_three_tiles", "fwd", 1, three, 96, 117, 3, 1, "same", 128, "ff", tile, _x_family("ff", tile))
        add("x_wide", "fwd", 1, wide, 32, 144, 3, 1, "same", 160, "pf", tile, _x_family("pf", tile))
        add("x_images", "fwd", images, [(5, 5)], 64, 144, 3, 1, "same", 160, "fp", tile, _x_family("fp", tile))
        add("x_levels", "fwd", nl, levels, 64, 144, 3, 1, "same", 160, "pp", tile, _x_family("pp", tile))
        add("x_last_row", "fwd", 1, last1, 64, 64, 3, 1, "same", 64, "cap", tile, _x_family("cap", tile))
        add("x_levels", "dgrad", nl, levels, 64, 80, 3, 1, "same", 96, "ff", tile, _x_family("ff", tile))
        add("x_three_tiles", "dgrad", 1, three, 160, 80, 3, 1, "same", 96, "pf", tile, _x_family("pf", tile))
        add("x_wide", "dgrad", 1, wide, 64, 80, 3, 1, "same", 96, "fp", tile, _x_family("fp", tile))
        add("x_images", "dgrad", images, [(5, 5)], 96, 144, 3, 1, "same", 160, "pp", tile, _x_family("pp", tile))
        add("x_wide", "dgrad", 1, wide, 64, 80, 3, 1, "same", 96, "cap", tile, _x_family("cap", tile))
    # ---- split-K: the slices of igemm3x[planes->f32] / igemm3f plus splitk_finish_kernel writing f32 and planes
    for tile in ("128x128", "128x64"):
        for splits in (2, 3):
            # 3 kernel rows x 3 chunks = 9 (kernel row, chunk) groups; 1x1 with cin 160 = 5 steps: neither 2 nor 3 divides it
            add("split_x_levels", "fwd", 2, [(9, 12), (5, 6), (3, 3), (1, 1)], 96, 144, 3, 1, "same", 160, "pp", tile, _x_family("pp", tile, splits),
                splits, 8 * MB)
            add("split_x_three_tiles", "fwd", 1, [(11, 23)], 96, 117, 3, 1, "same", 128, "pf", tile, _x_family("pf", tile, splits), splits, 8 * MB)
            add("split_x_levels", "dgrad", 2, [(9, 12), (5, 6), (3, 3), (1, 1)], 160, 80, 3, 1, "same", 96, "pp", tile,
                _x_family("pp", tile, splits), splits, 8 * MB)
            add("split_x_wide", "dgrad", 1, [(3, 130)], 64, 80, 3, 1, "same", 96, "pf", tile, _x_family("pf", tile, splits), splits, 8 * MB)
            add("split_pw_m_plus1", "fwd", 1, [(3, 43)], 160, 144, 1, 1, 0, 160, "pp", tile, "igemm3f", splits, 8 * MB)
    # ---- the remaining plan signatures of the pinned bench step (tests/test_conv_tile_cases_cpu.py names what each covers)
    add("split_pw_m_plus1", "fwd", 1, [(5, 13)], 160, 144, 1, 1, 0, 160, "pp", "64x128", "igemm3f", 3, 8 * MB)
    add("split_pw_m_plus1", "fwd", 1, [(5, 13)], 160, 144, 1, 1, 0, 160, "pp", "64x64", "igemm3f", 3, 8 * MB)
    add("split_pw_m_plus1", "dgrad", 1, [(5, 13)], 96, 144, 1, 1, 0, 160, "pp", "64x128", "igemm3f", 3, 8 * MB)
    add("split_down", "fwd", 1, [(5, 85)], 96, 144, 3, 2, "same", 160, "pp", "128x128", "igemm3f", 3, 8 * MB)
    add("split_down", "fwd", 1, [(9, 25)], 96, 144, 3, 2, "same", 160, "pp", "64x64", "igemm3f", 3, 8 * MB)
    add("split_x_three_tiles", "fwd", 1, [(5, 25)], 96, 144, 3, 1, "same", 160, "pp", "64x128", "igemm3x[planes->f32]", 3, 8 * MB)
    add("split_x_three_tiles", "fwd", 1, [(5, 25)], 96, 144, 3, 1, "same", 160, "pp", "64x64", "igemm3x[planes->f32]", 3, 8 * MB)
    add("split_x_three_tiles", "dgrad", 1, [(5, 25)], 96, 80, 3, 1, "same", 96, "pp", "64x128", "igemm3x[planes->f32]", 3, 8 * MB)
    add("split_x_three_tiles", "dgrad", 1, [(5, 25)], 96, 80, 3, 1, "same", 96, "pp", "64x64", "igemm3x[planes->f32]", 3, 8 * MB)
    # the 64 x 64 launches that stay: one per family (every other row uses them as its comparison partner)
    add("pw_m_plus1", "fwd", 1, [(5, 13)], 96, 144, 1, 1, 0, 160, "pp", "64x64", "igemm3f")
    add("pw_s2", "fwd", 2, [(9, 13)], 96, 144, 1, 2, 0, 160, "pp", "64x64", "igemm3f")
    add("pw_m_plus1", "dgrad", 1, [(5, 13)], 96, 144, 1, 1, 0, 160, "pp", "64x64", "igemm3f")
    add("s2_3x3_odd", "dgrad", 2, [(17, 23)], 64, 80, 3, 2, "same", 96, "pp", "64x64", "igemm3f[parity class]")
    add("s2_1x1_odd", "dgrad", 4, [(9, 13)], 160, 80, 1, 2, 0, 96, "pp", "64x64", "igemm3f[parity class]")
    add("pw_s2", "fwd", 2, [(9, 13)], 96, 144, 1, 2, 0, 160, "pp", "64x128", "igemm3f")
    add("pw_s2", "fwd", 4, [(9, 13)], 96, 144, 1, 2, 0, 160, "pp", "128x128", "igemm3f")
    # the sparse data gradient over the listed 32-row blocks (tile 128 x 128 by PP_SPARSE_DGRAD's default), unsplit and split two ways
    rows.append(Row("rowlist_dgrad_pp_128x128", "gemm", "dgrad", 2, [(20, 26), (10, 13), (5, 7)], 64, 192, 3, 1, "same", 192, ("pin", "pout", "list"),
                    {}, 0, "igemm3f[row list]", "128x128", 1))
    rows.append(Row("rowlist_split_dgrad_pp_128x128", "gemm", "dgrad", 2, [(20, 26), (10, 13), (5, 7)], 64, 192, 3, 1, "same", 192,
                    ("pin", "pout", "list"), {}, 16 * MB, "igemm3f[row list]", "128x128", 2))
    return rows


def _wgrad_rows():
    rows = []

    def add(name, B, shapes, cin, cout, k, stride, forms, family, tile, splits, env=None, ws=0):
        rows.append(Row(name, "wgrad", "wgrad", B, shapes, cin, cout, k, stride, "same" if k == 3 else 0, None, forms, dict(env or {}), ws, family,
                        tile, splits))

    # ---- wgrad3f: its four tiles by channel counts x its four operand forms; every level has at least 32 cells (fast 1); the level
    # boundary (row 216) is not on a 32-row block
    two = [(9, 12), (6, 7)]
    # (cout 144 alone gets 128 x 64 -- three column tiles, 192 columns, against 256 --: PP_WGRAD3_TILE keeps the 128 x 128 tile on it,
    # whose second column tile is then 16 wide)
    T22 = {"PP_WGRAD3R": "0", "PP_WGRAD3_TILE": "2,2"}
    for cin, cout, tile in ((64, 64, "64x64"), (64, 65, "64x128"), (128, 64, "128x64"), (128, 144, "128x128")):
        for forms, fam in (((), "wgrad3f[f32]"), (("pin",), "wgrad3f[planes]"), (("list",), "wgrad3f[f32, list]"), (("pin", "list"), "wgrad3f[planes, list]")):
            add("w_%dx%d_%s" % (cin, cout, "_".join(forms) or "f32"), 2, two, cin, cout, 3, 1, forms, fam, tile, 1, T22 if cout == 144 else {"PP_WGRAD3R": "0"})
    # ---- row-split edges (PP_WGRAD3_SPLITS=2): M = 2 * 32 * 9 exactly, that + 1, M no multiple of 32, a level boundary off the 32-row
    # blocks; with atomics, and with PP_WGRAD3_DETERMINISTIC=1 + scratch (slices + wgrad_finish_kernel)
    for nm, shapes in (("m576", [(24, 24)]), ("m577", [(16, 34), (3, 11)]), ("m600", [(24, 25)]), ("m599_levels", [(20, 25), (9, 11)])):
        for det in (0, 1):
            env = {"PP_WGRAD3R": "0", "PP_WGRAD3_SPLITS": "2"}
            if det:
                env["PP_WGRAD3_DETERMINISTIC"] = "1"
            add("w_split2_%s_%s" % (nm, "slices" if det else "atomics"), 1, shapes, 128, 64, 3, 1, ("pin",) if det else (), "wgrad3f[planes]" if det
                else "wgrad3f[f32]", "128x64", 2, env, 4 * MB if det else 0)
    S2 = dict(T22, PP_WGRAD3_SPLITS="2")
    add("w_split2_1x1_s2", 4, [(24, 25)], 128, 144, 1, 2, ("pin",), "wgrad3f[planes]", "128x128", 2, S2)       # 4 x 12 x 13 = 624 rows
    add("w_split2_3x3_s2", 4, [(24, 25)], 128, 144, 3, 2, ("pin",), "wgrad3f[planes]", "128x128", 2, S2)
    add("w_split2_1x1_s1", 1, [(24, 25)], 128, 144, 1, 1, ("pin",), "wgrad3f[planes]", "128x128", 2, S2)
    add("w_split2_3x3_s1", 1, [(20, 25), (9, 11)], 128, 144, 3, 1, ("pin",), "wgrad3f[planes]", "128x128", 2, S2)
    add("w_split2_list_128x128", 1, [(20, 25), (9, 11)], 128, 144, 3, 1, ("pin", "list"), "wgrad3f[planes, list]", "128x128", 2, S2)
    add("w_split2_list_128x64", 1, [(20, 25), (9, 11)], 128, 64, 3, 1, ("pin", "list"), "wgrad3f[planes, list]", "128x64", 2,
        {"PP_WGRAD3R": "0", "PP_WGRAD3_SPLITS": "2"})
    # ---- the non-fast wgrad3 (a level under 32 cells), at two of its tiles, both operand forms
    small = [(9, 12), (5, 6)]
    for cin, cout, tile in ((64, 64, "64x64"), (128, 144, "128x128")):
        for forms in ((), ("pin",)):
            add("w_slow_%dx%d_%s" % (cin, cout, "_".join(forms) or "f32"), 2, small, cin, cout, 3, 1, forms, "wgrad3", tile, 1,
                T22 if cout == 144 else {"PP_WGRAD3R": "0"})
    # ---- wgrad3w / wgrad3r (PP_WGRAD3R=2 / 1): cin 128, cout 144; one narrow level (width 2 dense, 12 over a list) and three levels whose
    # later levels start on 32-row blocks (rows 512 and 640 / 704)
    for r, fam in (("2", "wgrad3w"), ("1", "wgrad3r")):
        add("%s_narrow" % fam, 3, [(40, 2)], 128, 144, 3, 1, ("pin",), fam, "128x128", 2, {"PP_WGRAD3R": r})
        add("%s_three_levels" % fam, 2, [(16, 16), (8, 8), (4, 4)], 128, 144, 3, 1, ("pin",), fam, "128x128", 3, {"PP_WGRAD3R": r})
    add("wgrad3r_list_narrow", 3, [(20, 12)], 128, 144, 3, 1, ("pin", "list"), "wgrad3r", "128x128", 3, {"PP_WGRAD3R": "1"})
    add("wgrad3r_list_three_levels", 2, [(16, 16), (8, 12), (4, 12)], 128, 144, 3, 1, ("pin", "list"), "wgrad3r", "128x128", 4, {"PP_WGRAD3R": "1"})
    return rows


def _f32_rows():
    """conv.hip: PP_CONV_TILE is read per launch; these kernels take no plan text, so the declared tile is the switch itself (the
    weight gradient's tile follows the channel counts; the stem, cin == 4, has the 128 x 64 and the 128 x 128 tile)"""
    rows = []
    for tile in BIG_TILES:
        bm = _bm(tile)
        env = {"PP_CONV_TILE": TILE_ENV[tile]}
        one = {64: [(5, 13)], 128: [(3, 43)], 256: [(16, 16), (1, 1)]}[bm]
        wide = [(3, {64: 66, 128: 130, 256: 258}[bm])]
        nl = 2 if bm < 256 else 4
        for pass_ in ("fwd", "dgrad"):
            rows.append(Row("f32_m_plus1_%s_%s" % (pass_, tile), "f32", pass_, 1, one, 64, 117 if pass_ == "fwd" else 80, 1, 1, 0, 128, (), env, 0,
                            "igemm", tile, 1))
            rows.append(Row("f32_levels_%s_%s" % (pass_, tile), "f32", pass_, nl, [(9, 12), (5, 6), (3, 3), (1, 1)], 96 if pass_ == "fwd" else 64, 144, 3, 1,
                            "same", 144, (), env, 0, "igemm", tile, 1))
            rows.append(Row("f32_wide_%s_%s" % (pass_, tile), "f32", pass_, 1, wide, 64, 80, 3, 1, "same", 80, (), env, 0, "igemm", tile, 1))
        rows.append(Row("f32_s2_odd_dgrad_%s" % tile, "f32", "dgrad", nl, [(17, 23)], 64, 80, 3, 2, "same", 80, (), env, 0, "igemm", tile, 1))
        rows.append(Row("f32_s2_even_fwd_%s" % tile, "f32", "fwd", nl, [(12, 16)], 64, 144, 3, 2, "same", 144, (), env, 0, "igemm", tile, 1))
    for cin, cout, tile in ((64, 64, "64x64"), (64, 65, "64x128"), (128, 64, "128x64"), (128, 144, "128x128")):
        rows.append(Row("f32_wgrad_%dx%d" % (cin, cout), "f32", "wgrad", 2, [(9, 12), (5, 6), (1, 1)], cin, cout, 3, 1, "same", None, (), {}, 0, "wgrad", tile, 1))
    return rows


GEMM_ROWS, WGRAD_ROWS, F32_ROWS = _gemm_rows(), _wgrad_rows(), _f32_rows()
TABLE = GEMM_ROWS + WGRAD_ROWS + F32_ROWS
assert len({r.name for r in TABLE}) == len(TABLE)


# ---- the plan of a row, and its declaration ----
def plan_pass(row):
    from pyrapose_amd import ops
    return {"fwd": ops.PLAN_FWD, "dgrad": ops.PLAN_BWD_DATA, "wgrad": ops.PLAN_BWD_WEIGHT}[row.pass_]


def plan_forms(row):
    from pyrapose_amd import ops
    bits = {"pin": ops.PLAN_PLANES_IN, "pout": ops.PLAN_PLANES_OUT, "f32out": ops.PLAN_F32_OUT, "capture": ops.PLAN_CAPTURE, "list": ops.PLAN_LIST}
    return sum(bits[f] for f in row.forms)


def geometry(row):
    """(out_shapes, pad_t, pad_l, ld_y, ld_w) of a row's descriptor"""
    k, s = row.k, row.stride
    if row.pad == "same":
        out = [(-(-h // s), -(-w // s)) for h, w in row.shapes]
        pt, pl = tf_same(row.shapes[0][0], k, s)[0], tf_same(row.shapes[0][1], k, s)[0]
    else:
        out = [((h + 2 * row.pad - k) // s + 1, (w + 2 * row.pad - k) // s + 1) for h, w in row.shapes]
        pt = pl = row.pad
    ld_y = row.ld_y or (row.cout + 31) // 32 * 32
    return out, pt, pl, ld_y, (row.cout + 15) // 16 * 16


def make_desc(row):
    from pyrapose_amd import ops
    out, pt, pl, ld_y, ld_w = geometry(row)
    return ops.make_conv_desc(row.B, row.shapes, out, row.cin, row.cout, row.k, row.stride, pt, pl, row.cin, ld_y, ld_w)


def assert_plan(row, heads, tile=None, splits=None, family=None):
    """heads: the plan lines of the call (without their detail part).  Every GEMM line must be the declared family at the declared tile
    with the declared split count (the classes of a stride-2 data gradient are several lines; a class without taps only fills)."""
    import re
    tile, splits, family = tile or row.tile, row.splits if splits is None else splits, row.family if family is None else family
    gemm = [h for h in heads if "class_fill" not in h]
    assert gemm, heads
    for h in gemm:
        if row.pass_ == "wgrad":
            if row.family in ("wgrad3r", "wgrad3w"):
                assert h.endswith(" " + family) and re.search(r"splits (\d+) ", h).group(1) == str(splits), (row.name, h)
            else:
                assert h.endswith(" " + family) and ("tile %s " % tile) in h and (" splits %d " % splits) in h, (row.name, h)
                assert ("fast 0" in h) == (family == "wgrad3"), (row.name, h)
        else:
            assert ("tile %s " % tile) in h and (" splits %d " % splits) in h, (row.name, h)
            if family != "*":
                assert h.endswith(" " + family), (row.name, h)


# ---- device side ----
FMT = [0]


@pytest.fixture(scope="module", params=[0, 1], ids=["bf16x3", "f16c8"])
def ctx(request):
    from pyrapose_amd.runtime import default_context
    FMT[0] = request.param
    return default_context().twin(request.param)


@pytest.fixture(scope="module")
def fctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


def _split(ctx, t):
    from pyrapose_amd import ops
    hi, lo = ops.new_planes(t.shape[0], t.shape[1])
    ops.split_planes3(ctx, t, hi, lo)
    return hi, lo


def _merged(pl):
    from pyrapose_amd import ops
    return ops.planes_to_f32(pl, FMT[0])


def _flat(t):
    return t.reshape(t.shape[0], -1)


NAN_BITS = 0x7fc00000


class Guarded(object):
    """an output of `rows` rows between two bands of `band` rows: f32 filled with NaN (0x7fc00000) and / or planes filled with 0x7fc0"""

    def __init__(self, rows, ld, band, f32, planes):
        from pyrapose_amd import ops
        self.rows, self.band = rows, band
        self.full = torch.full((rows + 2 * band, ld), float("nan"), dtype=torch.float32, device="cuda") if f32 else None
        self.pfull = ops.new_planes(rows + 2 * band, ld, fill=0x7fc0) if planes else None
        self.t = self.full[band: band + rows] if f32 else None
        self.pl = (self.pfull[0][band: band + rows], self.pfull[1][band: band + rows]) if planes else None

    def check(self, cols, what):
        """the bands bit-unchanged, no sentinel left in the live [:, :cols] block"""
        b, r = self.band, self.rows
        if self.full is not None:
            bits = self.full.view(torch.int32)
            assert bool((bits[:b] == NAN_BITS).all()) and bool((bits[b + r:] == NAN_BITS).all()), "%s: f32 guard band written" % what
            assert not bool(torch.isnan(self.t[:, :cols]).any()), "%s: live f32 element left unwritten" % what
        if self.pfull is not None:
            for p in self.pfull:
                f = _flat(p)
                assert bool((f[:b] == 0x7fc0).all()) and bool((f[b + r:] == 0x7fc0).all()), "%s: plane guard band written" % what
                assert not bool((f[b: b + r, :cols] == 0x7fc0).any()), "%s: live plane element left unwritten" % what


def _data(row, seed=7):
    """operands of a row on the host, float64 (deterministic per row name)"""
    rng = np.random.default_rng([seed, sum(map(ord, row.name))])
    out, pt, pl, ld_y, ld_w = geometry(row)
    k = row.k
    xs = [torch.as_tensor(rng.standard_normal((row.B, h, w, row.cin)), dtype=torch.float64) for h, w in row.shapes]
    w = rng.standard_normal((k, k, row.cin, row.cout)) / np.sqrt(k * k * row.cin)
    bias = rng.standard_normal((row.cout,))
    gys = [torch.as_tensor(rng.standard_normal((row.B, h, ww, row.cout)), dtype=torch.float64) for h, ww in out]
    return rng, xs, w, bias, gys


def _f64_conv(row, xs, w):
    """per level NHWC float64 conv of xs (autograd-capable), no bias"""
    k, s = row.k, row.stride
    wt = w.permute(3, 2, 0, 1)
    outs = []
    for t in xs:
        xt = t.permute(0, 3, 1, 2)
        if row.pad == "same":
            a, b_, _ = tf_same(xt.shape[2], k, s)
            c_, e_, _ = tf_same(xt.shape[3], k, s)
        else:
            a = b_ = c_ = e_ = row.pad
        outs.append(F.conv2d(F.pad(xt, (c_, e_, a, b_)), wt, None, stride=s).permute(0, 2, 3, 1))
    return outs


def _rows2d(ts, c):
    return torch.cat([t.reshape(-1, c) for t in ts], dim=0)


def _band(row):
    return max(_bm(row.tile), 64)


def _weights3(ctx, row, d, w):
    from pyrapose_amd import ops
    wd, ld_w = _device_weight(w, row.cout)
    taps, cred = row.k * row.k, (row.cout + 31) // 32 * 32
    u16 = dict(dtype=torch.int16, device="cuda")
    fh, fl = torch.zeros((taps, row.cout, row.cin), **u16), torch.zeros((taps, row.cout, row.cin), **u16)
    dh, dl = torch.zeros((taps, row.cin, cred), **u16), torch.zeros((taps, row.cin, cred), **u16)
    ops.conv_split_weights3(ctx, d, wd, fh, fl, dh, dl)
    return (fh, fl), (dh, dl), ld_w


def _set_env(monkeypatch, env):
    for k in ("PP_CONV3_TILE", "PP_CONV3_SPLITS", "PP_WGRAD3_TILE", "PP_WGRAD3_SPLITS", "PP_WGRAD3R", "PP_WGRAD3_DETERMINISTIC", "PP_CONV_TILE",
              "PP_CONV3_DMA"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


PLANE_TOL = {0: 4e-5, 1: 8e-5}


def _close(got, want, tol, what):
    e = rel_err(got.detach().cpu().numpy(), want.detach().cpu().numpy())
    print("%s: %.3g (bound %.3g)" % (what, e, tol))
    assert e <= tol, (what, e, tol)


def _forward(ctx, row, d, monkeypatch, env, ws, declared, ops_in):
    """one forward launch under env; returns (values, Guarded out, Guarded capture or None)"""
    from pyrapose_amd import ops
    x, xp, wf, bias, res, rp, rows_out, ld_y = ops_in
    pin, pout, cap = "pin" in row.forms, "pout" in row.forms, "capture" in row.forms
    _set_env(monkeypatch, env)
    ctx.set_workspace(ws)
    try:
        if ws:
            ctx.workspace.fill_(float("nan"))    # any contents: every word a launch reads it has written first
        assert_plan(row, planned(ctx, d, ops.PLAN_FWD, plan_forms(row)), **declared)
        out = Guarded(rows_out, ld_y, _band(row), not pout, pout)
        capg = Guarded(x.shape[0], x.shape[1], _band(row), False, True) if cap else None
        ops.conv_fwd3(ctx, d, None if pin else x, wf[0], wf[1], bias, None if (pin and pout) else res, True, out.t, x_planes=xp if pin else None,
                      y_planes=out.pl, x_capture=capg.pl if cap else None, res_planes=rp if (pin and pout) else None)
        torch.cuda.synchronize()
    finally:
        ctx.set_workspace(0)
    val = _merged(out.pl) if pout else out.t
    return val[:, :row.cout].clone(), out, capg


def _dgrad(ctx, row, d, monkeypatch, env, ws, declared, ops_in):
    from pyrapose_amd import ops
    gy, gp, wd_, add, ap, msk, mp, rows_in, skip = ops_in
    pin, pout, cap, lst = "pin" in row.forms, "pout" in row.forms, "capture" in row.forms, "list" in row.forms
    _set_env(monkeypatch, env)
    ctx.set_workspace(ws)
    try:
        if ws:
            ctx.workspace.fill_(float("nan"))
        assert_plan(row, planned(ctx, d, ops.PLAN_BWD_DATA, plan_forms(row)), **declared)
        out = Guarded(rows_in, row.cin, _band(row), not pout, pout)
        capg = Guarded(gy.shape[0], gy.shape[1], _band(row), False, True) if cap else None
        planes_ep = pin and pout
        ops.conv_bwd_data3(ctx, d, None if pin else gy, wd_[0], wd_[1], None if planes_ep else add, None if planes_ep else msk, out.t,
                           dy_planes=gp if pin else None, dx_planes=out.pl, dy_capture=capg.pl if cap else None,
                           dy_skip=(skip[0].clone(), skip[1].clone()) if lst else None, addend_planes=ap if planes_ep else None,
                           relu_src_hi=mp[0] if planes_ep else None)
        torch.cuda.synchronize()
    finally:
        ctx.set_workspace(0)
    val = _merged(out.pl) if pout else out.t
    return val.clone(), out, capg


@pytest.mark.parametrize("row", GEMM_ROWS, ids=[r.name for r in GEMM_ROWS])
def test_tile_against_float64_and_the_64x64_tile(ctx, row, monkeypatch):
    """bf16x3 / P16 forward and data gradient at the declared tile: against float64 (1e-4), against the same entry point at 64 x 64
    (2e-6; planes out: one remainder step), guard bands, capture planes and pre-split output planes"""
    from pyrapose_amd import ops
    rng, xs, w, bias, gys = _data(row)
    out_shapes, pt, pl, ld_y, ld_w = geometry(row)
    d = make_desc(row)
    wf, wdg, _ = _weights3(ctx, row, d, w)
    pin, pout = "pin" in row.forms, "pout" in row.forms
    rows_out = sum(row.B * h * ww for h, ww in out_shapes)
    rows_in = sum(row.B * h * ww for h, ww in row.shapes)
    partner_env = dict(row.env, PP_CONV3_TILE="1,1", PP_CONV3_SPLITS="1")
    partner = dict(tile="64x64", splits=1, family="*")
    if "list" in row.forms:
        partner_env, partner = None, None
    tol_partner = PLANE_TOL[FMT[0]] if pout else 2e-6
    wt = torch.as_tensor(w, dtype=torch.float64)
    if row.pass_ == "fwd":
        x = _cat_rows(xs)
        xp = _split(ctx, x)
        res = torch.zeros((rows_out, ld_y), dtype=torch.float32, device="cuda")
        res[:, :row.cout] = torch.as_tensor(rng.standard_normal((rows_out, row.cout)), dtype=torch.float32).cuda()
        rp = _split(ctx, res)
        bd = torch.zeros((ld_w,), dtype=torch.float32)
        bd[:row.cout] = torch.as_tensor(bias, dtype=torch.float32)
        bd = bd.cuda()
        ops_in = (x, xp, wf, bd, res, rp, rows_out, ld_y)
        got, out, capg = _forward(ctx, row, d, monkeypatch, row.env, row.ws, {}, ops_in)
        out.check(row.cout, "forward output")
        # float64: the operands as the launch reads them (a plane-stored operand IS the planes' value)
        xv = (_merged(xp) if pin else x).double().cpu()
        rv = (_merged(rp) if (pin and pout) else res).double().cpu()[:, :row.cout]
        xl, r0 = [], 0
        for (h, ww) in row.shapes:
            n = row.B * h * ww
            xl.append(xv[r0: r0 + n].reshape(row.B, h, ww, row.cin))
            r0 += n
        ref = torch.relu(_rows2d(_f64_conv(row, xl, wt), row.cout) + torch.as_tensor(bias) + rv)
        _close(got.cpu(), ref, 1e-4, "%s vs float64" % row.name)
        if capg is not None:
            capg.check(row.cin, "capture planes")
            assert torch.equal(capg.pl[0], xp[0]) and torch.equal(capg.pl[1], xp[1])
        if pout:   # the pre-split output is what split_planes3 makes of the f32 output of the same launch
            both = Row(*row)._replace(forms=tuple(f for f in row.forms) + ("f32out",))
            _set_env(monkeypatch, row.env)
            ctx.set_workspace(row.ws)
            try:
                y2 = torch.full((rows_out, ld_y), float("nan"), dtype=torch.float32, device="cuda")
                yp2 = ops.new_planes(rows_out, ld_y, fill=0x7fc0)
                assert_plan(both, planned(ctx, d, ops.PLAN_FWD, plan_forms(both)), family="*")
                ops.conv_fwd3(ctx, d, None if pin else x, wf[0], wf[1], bd, None if pin else res, True, y2, x_planes=xp if pin else None, y_planes=yp2,
                              res_planes=rp if pin else None)
                torch.cuda.synchronize()
            finally:
                ctx.set_workspace(0)
            wh, wl = _split(ctx, torch.nan_to_num(y2))
            assert torch.equal(_flat(yp2[0])[:, :row.cout], _flat(wh)[:, :row.cout]) and torch.equal(_flat(yp2[1])[:, :row.cout], _flat(wl)[:, :row.cout])
        if row.tile != "64x64" or row.splits > 1:
            base, _, _ = _forward(ctx, row, d, monkeypatch, partner_env, 0, partner, ops_in)
            _close(got, base, tol_partner, "%s vs the 64x64 tile" % row.name)
        return
    # ---- data gradient
    gy = _cat_rows(gys, ld_y)
    gp = _split(ctx, gy)
    add = torch.as_tensor(rng.standard_normal((rows_in, row.cin)), dtype=torch.float32).cuda()
    msk = torch.relu(torch.as_tensor(rng.standard_normal((rows_in, row.cin)), dtype=torch.float32)).cuda()   # a post-ReLU activation
    skip = None
    if "list" in row.forms:   # a sparse gradient: ~3 % of the rows live
        live = torch.as_tensor(rng.uniform(size=gy.shape[0]) < 0.03).cuda()
        gy = torch.where(live[:, None], gy, torch.zeros_like(gy))
        gp = _split(ctx, gy)
        f_, b_ = ops.row_block_list(ctx, gy, row.cout)
        skip = (f_, b_)
    ap, mp = _split(ctx, add), _split(ctx, msk)
    ops_in = (gy, gp, wdg, add, ap, msk, mp, rows_in, skip)
    got, out, capg = _dgrad(ctx, row, d, monkeypatch, row.env, row.ws, {}, ops_in)
    out.check(row.cin, "data gradient")
    planes_ep = pin and pout
    gv = (_merged(gp) if pin else gy).double().cpu()[:, :row.cout]
    av = (_merged(ap) if planes_ep else add).double().cpu()
    gl, r0 = [], 0
    for (h, ww) in out_shapes:
        n = row.B * h * ww
        gl.append(gv[r0: r0 + n].reshape(row.B, h, ww, row.cout))
        r0 += n
    xg = [torch.zeros_like(t).requires_grad_(True) for t in xs]
    outs = _f64_conv(row, xg, wt)
    gx = torch.autograd.grad(sum((o * g).sum() for o, g in zip(outs, gl)), xg)
    ref = (_rows2d(gx, row.cin) + av) * (msk.cpu() > 0)
    _close(got.cpu(), ref, 1e-4, "%s vs float64" % row.name)
    if capg is not None:
        cred = (row.cout + 31) // 32 * 32
        capg.check(cred, "capture planes")
        assert torch.equal(_flat(capg.pl[0])[:, :cred], _flat(gp[0])[:, :cred]) and torch.equal(_flat(capg.pl[1])[:, :cred], _flat(gp[1])[:, :cred])
    if pout:   # dx as planes == split_planes3 of the f32 dx of the same launch
        if "list" not in row.forms:
            _set_env(monkeypatch, row.env)
            ctx.set_workspace(row.ws)
            try:
                dx2 = torch.full((rows_in, row.cin), float("nan"), dtype=torch.float32, device="cuda")
                xp2 = ops.new_planes(rows_in, row.cin, fill=0x7fc0)
                ops.conv_bwd_data3(ctx, d, None if pin else gy, wdg[0], wdg[1], add, msk, dx2, dy_planes=gp if pin else None, dx_planes=xp2)
                torch.cuda.synchronize()
            finally:
                ctx.set_workspace(0)
            wh, wl = _split(ctx, dx2)
            assert torch.equal(xp2[0], wh) and torch.equal(xp2[1], wl)
    if partner is not None and (row.tile != "64x64" or row.splits > 1):
        base, _, _ = _dgrad(ctx, row, d, monkeypatch, partner_env, 0, partner, ops_in)
        _close(got, base, tol_partner, "%s vs the 64x64 tile" % row.name)


def _wgrad_ref(row, xv, gv):
    """float64 dW [k*k*cin, cout] and bias gradient from the operands as 2-D row matrices (host, float64)"""
    out_shapes = geometry(row)[0]
    xl, gl, r0, g0 = [], [], 0, 0
    for (h, ww), (oh, ow) in zip(row.shapes, out_shapes):
        n, m = row.B * h * ww, row.B * oh * ow
        xl.append(xv[r0: r0 + n].reshape(row.B, h, ww, row.cin))
        gl.append(gv[g0: g0 + m].reshape(row.B, oh, ow, row.cout))
        r0 += n
        g0 += m
    wt = torch.zeros((row.k, row.k, row.cin, row.cout), dtype=torch.float64, requires_grad=True)
    outs = _f64_conv(row, xl, wt)
    gw, = torch.autograd.grad(sum((o * g).sum() for o, g in zip(outs, gl)), [wt])
    return gw.reshape(-1, row.cout), gv.sum(0)


@pytest.mark.parametrize("row", WGRAD_ROWS, ids=[r.name for r in WGRAD_ROWS])
def test_weight_gradient_tile_against_float64(ctx, row, monkeypatch):
    """conv_bwd_weight3 at the declared kernel, tile and split count against float64 autograd: dW 1e-4, bias gradient 5e-5, padding
    columns of dW exactly zero; over a block list with ~5 % live rows and with one single live row; slices mode: bit-identical runs"""
    from pyrapose_amd import ops
    rng, xs, w, bias, gys = _data(row)
    out_shapes, pt, pl, ld_y, ld_w = geometry(row)
    d = make_desc(row)
    pin, lst = "pin" in row.forms, "list" in row.forms
    x = _cat_rows(xs)
    gy_dense = _cat_rows(gys, ld_y)
    M = gy_dense.shape[0]
    variants = [("dense", gy_dense)]
    if lst:
        live = torch.as_tensor(rng.uniform(size=M) < 0.05).cuda()
        one = torch.zeros((M,), dtype=torch.bool, device="cuda")
        one[int(rng.integers(0, M))] = True
        variants = [("5 % live", torch.where(live[:, None], gy_dense, torch.zeros_like(gy_dense))),
                    ("one live row", torch.where(one[:, None], gy_dense, torch.zeros_like(gy_dense)))]
    det = row.env.get("PP_WGRAD3_DETERMINISTIC") == "1"
    _set_env(monkeypatch, row.env)
    ctx.set_workspace(row.ws)
    try:
        for what, gy in variants:
            xp, gp = _split(ctx, x), _split(ctx, gy)
            skip = ops.row_block_list(ctx, gy, row.cout) if lst else None
            runs = []
            for _ in range(2 if det else 1):
                if row.ws:
                    ctx.workspace.fill_(float("nan"))
                assert_plan(row, planned(ctx, d, ops.PLAN_BWD_WEIGHT, plan_forms(row)))
                dw = torch.zeros((row.k * row.k * row.cin, ld_w), dtype=torch.float32, device="cuda")
                db = torch.zeros((ld_w,), dtype=torch.float32, device="cuda")
                if pin:
                    ops.conv_bwd_weight3(ctx, d, None, None, dw, db, x_planes=xp, dy_planes=gp, dy_skip=skip)
                else:
                    ops.conv_bwd_weight3(ctx, d, x, gy, dw, db, dy_skip=skip)
                torch.cuda.synchronize()
                runs.append((dw, db))
            dw, db = runs[0]
            if det:
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "slices mode is not bit-reproducible"
            xv = (_merged(xp) if pin else x).double().cpu()
            gv = (_merged(gp) if pin else gy).double().cpu()[:, :row.cout]
            gw_ref, db_ref = _wgrad_ref(row, xv, gv)
            _close(dw[:, :row.cout].cpu(), gw_ref, 1e-4, "%s dW (%s) vs float64" % (row.name, what))
            assert bool((dw[:, row.cout:] == 0).all()), "padding columns of dW written"
            _close(db[:row.cout].cpu(), db_ref, 5e-5, "%s dbias (%s) vs float64" % (row.name, what))
            assert bool((db[row.cout:] == 0).all())
    finally:
        ctx.set_workspace(0)


@pytest.mark.parametrize("row", F32_ROWS, ids=[r.name for r in F32_ROWS])
def test_f32_kernels_at_each_tile_against_float64(fctx, row, monkeypatch):
    """conv.hip (exact-f32 fma chains) under PP_CONV_TILE: forward with bias + residual + ReLU, data gradient with addend + mask,
    weight gradient; 2e-5 (dW, bias gradient 5e-5) of the output's max magnitude; guard bands"""
    from pyrapose_amd import ops
    ctx = fctx
    rng, xs, w, bias, gys = _data(row)
    out_shapes, pt, pl, ld_y, ld_w = geometry(row)
    ld_y = row.ld_y or (row.cout + 15) // 16 * 16
    d = ops.make_conv_desc(row.B, row.shapes, out_shapes, row.cin, row.cout, row.k, row.stride, pt, pl, row.cin, ld_y, ld_w)
    wd, _ = _device_weight(w, row.cout)
    wt = torch.as_tensor(w, dtype=torch.float64)
    rows_out = sum(row.B * h * ww for h, ww in out_shapes)
    rows_in = sum(row.B * h * ww for h, ww in row.shapes)
    _set_env(monkeypatch, row.env)
    if row.pass_ == "fwd":
        ref = ref_conv(xs, w, bias, row.stride, row.pad)
        res = [torch.as_tensor(rng.standard_normal(tuple(r.shape)), dtype=torch.float64) for r in ref]
        bd = torch.zeros((ld_w,), dtype=torch.float32)
        bd[:row.cout] = torch.as_tensor(bias, dtype=torch.float32)
        out = Guarded(rows_out, ld_y, _band(row), True, False)
        ops.conv_fwd(ctx, d, _cat_rows(xs), wd, bd.cuda(), _cat_rows(res, ld_y), True, out.t)
        torch.cuda.synchronize()
        out.check(row.cout, "f32 forward")
        want = torch.cat([torch.relu(r + q).reshape(-1, row.cout) for r, q in zip(ref, res)], dim=0)
        _close(out.t[:, :row.cout].cpu(), want, 2e-5, "%s vs float64" % row.name)
        return
    xg = [t.clone().requires_grad_(True) for t in xs]
    wg = wt.clone().requires_grad_(True)
    outs = _f64_conv(row, xg, wg)
    grads = torch.autograd.grad(sum((o * g).sum() for o, g in zip(outs, gys)), xg + [wg])
    gy = _cat_rows(gys, ld_y)
    if row.pass_ == "dgrad":
        add = torch.as_tensor(rng.standard_normal((rows_in, row.cin)), dtype=torch.float64)
        msk = torch.as_tensor(rng.standard_normal((rows_in, row.cin)), dtype=torch.float64)
        out = Guarded(rows_in, row.cin, _band(row), True, False)
        ops.conv_bwd_data(ctx, d, gy, wd, add.float().cuda(), msk.float().cuda(), out.t)
        torch.cuda.synchronize()
        out.check(row.cin, "f32 data gradient")
        want = (_rows2d(grads[:-1], row.cin) + add) * (msk > 0)
        _close(out.t.cpu(), want, 2e-5, "%s vs float64" % row.name)
        return
    dw = torch.zeros((row.k * row.k * row.cin, ld_w), dtype=torch.float32, device="cuda")
    db = torch.zeros((ld_w,), dtype=torch.float32, device="cuda")
    ops.conv_bwd_weight(ctx, d, _cat_rows(xs), gy, dw, db)
    torch.cuda.synchronize()
    _close(dw[:, :row.cout].cpu(), grads[-1].reshape(-1, row.cout), 5e-5, "%s dW vs float64" % row.name)
    assert bool((dw[:, row.cout:] == 0).all())
    _close(db[:row.cout].cpu(), _rows2d(gys, row.cout).sum(0), 5e-5, "%s dbias vs float64" % row.name)


@pytest.mark.parametrize("tile", ["128x64", "128x128"])
def test_f32_stem_at_both_tiles(fctx, tile, monkeypatch):
    """conv1 (cin == 4, 7x7 / 2 on the packed RGB input) at the two tiles its launcher has, guard bands, two row tiles + 1 row"""
    from pyrapose_amd import ops
    ctx = fctx
    rng = np.random.default_rng(3)
    B, H, W = 1, 6, 85      # -> 3 x 43 = 129 output rows: BM + 1
    x = torch.as_tensor(rng.standard_normal((B, H, W, 3)), dtype=torch.float64)
    w = rng.standard_normal((7, 7, 3, 64)) / 12.0
    ref = ref_conv([x], w, None, 2, 3)[0]
    oh, ow = ref.shape[1], ref.shape[2]
    assert B * oh * ow == 129
    w4 = np.concatenate([w, np.zeros((7, 7, 1, 64))], axis=2).reshape(-1, 64)
    buf = np.zeros(((w4.shape[0] + 15) // 16 * 16, 64), np.float32)
    buf[: w4.shape[0]] = w4
    x4 = torch.empty((B * H * W, 4), dtype=torch.float32, device="cuda")
    ops.pack_rgb_to_4(ctx, x.to(torch.float32).contiguous().cuda(), x4)
    d = ops.make_conv_desc(B, [(H, W)], [(oh, ow)], 4, 64, 7, 2, 3, 3, 4, 64, 64)
    _set_env(monkeypatch, {"PP_CONV_TILE": TILE_ENV[tile]})
    out = Guarded(B * oh * ow, 64, 128, True, False)
    ops.conv_fwd(ctx, d, x4, torch.from_numpy(buf).cuda(), None, None, False, out.t)
    torch.cuda.synchronize()
    out.check(64, "stem")
    _close(out.t.cpu(), ref.reshape(-1, 64), 2e-5, "stem %s vs float64" % tile)
