"""The conv launch policy (csrc/conv_plan.h) through pp_conv_plan_text: host only, no context, nothing allocated.  Properties
that hold for every plan, each decision on either side of its edge, every per-launch switch that a plan depends on flipped inside
one process, and the pinned table of the bench step's plans.

Not reachable through this interface, so not covered here: PP_CONV_DEBUG (it only prints the plan, the text is the same with and
without it) and PP_CONV_TILE (conv.hip's f32 kernels take no plan); `Cred % 32 != 0` (the forward entry point and the export
refuse cin % 32 != 0 before planning, and the data gradient rounds its reduction up to 32, so that condition of the LDS-DMA
branch is never false from a descriptor)."""
import itertools
import os
import re
import subprocess
import sys

import pytest

from pyrapose_amd import ops

FWD, DGRAD, WGRAD = ops.PLAN_FWD, ops.PLAN_BWD_DATA, ops.PLAN_BWD_WEIGHT
PIN, POUT, LIST, LAZY_IN = ops.PLAN_PLANES_IN, ops.PLAN_PLANES_OUT, ops.PLAN_LIST, ops.PLAN_LAZY_IN
PP = PIN | POUT
MB = 1 << 20
SWITCHES = ("PP_CONV3_DMA", "PP_CONV3_DMA_VAR", "PP_CONV3_DMA2", "PP_CONV3_DMA2_MIN", "PP_CONV4P", "PP_CONV4P_NST", "PP_CONV4P_SPLITS",
            "PP_WGRAD3R", "PP_WGRAD3_DETERMINISTIC", "PP_CONV3_TILE", "PP_CONV3_SPLITS", "PP_WGRAD3_SPLITS", "PP_WGRAD3_TILE",
            "PP_WGRAD3R_SPLITS", "PP_CONV_DEBUG")
FAMILIES = ("igemm3f[parity class]", "igemm3f[row list]", "igemm3x[capture]", "igemm3x[planes->planes]", "igemm3x[planes->f32]",
            "igemm3x[f32->planes]", "igemm3x[f32->f32]", "igemm4x<NWM=2>", "igemm4x", "igemm4p", "igemm3f", "igemm3",
            "wgrad3f[planes, list]", "wgrad3f[planes]", "wgrad3f[f32, list]", "wgrad3f[f32]", "wgrad3r", "wgrad3w", "wgrad3")


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def desc(shapes, cin, cout, k=3, stride=1, n_img=1):
    out = [(-(-h // stride), -(-w // stride)) for h, w in shapes]
    pad = k // 2
    r32, r16 = (cout + 31) // 32 * 32, (cout + 15) // 16 * 16
    return ops.make_conv_desc(n_img, shapes, out, cin, cout, k, stride, pad, pad, cin, r32, r16)


def plans(d, pass_, forms=PP, fmt=1, n_cu=256, ws=0):
    """[{head, family, key: int ...}] of one call"""
    res = []
    for line in ops.conv_plan_text(d, pass_, forms, fmt, n_cu, ws).splitlines():
        head, _, detail = line.partition(" | ")
        fam = next((f for f in FAMILIES if head.endswith(" " + f)), None)
        p = {"head": head, "family": fam, "line": line}
        for kv in detail.split():
            k, _, v = kv.partition("=")
            p[k] = int(v) if re.fullmatch(r"-?\d+", v) else v
        for k in ("M", "N", "splits", "tiles"):
            m = re.search(r"\b%s (\d+)" % k, head) or (k == "splits" and re.search(r"x (\d+) splits", head))   # (igemm4p: "tiles x S splits")
            if m:
                p.setdefault(k if k != "splits" else "head_splits", int(m.group(1)))
        res.append(p)
    return res


def plan(*a, **k):
    p, = plans(*a, **k)
    return p


# ---- properties of every plan ----
SHAPES = [([(5, 7)], 32, 16), ([(60, 80)], 64, 256), ([(60, 80), (30, 40), (15, 20)], 128, 256), ([(127, 256)], 64, 512),
          ([(665, 254)], 32, 128), ([(300, 254)], 128, 384), ([(33, 31)], 256, 144)]


@pytest.mark.parametrize("shapes,cin,cout", SHAPES)
def test_properties_of_every_plan(monkeypatch, shapes, cin, cout):
    for k, stride, pass_, forms, ws, n_cu, fmt, det in itertools.product((1, 3), (1, 2), (FWD, DGRAD, WGRAD), (0, PIN, PP, PP | LIST),
                                                                          (0, 1 * MB, 64 * MB), (256, 104), (0, 1), ("0", "1")):
        if (stride == 2 and len(shapes) > 1) or (pass_ == WGRAD and cin % 64) or (pass_ == FWD and forms & LIST and not (forms == PP | LIST and k == 3 and stride == 1)):
            continue
        if det == "1" and pass_ != WGRAD:
            continue
        monkeypatch.setenv("PP_WGRAD3_DETERMINISTIC", det)
        d = desc(shapes, cin, cout, k, stride)
        for p in plans(d, pass_, forms, fmt, n_cu, ws):
            if "class_fill" in p["head"]:
                assert p["grid"] > 0
                continue
            assert p["family"] is not None and p["grid"] > 0, p["line"]
            assert p["ws_need"] <= ws, p["line"]
            if pass_ == WGRAD:
                assert p["splits"] * p["rows_per_split"] >= p["M"] and p["rows_per_split"] % 32 == 0, p["line"]
                if p["family"] in ("wgrad3r", "wgrad3w"):
                    assert forms & PIN and not (det == "1" and ws > 0), p["line"]
                continue
            if p["family"] == "igemm4x":
                assert ws > 0 or p["tail_splits"] == 0
                ntn = p["n_tiles_n"]
                if p["tail_splits"]:
                    # a tail exists only with a workspace and at least two whole rounds; whole rounds + tail cover M exactly once
                    assert ws > 0 and p["full_rt"] * ntn >= 2 * n_cu and p["full_rt"] * ntn % n_cu < ntn, p["line"]
                    assert p["tail_m_off"] == p["full_rt"] * 254 < p["M"] and p["tail_grid"] > 0 and p["finish_blocks"] > 0, p["line"]
                else:
                    assert (p["full_rt"] - 1) * 254 < p["M"] <= p["full_rt"] * 254, p["line"]
                assert p["grid"] == p["full_rt"] * ntn
            if p["family"] == "igemm3f[parity class]":
                assert p["head_splits"] == 1 and p["finish_blocks"] == 0, p["line"]
            assert (p["finish_blocks"] > 0) == (p["ws_need"] > 0), p["line"]


def test_lazy_dy_without_a_list_is_refused():
    d = desc([(60, 80)], 128, 256)
    assert "refused" in ops.conv_plan_text(d, WGRAD, PIN | LAZY_IN, 1, 256, 0)
    assert "refused" not in ops.conv_plan_text(d, WGRAD, PIN | LAZY_IN | LIST, 1, 256, 0)
    assert "refused" in ops.conv_plan_text(desc([(60, 80)], 128, 256, k=1), DGRAD, PP | LAZY_IN | LIST, 1, 256, 0)   # (no listed launch for 1x1)
    assert "row list" in ops.conv_plan_text(d, DGRAD, PP | LAZY_IN | LIST, 1, 256, 0)


# ---- each decision at its edge ----
def test_lds_dma_from_two_rounds_of_tiles(monkeypatch):
    monkeypatch.setenv("PP_CONV3_TILE", "2,2")
    # cout 512 -> 4 column tiles; 128 row tiles of 254 rows -> 512 tiles = PP_CONV3_DMA_MIN; one row tile fewer -> 508
    assert plan(desc([(127, 256)], 64, 512), FWD, ws=64 * MB)["family"] == "igemm4x"
    assert plan(desc([(127, 254)], 64, 512), FWD, ws=64 * MB)["family"] == "igemm3x[planes->planes]"
    # the kernel's own conditions: cout % 128, a 3-row kernel, planes on both sides
    assert plan(desc([(127, 256)], 64, 448), FWD, ws=64 * MB)["family"] == "igemm3x[planes->planes]"
    assert plan(desc([(127, 256)], 64, 512, k=1), FWD, ws=64 * MB)["family"] == "igemm3f"
    assert plan(desc([(127, 256)], 64, 512), FWD, PIN, ws=64 * MB)["family"] == "igemm3x[planes->f32]"


def test_lds_dma_tail_rule(monkeypatch):
    monkeypatch.setenv("PP_CONV3_TILE", "2,2")
    # one column tile; 2 rounds + 153 tiles: 153 * 100 < 60 * 256 -> tail; + 154: the last round stays in the one launch
    a = plan(desc([(665, 254)], 256, 128), FWD, ws=64 * MB)
    b = plan(desc([(666, 254)], 256, 128), FWD, ws=64 * MB)
    assert a["family"] == b["family"] == "igemm4x"
    assert a["full_rt"] == 512 and a["tail_splits"] > 1 and a["tail_m_off"] == 512 * 254
    assert b["full_rt"] == 666 and b["tail_splits"] == 0 and b["ws_need"] == 0
    # no scratch, or one too small for two slices of the tail's rows: everything in the one launch
    for ws in (0, 2 * 153 * 254 * 128 * 4 - 4):
        c = plan(desc([(665, 254)], 256, 128), FWD, ws=ws)
        assert c["full_rt"] == 665 and c["tail_splits"] == 0, c["line"]
    # every split keeps at least 4 (kernel row, 32 channels) groups: 64 channels x 3 rows = 6 groups allow none, 96 channels two
    assert plan(desc([(665, 254)], 64, 128), FWD, ws=64 * MB)["tail_splits"] == 0
    assert plan(desc([(665, 254)], 96, 128), FWD, ws=64 * MB)["tail_splits"] == 2


def test_tile_falls_to_128x128_where_row_reuse_applies():
    big = [(480, 640)]
    assert "tile 256x128" in plan(desc(big, 64, 256, k=1), FWD)["head"]            # no row reuse for 1x1: the model's 256 x 128 stays
    p = plan(desc(big, 64, 256), FWD)
    assert "tile 128x128" in p["head"] and p["family"].startswith("igemm")
    assert "tile 256x128" not in plan(desc(big, 64, 256), FWD, 0)["head"]           # f32 operands alike


def test_split_k_needs_eight_steps_and_room_for_its_slices():
    d = desc([(20, 30)], 512, 256)                       # 600 rows, 144 steps: 10 tiles on 256 CUs
    p = plan(d, FWD, ws=64 * MB)
    assert p["head_splits"] > 1 and p["finish_blocks"] > 0 and p["ws_need"] == p["head_splits"] * 600 * 256 * 4
    assert plan(d, FWD, ws=2 * 600 * 256 * 4 - 4)["head_splits"] == 1     # not even two slices fit
    assert plan(d, FWD, ws=2 * 600 * 256 * 4)["head_splits"] == 2
    assert plan(d, FWD, ws=0)["head_splits"] == 1
    assert plan(desc([(20, 30)], 32, 256), FWD, ws=64 * MB)["head_splits"] == 1    # 9 steps: 9 / 2 < 8


def test_weight_gradient_split_clamps(monkeypatch):
    monkeypatch.setenv("PP_WGRAD3R", "0")
    assert plan(desc([(16, 32)], 64, 64, k=1), WGRAD, PIN)["splits"] == 1                      # 512 rows: max_splits 1
    p = plan(desc([(480, 640)], 64, 64, k=1), WGRAD, PIN, n_cu=256)                              # 1 tile, 307 200 rows: capped at 64
    assert p["splits"] == 64
    monkeypatch.setenv("PP_WGRAD3_DETERMINISTIC", "1")
    slice_bytes = (64 * 64 + 64) * 4
    q = plan(desc([(480, 640)], 64, 64, k=1), WGRAD, PIN, ws=3 * slice_bytes)
    assert q["use_ws"] == 1 and q["splits"] == 3 and q["ws_need"] == 3 * slice_bytes and q["finish_blocks"] > 0
    assert plan(desc([(480, 640)], 64, 64, k=1), WGRAD, PIN, ws=slice_bytes - 4)["use_ws"] == 0


@pytest.mark.parametrize("cin,cout,tile", [(64, 64, "64x64"), (64, 65, "64x128"), (64, 128, "64x128"), (128, 64, "128x64"),
                                           (128, 65, "128x128"), (128, 128, "128x128")])
def test_weight_gradient_tile(monkeypatch, cin, cout, tile):
    monkeypatch.setenv("PP_WGRAD3R", "0")
    assert plan(desc([(30, 40)], cin, cout), WGRAD, PIN)["tile"] == tile


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("cout", [511, 512])
def test_tap_row_reuse_weight_gradient_switch(monkeypatch, fmt, cout):
    d = desc([(30, 40)], 128, cout)
    want = {None: "wgrad3w" if (fmt == 1 and cout >= 512) else "wgrad3f[planes]", "0": "wgrad3f[planes]", "1": "wgrad3r", "2": "wgrad3w"}
    for r, fam in want.items():
        if r is None:
            monkeypatch.delenv("PP_WGRAD3R", raising=False)
        else:
            monkeypatch.setenv("PP_WGRAD3R", r)
        assert plan(d, WGRAD, PIN, fmt)["family"] == fam, (r, fmt, cout)
        assert plan(d, WGRAD, 0, fmt)["family"] == "wgrad3f[f32]"                                  # planes only
        assert plan(d, WGRAD, PIN | LIST, fmt)["family"] == ("wgrad3r" if r == "1" else "wgrad3f[planes, list]")   # wgrad3w: dense only


# ---- every per-launch switch that changes a plan, flipped between two calls of one process (see the module docstring for the two that do not) ----
def test_per_launch_switches_flip_inside_one_process(monkeypatch):
    big, head, one = desc([(127, 256)], 64, 512), desc([(60, 80), (30, 40), (15, 20)], 64, 256, n_img=2), desc([(30, 40)], 512, 128, k=1)
    monkeypatch.setenv("PP_CONV3_TILE", "2,2")
    assert plan(big, FWD, ws=64 * MB)["family"] == "igemm4x"                    # (this call walks the LDS-DMA branch)
    monkeypatch.setenv("PP_CONV3_DMA", "0")
    assert plan(big, FWD, ws=64 * MB)["family"] == "igemm3x[planes->planes]"
    monkeypatch.delenv("PP_CONV3_DMA")
    for var in (0, 1, 2, 3, 4, 9):
        monkeypatch.setenv("PP_CONV3_DMA_VAR", str(var))
        assert plan(big, FWD, ws=64 * MB)["variant"] == var
    # PP_CONV3_DMA2 and, after the branch above was taken, PP_CONV3_DMA2_MIN: 200 tiles against the default 512
    assert plan(head, FWD)["family"] == "igemm3x[planes->planes]"
    monkeypatch.setenv("PP_CONV3_DMA2", "1")
    assert plan(head, FWD)["family"] == "igemm3x[planes->planes]"
    monkeypatch.setenv("PP_CONV3_DMA2_MIN", "200")
    assert plan(head, FWD)["family"] == "igemm4x<NWM=2>" and plan(head, FWD)["grid"] == 200
    monkeypatch.setenv("PP_CONV3_DMA2_MIN", "201")
    assert plan(head, FWD)["family"] == "igemm3x[planes->planes]"
    monkeypatch.setenv("PP_CONV3_DMA2", "0")
    monkeypatch.setenv("PP_CONV3_DMA2_MIN", "1")
    assert plan(head, FWD)["family"] == "igemm3x[planes->planes]"
    # tile and split hooks
    monkeypatch.setenv("PP_CONV3_TILE", "1,2")
    assert "tile 64x128" in plan(head, FWD)["head"]
    monkeypatch.delenv("PP_CONV3_TILE")
    monkeypatch.setenv("PP_CONV3_SPLITS", "3")
    assert plan(one, FWD, ws=64 * MB)["head_splits"] == 3 and plan(one, FWD, ws=0)["head_splits"] == 1
    monkeypatch.delenv("PP_CONV3_SPLITS")
    # igemm4p, its ring and its split
    assert plan(one, FWD, ws=64 * MB)["family"] == "igemm3f"
    monkeypatch.setenv("PP_CONV4P", "1")
    p = plan(one, FWD, ws=64 * MB)
    assert p["family"] == "igemm4p" and p["stages"] == 4 and p["head_splits"] > 1           # 10 tiles on 256 CUs: its own split
    monkeypatch.setenv("PP_CONV4P_NST", "3")
    monkeypatch.setenv("PP_CONV4P_SPLITS", "1")
    p = plan(one, FWD, ws=64 * MB)
    assert p["stages"] == 3 and p["head_splits"] == 1 and p["finish_blocks"] == 0
    assert plan(head, FWD)["family"] != "igemm4p"                                              # 1x1 only
    monkeypatch.delenv("PP_CONV4P")
    # weight gradient
    w = desc([(60, 80)], 128, 256)
    monkeypatch.setenv("PP_WGRAD3R", "1")
    assert plan(w, WGRAD, PIN)["family"] == "wgrad3r"
    monkeypatch.setenv("PP_WGRAD3R_SPLITS", "5")
    assert plan(w, WGRAD, PIN)["splits"] == 5
    monkeypatch.setenv("PP_WGRAD3_DETERMINISTIC", "1")
    assert plan(w, WGRAD, PIN, ws=64 * MB)["family"] == "wgrad3f[planes]" and plan(w, WGRAD, PIN, ws=0)["family"] == "wgrad3r"
    monkeypatch.setenv("PP_WGRAD3R", "0")
    monkeypatch.setenv("PP_WGRAD3_SPLITS", "4")
    p = plan(w, WGRAD, PIN, ws=64 * MB)
    assert p["splits"] == 4 and p["use_ws"] == 1 and p["rows_per_split"] == 1216
    monkeypatch.setenv("PP_WGRAD3_TILE", "1,1")
    assert plan(w, WGRAD, PIN)["tile"] == "64x64"
    monkeypatch.setenv("PP_WGRAD3_TILE", "2,2")
    assert plan(w, WGRAD, PIN)["tile"] == "128x128"


def test_once_read_switches_in_a_fresh_process():
    """PP_CONV3_DMA_FRAC (the one-and-a-bit rule) and PP_CONV3_X4 are read once: another process sees another value"""
    code = ("from tests.test_conv_plan_cpu import *\n"
            "for h in (100, 99):\n"     # 400 / 396 tiles of 256 x 128 on 256 CUs: the second round 56.3 % / 54.7 % full
            "    print(plan(desc([(h, 254)], 64, 512), FWD)['family'])\n"
            "print(plan(desc([(480, 640)], 64, 256), FWD)['head'])\n")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(**extra):
        return subprocess.run([sys.executable, "-c", code], env=dict(env, PP_CONV3_TILE="2,2", **extra), cwd=root, capture_output=True, text=True,
                              check=True).stdout.split("\n")
    off = run()
    assert off[0] == off[1] == "igemm3x[planes->planes]"
    on = run(PP_CONV3_DMA_FRAC="55")
    assert on[0] == "igemm4x" and on[1] == "igemm3x[planes->planes]"
    env.pop("PP_CONV3_TILE", None)
    x4 = subprocess.run([sys.executable, "-c", code], env=dict(env, PP_CONV3_X4="1"), cwd=root, capture_output=True, text=True, check=True).stdout
    assert "tile 256x128" in x4.split("\n")[2]


# ---- the pinned table ----
def test_pinned_plans_of_the_bench_step():
    """tests/golden/conv_plans.txt: per line a call of one of the three bf16x3 entry points (pass, operand forms, plane format,
    CUs, scratch bytes, descriptor; JSON) and, behind a tab, its plan text -- every distinct call of one training step (default
    and with PP_SPARSE_BWD=0) and one inference call of bench configuration 1 (LineMOD, 13 classes, batch 8, 640x480, default
    mode), recorded on a commit whose launches (kernel, grid, workgroup, LDS bytes) equalled the parent's over those runs."""
    import json
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans.txt")
    lines = [ln for ln in open(path).read().split("\n") if ln]
    assert len(lines) >= 90
    seen = set()
    for ln in lines:
        key, _, want = ln.partition("\t")
        k = json.loads(key)
        d = ops.make_conv_desc(k["in"][0], [tuple(s) for s in k["in"][1]], [tuple(s) for s in k["out"][1]], k["conv"][0], k["conv"][1], k["conv"][2],
                               k["conv"][4], k["conv"][5], k["conv"][6], k["conv"][7], k["conv"][8], k["conv"][9])
        assert k["conv"][2] == k["conv"][3]
        got = ops.conv_plan_text(d, k["pass"], k["forms"], k["fmt"], k["n_cu"], k["ws"]).rstrip("\n").replace("\n", " ;; ")
        assert got == want, key
        seen.add(next(f for f in FAMILIES if want.split(" | ")[0].endswith(" " + f)))
    assert {"igemm4x", "igemm3f[row list]", "igemm3f[parity class]", "igemm3x[planes->planes]", "igemm3f", "wgrad3f[planes, list]", "wgrad3f[planes]"} <= seen
