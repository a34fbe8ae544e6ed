"""The merged stride-2 data gradient (pp_conv2d_nhwc_bwd_data_s2_bf16x3) through pp_conv_plan_text's PP_PLAN_BWD_DATA_S2 pass: host
only, no context.  The six stride-2 data gradients of the bench step (their keys copied from lines 39, 40, 44, 45, 51 and 59 of
tests/golden/conv_plans.txt) each become ONE launch whose grid is the tile grids of the per-class route one behind the other;
that route's own text for the same keys is still the golden text (tests/test_conv_plan_cpu.py::test_pinned_plans_of_the_bench_step
asserts that for the whole table; here for the six lines, so that this file says on its own that the old pass did not move).
The host pieces of the route (class geometry, grid concatenation, prefix sums) also run as a stand-alone program under the address
and undefined-behaviour sanitizers (tools/s2_geometry_check.cpp)."""
import json
import os
import re
import shutil
import subprocess

import pytest

from pyrapose_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_LINES = (39, 40, 44, 45, 51, 59)
S2_FAMILY = "igemm3f[stride-2 merged]"
SWITCHES = ("PP_CONV3_TILE", "PP_CONV3_SPLITS", "PP_CONV4P", "PP_CONV_DEBUG", "PP_CONV3_S2MERGED")


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _golden():
    lines = [ln for ln in open(os.path.join(ROOT, "tests", "golden", "conv_plans.txt")).read().split("\n") if ln]
    out = []
    for no in GOLDEN_LINES:
        key, _, want = lines[no - 1].partition("\t")
        out.append((no, json.loads(key), want))
    return out


def _desc(k):
    c = k["conv"]
    return ops.make_conv_desc(k["in"][0], [tuple(s) for s in k["in"][1]], [tuple(s) for s in k["out"][1]], c[0], c[1], c[2], c[4], c[5], c[6], c[7], c[8],
                              c[9])


def _tiles(m, n, bm, bn):
    return -(-m // bm) * -(-n // bn)


@pytest.mark.parametrize("no,key,want", _golden(), ids=["line%d" % n for n in GOLDEN_LINES])
def test_bench_gradient_is_one_launch_over_the_class_grids(no, key, want):
    assert key["pass"] == ops.PLAN_BWD_DATA and key["conv"][4] == 2
    d = _desc(key)
    old = ops.conv_plan_text(d, ops.PLAN_BWD_DATA, key["forms"], key["fmt"], key["n_cu"], key["ws"])
    assert old.rstrip("\n").replace("\n", " ;; ") == want          # the per-class route: still the golden text
    new = ops.conv_plan_text(d, ops.PLAN_BWD_DATA_S2, key["forms"], key["fmt"], key["n_cu"], key["ws"])
    lines = new.splitlines()
    assert len(lines) == 1, new                                       # exactly one launch
    head, _, detail = lines[0].partition(" | ")
    assert "class_fill" not in new and "refused" not in new
    assert head.endswith(" " + S2_FAMILY) and S2_FAMILY not in old and "igemm3f[parity class]" not in new
    bm, bn = map(int, re.search(r"tile (\d+)x(\d+)", head).groups())
    kv = dict(x.split("=") for x in detail.split())
    # the grid: the old route's class grids, summed.  A GEMM class of the old route is a tile grid already (and on the same tile:
    # the merged launch takes the tile of the heaviest class, which is its first line); a class without taps is a pointwise fill
    # there -- its line gives rows and channels, from which its tile grid follows
    total, per_class = 0, []
    for ln in old.splitlines():
        m, n = map(int, re.search(r"\bM (\d+) N (\d+)", ln).groups())
        if "class_fill" in ln:
            g = _tiles(m, n, bm, bn)
        else:
            assert ("tile %dx%d " % (bm, bn)) in ln, (ln, head)
            g = int(re.search(r"grid=(\d+)", ln).group(1))
            assert g == _tiles(m, n, bm, bn)
        per_class.append(g)
        total += g
    assert int(kv["grid"]) == total
    assert sorted(map(int, kv["class_grids"].split("+"))) == sorted(per_class)
    # heaviest class first
    steps = [int(s) for s in re.findall(r"steps (\d+)", head)]
    assert steps == sorted(steps, reverse=True) and len(steps) == len(per_class)


def test_3x3_order_is_4_2_2_1_taps_and_1x1_is_one_tap_then_fills():
    (_, k3, _), (_, k1, _) = [g for g in _golden() if g[0] in (51, 39)][::-1]
    h3 = ops.conv_plan_text(_desc(k3), ops.PLAN_BWD_DATA_S2, k3["forms"], k3["fmt"], k3["n_cu"], k3["ws"])
    c = k3["conv"][1] // 32          # steps per tap
    assert [int(s) for s in re.findall(r"steps (\d+)", h3)] == [4 * c, 2 * c, 2 * c, c]
    h1 = ops.conv_plan_text(_desc(k1), ops.PLAN_BWD_DATA_S2, k1["forms"], k1["fmt"], k1["n_cu"], k1["ws"])
    assert [int(s) for s in re.findall(r"steps (\d+)", h1)] == [k1["conv"][1] // 32, 0, 0, 0]


def test_classes_without_rows_are_not_in_the_grid():
    # H = 1: both cy = 1 classes are empty; a 1 x 1 input: class (0, 0) alone
    d = ops.make_conv_desc(2, [(1, 9)], [(1, 5)], 64, 32, 1, 2, 0, 0, 64, 32, 32)
    t = ops.conv_plan_text(d, ops.PLAN_BWD_DATA_S2, ops.PLAN_PLANES_IN | ops.PLAN_PLANES_OUT, 1, 256, 0)
    assert ", 2 classes:" in t and "(0,0) M 10 " in t and "(0,1) M 8 " in t and "grid=2 " in t
    d = ops.make_conv_desc(3, [(1, 1)], [(1, 1)], 64, 32, 3, 2, 1, 1, 64, 32, 32)
    t = ops.conv_plan_text(d, ops.PLAN_BWD_DATA_S2, 0, 0, 256, 0)
    assert ", 1 classes:" in t and "(0,0) M 3 steps 1 " in t and "grid=1 " in t


def test_calls_the_route_does_not_take_are_refused():
    """like the lazy operand of tests/test_conv_plan_cpu.py: the text says what the entry point would do -- return PP_ERR_ARG"""
    PP = ops.PLAN_PLANES_IN | ops.PLAN_PLANES_OUT
    s2 = ops.make_conv_desc(2, [(6, 5)], [(3, 3)], 64, 32, 1, 2, 0, 0, 64, 32, 32)
    assert "refused" not in ops.conv_plan_text(s2, ops.PLAN_BWD_DATA_S2, PP)
    assert "refused" not in ops.conv_plan_text(s2, ops.PLAN_BWD_DATA_S2, 0)
    s1 = ops.make_conv_desc(2, [(6, 5)], [(6, 5)], 64, 32, 1, 1, 0, 0, 64, 32, 32)
    assert "refused" in ops.conv_plan_text(s1, ops.PLAN_BWD_DATA_S2, PP)                                    # stride 1
    two = ops.make_conv_desc(2, [(6, 5), (3, 3)], [(6, 5), (3, 3)], 64, 32, 1, 1, 0, 0, 64, 32, 32)
    assert "refused" in ops.conv_plan_text(two, ops.PLAN_BWD_DATA_S2, PP)                                   # two levels
    assert "refused" in ops.conv_plan_text(s2, ops.PLAN_BWD_DATA_S2, ops.PLAN_PLANES_IN)                    # planes in, f32 out
    assert "refused" in ops.conv_plan_text(s2, ops.PLAN_BWD_DATA_S2, ops.PLAN_PLANES_OUT)                   # f32 in, planes out
    assert "refused" in ops.conv_plan_text(s2, ops.PLAN_BWD_DATA_S2, PP | ops.PLAN_F32_OUT)                 # both output forms
    assert "refused" in ops.conv_plan_text(s2, ops.PLAN_BWD_DATA_S2, ops.PLAN_CAPTURE)                      # split capture
    assert "refused" in ops.conv_plan_text(s2, ops.PLAN_BWD_DATA_S2, PP | ops.PLAN_LIST)                    # row-block skip


def test_switch_is_read_at_every_query(monkeypatch):
    assert ops.conv_s2_merged() is True
    monkeypatch.setenv("PP_CONV3_S2MERGED", "0")
    assert ops.conv_s2_merged() is False
    monkeypatch.setenv("PP_CONV3_S2MERGED", "1")
    assert ops.conv_s2_merged() is True


def test_host_geometry_under_sanitizers(tmp_path):
    """tools/s2_geometry_check.cpp with the address and undefined-behaviour sanitizers: a stand-alone host program (nothing is loaded
    into this process)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "s2_geometry_check")
    # (the runtimes linked INTO the program: it then runs the same whatever else the environment loads beside it)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "pyrapose_amd", "csrc"), os.path.join(ROOT, "tools", "s2_geometry_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
