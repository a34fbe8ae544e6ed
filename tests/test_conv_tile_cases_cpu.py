"""Host-side ledger of tests/test_gpu_conv_tiles.py (no GPU): every row of its case table gets, from pp_conv_plan_text under the row's
switches, the kernel family, tile and split count it declares -- so the table is checked before anyone has a device --, and the
table's plan signatures cover every signature pinned in tests/golden/conv_plans.txt (the launches of one bench step).

A signature is (pass, kernel family, tile, split > 1, kernel size, stride, planes in, planes out, list)."""
import json
import os
import re

import pytest

from pyrapose_amd import ops
from tests.test_conv_plan_cpu import FAMILIES, SWITCHES
from tests.test_gpu_conv_tiles import TABLE, assert_plan, make_desc, plan_forms, plan_pass

# golden signatures the table does not have to cover, by kernel family, each with its reason
LEDGER_EXCEPTIONS = {
    "igemm4x": "needs two rounds of 256-row tiles (33 536 rows); tests/test_gpu_planes.py::test_lds_dma_kernel_matches_register_staged "
               "checks it against float64",
}

PLANNED = [r for r in TABLE if r.kind != "f32"]   # (conv.hip's f32 kernels take no plan)


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES + ("PP_CONV_TILE",):
        monkeypatch.delenv(k, raising=False)


def signatures(text, pass_, forms, k, stride):
    """the signatures of one call's plan text (several launches: the classes of a stride-2 data gradient, lines or ' ;; ' parts)"""
    sigs = set()
    for line in re.split(r"\n| ;; ", text.strip()):
        if not line or "class_fill" in line:
            continue
        head, _, detail = line.partition(" | ")
        fam = next(f for f in FAMILIES if head.endswith(" " + f))
        if pass_ == ops.PLAN_BWD_WEIGHT:
            tile = re.search(r"\btile=(\d+x\d+)", detail).group(1)
            splits = int(re.search(r"\bsplits=(\d+)", detail).group(1))
        else:
            tile = re.search(r"tile (\d+x\d+) ", head).group(1)
            splits = int(re.search(r" splits (\d+) ", head).group(1))
        sigs.add((pass_, fam, tile, splits > 1, k, stride, bool(forms & ops.PLAN_PLANES_IN), bool(forms & ops.PLAN_PLANES_OUT),
                  bool(forms & ops.PLAN_LIST)))
    return sigs


def row_plan(row, fmt):
    return ops.conv_plan_text(make_desc(row), plan_pass(row), plan_forms(row), fmt, 256, row.ws)


@pytest.mark.parametrize("row", PLANNED, ids=[r.name for r in PLANNED])
def test_row_gets_the_plan_it_declares(monkeypatch, row):
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)
    for fmt in (0, 1):
        text = row_plan(row, fmt)
        heads = [line.split(" | ")[0] for line in text.splitlines()]
        assert_plan(row, heads)
        for line in text.splitlines():
            if "class_fill" not in line:
                need = int(re.search(r"ws_need=(\d+)", line).group(1))
                assert need <= row.ws and (need > 0) == (row.ws > 0 and row.splits > 1), line
    if row.kind == "gemm" and row.tile != "64x64" and "list" not in row.forms:   # its comparison partner: 64 x 64, unsplit, no scratch
        monkeypatch.setenv("PP_CONV3_TILE", "1,1")
        monkeypatch.setenv("PP_CONV3_SPLITS", "1")
        heads = [line.split(" | ")[0] for line in ops.conv_plan_text(make_desc(row), plan_pass(row), plan_forms(row), 1, 256, 0).splitlines()]
        assert_plan(row, heads, tile="64x64", splits=1, family="*")


def test_table_covers_every_pinned_plan_signature(monkeypatch):
    have = set()
    for row in PLANNED:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in row.env.items():
            monkeypatch.setenv(k, v)
        for fmt in (0, 1):
            have |= signatures(row_plan(row, fmt), plan_pass(row), plan_forms(row), row.k, row.stride)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans.txt")
    want = {}
    for ln in open(path).read().split("\n"):
        if not ln:
            continue
        key, _, text = ln.partition("\t")
        k = json.loads(key)
        for s in signatures(text, k["pass"], k["forms"], k["conv"][2], k["conv"][4]):
            want.setdefault(s, key)
    assert len(want) >= 30
    missing = sorted((s, key) for s, key in want.items() if s not in have and s[1] not in LEDGER_EXCEPTIONS)
    assert not missing, "plan signatures of the bench step without a case in tests/test_gpu_conv_tiles.py:\n" + "\n".join(map(str, missing))
    assert any(s[1] in LEDGER_EXCEPTIONS for s in want)   # (the exception is still needed)
