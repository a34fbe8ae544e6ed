"""CPU (no GPU, no shared library): pyrapose_amd/switches.py -- the table of PP_* switches the Engine's plan depends on.  The
parse rules one by one, that reading never writes, that the two defaults owned by csrc/conv_plan.h are the header's, that
engine.py reads no environment itself and names no switch the table misses, and that DESIGN.md lists every row."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    # by file: `import pyrapose_amd` loads the shared library, which this module must not need
    spec = importlib.util.spec_from_file_location("pp_switches", os.path.join(ROOT, "pyrapose_amd", "switches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


S = _load()
ROWS = {s.env: s for s in S.SWITCHES}
# switches engine.py speaks of without depending on them itself (asked through ops.conv_s2_merged(): csrc/conv_plan.h reads it)
ONLY_MENTIONED = {"PP_CONV3_S2MERGED"}


def _read(path):
    with open(os.path.join(ROOT, path)) as f:
        return f.read()


def test_table_is_well_formed():
    assert len(ROWS) == len(S.SWITCHES) and len({s.field for s in S.SWITCHES}) == len(S.SWITCHES)
    for s in S.SWITCHES:
        assert re.fullmatch(r"PP_[A-Z0-9_]+", s.env) and s.owner in ("engine", "csrc/conv_plan.h") and s.doc and "\n" not in s.doc
        assert s.default is None or isinstance(s.default, str)
    assert [f.name for f in S.dataclasses.fields(S.EngineSwitches) if not f.name.startswith("_")] == [s.field for s in S.SWITCHES]


def test_defaults():
    sw = S.EngineSwitches.from_env({})
    want = dict(conv_mode="mixed", planes=True, trunk_lanes=True, stem3=True, sparse_inplace=True, sparse_within=True, sparse_lazy=True,
                capture=False, sparse_fwd=False, prefetch=False, sparse_bwd=("reg",), capture_skip=(), capture_min_cin=64,
                splitk_mb=256, lanes=2, mask_lane=None, prefetch_after=None, conv3_fast=True, sparse_dgrad=True)
    assert {s.field: getattr(sw, s.field) for s in S.SWITCHES} == want
    assert sw.non_default() == {}
    with pytest.raises(Exception):
        sw.planes = False  # immutable


@pytest.mark.parametrize("name", ["PP_PLANES", "PP_TRUNK_LANES", "PP_STEM3", "PP_SPARSE_INPLACE", "PP_SPARSE_WITHIN", "PP_SPARSE_LAZY",
                                  "PP_CONV3_FAST", "PP_SPARSE_DGRAD"])
def test_on_unless_exactly_0(name):
    f = ROWS[name].field
    assert getattr(S.EngineSwitches.from_env({name: "0"}), f) is False
    for v in ("00", "1", "", "off", " 0"):
        assert getattr(S.EngineSwitches.from_env({name: v}), f) is True, v


@pytest.mark.parametrize("name", ["PP_CAPTURE", "PP_SPARSE_FWD", "PP_PREFETCH"])
def test_off_unless_exactly_1(name):
    f = ROWS[name].field
    assert getattr(S.EngineSwitches.from_env({name: "1"}), f) is True
    for v in ("2", "0", "", "on", "01"):
        assert getattr(S.EngineSwitches.from_env({name: v}), f) is False, v


def test_lists():
    E = S.EngineSwitches.from_env
    assert E({"PP_SPARSE_BWD": "reg,,0,cls"}).sparse_bwd == ("reg", "cls")
    assert E({"PP_SPARSE_BWD": "0"}).sparse_bwd == () and E({"PP_SPARSE_BWD": ""}).sparse_bwd == ()
    assert E({"PP_CAPTURE_SKIP": "cls,,res5,0"}).capture_skip == ("cls", "res5", "0")  # (only PP_SPARSE_BWD drops "0")


def test_integers():
    E = S.EngineSwitches.from_env
    assert [E({"PP_LANES": v}).lanes for v in ("7", "0", "-3", "1", "2", "3")] == [3, 1, 1, 1, 2, 3]
    assert E({"PP_CAPTURE_MIN_CIN": "128"}).capture_min_cin == 128 and E({"PP_SPLITK_MB": "0"}).splitk_mb == 0
    assert E({"PP_MASK_LANE": "5"}).mask_lane == 5 and E({"PP_MASK_LANE": "0"}).mask_lane == 0 and E({}).mask_lane is None
    for name in ("PP_LANES", "PP_CAPTURE_MIN_CIN", "PP_SPLITK_MB", "PP_MASK_LANE"):  # int(), as before: no atoi leniency
        with pytest.raises(ValueError):
            E({name: "2x"})


def test_strings():
    E = S.EngineSwitches.from_env
    assert E({"PP_CONV_MODE": "f16c8"}).conv_mode == "f16c8"
    assert E({"PP_PREFETCH_AFTER": "res3a_branch2a"}).prefetch_after == "res3a_branch2a" and E({"PP_PREFETCH_AFTER": ""}).prefetch_after == ""


def test_reading_never_writes_and_is_repeatable():
    class ReadOnly(dict):
        def _no(self, *a, **k):
            raise AssertionError("from_env wrote to its mapping")
        __setitem__ = __delitem__ = pop = popitem = setdefault = update = clear = _no

    given = {"PP_LANES": "3", "PP_SPARSE_BWD": "reg,cls", "PP_PLANES": "1", "PP_UNRELATED": "x", "HOME": "/nowhere"}
    env = ReadOnly(given)
    a, b = S.EngineSwitches.from_env(env), S.EngineSwitches.from_env(env)
    assert dict(env) == given
    assert a == b and hash(a) == hash(b) and a.non_default() == b.non_default() == {"PP_LANES": "3", "PP_SPARSE_BWD": "reg,cls"}
    assert a != S.EngineSwitches.from_env({})
    assert a == S.EngineSwitches.from_env({"PP_LANES": "9", "PP_SPARSE_BWD": "reg,,cls"})  # (compared by value, not by spelling)


def test_process_environment_is_the_default(monkeypatch):
    for s in S.SWITCHES:
        monkeypatch.delenv(s.env, raising=False)
    assert S.EngineSwitches.from_env() == S.EngineSwitches.from_env({})
    monkeypatch.setenv("PP_LANES", "1")
    assert S.EngineSwitches.from_env().lanes == 1 and S.EngineSwitches.from_env().non_default() == {"PP_LANES": "1"}


def test_defaults_owned_by_the_conv_planner_are_the_headers():
    code = re.sub(r"/\*.*?\*/|//[^\n]*", "", _read("pyrapose_amd/csrc/conv_plan.h"), flags=re.S)
    assert {s.env for s in S.SWITCHES if s.owner == "csrc/conv_plan.h"} == {"PP_CONV3_FAST", "PP_SPARSE_DGRAD"}
    # on unless "0" on both sides (the header looks at the first character only; the engine keeps its own, exact test)
    assert re.search(r'pp_env_not0\(\s*"PP_CONV3_FAST"\s*\)', code)
    assert S.EngineSwitches.from_env({}).conv3_fast is True
    n = re.findall(r'pp_env_int\(\s*"PP_SPARSE_DGRAD"\s*,\s*(-?\d+)\s*\)', code)
    assert len(n) == 1 and int(ROWS["PP_SPARSE_DGRAD"].default) == int(n[0])
    assert int(n[0]) != 0 and S.EngineSwitches.from_env({}).sparse_dgrad is True


def test_engine_reads_no_environment_itself():
    text = _read("pyrapose_amd/engine.py")
    assert "environ" not in text and "getenv" not in text
    named = set(re.findall(r"PP_[A-Z0-9_]+", text))
    assert named - set(ROWS) == ONLY_MENTIONED
    assert re.search(r"self\.sw = (sw = )?EngineSwitches\.from_env\(\)", text)


def test_every_row_is_used_by_the_engine():
    text = _read("pyrapose_amd/engine.py")
    for s in S.SWITCHES:
        assert re.search(r"\bsw\.%s\b" % s.field, text), s.env


def test_design_lists_every_switch():
    design = _read("DESIGN.md")
    m = re.search(r"^#+ [^\n]*Engine switches[^\n]*\n(.*?)(?=^#+ )", design, flags=re.S | re.M)
    assert m, "DESIGN.md has no 'Engine switches' section"
    for s in S.SWITCHES:
        row = [l for l in m.group(1).splitlines() if l.startswith("| `%s` |" % s.env)]
        assert len(row) == 1 and s.owner in row[0], s.env
