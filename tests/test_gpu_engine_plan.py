"""GPU: the launch plan the Engine builds under each of its switches is the one recorded in tests/golden/engine_plans.json
(made by tests/golden/make_engine_plans.py from the commit named in the file's `made_at`, with a restatement of
Engine.plan_signature() that reads the engine from outside).  Construction alone makes the plan: no step runs.  Equality, so
there is no tolerance: order, names, kinds and lanes of every launch, format / laziness / flags of every plane-stored gradient,
the route of every stride-2 data gradient."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "engine_plans.json")) as f:
    GOLD = json.load(f)
PLANS = GOLD["plans"]
SIZE = dict(B=2, H=97, W=131, C=5)  # tests/test_gpu_pipeline.py: the smallest at which every pyramid level and the sparse head exist
# the settings the plans must cover at that size (PP_* = value, or the constructor's conv_mode)
REQUIRED = [{}, {"PP_LANES": "1"}, {"PP_LANES": "3"}, {"PP_TRUNK_LANES": "0"}, {"PP_SPARSE_BWD": "0"}, {"PP_SPARSE_FWD": "1"},
            {"PP_SPARSE_INPLACE": "0"}, {"PP_SPARSE_WITHIN": "0"}, {"PP_SPARSE_LAZY": "0"}, {"PP_PLANES": "0"},
            {"PP_PLANES": "0", "PP_CAPTURE": "1"}, {"PP_PREFETCH": "1"}, {"PP_STEM3": "0"},
            {"conv_mode": "bf16x3"}, {"conv_mode": "f16c8"}, {"conv_mode": "f32"}]


@pytest.fixture(scope="module")
def ctx():
    from pyrapose_amd.runtime import default_context
    return default_context()


@pytest.fixture(scope="module")
def weights():
    from pyrapose_amd import arch
    return arch.init_weights(SIZE["C"], seed=0)


def test_settings_cover_the_table():
    from pyrapose_amd.switches import SWITCHES
    have = [dict(p["env"], **p["kwargs"]) for p in PLANS if p["size"] == SIZE]
    assert all(p["size"]["C"] == SIZE["C"] for p in PLANS)
    assert all(r in have for r in REQUIRED)
    used = {k for p in PLANS for k in p["env"]}
    assert {s.env for s in SWITCHES if s.owner == "engine"} <= used
    assert used <= {s.env for s in SWITCHES}
    assert len({json.dumps(p["plan"], sort_keys=True) for p in PLANS}) == len(PLANS)  # (no two settings record the same thing)
    # at the second size (32 rows per image at every level) the gradients inside the sparse head are lazy, and the switch decides it
    lazy = {p["id"]: sum(g[3] for g in p["plan"]["plane_grads"]) for p in PLANS}
    assert lazy["lazy_size_defaults"] > 0 and lazy["lazy_size_sparse_lazy0"] == 0 and lazy["lazy_size_sparse_within0"] == 0


@pytest.mark.parametrize("rec", PLANS, ids=[p["id"] for p in PLANS])
def test_plan_is_the_recorded_one(ctx, weights, monkeypatch, rec):
    from pyrapose_amd.engine import Engine
    from pyrapose_amd.switches import SWITCHES
    for s in SWITCHES:
        monkeypatch.delenv(s.env, raising=False)
    for k, v in rec["env"].items():
        monkeypatch.setenv(k, v)
    sz = rec["size"]
    eng = Engine(ctx, sz["C"], sz["B"], sz["H"], sz["W"], weights=weights, train=True, **rec["kwargs"])
    try:
        got = eng.plan_signature()
    finally:
        eng.close()
    got = json.loads(json.dumps(got))  # (serialisable, and tuples as the lists the file holds)
    assert sorted(got) == sorted(rec["plan"])
    for key in sorted(got):
        assert got[key] == rec["plan"][key], key
