#!/usr/bin/env python3
"""Writes tests/golden/engine_plans.json: the launch plan the Engine builds under each setting of SETTINGS, at the size of
tests/test_gpu_pipeline.py (and, for the lazy sparse gradients, which need 32 rows per image at every level, at the smallest
size that has them).  Needs the MI355X (constructing an engine allocates its buffers); no step runs.

The file pins what a refactor of the engine must not change, so it is made from the commit BEFORE such a change: run

    PYTHONPATH=<checkout of that commit, built> python tests/golden/make_engine_plans.py --commit <its hash>

`signature` below reads an engine object from outside (it is Engine.plan_signature() restated), so it works on commits that
have no such method; without PYTHONPATH the script uses the tree it lies in.  tests/test_gpu_engine_plan.py takes its
settings from the file written here and compares Engine.plan_signature() with the recorded plans for equality."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.dirname(os.path.dirname(HERE)))  # (append: a checkout named in PYTHONPATH wins)

SIZE = dict(B=2, H=97, W=131, C=5)        # tests/test_gpu_pipeline.py: the smallest at which every pyramid level and the sparse head exist
LAZY_SIZE = dict(B=1, H=161, W=193, C=5)  # level 5 is 6 x 7: the smallest level has the 32 rows per image a lazy sparse gradient needs

# (id, environment, Engine keyword arguments[, size]).  Every value differs from the switch's default, so `env` is also what
# EngineSwitches.non_default() reports.  The engine trains with conv1 + res2 frozen by default: PP_PREFETCH needs no argument.
SETTINGS = [
    ("defaults", {}, {}),
    ("lanes1", {"PP_LANES": "1"}, {}),
    ("lanes3", {"PP_LANES": "3"}, {}),
    ("trunk_lanes0", {"PP_TRUNK_LANES": "0"}, {}),
    ("mask_lane0", {"PP_MASK_LANE": "0"}, {}),
    ("sparse_bwd0", {"PP_SPARSE_BWD": "0"}, {}),
    ("sparse_fwd1", {"PP_SPARSE_FWD": "1"}, {}),
    ("sparse_inplace0", {"PP_SPARSE_INPLACE": "0"}, {}),
    ("sparse_within0", {"PP_SPARSE_WITHIN": "0"}, {}),
    ("sparse_lazy0", {"PP_SPARSE_LAZY": "0"}, {}),
    ("planes0", {"PP_PLANES": "0"}, {}),
    ("planes0_capture1", {"PP_PLANES": "0", "PP_CAPTURE": "1"}, {}),
    ("planes0_capture1_min512_skip_heads", {"PP_PLANES": "0", "PP_CAPTURE": "1", "PP_CAPTURE_MIN_CIN": "512", "PP_CAPTURE_SKIP": "cls,mask"}, {}),
    ("prefetch1", {"PP_PREFETCH": "1"}, {}),
    ("prefetch1_after_res3a", {"PP_PREFETCH": "1", "PP_PREFETCH_AFTER": "res3a_branch2a"}, {}),
    ("stem3_0", {"PP_STEM3": "0"}, {}),
    ("splitk_mb0", {"PP_SPLITK_MB": "0"}, {}),
    ("env_conv_mode_f16c8", {"PP_CONV_MODE": "f16c8"}, {}),
    ("conv_mode_bf16x3", {}, {"conv_mode": "bf16x3"}),
    ("conv_mode_f16c8", {}, {"conv_mode": "f16c8"}),
    ("conv_mode_f32", {}, {"conv_mode": "f32"}),
    ("lazy_size_defaults", {}, {}, LAZY_SIZE),
    ("lazy_size_sparse_lazy0", {"PP_SPARSE_LAZY": "0"}, {}, LAZY_SIZE),
    ("lazy_size_sparse_within0", {"PP_SPARSE_WITHIN": "0"}, {}, LAZY_SIZE),
]


def signature(eng, env):
    launches = lambda plan: [[o.kind, o.name, o.lane] for o in plan]
    return dict(fwd_ops=launches(eng.fwd_ops), bwd_ops=launches(eng.bwd_ops),
                plane_grads=[list(g.shape()) + [g.fmt, bool(g.lazy), g.within is not None] for g in eng._plane_grads],
                s2_grads=[[layer, route] for layer, _, route in eng._s2_grads],
                arith=eng.arith, n_lanes=eng.n_lanes, prefix_lane=eng.prefix_lane, switches=dict(env))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose pyrapose_amd is imported (recorded in the file)")
    ap.add_argument("--out", default=os.path.join(HERE, "engine_plans.json"))
    args = ap.parse_args()
    from pyrapose_amd import arch
    from pyrapose_amd.engine import Engine
    from pyrapose_amd.runtime import default_context
    ctx = default_context()
    weights = arch.init_weights(SIZE["C"], seed=0)
    ours = sorted({k for s in SETTINGS for k in s[1]} & set(os.environ))
    assert not ours, "unset %s first: the plans are those of a clean environment" % ours
    plans = []
    for name, env, kwargs, size in [(tuple(s) + (SIZE,))[:4] for s in SETTINGS]:
        os.environ.update(env)
        try:
            eng = Engine(ctx, size["C"], size["B"], size["H"], size["W"], weights=weights, train=True, **kwargs)
            plans.append(dict(id=name, env=env, kwargs=kwargs, size=size, plan=signature(eng, env)))
            eng.close()
        finally:
            for k in env:
                del os.environ[k]
        p = plans[-1]["plan"]
        print(name, len(p["fwd_ops"]), "forward,", len(p["bwd_ops"]), "backward launches,", sum(g[3] for g in p["plane_grads"]), "lazy gradients")
    with open(args.out, "w") as f:  # one setting per line
        f.write('{"made_at": %s, "plans": [\n%s\n]}\n' % (json.dumps(args.commit), ",\n".join(json.dumps(p, sort_keys=True) for p in plans)))


if __name__ == "__main__":
    main()
