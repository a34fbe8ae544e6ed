"""The PP_* environment switches the Engine's launch plan depends on: one table, read once per engine
(Engine.__init__: `self.sw = EngineSwitches.from_env()`).  Pure Python -- no torch, no shared library -- so the table can be
checked and printed anywhere.  The switches of the conv kernels themselves live in csrc/conv_plan.h; the two
of them the engine also looks at are listed here with that header as their owner, and a test keeps the defaults equal."""
import dataclasses
import os
from collections import namedtuple

# rule: raw string (or the default, where unset) -> value of the field.  default: the raw string an unset variable stands for.
Switch = namedtuple("Switch", "env field rule default owner doc")


def _not0(v):
    return v != "0"


def _is1(v):
    return v == "1"


def _names(v):
    return tuple(t for t in v.split(",") if t)


def _names_not0(v):
    return tuple(t for t in v.split(",") if t and t != "0")


def _lanes(v):
    return max(1, min(3, int(v)))


def _opt_int(v):
    return None if v is None else int(v)


def _opt_str(v):
    return v


ENGINE, CONV_PLAN = "engine", "csrc/conv_plan.h"

SWITCHES = (
    Switch("PP_CONV_MODE", "conv_mode", str, "mixed", ENGINE,
           "conv arithmetic: f32 / bf16x3 / f16c8 / mixed (backbone bf16x3, FPN + heads f16c8); Engine(conv_mode=) wins"),
    Switch("PP_PLANES", "planes", _not0, "1", ENGINE,
           "activations and gradients stored as 16-bit plane pairs; 0 = float32 storage (bf16x3 arithmetic only)"),
    Switch("PP_CAPTURE", "capture", _is1, "0", ENGINE,
           "float32 storage only: 3x3 stride-1 launches also store the bf16 split of their operand for the weight gradient"),
    Switch("PP_CAPTURE_MIN_CIN", "capture_min_cin", int, "64", ENGINE, "fewest input channels of a layer that captures"),
    Switch("PP_CAPTURE_SKIP", "capture_skip", _names, "", ENGINE, "comma list of layer-name prefixes that never capture"),
    Switch("PP_SPARSE_BWD", "sparse_bwd", _names_not0, "reg", ENGINE,
           "comma list of head prefixes whose backward skips the 32-row blocks without a non-zero gradient; 0 = none"),
    Switch("PP_SPARSE_FWD", "sparse_fwd", _is1, "0", ENGINE,
           "training steps compute the 3D-box head's forward on the blocks its loss reads only"),
    Switch("PP_SPARSE_INPLACE", "sparse_inplace", _not0, "1", ENGINE,
           "a sparse data gradient that only adds to the earlier ones works in place on their sum"),
    Switch("PP_SPARSE_WITHIN", "sparse_within", _not0, "1", ENGINE,
           "a sparse data gradient without addend hands the flags of the blocks it wrote to its readers"),
    Switch("PP_SPARSE_LAZY", "sparse_lazy", _not0, "1", ENGINE,
           "such a gradient stays unwritten outside those blocks where every reader goes by the flags (no fill pass)"),
    Switch("PP_LANES", "lanes", _lanes, "2", ENGINE, "launch lanes (streams), clamped to 1..3; 1 serialises everything on lane 0"),
    Switch("PP_TRUNK_LANES", "trunk_lanes", _not0, "1", ENGINE, "backbone shortcut and FPN level 4-5 chains on lane 1"),
    Switch("PP_MASK_LANE", "mask_lane", _opt_int, None, ENGINE,
           "lane of the mask head; unset: beside the class head at two lanes (lane 0 with the sparse forward), else lane 2"),
    Switch("PP_SPLITK_MB", "splitk_mb", int, "256", ENGINE, "split-K / weight-gradient slice scratch per lane in MiB; 0 = none"),
    Switch("PP_PREFETCH", "prefetch", _is1, "0", ENGINE,
           "frozen prefix (conv1 + res2) on a stream of its own, so that the next batch's can run beside this batch's trunk"),
    Switch("PP_PREFETCH_AFTER", "prefetch_after", _opt_str, None, ENGINE,
           "name of the lane-0 forward launch after which the next batch's prefix is released; unset: as early as possible"),
    Switch("PP_STEM3", "stem3", _not0, "1", ENGINE, "conv1 as the row-as-tap bf16x3 stem kernel (needs PP_CONV3_FAST)"),
    Switch("PP_CONV3_FAST", "conv3_fast", _not0, "1", CONV_PLAN,
           "buffer-addressed conv loops; the engine asks because the stem and the lazy sparse gradients are forms of them"),
    Switch("PP_SPARSE_DGRAD", "sparse_dgrad", _not0, "22", CONV_PLAN,
           "tile of the listed-block data gradient; the engine only asks whether it is 0 (dense grid: nothing stays lazy)"),
)


def _from_env(cls, environ=None):
    """the switches as `environ` (any mapping; default os.environ) sets them; reads only"""
    environ = os.environ if environ is None else environ
    raw = tuple((s.env, environ[s.env]) for s in SWITCHES if s.env in environ)
    given = dict(raw)
    return cls(*(s.rule(given.get(s.env, s.default)) for s in SWITCHES), _raw=raw)


def _non_default(self):
    """{environment name: raw string} of every switch that was set to something other than its default"""
    given = dict(self._raw)
    return {s.env: given[s.env] for s in SWITCHES if s.env in given and getattr(self, s.field) != s.rule(s.default)}


EngineSwitches = dataclasses.make_dataclass(
    "EngineSwitches", [s.field for s in SWITCHES] + [("_raw", tuple, dataclasses.field(default=(), compare=False, repr=False))],
    frozen=True, namespace=dict(from_env=classmethod(_from_env), non_default=_non_default,
                                __doc__="One value per row of SWITCHES (field names: its second column), immutable."))
