"""The reference's utils/__init__.py:1 re-exports reproj, add, adi, re, te from utils/pose_error.py.  Here they resolve on
first use (module __getattr__), so that importing a host-only submodule such as utils.anchors does not load the HIP library.
mssd / mspd (BOP's symmetry-aware errors) come beside them."""
_POSE_ERROR_NAMES = ("reproj", "add", "adi", "re", "te", "mssd", "mspd")
__all__ = list(_POSE_ERROR_NAMES)


def __getattr__(name):
    if name in _POSE_ERROR_NAMES:
        from . import pose_error
        return getattr(pose_error, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
