"""Independent streaming sessions at the C ABI, without a device: the entry points exist and refuse bad arguments before they touch
anything.  (What they compute is tests/test_sessions_gpu.py.)"""
import ctypes as C
import os
import re

from artalk_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SESSION_SYMBOLS = ["artalk_sessions_reserve", "artalk_session_open", "artalk_session_step", "artalk_session_close", "artalk_session_count"]


def test_session_symbols_are_exported_and_declared():
    L = capi.lib()
    header = open(os.path.join(REPO, "include", "artalk_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SESSION_SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/artalk_hip.h"
        assert name in capi.SYMBOLS
        assert getattr(L, name).argtypes is not None, f"{name} has no prototype in capi.lib()"


def test_session_argument_errors_without_gpu():
    """A NULL model or NULL pointers: ARTALK_EINVAL, decided before the device is touched."""
    L = capi.lib()
    ids = (C.c_int64 * 2)(1, 2)
    assert L.artalk_sessions_reserve(None, 8) == capi.EINVAL
    assert L.artalk_session_open(None, 1, None, None, ids, None) == capi.EINVAL
    assert L.artalk_session_step(None, ids, 2, None, 64000, None, 10600, None, None, None) == capi.EINVAL
    assert L.artalk_session_close(None, ids, 2) == capi.EINVAL
    assert L.artalk_session_count(None) == capi.EINVAL
