"""dvbs2hip_set_streams without a GPU: the entry exists in header, binding and library (tests/test_abi.py holds the three to one another) and refuses a null handle."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_streams_is_declared_bound_and_exported():
    from dvbs2_amd import lib_binding as B
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvbs2hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+dvbs2hip_set_streams\s*\(\s*dvbs2hip_t\s*\*\s*h\s*,\s*int32_t\s+S\s*\)\s*;", txt)
    assert "dvbs2hip_set_streams" in B.ABI
    assert hasattr(B.load(), "dvbs2hip_set_streams")


def test_set_streams_refuses_a_null_handle():
    from dvbs2_amd import lib_binding as B
    L = B.load()
    assert L.dvbs2hip_set_streams(None, 2) == -1                   # DVBS2HIP_EINVAL
    assert L.dvbs2hip_set_streams(ctypes.c_void_p(), 1) == -1
