"""rtgo_whitted_launch_frames without a GPU: the entry is declared in include/rtgo.h, listed in capi.SYMBOLS, exported by the library and
bound, and the ABI's version and sizes stand (rtgo_whitted_frame 44 bytes, rtgo_stats 104 bytes, version 6)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import _build, capi as m
    _build.build_all()
    m.load()
    return m


def _header():
    with open(os.path.join(ROOT, "include", "rtgo.h")) as f:
        return f.read()


def test_entry_is_declared_listed_exported_and_bound(capi):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+rtgo_whitted_launch_frames\s*\(\s*rtgo_ctx\s*\*\s*\w+\s*,\s*const\s+rtgo_whitted_frame\s*\*\s*\w+\s*,"
                     r"\s*uint32_t\s+\w+\s*\)\s*;", code)
    assert "rtgo_whitted_launch_frames" in capi.SYMBOLS
    fn = capi.load().rtgo_whitted_launch_frames
    assert fn is not None
    assert list(fn.argtypes) == [C.c_void_p, C.POINTER(capi.WhittedFrame), C.c_uint32] and fn.restype is C.c_int
    assert callable(getattr(capi.Context, "whitted_launch_frames", None))


def test_header_names_the_reference_lines_that_allow_the_batching():
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+rtgo_whitted_launch_frames\b", _header(), flags=re.S)
    assert m, "no comment ahead of the declaration"
    assert "whitted.cu:226-239" in m.group(1) and "bit for bit" in m.group(1)


def test_abi_version_and_sizes_stand(capi):
    assert capi.load().rtgo_abi_version() == 6
    assert re.search(r"#define\s+RTGO_ABI_VERSION\s+6\b", _header())
    assert C.sizeof(capi.WhittedFrame) == 44
    assert C.sizeof(capi.Stats) == 104
