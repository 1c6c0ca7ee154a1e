"""rtgo_whitted_shade_rays without a GPU: the entry is declared in include/rtgo.h with its six arguments, listed in capi.SYMBOLS, exported
by the library and bound, its comment states the contract, and the ABI's version and sizes stand (rtgo_stats 104 bytes, version 6)."""
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
    assert re.search(r"\bint\s+rtgo_whitted_shade_rays\s*\(\s*rtgo_ctx\s*\*\s*\w+\s*,\s*const\s+void\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*,"
                     r"\s*void\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*\)\s*;", code)
    assert "rtgo_whitted_shade_rays" in capi.SYMBOLS
    fn = capi.load().rtgo_whitted_shade_rays
    assert fn is not None
    assert list(fn.argtypes) == [C.c_void_p] * 4 + [C.c_uint32] * 2 and fn.restype is C.c_int
    assert callable(getattr(capi.Context, "whitted_shade_rays", None)) and callable(getattr(capi.Context, "whitted_shade_rays_raw", None))


def test_header_states_the_contract():
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+rtgo_whitted_shade_rays\b", _header(), flags=re.S)
    assert m, "no comment ahead of the declaration"
    text = m.group(1)
    for phrase in ("whitted.cu:226-239", "bit for bit", "rtgo_whitted_trace_rays", "sample_index", "RTGO_E_INVALID", "RTGO_E_STATE", "rays_occlusion"):
        assert phrase in text, phrase


def test_abi_version_and_sizes_stand(capi):
    assert capi.load().rtgo_abi_version() == 6
    assert re.search(r"#define\s+RTGO_ABI_VERSION\s+6\b", _header())
    assert C.sizeof(capi.Stats) == 104 and C.sizeof(capi.Ray) == 32
