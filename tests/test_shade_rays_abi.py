"""rtgo_shade_rays without a GPU: the entry is declared in include/rtgo.h with its seven arguments, listed in capi.SYMBOLS, exported by
the library and bound; rtgo_shade_options is 16 bytes in the header's field order; its comment states the contract; the ABI's version
stands at 6; a NULL context is refused before anything else is looked at."""
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
    assert re.search(r"\bint\s+rtgo_shade_rays\s*\(\s*rtgo_ctx\s*\*\s*\w+\s*,\s*const\s+void\s*\*\s*\w+\s*,\s*const\s+void\s*\*\s*\w+\s*,"
                     r"\s*void\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*const\s+rtgo_shade_options\s*\*\s*\w+\s*\)\s*;", code)
    assert "rtgo_shade_rays" in capi.SYMBOLS
    fn = capi.load().rtgo_shade_rays
    assert fn is not None
    assert list(fn.argtypes) == [C.c_void_p] * 5 + [C.c_uint32, C.POINTER(capi.ShadeOptions)] and fn.restype is C.c_int
    assert callable(getattr(capi.Context, "shade_rays", None)) and callable(getattr(capi.Context, "shade_rays_raw", None))


def test_options_struct_is_16_bytes_in_the_header_order(capi):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"typedef\s+struct\s+rtgo_shade_options\s*\{(.*?)\}\s*rtgo_shade_options\s*;", code, flags=re.S)
    assert m, "rtgo_shade_options is not declared"
    fields = re.findall(r"(u?int32_t)\s+(\w+)\s*;", m.group(1))
    assert fields == [("int32_t", "max_trace_depth"), ("uint32_t", "path_tracing"), ("uint32_t", "use_ambient"), ("uint32_t", "sample_index")]
    assert C.sizeof(capi.ShadeOptions) == 16
    assert [(n, t) for n, t in capi.ShadeOptions._fields_] == [("max_trace_depth", C.c_int32), ("path_tracing", C.c_uint32),
                                                               ("use_ambient", C.c_uint32), ("sample_index", C.c_uint32)]


def test_header_states_the_contract():
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+rtgo_shade_rays\b", _header(), flags=re.S)
    assert m, "no comment ahead of the declaration"
    text = m.group(1)
    for phrase in ("kernel.cu:239-246", "bit for bit", "tea<16>(i, sample_index)", "unit vector", "1e-5", "RTGO_E_INVALID", "RTGO_E_UNSUPPORTED",
                   "RTGO_E_STATE", "rays_occlusion", "launches_trial"):
        assert phrase in text, phrase


def test_abi_version_and_sizes_stand(capi):
    assert capi.load().rtgo_abi_version() == 6
    assert re.search(r"#define\s+RTGO_ABI_VERSION\s+6\b", _header())
    assert C.sizeof(capi.Stats) == 104 and C.sizeof(capi.Ray) == 32


def test_null_context_is_refused(capi):
    # (no device is touched: the context is looked at first)
    opt = capi.ShadeOptions(5, 1, 0, 0)
    rc = capi.load().rtgo_shade_rays(None, None, None, None, None, 0, C.byref(opt))
    assert rc != 0
    assert rc == capi.load().rtgo_whitted_shade_rays(None, None, None, None, 0, 0)   # RTGO_E_INVALID, as there
