"""rtgo_update_prims without a GPU: the entry is declared in include/rtgo.h with its six arguments and its two flag values, listed in
capi.SYMBOLS, exported by the library and bound; its comment names the OptiX operation it stands for and states every refusal; the ABI's
version stands at 6; the session's call is declared in include/rtgo_host.h and exported; a NULL context is refused before anything else
is looked at."""
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


def _header(name="rtgo.h"):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_entry_is_declared_listed_exported_and_bound(capi):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+rtgo_update_prims\s*\(\s*rtgo_ctx\s*\*\s*\w+\s*,\s*const\s+uint32_t\s*\*\s*\w+\s*,\s*const\s+rtgo_prim\s*\*\s*\w+\s*,"
                     r"\s*const\s+rtgo_aabb\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*\)\s*;", code)
    assert "rtgo_update_prims" in capi.SYMBOLS
    fn = capi.load().rtgo_update_prims
    assert list(fn.argtypes) == [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(capi.Prim), C.POINTER(capi.Aabb), C.c_uint32, C.c_uint32]
    assert fn.restype is C.c_int
    assert callable(getattr(capi.Context, "update_prims", None))


def test_flag_values(capi):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bRTGO_UPDATE_REFIT\s*=\s*0\b", code) and re.search(r"\bRTGO_UPDATE_REBUILD\s*=\s*1\b", code)
    assert (capi.UPDATE_REFIT, capi.UPDATE_REBUILD) == (0, 1)


def test_header_states_the_contract():
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+rtgo_update_prims\b", _header(), flags=re.S)
    assert m, "no comment ahead of the declaration"
    text = m.group(1)
    for phrase in ("OPTIX_BUILD_OPERATION_UPDATE", "optixAccelBuild", "SBT", "bit for bit", "Synchronous", "RTGO_E_STATE", "RTGO_E_INVALID",
                   "RTGO_E_UNSUPPORTED", "named twice", "unknown flag bits", "n_updates == 0", "leaves the scene as it was", "CubeBox"):
        assert phrase in text, phrase


def test_abi_version_and_sizes_stand(capi):
    assert capi.load().rtgo_abi_version() == 6
    assert re.search(r"#define\s+RTGO_ABI_VERSION\s+6\b", _header())
    assert C.sizeof(capi.Stats) == 104 and C.sizeof(capi.Prim) == 108 and C.sizeof(capi.Aabb) == 24


def test_session_entry_is_declared_and_exported(capi):
    from raytracingo_amd import scene
    code = re.sub(r"/\*.*?\*/", "", _header("rtgo_host.h"), flags=re.S)
    assert re.search(r"\bint\s+rtgo_host_session_update_prims\s*\(\s*rtgo_host_session\s*\*\s*\w+\s*,\s*const\s+uint32_t\s*\*\s*\w+\s*,"
                     r"\s*const\s+rtgo_prim\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)\s*;", code)
    assert scene.load().rtgo_host_session_update_prims is not None
    assert callable(getattr(scene.Session, "update_prims", None))


def test_null_context_is_refused(capi):
    # (no device is touched: the context is looked at first)
    assert capi.load().rtgo_update_prims(None, None, None, None, 0, 0) == 1   # RTGO_E_INVALID
