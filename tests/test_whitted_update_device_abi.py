"""rtgo_whitted_update_meshes_device in the C ABI: declared in include/rtgo.h with the header's signature, listed in capi.SYMBOLS, exported
by the library and bound with that signature; the ABI version has not moved (an addition).  No compute calls: runs on a CPU-only box."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rtgo_whitted_update_meshes_device"


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import _build, capi as m
    _build.build_all()
    m.load()
    return m


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtgo.h")).read(), flags=re.S)


def test_the_call_is_declared_listed_exported_and_bound(capi):
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, header())
    assert decl, "not declared in include/rtgo.h"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["rtgo_ctx* ctx", "const rtgo_whitted_mesh_update* updates", "uint32_t n_updates", "uint32_t flags"]
    assert NAME in capi.SYMBOLS
    fn = getattr(capi.load(), NAME)
    assert fn.argtypes == [C.c_void_p, C.POINTER(capi.WhittedMeshUpdate), C.c_uint32, C.c_uint32] and fn.restype is C.c_int
    assert callable(getattr(capi.Context, "whitted_update_meshes_device"))


def test_the_flags_are_the_update_enum(capi):
    assert re.search(r"enum\s*\{\s*RTGO_UPDATE_REFIT\s*=\s*0\s*,\s*RTGO_UPDATE_REBUILD\s*=\s*1\s*\}", header())
    assert (capi.UPDATE_REFIT, capi.UPDATE_REBUILD) == (0, 1)


def test_abi_version_has_not_moved(capi):
    assert capi.load().rtgo_abi_version() == 6
    assert re.search(r"#define\s+RTGO_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "rtgo.h")).read())


def test_a_null_context_is_refused_without_a_device(capi):
    L = capi.load()
    for flags in (capi.UPDATE_REFIT, capi.UPDATE_REBUILD, 2):
        assert L.rtgo_whitted_update_meshes_device(None, None, 0, flags) == 1   # RTGO_E_INVALID
