"""rtgo_whitted_rebuild_meshes in the C ABI: declared in include/rtgo.h with rtgo_whitted_update_meshes's signature, listed in
capi.SYMBOLS, exported by the library, bound with the header's signature; the ABI version has not moved (an addition).  No compute calls:
runs on a CPU-only box."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rtgo_whitted_rebuild_meshes"


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import _build, capi as m
    _build.build_all()
    m.load()
    return m


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtgo.h")).read(), flags=re.S)


def arguments(name):
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header())
    assert decl, name + " is not declared in include/rtgo.h"
    return [" ".join(a.split()) for a in decl.group(1).split(",")]


def test_rebuild_meshes_is_declared_listed_exported_and_bound(capi):
    assert arguments(NAME) == ["rtgo_ctx* ctx", "const rtgo_whitted_mesh_update* updates", "uint32_t n_updates"]
    assert arguments(NAME) == arguments("rtgo_whitted_update_meshes"), "the two calls take the same arguments"
    assert NAME in capi.SYMBOLS
    fn = getattr(capi.load(), NAME)
    assert fn.argtypes == [C.c_void_p, C.POINTER(capi.WhittedMeshUpdate), C.c_uint32] and fn.restype is C.c_int
    assert callable(getattr(capi.Context, "whitted_rebuild_meshes"))


def test_abi_version_has_not_moved(capi):
    assert capi.load().rtgo_abi_version() == 6
    assert re.search(r"#define\s+RTGO_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "rtgo.h")).read())


def test_a_null_context_is_refused_without_a_device(capi):
    assert getattr(capi.load(), NAME)(None, None, 0) != 0
