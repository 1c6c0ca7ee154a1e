"""rtgo_whitted_update_meshes in the C ABI: declared in include/rtgo.h with the struct it takes, listed in capi.SYMBOLS, exported by the
library, bound with the header's signature; the ABI version has not moved (an addition).  No compute calls: runs on a CPU-only box."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rtgo_whitted_update_meshes"


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import _build, capi as m
    _build.build_all()
    m.load()
    return m


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtgo.h")).read(), flags=re.S)


def test_the_struct_is_laid_out_as_the_header_declares_it(capi):
    body = re.search(r"typedef\s+struct\s+rtgo_whitted_mesh_update\s*\{(.*?)\}\s*rtgo_whitted_mesh_update\s*;", header(), flags=re.S)
    assert body, "rtgo_whitted_mesh_update is not declared in include/rtgo.h"
    fields = [" ".join(f.split()) for f in body.group(1).split(";") if f.strip()]
    assert fields == ["uint32_t mesh", "const float* positions", "const float* normals", "uint32_t n_vertices"]
    U = capi.WhittedMeshUpdate
    assert [name for name, _ in U._fields_] == [f.split()[-1] for f in fields]
    # a C compiler on this ABI: the pointers aligned to their size, the struct padded to a multiple of it
    ptr = C.sizeof(C.c_void_p)
    assert (U.mesh.offset, U.positions.offset, U.normals.offset, U.n_vertices.offset) == (0, ptr, 2 * ptr, 3 * ptr)
    assert C.sizeof(U) == 4 * ptr and C.alignment(U) == ptr
    assert U.mesh.size == U.n_vertices.size == 4 and U.positions.size == U.normals.size == ptr


def test_update_meshes_is_declared_listed_and_exported(capi):
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, header())
    assert decl, "not declared in include/rtgo.h"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["rtgo_ctx* ctx", "const rtgo_whitted_mesh_update* updates", "uint32_t n_updates"]
    assert NAME in capi.SYMBOLS
    fn = getattr(capi.load(), NAME)
    assert fn.argtypes == [C.c_void_p, C.POINTER(capi.WhittedMeshUpdate), C.c_uint32] and fn.restype is C.c_int
    assert callable(getattr(capi.Context, "whitted_update_meshes"))


def test_abi_version_has_not_moved(capi):
    assert capi.load().rtgo_abi_version() == 6
    assert re.search(r"#define\s+RTGO_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "rtgo.h")).read())


def test_a_null_context_is_refused_without_a_device(capi):
    assert capi.load().rtgo_whitted_update_meshes(None, None, 0) != 0
