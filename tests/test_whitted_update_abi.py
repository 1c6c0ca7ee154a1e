"""rtgo_whitted_update_mesh in the C ABI: declared in include/rtgo.h, listed in capi.SYMBOLS, exported by the library; the ABI version
has not moved (an addition).  No compute calls: runs on a CPU-only box."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rtgo_whitted_update_mesh"


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import _build, capi as m
    _build.build_all()
    m.load()
    return m


def test_update_mesh_is_declared_listed_and_exported(capi):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtgo.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, src)
    assert decl, "not declared in include/rtgo.h"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["rtgo_ctx* ctx", "uint32_t mesh", "const float* positions", "const float* normals", "uint32_t n_vertices"]
    assert NAME in capi.SYMBOLS
    L = capi.load()
    assert getattr(L, NAME) is not None
    assert len(L.rtgo_whitted_update_mesh.argtypes) == 5
    assert callable(getattr(capi.Context, "whitted_update_mesh"))


def test_abi_version_has_not_moved(capi):
    assert capi.load().rtgo_abi_version() == 6
    src = open(os.path.join(ROOT, "include", "rtgo.h")).read()
    assert re.search(r"#define\s+RTGO_ABI_VERSION\s+6\b", src)


def test_a_null_context_is_refused_without_a_device(capi):
    assert capi.load().rtgo_whitted_update_mesh(None, 0, None, None, 0) != 0
