"""rtgo_set_large_scene on a CPU-only box: declared, exported, its limit agrees between the header and the binding, and a NULL context is
refused before anything touches a device."""
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


def header():
    return open(os.path.join(ROOT, "include", "rtgo.h")).read()


def test_declared_and_exported(capi):
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+rtgo_set_large_scene\s*\(\s*rtgo_ctx\s*\*\s*ctx\s*,\s*const\s+rtgo_prim\s*\*\s*prims\s*,"
                     r"\s*const\s+rtgo_aabb\s*\*\s*aabbs\s*,\s*uint32_t\s+n\s*\)\s*;", src)
    assert "rtgo_set_large_scene" in capi.SYMBOLS
    assert capi.load().rtgo_set_large_scene is not None


def test_limit_matches_header(capi):
    m = re.search(r"#define\s+RTGO_MAX_SCENE_PRIMS\s+\(1\s*<<\s*(\d+)\)", header())
    assert m is not None
    assert capi.RTGO_MAX_SCENE_PRIMS == 1 << int(m.group(1)) == 1 << 20
    assert capi.RTGO_MAX_PRIMS == 512   # rtgo_set_scene's limit does not move


def test_prim_record_packing(capi):
    """the numpy record set_large_scene packs is rtgo_prim field for field"""
    assert capi.PRIM_DTYPE.itemsize == C.sizeof(capi.Prim)
    for name, off in (("type", 0), ("model", 4), ("kd", 68), ("kr", 80), ("specularity", 92), ("Le", 96)):
        assert capi.PRIM_DTYPE.fields[name][1] == off == getattr(capi.Prim, name).offset


def test_null_context_is_invalid(capi):
    L = capi.load()
    prims = (capi.Prim * 2)()
    assert L.rtgo_set_large_scene(None, prims, None, 2) == 1          # RTGO_E_INVALID
    assert L.rtgo_set_large_scene(None, None, None, 0) == 1

