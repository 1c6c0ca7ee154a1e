"""The ray-query ABI on a CPU-only box: rtgo_trace_rays / rtgo_whitted_trace_rays / rtgo_host_session_pick are declared, exported and
bound, rtgo_ray and rtgo_hit have the layout include/rtgo.h states, and the ABI version has not moved (only entry points were added)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import _build, capi as m
    _build.build_all()
    m.load()
    return m


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_entry_points_are_declared_exported_and_listed(capi):
    from raytracingo_amd import scene
    src = header("rtgo.h")
    for name in ("rtgo_trace_rays", "rtgo_whitted_trace_rays"):
        assert re.search(r"\bint\s+%s\s*\(\s*rtgo_ctx\s*\*[^;]*const\s+void\s*\*[^;]*void\s*\*[^;]*uint32_t[^;]*uint32_t[^;]*\)\s*;" % name, src), name
        assert name in capi.SYMBOLS
        assert getattr(capi.load(), name) is not None
    assert re.search(r"\bint\s+rtgo_host_session_pick\s*\(", header("rtgo_host.h"))
    host = scene.load()
    assert host.rtgo_host_session_pick is not None and host.rtgo_host_session_camera is not None
    for const, value in (("RTGO_TRACE_CLOSEST", 0), ("RTGO_TRACE_ANY_HIT", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (const, value), src), const
    assert re.search(r"#define\s+RTGO_HIT_MISS\s+\(-1\)", src) and re.search(r"#define\s+RTGO_HIT_INVALID\s+\(-2\)", src)
    assert (capi.TRACE_CLOSEST, capi.TRACE_ANY_HIT, capi.HIT_MISS, capi.HIT_INVALID) == (0, 1, -1, -2)


def test_record_layouts(capi):
    assert C.sizeof(capi.Ray) == C.sizeof(capi.Hit) == 32
    assert (capi.Ray.origin.offset, capi.Ray.tmin.offset, capi.Ray.dir.offset, capi.Ray.tmax.offset) == (0, 12, 16, 28)
    assert (capi.Hit.t.offset, capi.Hit.prim.offset, capi.Hit.instance.offset, capi.Hit.u.offset, capi.Hit.v.offset, capi.Hit.n.offset) == (0, 4, 8, 12, 16, 20)
    assert capi.RAY_DTYPE.itemsize == capi.HIT_DTYPE.itemsize == 32
    for dt, st in ((capi.RAY_DTYPE, capi.Ray), (capi.HIT_DTYPE, capi.Hit)):
        for name, _ in st._fields_:
            assert dt.fields[name][1] == getattr(st, name).offset, name
    # the header states the same fields in the same order
    src = header("rtgo.h")
    ray = re.search(r"typedef struct rtgo_ray \{(.*?)\} rtgo_ray;", src, flags=re.S).group(1)
    hit = re.search(r"typedef struct rtgo_hit \{(.*?)\} rtgo_hit;", src, flags=re.S).group(1)
    assert re.findall(r"\b(origin|tmin|dir|tmax)\b", ray) == ["origin", "tmin", "dir", "tmax"]
    assert re.findall(r"\b(t|prim|instance|u|v|n)\b", hit) == ["t", "prim", "instance", "u", "v", "n"]


def test_make_rays_packs_the_record(capi):
    r = capi.make_rays([[1, 2, 3], [4, 5, 6]], [[0, 0, -1]], tmin=0.5, tmax=[7, 8])
    assert r.dtype == capi.RAY_DTYPE and len(r) == 2
    assert np.array_equal(r.view(np.float32).reshape(2, 8), np.float32([[1, 2, 3, 0.5, 0, 0, -1, 7], [4, 5, 6, 0.5, 0, 0, -1, 8]]))


def test_abi_version_and_sizes_have_not_moved(capi):
    assert capi.load().rtgo_abi_version() == 6
    assert C.sizeof(capi.Stats) == 104 and C.sizeof(capi.Frame) == 64 and C.sizeof(capi.Prim) == 108
