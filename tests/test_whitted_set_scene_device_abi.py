"""rtgo_whitted_set_scene_device, rtgo_whitted_set_mesh_device and rtgo_whitted_set_texcoords_device in the C ABI: declared in
include/rtgo.h with the header's signatures, listed in capi.SYMBOLS, exported by the library and bound with those signatures; the ABI
version has not moved (additions).  Also the binding's validators, which need no device: device_mesh_args and device_mesh_tensor refuse
what the calls could not read.  No compute calls: runs on a CPU-only box."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u32 = C.c_void_p, C.c_uint32
CALLS = {
    "rtgo_whitted_set_scene_device": (["rtgo_ctx* ctx", "const rtgo_whitted_mesh* meshes", "uint32_t n_meshes", "const rtgo_whitted_instance* instances",
                                       "uint32_t n_instances", "const rtgo_pbr* materials", "uint32_t n_materials"], "whitted_set_scene_device"),
    "rtgo_whitted_set_mesh_device": (["rtgo_ctx* ctx", "const void* d_positions", "const void* d_normals", "uint32_t n_vertices", "const void* d_indices",
                                      "const void* d_material_of_triangle", "uint32_t n_triangles", "const rtgo_pbr* materials", "uint32_t n_materials"],
                                     "whitted_set_mesh_device"),
    "rtgo_whitted_set_texcoords_device": (["rtgo_ctx* ctx", "const void* d_uv", "uint32_t n_vertices"], "whitted_set_texcoords_device"),
}


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import _build, capi as m
    _build.build_all()
    m.load()
    return m


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtgo.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_the_call_is_declared_listed_exported_and_bound(capi, name):
    want, method = CALLS[name]
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header())
    assert decl, "not declared in include/rtgo.h"
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == want
    assert name in capi.SYMBOLS
    fn = getattr(capi.load(), name)
    bound = {"rtgo_whitted_set_scene_device": [vp, C.POINTER(capi.WhittedMesh), u32, C.POINTER(capi.WhittedInstance), u32, vp, u32],
             "rtgo_whitted_set_mesh_device": [vp, vp, vp, u32, vp, vp, u32, vp, u32], "rtgo_whitted_set_texcoords_device": [vp, vp, u32]}[name]
    assert fn.argtypes == bound and fn.restype is C.c_int
    assert callable(getattr(capi.Context, method))


def test_the_signatures_are_the_twins_with_device_pointers(capi):
    """the scene call's is the twin's own; the other two take const void* where the twins take typed host pointers"""
    def args(name):
        return [" ".join(a.split()) for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header()).group(1).split(",")]
    assert args("rtgo_whitted_set_scene_device") == args("rtgo_whitted_set_scene")
    for name in ("rtgo_whitted_set_mesh", "rtgo_whitted_set_texcoords"):
        twin, dev = args(name), args(name + "_device")
        assert len(twin) == len(dev)
        for a, b in zip(twin, dev):
            assert a == b or (b.startswith("const void* d_") and a.split()[-1] == b.split()[-1][2:]), (a, b)


def test_abi_version_has_not_moved(capi):
    assert capi.load().rtgo_abi_version() == 6
    assert re.search(r"#define\s+RTGO_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "rtgo.h")).read())


def test_a_null_context_is_refused_without_a_device(capi):
    L = capi.load()
    assert L.rtgo_whitted_set_scene_device(None, None, 0, None, 0, None, 0) == 1   # RTGO_E_INVALID
    assert L.rtgo_whitted_set_mesh_device(None, None, None, 0, None, None, 0, None, 0) == 1
    assert L.rtgo_whitted_set_texcoords_device(None, None, 0) == 1


def test_the_validators_refuse_what_the_calls_could_not_read(capi):
    import torch
    who = "whitted_set_scene_device: mesh 0"
    pos, idx = torch.zeros((5, 3), dtype=torch.float32), torch.zeros((4, 3), dtype=torch.int32)
    uv, tm = torch.zeros((5, 2), dtype=torch.float32), torch.zeros(4, dtype=torch.int32)
    bad = {
        "numpy positions": dict(positions=np.zeros((5, 3), np.float32)),
        "numpy indices": dict(indices=np.zeros((4, 3), np.uint32)),
        "no positions": dict(positions=None),
        "no indices": dict(indices=None),
        "float64 positions": dict(positions=pos.double()),
        "float16 normals": dict(normals=pos.half()),
        "int64 indices": dict(indices=idx.long()),
        "float indices": dict(indices=idx.float()),
        "float materials": dict(tri_material=tm.float()),
        "flat positions": dict(positions=pos.reshape(-1)),
        "positions [n, 4]": dict(positions=torch.zeros((5, 4), dtype=torch.float32)),
        "texcoords [n, 3]": dict(texcoords=pos),
        "indices [n, 2]": dict(indices=torch.zeros((4, 2), dtype=torch.int32)),
        "materials [n, 1]": dict(tri_material=tm.reshape(-1, 1)),
        "non-contiguous positions": dict(positions=torch.zeros((5, 6), dtype=torch.float32)[:, ::2]),
        "every other index row": dict(indices=torch.zeros((8, 3), dtype=torch.int32)[::2]),
        "non-contiguous texcoords": dict(texcoords=torch.zeros((2, 5), dtype=torch.float32).t()),
        "a normal too few": dict(normals=pos[:-1]),
        "a texcoord too many": dict(texcoords=torch.zeros((6, 2), dtype=torch.float32)),
        "a material too few": dict(tri_material=tm[:-1]),
        "CPU tensors of the right layout": dict(),
    }
    for what, change in bad.items():
        kw = dict(dict(positions=pos, normals=None, texcoords=uv, indices=idx, tri_material=tm), **change)
        with pytest.raises(ValueError, match="whitted_set_scene_device: mesh 0"):
            capi.device_mesh_args(who, 0, **kw)
    for t in (np.zeros((5, 2), np.float32), uv, uv.double(), pos, uv.reshape(-1), torch.zeros((5, 4), dtype=torch.float32)[:, ::2]):
        with pytest.raises(ValueError, match="whitted_set_texcoords_device: uv"):
            capi.device_mesh_tensor("whitted_set_texcoords_device", 0, "uv", t, ("torch.float32",), 2)
