"""rtgo_set_scene_device, rtgo_set_large_scene_device and rtgo_update_prims_device in the C ABI: declared in include/rtgo.h with the
header's signatures, listed in capi.SYMBOLS, exported by the library and bound with those signatures; the ABI version has not moved (an
addition).  And the two pieces of the binding that need no device: capi.prims_tensor packs the records Context.set_large_scene packs,
and the tensor validator refuses what the calls cannot take.  No compute calls: runs on a CPU-only box."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET_ARGS = ["rtgo_ctx* ctx", "const void* d_prims", "const void* d_aabbs", "uint32_t n"]
CALLS = {"rtgo_set_scene_device": (SET_ARGS, "set_scene_device"),
         "rtgo_set_large_scene_device": (SET_ARGS, "set_large_scene_device"),
         "rtgo_update_prims_device": (["rtgo_ctx* ctx", "const void* d_indices", "const void* d_prims", "const void* d_aabbs", "uint32_t n_updates",
                                       "uint32_t flags"], "update_prims_device")}


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import _build, capi as m
    _build.build_all()
    m.load()
    return m


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


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
    n_pointers = sum("*" in a for a in want)   # the context and the device pointers, then the counts and flags
    assert fn.argtypes == [C.c_void_p] * n_pointers + [C.c_uint32] * (len(want) - n_pointers) and fn.restype is C.c_int
    assert callable(getattr(capi.Context, method))


def test_abi_version_has_not_moved(capi):
    assert capi.load().rtgo_abi_version() == 6
    assert re.search(r"#define\s+RTGO_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "rtgo.h")).read())


def test_a_null_context_is_refused_without_a_device(capi):
    L = capi.load()
    assert L.rtgo_set_scene_device(None, None, None, 1) == 1   # RTGO_E_INVALID
    assert L.rtgo_set_large_scene_device(None, None, None, 1) == 1
    for flags in (capi.UPDATE_REFIT, capi.UPDATE_REBUILD, 2):
        assert L.rtgo_update_prims_device(None, None, None, None, 0, flags) == 1


def arrays(k):
    """k primitives with every type among them (k >= 4), no two values of a record alike"""
    rng = np.random.default_rng(40 + k)
    types = (np.arange(k) % 4)[::-1].astype(np.uint32) if k >= 4 else np.array([3, 0, 2][:k], np.uint32)
    return types, rng.normal(size=(k, 16)).astype(np.float32), rng.uniform(size=(k, 10)).astype(np.float32)


@pytest.mark.parametrize("k", [1, 3, 4])
def test_prims_tensor_packs_the_records_of_set_large_scene(capi, torch, k):
    """k = 1 and k = 3 (types 3; 3, 0, 2) and k = 4 (all four types): byte for byte what Context.set_large_scene packs"""
    types, models, mat = arrays(k)
    rec = np.zeros(k, dtype=capi.PRIM_DTYPE)   # Context.set_large_scene's packing
    rec["type"], rec["model"] = types, models
    rec["kd"], rec["kr"], rec["specularity"], rec["Le"] = mat[:, 0:3], mat[:, 3:6], mat[:, 6], mat[:, 7:10]
    t = capi.prims_tensor(torch.from_numpy(types.astype(np.int64)), torch.from_numpy(models), torch.from_numpy(mat))
    assert t.dtype == torch.float32 and tuple(t.shape) == (k, 27) and t.is_contiguous()
    assert t.numpy().tobytes() == rec.tobytes()
    # int32 types and a [k, 4, 4] matrix stack are taken alike
    t2 = capi.prims_tensor(torch.from_numpy(types.astype(np.int32)), torch.from_numpy(models.reshape(k, 4, 4)), torch.from_numpy(mat))
    assert t2.numpy().tobytes() == rec.tobytes()


def test_all_four_types_at_k_3_and_1(capi, torch):
    """the issue's cases: k = 1 and k = 3, each over all four types in turn"""
    for k in (1, 3):
        _, models, mat = arrays(k)
        for first in range(4):
            types = ((np.arange(k) + first) % 4).astype(np.uint32)
            rec = np.zeros(k, dtype=capi.PRIM_DTYPE)
            rec["type"], rec["model"] = types, models
            rec["kd"], rec["kr"], rec["specularity"], rec["Le"] = mat[:, 0:3], mat[:, 3:6], mat[:, 6], mat[:, 7:10]
            t = capi.prims_tensor(torch.from_numpy(types.astype(np.int32)), torch.from_numpy(models), torch.from_numpy(mat))
            assert t.numpy().tobytes() == rec.tobytes(), (k, first)


def test_the_validator_refuses_what_the_calls_cannot_take(capi, torch):
    check = lambda *a: capi.device_prims_args("test", 0, *a)
    good = torch.zeros((3, 27), dtype=torch.float32)
    with pytest.raises(ValueError, match="must lie on device 0"):   # a CPU tensor, right in every other way
        check(None, good, None)
    with pytest.raises(ValueError, match="must lie on device 0"):
        check(torch.zeros(3, dtype=torch.int32), good.view(torch.int32), torch.zeros((3, 6), dtype=torch.float32))
    for wrong in (torch.zeros((3, 107), dtype=torch.uint8), torch.zeros((3, 26), dtype=torch.float32), torch.zeros(81, dtype=torch.float32),
                  torch.zeros((3, 27), dtype=torch.float64)):   # a wrong byte count or layout
        with pytest.raises(ValueError, match="108 bytes per record"):
            check(None, wrong, None)
    with pytest.raises(ValueError, match="for 2 indices"):          # 3 records for 2 indices
        check(torch.zeros(2, dtype=torch.int32), good, None)
    with pytest.raises(ValueError, match="boxes"):                  # 2 boxes for 3 records
        check(None, good, torch.zeros((2, 6), dtype=torch.float32))
    with pytest.raises(ValueError, match="int32"):
        check(torch.zeros(3, dtype=torch.int64), good, None)
    for name, args in (("prims", (None, torch.zeros((27, 3), dtype=torch.float32).t(), None)),   # non-contiguous tensors
                       ("indices", (torch.zeros(6, dtype=torch.int32)[::2], good, None)),
                       ("aabbs", (None, good, torch.zeros((3, 12), dtype=torch.float32)[:, ::2]))):
        with pytest.raises(ValueError, match=name + " must be contiguous"):
            check(*args)
    with pytest.raises(ValueError, match="torch tensor"):
        check(None, np.zeros((3, 27), np.float32), None)
