"""rtgo_update_prims_device_async and rtgo_update_prims_status in the C ABI: declared in include/rtgo.h with the signatures of the issue,
listed in capi.SYMBOLS, exported by the library and bound with those signatures; rtgo_update_status is 16 bytes on both sides; the ABI
version has not moved (an addition).  A NULL context is refused by both without a device, and the binding's validator refuses a CPU
tensor before anything reaches the library.  No compute calls: runs on a CPU-only box."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p
CALLS = {"rtgo_update_prims_device_async": (["rtgo_ctx* ctx", "const void* d_indices", "const void* d_prims", "const void* d_aabbs", "uint32_t n_updates",
                                             "const rtgo_aabb* reach", "uint64_t* ticket"], "update_prims_device_async",
                                            lambda m: [VP, VP, VP, VP, C.c_uint32, C.POINTER(m.Aabb), C.POINTER(C.c_uint64)]),
         "rtgo_update_prims_status": (["rtgo_ctx* ctx", "uint64_t ticket", "rtgo_update_status* out"], "update_prims_status",
                                      lambda m: [VP, C.c_uint64, C.POINTER(m.UpdateStatus)])}


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import _build, capi as m
    _build.build_all()
    m.load()
    return m


def header(comments=False):
    text = open(os.path.join(ROOT, "include", "rtgo.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_the_call_is_declared_listed_exported_and_bound(capi, name):
    want, method, argtypes = CALLS[name]
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header())
    assert decl, "not declared in include/rtgo.h"
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == want
    assert name in capi.SYMBOLS
    fn = getattr(capi.load(), name)
    assert fn.argtypes == argtypes(capi) and fn.restype is C.c_int
    assert callable(getattr(capi.Context, method))


def test_the_status_struct_is_16_bytes_with_the_fields_of_the_header(capi):
    body = re.search(r"typedef\s+struct\s+rtgo_update_status\s*\{(.*?)\}\s*rtgo_update_status\s*;", header(), flags=re.S)
    assert body, "rtgo_update_status is not declared"
    fields = re.findall(r"uint32_t\s+(\w+)\s*;", body.group(1))
    assert fields == ["state", "fault", "entry", "reserved"]
    assert [f for f, _ in capi.UpdateStatus._fields_] == fields and all(t is C.c_uint32 for _, t in capi.UpdateStatus._fields_)
    assert C.sizeof(capi.UpdateStatus) == 16
    states = re.search(r"enum\s*\{\s*RTGO_UPDATE_PENDING\s*=\s*0\s*,\s*RTGO_UPDATE_APPLIED\s*=\s*1\s*,\s*RTGO_UPDATE_REFUSED\s*=\s*2\s*\}", header())
    assert states and (capi.UPDATE_PENDING, capi.UPDATE_APPLIED, capi.UPDATE_REFUSED) == (0, 1, 2)


def test_the_header_states_the_contract(capi):
    """what the issue asks the header to say: the first calls may allocate, a scene of rtgo_set_scene stays with the synchronous call, and
    which statistics may differ from the twin's"""
    text = " ".join(header(comments=True).split())
    for phrase in ("first call allocates", "RTGO_E_UNSUPPORTED: a scene of rtgo_set_scene", "rays_culled and the collect_stats == 2 counters may differ",
                   "waits for nothing on the host"):
        assert phrase in text, phrase


def test_abi_version_has_not_moved(capi):
    assert capi.load().rtgo_abi_version() == 6
    assert re.search(r"#define\s+RTGO_ABI_VERSION\s+6\b", header(comments=True))


def test_a_null_context_is_refused_without_a_device(capi):
    L = capi.load()
    ticket, st, box = C.c_uint64(77), capi.UpdateStatus(9, 9, 9, 9), capi.Aabb(0, 0, 0, 1, 1, 1)
    for k in (0, 1):
        for reach in (None, C.byref(box)):
            assert L.rtgo_update_prims_device_async(None, None, None, None, k, reach, C.byref(ticket)) == 1   # RTGO_E_INVALID
    assert ticket.value == 77, "a refused call issued a ticket"
    for t in (0, 1, 1 << 40):
        assert L.rtgo_update_prims_status(None, t, C.byref(st)) == 1
    assert (st.state, st.fault, st.entry, st.reserved) == (9, 9, 9, 9)


def test_the_validator_refuses_a_cpu_tensor():
    """Context.update_prims_device_async checks its tensors with capi.device_prims_args before the library sees a pointer (and, unlike
    the synchronous binding, waits for nothing): a CPU tensor never gets there"""
    import inspect
    import torch
    from raytracingo_amd import capi as m
    good = (torch.zeros(3, dtype=torch.int32), torch.zeros((3, 27), dtype=torch.float32), torch.zeros((3, 6), dtype=torch.float32))
    with pytest.raises(ValueError, match="must lie on device 0"):
        m.device_prims_args("update_prims_device_async", 0, *good)
    ctx = m.Context.__new__(m.Context)   # no rtgo_create: the validator runs first and needs no device
    ctx.device, ctx._h, ctx._lib = 0, None, None
    with pytest.raises(ValueError, match="update_prims_device_async: indices must lie on device 0"):
        ctx.update_prims_device_async(*good)
    source = inspect.getsource(m.Context.update_prims_device_async)
    assert "device_prims_args" in source and "hipDeviceSynchronize" not in source and "_device_args" not in source
