"""rtgo_whitted_refit_instances_device_async on the MI355X: rtgo_whitted_set_instances_device's RTGO_UPDATE_REFIT enqueued on the
context's stream, with its verdict left on the device and asked about later (rtgo_whitted_refit_instances_status).

The twin is the synchronous REFIT on a second context over the same scene: an applied update leaves, span for span of the build digest,
what the twin leaves; a refused one leaves digests, frames and the caller's tensor as they were and names the kind and the instance the
twin's message names.  Every comparison is an equality.

Shapes are the smallest at which each path can go wrong: 4 instances (a top level of one leaf: no records, the commit alone), 5 (the first
records), 61, 257 (two workgroups, the second with one entry), 8192 once (the cap); 64 x 48 frames."""
import ctypes as C
import re

import numpy as np
import pytest

import accel_check as A
import whitted_instances as WI
from test_whitted_instances_device import (bits, depth_fields, device_faults, mixed, on_device, poisoned, refit_case, refusal_scene, same_results, small_meshes,
                                           sorted_walk, span, with_entry)
from test_whitted_rebuild_meshes import same_digests
from test_whitted_update_meshes import E_INVALID, H, W, big, frames, no_violations, same_frames, scene_ctx, world_view

pytestmark = pytest.mark.gpu
PENDING, APPLIED, REFUSED = 0, 1, 2
CLEAN = {"state": APPLIED, "fault": 0, "entry": 0}
# rtgo_update_status.fault -> the words of rtgo_whitted_set_instances_device's message for that kind
WORDING = {1: "names a mesh beyond the meshes array", 2: "names another mesh than it names in the scene", 3: "material offset + material index beyond",
           4: "has a non-finite or singular transform", 5: "places its mesh beyond the float range"}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def capi(torch):
    from raytracingo_amd import capi as m
    m.load()
    if torch.cuda.is_available():
        torch.cuda.init()   # torch's HIP runtime up before this module's first context (the tests hand the library torch tensors)
    return m


def jittered(first, seed=12, scale=0.08):
    """refit_case's mild jitter over any instances: every translation but the first moved a little"""
    rng = np.random.RandomState(seed)
    new = list(first)
    for k in range(1, len(first)):
        tr = np.array(first[k][0], np.float32).reshape(3, 4)
        tr[:, 3] += np.float32(scale * rng.normal(size=3))
        new[k] = (tr, first[k][1], first[k][2])
    return new


def async_case(name):
    """(meshes, the scene's instances, the new ones): the same count and mesh choices"""
    if name == "n = 5":
        first = mixed(5, 3, 11)
        return small_meshes(), first, jittered(first)
    if name == "n = 8192":
        meshes, first = WI.octahedra_scene(8191)
        return meshes, first, jittered(first, scale=0.02)
    return refit_case(name)


def refit_async(ctx, t):
    """the call and the wait: the ticket's status afterwards"""
    ticket = ctx.whitted_refit_instances_device_async(t)
    ctx.sync()
    return ctx.whitted_refit_instances_status(ticket)


def refit_sync(torch, ctx, inst):
    ctx.whitted_set_instances_device(on_device(torch, inst), refit=True)


def same_everything(capi, dev, twin, cam, what):
    same_digests(dev, twin, what)
    same_results(capi, dev, twin, cam, what)
    assert np.array_equal(sorted_walk(dev), sorted_walk(twin)), what + ": the InstWalk records differ"
    assert depth_fields(dev) == depth_fields(twin), what


# ---- 1. it is the twin ----------------------------------------------------------------------------------------------------------
JITTER = ("n = 4", "n = 5", "a mild jitter", "n = 257", "n = 8192")


@pytest.mark.parametrize("name", JITTER[:4] + ("permuted", "material offsets", "n = 8192"))
def test_it_is_the_twin(capi, oracle, torch, name):
    meshes, first, new = async_case(name)
    cam, extra = world_view(oracle, meshes, new)
    dev, twin = (scene_ctx(capi, meshes, first, WI.materials(), cam, extra) for _ in range(2))
    try:
        depths, recs_before, inst_before = depth_fields(dev), span(dev, "top.recs"), span(dev, "top.inst")
        assert (depths[3] == 0) == (len(new) <= 4), "a top level has records from five instances on"
        t = on_device(torch, new, "float32")
        kept = bits(t)
        assert refit_async(dev, t) == CLEAN
        refit_sync(torch, twin, new)
        assert np.array_equal(bits(t), kept), "the caller's tensor changed"
        same_everything(capi, dev, twin, cam, name)
        assert depth_fields(dev) == depths, name + ": a refit moved the depths"
        no_violations(A.check_instanced(dev.read_build(True), meshes, new), name)
        if name in JITTER:
            assert span(dev, "top.inst") != inst_before, name + ": the InstWalk records did not move"
            if len(new) > 4:   # (four instances are one leaf: there are no records to move)
                assert span(dev, "top.recs") != recs_before, name + ": the records did not move"
    finally:
        dev.close()
        twin.close()


# ---- 2. three updates without a wait are one ------------------------------------------------------------------------------------
def test_three_updates_without_a_wait_are_one(capi, oracle, torch):
    meshes, first, a = refit_case("a mild jitter")
    _, _, b = refit_case("permuted")
    c = jittered(b, seed=21)
    cam, extra = world_view(oracle, meshes, c)
    dev, twin = (scene_ctx(capi, meshes, first, WI.materials(), cam, extra) for _ in range(2))
    try:
        ts = [on_device(torch, x) for x in (a, b, c)]
        tickets = [dev.whitted_refit_instances_device_async(t) for t in ts]
        dev.whitted_launch(W, H, 0)
        dev.sync()
        assert tickets == [1, 2, 3]
        assert [dev.whitted_refit_instances_status(k) for k in tickets] == [CLEAN] * 3
        shown = dev.read_accum(H, W)
        refit_sync(torch, twin, c)
        twin.whitted_launch(W, H, 0)
        twin.sync()
        assert np.array_equal(shown.view(np.uint32), twin.read_accum(H, W).view(np.uint32)), "the launch behind the three updates"
        same_everything(capi, dev, twin, cam, "three updates")
    finally:
        dev.close()
        twin.close()


# ---- 3. a fault found on the device changes nothing -----------------------------------------------------------------------------
def twin_says(capi, torch, twin, inst):
    """(fault, entry) as the synchronous call's message names them on the same data"""
    with pytest.raises(capi.RtgoError, match=E_INVALID) as err:
        refit_sync(torch, twin, inst)
    msg = str(err.value)
    kinds = [f for f, words in WORDING.items() if words in msg]
    assert len(kinds) == 1, msg
    return kinds[0], int(re.search(r"instance (\d+)", msg).group(1))


def test_a_fault_found_on_the_device_changes_nothing(capi, oracle, torch):
    meshes, inst, cam, extra = refusal_scene(capi, oracle)
    dev, twin = (scene_ctx(capi, meshes, inst, WI.materials(), cam, extra) for _ in range(2))
    try:
        before, shown = list(dev.build_digest(True)), frames(dev)
        faults = dict(device_faults(inst))
        faults["a changed mesh choice"] = with_entry(inst, 5, mesh=3 - inst[5][1])
        seen = set()
        for what, bad in faults.items():
            t = on_device(torch, bad)
            kept = bits(t)
            ticket = dev.whitted_refit_instances_device_async(t)   # RTGO_OK and a ticket: the binding raises on anything else
            assert ticket >= 1, what
            dev.sync()
            fault, entry = twin_says(capi, torch, twin, bad)
            assert dev.whitted_refit_instances_status(ticket) == {"state": REFUSED, "fault": fault, "entry": entry}, what
            assert list(dev.build_digest(True)) == before, what
            same_frames(frames(dev), shown, what)
            assert np.array_equal(bits(t), kept), what + ": the caller's tensor changed"
            seen.add(fault)
        assert seen == {1, 2, 3, 4, 5}
        same_digests(dev, twin, "after the refusals")
        # a clean update right behind a refused one, no wait between
        new = jittered(inst, seed=22)
        t_bad, t_new = on_device(torch, faults["a NaN in a transform"]), on_device(torch, new)
        refused, applied = dev.whitted_refit_instances_device_async(t_bad), dev.whitted_refit_instances_device_async(t_new)
        dev.sync()
        assert dev.whitted_refit_instances_status(refused) == {"state": REFUSED, "fault": 4, "entry": 4}
        assert dev.whitted_refit_instances_status(applied) == CLEAN
        refit_sync(torch, twin, new)
        same_everything(capi, dev, twin, cam, "a clean update behind a refused one")
    finally:
        dev.close()
        twin.close()


def test_the_lowest_offending_instance_is_named_across_workgroups(capi, oracle, torch):
    meshes, _, _, _ = refusal_scene(capi, oracle)
    inst = mixed(512, 3, 14, spacing=0.3)
    cam, extra = world_view(oracle, meshes, inst)
    dev, twin = (scene_ctx(capi, meshes, inst, WI.materials(), cam, extra) for _ in range(2))
    try:
        before = list(dev.build_digest(True))
        bad = with_entry(with_entry(inst, 300, mesh=9), 40, transform=poisoned(inst[40][0], 0, 0, np.nan))
        assert twin_says(capi, torch, twin, bad) == (4, 40)
        assert refit_async(dev, on_device(torch, bad)) == {"state": REFUSED, "fault": 4, "entry": 40}
        bad = with_entry(with_entry(inst, 300, transform=poisoned(inst[300][0], 0, 0, np.nan)), 40, off=0xFFFFFFFF)
        assert twin_says(capi, torch, twin, bad) == (3, 40)
        assert refit_async(dev, on_device(torch, bad)) == {"state": REFUSED, "fault": 3, "entry": 40}
        assert list(dev.build_digest(True)) == before
    finally:
        dev.close()
        twin.close()


# ---- 4. what the host refuses at once -------------------------------------------------------------------------------------------
def test_what_the_host_refuses_at_once(capi, oracle, torch):
    meshes, inst, cam, extra = refusal_scene(capi, oracle)
    dev = scene_ctx(capi, meshes, inst, WI.materials(), cam, extra)
    none, single = capi.Context(0), capi.Context(0)
    try:
        tor = meshes[1]
        single.whitted_set_mesh(tor["positions"], tor["normals"], tor["indices"], tor["tri_material"], WI.materials())
        t = on_device(torch, inst)
        wide = on_device(torch, mixed(8193, 3, 15))
        n = len(inst)
        first = dev.whitted_refit_instances_device_async(t)
        dev.sync()
        before = list(dev.build_digest(True))
        fn, sync_fn = dev._lib.rtgo_whitted_refit_instances_device_async, dev._lib.rtgo_whitted_set_instances_device
        ticket = C.c_uint64(0xDEAD)
        off_by_one = t[1:].reshape(-1)[1:].data_ptr()
        cases = [("a NULL context", None, t.data_ptr(), n, 1), ("a NULL pointer", dev._h, None, n, 1), ("a pointer one byte off", dev._h, off_by_one, n - 2, 1),
                 ("one instance fewer", dev._h, t.data_ptr(), n - 1, 1), ("one more", dev._h, wide.data_ptr(), n + 1, 1), ("n = 0", dev._h, t.data_ptr(), 0, 4),
                 ("n = 8193", dev._h, wide.data_ptr(), 8193, 4), ("no scene", none._h, t.data_ptr(), n, 3),
                 ("a scene of rtgo_whitted_set_mesh", single._h, t.data_ptr(), n, 3)]
        for what, h, ptr, count, code in cases:
            assert fn(h, ptr, count, C.byref(ticket)) == code, what
            assert sync_fn(h, ptr, count, capi.UPDATE_REFIT) == code, what + ": the twin's code"
            assert ticket.value == 0xDEAD, what + ": the ticket word was written"
        assert fn(dev._h, t.data_ptr(), n, None) == 1, "a NULL ticket"
        for bad in (t.cpu(), t[:, :48], t.reshape(-1), t.to(torch.int16)):
            with pytest.raises(ValueError):
                dev.whitted_refit_instances_device_async(bad)
        assert list(dev.build_digest(True)) == before
        assert dev.whitted_refit_instances_device_async(t) == first + 1, "a refused call took a ticket"
        dev.sync()
        assert list(dev.build_digest(True)) == before   # (the scene's own instances)
    finally:
        for c in (dev, none, single):
            c.close()


# ---- 5. the ring ----------------------------------------------------------------------------------------------------------------
def test_seventy_updates_pass_through_the_ring_of_64(capi, oracle, torch):
    meshes, first, a = refit_case("a mild jitter")
    _, _, b = refit_case("permuted")
    last = jittered(first, seed=23)
    cam, extra = world_view(oracle, meshes, last)
    dev, twin = (scene_ctx(capi, meshes, first, WI.materials(), cam, extra) for _ in range(2))
    try:
        ta, tb, tl = (on_device(torch, x) for x in (a, b, last))
        tickets = [dev.whitted_refit_instances_device_async(tl if k == 69 else (ta, tb)[k % 2]) for k in range(70)]
        dev.sync()
        assert tickets == list(range(1, 71))
        assert all(dev.whitted_refit_instances_status(k) == CLEAN for k in tickets[-64:])
        for gone in (6, 1, 71, 1000, 0):
            with pytest.raises(capi.RtgoError, match=E_INVALID):
                dev.whitted_refit_instances_status(gone)
        refit_sync(torch, twin, last)
        same_everything(capi, dev, twin, cam, "after the 70th array")
    finally:
        dev.close()
        twin.close()


# ---- 6. the other calls work afterwards: the lazy refresh and the mesh table ------------------------------------------------------
def test_the_other_calls_work_afterwards(capi, oracle, torch):
    mesh, tor, octa = big(8320), WI.torus(16, 8), WI.octahedron(0.3)
    meshes = [WI.ground(4.0, -0.5), mesh, tor, octa]
    first = mixed(14, 4, 16, spacing=1.2)
    rng = np.random.RandomState(17)
    new = [(tr if k == 0 else WI.transform(np.asarray(tr)[:, :3] @ WI.rotation(rng), np.asarray(tr)[:, 3] + [0.1, 0.05, -0.1]), m, (off + 1) % 3)
           for k, (tr, m, off) in enumerate(first)]
    again = [(tr, m, (off + 2) % 3) for tr, m, off in new]
    third = jittered(new, seed=24)
    spoiled = with_entry(third, 4, transform=poisoned(third[4][0], 1, 2, np.nan))
    cam, extra = world_view(oracle, meshes, new)
    dev, host = (scene_ctx(capi, meshes, first, WI.materials(), cam, extra) for _ in range(2))

    def refit(c, inst):
        if c is dev:
            assert refit_async(c, on_device(torch, inst)) == CLEAN
        else:
            refit_sync(torch, c, inst)

    try:
        refit(dev, new)
        refit(host, new)
        same_everything(capi, dev, host, cam, "the refit")
        centre = np.float32([0.05, 0.1, -0.05])
        # each mesh-update call lays the instances out again from the host's copy, which the asynchronous call never read back
        steps = [("update_mesh", lambda c: c.whitted_update_mesh(2, tor["positions"] * np.float32(1.2))),
                 ("a refit behind update_mesh", lambda c: refit(c, again)),
                 ("update_meshes, a clustered entry included", lambda c: c.whitted_update_meshes([(1, mesh["positions"] + centre, None), (3, octa["positions"] * np.float32(1.5), None)])),
                 ("a refit behind update_meshes", lambda c: refit(c, new)),
                 ("rebuild_meshes", lambda c: c.whitted_rebuild_meshes([(1, mesh["positions"] * np.float32(1.05), None), (2, tor["positions"], None)])),
                 ("a refit behind rebuild_meshes", lambda c: refit(c, again)),
                 ("set_instances", lambda c: c.whitted_set_instances(again)),
                 ("a refit behind set_instances", lambda c: refit(c, new)),
                 ("a synchronous device refit", lambda c: refit_sync(torch, c, again)),
                 # no set call in between: the meshes' boxes moved under the device's mesh table
                 ("update_meshes that scales a mesh", lambda c: c.whitted_update_meshes([(3, octa["positions"] * np.float32(2.5), None)])),
                 ("a refit behind the scaled mesh", lambda c: refit(c, third)),
                 ("update_mesh behind it", lambda c: c.whitted_update_mesh(2, tor["positions"] * np.float32(0.9)))]
        for what, step in steps:
            step(dev)
            step(host)
            same_digests(dev, host, what)
        # a refused update, then a mesh update: once with nothing applied since the staging was made, once behind an applied one
        for what in ("nothing applied before", "an applied update before"):
            if what == "an applied update before":
                refit(dev, again)
                refit(host, again)
            assert refit_async(dev, on_device(torch, spoiled)) == {"state": REFUSED, "fault": 4, "entry": 4}
            for c in (dev, host):
                c.whitted_update_mesh(2, tor["positions"] * np.float32(1.1))
            same_digests(dev, host, "a refused update, then update_mesh: " + what)
        same_results(capi, dev, host, cam, "after every step")
        moved = [meshes[0], dict(mesh, positions=mesh["positions"] * np.float32(1.05)), dict(tor, positions=tor["positions"] * np.float32(1.1)),
                 dict(octa, positions=octa["positions"] * np.float32(2.5))]
        no_violations(A.check_instanced(dev.read_build(True), moved, again), "after every step")
    finally:
        dev.close()
        host.close()


# ---- 7. a first call on a scene whose instances came from each of the set calls ---------------------------------------------------
@pytest.mark.parametrize("origin", ["set_instances", "a device rebuild", "a fresh set_scene"])
def test_a_first_call_after_each_set_call(capi, oracle, torch, origin):
    meshes, first, new = refit_case("a mild jitter")
    tor = meshes[1]
    cam, extra = world_view(oracle, meshes, new)
    start = first if origin == "a fresh set_scene" else mixed(9, 3, 4)
    dev, twin = (scene_ctx(capi, meshes, start, WI.materials(), cam, extra) for _ in range(2))
    try:
        for c in (dev, twin):
            if origin == "set_instances":
                c.whitted_set_instances(first)
            elif origin == "a device rebuild":
                c.whitted_set_instances_device(on_device(torch, first))
        assert refit_async(dev, on_device(torch, new)) == CLEAN
        refit_sync(torch, twin, new)
        same_everything(capi, dev, twin, cam, origin)
        for c in (dev, twin):
            c.whitted_update_mesh(1, tor["positions"] * np.float32(1.2))
        same_digests(dev, twin, origin + ", then update_mesh")
    finally:
        dev.close()
        twin.close()
