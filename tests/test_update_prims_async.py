"""rtgo_update_prims_device_async and rtgo_update_prims_status on the MI355X: the refit of a scene of rtgo_set_large_scene from device
buffers that waits for nothing on the host.

An applied update is held to its synchronous twin, rtgo_update_prims_device with RTGO_UPDATE_REFIT, array for array and bit for bit; a
refused one -- its verdict is read by the kernels that would write the scene, not by the host -- to the scene as it was; several in a
row without a wait to one set call.  The sizes are those of tests/test_prims_device.py, for the same workgroup of 256 entries, which the
new update kernel stages in LDS as the check does: 1 (no internal node), 2 (one), 3 (the first chain), 257 (one entry in a second
workgroup's tail), 513 (a third workgroup).  No test hands the library a pointer that is not what it claims to be."""
import ctypes as C
import re

import numpy as np
import pytest

import shade_rays_ref as R
import shading_scenes as SC
import test_large_scenes as TL
import test_prims_device as TP
import test_update_prims as TU

pytestmark = pytest.mark.gpu

RTGO_OK, RTGO_E_INVALID, RTGO_E_STATE, RTGO_E_UNSUPPORTED = 0, 1, 3, 4
PENDING, APPLIED, REFUSED = 0, 1, 2
W, H = TU.LW, TU.LH   # 48 x 36
SIZES = TP.SIZES      # 1, 2, 3, 257, 513
NO_TICKET = 0xABCDEF  # what a ticket holds before a call
# rtgo_update_prims_device's message for each fault of rtgo_update_status (the seventh is the asynchronous call's alone)
MESSAGE = {1: "unknown primitive type", 2: "not finite", 3: "singular model matrix", 4: "box that is empty or not finite",
           5: "index beyond the scene", 6: "another entry names"}


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


def boxes_of(oracle, t, idx=None):
    """the boxes of primitives idx (None: all) of tables t: the caller's, or the CubeBox rule's"""
    sel = slice(None) if idx is None else np.asarray(idx)
    return t["aabb"][sel] if t.get("aabb") is not None else TL.oracle_boxes(oracle, t["M"][sel])


def union(*boxes):
    b = np.concatenate([np.asarray(x, np.float32).reshape(-1, 6) for x in boxes])
    return np.concatenate([b[:, :3].min(axis=0), b[:, 3:].max(axis=0)]).astype(np.float32)


def raw(capi, ctx, idx, prims, aabbs, k, reach=None, offset=(0, 0, 0), with_ticket=True):
    """the bare C call on tensors (or None): (code, ticket); offset: bytes added to the three pointers"""
    p = lambda t, o: C.c_void_p(None if t is None else t.data_ptr() + o)
    box = None if reach is None else capi.Aabb(*[float(x) for x in reach])
    ticket = C.c_uint64(NO_TICKET)
    rc = capi.load().rtgo_update_prims_device_async(ctx._h, p(idx, offset[0]), p(prims, offset[1]), p(aabbs, offset[2]), k,
                                                    None if box is None else C.byref(box), C.byref(ticket) if with_ticket else None)
    return rc, ticket.value


def raw_status(capi, ctx, ticket):
    st = capi.UpdateStatus(9, 9, 9, 9)
    return capi.load().rtgo_update_prims_status(ctx._h, ticket, C.byref(st)), (st.state, st.fault, st.entry)


def frame_of(capi, ctx, f=None):
    ctx.launch(f or capi.make_frame(W, H, 1, 0, True, False))
    ctx.sync()
    return ctx.read_accum(H, W).copy()


def state_of(capi, ctx):
    """what a refused update must leave: rtgo_read_bvh's four arrays, the build digests and a frame"""
    return [TU.bits(a).copy() for a in ctx.read_bvh()] + [ctx.build_digest(False), TU.bits(frame_of(capi, ctx)).copy()]


def same_state(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def same_as_fresh(capi, ctx, fresh, t_new, what):
    """ctx, refitted, against a context set with the edited array: records and boxes, a tree that closes over them under the fresh root
    box, and the answers (the refitted tree keeps its depth)"""
    boxes, links, inv, aabb = ctx.read_bvh()
    fboxes, _, finv, faabb = fresh.read_bvh()
    assert np.array_equal(TU.bits(inv), TU.bits(finv)) and np.array_equal(TU.bits(aabb), TU.bits(faabb)), what + ": records or boxes"
    assert not TU.closure_violations(boxes, links, aabb), what
    assert np.array_equal(TU.bits(boxes[0]), TU.bits(fboxes[0])), what + ": root box"
    got, want = TU.answers(capi, ctx, t_new, W, H, frames=(0,)), TU.answers(capi, fresh, t_new, W, H, frames=(0,))
    got["scene stats"] = (got["scene stats"][0], want["scene stats"][1]) + got["scene stats"][2:]
    TU.assert_same_answers(got, want, what)


# ---- 1. an applied update is the twin's -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_aabbs", [True, False], ids=["boxes", "cube"])
@pytest.mark.parametrize("n", SIZES)
def test_it_is_the_twin(capi, torch, oracle, n, with_aabbs):
    t = TP.scene(oracle, ("large", n, with_aabbs))
    d, h = capi.Context(0), capi.Context(0)
    for what, idx in (("the first", [0]), ("the last", [n - 1]), ("all, reversed", np.arange(n)[::-1])):
        for ctx in (d, h):
            TU.set_scene(ctx, t, True, W * H)
            ctx.launch(capi.make_frame(W, H, 1, 0, True, False))   # (a mask and seeds over the old bounds)
        _, links0, _, _ = d.read_bvh()
        depth0 = d.stats()["lbvh_depth"]
        t_new = TU.large_edit(oracle, t, idx, 7 * n + len(idx))
        label = "n %d, %s" % (n, what)
        ts = TP.tensors(torch, capi, t_new, idx)
        before = TP.words(torch, ts)
        ticket = d.update_prims_device_async(*ts, reach=union(boxes_of(oracle, t), boxes_of(oracle, t_new, idx)))
        h.update_prims_device(*ts)
        d.sync()
        assert d.update_prims_status(ticket) == {"state": APPLIED, "fault": 0, "entry": 0}, label
        TP.unchanged(torch, ts, before, label)
        TP.same_bvh(d, h, label)
        boxes, links, _, aabb = d.read_bvh()
        assert np.array_equal(links, links0), label + ": the topology moved"
        assert not TU.closure_violations(boxes, links, aabb), label
        assert d.stats()["lbvh_depth"] == h.stats()["lbvh_depth"] == depth0
        TU.assert_same_answers(TU.answers(capi, d, t_new, W, H, frames=(0,)), TU.answers(capi, h, t_new, W, H, frames=(0,)), label)
    d.close()
    h.close()


# ---- 2. nothing moved: no node is written -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_aabbs", [True, False], ids=["boxes", "cube"])
def test_a_material_only_edit_leaves_the_nodes(capi, torch, oracle, with_aabbs):
    """(reach NULL: the bounds the context holds, which the unmoved boxes touch from inside)"""
    t = TP.scene(oracle, ("large", 257, with_aabbs))
    ctx = TU.set_scene(capi.Context(0), t, True, W * H)
    before = ctx.read_build(False)
    idx = np.array([0, 100, 256])
    t_new = TU.edit(oracle, t, idx, mat=t["mat"][idx][:, ::-1].copy())
    ts = TP.tensors(torch, capi, t_new, idx)
    ticket = ctx.update_prims_device_async(*ts)
    ctx.sync()
    assert ctx.update_prims_status(ticket)["state"] == APPLIED
    after = ctx.read_build(False)
    assert np.array_equal(TU.bits(before["nodes"]), TU.bits(after["nodes"])) and np.array_equal(TU.bits(before["aabb"]), TU.bits(after["aabb"]))
    assert not np.array_equal(TU.bits(before["prims"]), TU.bits(after["prims"]))
    fresh = TU.set_scene(capi.Context(0), t_new, True, W * H)
    TU.same_digests(ctx, fresh, "material-only edit")   # (nothing moved: the refit is the fresh build)
    ctx.close()
    fresh.close()


# ---- 3. several in a row, no wait between them ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_aabbs", [True, False], ids=["boxes", "cube"])
def test_three_updates_without_a_wait_are_one_set_call(capi, torch, oracle, with_aabbs):
    t = TP.scene(oracle, ("large", 513, with_aabbs))
    steps = [np.array([0, 512]), np.arange(100, 300), np.array([512, 7, 150])]   # (overlapping: the later edit stands)
    stages, t_new = [], t
    for k, idx in enumerate(steps):
        t_new = TU.large_edit(oracle, t_new, idx, 40 + k)
        stages.append((t_new, TP.tensors(torch, capi, t_new, idx)))
    reach = union(boxes_of(oracle, t), *[boxes_of(oracle, s, idx) for (s, _), idx in zip(stages, steps)])
    ctx = TU.set_scene(capi.Context(0), t, True, W * H)
    tickets = [ctx.update_prims_device_async(*ts, reach=reach) for _, ts in stages]
    ctx.sync()
    assert tickets == [1, 2, 3] and [ctx.update_prims_status(k)["state"] for k in tickets] == [APPLIED] * 3
    fresh = TU.set_scene(capi.Context(0), t_new, True, W * H)
    same_as_fresh(capi, ctx, fresh, t_new, "three updates in a row")
    ctx.close()
    fresh.close()


# ---- 4. refusals that are decided on the device ---------------------------------------------------------------------------------------------
def spoil(idx, rec, box, fault, j):
    """the good update with entry j given `fault`; for fault 6 also the other entry that then names the index: (idx, rec, box, entries)"""
    idx, rec, box = idx.copy(), rec.copy(), None if box is None else box.copy()
    entries = (j,)
    if fault == 1:
        rec["type"][j] = 4
    elif fault == 2:
        rec["model"][j][5] = np.nan          # (the determinant is then no number either: the lower kind is the one to name)
    elif fault == 3:
        rec["model"][j].reshape(4, 4)[:3, 1] = 0.0
    elif fault == 4:
        box[j, 4] = box[j, 1] - 1.0
    elif fault == 5:
        idx[j] = len(idx) if j else 0xFFFFFFFF
    elif fault == 6:
        other = (j + 7) % len(idx)
        idx[j] = idx[other]
        entries = (j, other)
    else:                                    # a good record and a good box, 100 units beyond the reach
        rec["model"][j][3] += 100.0
        if box is not None:
            box[j, [0, 3]] += 100.0
    return idx, rec, box, entries


def visible_edit(oracle, t, radius):
    """primitive 3 becomes a sphere in the middle of the view"""
    return TU.edit(oracle, t, [3], types=[SC.SPHERE], M=[SC.model((0.0, 0.0, 2.0), np.eye(3), radius)])


class Refusals:
    """A scene of 513 primitives on three contexts: d takes the asynchronous calls, h the synchronous twin's refusals (it never changes),
    g only the good updates, through the twin.  The update under test names every primitive, in reversed order."""

    def __init__(self, capi, torch, oracle, with_aabbs):
        self.capi, self.torch = capi, torch
        self.t = t = TP.scene(oracle, ("large", 513, with_aabbs))
        self.k = n = len(t["type"])
        self.d, self.h, self.g = (TU.set_scene(capi.Context(0), t, True, W * H) for _ in range(3))
        order = np.arange(n)[::-1].copy()
        t_new = TU.large_edit(oracle, t, order, 77)
        self.idx, self.rec = order.astype(np.uint32), TU.records(capi, t_new, order)
        self.box = np.ascontiguousarray(t_new["aabb"][order], np.float32) if with_aabbs else None
        self.goods = [(e, TP.tensors(torch, capi, e, [3])) for e in (visible_edit(oracle, t, 0.9), visible_edit(oracle, t, 0.5))]
        self.reach = union(boxes_of(oracle, t), boxes_of(oracle, t_new), *[boxes_of(oracle, e, [3]) for e, _ in self.goods])
        self.turn = 0

    def check(self, what, idx, rec, box, fault, entries):
        capi, torch, d, g = self.capi, self.torch, self.d, self.g
        ts = TP.upload(torch, idx, rec, box)
        words = TP.words(torch, ts)
        before = state_of(capi, d)
        # alone: the call returns a ticket, the verdict comes later, nothing changes
        rc, ticket = raw(capi, d, *ts, self.k, self.reach)
        assert rc == RTGO_OK and ticket != NO_TICKET, what
        d.sync()
        st = d.update_prims_status(ticket)
        assert st["state"] == REFUSED and st["fault"] == fault and st["entry"] in entries, "%s: %r" % (what, st)
        if fault != 7:   # what the synchronous call says of the same data
            assert TP.raw(capi, self.h, *ts, self.k) == RTGO_E_INVALID, what
            msg = TP.last_error(capi, self.h)
            named = int(re.search(r"entry (\d+)", msg).group(1))
            assert MESSAGE[fault] in msg and named in entries and (fault == 6 or named == st["entry"]), "%s: %r against %r" % (what, st, msg)
        assert same_state(state_of(capi, d), before), what + ": a refused update changed the scene"
        # again, with a good update right behind it and no wait in between: judged by its own verdict alone
        _, good = self.goods[self.turn % 2]
        self.turn += 1
        rc, ticket = raw(capi, d, *ts, self.k, self.reach)
        applied = d.update_prims_device_async(*good, reach=self.reach)
        assert rc == RTGO_OK and applied == ticket + 1
        g.update_prims_device(*good)
        d.sync()
        assert d.update_prims_status(ticket)["state"] == REFUSED and d.update_prims_status(applied) == {"state": APPLIED, "fault": 0, "entry": 0}, what
        after = state_of(capi, d)
        assert same_state(after, state_of(capi, g)), what + ": not the scene the good update alone leaves"
        assert not np.array_equal(after[-1], before[-1]), what + ": the good update does not show in the frame"
        TP.unchanged(torch, ts, words, what)

    def close(self):
        for ctx in (self.d, self.h, self.g):
            ctx.close()


# (under the CubeBox rule no boxes are given: there is none to spoil)
@pytest.mark.parametrize("fault,with_aabbs", [(f, b) for f in range(1, 8) for b in (True, False) if b or f != 4],
                         ids=lambda v: {True: "boxes", False: "cube"}.get(v, str(v)) if isinstance(v, bool) else "fault %d" % v)
def test_a_fault_found_on_the_device_changes_nothing(capi, torch, oracle, fault, with_aabbs):
    """one entry spoiled: the first, entry 256 (the first of the second workgroup) and the last of 513"""
    s = Refusals(capi, torch, oracle, with_aabbs)
    for j in (0, 256, s.k - 1):
        idx, rec, box, entries = spoil(s.idx, s.rec, s.box, fault, j)
        s.check("fault %d at entry %d" % (fault, j), idx, rec, box, fault, entries)
    s.close()


@pytest.mark.parametrize("with_aabbs", [True, False], ids=["boxes", "cube"])
def test_the_lowest_entry_is_named(capi, torch, oracle, with_aabbs):
    """two entries with faults of different kinds: the lower entry's, whichever kind has the lower number"""
    s = Refusals(capi, torch, oracle, with_aabbs)
    for (fa, ja), (fb, jb) in (((1, 300), (2, 100)), ((2, 400), (7, 20)), ((7, 511), (5, 257))):
        idx, rec, box, _ = spoil(s.idx, s.rec, s.box, fa, ja)
        idx, rec, box, _ = spoil(idx, rec, box, fb, jb)
        lowest = (fa, ja) if ja < jb else (fb, jb)
        if lowest[0] == 7:   # (the twin knows no reach: it would name the other entry)
            ts = TP.upload(torch, idx, rec, box)
            rc, ticket = raw(capi, s.d, *ts, s.k, s.reach)
            s.d.sync()
            assert rc == RTGO_OK and s.d.update_prims_status(ticket) == {"state": REFUSED, "fault": 7, "entry": lowest[1]}
        else:
            s.check("faults %d and %d" % (fa, fb), idx, rec, box, lowest[0], (lowest[1],))
    s.close()


# ---- 5. refusals the host decides at once ----------------------------------------------------------------------------------------------------
def test_what_the_host_refuses_at_once(capi, torch, oracle):
    t = TP.scene(oracle, ("large", 257, True))
    n = len(t["type"])
    d = TU.set_scene(capi.Context(0), t, True, W * H)
    before, stats = state_of(capi, d), d.stats()
    order = np.arange(n)[::-1].copy()
    t_new = TU.large_edit(oracle, t, order, 78)
    g_idx, g_rec, g_box = order.astype(np.uint32), TU.records(capi, t_new, order), np.ascontiguousarray(t_new["aabb"][order], np.float32)
    good = TP.upload(torch, g_idx, g_rec, g_box)
    more = TP.upload(torch, np.append(g_idx, 0).astype(np.uint32), np.append(g_rec, g_rec[:1]), np.concatenate([g_box, g_box[:1]]))
    reach = union(t["aabb"], t_new["aabb"])
    words = TP.words(torch, good)

    def refused(what, ts, k, code, **kw):
        rc, ticket = raw(capi, d, ts[0], ts[1], ts[2], k, kw.pop("reach", reach), **kw)
        assert rc == code and ticket == NO_TICKET, "%s: code %d, ticket %#x" % (what, rc, ticket)
        assert TP.last_error(capi, d), what

    refused("NULL indices", (None, good[1], good[2]), n, RTGO_E_INVALID)
    refused("NULL prims", (good[0], None, good[2]), n, RTGO_E_INVALID)
    refused("NULL ticket", good, n, RTGO_E_INVALID, with_ticket=False)
    for which in range(3):   # (the call refuses the pointer before any dereference: the tensors are good, the address is not used)
        refused("a pointer one byte off", good, n, RTGO_E_INVALID, offset=tuple(1 if q == which else 0 for q in range(3)))
    refused("no boxes for a scene set with boxes", (good[0], good[1], None), n, RTGO_E_INVALID)
    refused("n_updates = n + 1", more, n + 1, RTGO_E_INVALID)
    for what, j, v in (("a NaN", 4, np.nan), ("+Inf", 5, np.inf), ("-Inf", 0, -np.inf), ("min above max", 1, reach[4] + 1.0)):
        r = reach.copy()
        r[j] = v
        refused("reach with " + what, good, n, RTGO_E_INVALID, reach=r)
    assert raw(capi, d, None, None, None, 0, reach) == (RTGO_OK, 0)   # no updates: nothing is enqueued, the ticket of nothing
    assert raw(capi, d, good[0], good[1], good[2], 0, None) == (RTGO_OK, 0)
    assert raw_status(capi, d, 0) == (RTGO_OK, (APPLIED, 0, 0))
    assert raw_status(capi, d, 1)[0] == RTGO_E_INVALID, "no ticket was issued yet"
    assert same_state(state_of(capi, d), before) and d.stats()["lbvh_depth"] == stats["lbvh_depth"]
    TP.unchanged(torch, good, words, "the refused calls")
    # and the call as given is good
    rc, ticket = raw(capi, d, good[0], good[1], good[2], n, reach)
    d.sync()
    assert (rc, ticket) == (RTGO_OK, 1) and raw_status(capi, d, 1) == (RTGO_OK, (APPLIED, 0, 0))
    assert not same_state(state_of(capi, d), before)
    d.close()


def test_boxes_for_a_scene_set_without_are_refused(capi, torch, oracle):
    t = TP.scene(oracle, ("large", 257, False))
    d = TU.set_scene(capi.Context(0), t, True, W * H)
    before = state_of(capi, d)
    idx, prims, _ = TP.tensors(torch, capi, t, [3, 256])
    boxes = TP.dev(torch, np.array([[0, 0, 0, 1, 1, 1]] * 2), np.float32)
    torch.cuda.synchronize()
    assert raw(capi, d, idx, prims, boxes, 2) == (RTGO_E_INVALID, NO_TICKET) and "without boxes" in TP.last_error(capi, d)
    assert same_state(state_of(capi, d), before)
    d.close()


def test_no_scene_and_a_scene_of_set_scene(capi, torch, oracle):
    t3 = TP.scene(oracle, ("large", 3, False))
    idx, prims, _ = TP.tensors(torch, capi, t3, [0])
    d = capi.Context(0)
    assert raw(capi, d, idx, prims, None, 1) == (RTGO_E_STATE, NO_TICKET)
    assert raw(capi, d, None, None, None, 0) == (RTGO_E_STATE, NO_TICKET)
    d.close()
    t, w, h = TU.tables(oracle, "cornell")   # the update of a scene of rtgo_set_scene is a build with host readers: the synchronous call's
    d = TU.set_scene(capi.Context(0), t, False, w * h)
    digests = d.build_digest(False)
    ts = TP.tensors(torch, capi, t, [6, 7])
    for k in (2, 0):
        assert raw(capi, d, *ts, k) == (RTGO_E_UNSUPPORTED, NO_TICKET)
    assert "rtgo_set_scene" in TP.last_error(capi, d) and d.build_digest(False) == digests
    d.close()


# ---- 6. reach ---------------------------------------------------------------------------------------------------------------------------------
def test_reach_is_what_lets_a_primitive_leave_the_old_bounds(capi, torch, oracle):
    """tests/test_update_prims.py's test_a_primitive_moved_outside_the_old_bounds_shows: the screen rectangle follows `reach`, since no
    root box is read back; without one the move is refused"""
    t = TU.compact_scene(oracle)
    f0 = capi.make_frame(W, H, 1, 0, True, False, bands=(1, 1, 0))
    ctx = TU.set_scene(capi.Context(0), t, True, W * H)
    ctx.reset_stats()
    old = frame_of(capi, ctx, f0)
    assert ctx.stats()["rays_culled"] > 0, "the old screen rectangle culls nothing: the case shows nothing"
    o, d, _ = R.raygen32(t["cam"], W, H, 0)
    rays = capi.make_rays(o, d, TU.TMIN, TU.TMAX)
    before = ctx.trace_rays(rays)["prim"].reshape(H, W)
    t_new = TU.edit(oracle, t, [0], M=[SC.model((3.0, 4.0, 0.0), np.eye(3), 0.7)])
    ts = TP.tensors(torch, capi, t_new, [0])
    # no reach: the bounds the context holds, which the new place lies outside of
    ticket = ctx.update_prims_device_async(*ts)
    ctx.launch(f0)
    ctx.sync()
    assert ctx.update_prims_status(ticket) == {"state": REFUSED, "fault": 7, "entry": 0}
    assert np.array_equal(TU.bits(ctx.read_accum(H, W)), TU.bits(old)), "a refused move shows"
    # a reach that covers it
    ticket = ctx.update_prims_device_async(*ts, reach=union(boxes_of(oracle, t), boxes_of(oracle, t_new, [0])))
    ctx.launch(f0)
    ctx.sync()
    assert ctx.update_prims_status(ticket)["state"] == APPLIED
    acc = ctx.read_accum(H, W).copy()
    fresh = TU.set_scene(capi.Context(0), t_new, True, W * H)
    assert np.array_equal(TU.bits(acc), TU.bits(frame_of(capi, fresh, f0)))
    after = ctx.trace_rays(rays)["prim"].reshape(H, W)
    cols, rows = np.flatnonzero((before >= 0).any(axis=0)), np.flatnonzero((before >= 0).any(axis=1))
    y, x = np.mgrid[0:H, 0:W]
    new = (after == 0) & ((x > cols.max() + 3) | (y > rows.max() + 3))   # beyond the old rectangle and its pad
    assert new.sum() > 10, "the moved sphere does not reach beyond the old rectangle"
    bg = np.broadcast_to(t["bg"], (H, W, 3))
    assert (acc[new][:, :3] != bg[new]).any(axis=1).all(), "pixels of the moved sphere were answered as background"
    ctx.close()
    fresh.close()


# ---- 7. the ring ------------------------------------------------------------------------------------------------------------------------------
def test_seventy_updates_pass_through_the_ring_of_64(capi, torch, oracle):
    """70 updates of one primitive each with no wait in between (the 65th may wait for the first: that is the contract)"""
    t = TP.scene(oracle, ("large", 3, True))
    count = 70
    types, M, mat = TL.random_scene(count, 9, spread=3.0)
    pads = TU.box_pad(count, 10)
    stages, t_new = [], t
    for j in range(count):
        t_new = TU.edit(oracle, t_new, [j % 3], types=types[j:j + 1], M=M[j:j + 1], mat=mat[j:j + 1], pad=pads[j:j + 1])
        stages.append(TP.tensors(torch, capi, t_new, [j % 3]))
    reach = union(t["aabb"], TL.oracle_boxes(oracle, M) + pads)
    ctx = TU.set_scene(capi.Context(0), t, True, W * H)
    tickets = [ctx.update_prims_device_async(*ts, reach=reach) for ts in stages]
    ctx.sync()
    assert tickets == list(range(1, count + 1))
    assert all(raw_status(capi, ctx, k) == (RTGO_OK, (APPLIED, 0, 0)) for k in tickets[-64:]), "the last 64 tickets"
    for gone in (tickets[0], tickets[-65], tickets[-1] + 1, tickets[-1] + 1000):
        assert raw_status(capi, ctx, gone)[0] == RTGO_E_INVALID, gone
    fresh = TU.set_scene(capi.Context(0), t_new, True, W * H)
    same_as_fresh(capi, ctx, fresh, t_new, "70 updates")
    ctx.close()
    fresh.close()
