"""rtgo_set_scene_device, rtgo_set_large_scene_device and rtgo_update_prims_device on the MI355X: analytic scenes set and edited from
records, boxes and indices that are on the device already (torch tensors).

One claim: after an accepted call the context holds, array for array, what its host-pointer twin holds after the same data.  So every
comparison here is an equality between two contexts, one driven through the twin: the build digests span for span, rtgo_read_bvh's four
arrays bit for bit (the refitted nodes too: both start from the same build and the refit is deterministic), and the answers of
tests/test_update_prims.py -- frames in the three modes, collect_stats launches, ray queries, ray counts.  A refused call leaves digests,
a frame, every field of rtgo_stats and the caller's tensors as they were, and rtgo_last_error names the offending entry.

The sizes are chosen for the check kernel's workgroup of 256 entries: 1, 2, 3; 257 (a tail of one entry in a second workgroup); 513 (three
workgroups).  No test hands the library a pointer that is not what it claims to be."""
import ctypes as C
import re

import numpy as np
import pytest

import shading_scenes as SC
import test_large_scenes as TL
import test_update_prims as TU

pytestmark = pytest.mark.gpu

RTGO_OK, RTGO_E_INVALID, RTGO_E_STATE, RTGO_E_UNSUPPORTED = 0, 1, 3, 4
W, H = TU.LW, TU.LH   # 48 x 36
SIZES = [1, 2, 3, 257, 513]


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


_scenes = {}


def scene(oracle, key):
    """the scenes of this file, made once: ("large", n, with_aabbs) of tests/test_update_prims.py, "cornell" (the reference's boxes) and
    "quadrics" (set without boxes), all seen through 48 x 36 frames"""
    if key not in _scenes:
        if key == "cornell":
            _scenes[key] = oracle.scene_tables(oracle.scene("cornell", W, H))
        elif key == "quadrics":
            _scenes[key] = SC.SCENES["quadrics"](W / H)
        else:
            _, n, with_aabbs = key
            _scenes[key] = TU.large_scene(oracle, n, 100 + n, with_aabbs)
    return _scenes[key]


def dev(torch, a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def tensors(torch, capi, t, idx=None):
    """(indices or None, prims, aabbs or None) on the device for the primitives idx of tables t (None: all, no indices), their uploads
    complete; the records packed there by capi.prims_tensor"""
    sel = slice(None) if idx is None else np.asarray(idx)
    prims = capi.prims_tensor(dev(torch, t["type"][sel], np.int32), dev(torch, t["M"][sel], np.float32), dev(torch, t["mat"][sel], np.float32))
    out = (None if idx is None else dev(torch, np.ascontiguousarray(idx, np.uint32).view(np.int32), np.int32), prims,
           None if t.get("aabb") is None else dev(torch, t["aabb"][sel], np.float32))
    torch.cuda.synchronize()
    return out


def words(torch, ts):
    """the tensors' bits, on the host"""
    return [None if t is None else t.contiguous().view(torch.int32).cpu().numpy().copy() for t in ts]


def unchanged(torch, ts, before, what):
    for t, b in zip(words(torch, ts), before):
        assert (t is None and b is None) or np.array_equal(t, b), what + ": a tensor of the caller's was written"


def same_bvh(a, b, what):
    for name, x, y in zip(("boxes", "links", "inverses", "aabbs"), a.read_bvh(), b.read_bvh()):
        assert np.array_equal(TU.bits(x), TU.bits(y)), "%s: rtgo_read_bvh's %s differ" % (what, name)


def same_context(capi, a, b, t, what, frames=(0,)):
    """a and b hold scene t alike: digests, rtgo_read_bvh, and what they answer"""
    TU.same_digests(a, b, what)
    same_bvh(a, b, what)
    TU.assert_same_answers(TU.answers(capi, a, t, W, H, frames=frames), TU.answers(capi, b, t, W, H, frames=frames), what)


def view(ctx, t):
    c = t["cam"]
    ctx.set_camera(c[0:3], c[3:6], c[6:9], c[9:12])
    ctx.set_background(t["bg"])
    ctx.set_lights(t["lights"])
    ctx.resize(W * H)
    return ctx


def last_error(capi, ctx):
    return capi.load().rtgo_last_error(ctx._h).decode()


# ---- 1. the set calls ---------------------------------------------------------------------------------------------------------------------
def set_both(torch, capi, t, large, what):
    """(a context set from device tensors, one set by the twin), the tensors checked to be as they were"""
    ts = tensors(torch, capi, t)
    before = words(torch, ts)
    d, h = capi.Context(0), capi.Context(0)
    (d.set_large_scene_device if large else d.set_scene_device)(ts[1], ts[2])
    unchanged(torch, ts, before, what)
    (h.set_large_scene if large else h.set_scene)(t["type"], t["M"], t["mat"], t.get("aabb"))
    return view(d, t), view(h, t)


@pytest.mark.parametrize("with_aabbs", [True, False], ids=["boxes", "cube"])
@pytest.mark.parametrize("n", SIZES)
def test_set_large_scene_device_is_the_twin(capi, torch, oracle, n, with_aabbs):
    t = scene(oracle, ("large", n, with_aabbs))
    what = "rtgo_set_large_scene_device, n %d" % n
    d, h = set_both(torch, capi, t, True, what)
    assert d.stats()["lbvh_depth"] == h.stats()["lbvh_depth"]
    same_context(capi, d, h, t, what, frames=(0, 1))
    d.close()
    h.close()


@pytest.mark.parametrize("name", ["cornell", "quadrics"])
def test_set_scene_device_is_the_twin(capi, torch, oracle, name):
    t = scene(oracle, name)
    what = "rtgo_set_scene_device, " + name
    d, h = set_both(torch, capi, t, False, what)
    same_context(capi, d, h, t, what, frames=(0, 1))
    d.close()
    h.close()


# ---- 2. the update call = its twin ----------------------------------------------------------------------------------------------------------
def update_both(torch, capi, d, h, t_new, idx, rebuild, what):
    ts = tensors(torch, capi, t_new, idx)
    before = words(torch, ts)
    d.update_prims_device(*ts, rebuild=rebuild)
    unchanged(torch, ts, before, what)
    TU.update(h, t_new, idx, rebuild)


@pytest.mark.parametrize("with_aabbs", [True, False], ids=["boxes", "cube"])
@pytest.mark.parametrize("rebuild", [False, True], ids=["refit", "rebuild"])
@pytest.mark.parametrize("n", SIZES)
def test_update_of_a_large_scene_is_the_twin(capi, torch, oracle, n, rebuild, with_aabbs):
    t = scene(oracle, ("large", n, with_aabbs))
    d, h = capi.Context(0), capi.Context(0)
    for what, idx in (("the first", [0]), ("the last", [n - 1]), ("all", np.arange(n)[::-1])):
        for ctx in (d, h):
            TU.set_scene(ctx, t, True, W * H)
            ctx.launch(capi.make_frame(W, H, 1, 0, True, False))   # (a mask and seeds over the old bounds)
        t_new = TU.large_edit(oracle, t, idx, 7 * n + len(idx))
        label = "n %d, %s, %s" % (n, what, "rebuild" if rebuild else "refit")
        update_both(torch, capi, d, h, t_new, idx, rebuild, label)
        assert d.stats()["lbvh_depth"] == h.stats()["lbvh_depth"]
        same_context(capi, d, h, t_new, label)
    d.close()
    h.close()


@pytest.mark.parametrize("rebuild", [False, True], ids=["refit", "rebuild"])
@pytest.mark.parametrize("name", ["cornell", "balls", "room", "quadrics"])
def test_update_of_a_resident_scene_is_the_twin(capi, torch, oracle, name, rebuild):
    """the first edit of tests/test_update_prims.py's lds_edits for each scene of rtgo_set_scene, both flags"""
    t, w, h_ = TU.tables(oracle, name)
    what, steps = TU.lds_edits(oracle, name, t)[0]
    d, h = TU.set_scene(capi.Context(0), t, False, w * h_), TU.set_scene(capi.Context(0), t, False, w * h_)
    for ctx in (d, h):
        ctx.launch(capi.make_frame(w, h_, 1, 0, True, False))   # (a mask, seeds and a trial to drop)
    for k, (idx, t_new) in enumerate(steps):
        label = "%s: %s, step %d" % (name, what, k)
        update_both(torch, capi, d, h, t_new, idx, rebuild, label)
        TU.same_digests(d, h, label)
        same_bvh(d, h, label)
        TU.assert_same_answers(TU.answers(capi, d, t_new, w, h_, name, frames=(0,)), TU.answers(capi, h, t_new, w, h_, name, frames=(0,)), label)
    d.close()
    h.close()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------------
def raw(capi, ctx, idx, prims, aabbs, k, flags=0, offset=(0, 0, 0)):
    """the bare C call on tensors (or None); offset: bytes added to the three pointers"""
    p = lambda t, o: C.c_void_p(None if t is None else t.data_ptr() + o)
    return capi.load().rtgo_update_prims_device(ctx._h, p(idx, offset[0]), p(prims, offset[1]), p(aabbs, offset[2]), k, flags)


def refusal_cases(n, k, positions):
    """[(what, field, entry, value)]: each bad entry of the list at each position"""
    out = []
    for j in positions:
        out += [("a NaN in the model matrix", "model", j, "nan"), ("+Inf in Le", "Le", j, None), ("a zero scale column", "model", j, "column"),
                ("type 4", "type", j, 4), ("a box with min > max", "box", j, "empty"), ("a NaN in a box", "box", j, "nan"),
                ("an index equal to n", "index", j, n), ("index 0xFFFFFFFF", "index", j, 0xFFFFFFFF)]
    return out


def spoiled(capi, good_idx, good_rec, good_box, field, j, value):
    idx, rec, box = good_idx.copy(), good_rec.copy(), good_box.copy()
    if field == "model" and value == "column":
        rec["model"][j].reshape(4, 4)[:3, 1] = 0.0          # the y axis scaled to nothing: determinant 0
    elif field == "model":
        rec["model"][j][5] = np.nan
    elif field == "Le":
        rec["Le"][j][2] = np.inf
    elif field == "type":
        rec["type"][j] = value
    elif field == "box" and value == "empty":
        box[j, 4] = box[j, 1] - 1.0                           # maxY below minY
    elif field == "box":
        box[j, 2] = np.nan
    else:
        idx[j] = value
    return idx, rec, box


def upload(torch, idx, rec, box):
    ts = (dev(torch, idx.view(np.int32), np.int32), dev(torch, rec.view(np.uint8).reshape(len(rec), 108), np.uint8), dev(torch, box, np.float32))
    torch.cuda.synchronize()
    return ts


@pytest.mark.parametrize("rebuild", [False, True], ids=["refit", "rebuild"])
@pytest.mark.parametrize("kind", ["large", "cornell"])
def test_refusals_leave_everything(capi, torch, oracle, kind, rebuild):
    large = kind == "large"
    t = scene(oracle, ("large", 513, True) if large else "cornell")
    n = len(t["type"])
    k, flags = n, int(rebuild)
    positions = (0, 256, k - 1) if large else (0, k - 1)
    d, h = TU.set_scene(capi.Context(0), t, large, W * H), TU.set_scene(capi.Context(0), t, large, W * H)
    f0 = capi.make_frame(W, H, 1, 0, True, False)
    d.launch(f0)
    d.sync()
    frame, digests, stats = d.read_accum(H, W).copy(), d.build_digest(False), d.stats()
    # a good update of every primitive, in reversed order: what is refused below is this with one entry spoiled
    order = np.arange(n)[::-1].copy()
    t_new = TU.large_edit(oracle, t, order, 77) if large else TU.edit(oracle, t, order, M=TU.moved(t["M"][order], (0.05, 0.0, -0.05)))
    g_idx, g_rec, g_box = order.astype(np.uint32), TU.records(capi, t_new, order), np.ascontiguousarray(t_new["aabb"][order], np.float32)

    def refused(what, ts, count, code, entries=None, fl=flags, offset=(0, 0, 0)):
        before = words(torch, ts)
        assert raw(capi, d, ts[0], ts[1], ts[2], count, fl, offset) == code, "%s: %s" % (kind, what)
        msg = last_error(capi, d)
        assert msg, what
        if entries is not None:
            named = re.search(r"entry (\d+)", msg)
            assert named and int(named.group(1)) in entries, "%s: %r does not name entry %s" % (what, msg, entries)
        unchanged(torch, ts, before, what)
        assert d.build_digest(False) == digests, what
        assert d.stats() == stats, what

    for what, field, j, value in refusal_cases(n, k, positions):
        refused("%s at entry %d" % (what, j), upload(torch, *spoiled(capi, g_idx, g_rec, g_box, field, j, value)), k, RTGO_E_INVALID, (j,))
    # an index named twice: a pair next to each other in one wave, and a pair a whole call apart (then one index is named by no entry)
    near = 100 if large else 3
    for what, a, b in (("neighbours", near, near + 1), ("the first and the last entry", 0, k - 1)):
        idx = g_idx.copy()
        idx[b] = idx[a]
        refused("an index named twice, " + what, upload(torch, idx, g_rec, g_box), k, RTGO_E_INVALID, (a, b))
    # what the host decides, before any launch
    good = upload(torch, g_idx, g_rec, g_box)
    more = upload(torch, np.append(g_idx, 0).astype(np.uint32), np.append(g_rec, g_rec[:1]), np.concatenate([g_box, g_box[:1]]))
    refused("n_updates = n + 1", more, k + 1, RTGO_E_INVALID)
    for which in range(3):   # (the call refuses the pointer before any dereference: the tensors are good, the address is not used)
        refused("a pointer one byte off", good, k, RTGO_E_INVALID, offset=tuple(1 if q == which else 0 for q in range(3)))
    refused("no boxes for a scene set with boxes", (good[0], good[1], None), k, RTGO_E_INVALID)
    refused("flag 2", good, k, RTGO_E_INVALID, fl=2)
    refused("a high flag bit", good, k, RTGO_E_INVALID, fl=flags | 1 << 31)
    refused("NULL indices", (None, good[1], good[2]), k, RTGO_E_INVALID)
    refused("NULL prims", (good[0], None, good[2]), k, RTGO_E_INVALID)
    assert raw(capi, d, None, None, None, 0, flags) == RTGO_OK   # no updates: nothing to check, nothing changes
    assert raw(capi, d, good[0], good[1], good[2], 0, flags) == RTGO_OK
    assert d.build_digest(False) == digests and d.stats() == stats
    d.launch(f0)
    d.sync()
    assert np.array_equal(TU.bits(d.read_accum(H, W)), TU.bits(frame)), kind
    # and the call as given is good -- the claim words of the refused calls do not stand in its way -- and equals the twin's
    assert raw(capi, d, good[0], good[1], good[2], k, flags) == RTGO_OK, last_error(capi, d)
    TU.update(h, t_new, order, rebuild)
    assert d.build_digest(False) != digests
    same_context(capi, d, h, t_new, kind + ": a good update after the refusals")
    d.close()
    h.close()


def test_boxes_for_a_scene_set_without_are_refused(capi, torch, oracle):
    t = scene(oracle, ("large", 257, False))
    d = TU.set_scene(capi.Context(0), t, True, W * H)
    digests, stats = d.build_digest(False), d.stats()
    idx, prims, _ = tensors(torch, capi, t, [3, 256])
    boxes = dev(torch, np.array([[0, 0, 0, 1, 1, 1]] * 2), np.float32)
    torch.cuda.synchronize()
    for flags in (0, 1):
        assert raw(capi, d, idx, prims, boxes, 2, flags) == RTGO_E_INVALID
        assert "without boxes" in last_error(capi, d)
    assert d.build_digest(False) == digests and d.stats() == stats
    d.close()


def test_no_analytic_scene_is_a_state_error(capi, torch, oracle):
    t = scene(oracle, ("large", 3, False))
    idx, prims, _ = tensors(torch, capi, t, [0])
    d = capi.Context(0)
    for flags in (0, 1):
        assert raw(capi, d, idx, prims, None, 1, flags) == RTGO_E_STATE
        assert raw(capi, d, None, None, None, 0, flags) == RTGO_E_STATE
    d.close()


@pytest.mark.parametrize("kind", ["large", "cornell"])
def test_a_refused_set_call_keeps_the_scene(capi, torch, oracle, kind):
    """a NaN at record 256 of 513 (rtgo_set_large_scene_device) and at record 5 of cornell (rtgo_set_scene_device): the context holds and
    renders the scene it had"""
    large = kind == "large"
    t = scene(oracle, ("large", 513, True) if large else "cornell")
    n, j = len(t["type"]), 256 if large else 5
    d = TU.set_scene(capi.Context(0), t, large, W * H)
    f0 = capi.make_frame(W, H, 1, 0, True, False)
    d.launch(f0)
    d.sync()
    frame, digests, stats = d.read_accum(H, W).copy(), d.build_digest(False), d.stats()
    every = np.arange(n)
    rec = TU.records(capi, t, every)
    rec["model"][j][6] = np.nan
    _, prims, boxes = upload(torch, every.astype(np.uint32), rec, np.ascontiguousarray(t["aabb"], np.float32))
    before = words(torch, (prims, boxes))
    fn = capi.load().rtgo_set_large_scene_device if large else capi.load().rtgo_set_scene_device
    assert fn(d._h, C.c_void_p(prims.data_ptr()), C.c_void_p(boxes.data_ptr()), n) == RTGO_E_INVALID
    named = re.search(r"entry (\d+)", last_error(capi, d))
    assert named and int(named.group(1)) == j, last_error(capi, d)
    assert fn(d._h, C.c_void_p(prims.data_ptr() + 2), C.c_void_p(boxes.data_ptr()), n) == RTGO_E_INVALID   # (refused before any dereference)
    assert fn(d._h, C.c_void_p(prims.data_ptr()), C.c_void_p(boxes.data_ptr()), 0) == RTGO_E_UNSUPPORTED
    unchanged(torch, (prims, boxes), before, kind)
    assert d.build_digest(False) == digests and d.stats() == stats
    d.launch(f0)
    d.sync()
    assert np.array_equal(TU.bits(d.read_accum(H, W)), TU.bits(frame)), kind
    d.close()


# ---- 4. twice in a row ----------------------------------------------------------------------------------------------------------------------
def test_two_refits_of_the_same_indices_then_a_rebuild(capi, torch, oracle):
    """the claim words of one call carry the call's own stamp: the same 257 indices are free again for the next call"""
    t = scene(oracle, ("large", 513, True))
    d, h = TU.set_scene(capi.Context(0), t, True, W * H), TU.set_scene(capi.Context(0), t, True, W * H)
    idx = np.arange(0, 513, 2)
    assert len(idx) == 257
    t_new = t
    for step, rebuild in enumerate((False, False, True)):
        t_new = TU.large_edit(oracle, t_new, idx, 60 + step)
        update_both(torch, capi, d, h, t_new, idx, rebuild, "step %d" % step)
        TU.same_digests(d, h, "step %d" % step)
        same_bvh(d, h, "step %d" % step)
    same_context(capi, d, h, t_new, "two refits and a rebuild")
    d.close()
    h.close()
