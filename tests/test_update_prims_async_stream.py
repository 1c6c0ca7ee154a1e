"""rtgo_update_prims_device_async on a caller's stream that is backed up behind a delay (tests/stream_order.py), on the MI355X.

The header calls it asynchronous: it "waits for nothing on the host".  So behind a stall the call returns at once, while the buffers it
was given are not written yet; the update, and the launch enqueued behind it, see what the stream wrote.  Cornell is set as a large
scene, in frames of tests/test_stream_order.py's size.  Every case first makes one accepted call and waits: the context's ring and the
scene's claim words are allocated by then, and no later call allocates."""
import numpy as np
import pytest

import stream_order as SO
import test_prims_device as TP
import test_stream_order as TS
import test_update_prims as TU
import test_update_prims_async as TA

pytestmark = pytest.mark.gpu

W, H = TS.W, TS.H
PENDING, APPLIED, REFUSED = TA.PENDING, TA.APPLIED, TA.REFUSED
NAME = "rtgo_update_prims_device_async"


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


def cornell(oracle):
    """(cornell, its short box's indices and cornell with it moved, the tall box's, a reach that holds all three)"""
    t0 = TS.analytic(oracle, "cornell")
    idx_a, t_a = TS.box_moved(oracle, t0, "short")
    idx_b, t_b = TS.box_moved(oracle, t0, "tall")
    return t0, (idx_a, t_a), (idx_b, t_b), TA.union(t0["aabb"], t_a["aabb"], t_b["aabb"])


def warmed(capi, torch, R, t0, idx, reach):
    """R's context with cornell as a large scene, one accepted update (of nothing: primitives idx as they are) made and waited for"""
    ctx = TS.analytic_ctx(R.ctx, t0, True)
    same = R.keep(*TP.tensors(torch, capi, t0, idx))
    ticket = ctx.update_prims_device_async(*same, reach=reach)
    ctx.sync()
    assert ctx.update_prims_status(ticket)["state"] == APPLIED
    return ctx


def test_behind_a_stall_it_reads_what_the_stream_wrote(capi, torch, oracle):
    t0, (idx_a, t_a), (idx_b, t_b), reach = cornell(oracle)

    def case(R, stale):
        ctx = warmed(capi, torch, R, t0, idx_a, reach)
        acc, img = R.bound(W * H)
        ctx.launch(TS.frame(capi))   # (a screen rectangle over the old scene)
        ctx.sync()
        bufs = R.keep(*TP.tensors(torch, capi, t_a, idx_a))
        new = R.keep(*TP.tensors(torch, capi, t_b, idx_b))
        R.begin()
        with R.on():
            if not stale:
                for dst, src in zip(bufs, new):
                    dst.copy_(src)
            R.call(ctx.update_prims_device_async, bufs[0], bufs[1], bufs[2], reach, asynchronous=True, name=NAME)
            R.call(ctx.launch, TS.frame(capi))
            return {"accum": acc.clone(), "image": img.clone()}

    SO.wrote_all(SO.regimes(torch, capi, case), ["accum"])


def test_the_status_is_pending_while_the_stall_is(capi, torch, oracle):
    t0, (idx_a, t_a), _, reach = cornell(oracle)
    ctx = capi.Context(0)
    R = SO.Run(torch, [ctx], torch.cuda.Stream())
    try:
        warmed(capi, torch, R, t0, idx_a, reach)
        bufs = R.keep(*TP.tensors(torch, capi, t_a, idx_a))
        R.begin()
        with R.on():
            ticket = R.call(ctx.update_prims_device_async, bufs[0], bufs[1], bufs[2], reach, asynchronous=True, name=NAME)
            st = R.call(ctx.update_prims_status, ticket, asynchronous=True, name="rtgo_update_prims_status")
        assert st == {"state": PENDING, "fault": 0, "entry": 0}
        R.finish()
        assert ctx.update_prims_status(ticket) == {"state": APPLIED, "fault": 0, "entry": 0}
    finally:
        torch.cuda.synchronize()
        ctx.close()


def test_a_deferred_refusal_is_decided_on_what_the_stream_wrote(capi, torch, oracle):
    """the stream spoils the indices (one named twice: valid data all the same), the call is made, a frame rendered; then the stream
    writes the good indices back and the same happens again.  SO.regimes' three runs and comparisons, with the tickets asked about
    once each run has finished: the unwaited run never waits before that"""
    t0, (idx, t_a), _, reach = cornell(oracle)
    out, said = {}, {}
    for regime in ("waited", "stale", "unwaited"):
        ctx = capi.Context(0)
        R = SO.Run(torch, [ctx], torch.cuda.Stream() if regime == "unwaited" else None)
        try:
            warmed(capi, torch, R, t0, idx, reach)
            acc, img = R.bound(W * H)
            i, rec, boxes = R.keep(*TP.tensors(torch, capi, t_a, idx))
            good, bad = R.keep(i.clone(), i.clone())
            bad[1] = bad[0]
            R.begin()
            with R.on():
                if regime != "stale":
                    i.copy_(bad)
                first = R.call(ctx.update_prims_device_async, i, rec, boxes, reach, asynchronous=True, name=NAME)
                R.call(ctx.launch, TS.frame(capi))
                res = {"accum after the spoiled indices": acc.clone()}
                if regime != "stale":
                    i.copy_(good)
                second = R.call(ctx.update_prims_device_async, i, rec, boxes, reach, asynchronous=True, name=NAME)
                R.call(ctx.launch, TS.frame(capi))
                res["accum after the good indices"] = acc.clone()
            R.finish()
            out[regime] = SO.host(torch, res)
            said[regime] = [ctx.update_prims_status(k) for k in (first, second)]
        finally:
            torch.cuda.synchronize()
            ctx.close()
    assert SO.differing(out["stale"], out["waited"]), "the stale inputs give the same results as the written ones: the case shows nothing"
    assert not SO.differing(out["unwaited"], out["waited"])
    SO.wrote_all(out["waited"], list(out["waited"]))
    for regime in ("waited", "unwaited"):
        refused, applied = said[regime]
        assert refused["state"] == REFUSED and refused["fault"] == 6 and refused["entry"] in (0, 1), (regime, refused)
        assert applied == {"state": APPLIED, "fault": 0, "entry": 0}, (regime, applied)
    assert [s["state"] for s in said["stale"]] == [APPLIED, APPLIED]
    # the refused update left the scene un-updated, the good one moved the box
    plain, moved = capi.Context(0), capi.Context(0)
    try:
        for ctx, t in ((plain, t0), (moved, t_a)):
            TU.set_scene(ctx, t, True, W * H)
            ctx.launch(TS.frame(capi))
            ctx.sync()
        for key, ctx in (("accum after the spoiled indices", plain), ("accum after the good indices", moved)):
            assert np.array_equal(out["unwaited"][key].reshape(-1), ctx.read_accum(H, W).view(np.uint8).reshape(-1)), key
    finally:
        plain.close()
        moved.close()
