"""rtgo_whitted_refit_instances_device_async on a caller's stream that is backed up behind a delay (tests/stream_order.py), on the MI355X.

The header calls it asynchronous: it "waits for nothing on the host".  So behind a stall the call returns at once, while the tensor it
was given is not written yet; the update, and the launch enqueued behind it, see what the stream wrote.  The scene is
tests/test_stream_order.py's small instanced one, in its 64 x 48 frames.  Every case first makes one accepted call and waits: the
context's ring and the scene's staging are allocated by then, and no later call allocates."""
import numpy as np
import pytest

import stream_order as SO
import test_stream_order as TS
import test_whitted_instances_device as TI

pytestmark = pytest.mark.gpu

W, H = TS.WW, TS.WH
PENDING, APPLIED, REFUSED = 0, 1, 2
CLEAN = {"state": APPLIED, "fault": 0, "entry": 0}
NAME, STATUS = "rtgo_whitted_refit_instances_device_async", "rtgo_whitted_refit_instances_status"
SHIFT = [0, 0, 0, 0.3, 0, 0, 0, -0.2, 0, 0, 0, 0.25]   # added to the twelve words of every transform: a translation


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


def shifted(inst):
    return [(np.asarray(tr, np.float32) + np.float32(SHIFT).reshape(3, 4), m, off) for tr, m, off in inst]


def warmed(capi, torch, oracle, R, meshes, inst):
    """R's context with the scene and its view, one accepted update (the scene's own instances) made and waited for; the records as a
    float32 [n, 14] tensor the case may write"""
    ctx = R.ctx
    TS.whitted_ctx(capi, oracle, ctx, meshes, inst)
    rec = R.keep(torch.from_numpy(TI.records(inst).view(np.float32).copy()).cuda())
    torch.cuda.synchronize()
    ticket = ctx.whitted_refit_instances_device_async(rec)
    ctx.sync()
    assert ctx.whitted_refit_instances_status(ticket) == CLEAN
    return ctx, rec


def reference_frame(capi, torch, oracle, meshes, inst, new=None):
    """the accumulation buffer of a context of its own: the scene, then (new) the synchronous refit, one launch"""
    ctx = capi.Context(0)
    try:
        TS.whitted_ctx(capi, oracle, ctx, meshes, inst)
        ctx.resize(W * H)
        if new is not None:
            ctx.whitted_set_instances_device(TI.on_device(torch, new), refit=True)
        ctx.whitted_launch(W, H, 0)
        ctx.sync()
        return ctx.read_accum(H, W).view(np.uint8).reshape(-1)
    finally:
        ctx.close()


def test_behind_a_stall_it_reads_what_the_stream_wrote(capi, torch, oracle):
    meshes, inst = TS.whitted_small()

    def case(R, stale):
        ctx, rec = warmed(capi, torch, oracle, R, meshes, inst)
        acc, img = R.bound(W * H)
        shift = R.keep(torch.tensor(SHIFT, dtype=torch.float32, device="cuda"))
        R.begin()
        with R.on():
            if not stale:
                rec[:, :12] += shift
            R.call(ctx.whitted_refit_instances_device_async, rec, asynchronous=True, name=NAME)
            R.call(ctx.whitted_launch, W, H, 0)
            return {"accum": acc.clone(), "image": img.clone()}

    waited = SO.regimes(torch, capi, case)
    SO.wrote_all(waited, ["accum"])
    assert np.array_equal(waited["accum"].reshape(-1), reference_frame(capi, torch, oracle, meshes, inst, shifted(inst))), "against the synchronous refit"


def test_the_status_is_pending_while_the_stall_is(capi, torch, oracle):
    meshes, inst = TS.whitted_small()
    ctx = capi.Context(0)
    R = SO.Run(torch, [ctx], torch.cuda.Stream())
    try:
        _, rec = warmed(capi, torch, oracle, R, meshes, inst)
        R.begin()
        with R.on():
            ticket = R.call(ctx.whitted_refit_instances_device_async, rec, asynchronous=True, name=NAME)
            st = R.call(ctx.whitted_refit_instances_status, ticket, asynchronous=True, name=STATUS)
        assert st == {"state": PENDING, "fault": 0, "entry": 0}
        R.finish()
        assert ctx.whitted_refit_instances_status(ticket) == CLEAN
    finally:
        torch.cuda.synchronize()
        ctx.close()


@pytest.mark.parametrize("which", ["the stream spoils the tensor", "the stream repairs the tensor"])
def test_a_deferred_refusal_is_decided_on_what_the_stream_wrote(capi, torch, oracle, which):
    """a NaN in instance 2's transform: written by torch on the stream behind the stall (PENDING at return, REFUSED afterwards, the frame
    the untouched scene's), or there before the call and overwritten by the stream with good records (APPLIED, the frame the twin's)"""
    meshes, inst = TS.whitted_small()
    new = shifted(inst)
    spoils = which == "the stream spoils the tensor"
    ctx = capi.Context(0)
    R = SO.Run(torch, [ctx], torch.cuda.Stream())
    try:
        _, rec = warmed(capi, torch, oracle, R, meshes, inst)
        acc, _ = R.bound(W * H)
        good = R.keep(torch.from_numpy(TI.records(new).view(np.float32).copy()).cuda())
        nan = R.keep(torch.full((1,), float("nan"), dtype=torch.float32, device="cuda"))
        if not spoils:
            rec[2, 5:6] = nan
        R.begin()
        with R.on():
            if spoils:
                rec[2, 5:6] = nan
            else:
                rec.copy_(good)
            ticket = R.call(ctx.whitted_refit_instances_device_async, rec, asynchronous=True, name=NAME)
            st = R.call(ctx.whitted_refit_instances_status, ticket, asynchronous=True, name=STATUS)
            R.call(ctx.whitted_launch, W, H, 0)
            shown = acc.clone()
        assert st == {"state": PENDING, "fault": 0, "entry": 0}
        R.finish()
        said = ctx.whitted_refit_instances_status(ticket)
        assert said == ({"state": REFUSED, "fault": 4, "entry": 2} if spoils else CLEAN), said
        want = reference_frame(capi, torch, oracle, meshes, inst, None if spoils else new)
        assert np.array_equal(SO.host(torch, {"accum": shown})["accum"].reshape(-1), want)
    finally:
        torch.cuda.synchronize()
        ctx.close()
