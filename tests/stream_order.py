"""What tests/test_stream_order.py shares: a stall that ends by itself, the two regimes a case runs in, and the comparison.

The yardstick of every case is the waited regime, which the rest of the suite already pins to its references: the context keeps its own
stream, torch.cuda.synchronize() runs before each call and ctx.sync() after it.  The unwaited regime runs the same case on a second
context that was handed a torch side stream (rtgo_set_stream): a delay is enqueued on that stream first, the case's torch writes and the
library's calls follow with no host wait, and results are cloned on the stream.  A third, `stale` run is the waited one without the
writes: what a library would answer that read its inputs before the stream had written them.  All three only ever see valid data."""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 7.5        # what output tensors hold before a call (float32; the 8-bit image holds IMAGE_SENTINEL)
IMAGE_SENTINEL = 0xAB
STALL_MS = 50.0       # 20 x the slowest idle-stream host time of an asynchronous call, at least 50, at most 250

IDLE_MS = {}          # name of an asynchronous call -> its longest host time in the waited regime (the stream is idle there), in ms
_calibration = {}


def _elapsed_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _rate(torch, work):
    """units of work(n) per ms: a probe picks n for about 10 ms, then the lowest of three timings; None when they disagree by a quarter"""
    torch.cuda.synchronize()
    probe = 1 << 16
    t = max(_elapsed_ms(torch, lambda: work(probe)), 1e-3)
    n = max(int(probe * 10.0 / t), 1)
    rates = [n / max(_elapsed_ms(torch, lambda: work(n)), 1e-3) for _ in range(3)]
    return min(rates) if max(rates) <= 1.25 * min(rates) else None


def calibrate(torch):
    """once per process: ("sleep", cycles of torch.cuda._sleep per ms), or, where _sleep is missing or unstable, ("matmul", units per ms of a
    chain of 512 x 512 matrix products, 1024 units to a product, the matrix)"""
    if "kind" not in _calibration:
        rate = _rate(torch, lambda n: torch.cuda._sleep(int(n))) if hasattr(torch.cuda, "_sleep") else None
        if rate is not None:
            _calibration.update(kind="sleep", rate=rate)
        else:
            m = torch.eye(512, device="cuda") * 0.5

            def chain(n):
                x = m
                for _ in range(max(int(n) >> 10, 1)):
                    x = x @ m
            rate = _rate(torch, chain)
            assert rate is not None, "neither torch.cuda._sleep nor a matmul chain gives a stable delay on this device"
            _calibration.update(kind="matmul", rate=rate, m=m)
    return _calibration


def stall(torch, stream, ms):
    """a delay of ms on `stream`, then an event: returns the event.  The delay is device work of a fixed length: it ends by itself"""
    cal = calibrate(torch)
    with torch.cuda.stream(stream):
        if cal["kind"] == "sleep":
            torch.cuda._sleep(int(ms * cal["rate"]) + 1)
        else:
            x = cal["m"]
            for _ in range(max((int(ms * cal["rate"]) + 1) >> 10, 1)):
                x = x @ cal["m"]
        ev = torch.cuda.Event()
        ev.record()
    return ev


def dev(torch, a):
    """a numpy array as a device tensor (uint32 as its int32 bits)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def ok(capi, ctx, rc, what="the call"):
    assert rc == 0, "%s failed (%d): %s" % (what, rc, capi.load().rtgo_last_error(ctx._h).decode())


class Run:
    """One regime of a case over some contexts.  stream None: waited.  Otherwise the contexts run on `stream`, behind a stall."""

    def __init__(self, torch, ctxs, stream=None, stall_ms=STALL_MS):
        self.torch, self.ctxs, self.stream, self.stall_ms = torch, list(ctxs), stream, stall_ms
        self.ctx = self.ctxs[0]
        self.waited = stream is None
        self.ev = None
        self.kept = []

    # ---- tensors of the case, alive until finish(): the stream may still read or write them when the case returns
    def keep(self, *ts):
        self.kept += ts
        return ts[0] if len(ts) == 1 else ts

    def dev(self, a):
        return self.keep(dev(self.torch, a))

    def outputs(self, pixels):
        """(accum float32 [pixels, 4], image uint8 [pixels, 4]) holding the sentinels"""
        t = self.torch
        return self.keep(t.full((pixels, 4), SENTINEL, dtype=t.float32, device="cuda"), t.full((pixels, 4), IMAGE_SENTINEL, dtype=t.uint8, device="cuda"))

    def bound(self, pixels, ctx=None):
        acc, img = self.outputs(pixels)
        (ctx or self.ctx).bind_output(acc.data_ptr(), img.data_ptr(), pixels)
        return acc, img

    # ---- the regime
    def begin(self, synchronize=True):
        """the set-up is complete; from here on nothing waits but what the regime says"""
        if synchronize:
            self.torch.cuda.synchronize()
        if not self.waited:
            for c in self.ctxs:
                c.set_stream(self.stream.cuda_stream)
            self.ev = stall(self.torch, self.stream, self.stall_ms)

    def on(self):
        """the stream the case's torch work goes to"""
        return contextlib.nullcontext() if self.waited else self.torch.cuda.stream(self.stream)

    def call(self, fn, *args, asynchronous=False, ctx=None, name=None):
        """fn(*args) in this regime.  asynchronous: the header calls it so -- unwaited, it must return within a quarter of the stall and
        while the stall is still pending (so before its inputs were written); waited, its host time over an idle stream is noted"""
        name = name or getattr(fn, "__name__", "call")
        if self.waited:
            self.torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*args)
            dt = (time.perf_counter() - t0) * 1e3
            (ctx or self.ctx).sync()
            if asynchronous:
                IDLE_MS[name] = max(IDLE_MS.get(name, 0.0), dt)
            return r
        t0 = time.perf_counter()
        r = fn(*args)
        dt = (time.perf_counter() - t0) * 1e3
        pending = not self.ev.query()
        if asynchronous:
            assert dt < self.stall_ms / 4, "%s took %.2f ms of host time behind a stall of %.0f ms: it waited" % (name, dt, self.stall_ms)
            assert pending, "%s returned after the stall had ended (%.2f ms): the call proves nothing about its inputs" % (name, dt)
        return r

    def finish(self):
        self.torch.cuda.synchronize()
        for c in self.ctxs:
            c.sync()
        if not self.waited:
            for c in self.ctxs:
                c.set_stream(None)


COUNTERS = ("rays_total", "rays_occlusion", "rays_culled", "launches")


def host(torch, res):
    """a case's results on the host: tensors as bytes, everything else as it is"""
    return {k: (v.contiguous().cpu().numpy().view(np.uint8).copy() if hasattr(v, "data_ptr") else v) for k, v in res.items()}


def differing(a, b):
    assert list(a) == list(b), (list(a), list(b))
    return [k for k in a if not (np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k])]


def regimes(torch, capi, case, n_ctx=1, differs=True, stall_ms=STALL_MS, separate=False):
    """case(R, stale) -> dict of tensors and values, run waited, stale (differs: its results must differ from the waited ones) and
    unwaited, each on fresh contexts; the unwaited results must equal the waited ones bit for bit, the ray counters too.  separate: one
    Run and one stream per context, handed to the case as a list.  Returns the waited results and counters."""
    out = {}
    for regime in ("waited", "stale", "unwaited") if differs else ("waited", "unwaited"):
        ctxs = [capi.Context(0) for _ in range(n_ctx)]
        unwaited = regime == "unwaited"
        if separate:
            runs = [Run(torch, [c], torch.cuda.Stream() if unwaited else None, stall_ms) for c in ctxs]
        else:
            runs = [Run(torch, ctxs, torch.cuda.Stream() if unwaited else None, stall_ms)]
        try:
            res = case(runs if separate else runs[0], regime == "stale")
            for r in runs:
                r.finish()
            res = host(torch, res)
            for k, c in enumerate(ctxs):
                st = c.stats()
                res["counters %d" % k] = tuple(st[f] for f in COUNTERS)
            out[regime] = res
        finally:
            torch.cuda.synchronize()   # (a failed case may leave work queued that reads the contexts' buffers)
            for c in ctxs:
                c.close()
    if differs:
        assert differing(out["stale"], out["waited"]), "the stale inputs give the same results as the written ones: the case shows nothing"
    bad = differing(out["unwaited"], out["waited"])
    assert not bad, "on a backed-up stream these differ from the waited run: %s" % bad
    return out["waited"]


def wrote_all(res, keys):
    """the accumulation buffers `keys` of host results hold no sentinel: alpha is 1 in every pixel"""
    for k in keys:
        a = res[k].view(np.float32).reshape(-1, 4)
        assert (a[:, 3] == 1.0).all(), "%s: %d pixels were never written" % (k, (a[:, 3] != 1.0).sum())


# ---- the bare calls the binding wraps with a device-wide wait -----------------------------------------------------------------------------
def raw_set_scene_device(capi, ctx, prims, aabbs, large):
    L = capi.load()
    n, p = capi.device_prims_args("set_scene_device", ctx.device, None, prims, aabbs)
    rc = (L.rtgo_set_large_scene_device if large else L.rtgo_set_scene_device)(ctx._h, C.c_void_p(p[1]), C.c_void_p(p[2]), n)
    if rc == 0:
        ctx.n_prims = n
    return rc


def raw_update_prims_device(capi, ctx, indices, prims, aabbs, rebuild):
    k, p = capi.device_prims_args("update_prims_device", ctx.device, indices, prims, aabbs)
    return capi.load().rtgo_update_prims_device(ctx._h, C.c_void_p(p[0]), C.c_void_p(p[1]), C.c_void_p(p[2]), k,
                                                capi.UPDATE_REBUILD if rebuild else capi.UPDATE_REFIT)


def assemble_bands(capi, ctx, hip_stream, gathered, full, w, h, band_h, n_ranks, rows_pad, elem_bytes):
    return capi.load().rtgo_assemble_bands(ctx._h, C.c_void_p(hip_stream or 0), C.c_void_p(gathered.data_ptr()), C.c_void_p(full.data_ptr()), w, h,
                                           band_h, n_ranks, rows_pad, elem_bytes)


def rays_tensor(capi, o, d, tmin, tmax):
    """rtgo_ray records as float32 [n, 8] on the host"""
    return capi.make_rays(o, d, tmin, tmax).view(np.float32).reshape(-1, 8)
