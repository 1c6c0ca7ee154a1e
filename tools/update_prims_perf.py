"""developer tool: what rtgo_update_prims costs and what a refit does to the walk, against setting the scene again
   python tools/update_prims_perf.py [W] [H]
Sphere fields of tools/large_scene_perf.py (one sphere of radius <= 0.3 per unit cube) of n = 1K, 256K and 2^20 primitives, boxes by the
CubeBox rule on the device.
1. Per n and k = 1, 1 % of n, n: k spheres (evenly spaced indices) nudged by up to a radius, back and forth between two positions.
      set      ms of rtgo_set_large_scene over the edited array (the yardstick: the only way to edit before rtgo_update_prims)
      refit    ms of rtgo_update_prims(RTGO_UPDATE_REFIT) over the k records
      rebuild  ms of rtgo_update_prims(RTGO_UPDATE_REBUILD) over the k records
      set_device, refit_device, rebuild_device
               the same three through rtgo_set_large_scene_device and rtgo_update_prims_device, the records and indices in device memory
               beforehand (a second line per k, each with the least and the largest of its samples; `set` again with its spread)
      refit_async
               rtgo_update_prims_device_async over the same device buffers (a third line per k), its `reach` the field's box: `host`, the
               wall clock of the C call over an idle stream (it only enqueues), and `device`, the HIP-event time on the stream from before the
               call to after its last kernel; then host / refit_device and device against refit_device's median and least sample
   All but `device` are WALL-CLOCK times of the C call on records packed beforehand (no Python packing inside), medians of REPS calls
   after WARM, host and device calls in the same run.
2. Per n: a fraction of the spheres scattered to random places of the field by a refit, then the same scene rebuilt: ms per frame at W x H,
   path mode, 1 spp -- HIP-EVENT times (rtgo_stats' total_launch_ms over K launches).  The fractions grow tenfold and stop once a refitted
   frame takes over 30 ms: a refit keeps the topology chosen for the old places, every ancestor of a scattered leaf spans the way it went,
   and the walk pays for it.  refit/rebuilt is that price."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from raytracingo_amd import capi, scene as hscene

W = int(sys.argv[1]) if len(sys.argv) > 1 else 1280
H = int(sys.argv[2]) if len(sys.argv) > 2 else 720
WARM, REPS, K = 2, 9, 8


def field(n):
    rng = np.random.default_rng(n)
    side = 2.0 * round(n ** (1.0 / 3.0)) / 2.0
    rec = np.zeros(n, dtype=capi.PRIM_DTYPE)
    rec["type"] = capi.SPHERE
    M = rec["model"]
    r = rng.uniform(0.05, 0.3, size=n)
    M[:, 0] = M[:, 5] = M[:, 10] = r
    M[:, 3] = rng.uniform(-side / 2, side / 2, size=n)
    M[:, 7] = rng.uniform(-side / 2, side / 2, size=n)
    M[:, 11] = rng.uniform(-side, 0.0, size=n) - 2.0
    M[:, 15] = 1.0
    mat = rng.uniform(0.0, 1.0, size=(n, 10)).astype(np.float32)
    mat[:, 7:10] *= (rng.uniform(size=(n, 1)) < 0.02) * 4.0
    rec["kd"], rec["kr"], rec["specularity"], rec["Le"] = mat[:, 0:3], mat[:, 3:6], mat[:, 6], mat[:, 7:10]
    return rec, side


def samples_ms(call):
    for k in range(WARM):   # (the calls alternate between two inputs: the warm-up goes through both)
        call(k)
    ts = []
    for k in range(REPS):
        t0 = time.perf_counter()
        call(WARM + k)
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def median_ms(call):
    return float(np.median(samples_ms(call)))


def spread(ts):
    return "%8.3f ms [%.3f, %.3f]" % (float(np.median(ts)), min(ts), max(ts))


def c_set(L, ctx, rec):
    rc = L.rtgo_set_large_scene(ctx._h, rec.ctypes.data_as(C.POINTER(capi.Prim)), None, len(rec))
    assert rc == 0, L.rtgo_last_error(ctx._h)
    ctx.n_prims = len(rec)


def c_update(L, ctx, idx, rec, flags):
    rc = L.rtgo_update_prims(ctx._h, idx.ctypes.data_as(C.POINTER(C.c_uint32)), rec.ctypes.data_as(C.POINTER(capi.Prim)), None, len(idx), flags)
    assert rc == 0, L.rtgo_last_error(ctx._h)


class DeviceCopy:
    """a numpy array's bytes in device memory of the process's HIP runtime, freed with the object"""

    def __init__(self, a):
        self.H, self.p = capi.hip_runtime(), C.c_void_p()
        a = np.ascontiguousarray(a)
        assert self.H.hipMalloc(C.byref(self.p), a.nbytes) == 0 and self.H.hipMemcpy(self.p, a.ctypes.data, a.nbytes, 1) == 0

    def __del__(self):
        self.H.hipFree(self.p)


def c_set_device(L, ctx, d_rec, n):
    rc = L.rtgo_set_large_scene_device(ctx._h, d_rec.p, None, n)
    assert rc == 0, L.rtgo_last_error(ctx._h)
    ctx.n_prims = n


def c_update_device(L, ctx, d_idx, d_rec, k, flags):
    rc = L.rtgo_update_prims_device(ctx._h, d_idx.p, d_rec.p, None, k, flags)
    assert rc == 0, L.rtgo_last_error(ctx._h)


class Timer:
    """a stream of the process's HIP runtime for the context and two events on it"""

    def __init__(self, ctx):
        self.H, self.ctx, self.stream, self.ev = capi.hip_runtime(), ctx, C.c_void_p(), [C.c_void_p(), C.c_void_p()]
        H = self.H
        H.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        H.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        H.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        H.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        for fn in (H.hipEventSynchronize, H.hipEventDestroy, H.hipStreamDestroy):
            fn.argtypes = [C.c_void_p]
        assert H.hipStreamCreate(C.byref(self.stream)) == 0 and all(H.hipEventCreate(C.byref(e)) == 0 for e in self.ev)
        ctx.set_stream(self.stream.value)

    def close(self):
        self.ctx.set_stream(None)
        for e in self.ev:
            self.H.hipEventDestroy(e)
        self.H.hipStreamDestroy(self.stream)


def samples_async(L, ctx, timer, d_idx, d_edits, k, reach):
    """per call of rtgo_update_prims_device_async over an idle stream: ([host ms], [device ms]), the warm-up calls left out"""
    H, ticket, status, ms = timer.H, C.c_uint64(), capi.UpdateStatus(), C.c_float()
    host, device = [], []
    for j in range(WARM + REPS):
        ctx.sync()
        H.hipEventRecord(timer.ev[0], timer.stream)
        t0 = time.perf_counter()
        rc = L.rtgo_update_prims_device_async(ctx._h, d_idx.p, d_edits[j % 2].p, None, k, C.byref(reach), C.byref(ticket))
        dt = (time.perf_counter() - t0) * 1e3
        H.hipEventRecord(timer.ev[1], timer.stream)
        assert rc == 0, L.rtgo_last_error(ctx._h)
        assert H.hipEventSynchronize(timer.ev[1]) == 0 and H.hipEventElapsedTime(C.byref(ms), timer.ev[0], timer.ev[1]) == 0
        assert L.rtgo_update_prims_status(ctx._h, ticket, C.byref(status)) == 0 and status.state == capi.UPDATE_APPLIED, (status.state, status.fault, status.entry)
        if j >= WARM:
            host.append(dt)
            device.append(ms.value)
    return host, device


def frame_ms(ctx):
    for f in range(2):
        ctx.launch(capi.make_frame(W, H, 1, f, True))
        ctx.sync()
    ctx.reset_stats()
    for f in range(K):
        ctx.launch(capi.make_frame(W, H, 1, 2 + f, True))
    ctx.sync()
    return ctx.stats()["total_launch_ms"] / K


L = capi.load()
t = hscene.tables("cornell", W, H)
print("rtgo_update_prims, sphere fields, medians of %d calls after %d (wall clock of the synchronous C call); frames %d x %d path 1 spp, HIP events over %d launches" %
      (REPS, WARM, W, H, K), flush=True)
for n in (1 << 10, 1 << 18, 1 << 20):
    rec, side = field(n)
    ctx = capi.Context(0)
    c_set(L, ctx, rec)
    ctx.set_camera(t["cam"][0:3], t["cam"][3:6], t["cam"][6:9], t["cam"][9:12])
    ctx.set_background(t["bg"])
    ctx.set_lights(t["lights"])
    ctx.resize(W * H)
    depth = ctx.stats()["lbvh_depth"]
    centre, r_max = rec["model"][:, [3, 7, 11]], 2.0 * rec["model"][:, 0].max() + 0.01   # (a sphere and its nudge by a radius; the CubeBox pad)
    reach = capi.Aabb(*[float(x) for x in np.concatenate([centre.min(axis=0) - r_max, centre.max(axis=0) + r_max])])
    print("n = %d  LBVH depth %d  as built %.3f ms/frame" % (n, depth, frame_ms(ctx)), flush=True)
    for k in sorted({1, max(n // 100, 1), n}):
        idx = np.ascontiguousarray(np.linspace(0, n - 1, k).astype(np.uint32))
        there = rec[idx].copy()
        there["model"][:, 3] += there["model"][:, 0]
        edits = [there, rec[idx].copy()]     # the calls alternate between the two: every one moves k boxes
        whole = [rec.copy(), rec]
        whole[0][idx] = there
        c_set(L, ctx, rec)
        t_refit = median_ms(lambda j: c_update(L, ctx, idx, edits[j % 2], capi.UPDATE_REFIT))
        c_set(L, ctx, rec)
        t_rebuild = median_ms(lambda j: c_update(L, ctx, idx, edits[j % 2], capi.UPDATE_REBUILD))
        s_set = samples_ms(lambda j: c_set(L, ctx, whole[j % 2]))
        t_set = float(np.median(s_set))
        print("    k = %-8d set %8.3f ms   refit %8.3f ms   rebuild %8.3f ms   set/refit %6.1fx   set/rebuild %5.2fx" %
              (k, t_set, t_refit, t_rebuild, t_set / t_refit, t_set / t_rebuild), flush=True)
        # the same calls from device memory
        d_idx, d_edits, d_whole = DeviceCopy(idx), [DeviceCopy(e) for e in edits], [DeviceCopy(w) for w in whole]
        c_set(L, ctx, rec)
        s_refit_d = samples_ms(lambda j: c_update_device(L, ctx, d_idx, d_edits[j % 2], k, capi.UPDATE_REFIT))
        c_set(L, ctx, rec)
        s_rebuild_d = samples_ms(lambda j: c_update_device(L, ctx, d_idx, d_edits[j % 2], k, capi.UPDATE_REBUILD))
        s_set_d = samples_ms(lambda j: c_set_device(L, ctx, d_whole[j % 2], n))
        print("                 set %s   set_device %s   refit_device %s   rebuild_device %s" %
              (spread(s_set), spread(s_set_d), spread(s_refit_d), spread(s_rebuild_d)), flush=True)
        # the refit that waits for nothing, over the same buffers
        c_set(L, ctx, rec)
        timer = Timer(ctx)
        s_host, s_dev = samples_async(L, ctx, timer, d_idx, d_edits, k, reach)
        timer.close()
        print("                 refit_async host %s   device %s   host / refit_device %.4f   device / refit_device median %.3f, least %.3f" %
              (spread(s_host), spread(s_dev), float(np.median(s_host)) / float(np.median(s_refit_d)), float(np.median(s_dev)) / float(np.median(s_refit_d)),
               float(np.median(s_dev)) / min(s_refit_d)), flush=True)
        del d_idx, d_edits, d_whole
    frac, last_k = 1e-4, 0
    while frac <= 0.011:
        k = max(int(n * frac), 1)
        if k == last_k:
            frac *= 10.0
            continue
        last_k = k
        rng = np.random.default_rng(k)
        idx = np.ascontiguousarray(rng.choice(n, size=k, replace=False).astype(np.uint32))
        far = rec[idx].copy()
        far["model"][:, 3] = rng.uniform(-side / 2, side / 2, size=k)
        far["model"][:, 7] = rng.uniform(-side / 2, side / 2, size=k)
        far["model"][:, 11] = rng.uniform(-side, 0.0, size=k) - 2.0
        c_set(L, ctx, rec)
        c_update(L, ctx, idx, far, capi.UPDATE_REFIT)
        refit = frame_ms(ctx)
        c_update(L, ctx, idx, far, capi.UPDATE_REBUILD)
        rebuilt = frame_ms(ctx)
        print("    %7d scattered (%.2f %%): refitted %9.3f ms/frame   rebuilt %8.3f ms/frame   refit/rebuilt %6.2f   depth %d / %d" %
              (k, 100.0 * k / n, refit, rebuilt, refit / rebuilt, depth, ctx.stats()["lbvh_depth"]), flush=True)
        if refit > 30.0:
            print("    (a refitted frame took over 30 ms: larger fractions not run)", flush=True)
            break
        frac *= 10.0
    ctx.close()
