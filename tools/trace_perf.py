"""developer tool: throughput of the ray queries (rtgo_trace_rays, rtgo_whitted_trace_rays).  python tools/trace_perf.py [repeats]
  1. cornell and checkered, the 1920x1080 pixel-centre primary rays, in raster order and shuffled, with the scene read from global
     memory (RTGO_TRACE_MODE=0) and staged in LDS (RTGO_TRACE_MODE=1): Gray/s
  2. the same two forms over batches of 1 .. 2M raster rays: where staging the scene starts to pay (the host's threshold)
  3. the WaterBottle (tests/golden/waterbottle) through rtgo_whitted_set_mesh: 1080p primaries, raster and shuffled, closest and any-hit
Times are HIP-event times on the context's stream, the best and the median of `repeats` calls after two warm-up calls."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from raytracingo_amd import capi, scene as hscene

W, H = 1920, 1080
K = int(sys.argv[1]) if len(sys.argv) > 1 else 10


def primaries(cam, w, h):
    cam = np.asarray(cam, np.float32)
    eye, U, V, Wv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    fx = 2 * (x + 0.5) / w - 1
    fy = 2 * (y + 0.5) / h - 1
    d = U * fx[..., None] + V * fy[..., None] + Wv
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return capi.make_rays(eye[None], d.reshape(-1, 3).astype(np.float32))


def upload(rays):
    return torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).to("cuda:0")


def timed(ctx, d_rays, n, whitted=False, flags=0, mode=None):
    """(best ms, median ms) of K calls over the first n rays of d_rays"""
    if mode is None:
        os.environ.pop("RTGO_TRACE_MODE", None)
    else:
        os.environ["RTGO_TRACE_MODE"] = str(mode)
    hits = torch.empty((n, 8), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream()
    ms = []
    for k in range(K + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = ctx.trace_rays_raw(d_rays.data_ptr(), hits.data_ptr(), n, flags, whitted)
        e1.record(stream)
        assert rc == 0, rc
        e1.synchronize()
        if k >= 2:
            ms.append(e0.elapsed_time(e1))
    os.environ.pop("RTGO_TRACE_MODE", None)
    return min(ms), float(np.median(ms)), hits


def line(what, n, best, med):
    print("%-44s %8d rays  best %8.3f ms  median %8.3f ms  %7.3f Gray/s" % (what, n, best, med, n / best / 1e6), flush=True)


stream = torch.cuda.Stream(device="cuda:0")
with torch.cuda.stream(stream):
    rng = np.random.RandomState(1)
    print("== analytic path, %dx%d primaries, %d timed calls" % (W, H, K), flush=True)
    for name in ("cornell", "checkered"):
        t = hscene.tables(name, W, H)
        ctx = capi.Context(0)
        ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
        ctx.set_stream(stream.cuda_stream)
        rays = primaries(t["cam"], W, H)
        raster, shuffled = upload(rays), upload(rays[rng.permutation(len(rays))])
        stream.synchronize()
        for order, d_rays in (("raster", raster), ("shuffled", shuffled)):
            for mode, form in ((0, "global"), (1, "LDS")):
                best, med, hits = timed(ctx, d_rays, len(rays), mode=mode)
                line("%s %s, scene in %s" % (name, order, form), len(rays), best, med)
        print("   (%d primitives; %.1f %% of the rays hit)" % (len(t["type"]), 100.0 * (hits[:, 1].view(torch.int32) >= 0).float().mean().item()), flush=True)
        print("== %s: batch size against form (raster rays)" % name, flush=True)
        for sh in (0, 6, 8, 10, 12, 14, 16, 17, 18, 19, 20, 21):
            n = 1 << sh
            g, l = timed(ctx, raster, n, mode=0), timed(ctx, raster, n, mode=1)
            print("   n = %8d   global %8.4f ms   LDS %8.4f ms   %s" % (n, g[0], l[0], "LDS" if l[0] < g[0] else "global"), flush=True)
        ctx.close()

    print("== triangle path: WaterBottle, %dx%d primaries" % (W, H), flush=True)
    import whitted_scene
    wb = whitted_scene.waterbottle()
    eye, look, up, fov = np.array([0.12, 0.08, 0.42]), np.zeros(3), np.array([0.0, 1.0, 0.0]), 40.0
    Wv = look - eye
    U = np.cross(Wv, up)
    U /= np.linalg.norm(U)
    V = np.cross(U, Wv)
    V /= np.linalg.norm(V)
    vlen = np.linalg.norm(Wv) * np.tan(0.5 * np.radians(fov))
    cam = np.concatenate([eye, U * vlen * W / H, V * vlen, Wv]).astype(np.float32)
    ctx = capi.Context(0)
    ctx.whitted_set_mesh(wb["positions"], wb["normals"], wb["indices"], None, wb["materials"])
    ctx.set_stream(stream.cuda_stream)
    rays = primaries(cam, W, H)
    rays["tmin"] = 0.01
    raster, shuffled = upload(rays), upload(rays[rng.permutation(len(rays))])
    stream.synchronize()
    for order, d_rays in (("raster", raster), ("shuffled", shuffled)):
        for flags, kind in ((0, "closest"), (capi.TRACE_ANY_HIT, "any-hit")):
            best, med, hits = timed(ctx, d_rays, len(rays), whitted=True, flags=flags)
            line("WaterBottle %s, %s" % (order, kind), len(rays), best, med)
    print("   (%d triangles; %.1f %% of the rays hit)" % (len(wb["indices"]), 100.0 * (hits[:, 1].view(torch.int32) >= 0).float().mean().item()), flush=True)
    ctx.close()
