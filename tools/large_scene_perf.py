"""developer tool: what rtgo_set_large_scene costs.  python tools/large_scene_perf.py [frames]
  1. ms per frame of cornell / balls / checkered at 1920x1080 through rtgo_set_scene (fast walk, LDS) and rtgo_set_large_scene (canonical
     walk, global memory), path mode, N = 2 (4 spp)
  2. random sphere fields of 1K, 16K, 256K and 1M primitives at 1920x1080, N = 2, path mode: rtgo_set_large_scene time, LBVH depth, ms per frame
Each case's first launch runs with RTGO_DEBUG set: rtgo_launch's line on stderr gives the launch shape (threads per workgroup, LDS,
workgroups per CU)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from raytracingo_amd import capi, scene as hscene

W, H, N = 1920, 1080, 2
K = int(sys.argv[1]) if len(sys.argv) > 1 else 10


def setup(ctx, t):
    ctx.set_camera(t["cam"][0:3], t["cam"][3:6], t["cam"][6:9], t["cam"][9:12])
    ctx.set_background(t["bg"])
    ctx.set_lights(t["lights"])
    ctx.resize(W * H)


def time_frames(ctx, what):
    os.environ["RTGO_DEBUG"] = "1"
    sys.stderr.write("%s: " % what)
    sys.stderr.flush()
    ctx.launch(capi.make_frame(W, H, N, 0, True))
    ctx.sync()
    del os.environ["RTGO_DEBUG"]
    for f in range(1, 4):   # (the fast walk's launch-time trial, when there is one)
        ctx.launch(capi.make_frame(W, H, N, f, True))
        ctx.sync()
    ctx.reset_stats()
    for f in range(K):
        ctx.launch(capi.make_frame(W, H, N, 4 + f, True))
        ctx.sync()
    st = ctx.stats()
    return st["total_launch_ms"] / K, st


print("== reference scenes, %dx%d N=%d path, %d timed frames" % (W, H, N, K), flush=True)
for name in ("cornell", "balls", "checkered"):
    t = hscene.tables(name, W, H)
    ms = {}
    for large in (False, True):
        ctx = capi.Context(0)
        (ctx.set_large_scene if large else ctx.set_scene)(t["type"], t["M"], t["mat"], t["aabb"])
        setup(ctx, t)
        ms[large], st = time_frames(ctx, "%s %s" % (name, "large" if large else "small"))
        ctx.close()
    print("%-10s %4d prims  rtgo_set_scene %7.3f ms  rtgo_set_large_scene %7.3f ms  (x%.2f)  depth %d" %
          (name, len(t["type"]), ms[False], ms[True], ms[True] / ms[False], st["lbvh_depth"]), flush=True)

print("== sphere fields, %dx%d N=%d path, %d timed frames" % (W, H, N, K), flush=True)
t = hscene.tables("cornell", W, H)
for n in (1 << 10, 1 << 14, 1 << 18, 1 << 20):
    rng = np.random.default_rng(n)
    # spheres in a cube of side ~ n^(1/3) in front of the camera (density fixed: one sphere of radius <= 0.3 per unit cube)
    side = 2.0 * round(n ** (1.0 / 3.0)) / 2.0
    M = np.zeros((n, 16), dtype=np.float32)
    r = rng.uniform(0.05, 0.3, size=n)
    M[:, 0] = M[:, 5] = M[:, 10] = r
    M[:, 3] = rng.uniform(-side / 2, side / 2, size=n)
    M[:, 7] = rng.uniform(-side / 2, side / 2, size=n)
    M[:, 11] = rng.uniform(-side, 0.0, size=n) - 2.0
    M[:, 15] = 1.0
    mat = rng.uniform(0.0, 1.0, size=(n, 10)).astype(np.float32)
    mat[:, 7:10] *= (rng.uniform(size=(n, 1)) < 0.02) * 4.0
    types = np.full(n, 3, dtype=np.uint32)
    ctx = capi.Context(0)
    builds = []
    for rep in range(3):
        t0 = time.perf_counter()
        ctx.set_large_scene(types, M, mat, None)
        builds.append((time.perf_counter() - t0) * 1e3)
    setup(ctx, t)
    ctx.set_camera([0.0, 0.0, side * 0.6], [1.0 * W / H, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.5])
    ms, st = time_frames(ctx, "spheres %d" % n)
    print("spheres %8d  rtgo_set_large_scene %8.1f ms (best of 3: %s)  depth %d  %8.3f ms/frame  %.1f Mray/s" %
          (n, min(builds), " ".join("%.1f" % b for b in builds), st["lbvh_depth"], ms, st["rays_total"] / K / ms / 1e3), flush=True)
    ctx.close()
