"""developer tool: rtgo_whitted_set_instances_device against rtgo_whitted_set_instances, and what a refitted top level costs a frame
   python tools/whitted_instances_perf.py [rounds] [W] [H]

tools/whitted_inst_perf.py field's scene -- instances of a 1120-triangle torus on a grid over a ground -- at 1024 and at 8192
instances, the instances held as a device tensor (capi.instances_tensor's layout).

  1. time per call, a host clock around the synchronous calls, the three alternating in one process, every shape warmed up first;
     median and spread (min .. max) over `rounds` (default 30, at least 20) rounds:
       host      the tensor copied to the host (what a caller whose transforms are a tensor pays first), then rtgo_whitted_set_instances
       rebuild   rtgo_whitted_set_instances_device, RTGO_UPDATE_REBUILD
       refit     rtgo_whitted_set_instances_device, RTGO_UPDATE_REFIT (the other of two jittered sets each round: the boxes do move)
       async     rtgo_whitted_refit_instances_device_async on the same sets: the host time of the call (nothing is waited for), and
                 beside it the device time of what it enqueued, between two events on the context's stream
  2. ms per W x H frame (default 1920 x 1080, the mean of 20 subframes, launch times from the context's events) after a REFIT and after
     a REBUILD with the same instances, the tree built over the base layout before each: a mild jitter of the translations, and the
     transforms permuted among the instances (far moves: what a refit cannot keep is the tree's quality).
  3. a frame loop, `LOOP` iterations of "torch writes the tensor, refit, rtgo_whitted_launch at W x H" on one stream, timed from the
     first write to the end of the last frame: frames per second with the synchronous REFIT and with the asynchronous one, the two
     alternating, every shape warmed up first; median and spread over `rounds` loops each.
The context runs on a torch side stream throughout (rtgo_set_stream), so that the events and the tensor writes share its order.
Prints a table and one JSON line."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import whitted_instances as WI
from raytracingo_amd import capi

ROUNDS = max(int(sys.argv[1]) if len(sys.argv) > 1 else 30, 20)
W = int(sys.argv[2]) if len(sys.argv) > 2 else 1920
H = int(sys.argv[3]) if len(sys.argv) > 3 else 1080
LOOP = 20
MATS = np.array([[0.8, 0.8, 0.75, 1.0, 0.0, 0.9], [0.9, 0.25, 0.2, 1.0, 0.1, 0.35], [0.95, 0.8, 0.3, 1.0, 1.0, 0.25]], np.float32)


def frame(eye, look, fov=50.0):
    eye, look, up = np.array(eye, float), np.array(look, float), np.array([0.0, 1.0, 0.0])
    Wv = look - eye
    U = np.cross(Wv, up); U /= np.linalg.norm(U)
    V = np.cross(U, Wv); V /= np.linalg.norm(V)
    vlen = np.linalg.norm(Wv) * np.tan(0.5 * np.radians(fov))
    return [a.astype(np.float32) for a in (eye, U * vlen * W / H, V * vlen, Wv)]


def field(n):
    """the ground (instance 0) and n - 1 tori on a square grid, one unit apart"""
    side = int(np.ceil(np.sqrt(n - 1)))
    half = 0.5 * side
    meshes = [WI.torus(n_u=40, n_v=14, R=0.35, r=0.12), WI.ground(half + 4.0, normals=True)]
    rng = np.random.RandomState(5)
    inst = [(np.eye(3, 4, dtype=np.float32), 1, 0)]
    for k in range(n - 1):
        inst.append((WI.transform(WI.rotation(rng), [-half + 1.0 * (k % side), 0.5, -half + 1.0 * (k // side)]), 0, 1))
    return meshes, inst, frame([0.0, 0.28 * side, 0.62 * side], [0.0, 0.0, -0.06 * side])


def pack(inst):
    tr = torch.from_numpy(np.stack([np.asarray(t, np.float32).reshape(12) for t, _, _ in inst])).cuda()
    return capi.instances_tensor(tr, torch.tensor([m for _, m, _ in inst], device="cuda"), torch.tensor([o for _, _, o in inst], device="cuda"))


def jittered(t, seed, sigma=0.05):
    out = t.clone()
    g = torch.Generator(device="cuda").manual_seed(seed)
    out[1:, [3, 7, 11]] += sigma * torch.randn((t.shape[0] - 1, 3), device="cuda", generator=g)
    return out


def permuted(t, seed):
    out = t.clone()
    g = torch.Generator(device="cuda").manual_seed(seed)
    out[1:, :12] = t[1:, :12][torch.randperm(t.shape[0] - 1, device="cuda", generator=g)]
    return out


def frame_ms(ctx, K=20):
    for sf in range(3):
        ctx.whitted_launch(W, H, sf)
    ctx.sync()
    ctx.reset_stats()
    for sf in range(K):
        ctx.whitted_launch(W, H, 3 + sf)
    ctx.sync()
    return ctx.stats()["total_launch_ms"] / K


def host_call(ctx, t):
    """the tensor to the host, then the host call on those bytes (no repacking: the tensor has the struct's layout)"""
    a = t.cpu().numpy()
    rc = ctx._lib.rtgo_whitted_set_instances(ctx._h, C.cast(a.ctypes.data, C.POINTER(capi.WhittedInstance)), a.shape[0])
    assert rc == 0, rc


def loop_fps(ctx, stream, cur, sets, asynchronous):
    """LOOP frames of write, refit, launch on `stream`: frames per second, the final wait included"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        for i in range(LOOP):
            cur.copy_(sets[i % 2])
            if asynchronous:
                ctx.whitted_refit_instances_device_async(cur)
            else:
                ctx.whitted_set_instances_device(cur, refit=True)
            ctx.whitted_launch(W, H, i)
    ctx.sync()
    return LOOP / (time.perf_counter() - t0)


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms[0]), "max_ms": float(ms[-1])}


result = {"rounds": ROUNDS, "frame": [W, H], "sizes": {}}
for n in (1024, 8192):
    meshes, inst, cam = field(n)
    ctx = capi.Context(0)
    ctx.whitted_set_scene(meshes, inst, MATS)
    lights = np.zeros((2, 8), dtype=np.float32)
    lights[0] = [1.0, 0.95, 0.9, 2.5, 4.0, 12.0, 6.0, 0]
    lights[1] = [0.6, 0.7, 1.0, 1.2, -8.0, 8.0, -4.0, 0]
    ctx.whitted_set_lights(lights)
    ctx.whitted_set_miss_color(np.array([0.1, 0.15, 0.25], np.float32))
    ctx.set_camera(*cam)
    ctx.resize(W * H)
    base = pack(inst)
    sets = [jittered(base, 1), jittered(base, 2)]
    far = permuted(base, 3)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = {"host": lambda r: host_call(ctx, sets[r % 2]),
             "rebuild": lambda r: ctx.whitted_set_instances_device(sets[r % 2]),
             "refit": lambda r: ctx.whitted_set_instances_device(sets[(r + 1) % 2], refit=True),
             "async": lambda r: ctx.whitted_refit_instances_device_async(sets[r % 2])}
    times = {k: [] for k in calls}
    device = []
    for r in range(3 + ROUNDS):   # the first three rounds warm every shape up
        for k, call in calls.items():
            if k == "async":
                e0.record(stream)
            t0 = time.perf_counter()
            call(r)
            dt = 1e3 * (time.perf_counter() - t0)
            if k == "async":
                e1.record(stream)
                e1.synchronize()
            if r >= 3:
                times[k].append(dt)
                if k == "async":
                    device.append(e0.elapsed_time(e1))
    row = {"calls": {k: stats(v) for k, v in times.items()}, "frames": {}}
    row["calls"]["async, on the device"] = stats(device)
    cur = sets[0].clone()
    fps = {"refit": [], "async": []}
    for r in range(3 + ROUNDS):
        for k in fps:
            f = loop_fps(ctx, stream, cur, sets, k == "async")
            if r >= 3:
                fps[k].append(f)
    row["loop_fps"] = {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in fps.items()}
    ctx.whitted_set_instances_device(base)
    row["frames"]["base"] = frame_ms(ctx)
    for what, new in (("jitter", sets[0]), ("permuted", far)):
        ctx.whitted_set_instances_device(base)
        ctx.whitted_set_instances_device(new, refit=True)
        refit_ms = frame_ms(ctx)
        ctx.whitted_set_instances_device(new)
        row["frames"][what] = {"refit_ms": refit_ms, "rebuild_ms": frame_ms(ctx)}
    ctx.close()
    result["sizes"][str(n)] = row
    print("%d instances, per call (median of %d, min .. max):" % (n, ROUNDS))
    for k, s in row["calls"].items():
        print("  %-20s %8.3f ms  (%.3f .. %.3f)" % (k, s["median_ms"], s["min_ms"], s["max_ms"]))
    for k, s in row["loop_fps"].items():
        print("  loop of %d frames, %-6s %8.1f frames/s  (%.1f .. %.1f)" % (LOOP, k, s["median"], s["min"], s["max"]))
    print("  %d x %d frame: base %.3f ms" % (W, H, row["frames"]["base"]))
    for what in ("jitter", "permuted"):
        f = row["frames"][what]
        print("  after %-8s refit %.3f ms, rebuild %.3f ms  (refit / rebuild %.2f)" % (what, f["refit_ms"], f["rebuild_ms"], f["refit_ms"] / f["rebuild_ms"]))
print(json.dumps(result))
