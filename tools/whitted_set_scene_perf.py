"""developer tool: rtgo_whitted_set_scene_device against rtgo_whitted_set_scene
   python tools/whitted_set_scene_perf.py [rounds]

Two scenes: one clustered mesh of 1 000 000 triangles (tools/whitted_rebuild_perf.py's displaced torus, with normals) under one
instance, and 256 meshes of 256 triangles (tori with normals and materials) under one instance each.  The data is resident before the
timing starts -- numpy arrays for the host call, device tensors for the device call -- and the rtgo_whitted_mesh tables are made once,
so a round times the C call alone: a host clock around the synchronous call, a device synchronise at both ends.  The calls alternate in
one process, two warm-up rounds first; median and range (min .. max) over `rounds` (default 12, at least 10):

  host         rtgo_whitted_set_scene on the numpy arrays
  device       rtgo_whitted_set_scene_device on the tensors
  copy + host  the tensors copied to the host first (what a caller whose mesh is a tensor pays today), then the host call

Prints a table and one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import whitted_big_meshes as BM
import whitted_instances as WI
from raytracingo_amd import capi

ROUNDS = max(int(sys.argv[1]) if len(sys.argv) > 1 else 12, 10)
ARRAYS = ("positions", "normals", "texcoords", "indices", "tri_material")
EYE = np.eye(3, 4, dtype=np.float32)


def scenes():
    big = BM.displaced_torus(1000, 500, R=1.0, r=0.35, amp=0.04, freq=(23, 11), texcoords=False)   # 1 000 000 triangles
    yield "1 mesh of 1 000 000 triangles", [big], [(EYE, 0, 0)]
    small = []
    for k in range(256):
        t = WI.torus(16, 8)
        small.append(dict(t, positions=(t["positions"] * np.float32(0.5 + 0.002 * k)).astype(np.float32)))
    yield "256 meshes of 256 triangles", small, [(WI.transform(np.eye(3), [1.5 * (k % 16), 0.0, 1.5 * (k // 16)]), k, k % 3) for k in range(256)]


def host_arrays(meshes):
    return [{k: None if m.get(k) is None else np.ascontiguousarray(m[k], np.float32 if k in ARRAYS[:3] else np.uint32) for k in ARRAYS} for m in meshes]


def table(arrays, ptr):
    ms = (capi.WhittedMesh * len(arrays))()
    for k, m in enumerate(arrays):
        p = [None if m[name] is None else ptr(m[name]) for name in ARRAYS]
        ms[k] = capi.WhittedMesh(p[0], p[1], p[2], len(m["positions"]), p[3], p[4], len(m["indices"]))
    return ms


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms[0]), "max_ms": float(ms[-1])}


result = {"rounds": ROUNDS, "scenes": {}}
mats = WI.materials()
for name, meshes, inst in scenes():
    ctx = capi.Context(0)
    L = ctx._lib
    host = host_arrays(meshes)
    dev = [{k: None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for k, a in m.items()} for m in host]
    torch.cuda.synchronize()
    host_table, dev_table = table(host, lambda a: a.ctypes.data), table(dev, lambda t: t.data_ptr())
    arr = capi.whitted_instances(inst)
    n = len(meshes)

    def host_call(ms=host_table):
        assert L.rtgo_whitted_set_scene(ctx._h, ms, n, arr, len(inst), mats.ctypes.data, len(mats)) == 0, L.rtgo_last_error(ctx._h)

    def device_call():
        assert L.rtgo_whitted_set_scene_device(ctx._h, dev_table, n, arr, len(inst), mats.ctypes.data, len(mats)) == 0, L.rtgo_last_error(ctx._h)

    def copy_then_host():
        down = [{k: None if t is None else t.cpu().numpy() for k, t in m.items()} for m in dev]
        host_call(table(down, lambda a: a.ctypes.data))

    calls = {"host": host_call, "device": device_call, "copy + host": copy_then_host}
    times = {k: [] for k in calls}
    digests = {}
    for r in range(2 + ROUNDS):
        for k, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
            if r >= 2:
                times[k].append(dt)
            elif r == 0:
                digests[k] = list(ctx.build_digest(True))
    assert digests["device"] == digests["host"] == digests["copy + host"], "the calls built different scenes"
    ctx.close()
    nbytes = sum(a.nbytes for m in host for a in m.values() if a is not None)
    row = {"mesh_bytes": nbytes, "calls": {k: stats(v) for k, v in times.items()}}
    result["scenes"][name] = row
    print("%s (%.1f MB of mesh data), per call (median of %d, min .. max):" % (name, nbytes / 1e6, ROUNDS))
    for k, s in row["calls"].items():
        print("  %-12s %8.3f ms  (%.3f .. %.3f)" % (k, s["median_ms"], s["min_ms"], s["max_ms"]))
    print("  host - device: %.3f ms" % (row["calls"]["host"]["median_ms"] - row["calls"]["device"]["median_ms"]))
print(json.dumps(result))
