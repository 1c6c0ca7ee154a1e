"""developer tool: time the whitted path over instanced meshes (rtgo_whitted_set_scene)
   python tools/whitted_inst_perf.py one [W] [H]     one identity instance of tests/whitted_scene.build(40, 48) (3758 triangles) against
                                                     rtgo_whitted_set_mesh on the same mesh
   python tools/whitted_inst_perf.py field [W] [H]   1024 instances of a 1120-triangle torus (1.15 M triangles) on a ground
   python tools/whitted_inst_perf.py big [W] [H]     a 1 M-triangle displaced torus on a ground: one clustered instance against the caller's
                                                     cut into contiguous 8192-triangle identity instances; set_scene wall time at 1 M and 4 M"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import whitted_scene
import whitted_instances as WI
import whitted_big_meshes as BM
import time
from raytracingo_amd import capi

what = sys.argv[1] if len(sys.argv) > 1 else "one"
W = int(sys.argv[2]) if len(sys.argv) > 2 else 1920
H = int(sys.argv[3]) if len(sys.argv) > 3 else 1080


def frame(eye, look, fov=45.0):
    # pinhole frame like sutil::Camera::UVWFrame (float64 here: a timing tool, not a parity test)
    eye, look, up = np.array(eye, float), np.array(look, float), np.array([0.0, 1.0, 0.0])
    Wv = look - eye
    U = np.cross(Wv, up); U /= np.linalg.norm(U)
    V = np.cross(U, Wv); V /= np.linalg.norm(V)
    vlen = np.linalg.norm(Wv) * np.tan(0.5 * np.radians(fov))
    return [a.astype(np.float32) for a in (eye, U * vlen * W / H, V * vlen, Wv)]


def time_ctx(ctx, lights, miss, cam, K=20):
    ctx.whitted_set_lights(lights)
    ctx.whitted_set_miss_color(miss)
    ctx.set_camera(*cam)
    ctx.resize(W * H)
    for sf in range(3):
        ctx.whitted_launch(W, H, sf)
    ctx.sync()
    ctx.reset_stats()
    for sf in range(K):
        ctx.whitted_launch(W, H, 3 + sf)
    ctx.sync()
    st = ctx.stats()
    ms = st["total_launch_ms"] / K
    return ms, st["rays_total"] / K


if what == "one":
    mesh = whitted_scene.build(n_lat=40, n_lon=48)
    cam = frame([0.5, 3.0, 7.0], [0.0, 1.0, 0.0])
    ctx = capi.Context(0)
    ctx.whitted_set_mesh(mesh["positions"], mesh["normals"], mesh["indices"], mesh["tri_material"], mesh["materials"])
    ms1, r1 = time_ctx(ctx, mesh["lights"], mesh["miss"], cam)
    ctx.close()
    ctx = capi.Context(0)
    ctx.whitted_set_scene([mesh], [(np.eye(3, 4, dtype=np.float32), 0, 0)], mesh["materials"])
    ms2, r2 = time_ctx(ctx, mesh["lights"], mesh["miss"], cam)
    print("whitted %dx%d, %d triangles: single mesh %.3f ms (%.0f Mray/s), one identity instance %.3f ms (%.0f Mray/s): %.2fx" %
          (W, H, len(mesh["indices"]), ms1, r1 / ms1 / 1e3, ms2, r2 / ms2 / 1e3, ms2 / ms1))
elif what == "big":
    big = BM.displaced_torus(1000, 500, R=1.0, r=0.35, amp=0.04, freq=(23, 11), texcoords=False)   # 1 000 000 triangles
    meshes = [WI.ground(4.0, -0.5, normals=True), big]
    inst = [(np.eye(3, 4, dtype=np.float32), 0, 0), (np.eye(3, 4, dtype=np.float32), 1, 1)]
    mats = WI.materials()
    lt = WI.lights()
    cam = frame([0.4, 1.6, 2.6], [0.0, -0.1, 0.0], 45.0)
    ctx = capi.Context(0)
    t0 = time.perf_counter()
    ctx.whitted_set_scene(meshes, inst, mats)
    t_big = time.perf_counter() - t0
    ms1, r1 = time_ctx(ctx, lt["lights"], lt["miss"], cam)
    ctx.close()
    cm, ci = BM.chunked_scene(meshes, inst, big={1})
    ctx = capi.Context(0)
    t0 = time.perf_counter()
    ctx.whitted_set_scene(cm, ci, mats)
    t_cut = time.perf_counter() - t0
    ms2, r2 = time_ctx(ctx, lt["lights"], lt["miss"], cam)
    ctx.close()
    print("whitted %dx%d, 1 000 002 triangles: one clustered instance %.3f ms/subframe (%.2f Gray/s, set_scene %.2f s); caller's cut into %d "
          "instances %.3f ms/subframe (%.2f Gray/s, set_scene %.2f s): clustered/cut %.3f" %
          (W, H, ms1, r1 / ms1 / 1e6, t_big, len(ci), ms2, r2 / ms2 / 1e6, t_cut, ms1 / ms2))
    if len(sys.argv) > 4 and sys.argv[4] == "build4m":
        big4 = BM.displaced_torus(2000, 1000, R=1.0, r=0.35, amp=0.04, freq=(23, 11), texcoords=False)
        ctx = capi.Context(0)
        t0 = time.perf_counter()
        ctx.whitted_set_scene([meshes[0], big4], inst, mats)
        print("set_scene of a 4 000 000-triangle mesh: %.2f s" % (time.perf_counter() - t0))
        ctx.close()
else:
    tor = WI.torus(n_u=40, n_v=14, R=0.35, r=0.12)
    meshes = [tor, WI.ground(20.0, normals=True)]
    rng = np.random.RandomState(5)
    inst = [(np.eye(3, 4, dtype=np.float32), 1, 0)]
    for k in range(1024):
        t = [-16.0 + 1.0 * (k % 32), 0.5, -16.0 + 1.0 * (k // 32)]
        inst.append((WI.transform(WI.rotation(rng), t), 0, 1))
    mats = np.array([[0.8, 0.8, 0.75, 1.0, 0.0, 0.9], [0.9, 0.25, 0.2, 1.0, 0.1, 0.35], [0.95, 0.8, 0.3, 1.0, 1.0, 0.25]], np.float32)
    lights = np.zeros((2, 8), dtype=np.float32)
    lights[0] = [1.0, 0.95, 0.9, 2.5, 4.0, 12.0, 6.0, 0]
    lights[1] = [0.6, 0.7, 1.0, 1.2, -8.0, 8.0, -4.0, 0]
    ctx = capi.Context(0)
    ctx.whitted_set_scene(meshes, inst, mats)
    ms, rays = time_ctx(ctx, lights, np.array([0.1, 0.15, 0.25], np.float32), frame([0.0, 9.0, 20.0], [0.0, 0.0, -2.0], 50.0))
    n_tri = len(tor["indices"]) * 1024 + 2
    print("whitted %dx%d, %d instances, %d triangles: %.3f ms/subframe, %.2f Gray/s (%.2f rays per pixel)" %
          (W, H, len(inst), n_tri, ms, rays / ms / 1e6, rays / (W * H)))
