"""developer tool: what a refit (rtgo_whitted_update_mesh, rtgo_whitted_update_meshes) costs and what it does to the walk, against setting the mesh again
   python tools/whitted_refit_perf.py [W] [H]        single meshes up to 8192 triangles, rtgo_whitted_update_mesh against rtgo_whitted_set_mesh
   python tools/whitted_refit_perf.py big [W] [H]    tools/whitted_inst_perf.py big's 1 000 000-triangle displaced torus (a clustered mesh) on a ground:
                                                     rtgo_whitted_update_meshes against rtgo_whitted_set_scene over the same vertices, subframe time of the
                                                     refitted scene against the fresh one (smooth, twist); and a batch of k meshes against k calls of
                                                     rtgo_whitted_update_mesh on a field of 1024 tori drawn from k meshes; and
                                                     rtgo_whitted_update_meshes_device (the same vertices as torch device tensors) beside its host
                                                     twins, refit and rebuild, on both scenes, in the same process
Per mesh and deformation, medians of repeated calls after a warm-up:
   update    ms of rtgo_whitted_update_mesh (synchronous: wall time of the call)
   set_mesh  ms of rtgo_whitted_set_mesh over the same new vertices
   subframe  ms per subframe of the mesh as built, of the refitted mesh, and of a fresh build over the new vertices
A refitted tree keeps a topology chosen for the old vertices, so it walks worse than a rebuilt one: refit/fresh is that price.
Deformations: `smooth` (a sine displacement along the normals, 3 % of the extent), `twist` (a turn about the y axis that grows with height
to 180 degrees) and `shuffle` (vertex positions permuted: the worst a refit can meet)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import time
import numpy as np
import whitted_scene
import whitted_instances as WI
import whitted_big_meshes as BM
from raytracingo_amd import capi

BIG = len(sys.argv) > 1 and sys.argv[1] == "big"
ARGS = sys.argv[2:] if BIG else sys.argv[1:]
W = int(ARGS[0]) if len(ARGS) > 0 else 1920
H = int(ARGS[1]) if len(ARGS) > 1 else 1080
WARM, REPS = 3, 15


def frame(eye, look, fov=45.0):
    eye, look, up = np.array(eye, float), np.array(look, float), np.array([0.0, 1.0, 0.0])
    Wv = look - eye
    U = np.cross(Wv, up); U /= np.linalg.norm(U)
    V = np.cross(U, Wv); V /= np.linalg.norm(V)
    vlen = np.linalg.norm(Wv) * np.tan(0.5 * np.radians(fov))
    return [a.astype(np.float32) for a in (eye, U * vlen * W / H, V * vlen, Wv)]


def median_ms(call):
    for _ in range(WARM):
        call()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def subframe_ms(ctx, K=20, rounds=5):
    for sf in range(3):
        ctx.whitted_launch(W, H, sf)
    ctx.sync()
    out = []
    for _ in range(rounds):
        ctx.reset_stats()
        for sf in range(K):
            ctx.whitted_launch(W, H, 3 + sf)
        ctx.sync()
        out.append(ctx.stats()["total_launch_ms"] / K)
    return float(np.median(out))


def set_mesh(ctx, mesh, positions):
    ctx.whitted_set_mesh(positions, mesh.get("normals"), mesh["indices"], mesh.get("tri_material"), mesh["materials"])


def deformations(mesh):
    p = mesh["positions"].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    ext = float((hi - lo).max())
    n = mesh["normals"].astype(np.float64) if mesh.get("normals") is not None else np.tile([0.0, 1.0, 0.0], (len(p), 1))
    k = 12.0 / ext
    smooth = p + (0.03 * ext * np.sin(k * (p[:, 0] + 0.7 * p[:, 2]) + 0.5 * k * p[:, 1]))[:, None] * n
    c = 0.5 * (lo + hi)
    a = np.pi * (p[:, 1] - lo[1]) / max(hi[1] - lo[1], 1e-9)
    q = p - c
    twist = np.stack([np.cos(a) * q[:, 0] + np.sin(a) * q[:, 2], q[:, 1], -np.sin(a) * q[:, 0] + np.cos(a) * q[:, 2]], axis=1) + c
    shuffle = p[np.random.RandomState(1).permutation(len(p))]
    return [("smooth", smooth.astype(np.float32)), ("twist", twist.astype(np.float32)), ("shuffle", shuffle.astype(np.float32))]


def view(ctx, lights, miss, cam):
    ctx.whitted_set_lights(lights)
    ctx.whitted_set_miss_color(miss)
    ctx.set_camera(*cam)
    ctx.resize(W * H)


def device_against_host(ctx, what, updates):
    """the synchronous calls over the same vertices: from host arrays (update_meshes, rebuild_meshes) and from device tensors"""
    import torch
    on_device = [(m, torch.from_numpy(q).cuda(), None if n is None else torch.from_numpy(n).cuda()) for m, q, n in updates]
    torch.cuda.synchronize()
    for rebuild, host in ((False, ctx.whitted_update_meshes), (True, ctx.whitted_rebuild_meshes)):
        t_host = median_ms(lambda: host(updates))
        t_dev = median_ms(lambda: ctx.whitted_update_meshes_device(on_device, rebuild=rebuild))
        print("%s, %s: %-22s %8.3f ms   update_meshes_device %8.3f ms   host/device %5.2fx" %
              (what, "rebuild" if rebuild else "refit", host.__name__[len("whitted_"):], t_host, t_dev, t_host / t_dev))


def big_mode():
    import torch
    torch.cuda.init()   # torch's HIP runtime up before the first context: device_against_host hands the library torch tensors
    eye34 = np.eye(3, 4, dtype=np.float32)
    big = BM.displaced_torus(1000, 500, R=1.0, r=0.35, amp=0.04, freq=(23, 11), texcoords=False)   # 1 000 000 triangles
    meshes, inst, mats, lt = [WI.ground(4.0, -0.5, normals=True), big], [(eye34, 0, 0), (eye34, 1, 1)], WI.materials(), WI.lights()
    cam = frame([0.4, 1.6, 2.6], [0.0, -0.1, 0.0])
    p = big["positions"]
    print("whitted refit of a clustered mesh, %d x %d, medians of %d after %d warm-up calls" % (W, H, REPS, WARM))
    ctx = capi.Context(0)
    ctx.whitted_set_scene(meshes, inst, mats)
    view(ctx, lt["lights"], lt["miss"], cam)
    print("%d triangles  %d vertices  as built %.3f ms/subframe" % (len(big["indices"]), len(p), subframe_ms(ctx)))
    for k, (what, q) in enumerate(deformations(big)[:2]):
        ctx.whitted_update_meshes([(1, p, None)])
        t_update = median_ms(lambda: ctx.whitted_update_meshes([(1, q, None)]))
        refit = subframe_ms(ctx)
        moved = [meshes[0], dict(big, positions=q)]
        if k == 0:
            t_set = median_ms(lambda: ctx.whitted_set_scene(moved, inst, mats))
        else:
            ctx.whitted_set_scene(moved, inst, mats)
        fresh = subframe_ms(ctx)
        print("    %-8s update_meshes %8.3f ms   set_scene %9.3f ms   set_scene/update_meshes %6.1fx   subframe refit %.3f ms  fresh %.3f ms  refit/fresh %.3f" %
              (what, t_update, t_set, t_set / t_update, refit, fresh, refit / fresh))
        ctx.whitted_set_scene(meshes, inst, mats)
    device_against_host(ctx, "%d triangles, one clustered mesh" % len(big["indices"]), [(1, deformations(big)[0][1], None)])
    ctx.close()
    # a field of 1024 tori drawn from K meshes: all K moved by one call against one call each
    K = 16
    tor = WI.torus(n_u=40, n_v=14, R=0.35, r=0.12)
    meshes = [WI.ground(20.0, normals=True)] + [dict(tor) for _ in range(K)]
    rng = np.random.RandomState(5)
    inst = [(eye34, 0, 0)] + [(WI.transform(WI.rotation(rng), [-16.0 + 1.0 * (k % 32), 0.5, -16.0 + 1.0 * (k // 32)]), 1 + k % K, 1) for k in range(1024)]
    ctx = capi.Context(0)
    ctx.whitted_set_scene(meshes, inst, mats)
    grown = [(1 + k, tor["positions"] * np.float32(1.0 + 0.02 * k), None) for k in range(K)]
    t_batch = median_ms(lambda: ctx.whitted_update_meshes(grown))
    t_single = median_ms(lambda: [ctx.whitted_update_mesh(m, q) for m, q, _ in grown])
    t_set = median_ms(lambda: ctx.whitted_set_scene(meshes, inst, mats))
    print("1024 tori of %d triangles drawn from %d meshes: update_meshes over all %d %.3f ms   %d calls of update_mesh %.3f ms   single/batch %.1fx   set_scene %.3f ms" %
          (len(tor["indices"]), K, K, t_batch, K, t_single, t_single / t_batch, t_set))
    device_against_host(ctx, "%d meshes of %d triangles in one call" % (K, len(tor["indices"])), grown)
    ctx.close()


if BIG:
    big_mode()
else:
    torus = BM.displaced_torus(64, 64, texcoords=False)
    torus.update(materials=WI.materials(), **WI.lights())
    MESHES = [("scene 342", whitted_scene.build()), ("scene 3758", whitted_scene.build(n_lat=40, n_lon=48)), ("waterbottle", whitted_scene.waterbottle()),
              ("torus 8192", torus)]

    print("whitted refit, %d x %d, medians of %d after %d warm-up calls" % (W, H, REPS, WARM))
    for name, mesh in MESHES:
        p = mesh["positions"]
        lo, hi = p.min(0), p.max(0)
        c, ext = 0.5 * (lo + hi), float((hi - lo).max())
        cam = frame(c + ext * np.array([0.08, 0.45, 1.1]), c)
        ctx = capi.Context(0)
        set_mesh(ctx, mesh, p)
        ctx.whitted_set_lights(mesh["lights"])
        ctx.whitted_set_miss_color(mesh["miss"])
        ctx.set_camera(*cam)
        ctx.resize(W * H)
        built = subframe_ms(ctx)
        print("%-12s %5d triangles  %5d vertices  as built %.3f ms/subframe" % (name, len(mesh["indices"]), len(p), built))
        for what, q in deformations(mesh):
            set_mesh(ctx, mesh, p)
            t_update = median_ms(lambda: ctx.whitted_update_mesh(0, q))
            refit = subframe_ms(ctx)
            t_set = median_ms(lambda: set_mesh(ctx, mesh, q))
            fresh = subframe_ms(ctx)
            print("    %-8s update %7.3f ms   set_mesh %7.3f ms   set_mesh/update %5.1fx   subframe refit %.3f ms  fresh %.3f ms  refit/fresh %.3f" %
                  (what, t_update, t_set, t_set / t_update, refit, fresh, refit / fresh))
        ctx.close()
