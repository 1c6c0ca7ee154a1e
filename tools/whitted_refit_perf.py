"""developer tool: what a refit (rtgo_whitted_update_mesh) costs and what it does to the walk, against setting the mesh again
   python tools/whitted_refit_perf.py [W] [H]
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

W = int(sys.argv[1]) if len(sys.argv) > 1 else 1920
H = int(sys.argv[2]) if len(sys.argv) > 2 else 1080
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
