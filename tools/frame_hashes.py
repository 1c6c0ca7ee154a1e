"""developer tool: a hash of the accumulation buffer after a few progressive frames of every scene x mode, one line each -- two builds of
the library (RTGO_HIP_LIB) give the same lines iff they give the same pixels.   python tools/frame_hashes.py [W] [H] [N] [frames] [whitted]
(whitted: the whitted cases alone)"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
from raytracingo_amd import capi, scene as hscene
W = int(sys.argv[1]) if len(sys.argv) > 1 else 1920
H = int(sys.argv[2]) if len(sys.argv) > 2 else 1080
N = int(sys.argv[3]) if len(sys.argv) > 3 else 4
F = int(sys.argv[4]) if len(sys.argv) > 4 else 3
ANALYTIC = ["cornell", "slide", "mirror_spheres", "plateau", "window", "checkered", "balls", "soft_mirrors"]
for name in ANALYTIC if sys.argv[5:6] != ["whitted"] else []:
    t = hscene.tables(name, W, H)
    for mode in ("path", "distributed", "ambient"):
        for stats in (False, True):
            ctx = capi.Context(0)
            ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"]); ctx.set_camera(t["cam"][0:3], t["cam"][3:6], t["cam"][6:9], t["cam"][9:12])
            ctx.set_background(t["bg"]); ctx.set_lights(t["lights"]); ctx.resize(W * H)
            for f in range(F):
                ctx.launch(capi.make_frame(W, H, N, f, mode == "path", mode == "ambient", stats=stats))
            ctx.sync()
            acc = ctx.read_accum(H, W)
            print("%-14s %-11s %-9s %dx%d N=%d x%d  %s  rays %d" % (name, mode, "canonical" if stats else "fast", W, H, N, F,
                  hashlib.sha1(np.ascontiguousarray(acc).tobytes()).hexdigest()[:16], ctx.stats()["rays_total"]), flush=True)
            ctx.close()

# the whitted triangle path: one mesh under each LDS residency, textured meshes, instanced and clustered scenes, one row band.  A line
# hashes the accumulation buffer and the image of the launch's share after F subframes, beside the two ray counters.
sys.path.insert(0, os.path.join(ROOT, "tests"))
import whitted_scene, whitted_instances as WI, whitted_big_meshes as BM
eye, look, up, fov = np.array([0.5, 3.0, 7.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 1.0, 0.0]), 45.0
Wv = look - eye
U = np.cross(Wv, up); U /= np.linalg.norm(U)
V = np.cross(U, Wv); V /= np.linalg.norm(V)
vlen = np.linalg.norm(Wv) * np.tan(0.5 * np.radians(fov))
V *= vlen; U *= vlen * W / H


def whitted_case(name, mode, setup, extra, bands=(4, 1, 0)):
    os.environ["RTGO_WHITTED_MODE"] = mode
    ctx = capi.Context(0)
    setup(ctx)
    for mi, (bc, mr, nm) in (extra.get("textures") or {}).items():
        ctx.whitted_set_material_textures(mi, bc, mr, nm)
    ctx.whitted_set_lights(extra["lights"]); ctx.whitted_set_miss_color(extra["miss"])
    ctx.set_camera(eye.astype(np.float32), U.astype(np.float32), V.astype(np.float32), Wv.astype(np.float32)); ctx.resize(W * H)
    for sf in range(F):
        ctx.whitted_launch_frame(capi.make_whitted_frame(W, H, sf, bands=bands))
    ctx.sync()
    rows = capi.load().rtgo_local_rows(H, *bands)
    hsh = hashlib.sha1(np.ascontiguousarray(ctx.read_accum(rows, W)).tobytes() + np.ascontiguousarray(ctx.read_image(rows, W)).tobytes())
    st = ctx.stats()
    print("whitted %-22s mode %s %dx%d x%d  %s  rays %d occlusion %d" % (name, mode, W, H, F, hsh.hexdigest()[:16], st["rays_total"],
          st["rays_occlusion"]), flush=True)
    ctx.close()


def mesh_setup(m):
    def setup(ctx):
        ctx.whitted_set_mesh(m["positions"], m.get("normals"), m["indices"], m.get("tri_material"), m["materials"])
        if m.get("texcoords") is not None:
            ctx.whitted_set_texcoords(m["texcoords"])
    return setup


def scene_setup(meshes, inst, mats):
    return lambda ctx: ctx.whitted_set_scene(meshes, inst, mats)


mesh = whitted_scene.build(n_lat=40, n_lon=48)
for mode in ("2", "1", "0"):
    whitted_case("mesh", mode, mesh_setup(mesh), mesh)
for name, m in (("waterbottle", whitted_scene.waterbottle()), ("textured_quad", whitted_scene.textured_quad())):
    whitted_case(name, "2", mesh_setup(m), m)
meshes, inst = WI.tori_scene()
for mode in ("2", "0"):   # the top level in LDS / in L2
    whitted_case("tori", mode, scene_setup(meshes, inst, WI.materials()), WI.lights())
whitted_case("clustered", "2", scene_setup([BM.displaced_torus(200, 100)], [(WI.transform(np.eye(3), [0, 1, 0]), 0, 0)], WI.materials()), WI.lights())
whitted_case("mesh band 1 of 3", "2", mesh_setup(mesh), mesh, bands=(4, 3, 1))
