"""developer tool: digests of every device buffer the build kernels write (rtgo_debug_build_digest: the canonical LBVH, records, frames,
boxes, both fast-walk trees and their meta fields; the whitted records, triangles and grids; then the meta words, the grid image and the
per-mesh infos that capi.Context.read_build returns in the clear), one line per scene -- two builds of the
library (RTGO_HIP_LIB) give the same lines iff they build the same structures.   python tools/build_digest.py [analytic|whitted]"""
import importlib.util, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
from raytracingo_amd import capi, scene as hscene
W, H = 96, 64


def digest(ctx, whitted):
    return " ".join("%016x" % h for h in ctx.build_digest(whitted))


def analytic(name, types, M, mat, aabb, large=False):
    ctx = capi.Context(0)
    try:
        (ctx.set_large_scene if large else ctx.set_scene)(types, M, mat, aabb)
        line = digest(ctx, False)
    except capi.RtgoError as e:   # (a refused scene is a result too: both builds must refuse it alike)
        line = str(e)
    print("analytic %-28s n %3d boxes %-6s %s" % (name, len(types), "given" if aabb is not None else "own", line), flush=True)
    ctx.close()


def capacity_scene(seed, n):
    """n primitives of all four types under random translate * rotate * scale, float32 throughout"""
    rng = np.random.RandomState(seed)
    M = np.zeros((n, 16), np.float32)
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        A = np.eye(4)
        A[:3, :3] = q @ np.diag(rng.uniform(0.2, 1.5, 3))
        A[:3, 3] = rng.uniform(-20.0, 20.0, 3)
        M[k] = A.astype(np.float32).reshape(16)
    mat = np.zeros((n, 10), np.float32)
    mat[:, 0:3] = rng.uniform(0.1, 1.0, (n, 3))
    mat[:, 6] = 1.0
    return np.arange(n) % 4, M, mat


def main(ONLY):
    if ONLY != "whitted":
        import oracle_py as O
        O.build(); O.lib()
        spec = importlib.util.spec_from_file_location("tg", os.path.join(ROOT, "tests", "test_gpu_parity.py"))
        tg = importlib.util.module_from_spec(spec); spec.loader.exec_module(tg)
        for name in ["cornell", "slide", "mirror_spheres", "plateau", "window", "checkered", "balls", "soft_mirrors"]:
            t = hscene.tables(name, W, H)
            for bb in (t["aabb"], None):
                analytic(name, t["type"], t["M"], t["mat"], bb)
        t = hscene.tables("slide", W, H)
        for k in (1, 2, 7):
            analytic("slide[:%d]" % k, t["type"][:k], t["M"][:k], t["mat"][:k], None)
        for seed in range(100, 112):
            _, t = tg._random_scene(O, seed, W, H)
            analytic("random %d" % seed, t["type"], t["M"], t["mat"], None if seed % 2 else t["aabb"])
        for seed in range(100, 112):
            _, t = tg._box_scene(O, seed, W, H, (1, 6, 40)[seed % 3], bool(seed & 1), bool(seed & 2))
            analytic("boxes %d" % seed, t["type"], t["M"], t["mat"], None if (seed // 3) % 2 else t["aabb"])
        analytic("capacity", *capacity_scene(7, 512), None)
        analytic("large 8193", *capacity_scene(7, 8193), None, large=True)   # (kRadixTile = 8192: the first size with two radix tiles)

    if ONLY != "analytic":
        import whitted_scene, whitted_instances as WI, whitted_big_meshes as BM

        def whitted(name, setup):
            ctx = capi.Context(0)
            t0 = time.perf_counter()
            setup(ctx)
            print("whitted  %-28s set up in %.1f ms" % (name, 1e3 * (time.perf_counter() - t0)), file=sys.stderr, flush=True)   # (stderr: the lines compare)
            print("whitted  %-28s %s" % (name, digest(ctx, True)), flush=True)
            ctx.close()

        def mesh_setup(m):
            return lambda ctx: ctx.whitted_set_mesh(m["positions"], m.get("normals"), m["indices"], m.get("tri_material"), m["materials"])

        whitted("mesh", mesh_setup(whitted_scene.build(n_lat=40, n_lon=48)))
        whitted("waterbottle", mesh_setup(whitted_scene.waterbottle()))
        whitted("textured_quad", mesh_setup(whitted_scene.textured_quad()))
        meshes, inst = WI.tori_scene()
        whitted("tori", lambda ctx: ctx.whitted_set_scene(meshes, inst, WI.materials()))
        whitted("clustered", lambda ctx: ctx.whitted_set_scene([BM.displaced_torus(200, 100)], [(WI.transform(np.eye(3), [0, 1, 0]), 0, 0)], WI.materials()))
        # just over kMaxTriangles: 8320 triangles, three clusters, a mid level of one leaf without records
        whitted("clustered 8320", lambda ctx: ctx.whitted_set_scene([BM.displaced_torus(65, 64)], [(WI.transform(np.eye(3), [0, 1, 0]), 0, 0)], WI.materials()))
        # test_whitted_coincident_triangles' mesh: every split of the surface-area sweep ties
        base = np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.5, 0.0]], np.float32)
        extra = np.array([[-2.0, 0.0, -1.0], [2.0, 0.0, -1.0], [0.0, 2.5, -1.0], [-0.5, 0.2, 0.5], [0.5, 0.2, 0.5], [0.0, 0.9, 0.5]], np.float32)
        idx = np.array([[0, 1, 2]] * 200 + [[3, 4, 5], [6, 7, 8]], np.uint32)
        whitted("coincident", mesh_setup({"positions": np.concatenate([base, extra]), "indices": idx, "tri_material": (np.arange(len(idx)) % 2).astype(np.uint32),
                                          "materials": np.array([[0.7, 0.3, 0.2, 1, 0.0, 0.5], [0.2, 0.6, 0.8, 1, 0.3, 0.4]], np.float32)}))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "")
