"""developer tool: what building a clustered mesh costs -- rtgo_whitted_set_scene through the batched builds against the cluster-by-cluster
loop (RTGO_WHITTED_SEQ_BUILD=1, and the commit before the batched builds), and rtgo_whitted_rebuild_meshes against set_scene and a refit
   python tools/whitted_rebuild_perf.py set_scene [reps]      ms of rtgo_whitted_set_scene over tools/whitted_refit_perf.py big's 1 000 000-triangle
                                                              displaced torus on a ground, one line per call (the environment's knobs apply)
   python tools/whitted_rebuild_perf.py ab PARENT [rounds]    that, in fresh processes, alternating: this tree, the checkout at PARENT (built),
                                                              this tree with RTGO_WHITTED_SEQ_BUILD=1
   python tools/whitted_rebuild_perf.py small [reps]          set_scene of the smallest clustered mesh (8320 triangles), batched and sequential
                                                              alternating in one process, with the sequential path's own spread
   python tools/whitted_rebuild_perf.py rebuild [W] [H]       the 1 000 000-triangle mesh: rebuild_meshes, set_scene, update_meshes (refit); 16 small
                                                              meshes rebuilt by one call, by 16 calls and one after another; subframe time after
                                                              the `twist` deformation: refitted, rebuilt, fresh
RTGO_TREE names the checkout whose package is imported (default: this one).  How a set_scene splits between sort, builds, pack and mid
level is read from a kernel trace of `set_scene 1` (rocprofv3 --kernel-trace --stats)."""
import os, sys
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("RTGO_TREE", HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(HERE, "tests"))
import subprocess
import time
import numpy as np

MODE = sys.argv[1] if len(sys.argv) > 1 else "set_scene"
EYE = np.eye(3, 4, dtype=np.float32)


def big_scene():
    import whitted_big_meshes as BM
    import whitted_instances as WI
    big = BM.displaced_torus(1000, 500, R=1.0, r=0.35, amp=0.04, freq=(23, 11), texcoords=False)   # 1 000 000 triangles
    return [WI.ground(4.0, -0.5, normals=True), big], [(EYE, 0, 0), (EYE, 1, 1)], WI.materials(), WI.lights()


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return "median %9.3f  min %9.3f  max %9.3f ms" % (float(np.median(ts)), min(ts), max(ts))


def set_scene_mode(reps):
    from raytracingo_amd import capi
    meshes, inst, mats, _ = big_scene()
    ctx = capi.Context(0)
    ts = [timed(lambda: ctx.whitted_set_scene(meshes, inst, mats)) for _ in range(reps)]
    for t in ts:
        print("set_scene %10.3f ms" % t)
    ctx.close()


def ab_mode(parent, rounds):
    runs = {"this tree": {}, "parent": {"RTGO_TREE": parent}, "this tree, RTGO_WHITTED_SEQ_BUILD=1": {"RTGO_WHITTED_SEQ_BUILD": "1"}}
    ts = {k: [] for k in runs}
    for r in range(rounds):
        for name, extra in runs.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "set_scene", "2"], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                sys.exit("%s: exit %d\n%s" % (name, out.returncode, out.stderr[-2000:]))
            got = [float(l.split()[1]) for l in out.stdout.splitlines() if l.startswith("set_scene")]
            ts[name].append(got[-1])   # the second call of the process: the first pays for loading the code object
            print("round %d  %-40s first %10.3f  second %10.3f ms" % (r, name, got[0], got[-1]), flush=True)
    for name in runs:
        print("%-40s %s" % (name, stats(ts[name])))
    print("parent / this tree: %.1fx" % (np.median(ts["parent"]) / np.median(ts["this tree"])))


def small_mode(reps):
    from raytracingo_amd import capi
    import whitted_big_meshes as BM
    import whitted_instances as WI
    mesh = BM.displaced_torus(65, 64)
    args = ([mesh], [(EYE, 0, 0)], WI.materials())
    ctx = capi.Context(0)
    ts = {"batched": [], "sequential": []}
    for r in range(reps + 3):
        for name in ts:
            os.environ.pop("RTGO_WHITTED_SEQ_BUILD", None)
            if name == "sequential":
                os.environ["RTGO_WHITTED_SEQ_BUILD"] = "1"
            t = timed(lambda: ctx.whitted_set_scene(*args))
            if r >= 3:
                ts[name].append(t)
    os.environ.pop("RTGO_WHITTED_SEQ_BUILD", None)
    ctx.close()
    for name, t in ts.items():
        print("set_scene, %d triangles, %-10s %s  (%d calls, alternating)" % (len(mesh["indices"]), name, stats(t), len(t)))
    s = np.array(ts["sequential"])
    print("sequential spread: max - min %.3f ms, standard deviation %.3f ms; batched median - sequential median %+.3f ms" %
          (s.max() - s.min(), s.std(), np.median(ts["batched"]) - np.median(s)))


def rebuild_mode(W, H):
    from raytracingo_amd import capi
    import whitted_instances as WI
    meshes, inst, mats, lt = big_scene()
    big = meshes[1]

    def deformations(mesh):   # tools/whitted_refit_perf.py's smooth and twist
        q = mesh["positions"].astype(np.float64)
        lo, hi = q.min(0), q.max(0)
        ext = float((hi - lo).max())
        k = 12.0 / ext
        smooth = q + (0.03 * ext * np.sin(k * (q[:, 0] + 0.7 * q[:, 2]) + 0.5 * k * q[:, 1]))[:, None] * mesh["normals"].astype(np.float64)
        c = 0.5 * (lo + hi)
        a = np.pi * (q[:, 1] - lo[1]) / max(hi[1] - lo[1], 1e-9)
        d = q - c
        twist = np.stack([np.cos(a) * d[:, 0] + np.sin(a) * d[:, 2], d[:, 1], -np.sin(a) * d[:, 0] + np.cos(a) * d[:, 2]], axis=1) + c
        return smooth.astype(np.float32), twist.astype(np.float32)

    def frame(eye, look, fov=45.0):
        eye, look, up = np.array(eye, float), np.array(look, float), np.array([0.0, 1.0, 0.0])
        Wv = look - eye
        U = np.cross(Wv, up); U /= np.linalg.norm(U)
        V = np.cross(U, Wv); V /= np.linalg.norm(V)
        vlen = np.linalg.norm(Wv) * np.tan(0.5 * np.radians(fov))
        return [a.astype(np.float32) for a in (eye, U * vlen * W / H, V * vlen, Wv)]

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
        return float(np.median(out)), min(out), max(out)

    def several(call, reps=7, warm=2):
        return [timed(call) for _ in range(reps + warm)][warm:]

    smooth, twist = deformations(big)
    ctx = capi.Context(0)
    ctx.whitted_set_scene(meshes, inst, mats)
    ctx.whitted_set_lights(lt["lights"])
    ctx.whitted_set_miss_color(lt["miss"])
    ctx.set_camera(*frame([0.4, 1.6, 2.6], [0.0, -0.1, 0.0]))
    ctx.resize(W * H)
    print("%d triangles, %d x %d; as built %.3f ms/subframe (min %.3f max %.3f)" % ((len(big["indices"]), W, H) + subframe_ms(ctx)))
    print("rebuild_meshes  %s" % stats(several(lambda: ctx.whitted_rebuild_meshes([(1, smooth, None)]))))
    print("update_meshes   %s" % stats(several(lambda: ctx.whitted_update_meshes([(1, smooth, None)]))))
    print("set_scene       %s" % stats(several(lambda: ctx.whitted_set_scene([meshes[0], dict(big, positions=smooth)], inst, mats), reps=5, warm=1)))
    ctx.whitted_set_scene(meshes, inst, mats)
    ctx.whitted_update_meshes([(1, twist, None)])
    print("twist: refitted %.3f ms/subframe (min %.3f max %.3f)" % subframe_ms(ctx))
    ctx.whitted_rebuild_meshes([(1, twist, None)])
    print("twist: rebuilt  %.3f ms/subframe (min %.3f max %.3f)" % subframe_ms(ctx))
    ctx.whitted_set_scene([meshes[0], dict(big, positions=twist)], inst, mats)
    print("twist: fresh    %.3f ms/subframe (min %.3f max %.3f)" % subframe_ms(ctx))
    ctx.close()
    # 16 small meshes: one call, 16 calls, one call that builds them one after another
    K = 16
    tor = WI.torus(n_u=40, n_v=14, R=0.35, r=0.12)
    meshes = [WI.ground(20.0, normals=True)] + [dict(tor) for _ in range(K)]
    rng = np.random.RandomState(5)
    inst = [(EYE, 0, 0)] + [(WI.transform(WI.rotation(rng), [-16.0 + 1.0 * (k % 32), 0.5, -16.0 + 1.0 * (k // 32)]), 1 + k % K, 1) for k in range(1024)]
    ctx = capi.Context(0)
    ctx.whitted_set_scene(meshes, inst, mats)
    grown = [(1 + k, tor["positions"] * np.float32(1.0 + 0.02 * k), None) for k in range(K)]
    print("%d meshes of %d triangles under 1024 instances:" % (K, len(tor["indices"])))
    print("  one rebuild_meshes call             %s" % stats(several(lambda: ctx.whitted_rebuild_meshes(grown), reps=15)))
    print("  %d rebuild_meshes calls             %s" % (K, stats(several(lambda: [ctx.whitted_rebuild_meshes([g]) for g in grown], reps=15))))
    os.environ["RTGO_WHITTED_SEQ_BUILD"] = "1"
    print("  one call, RTGO_WHITTED_SEQ_BUILD=1  %s" % stats(several(lambda: ctx.whitted_rebuild_meshes(grown), reps=15)))
    os.environ.pop("RTGO_WHITTED_SEQ_BUILD")
    print("  update_meshes (refit), one call     %s" % stats(several(lambda: ctx.whitted_update_meshes(grown), reps=15)))
    ctx.close()


if MODE == "set_scene":
    set_scene_mode(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
elif MODE == "ab":
    ab_mode(os.path.abspath(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 3)
elif MODE == "small":
    small_mode(int(sys.argv[2]) if len(sys.argv) > 2 else 25)
elif MODE == "rebuild":
    rebuild_mode(int(sys.argv[2]) if len(sys.argv) > 2 else 1920, int(sys.argv[3]) if len(sys.argv) > 3 else 1080)
else:
    sys.exit(__doc__)
