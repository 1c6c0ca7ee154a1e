"""rtgo_set_large_scene on the MI355X: the global-memory build against the oracle's canonical LBVH, bit for bit, and renders through the
global-memory walk against rtgo_set_scene's, bit for bit -- for the reference scenes, for scenes beyond RTGO_MAX_PRIMS made by duplicating
primitives (ties keep the lower SBT index) or by hiding primitives inside a closed box, in windows and row bands -- plus the limits, the
error paths and the context's state across scene changes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REF_SCENES = ["cornell", "slide", "mirror_spheres", "plateau", "window", "checkered", "balls", "soft_mirrors"]
RTGO_E_INVALID, RTGO_E_UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import capi as m
    m.load()
    return m


def tables(oracle, name, W, H):
    return oracle.scene_tables(oracle.scene(name, W, H))


def make_ctx(capi, t, large, with_aabbs=True, types=None, M=None, mat=None, aabb=None, ctx=None):
    """a context holding scene t (or the given arrays) through rtgo_set_large_scene (large) or rtgo_set_scene, with t's camera and lights"""
    types = t["type"] if types is None else types
    M = t["M"] if M is None else M
    mat = t["mat"] if mat is None else mat
    aabb = (t["aabb"] if aabb is None else aabb) if with_aabbs else None
    ctx = ctx or capi.Context(0)
    (ctx.set_large_scene if large else ctx.set_scene)(types, M, mat, aabb)
    ctx.set_camera(t["cam"][0:3], t["cam"][3:6], t["cam"][6:9], t["cam"][9:12])
    ctx.set_background(t["bg"])
    ctx.set_lights(t["lights"])
    return ctx


def render(capi, ctx, W, H, n=2, frames=(0,), path=True, window=None, bands=(4, 1, 0), stats=0):
    """the accumulation buffer, image and counters after launching the given frames (progressive) on ctx"""
    x0, y0, w, h = window if window else (0, 0, W, H)
    rows = capi.local_rows(h, bands[0], bands[1], bands[2])
    ctx.resize(max(rows * w, 1))
    ctx.reset_stats()
    for f in frames:
        ctx.launch(capi.make_frame(W, H, n, f, path, False, window, bands, stats=stats))
    ctx.sync()
    return ctx.read_accum(rows, w), ctx.read_image(rows, w), ctx.stats()


def assert_same(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), what + ": accum"
    assert np.array_equal(a[1], b[1]), what + ": image"
    assert a[2]["rays_total"] == b[2]["rays_total"] and a[2]["rays_occlusion"] == b[2]["rays_occlusion"], what


def random_scene(n, seed, spread=10.0):
    """n primitives of all four types, each rotated, scaled and translated"""
    rng = np.random.default_rng(seed)
    types = rng.integers(0, 4, size=n).astype(np.uint32)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)
    S = rng.uniform(0.05, 0.6, size=(n, 3))
    M = np.zeros((n, 4, 4), dtype=np.float32)
    M[:, :3, :3] = R * S[:, None, :]
    M[:, :3, 3] = rng.uniform(-spread, spread, size=(n, 3))
    M[:, 3, 3] = 1.0
    mat = rng.uniform(0.0, 1.0, size=(n, 10)).astype(np.float32)
    mat[:, 7:10] *= rng.uniform(size=(n, 1)) < 0.05
    return types, M.reshape(n, 16), mat


def oracle_boxes(oracle, M):
    out = np.zeros((len(M), 6), dtype=np.float32)
    for i in range(len(M)):
        bb = np.zeros(6, dtype=np.float32)
        oracle.lib().oracle_prim_aabb(oracle.fptr(np.ascontiguousarray(M[i], dtype=np.float32)), oracle.fptr(bb))
        out[i] = bb
    return out


def oracle_inverses(oracle, M):
    out = np.zeros((len(M), 16), dtype=np.float32)
    for i in range(len(M)):
        oracle.lib().oracle_mat_inverse(oracle.fptr(np.ascontiguousarray(M[i], dtype=np.float32)), oracle.fptr(out[i]))
    return out[:, :12]


def tree_depth(links):
    """largest number of edges from the root (node 0) to a leaf"""
    depth = np.zeros(len(links), dtype=np.int64)
    best = 0
    stack = [0]
    while stack:
        k = stack.pop()
        if links[k, 1] >= 0:
            for ch in links[k]:
                depth[ch] = depth[k] + 1
                stack.append(int(ch))
        else:
            best = max(best, int(depth[k]))
    return best


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def hip():
    """the HIP runtime librtgo_hip.so runs on (device buffers for rtgo_assemble_bands, hipMemGetInfo): the copy this process has mapped
    (a process that imported torch first may run on torch's own)"""
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64.so" in line)
    L = C.CDLL(path)
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    L.hipFree.argtypes = [C.c_void_p]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    return L


def mem_free(H):
    free, total = C.c_size_t(), C.c_size_t()
    assert H.hipDeviceSynchronize() == 0 and H.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


# ---- 1. the build ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 513, 4099, 65536])
@pytest.mark.parametrize("with_aabbs", [True, False])
def test_build_matches_the_oracle(capi, oracle, n, with_aabbs):
    types, M, mat = random_scene(n, seed=n, spread=2.0 + n ** (1.0 / 3.0))
    boxes_in = oracle_boxes(oracle, M)
    if with_aabbs:   # boxes of the caller's own: larger than the CubeBox rule's, by a different pad per primitive
        boxes_in = boxes_in + np.random.default_rng(n + 1).uniform(0.0, 0.25, size=(n, 6)).astype(np.float32) * np.array([-1, -1, -1, 1, 1, 1], np.float32)
    ctx = capi.Context(0)
    ctx.set_large_scene(types, M, mat, boxes_in if with_aabbs else None)
    boxes, links, inv, aabb = ctx.read_bvh()
    assert np.array_equal(bits(aabb), bits(boxes_in)), "boxes per primitive"
    oboxes, olinks, _, _ = oracle.lbvh(boxes_in)
    assert np.array_equal(links, olinks), "links"
    assert np.array_equal(bits(boxes), bits(oboxes)), "node boxes"
    assert np.array_equal(bits(inv), bits(oracle_inverses(oracle, M))), "inverses"
    assert ctx.stats()["lbvh_depth"] == tree_depth(olinks)
    assert ctx.stats()["cuboid_groups"] == 0
    ctx.close()


def test_reference_scenes_build_the_same_tree(capi, oracle):
    for name in REF_SCENES:
        t = tables(oracle, name, 64, 64)
        for with_aabbs in (True, False):
            small = make_ctx(capi, t, False, with_aabbs)
            large = make_ctx(capi, t, True, with_aabbs)
            for a, b in zip(small.read_bvh(), large.read_bvh()):
                assert np.array_equal(bits(a), bits(b)), name
            assert small.stats()["lbvh_depth"] == large.stats()["lbvh_depth"], name
            small.close()
            large.close()


# ---- 2. the same pixels as rtgo_set_scene -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", REF_SCENES)
@pytest.mark.parametrize("path", [True, False], ids=["path", "distributed"])
def test_reference_scenes_render_the_same(capi, oracle, name, path):
    W, H = 96, 64
    t = tables(oracle, name, W, H)
    small, large = make_ctx(capi, t, False), make_ctx(capi, t, True)
    cases = [("frames 0, 1", dict(frames=(0, 1))), ("window", dict(frames=(0,), window=(13, 9, 51, 37)))]
    cases += [("band %d/3" % r, dict(frames=(1,), bands=(4, 3, r))) for r in range(3)]
    for what, kw in cases:
        a = render(capi, small, W, H, 2, path=path, **kw)
        b = render(capi, large, W, H, 2, path=path, **kw)
        assert_same(a, b, "%s %s" % (name, what))
        assert b[2]["last_variant"] & 0x24 == 0x24 and b[2]["launches_canonical"] == len(kw["frames"])
    # collect_stats 1 traces every pixel through the canonical walk on both sides: the same walk, the same counters
    a, b = render(capi, small, W, H, 2, path=path, stats=1), render(capi, large, W, H, 2, path=path, stats=1)
    assert_same(a, b, name + " collect_stats 1")
    for k in ("node_visits", "prim_tests", "hits"):
        assert a[2][k] == b[2][k], (name, k, a[2][k], b[2][k])
    assert b[2]["node_visits"] > 0
    # collect_stats 2 culls by each side's own screen rectangle: the traversal counters may differ, the hits may not
    a, b = render(capi, small, W, H, 2, path=path, stats=2), render(capi, large, W, H, 2, path=path, stats=2)
    assert_same(a, b, name + " collect_stats 2")
    assert a[2]["hits"] == b[2]["hits"]
    small.close()
    large.close()


# ---- 3. beyond RTGO_MAX_PRIMS by duplication --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,copies", [("checkered", 3), ("balls", 4), ("cornell", 40)])
@pytest.mark.parametrize("path", [True, False], ids=["path", "distributed"])
def test_duplicated_primitives_render_like_the_original(capi, oracle, name, copies, path):
    W, H = 128, 96
    t = tables(oracle, name, W, H)
    rep = lambda a: np.concatenate([a] * copies)
    assert len(t["type"]) * copies > capi.RTGO_MAX_PRIMS
    small = make_ctx(capi, t, False)
    large = make_ctx(capi, t, True, types=rep(t["type"]), M=rep(t["M"]), mat=rep(t["mat"]), aabb=rep(t["aabb"]))
    for frames in ((0,), (0, 1)):
        assert_same(render(capi, small, W, H, 2, frames, path), render(capi, large, W, H, 2, frames, path),
                    "%s x%d frames %s" % (name, copies, frames))
    small.close()
    large.close()


def test_duplicated_balls_at_1080p(capi, oracle):
    W, H = 1920, 1080
    t = tables(oracle, "balls", W, H)
    rep = lambda a: np.concatenate([a] * 4)
    small = make_ctx(capi, t, False)
    large = make_ctx(capi, t, True, types=rep(t["type"]), M=rep(t["M"]), mat=rep(t["mat"]), aabb=rep(t["aabb"]))
    assert_same(render(capi, small, W, H, 2), render(capi, large, W, H, 2), "balls x4 1080p")
    small.close()
    large.close()


# ---- 4. beyond RTGO_MAX_PRIMS, hidden geometry ------------------------------------------------------------------------------------------
def closed_cube(center, half, ext):
    """six one-sided rectangles facing out (object-space square |x|, |z| < 1/2 in y = 0, hit from +y) of side 2 (half + ext): each
    reaches `ext` past the cube's edges, so every ray from outside into the cube crosses one of them first"""
    c = np.asarray(center, dtype=np.float64)
    L = 2.0 * (half + ext)
    M = []
    for k in range(3):
        for s in (1.0, -1.0):
            i, j = [a for a in range(3) if a != k]
            m = np.eye(4)
            m[:3, 0] = 0.0
            m[:3, 1] = 0.0
            m[:3, 2] = 0.0
            m[i, 0] = L
            m[k, 1] = s
            m[j, 2] = L
            m[:3, 3] = c
            m[k, 3] += s * half
            M.append(m.astype(np.float32).reshape(16))
    types = np.full(6, 2, dtype=np.uint32)
    mat = np.tile(np.array([0.6, 0.5, 0.4, 0.0, 0.0, 0.0, 10.0, 0.0, 0.0, 0.0], np.float32), (6, 1))
    return types, np.array(M), mat


def hidden_scene(oracle, n_spheres, W, H):
    """cornell + a closed cube on its floor (t, the visible part: cornell + the cube) and the same with n_spheres small spheres inside"""
    t = tables(oracle, "cornell", W, H)
    center, half = (-2.4, -3.2, 2.4), 0.6
    ct, cM, cm = closed_cube(center, half, 0.1)
    rng = np.random.default_rng(7)
    r = rng.uniform(0.002, 0.01, size=n_spheres)
    p = np.asarray(center) + rng.uniform(-(half - 0.05), half - 0.05, size=(n_spheres, 3))
    sM = np.zeros((n_spheres, 16), dtype=np.float32)
    sM[:, 0] = sM[:, 5] = sM[:, 10] = r
    sM[:, 3], sM[:, 7], sM[:, 11], sM[:, 15] = p[:, 0], p[:, 1], p[:, 2], 1.0
    smat = rng.uniform(0.0, 1.0, size=(n_spheres, 10)).astype(np.float32)
    st = np.full(n_spheres, 3, dtype=np.uint32)
    vis = dict(types=np.concatenate([t["type"], ct]), M=np.concatenate([t["M"], cM]), mat=np.concatenate([t["mat"], cm]))
    vis["aabb"] = np.concatenate([t["aabb"], oracle_boxes(oracle, cM)])
    full = {k: np.concatenate([vis[k], x]) for k, x in (("types", st), ("M", sM), ("mat", smat))}
    full["aabb"] = np.concatenate([vis["aabb"], oracle_boxes(oracle, sM)])
    return t, vis, full


@pytest.mark.parametrize("path", [True, False], ids=["path", "distributed"])
def test_hidden_spheres_render_like_the_empty_cube(capi, oracle, path):
    W, H = 160, 120
    t, vis, full = hidden_scene(oracle, 100000, W, H)
    small = make_ctx(capi, t, False, **vis)
    for with_aabbs in (True, False):
        large = make_ctx(capi, t, True, with_aabbs=with_aabbs, **full)
        assert_same(render(capi, small, W, H, 2, (0, 1), path), render(capi, large, W, H, 2, (0, 1), path), "hidden, boxes %s" % with_aabbs)
        large.close()
    small.close()


# ---- 5. row bands of a 100 000-primitive scene ------------------------------------------------------------------------------------------
def test_bands_reassemble_the_frame(capi, oracle):
    W, H, G, band_h = 200, 150, 4, 4
    t, _, full = hidden_scene(oracle, 100000 - 25, W, H)
    assert len(full["types"]) == 100000
    whole = make_ctx(capi, t, True, **full)
    ref = render(capi, whole, W, H, 2, (0,))
    rows_pad = max(capi.local_rows(H, band_h, G, g) for g in range(G))
    gathered = np.zeros((G * rows_pad, W, 4), dtype=np.float32)
    gathered_img = np.zeros((G * rows_pad, W, 4), dtype=np.uint8)
    rays = 0
    for g in range(G):
        share = render(capi, whole, W, H, 2, (0,), bands=(band_h, G, g))
        k = capi.local_rows(H, band_h, G, g)
        gathered[g * rows_pad:g * rows_pad + k] = share[0]
        gathered_img[g * rows_pad:g * rows_pad + k] = share[1]
        rays += share[2]["rays_total"]
    assert rays == ref[2]["rays_total"]
    L, Hp = capi.load(), hip()
    for src, elem, want in ((gathered, 16, ref[0]), (gathered_img, 4, ref[1])):
        d_g, d_f = C.c_void_p(), C.c_void_p()
        assert Hp.hipMalloc(C.byref(d_g), src.nbytes) == 0 and Hp.hipMalloc(C.byref(d_f), want.nbytes) == 0
        assert Hp.hipMemcpy(d_g, src.ctypes.data, src.nbytes, 1) == 0   # hipMemcpyHostToDevice
        assert L.rtgo_assemble_bands(whole._h, None, d_g, d_f, W, H, band_h, G, rows_pad, elem) == 0
        whole.sync()
        got = np.empty_like(want)
        assert Hp.hipMemcpy(got.ctypes.data, d_f, got.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        Hp.hipFree(d_g)
        Hp.hipFree(d_f)
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), elem
    whole.close()


# ---- 6. limits and state ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene(capi, oracle):
    W, H = 64, 48
    t = tables(oracle, "balls", W, H)
    ctx = make_ctx(capi, t, True)
    before = render(capi, ctx, W, H)
    L = capi.load()
    one = (capi.Prim * 1)()
    one[0].type = 3
    one[0].model[:] = np.eye(4, dtype=np.float32).reshape(16).tolist()
    assert L.rtgo_set_large_scene(ctx._h, one, None, 0) == RTGO_E_UNSUPPORTED
    assert L.rtgo_set_large_scene(ctx._h, one, None, capi.RTGO_MAX_SCENE_PRIMS + 1) == RTGO_E_UNSUPPORTED
    assert L.rtgo_set_large_scene(ctx._h, None, None, 4) == RTGO_E_INVALID
    singular = np.array(t["M"], copy=True)
    singular[5, 0:3] = 0.0
    with pytest.raises(capi.RtgoError, match="primitive 5"):
        ctx.set_large_scene(t["type"], singular, t["mat"], None)
    bad_box = np.array(t["aabb"], copy=True)
    bad_box[7, 0] = bad_box[7, 3] + 1.0
    with pytest.raises(capi.RtgoError, match="box 7"):
        ctx.set_large_scene(t["type"], t["M"], t["mat"], bad_box)
    bad_type = np.array(t["type"], copy=True)
    bad_type[3] = 9
    with pytest.raises(capi.RtgoError):
        ctx.set_large_scene(bad_type, t["M"], t["mat"], None)
    assert_same(before, render(capi, ctx, W, H), "after refused calls")
    assert L.rtgo_set_large_scene(None, one, None, 1) == RTGO_E_INVALID
    ctx.close()


def test_large_small_large_on_one_context(capi, oracle):
    W, H = 96, 64
    tb, tc = tables(oracle, "balls", W, H), tables(oracle, "cornell", W, H)
    fresh_large = make_ctx(capi, tb, True)
    fresh_small = make_ctx(capi, tc, False)
    want_large, want_small = render(capi, fresh_large, W, H, 2, (0, 1)), render(capi, fresh_small, W, H, 2, (0, 1))
    ctx = make_ctx(capi, tb, True)
    assert_same(render(capi, ctx, W, H, 2, (0, 1)), want_large, "large")
    make_ctx(capi, tc, False, ctx=ctx)
    got = render(capi, ctx, W, H, 2, (0, 1))
    assert_same(got, want_small, "small after large")
    assert got[2]["last_variant"] & 0x20 == 0
    make_ctx(capi, tb, True, ctx=ctx)
    assert_same(render(capi, ctx, W, H, 2, (0, 1)), want_large, "large after small")
    for c in (ctx, fresh_large, fresh_small):
        c.close()


def sphere_field(n, seed):
    """n spheres spread over a 40-unit cube in front of cornell's camera (a million fits RTGO_MAX_SCENE_PRIMS exactly)"""
    rng = np.random.default_rng(seed)
    M = np.zeros((n, 16), dtype=np.float32)
    r = rng.uniform(0.01, 0.08, size=n)
    M[:, 0] = M[:, 5] = M[:, 10] = r
    M[:, 3], M[:, 7], M[:, 11] = rng.uniform(-20, 20, size=(3, n))
    M[:, 15] = 1.0
    mat = rng.uniform(0.0, 1.0, size=(n, 10)).astype(np.float32)
    mat[:, 7:10] = 0.0
    return np.full(n, 3, dtype=np.uint32), M, mat


def test_full_size_scene_renders_the_same_on_two_contexts(capi, oracle):
    W, H = 256, 256
    t = tables(oracle, "cornell", W, H)
    types, M, mat = sphere_field(capi.RTGO_MAX_SCENE_PRIMS, 11)
    out = []
    for _ in range(2):
        ctx = make_ctx(capi, t, True, types=types, M=M, mat=mat, with_aabbs=False)
        assert 0 < ctx.stats()["lbvh_depth"] <= 64
        out.append(render(capi, ctx, W, H, 2, (0, 1)))
        ctx.close()
    assert np.isfinite(out[0][0]).all()
    assert_same(out[0], out[1], "two contexts")


def test_contexts_release_their_memory(capi, oracle):
    t = tables(oracle, "cornell", 64, 64)
    types, M, mat = sphere_field(capi.RTGO_MAX_SCENE_PRIMS, 12)
    warm = make_ctx(capi, t, True)   # (the first launch of the process loads the code objects)
    render(capi, warm, 64, 64, 1)
    warm.close()
    H = hip()
    free0 = mem_free(H)
    for _ in range(10):
        ctx = make_ctx(capi, t, True, types=types, M=M, mat=mat, with_aabbs=False)
        render(capi, ctx, 64, 64, 1)
        ctx.close()
    free1 = mem_free(H)
    assert free0 - free1 < 8 << 20, (free0, free1)
