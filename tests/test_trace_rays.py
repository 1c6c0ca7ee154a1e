"""rtgo_trace_rays on the MI355X: caller-supplied rays against the analytic scene, held to a brute force over the oracle's intersection
programs; the acceptance window and the tie rule; the kernel's forms (scene in LDS or in global memory, rtgo_set_scene or
rtgo_set_large_scene, any batch size, any grid) bit for bit; the error codes and edges; and rtgo_host_session_pick."""
import os

import numpy as np
import pytest

import trace_rays_ref as R

pytestmark = pytest.mark.gpu

RTGO_E_INVALID, RTGO_E_STATE = 1, 3
TMIN, TMAX = np.float32(1e-3), np.float32(1e16)
# Largest relative deviation of the device's t and n from the oracle's over the clear rays of the four scenes below, as measured on an
# MI355X: 0 and 0 -- the canonical walk keeps the plain IEEE operators and the build forbids contraction, as the oracle's
# does, so the two run the same roundings.  The bounds are 4 x that: equality.
T_BOUND, N_BOUND = 4 * 0.0, 4 * 0.0
UNCLEAR_CAP = 0.02


@pytest.fixture(scope="module")
def capi():
    import torch
    from raytracingo_amd import capi as m
    m.load()
    if torch.cuda.is_available():
        torch.cuda.init()   # torch's HIP runtime up before this module's first context (some tests hand the library torch buffers)
    return m


class Knob:
    """an environment knob set for the length of a with block (the library reads them afresh at every call)"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


SCENES = {"cornell": (1, 768), "plateau": (1, 768), "mirror_spheres": (1, 768), "checkered": (4, 200)}
_cache = {}


def scene_case(oracle, name):
    """the scene's tables, its rays (32 x 24 pixel-centre primaries, every step-th, plus random rays; seed 7) and the brute-force
    reference, computed once"""
    if name not in _cache:
        step, n_random = SCENES[name]
        sc = oracle.scene(name, 32, 24)
        t = oracle.scene_tables(sc)
        o, d = R.scene_rays(t, 32, 24, n_random, step)
        _cache[name] = (t, sc, o, d, R.reference(oracle, sc, o, d, TMIN, TMAX))
    return _cache[name]


def make_ctx(capi, t, large=False):
    ctx = capi.Context(0)
    (ctx.set_large_scene if large else ctx.set_scene)(t["type"], t["M"], t["mat"], t["aabb"])
    return ctx


def same_hits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", list(SCENES))
def test_analytic_path_against_brute_force(capi, oracle, name):
    t, sc, o, d, ref = scene_case(oracle, name)
    ctx = make_ctx(capi, t)
    hits = ctx.trace_rays(capi.make_rays(o, d, TMIN, TMAX))
    clear = ~ref["unclear"]
    share = ref["unclear"].mean()
    hit = clear & (ref["prim"] >= 0)
    dt = R.rel_dev(hits["t"][hit], ref["t"][hit])
    dn = R.rel_dev(hits["n"][hit], ref["n"][hit])
    print("%s: %d rays, %d hit, unclear %.4f, t deviation %.3g, n deviation %.3g" % (name, len(o), hit.sum(), share, dt, dn))
    assert share <= UNCLEAR_CAP
    assert np.array_equal(hits["prim"][clear], ref["prim"][clear]), np.nonzero(hits["prim"] != ref["prim"])[0][:10]
    assert dt <= T_BOUND and dn <= N_BOUND, (dt, dn)
    # the rest of the record
    miss = hits["prim"] == capi.HIT_MISS
    assert (hits["prim"] >= -1).all()
    assert np.array_equal(hits["t"][miss], np.full(miss.sum(), TMAX)) and (hits["instance"][miss] == 0).all() and (hits["n"][miss] == 0).all()
    assert (hits["instance"][~miss] == -1).all() and (hits["u"] == 0).all() and (hits["v"] == 0).all()


def test_acceptance_window(capi, oracle):
    """re-trace the rays that hit with the window's ends at the GPU's own t: the hit is kept exactly when tmin < t < tmax"""
    t, sc, o, d, ref = scene_case(oracle, "cornell")
    ctx = make_ctx(capi, t)
    first = ctx.trace_rays(capi.make_rays(o, d, TMIN, TMAX))
    h = first["prim"] >= 0
    o, d, first = o[h], d[h], first[h]
    th = first["t"]
    assert len(th) > 300
    inf, zero = np.float32(np.inf), np.float32(0)
    # tmax = t: nothing is nearer than the closest hit, so a miss, with the new tmax as its t
    got = ctx.trace_rays(capi.make_rays(o, d, TMIN, th))
    assert (got["prim"] == capi.HIT_MISS).all() and np.array_equal(got["t"], th)
    # tmax just above t: the same hit, bit for bit
    assert same_hits(ctx.trace_rays(capi.make_rays(o, d, TMIN, np.nextafter(th, inf))), first)
    # tmin = t: that hit is refused; whatever is reported lies strictly behind it
    got = ctx.trace_rays(capi.make_rays(o, d, th, TMAX))
    behind = got["prim"] >= 0
    assert (got["prim"][~behind] == capi.HIT_MISS).all() and (got["t"][behind] > th[behind]).all()
    assert behind.any() and (~behind).any()
    for k in np.nonzero(behind)[0][:64]:   # ... and is what the brute force finds behind it, where that is clear
        p, tv, _, second = R.brute(oracle, sc, o[k], d[k], th[k], TMAX)
        if second - float(tv) > 1e-4 * max(1.0, float(tv)):
            assert p == got["prim"][k], (k, p, got[k])
    # tmin just below t: the same hit
    assert same_hits(ctx.trace_rays(capi.make_rays(o, d, np.nextafter(th, zero), TMAX)), first)


def test_ties_keep_the_lower_sbt_index(capi, oracle):
    """two rectangles under one model matrix (and a third elsewhere), in either order of their materials: index 0 is reported"""
    t = oracle.scene_tables(oracle.scene("cornell", 32, 24))
    rect = int(np.nonzero(t["type"] == capi.RECTANGLE)[0][0])
    other = int(np.nonzero(t["type"] == capi.RECTANGLE)[0][1])
    M = t["M"][rect].reshape(4, 4).astype(np.float64)
    centre, normal = M[:3, 3], M[:3, 1] / np.linalg.norm(M[:3, 1])
    rng = np.random.RandomState(3)
    pts = centre + (M[:3, :3] @ np.stack([rng.uniform(-0.4, 0.4, 64), np.zeros(64), rng.uniform(-0.4, 0.4, 64)])).T
    o = (pts + 2.0 * normal).astype(np.float32)
    d = np.tile(-normal, (64, 1)).astype(np.float32)
    for order in ((0, 1), (1, 0)):
        mats = np.stack([t["mat"][rect], t["mat"][other]])[list(order)]
        types = np.array([capi.RECTANGLE] * 3)
        ctx = capi.Context(0)
        far = t["M"][other].copy()
        far[3] += 100.0   # (out of every ray's way)
        ctx.set_scene(types, np.stack([t["M"][rect], t["M"][rect], far]), np.concatenate([mats, t["mat"][other:other + 1]]), None)
        hits = ctx.trace_rays(capi.make_rays(o, d, TMIN, TMAX))
        assert (hits["prim"] == 0).all(), hits["prim"]
        # with the front one out of the window's reach nothing changes: both lie at the same t
        again = ctx.trace_rays(capi.make_rays(o, d, hits["t"], TMAX))
        assert (again["prim"] != 0).all() and (again["prim"] != 1).all()


@pytest.mark.parametrize("name", ["cornell", "checkered"])
def test_forms_agree_bitwise(capi, oracle, name):
    t, sc, o, d, ref = scene_case(oracle, name)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    ctx = make_ctx(capi, t)
    with Knob(RTGO_TRACE_MODE=0, RTGO_TRACE_BLOCKS=None):
        base = ctx.trace_rays(rays)
    assert (base["prim"] >= 0).sum() > 50
    with Knob(RTGO_TRACE_MODE=1):
        assert same_hits(ctx.trace_rays(rays), base), "scene in LDS"
    with Knob(RTGO_TRACE_MODE=None):
        assert same_hits(ctx.trace_rays(rays), base), "the host's own choice"
    assert same_hits(make_ctx(capi, t, large=True).trace_rays(rays), base), "rtgo_set_large_scene"
    perm = np.random.RandomState(1).permutation(len(rays))
    for mode in (0, 1):
        with Knob(RTGO_TRACE_MODE=mode):
            assert same_hits(ctx.trace_rays(rays[perm]), base[perm]), "permuted rays"
            for n in (1, 63, 64, 65, 256, 257):
                assert same_hits(ctx.trace_rays(rays[:n]), base[:n]), "batch of %d" % n
            # two workgroups of at most 1024 lanes: 257 rays are two passes and one ray of the smallest workgroup, 4097 of the largest
            with Knob(RTGO_TRACE_BLOCKS=2):
                big = np.tile(rays, 3)[:4097]
                got = ctx.trace_rays(big)
                assert same_hits(got, np.tile(base, 3)[:4097]), "grid-stride loop"
                assert same_hits(ctx.trace_rays(rays[:257]), base[:257])
            with Knob(RTGO_TRACE_BLOCKS=1):
                assert same_hits(ctx.trace_rays(rays[:300]), base[:300])


def test_any_hit_gives_the_same_mask(capi, oracle):
    t, sc, o, d, ref = scene_case(oracle, "mirror_spheres")
    ctx = make_ctx(capi, t)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    a, b = ctx.trace_rays(rays), ctx.trace_rays(rays, capi.TRACE_ANY_HIT)
    assert np.array_equal(a["prim"] >= 0, b["prim"] >= 0)


def test_error_codes(capi, oracle):
    import torch
    t = oracle.scene_tables(oracle.scene("cornell", 32, 24))
    ctx = capi.Context(0)
    buf = torch.zeros((64, 8), dtype=torch.float32, device="cuda:0")
    rays, hits = buf[:16].data_ptr(), buf[16:].data_ptr()
    assert rays % 16 == 0 and hits % 16 == 0
    assert ctx.trace_rays_raw(rays, hits, 4) == RTGO_E_STATE            # no scene of this kind
    assert ctx.trace_rays_raw(rays, hits, 4, whitted=True) == RTGO_E_STATE
    ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
    assert ctx.trace_rays_raw(rays, hits, 4, whitted=True) == RTGO_E_STATE   # an analytic scene is no mesh
    for whitted in (False, True):
        assert ctx.trace_rays_raw(0, hits, 4, whitted=whitted) == RTGO_E_INVALID
        assert ctx.trace_rays_raw(rays, 0, 4, whitted=whitted) == RTGO_E_INVALID
        assert ctx.trace_rays_raw(rays + 4, hits, 4, whitted=whitted) == RTGO_E_INVALID
        assert ctx.trace_rays_raw(rays, hits + 8, 4, whitted=whitted) == RTGO_E_INVALID
        assert ctx.trace_rays_raw(rays, hits, 4, flags=2, whitted=whitted) == RTGO_E_INVALID
        assert ctx.trace_rays_raw(rays, hits, 4, flags=0x80000001, whitted=whitted) == RTGO_E_INVALID
        assert ctx.trace_rays_raw(rays, hits, (1 << 30) + 1, whitted=whitted) == RTGO_E_INVALID
    assert ctx.trace_rays_raw(rays, hits, 4) == 0
    ctx.sync()


def test_invalid_rays_and_empty_batches(capi, oracle):
    import torch
    t, sc, o, d, ref = scene_case(oracle, "cornell")
    ctx = make_ctx(capi, t)
    rays = capi.make_rays(o[:200], d[:200], TMIN, TMAX)
    alone = ctx.trace_rays(rays)
    bad = rays.copy()
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    spoil = {3: ("origin", (nan, 0, 0)), 10: ("dir", (0, 0, 0)), 64: ("tmax", TMIN), 65: ("tmax", np.float32(0)), 66: ("tmin", np.float32(-1)),
             100: ("dir", (1, inf, 0)), 127: ("tmax", nan), 128: ("tmin", nan), 150: ("origin", (0, -inf, 0)), 199: ("tmax", inf)}
    for k, (field, value) in spoil.items():
        bad[field][k] = value
    got = ctx.trace_rays(bad)
    ks = np.array(sorted(spoil))
    assert (got["prim"][ks] == capi.HIT_INVALID).all(), got["prim"][ks]
    assert not got[ks].view(np.uint32).reshape(len(ks), 8)[:, [0, 2, 3, 4, 5, 6, 7]].any(), "an invalid ray's record is zero beside prim"
    keep = np.ones(len(rays), bool)
    keep[ks] = False
    assert same_hits(got[keep], alone[keep]), "the neighbours of invalid rays"
    # n == 0: nothing is written
    sentinel = torch.full((8, 8), 1234.5, dtype=torch.float32, device="cuda:0")
    before = ctx.stats()
    assert ctx.trace_rays_raw(sentinel.data_ptr(), sentinel.data_ptr(), 0) == 0
    ctx.sync()
    torch.cuda.synchronize()
    assert (sentinel == 1234.5).all().item()
    assert ctx.stats()["rays_total"] == before["rays_total"]
    assert len(ctx.trace_rays(rays[:0])) == 0


def test_stats_and_renders_are_left_alone(capi, oracle):
    W, H = 64, 48
    t, sc, o, d, ref = scene_case(oracle, "cornell")
    ctx = make_ctx(capi, t)
    ctx.set_camera(t["cam"][0:3], t["cam"][3:6], t["cam"][6:9], t["cam"][9:12])
    ctx.set_background(t["bg"])
    ctx.set_lights(t["lights"])
    ctx.resize(W * H)

    def render():
        for f in (0, 1):
            ctx.launch(capi.make_frame(W, H, 2, f, True))
        ctx.sync()
        return ctx.read_accum(H, W), ctx.read_image(H, W)

    a0, i0 = render()
    s0 = ctx.stats()
    rays = capi.make_rays(o, d, TMIN, TMAX)
    ctx.trace_rays(rays)
    s1 = ctx.stats()
    assert s1["rays_total"] == s0["rays_total"] + len(rays) and s1["rays_occlusion"] == s0["rays_occlusion"]
    ctx.trace_rays(rays[:100], capi.TRACE_ANY_HIT)
    s2 = ctx.stats()
    assert s2["rays_total"] == s1["rays_total"] + 100 and s2["rays_occlusion"] == s1["rays_occlusion"] + 100
    for k in ("launches", "last_launch_ms", "last_variant", "launches_trial", "launches_canonical", "total_launch_ms"):
        assert s2[k] == s0[k], k
    a1, i1 = render()
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)) and np.array_equal(i0, i1)
    ctx.reset_stats()
    assert ctx.stats()["rays_total"] == 0 and ctx.stats()["rays_occlusion"] == 0


def test_torch_tensor_input(capi, oracle):
    import torch
    t, sc, o, d, ref = scene_case(oracle, "cornell")
    ctx = make_ctx(capi, t)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).to("cuda:0")
    assert same_hits(ctx.trace_rays(dev), ctx.trace_rays(rays))


def test_host_session_pick(capi, oracle):
    """rtgo_host_session_pick equals Context.trace_rays of the same ray at one pixel of every primitive the camera sees (the walls, each
    box's faces) and of the background, before and after a camera move and a resize; the frame loop's state is left alone"""
    from raytracingo_amd import scene
    W, H = 64, 48
    t = scene.tables("cornell", W, H)
    ctx = capi.Context(0)
    ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
    s = scene.Session("cornell", "path", W, H)
    try:
        def check(w, h):
            eye, U, V, Wv = s.camera()
            o, d = R.primaries(np.concatenate([eye, U, V, Wv]), w, h)
            hits = ctx.trace_rays(capi.make_rays(o, d, TMIN, TMAX)).reshape(h, w)
            seen = np.unique(hits["prim"])
            for p in seen:
                ys, xs = np.nonzero(hits["prim"] == p)
                k = len(ys) // 2
                x, y = int(xs[k]), int(ys[k])
                prim, tv = s.pick(x, y)
                assert prim == p and np.float32(tv) == hits["t"][y, x], ((x, y), prim, tv, hits[y, x])
            return seen

        seen = check(W, H)
        assert -1 in seen and len(seen) >= 5, seen     # background, walls, both boxes
        assert np.array_equal(np.concatenate(s.camera()), t["cam"])
        s.frame()
        s.frame()
        assert s.read()[2] == 1
        s.move_camera((3.0, 2.0, 13.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
        assert len(check(W, H)) >= 5
        s.frame()
        assert s.read()[2] == 0   # the camera move still restarted the running average: pick did not use up the flag
        s.resize(80, 40)
        assert len(check(80, 40)) >= 5
        s.frame()
        assert s.read()[2] == 0
        with pytest.raises(capi.RtgoError):
            s.pick(80, 0)
    finally:
        s.close()
