"""rtgo_shade_rays on the MI355X: the analytic path's closest-hit, occlusion and miss programs for rays of the caller's own.

Held three ways.  Bit for bit to rtgo_launch, on the launch's own rays and seeds made on the host (shade_rays_ref.raygen32): both buffers
after every frame and the ray counts, in the three modes, over scenes of rtgo_set_scene and rtgo_set_large_scene, with the scene in LDS
and in global memory, with seeds handed over and left to the call.  To the float64 reference of tests/analytic_shading_ref64.py on a camera
the launches do not have (a lat-long window), under test_oracle_shading_float64.check_frame unchanged: the device gets no bound of its own.
And to the oracle's ray log: every node of a path is a ray, and shading it alone returns the node's payload (tests/parity.py's rule).
Then the call's own edges: batch shapes, invalid rays, the window at the device's t, the fold at later samples, refusals, and launches
left as they were.

Largest deviation from the float64 reference over the lat-long rays, in units of 2^-23 kappa (bound: T.DEV_BOUND), as printed by
test_latlong_rays_against_float64: see DESIGN.md 3.5.2."""
import ctypes as C

import numpy as np
import pytest

import analytic_shading_ref64 as S
import parity
import shade_rays_ref as R
import shading_scenes as SC
import test_oracle_shading_float64 as T
from test_shade_rays_ref import TILT, latlong_reference
from test_trace_rays import Knob

pytestmark = pytest.mark.gpu

W, H = T.W48, T.H36
RTGO_OK, RTGO_E_INVALID, RTGO_E_STATE, RTGO_E_UNSUPPORTED = 0, 1, 3, 4
TMIN, TMAX = R.T_MIN0, R.T_MAX0


@pytest.fixture(scope="module")
def capi():
    import torch
    from raytracingo_amd import capi as m
    m.load()
    if torch.cuda.is_available():
        torch.cuda.init()   # torch's HIP runtime up before this module's first context (some tests hand the library torch buffers)
    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """two (accum, image) pairs, bit for bit"""
    return np.array_equal(bits(a[0]), bits(b[0])) and (a[1] is None or b[1] is None or np.array_equal(a[1], b[1]))


_tables = {}


def tables(oracle, name):
    """(tables, width, height): the 48 x 36 shading scenes, and reference scenes at 64 x 48 -- cornell (a flat scene: the launch takes the
    two-leaf walk and precomputed frames) and balls (the launch walks the uniform grid)"""
    if name not in _tables:
        if name in SC.SCENES:
            _tables[name] = (SC.SCENES[name](W / H), W, H)
        else:
            _tables[name] = (oracle.scene_tables(oracle.scene(name, 64, 48)), 64, 48)
    return _tables[name]


def make_ctx(capi, t, pixels, large=False, lights=True):
    ctx = capi.Context(0)
    (ctx.set_large_scene if large else ctx.set_scene)(t["type"], t["M"], t["mat"], t.get("aabb"))
    c = t["cam"]
    ctx.set_camera(c[0:3], c[3:6], c[6:9], c[9:12])
    ctx.set_background(t["bg"])
    if lights:
        ctx.set_lights(t["lights"])
    ctx.resize(pixels)
    return ctx


def launch_frames(capi, ctx, w, h, mode, md, frames=3, between=None):
    """[(accum, image, rays_total delta, rays_occlusion delta, stats)] after each of the launches of frames 0 .. frames - 1"""
    path, amb = T.MODES[mode]
    out = []
    for f in range(frames):
        s0 = ctx.stats()
        ctx.launch(capi.make_frame(w, h, 1, f, path, amb, bands=(1, 1, 0), max_depth=md))
        ctx.sync()
        s1 = ctx.stats()
        out.append((ctx.read_accum(h, w).copy(), ctx.read_image(h, w).copy(), s1["rays_total"] - s0["rays_total"],
                    s1["rays_occlusion"] - s0["rays_occlusion"], s1))
        if between is not None:
            between(f)
    return out


def shade_frames(capi, ctx, cam, w, h, mode, md, frames=3, seeds=True):
    """the same through rtgo_shade_rays: the host raygen's rays and seeds of frame f, sample_index f, over the running buffer"""
    path, amb = T.MODES[mode]
    out, acc = [], None
    for f in range(frames):
        o, d, seed = R.raygen32(cam, w, h, f)
        s0 = ctx.stats()
        acc, img = ctx.shade_rays(capi.make_rays(o, d, TMIN, TMAX), seed if seeds else None, path, amb, md, f, acc)
        s1 = ctx.stats()
        out.append((acc.reshape(h, w, 4), img.reshape(h, w, 4), s1["rays_total"] - s0["rays_total"], s1["rays_occlusion"] - s0["rays_occlusion"], s1))
    return out


def assert_frames_equal(got, want, what):
    for f, (g, x) in enumerate(zip(got, want)):
        assert np.array_equal(bits(g[0]), bits(x[0])), "%s, frame %d: accum differs at %d pixels" % (what, f, (bits(g[0]) != bits(x[0])).any(-1).sum())
        assert np.array_equal(g[1], x[1]), "%s, frame %d: image" % (what, f)
        assert g[2:4] == x[2:4], "%s, frame %d: (rays_total, rays_occlusion) %r against %r" % (what, f, g[2:4], x[2:4])


# ---- 1. pinhole rays are the launch, bit for bit ------------------------------------------------------------------------------------------
PINHOLE = [(name, mode, md) for name in ("room", "two_lights", "quadrics", "cornell", "balls") for mode in T.MODES
           for md in ((0, 2) if name == "quadrics" else (0, 5))]


@pytest.mark.parametrize("name,mode,md", PINHOLE, ids=lambda v: str(v))
def test_pinhole_rays_are_the_launch(capi, oracle, name, mode, md):
    t, w, h = tables(oracle, name)
    ctx = make_ctx(capi, t, w * h)
    # (cornell at this size takes the two-leaf walk only at five waves per SIMD or more, and over the first tree: tests/test_pair_walk.py's knobs)
    with Knob(**({"RTGO_MAX_WPE": 6, "RTGO_TREE": 0} if name == "cornell" else {})):
        want = launch_frames(capi, ctx, w, h, mode, md)
    variants = [x[4]["last_variant"] for x in want]
    print(name, mode, md, "last_variant of the launches:", [hex(v) for v in variants])
    if name == "cornell" and mode == "path" and md == 5:
        assert all(v & 256 for v in variants), "the launches did not take the two-leaf walk"
    if name == "balls":
        assert any(v & 16 for v in variants), "no launch walked the grid"
    got = shade_frames(capi, ctx, t["cam"], w, h, mode, md)
    assert_frames_equal(got, want, "%s %s max_depth %d" % (name, mode, md))
    o, d, _ = R.raygen32(t["cam"], w, h, 0)
    assert (ctx.trace_rays(capi.make_rays(o, d, TMIN, TMAX))["prim"] >= 0).mean() > (0.3 if name in SC.SCENES else 0.1)   # the view sees the scene
    if mode != "path":
        assert got[0][3] > 0
    if md == 0:
        ctx.close()
        return
    # the kernel's other forms: the scene read from global memory / staged in LDS, and a scene of rtgo_set_large_scene
    for knob in (0, 1):
        with Knob(RTGO_TRACE_MODE=knob):
            assert_frames_equal(shade_frames(capi, ctx, t["cam"], w, h, mode, md), want, "%s %s RTGO_TRACE_MODE=%d" % (name, mode, knob))
    ctx.close()
    big = make_ctx(capi, t, w * h, large=True)
    want_big = launch_frames(capi, big, w, h, mode, md)
    assert_frames_equal(want_big, want, "%s %s: the large scene's launches" % (name, mode))
    assert_frames_equal(shade_frames(capi, big, t["cam"], w, h, mode, md), want, "%s %s through rtgo_set_large_scene" % (name, mode))
    big.close()


@pytest.mark.parametrize("mode", list(T.MODES))
def test_no_seeds_is_tea16_of_the_index(capi, oracle, mode):
    t, w, h = tables(oracle, "room")
    ctx = make_ctx(capi, t, w * h)
    path, amb = T.MODES[mode]
    o, d, _ = R.raygen32(t["cam"], w, h, 0)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    prev = None
    for k in (0, 1, 7):
        explicit = ctx.shade_rays(rays, R.index_seeds(len(rays), k), path, amb, 5, k, prev)
        implicit = ctx.shade_rays(rays, None, path, amb, 5, k, prev)
        assert same(explicit, implicit), (mode, k)
        other = ctx.shade_rays(rays, R.index_seeds(len(rays), k + 100), path, amb, 5, k, prev)
        assert not same(explicit, other)
        prev = explicit[0]
    ctx.close()


# ---- 2. a camera the launches do not have -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(T.MODES))
@pytest.mark.parametrize("name", list(SC.SCENES))
def test_latlong_rays_against_float64(capi, name, mode):
    path, amb = T.MODES[mode]
    ctx = None
    for md in T.DEPTHS[name]:
        t, r, o, d, seed = latlong_reference(name, mode, md)
        if ctx is None:
            ctx = make_ctx(capi, t, W * H)
        s0 = ctx.stats()
        acc, img = ctx.shade_rays(capi.make_rays(o, d, TMIN, TMAX), seed, path, amb, md, 0)
        s1 = ctx.stats()
        fig = T.check_frame(name, mode, md, 1, (t, r), acc.reshape(H, W, 4), img.reshape(H, W, 4),
                            rays_occlusion=s1["rays_occlusion"] - s0["rays_occlusion"], rays_total=s1["rays_total"] - s0["rays_total"])
        print("lat-long %s %s max_depth %d: largest dev %.2f units (bound %.2f), tilt %g" % (name, mode, md, fig["dev"], T.DEV_BOUND[(name, mode)], TILT[name]))
    ctx.close()


# ---- 3. any node of a path is a ray -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(T.MODES))
@pytest.mark.parametrize("name", ["room", "quadrics"])
def test_every_node_of_a_path_is_a_ray(capi, oracle, name, mode):
    t, w, h = tables(oracle, name)
    md = 2 if name == "quadrics" else 3
    path, amb = T.MODES[mode]
    log, _, _, _ = oracle.log_launch(T.scene_of(oracle, t), oracle.frame(w, h, 1, 0, path=path, ambient=amb, mode=1, max_depth=md))
    ctx = make_ctx(capi, t, w * h)
    total = 0
    for k in range(1, md + 1):
        node = log[(log["kind"] == S.RADIANCE) & (log["depth"] == k)]
        assert len(node) > 100, (name, mode, k, len(node))
        rays = capi.make_rays(node["o"], node["d"], node["tmin"], node["tmax"])
        acc, img = ctx.shade_rays(rays, node["seed"], path, amb, md - k, 0)
        finite = np.isfinite(node["d"]).all(1) & np.isfinite(node["o"]).all(1)
        assert not bits(acc[~finite]).any() and not img[~finite].any(), "a ray that is not finite comes back invalid"
        assert (np.abs((node["d"][finite].astype(np.float64) ** 2).sum(1) - 1.0) <= 1e-5).all()
        assert (acc[finite][:, 3] == 1.0).all()
        m = parity.assert_parity(acc[finite], node["payload"][finite], what="%s %s depth %d" % (name, mode, k))
        print(name, mode, "depth", k, "nodes", len(node), "not finite", int((~finite).sum()), m)
        total += len(node)
    assert total > 1000
    ctx.close()


# ---- 4. mechanics -------------------------------------------------------------------------------------------------------------------------
def room_case(capi, oracle, mode="distributed"):
    t, w, h = tables(oracle, "room")
    ctx = make_ctx(capi, t, w * h)
    o, d, seed = R.raygen32(t["cam"], w, h, 0)
    path, amb = T.MODES[mode]
    return t, ctx, capi.make_rays(o, d, TMIN, TMAX), seed, (path, amb)


@pytest.mark.parametrize("mode", ["path", "distributed"])
def test_batch_shape_and_order(capi, oracle, mode):
    import torch
    t, ctx, rays, seed, (path, amb) = room_case(capi, oracle, mode)
    base = ctx.shade_rays(rays, seed, path, amb)
    perm = np.random.RandomState(1).permutation(len(rays))
    for knob in (None, 0, 1):
        with Knob(RTGO_TRACE_MODE=knob):
            for n in (1, 63, 64, 65, 257):
                assert same(ctx.shade_rays(rays[:n], seed[:n], path, amb), (base[0][:n], base[1][:n])), ("batch of %d" % n, knob)
            assert same(ctx.shade_rays(rays[perm], seed[perm], path, amb), (base[0][perm], base[1][perm])), ("shuffled rays", knob)
            with Knob(RTGO_TRACE_BLOCKS=1):   # one workgroup of at most 1024 lanes: three trips of the loop at the least
                big_r, big_s = np.tile(rays, 2)[:2049], np.tile(seed, 2)[:2049]
                assert same(ctx.shade_rays(big_r, big_s, path, amb), (np.tile(base[0], (2, 1))[:2049], np.tile(base[1], (2, 1))[:2049])), ("grid-stride loop", knob)
    # torch device tensors are shaded where they are; an empty batch is an empty answer
    dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).to("cuda:0")
    dev_seed = torch.from_numpy(seed.view(np.int32)).to("cuda:0")
    assert same(ctx.shade_rays(dev, dev_seed, path, amb), base)
    assert same(ctx.shade_rays(dev, seed, path, amb), base)
    acc, img = ctx.shade_rays(rays[:0], seed[:0], path, amb)
    assert acc.shape == (0, 4) and img.shape == (0, 4)
    ctx.close()


def test_invalid_rays(capi, oracle):
    import torch
    t, ctx, rays, seed, (path, amb) = room_case(capi, oracle)
    n = len(rays)
    alone = ctx.shade_rays(rays, seed, path, amb)
    bad = rays.copy()
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    ks = np.array([0, 63, 64, 65, 66, 700, 701])
    bad["dir"][0] = 0                                   # dir == 0
    bad["origin"][63] = (0, nan, 0)                     # a component that is not finite
    bad["tmax"][64] = bad["tmin"][64]                   # tmax <= tmin
    bad["tmin"][65] = -1                                # tmin < 0
    bad["tmax"][66] = nan                               # tmax NaN
    bad["dir"][700] = bad["dir"][700] * np.float32(1.01)    # not a unit vector
    bad["dir"][701] = (1, inf, 0)
    keep = np.ones(n, bool)
    keep[ks] = False
    got = ctx.shade_rays(bad, seed, path, amb)
    assert not bits(got[0][ks]).any() and not got[1][ks].any()
    assert same((got[0][keep], got[1][keep]), (alone[0][keep], alone[1][keep])), "the neighbours of invalid rays"
    # sample 1: both buffers are left as they were at an invalid ray, and folded everywhere else
    prev = np.random.RandomState(3).uniform(0.0, 1.0, (n, 4)).astype(np.float32)
    d_rays = torch.from_numpy(bad.view(np.float32).reshape(-1, 8)).to("cuda:0")
    d_seed = torch.from_numpy(seed.view(np.int32)).to("cuda:0")
    d_acc = torch.from_numpy(prev).to("cuda:0")
    d_img = torch.full((n, 4), 77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    opt = capi.ShadeOptions(5, int(path), int(amb), 1)
    assert ctx.shade_rays_raw(d_rays.data_ptr(), d_seed.data_ptr(), d_acc.data_ptr(), d_img.data_ptr(), n, opt) == RTGO_OK
    ctx.sync()
    acc1, img1 = d_acc.cpu().numpy(), d_img.cpu().numpy()
    assert np.array_equal(bits(acc1[ks]), bits(prev[ks])) and (img1[ks] == 77).all()
    want1 = ctx.shade_rays(rays, seed, path, amb, 5, 1, prev)
    assert same((acc1[keep], img1[keep]), (want1[0][keep], want1[1][keep])) and not (img1[keep] == 77).all(axis=1).any()
    ctx.close()


@pytest.mark.parametrize("mode", ["path", "distributed"])
def test_window_at_the_device_s_t(capi, oracle, mode):
    t, ctx, rays, seed, (path, amb) = room_case(capi, oracle, mode)
    alone = ctx.shade_rays(rays, seed, path, amb)
    hits = ctx.trace_rays(rays)
    hh = hits["prim"] >= 0
    th = hits["t"][hh]
    assert hh.sum() > 0.9 * len(rays)
    o, d = rays["origin"][hh], rays["dir"][hh]
    bg4 = np.append(np.float32(t["bg"]), np.float32(1.0))
    closed = ctx.shade_rays(capi.make_rays(o, d, TMIN, th), seed[hh], path, amb)
    assert np.array_equal(bits(closed[0]), bits(np.tile(bg4, (hh.sum(), 1)))), "tmax = t: the hit is outside the window"
    assert same(ctx.shade_rays(capi.make_rays(o, d, TMIN, np.nextafter(th, np.float32(np.inf))), seed[hh], path, amb), (alone[0][hh], alone[1][hh]))
    # no image asked for: the same accumulation
    acc, img = ctx.shade_rays(rays, seed, path, amb, image=False)
    assert img is None and np.array_equal(bits(acc), bits(alone[0]))
    ctx.close()


@pytest.mark.parametrize("k", [1, 5, 1000])
def test_later_samples_fold_like_the_host(capi, oracle, k):
    t, ctx, rays, seed, (path, amb) = room_case(capi, oracle)
    r = ctx.shade_rays(rays, seed, path, amb)[0][:, :3]
    prev = np.random.RandomState(k).uniform(0.0, 1.5, (len(rays), 4)).astype(np.float32)
    acc, img = ctx.shade_rays(rays, seed, path, amb, 5, k, prev)
    a = np.float32(1.0) / np.float32(k + 1)
    want = prev[:, :3] + (r - prev[:, :3]) * a
    assert want.dtype == np.float32
    assert np.array_equal(bits(acc[:, :3]), bits(want)) and (acc[:, 3] == 1.0).all()
    byte = (np.clip(want, np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)      # make_color in float32: clamp, scale, truncate
    assert np.array_equal(img[:, :3], byte) and (img[:, 3] == 255).all()
    ctx.close()


def test_refusals_write_nothing(capi, oracle):
    import torch
    import test_oracle_whitted_float64 as TW
    from test_whitted_shading_float64 import _ctx as whitted_ctx
    t, w, h = tables(oracle, "room")
    buf = torch.full((320, 8), 1234.5, dtype=torch.float32, device="cuda:0")
    rays, acc, img, seeds = buf[:64].data_ptr(), buf[64:128].data_ptr(), buf[128:192].data_ptr(), buf[192:].data_ptr()
    assert rays % 16 == 0 and acc % 16 == 0 and img % 4 == 0 and seeds % 4 == 0
    torch.cuda.synchronize()
    ok = capi.ShadeOptions(5, 1, 0, 0)
    dist = capi.ShadeOptions(5, 0, 0, 0)
    ctx = capi.Context(0)
    assert ctx.shade_rays_raw(rays, seeds, acc, img, 4, ok) == RTGO_E_STATE                  # no scene at all
    ctx.close()
    ctx = whitted_ctx(capi, TW.scene("sweep"), False)
    assert ctx.shade_rays_raw(rays, seeds, acc, img, 4, ok) == RTGO_E_STATE                  # a whitted scene alone does not count
    assert ctx.shade_rays_raw(rays, seeds, acc, img, 0, ok) == RTGO_E_STATE
    ctx.close()
    ctx = make_ctx(capi, t, w * h, lights=False)
    s0 = ctx.stats()
    assert ctx.shade_rays_raw(rays, seeds, acc, img, 4, dist) == RTGO_E_STATE                # distributed mode without a surface light
    assert ctx.shade_rays_raw(rays, seeds, acc, img, 4, capi.ShadeOptions(5, 0, 1, 0)) == RTGO_E_STATE
    L = capi.load()
    assert L.rtgo_shade_rays(None, rays, seeds, acc, img, 4, C.byref(ok)) == RTGO_E_INVALID  # NULL ctx
    assert ctx.shade_rays_raw(0, seeds, acc, img, 4, ok) == RTGO_E_INVALID
    assert ctx.shade_rays_raw(rays, seeds, 0, img, 4, ok) == RTGO_E_INVALID
    assert ctx.shade_rays_raw(rays, seeds, acc, img, 4, None) == RTGO_E_INVALID
    assert ctx.shade_rays_raw(rays + 4, seeds, acc, img, 4, ok) == RTGO_E_INVALID
    assert ctx.shade_rays_raw(rays, seeds, acc + 8, img, 4, ok) == RTGO_E_INVALID
    assert ctx.shade_rays_raw(rays, seeds + 2, acc, img, 4, ok) == RTGO_E_INVALID
    assert ctx.shade_rays_raw(rays, seeds, acc, img + 2, 4, ok) == RTGO_E_INVALID
    assert ctx.shade_rays_raw(rays, seeds, acc, img + 1, 4, ok) == RTGO_E_INVALID
    assert ctx.shade_rays_raw(rays, seeds, acc, img, (1 << 30) + 1, ok) == RTGO_E_INVALID
    assert ctx.shade_rays_raw(rays, 0, acc, 0, (1 << 30) + 1, ok) == RTGO_E_INVALID
    assert ctx.shade_rays_raw(rays, seeds, acc, img, 4, capi.ShadeOptions(5, 2, 0, 0)) == RTGO_E_INVALID
    assert ctx.shade_rays_raw(rays, seeds, acc, img, 4, capi.ShadeOptions(5, 1, 2, 0)) == RTGO_E_INVALID
    assert ctx.shade_rays_raw(rays, seeds, acc, img, 4, capi.ShadeOptions(5, 0xFFFFFFFF, 0, 0)) == RTGO_E_INVALID
    assert ctx.shade_rays_raw(rays, seeds, acc, img, 4, capi.ShadeOptions(6, 1, 0, 0)) == RTGO_E_UNSUPPORTED
    assert ctx.shade_rays_raw(rays, seeds, acc, img, 4, capi.ShadeOptions(-1, 1, 0, 0)) == RTGO_E_UNSUPPORTED
    assert ctx.shade_rays_raw(rays, seeds, acc, img, 0, ok) == RTGO_OK                       # nothing to do
    assert ctx.shade_rays_raw(rays, 0, acc, 0, 0, capi.ShadeOptions(0, 1, 1, 3)) == RTGO_OK
    ctx.sync()
    torch.cuda.synchronize()
    assert (buf == 1234.5).all().item(), "a refused call wrote something"
    s1 = ctx.stats()
    for k in s0:
        assert s1[k] == s0[k], k
    # ... and the context still works: four rays that leave the room's lamp side upwards from outside, image 4 bytes into its buffer
    buf[0:4] = torch.tensor([0.0, 50.0, 0.0, 0.05, 0.0, 1.0, 0.0, 1e16], dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx.shade_rays_raw(rays, 0, acc, img + 4, 4, ok) == RTGO_OK
    ctx.sync()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[64:66].reshape(4, 4), np.tile(np.append(np.float32(t["bg"]), np.float32(1.0)), (4, 1)))
    image = got[128:192].view(np.uint8).reshape(-1, 4)
    assert np.array_equal(image[1:5], np.tile([0, 0, 0, 255], (4, 1)))      # (the room's background is black)
    assert (got[4:64] == 1234.5).all() and (got[66:128] == 1234.5).all() and got[128, 0] == 1234.5 and (got[128, 5:] == 1234.5).all() and (got[129:] == 1234.5).all()
    assert ctx.stats()["rays_total"] == s0["rays_total"] + 4 and ctx.stats()["rays_occlusion"] == s0["rays_occlusion"]
    ctx.close()


@pytest.mark.parametrize("mode", ["path", "distributed"])
def test_launches_are_left_alone(capi, oracle, mode):
    t, w, h = tables(oracle, "cornell")
    path, amb = T.MODES[mode]
    plain = make_ctx(capi, t, w * h)
    want = launch_frames(capi, plain, w, h, mode, 5)
    plain.close()
    ctx = make_ctx(capi, t, w * h)
    o, d = R.latlong(t["cam"], w, h)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    first = ctx.shade_rays(rays, None, path, amb)

    def between(f):
        st = ctx.stats()
        assert same(ctx.shade_rays(rays, None, path, amb), first), "the shade call after launch %d" % f
        after = ctx.stats()
        for k in ("launches", "launches_trial", "launches_canonical", "last_variant", "last_launch_ms", "total_launch_ms"):
            assert after[k] == st[k], k

    got = launch_frames(capi, ctx, w, h, mode, 5, between=between)
    assert_frames_equal(got, want, "launches with shade calls between them")
    for g, x in zip(got, want):
        for k in ("launches", "launches_trial", "last_variant"):
            assert g[4][k] == x[4][k], k
    ctx.close()
