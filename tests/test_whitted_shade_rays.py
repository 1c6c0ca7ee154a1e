"""rtgo_whitted_shade_rays on the MI355X: the triangle path's closest-hit and miss programs for rays of the caller's own.

Held two ways.  Bit for bit to rtgo_whitted_launch, on the launch's own rays made on the host (whitted_shade_rays_ref.raygen32): both
buffers after every subframe, and the ray counts -- over one mesh, instances, a clustered mesh, a refitted mesh, with the top level in
LDS and through L2.  And to the float64 reference of tests/whitted_ref64.py on a camera the launches do not have (an orthographic view,
directions not of unit length), with the bound and the 8-bit rule of test_oracle_whitted_float64.check_frame: the device gets no bound of
its own.  Then the call's own edges: batch shapes, invalid rays, the window at the device's t, the fold at later samples, refusals, and
launches left as they were."""
import numpy as np
import pytest

import whitted_big_meshes as BM
import whitted_instances as WI
import whitted_ref64 as R
import whitted_shade_rays_ref as SR
import whitted_shading_scenes as S
import test_oracle_whitted_float64 as T
from test_trace_rays import Knob
from test_whitted_shading_float64 import _ctx, _frames, _same

pytestmark = pytest.mark.gpu

W, H = S.W, S.H
TMIN, TMAX = SR.TMIN, SR.TMAX
RTGO_OK, RTGO_E_INVALID, RTGO_E_STATE = 0, 1, 3


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


def pinhole(capi, cam, s, w=W, h=H):
    o, d = SR.raygen32(cam, w, h, s)
    return capi.make_rays(o, d, TMIN, TMAX)


def shaded_frames(capi, ctx, cam, n=S.SUBFRAMES, w=W, h=H):
    """what _frames returns for launches, through the new call: [(accum, image)] after 1 .. n samples of the host raygen's rays folded
    into one pair of buffers, and sample 0's (rays_total, rays_occlusion)"""
    out, rays0, acc = [], None, None
    ctx.reset_stats()
    for s in range(n):
        acc, img = ctx.whitted_shade_rays(pinhole(capi, cam, s, w, h), s, acc)
        if s == 0:
            st = ctx.stats()
            rays0 = {"rays_total": st["rays_total"], "rays_occlusion": st["rays_occlusion"]}
        out.append((acc.reshape(h, w, 4), img.reshape(h, w, 4)))
    return out, rays0


# ---- 1. pinhole rays are the launch, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,instanced", [("sweep", False), ("sweep", True), ("textured", False), ("textured_nouv", False), ("instanced", True)])
def test_pinhole_rays_are_the_launch(capi, name, instanced):
    sc = T.scene(name)
    ctx = _ctx(capi, sc, instanced)
    want, want_rays = _frames(ctx)
    got, got_rays = shaded_frames(capi, ctx, sc["cam"])
    _same(got, want, "%s: shaded pinhole rays against the launch" % name)
    assert got_rays == want_rays and got_rays["rays_occlusion"] > 0, (got_rays, want_rays)
    if name == "instanced":
        for mode in (0, 1):
            with Knob(RTGO_TRACE_MODE=mode):
                _same(shaded_frames(capi, ctx, sc["cam"])[0], want, "instanced, RTGO_TRACE_MODE=%d" % mode)
    ctx.close()


# ---- 2. orthographic rays against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sweep", "textured", "textured_nouv", "instanced"])
def test_orthographic_rays_against_float64(capi, name):
    sc, o, d, ref = SR.ortho_case(name)
    ctx = _ctx(capi, sc, name == "instanced")
    acc, img = ctx.whitted_shade_rays(capi.make_rays(o, d, TMIN, TMAX))
    acc, img = acc.reshape(H, W, 4), img.reshape(H, W, 4)
    d64 = np.where(ref["clear"][..., None], R.dev(acc[..., :3], ref["color"], ref["kappa"]), 0.0)
    print("%s, orthographic: largest dev %.2f (bound %.1f)" % (name, d64.max(), T.BOUND["pipeline"]))
    worst, same8 = T.check_frame(name, acc, img, ref, sc["miss"], "orthographic")
    print("%s, orthographic: largest dev %.2f (bound %.1f), 8-bit identical %.4f" % (name, worst, T.BOUND["pipeline"], same8))
    missed = ref["clear"] & ~ref["hit"]
    assert missed.mean() > 0.02
    assert np.array_equal(bits(acc[missed]), bits(np.tile(np.append(np.float32(sc["miss"]), np.float32(1.0)), (missed.sum(), 1))))
    ctx.close()


# ---- 3. a clustered mesh ----------------------------------------------------------------------------------------------------------------
def test_clustered_mesh_is_the_launch_and_the_callers_cut(capi):
    """a displaced torus of 8320 triangles (beyond RTGO_MAX_TRIANGLES: a clustered mesh) over a ground: the three-level walk"""
    torus = BM.displaced_torus(65, 64, texcoords=False)
    assert len(torus["indices"]) == 8320
    meshes = [WI.ground(3.0, -0.35, normals=True), torus]
    inst = [(S.EYE34, 0, 2), (S.EYE34, 1, 0)]
    extra = WI.lights()
    sc = {"meshes": meshes, "instances": inst, "materials": WI.materials(), "textures": None, "lights": extra["lights"], "miss": extra["miss"],
          "cam": S.camera((0.6, 1.5, 2.2), (0.0, -0.1, 0.0), 45.0, W / H)}
    ctx = _ctx(capi, sc, True)
    want, want_rays = _frames(ctx)
    for mode in (None, 0, 1):
        with Knob(RTGO_TRACE_MODE=mode):
            got, got_rays = shaded_frames(capi, ctx, sc["cam"])
        _same(got, want, "clustered, RTGO_TRACE_MODE=%s: shaded pinhole rays against the launch" % mode)
        assert got_rays == want_rays and got_rays["rays_occlusion"] > 0
    hit = (want[0][0][..., :3] != np.float32(sc["miss"])).any(axis=-1)
    assert hit.mean() > 0.3
    cmeshes, cinst = BM.chunked_scene(meshes, inst, big={1})
    assert len(cinst) == 3
    cut = _ctx(capi, dict(sc, meshes=cmeshes, instances=cinst), True)
    _same(shaded_frames(capi, cut, sc["cam"])[0], got, "clustered: against the caller's cut")
    ctx.close()
    cut.close()


# ---- 4. batch shape ---------------------------------------------------------------------------------------------------------------------
def test_batch_shape_and_order(capi):
    import torch
    sc, o, d, ref = SR.ortho_case("instanced")
    ctx = _ctx(capi, sc, True)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    base = ctx.whitted_shade_rays(rays)
    assert (base[0][:, :3] != np.float32(sc["miss"])).any(axis=1).mean() > 0.4
    perm = np.random.RandomState(1).permutation(len(rays))
    for mode in (None, 0, 1):
        with Knob(RTGO_TRACE_MODE=mode):
            for n in (1, 63, 64, 65, 257):
                assert same(ctx.whitted_shade_rays(rays[:n]), (base[0][:n], base[1][:n])), ("batch of %d" % n, mode)
            assert same(ctx.whitted_shade_rays(rays[perm]), (base[0][perm], base[1][perm])), ("shuffled rays", mode)
            with Knob(RTGO_TRACE_BLOCKS=2):   # workgroups of 256 lanes: two passes and one ray
                assert same(ctx.whitted_shade_rays(rays[:1025]), (base[0][:1025], base[1][:1025])), ("grid-stride loop", mode)
    # a torch device tensor is shaded where it is; an empty batch is an empty answer
    dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).to("cuda:0")
    assert same(ctx.whitted_shade_rays(dev), base)
    acc, img = ctx.whitted_shade_rays(rays[:0])
    assert acc.shape == (0, 4) and img.shape == (0, 4)
    ctx.close()


# ---- 5. invalid rays and the window -----------------------------------------------------------------------------------------------------
def test_invalid_rays_and_window(capi):
    import torch
    sc, o, d, ref = SR.ortho_case("instanced")
    ctx = _ctx(capi, sc, True)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    n = len(rays)
    alone = ctx.whitted_shade_rays(rays)
    bad = rays.copy()
    nan = np.float32(np.nan)
    ks = np.array([0, 63, 64, 65, 700])
    bad["dir"][0] = 0
    bad["origin"][63] = (0, nan, 0)
    bad["tmax"][64] = bad["tmin"][64]
    bad["tmin"][65] = -1
    bad["tmax"][700] = nan
    keep = np.ones(n, bool)
    keep[ks] = False
    # sample 0: zeros, alpha too
    got = ctx.whitted_shade_rays(bad)
    assert not bits(got[0][ks]).any() and not got[1][ks].any()
    assert same((got[0][keep], got[1][keep]), (alone[0][keep], alone[1][keep])), "the neighbours of invalid rays"
    # sample 1: both buffers are left as they were at an invalid ray, and folded everywhere else
    prev = np.random.RandomState(3).uniform(0.0, 1.0, (n, 4)).astype(np.float32)
    d_rays = torch.from_numpy(bad.view(np.float32).reshape(-1, 8)).to("cuda:0")
    d_acc = torch.from_numpy(prev).to("cuda:0")
    d_img = torch.full((n, 4), 77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx.whitted_shade_rays_raw(d_rays.data_ptr(), d_acc.data_ptr(), d_img.data_ptr(), n, 1) == RTGO_OK
    ctx.sync()
    acc1, img1 = d_acc.cpu().numpy(), d_img.cpu().numpy()
    assert np.array_equal(bits(acc1[ks]), bits(prev[ks])) and (img1[ks] == 77).all()
    want1 = ctx.whitted_shade_rays(rays, 1, prev)
    assert same((acc1[keep], img1[keep]), (want1[0][keep], want1[1][keep])) and not (img1[keep] == 77).all(axis=1).any()
    # the window at the device's own t (rtgo_whitted_trace_rays runs the same walk)
    hits = ctx.whitted_trace_rays(rays)
    h = hits["prim"] >= 0
    th = hits["t"][h]
    assert h.sum() > 0.4 * n
    miss4 = np.append(np.float32(sc["miss"]), np.float32(1.0))
    closed = ctx.whitted_shade_rays(capi.make_rays(o[h], d[h], TMIN, th))
    assert np.array_equal(bits(closed[0]), bits(np.tile(miss4, (h.sum(), 1)))), "tmax = t: the hit is outside the window"
    assert same(ctx.whitted_shade_rays(capi.make_rays(o[h], d[h], TMIN, np.nextafter(th, np.float32(np.inf)))), (alone[0][h], alone[1][h]))
    assert np.array_equal(bits(alone[0][~h]), bits(np.tile(miss4, ((~h).sum(), 1))))
    # no image asked for: the same accumulation
    acc, img = ctx.whitted_shade_rays(rays, image=False)
    assert img is None and np.array_equal(bits(acc), bits(alone[0]))
    ctx.close()


# ---- 6. continuation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 1000])
def test_later_samples_fold_like_the_host(capi, k):
    sc, o, d, ref = SR.ortho_case("sweep")
    ctx = _ctx(capi, sc, False)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    r = ctx.whitted_shade_rays(rays)[0][:, :3]
    prev = np.random.RandomState(k).uniform(0.0, 1.5, (len(rays), 4)).astype(np.float32)
    acc, img = ctx.whitted_shade_rays(rays, k, prev)
    a = np.float32(1.0) / np.float32(k + 1)
    want = prev[:, :3] + (r - prev[:, :3]) * a
    assert want.dtype == np.float32
    assert np.array_equal(bits(acc[:, :3]), bits(want)) and (acc[:, 3] == 1.0).all()
    byte, exact = R.make_color(want.astype(np.float64))
    diff = np.abs(img[:, :3].astype(np.int64) - byte.astype(np.int64))
    assert (diff[exact] == 0).all() and (diff <= 1).all() and (img[:, 3] == 255).all()
    ctx.close()


# ---- 7. after rtgo_whitted_update_mesh --------------------------------------------------------------------------------------------------
def test_after_update_mesh(capi):
    rng = np.random.RandomState(9)
    torus = WI.torus(16, 8)
    meshes = [WI.ground(normals=True), torus]
    inst = [(WI.transform(np.eye(3), [0, 0, 0]), 0, 0), (WI.transform(np.eye(3), [-1.5, 0.6, 0.5]), 1, 1),
            (WI.transform(WI.rotation(rng) @ np.diag([1.6, 0.5, 1.0]), [0.2, 1.0, -0.5]), 1, 2)]
    extra = WI.lights()
    sc = {"meshes": meshes, "instances": inst, "materials": WI.materials(), "textures": None, "lights": extra["lights"], "miss": extra["miss"],
          "cam": S.camera((0.5, 3.5, 6.0), (0.0, 0.6, 0.0), 45.0, W / H)}
    ctx = _ctx(capi, sc, True)
    before = _frames(ctx)[0]
    _same(shaded_frames(capi, ctx, sc["cam"])[0], before, "before the update")
    # the torus twisted about its axis and bent along its normals
    p = torus["positions"].astype(np.float64)
    ang = 1.2 * p[:, 1]
    twisted = np.stack([np.cos(ang) * p[:, 0] - np.sin(ang) * p[:, 2], p[:, 1], np.sin(ang) * p[:, 0] + np.cos(ang) * p[:, 2]], 1)
    twisted = (twisted + 0.08 * np.sin(9.0 * p[:, [2, 0, 1]]) * torus["normals"]).astype(np.float32)
    ctx.whitted_update_mesh(1, twisted)
    after = _frames(ctx)[0]
    assert not np.array_equal(after[0][1], before[0][1])
    _same(shaded_frames(capi, ctx, sc["cam"])[0], after, "after the update")
    ctx.close()


# ---- 8. refusals through the raw call ---------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(capi, oracle):
    import torch
    sc = T.scene("sweep")
    buf = torch.full((256, 8), 1234.5, dtype=torch.float32, device="cuda:0")
    rays, acc, img = buf[:64].data_ptr(), buf[64:128].data_ptr(), buf[128:].data_ptr()
    assert rays % 16 == 0 and acc % 16 == 0 and img % 4 == 0
    torch.cuda.synchronize()
    ctx = capi.Context(0)
    assert ctx.whitted_shade_rays_raw(rays, acc, img, 4) == RTGO_E_STATE                 # no scene at all
    t = oracle.scene_tables(oracle.scene("cornell", 32, 24))
    ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
    assert ctx.whitted_shade_rays_raw(rays, acc, img, 4) == RTGO_E_STATE                 # an analytic scene is no mesh
    assert ctx.whitted_shade_rays_raw(rays, acc, img, 0) == RTGO_E_STATE
    ctx.close()
    ctx = _ctx(capi, sc, False)
    s0 = ctx.stats()
    L = capi.load()
    assert L.rtgo_whitted_shade_rays(None, rays, acc, img, 4, 0) == RTGO_E_INVALID       # NULL ctx
    assert ctx.whitted_shade_rays_raw(0, acc, img, 4) == RTGO_E_INVALID
    assert ctx.whitted_shade_rays_raw(rays, 0, img, 4) == RTGO_E_INVALID
    assert ctx.whitted_shade_rays_raw(rays + 4, acc, img, 4) == RTGO_E_INVALID
    assert ctx.whitted_shade_rays_raw(rays, acc + 8, img, 4) == RTGO_E_INVALID
    assert ctx.whitted_shade_rays_raw(rays, acc, img + 2, 4) == RTGO_E_INVALID
    assert ctx.whitted_shade_rays_raw(rays, acc, img + 1, 4) == RTGO_E_INVALID
    assert ctx.whitted_shade_rays_raw(rays, acc, img, (1 << 30) + 1) == RTGO_E_INVALID
    assert ctx.whitted_shade_rays_raw(rays, acc, 0, (1 << 30) + 1, 7) == RTGO_E_INVALID
    assert ctx.whitted_shade_rays_raw(rays, acc, img, 0) == RTGO_OK                      # nothing to do
    assert ctx.whitted_shade_rays_raw(rays, acc, img, 0, 3) == RTGO_OK
    ctx.sync()
    torch.cuda.synchronize()
    assert (buf == 1234.5).all().item(), "a refused call wrote something"
    s1 = ctx.stats()
    for k in ("rays_total", "rays_occlusion", "launches", "last_launch_ms", "last_variant"):
        assert s1[k] == s0[k], k
    # ... and the context still works: four rays that leave the plane upwards, image 4 bytes into its buffer
    buf[0:4] = torch.tensor([0.0, 5.0, 0.0, 0.01, 0.0, 1.0, 0.0, 1e16], dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx.whitted_shade_rays_raw(rays, acc, img + 4, 4) == RTGO_OK
    ctx.sync()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[64:66].reshape(4, 4), np.tile(np.append(np.float32(sc["miss"]), np.float32(1.0)), (4, 1)))
    image = got[128:].view(np.uint8).reshape(-1, 4)
    assert np.array_equal(image[1:5], np.tile(R.make_color(np.float32(sc["miss"]).astype(np.float64))[0].tolist() + [255], (4, 1)))
    assert (got[4:64] == 1234.5).all() and (got[66:128] == 1234.5).all() and got[128, 0] == 1234.5 and (got[128, 5:] == 1234.5).all() and (got[129:] == 1234.5).all()
    assert ctx.stats()["rays_total"] == s0["rays_total"] + 4 and ctx.stats()["rays_occlusion"] == s0["rays_occlusion"]
    ctx.close()


# ---- 9. no interference -----------------------------------------------------------------------------------------------------------------
def test_launches_are_left_alone(capi):
    sc, o, d, ref = SR.ortho_case("instanced")
    rays = capi.make_rays(o, d, TMIN, TMAX)
    ctx = _ctx(capi, sc, True)
    want, _ = _frames(ctx)
    first = ctx.whitted_shade_rays(rays)
    ctx.reset_stats()
    s0 = ctx.stats()
    got = []
    for s in range(S.SUBFRAMES):
        ctx.whitted_launch(W, H, s)
        ctx.sync()
        got.append((ctx.read_accum(H, W), ctx.read_image(H, W)))
        st = ctx.stats()
        assert same(ctx.whitted_shade_rays(rays), first), "the shade call between launches %d and %d" % (s, s + 1)
        after = ctx.stats()
        for k in ("launches", "last_launch_ms", "last_variant", "total_launch_ms"):
            assert after[k] == st[k], k
        assert after["launches"] == s0["launches"] + s + 1
    _same(got, want, "launches with shade calls between them")
    ctx.close()
