"""The triangle path's shading on the MI355X against tests/whitted_ref64.py: the three scenes of tests/whitted_shading_scenes.py held to
the float64 reference with the constants and the checks of tests/test_oracle_whitted_float64.py -- the device gets no bound of its own --
and the residency forms, the two-level form and a band split of them bitwise one frame."""
import numpy as np
import pytest

import whitted_ref64 as R
import whitted_shading_scenes as S
import test_oracle_whitted_float64 as T

pytestmark = pytest.mark.gpu

W, H = S.W, S.H


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import capi as m
    m.load()
    return m


def _ctx(capi, sc, instanced):
    """a context over the scene: rtgo_whitted_set_mesh on its one mesh, or rtgo_whitted_set_scene"""
    ctx = capi.Context(0)
    if instanced:
        ctx.whitted_set_scene(sc["meshes"], sc["instances"], sc["materials"])
    else:
        mesh = S.flat_mesh(sc)
        ctx.whitted_set_mesh(mesh["positions"], mesh.get("normals"), mesh["indices"], mesh.get("tri_material"), mesh["materials"])
        if mesh.get("texcoords") is not None:
            ctx.whitted_set_texcoords(mesh["texcoords"])
    for mi, (bc, mr, nm) in (sc["textures"] or {}).items():
        ctx.whitted_set_material_textures(mi, bc, mr, nm)
    ctx.whitted_set_lights(sc["lights"])
    ctx.whitted_set_miss_color(sc["miss"])
    cam = sc["cam"]
    ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])
    ctx.resize(W * H)
    return ctx


def _frames(ctx):
    """[(accum, image)] after 1, 2, 3 subframes, and subframe 0's (rays_total, rays_occlusion)"""
    out, rays0 = [], None
    ctx.reset_stats()
    for sf in range(S.SUBFRAMES):
        ctx.whitted_launch(W, H, sf)
        ctx.sync()
        if sf == 0:
            st = ctx.stats()
            rays0 = {"rays_total": st["rays_total"], "rays_occlusion": st["rays_occlusion"]}
        out.append((ctx.read_accum(H, W), ctx.read_image(H, W)))
    return out, rays0


def _same(a, b, what):
    for (acc_a, img_a), (acc_b, img_b) in zip(a, b):
        assert np.array_equal(acc_a.view(np.uint32), acc_b.view(np.uint32)), what + ": accumulation differs"
        assert np.array_equal(img_a, img_b), what + ": image differs"


def _against_float64(capi, name, sc, instanced):
    """the checks of test_oracle_whitted_float64.test_pipeline_against_float64 on the device's frames; returns them"""
    ref = T.reference(name)
    lit, shadow, unclear = T.check_conditions(name, ref)
    ctx = _ctx(capi, sc, instanced)
    frames, rays0 = _frames(ctx)
    # subframe 0's primaries through rtgo_whitted_trace_rays: the float64 brute force's (instance, triangle) on the clear rays
    o, d = R.primaries32(sc["cam"], W, H)
    hits = ctx.whitted_trace_rays(capi.make_rays(o, d, np.float32(0.01), np.float32(1e16)))
    rows = np.nonzero((ref[0]["clear"] & ref[0]["hit"]).reshape(-1))[0]
    key = ref[0]["key"].reshape(-1, 2)[rows]
    assert np.array_equal(hits["prim"][rows], key[:, 1].astype(np.int32)) and np.array_equal(hits["instance"][rows], key[:, 0].astype(np.int32)), "closest hit"
    clear_miss = np.nonzero((ref[0]["clear"] & ~ref[0]["hit"]).reshape(-1))[0]
    assert (hits["prim"][clear_miss] == capi.HIT_MISS).all()
    T.check_light_pattern(name, frames[0][0], ref[0])
    lo, hi = T.occlusion_ray_bounds(ref[0])
    assert rays0["rays_total"] - W * H == rays0["rays_occlusion"] and lo <= rays0["rays_occlusion"] <= hi, (rays0, lo, hi)
    T.check_miss(name, frames, ref, sc["miss"])
    for s, (acc, img) in enumerate(frames):
        worst, same8 = T.check_frame(name, acc, img, ref[s], sc["miss"], "subframes 0 .. %d" % s)
        print("%s (%s), subframes 0 .. %d: unclear %.4f of the hit pixels, largest dev %.2f (bound %.1f), 8-bit identical %.4f"
              % (name, "set_scene" if instanced else "set_mesh", s, unclear, worst, T.BOUND["pipeline"], same8))
    ctx.close()
    return frames


@pytest.mark.parametrize("name", ["textured", "textured_nouv"])
def test_textured_against_float64(capi, name):
    _against_float64(capi, name, T.scene(name), False)


def test_sweep_against_float64_in_every_form(capi, monkeypatch):
    """rtgo_whitted_set_mesh and one identity instance through rtgo_whitted_set_scene, both against the reference; the residency forms
    RTGO_WHITTED_MODE 0, 1, 2 bitwise that frame; subframes 0 .. 2 as two interleaved row bands (rtgo_whitted_launch_frame) put back
    together bitwise the full frame"""
    sc = T.scene("sweep")
    base = _against_float64(capi, "sweep", sc, False)
    _against_float64(capi, "sweep", sc, True)
    for mode in ("0", "1", "2"):
        monkeypatch.setenv("RTGO_WHITTED_MODE", mode)
        ctx = _ctx(capi, sc, False)
        _same(_frames(ctx)[0], base, "sweep, RTGO_WHITTED_MODE=" + mode)
        ctx.close()
    monkeypatch.delenv("RTGO_WHITTED_MODE", raising=False)
    # two shares of 8-row bands
    from raytracingo_amd import bands as B
    ctx = _ctx(capi, sc, False)
    acc, img = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.uint8)
    for g in range(2):
        rows = B.band_rows(H, 8, 2, g)
        assert len(rows) == capi.local_rows(H, 8, 2, g) == H // 2
        ctx.resize(len(rows) * W)
        for sf in range(S.SUBFRAMES):
            ctx.whitted_launch_frame(capi.make_whitted_frame(W, H, sf, bands=(8, 2, g)))
        ctx.sync()
        acc[rows], img[rows] = ctx.read_accum(len(rows), W), ctx.read_image(len(rows), W)
    ctx.close()
    _same([(acc, img)], [base[-1]], "sweep, two row bands")


def test_instanced_against_float64_in_both_forms(capi, monkeypatch):
    """the six instances against the reference; the top level in LDS (RTGO_WHITTED_MODE=2) and through L2 (0) bitwise that frame"""
    sc = T.scene("instanced")
    base = _against_float64(capi, "instanced", sc, True)
    for mode in ("2", "0"):
        monkeypatch.setenv("RTGO_WHITTED_MODE", mode)
        ctx = _ctx(capi, sc, True)
        _same(_frames(ctx)[0], base, "instanced, RTGO_WHITTED_MODE=" + mode)
        ctx.close()
    monkeypatch.delenv("RTGO_WHITTED_MODE", raising=False)
