"""rtgo_whitted_launch_frames on the MI355X: n subframes of a window or band share in ONE kernel launch, bit for bit what n calls of
rtgo_whitted_launch_frame leave -- accumulation, 8-bit image and both ray counts -- for every scene kind and residency of the path.

The reference is always the single launches: subframes 0 .. 10 rendered once per scene by rtgo_whitted_launch, with the outputs and ray
counts kept after every subframe.  The oracle's n-subframe renders hold the call to something other than the product.

The lanes per pixel the host picks (whitted_lanes_log2) for the counts used here: 2 -> 2, 3 -> 4, 4 -> 4, 5 -> 2, 7 -> 8, 8 -> 8,
11 -> 4: every tile shape, chunks that end in idle lanes (3, 5, 7, 11) and more than one chunk (5, 11)."""
import ctypes as C

import numpy as np
import pytest

import whitted_instances as WI
import whitted_big_meshes as BM
from parity import assert_parity
from test_whitted_bands import EYE, FIELDS, RTGO_E_INVALID, RTGO_E_STATE, RTGO_OK, _crop, _mesh_ctx, _same, _scene_ctx

N_REF = 11
CASES = [(0, 2), (0, 3), (0, 4), (0, 5), (0, 8), (0, 11), (3, 1), (3, 2), (3, 5), (1, 7)]   # (first subframe, n)
SCENE_CASES = [(0, 4), (2, 5)]


@pytest.fixture(scope="module")
def capi():
    import torch
    from raytracingo_amd import _build, capi as m
    _build.build_all()
    m.load()
    if torch.cuda.is_available():
        torch.cuda.init()   # torch's HIP runtime up before this module's first context (the GPU tests hand it buffers)
    return m


def _singles(ctx, W, H, upto=N_REF):
    """the reference: subframes 0 .. upto - 1 by rtgo_whitted_launch; snaps[k] = (accumulation, image, ray counts) after k subframes"""
    ctx.resize(W * H)
    ctx.reset_stats()
    snaps = {}
    for sf in range(upto):
        ctx.whitted_launch(W, H, sf)
        ctx.sync()
        st = ctx.stats()
        snaps[sf + 1] = (ctx.read_accum(H, W), ctx.read_image(H, W), (st["rays_total"], st["rays_occlusion"]))
    assert snaps[upto][2][1] > 0, "no occlusion rays: the scene is not lit"
    return snaps


def _batched(ctx, capi, W, H, first, n, window=None, bands=(4, 1, 0), reserve_cus=0):
    """subframes 0 .. first - 1 by single launches, then first .. first + n - 1 by ONE call of rtgo_whitted_launch_frames, into the
    context's own output sized to the share's compact rows.  Returns (accumulation, image, ray counts of all first + n subframes)"""
    x0, y0, w, h = window if window is not None else (0, 0, W, H)
    rows = capi.local_rows(h, bands[0] or 4, bands[1] or 1, bands[2])
    ctx.resize(max(rows * w, 1))
    ctx.reset_stats()
    for sf in range(first):
        ctx.whitted_launch_frame(capi.make_whitted_frame(W, H, sf, window=window, bands=bands, reserve_cus=reserve_cus))
    ctx.whitted_launch_frames(capi.make_whitted_frame(W, H, first, window=window, bands=bands, reserve_cus=reserve_cus), n)
    ctx.sync()
    st = ctx.stats()
    assert st["launches"] == first + 1, (first, n, st["launches"])
    return ctx.read_accum(rows, w), ctx.read_image(rows, w), (st["rays_total"], st["rays_occlusion"])


def _cases_are_the_singles(ctx, capi, W, H, cases, what):
    ref = _singles(ctx, W, H, max(f + n for f, n in cases))
    for first, n in cases:
        tag = "%s, subframes %d .. %d in one launch" % (what, first, first + n - 1)
        got = _batched(ctx, capi, W, H, first, n)
        _same(got, ref[first + n], tag)
        assert got[2] == ref[first + n][2], (tag, "ray counts", got[2], ref[first + n][2])
    return ref


# ---- bitwise equality on the single mesh ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_single_mesh_subframes_in_one_launch_are_the_single_launches(capi, oracle, monkeypatch, mode):
    """whitted_scene.build() at 157 x 99 (tiles cut on both edges) under each render_kernel residency"""
    import whitted_scene
    monkeypatch.setenv("RTGO_WHITTED_MODE", mode)
    W, H = 157, 99
    ctx = _mesh_ctx(capi, whitted_scene.build(), whitted_scene.camera(oracle, W, H))
    ref = _cases_are_the_singles(ctx, capi, W, H, CASES, "mode " + mode)
    # (0, 3) then (3, 5): the second call continues from what the first left
    ctx.resize(W * H)
    ctx.reset_stats()
    ctx.whitted_launch_frames(capi.make_whitted_frame(W, H, 0), 3)
    ctx.sync()
    assert ctx.stats()["launches"] == 1
    ctx.whitted_launch_frames(capi.make_whitted_frame(W, H, 3), 5)
    ctx.sync()
    st = ctx.stats()
    assert st["launches"] == 2
    _same((ctx.read_accum(H, W), ctx.read_image(H, W)), ref[8], "mode %s, 3 + 5 subframes" % mode)
    assert (st["rays_total"], st["rays_occlusion"]) == ref[8][2]
    assert st["last_launch_ms"] > 0.0
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", ["1", "2", "4", "8"])
def test_forced_lanes_per_pixel_change_no_bit(capi, oracle, monkeypatch, lanes):
    """RTGO_WHITTED_SUBFRAME_LANES (experiment knob): every lane count on counts below, at and above it -- 1 is one lane looping over its
    pixel's subframes, 8 lanes on 3 subframes leave five of eight idle"""
    import whitted_scene
    monkeypatch.setenv("RTGO_WHITTED_SUBFRAME_LANES", lanes)
    W, H = 157, 99
    ctx = _mesh_ctx(capi, whitted_scene.build(), whitted_scene.camera(oracle, W, H))
    _cases_are_the_singles(ctx, capi, W, H, [(0, 3), (1, 4), (0, 9)], "lanes " + lanes)
    ctx.close()


# ---- the same equality under more scenes -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_waterbottle_subframes_in_one_launch(capi, oracle):
    """the textured WaterBottle (base colour, metallic-roughness and normal maps)"""
    import whitted_scene
    W, H = 160, 120
    ctx = _mesh_ctx(capi, whitted_scene.waterbottle(), whitted_scene.camera(oracle, W, H, eye=(0.12, 0.08, 0.42), lookat=(0.0, 0.0, 0.0), fov=40.0))
    _cases_are_the_singles(ctx, capi, W, H, SCENE_CASES, "WaterBottle")
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["2", "0"])
def test_instanced_tori_subframes_in_one_launch(capi, oracle, monkeypatch, mode):
    """21 instances: the top level in LDS (RTGO_WHITTED_MODE=2) and in L2 (0)"""
    import whitted_scene
    monkeypatch.setenv("RTGO_WHITTED_MODE", mode)
    W, H = 120, 80
    meshes, inst = WI.tori_scene()
    ctx = _scene_ctx(capi, meshes, inst, WI.materials(), WI.lights(), whitted_scene.camera(oracle, W, H, eye=(0.5, 4.0, 6.0), lookat=(0.0, 0.4, -0.5)))
    _cases_are_the_singles(ctx, capi, W, H, SCENE_CASES, "tori, mode " + mode)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["2", "0"])
def test_clustered_mesh_subframes_in_one_launch(capi, oracle, monkeypatch, mode):
    """a ground plus a 40 000-triangle displaced torus (a clustered mesh), top level in LDS and in L2"""
    import whitted_scene
    monkeypatch.setenv("RTGO_WHITTED_MODE", mode)
    W, H = 112, 88
    meshes = [WI.ground(4.0, -0.4, normals=True), BM.displaced_torus(200, 100, texcoords=False)]
    inst = [(EYE, 0, 0), (EYE, 1, 1)]
    ctx = _scene_ctx(capi, meshes, inst, WI.materials(), WI.lights(), whitted_scene.camera(oracle, W, H, eye=(0.3, 2.0, 2.8), lookat=(0.0, -0.1, 0.0)))
    _cases_are_the_singles(ctx, capi, W, H, SCENE_CASES, "clustered torus, mode " + mode)
    ctx.close()


# ---- shares ----------------------------------------------------------------------------------------------------------------------
def _split_frames(ctx, capi, W, H, band_h, G, first, n):
    """a G-way split of the whole image, every share in its own slice of one device buffer (the layout of a gather to one root):
    subframes 0 .. first - 1 by single launches, the rest by one rtgo_whitted_launch_frames per share.  Returns the frame reassembled
    in numpy with the ray counts summed over the shares"""
    import torch
    from raytracingo_amd import bands as B
    rows_pad = B.max_local_rows(H, band_h, G)
    g_acc = torch.zeros((G * rows_pad, W, 4), dtype=torch.float32, device="cuda")
    g_img = torch.zeros((G * rows_pad, W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.reset_stats()
    for g in range(G):
        ctx.bind_output(g_acc[g * rows_pad].data_ptr(), g_img[g * rows_pad].data_ptr(), rows_pad * W)
        for sf in range(first):
            ctx.whitted_launch_frame(capi.make_whitted_frame(W, H, sf, bands=(band_h, G, g)))
        ctx.whitted_launch_frames(capi.make_whitted_frame(W, H, first, bands=(band_h, G, g)), n)
    ctx.sync()
    st = ctx.stats()
    assert st["launches"] == G * (first + 1)
    acc_np, img_np = g_acc.cpu().numpy(), g_img.cpu().numpy()
    n_acc, n_img = np.empty((H, W, 4), np.float32), np.empty((H, W, 4), np.uint8)
    for g in range(G):
        r = B.band_rows(H, band_h, G, g)
        n_acc[r] = acc_np[g * rows_pad:g * rows_pad + len(r)]
        n_img[r] = img_np[g * rows_pad:g * rows_pad + len(r)]
    return n_acc, n_img, (st["rays_total"], st["rays_occlusion"])


@pytest.mark.gpu
def test_shares_in_one_launch_are_crops_and_bands_of_the_full_frame(capi, oracle):
    """windows that cut every tile shape (one pixel, one column, one row, odd offsets, the bottom-right corner), 3-way and 8-way band
    splits, and reserved CUs, at 2, 4 and 8 lanes per pixel ((2, 5), (0, 4), (0, 8))"""
    import whitted_scene
    W, H = 157, 99
    ctx = _mesh_ctx(capi, whitted_scene.build(), whitted_scene.camera(oracle, W, H))
    ref = _singles(ctx, W, H, 8)
    for first, n in [(0, 4), (2, 5), (0, 8)]:
        full = ref[first + n]
        for window in [(77, 41, 1, 1), (9, 0, 1, 99), (0, 13, 157, 1), (3, 5, 61, 37), (112, 76, 45, 23)]:
            got = _batched(ctx, capi, W, H, first, n, window=window)
            _same(got, _crop(full, window), "window %r, subframes %d .. %d" % (window, first, first + n - 1))
        for band_h, G in [(3, 3), (4, 8)]:
            got = _split_frames(ctx, capi, W, H, band_h, G, first, n)
            _same(got, full, "%d-way split, band_h %d, subframes %d .. %d" % (G, band_h, first, first + n - 1))
            assert got[2] == full[2], ("ray counts of the split", got[2], full[2])
        for reserve in (8, 200):
            got = _batched(ctx, capi, W, H, first, n, reserve_cus=reserve)
            _same(got, full, "reserve_cus %d" % reserve)
            assert got[2] == full[2]
    ctx.close()


# ---- against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_four_subframes_in_one_launch_against_the_oracle(capi, oracle):
    """subframes 0 .. 3 in one launch against the oracle's own 4-subframe renders, under tests/parity.py's thresholds"""
    import whitted_scene
    W, H = 160, 100
    mesh = whitted_scene.build()
    cam = whitted_scene.camera(oracle, W, H)
    ctx = _mesh_ctx(capi, mesh, cam)
    got = _batched(ctx, capi, W, H, 0, 4)
    racc, rimg, _ = oracle.whitted_render(mesh, cam, W, H, 4)
    print("single mesh, 4 subframes in one launch against the oracle:", assert_parity(got[0], racc, got[1], rimg, what="single mesh, 4 subframes"))
    ctx.close()

    W, H = 96, 64
    meshes, inst = WI.tori_scene()
    mats, extra = WI.materials(), WI.lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.5, 4.0, 6.0), lookat=(0.0, 0.4, -0.5))
    ctx = _scene_ctx(capi, meshes, inst, mats, extra, cam)
    got = _batched(ctx, capi, W, H, 0, 4)
    racc, rimg, _ = oracle.whitted_render_instanced(meshes, inst, mats, extra, cam, W, H, 4)
    print("tori, 4 subframes in one launch against the instanced oracle:", assert_parity(got[0], racc, got[1], rimg, what="tori, 4 subframes"))
    ctx.close()


# ---- refusals and edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_and_edges(capi, oracle):
    """n = 0 and an index range past 2^32 are RTGO_E_INVALID; every frame rtgo_whitted_launch_frame refuses is refused with the same code;
    state errors are RTGO_E_STATE; a rowless rank enqueues nothing; refused calls between two valid ones change no pixel"""
    import torch
    import whitted_scene
    L = capi.load()
    W, H = 128, 72
    mesh = whitted_scene.build()
    cam = whitted_scene.camera(oracle, W, H)

    bare = capi.Context(0)
    for setup in (lambda c: None, lambda c: c.whitted_set_mesh(mesh["positions"], mesh["normals"], mesh["indices"], mesh["tri_material"], mesh["materials"]),
                  lambda c: c.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])):
        setup(bare)   # no mesh, then no camera, then no output
        assert L.rtgo_whitted_launch_frames(bare._h, C.byref(capi.make_whitted_frame(W, H, 0)), 4) == RTGO_E_STATE
    bare.close()

    ctx = _mesh_ctx(capi, mesh, cam)
    ref = _singles(ctx, W, H, 6)

    # a rank that owns no row: h = 4, G = 8, rank 7
    sentinel_a = torch.full((1, W, 4), 7.0, dtype=torch.float32, device="cuda")
    sentinel_i = torch.full((1, W, 4), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.bind_output(sentinel_a.data_ptr(), sentinel_i.data_ptr(), W)
    ctx.reset_stats()
    f = capi.make_whitted_frame(W, H, 0, window=(0, 10, W, 4), bands=(4, 8, 7))
    assert L.rtgo_whitted_launch_frames(ctx._h, C.byref(f), 4) == RTGO_OK
    ctx.sync()
    assert ctx.stats()["launches"] == 0 and ctx.stats()["rays_total"] == 0
    assert (sentinel_a.cpu().numpy() == 7.0).all() and (sentinel_i.cpu().numpy() == 7).all()

    # refusals between two valid calls of a band share (rank 0 of 2 of the window (3, 4, 100, 64)): subframes 0 .. 1, then 2 .. 5
    window, bands = (3, 4, 100, 64), (4, 2, 0)
    rows = capi.local_rows(64, 4, 2, 0)
    ctx.resize(rows * 100)
    refused = [capi.make_whitted_frame(W, H, 2, window=(W - 99, 4, 100, 64), bands=bands),    # window past the right edge
               capi.make_whitted_frame(W, H, 2, window=(3, H - 63, 100, 64), bands=bands),    # ... past the bottom
               capi.make_whitted_frame(W, H, 2, window=(0, 0, W + 1, 0), bands=bands),        # wider than the image
               capi.make_whitted_frame(W, H, 2, window=window, bands=(4, 2, 2)),              # rank >= n_ranks
               capi.make_whitted_frame(W, H, 2, window=window, bands=(4, 0, 1)),              # rank 1 of one rank
               capi.make_whitted_frame(W, H, 2, window=window, bands=(4, 1, 0)),              # 64 rows: beyond the output
               capi.make_whitted_frame(W, H, 2, window=(3, 4, 101, 64), bands=bands),         # 101 columns: beyond the output
               capi.make_whitted_frame(W, H, 2, window=window, bands=bands, reserve_cus=100000),   # no CU left
               capi.make_whitted_frame(0, H, 2)]                                               # empty image
    ctx.reset_stats()
    ctx.whitted_launch_frames(capi.make_whitted_frame(W, H, 0, window=window, bands=bands), 2)
    for fr in refused:
        assert L.rtgo_whitted_launch_frame(ctx._h, C.byref(fr)) == RTGO_E_INVALID, [getattr(fr, k) for k in FIELDS]
        assert L.rtgo_whitted_launch_frames(ctx._h, C.byref(fr), 4) == RTGO_E_INVALID, [getattr(fr, k) for k in FIELDS]
    good = capi.make_whitted_frame(W, H, 2, window=window, bands=bands)
    assert L.rtgo_whitted_launch_frames(ctx._h, C.byref(good), 0) == RTGO_E_INVALID
    assert L.rtgo_whitted_launch_frames(ctx._h, C.byref(capi.make_whitted_frame(W, H, 0xFFFFFFFE, window=window, bands=bands)), 3) == RTGO_E_INVALID
    assert L.rtgo_whitted_launch_frames(ctx._h, None, 4) == RTGO_E_INVALID
    ctx.whitted_launch_frames(good, 4)
    ctx.sync()
    assert ctx.stats()["launches"] == 2
    from raytracingo_amd import bands as B
    r = 4 + B.band_rows(64, 4, 2, 0)
    _same((ctx.read_accum(rows, 100), ctx.read_image(rows, 100)), (ref[6][0][r, 3:103], ref[6][1][r, 3:103]), "after refusals")
    ctx.close()
