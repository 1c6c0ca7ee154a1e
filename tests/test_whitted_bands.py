"""Windows and row bands of the whitted path (rtgo_whitted_launch_frame): a share of the frame is rendered into a compact buffer, and
the shares put back together -- in numpy or by rtgo_assemble_bands -- are bitwise the full frame of rtgo_whitted_launch, accumulation,
8-bit image and ray counts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import whitted_instances as WI
import whitted_big_meshes as BM
from parity import assert_parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(3, 4, dtype=np.float32)
FIELDS = ("image_width", "image_height", "subframe_index", "x0", "y0", "w", "h", "band_h", "n_ranks", "rank", "reserve_cus")


@pytest.fixture(scope="module")
def capi():
    import torch
    from raytracingo_amd import _build, capi as m
    _build.build_all()
    m.load()
    if torch.cuda.is_available():
        torch.cuda.init()   # torch's HIP runtime up before this module's first context (the GPU tests hand it buffers)
    return m


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_launch_frame_is_exported(capi):
    assert "rtgo_whitted_launch_frame" in capi.SYMBOLS
    assert capi.load().rtgo_whitted_launch_frame is not None


def test_whitted_frame_layout_is_the_headers(capi, tmp_path):
    """sizeof and offsetof of rtgo_whitted_frame as a C compiler lays out include/rtgo.h, against the ctypes binding"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rtgo.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(rtgo_whitted_frame));\n' +
                   "".join('    printf(" %%zu", offsetof(rtgo_whitted_frame, %s));\n' % f for f in FIELDS) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-x", "c", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(capi.WhittedFrame) == 11 * 4
    assert got[1:] == [getattr(capi.WhittedFrame, f).offset for f in FIELDS] == [4 * i for i in range(11)]


def test_make_whitted_frame_fills_the_fields(capi):
    f = capi.make_whitted_frame(1920, 1080, 7)
    assert [getattr(f, k) for k in FIELDS] == [1920, 1080, 7, 0, 0, 1920, 1080, 4, 1, 0, 0]
    f = capi.make_whitted_frame(640, 480, 2, window=(3, 5, 100, 50), bands=(8, 3, 2), reserve_cus=16)
    assert [getattr(f, k) for k in FIELDS] == [640, 480, 2, 3, 5, 100, 50, 8, 3, 2, 16]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
RTGO_OK, RTGO_E_INVALID, RTGO_E_STATE = 0, 1, 3
N_SUB = 3


def _mesh_ctx(capi, mesh, cam):
    ctx = capi.Context(0)
    ctx.whitted_set_mesh(mesh["positions"], mesh.get("normals"), mesh["indices"], mesh.get("tri_material"), mesh["materials"])
    if mesh.get("texcoords") is not None:
        ctx.whitted_set_texcoords(mesh["texcoords"])
    for mi, (bc, mr, nm) in (mesh.get("textures") or {}).items():
        ctx.whitted_set_material_textures(mi, bc, mr, nm)
    return _lit(ctx, mesh, cam)


def _scene_ctx(capi, meshes, instances, materials, extra, cam):
    ctx = capi.Context(0)
    ctx.whitted_set_scene(meshes, instances, materials)
    return _lit(ctx, extra, cam)


def _lit(ctx, extra, cam):
    ctx.whitted_set_lights(extra["lights"])
    ctx.whitted_set_miss_color(extra["miss"])
    ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])
    return ctx


def _full(ctx, W, H, n=N_SUB):
    """rtgo_whitted_launch over the whole image: (accumulation, image, (rays_total, rays_occlusion))"""
    ctx.resize(W * H)
    ctx.reset_stats()
    for sf in range(n):
        ctx.whitted_launch(W, H, sf)
    ctx.sync()
    st = ctx.stats()
    return ctx.read_accum(H, W), ctx.read_image(H, W), (st["rays_total"], st["rays_occlusion"])


def _share(ctx, capi, W, H, window=None, bands=(4, 1, 0), reserve_cus=0, n=N_SUB):
    """one share into the context's own output, sized to its compact rows"""
    x0, y0, w, h = window if window is not None else (0, 0, W, H)
    rows = capi.local_rows(h, bands[0] or 4, bands[1] or 1, bands[2])
    ctx.resize(max(rows * w, 1))
    ctx.reset_stats()
    for sf in range(n):
        ctx.whitted_launch_frame(capi.make_whitted_frame(W, H, sf, window=window, bands=bands, reserve_cus=reserve_cus))
    ctx.sync()
    st = ctx.stats()
    return ctx.read_accum(rows, w), ctx.read_image(rows, w), (st["rays_total"], st["rays_occlusion"])


def _same(a, b, what):
    assert a[0].shape == b[0].shape, (what, a[0].shape, b[0].shape)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), what + ": accumulation differs"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), what + ": image differs"


def _split(ctx, capi, W, H, window, band_h, G, n=N_SUB):
    """a G-way split of the window, every share in its own slice of one device buffer (the layout of a gather to one root), the
    subframes interleaved over the shares.  Returns the window reassembled in numpy, the same by rtgo_assemble_bands, and the ray counts
    summed over the shares"""
    import torch
    from raytracingo_amd import bands as B
    x0, y0, w, h = window
    rows_pad = B.max_local_rows(h, band_h, G)
    g_acc = torch.zeros((G * rows_pad, w, 4), dtype=torch.float32, device="cuda")
    g_img = torch.zeros((G * rows_pad, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.reset_stats()
    for sf in range(n):
        for g in range(G):
            ctx.bind_output(g_acc[g * rows_pad].data_ptr(), g_img[g * rows_pad].data_ptr(), rows_pad * w)
            ctx.whitted_launch_frame(capi.make_whitted_frame(W, H, sf, window=window, bands=(band_h, G, g)))
    ctx.sync()
    st = ctx.stats()
    acc_np, img_np = g_acc.cpu().numpy(), g_img.cpu().numpy()
    n_acc, n_img = np.empty((h, w, 4), np.float32), np.empty((h, w, 4), np.uint8)
    for g in range(G):
        r = B.band_rows(h, band_h, G, g)
        n_acc[r] = acc_np[g * rows_pad:g * rows_pad + len(r)]
        n_img[r] = img_np[g * rows_pad:g * rows_pad + len(r)]
    d_acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    d_img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L = capi.load()
    assert L.rtgo_assemble_bands(ctx._h, None, g_acc.data_ptr(), d_acc.data_ptr(), w, h, band_h, G, rows_pad, 16) == RTGO_OK
    assert L.rtgo_assemble_bands(ctx._h, None, g_img.data_ptr(), d_img.data_ptr(), w, h, band_h, G, rows_pad, 4) == RTGO_OK
    ctx.sync()
    rays = (st["rays_total"], st["rays_occlusion"])
    return (n_acc, n_img, rays), (d_acc.cpu().numpy(), d_img.cpu().numpy(), rays)


def _crop(full, window):
    x0, y0, w, h = window
    return full[0][y0:y0 + h, x0:x0 + w], full[1][y0:y0 + h, x0:x0 + w], full[2]


def _splits_are_the_frame(ctx, capi, W, H, what):
    """G in {2, 3, 8} x band_h in {1, 3, 4, 8} over the whole image, and a window under bands: numpy and device reassembly both bitwise
    the full frame; ray counts summed over the shares equal the full frame's exactly"""
    ref = _full(ctx, W, H)
    assert ref[2][1] > 0, what + ": no occlusion rays: the scene is not lit"
    cases = [((0, 0, W, H), b, G) for G in (2, 3, 8) for b in (1, 3, 4, 8)] + [((5, 7, W - 27, H - 30), 3, 3), ((1, 2, W - 3, 21), 4, 8)]
    for window, band_h, G in cases:
        tag = "%s window %r band_h %d G %d" % (what, window, band_h, G)
        host, dev = _split(ctx, capi, W, H, window, band_h, G)
        crop = _crop(ref, window)
        _same(host, crop, tag + " (numpy)")
        _same(dev, crop, tag + " (rtgo_assemble_bands)")
        if window == (0, 0, W, H):
            assert host[2] == ref[2], (tag, "ray counts", host[2], ref[2])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_windows_are_crops_of_the_full_frame(capi, oracle, monkeypatch, mode):
    """the single-mesh procedural scene under each render_kernel residency: windows that cut 8 x 8 tiles (odd offsets, one pixel, a
    full-width strip, the bottom-right corner) are bitwise the same crop of the full frame"""
    import whitted_scene
    monkeypatch.setenv("RTGO_WHITTED_MODE", mode)
    W, H = 157, 99
    mesh = whitted_scene.build()
    ctx = _mesh_ctx(capi, mesh, whitted_scene.camera(oracle, W, H))
    ref = _full(ctx, W, H)
    for window in [(3, 5, 61, 37), (77, 41, 1, 1), (0, 13, W, 9), (W - 45, H - 23, 45, 23), (0, 0, W, H), (9, 0, 17, H)]:
        got = _share(ctx, capi, W, H, window=window)
        _same(got, _crop(ref, window), "mode %s window %r" % (mode, window))
    assert ref[2][1] > 0
    ctx.close()


@pytest.mark.gpu
def test_band_splits_of_the_waterbottle(capi, oracle):
    """the textured WaterBottle (base colour, metallic-roughness and normal maps)"""
    import whitted_scene
    W, H = 160, 120
    wb = whitted_scene.waterbottle()
    ctx = _mesh_ctx(capi, wb, whitted_scene.camera(oracle, W, H, eye=(0.12, 0.08, 0.42), lookat=(0.0, 0.0, 0.0), fov=40.0))
    _splits_are_the_frame(ctx, capi, W, H, "WaterBottle")
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["2", "0"])
def test_band_splits_of_instanced_tori(capi, oracle, monkeypatch, mode):
    """21 instances: the top level in LDS (RTGO_WHITTED_MODE=2, render_inst_kernel<true>) and in L2 (0, render_inst_kernel<false>)"""
    import whitted_scene
    monkeypatch.setenv("RTGO_WHITTED_MODE", mode)
    W, H = 120, 80
    meshes, inst = WI.tori_scene()
    ctx = _scene_ctx(capi, meshes, inst, WI.materials(), WI.lights(), whitted_scene.camera(oracle, W, H, eye=(0.5, 4.0, 6.0), lookat=(0.0, 0.4, -0.5)))
    _splits_are_the_frame(ctx, capi, W, H, "tori, mode " + mode)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["2", "0"])
def test_band_splits_with_a_clustered_mesh(capi, oracle, monkeypatch, mode):
    """a 40 000-triangle displaced torus (a clustered mesh: render_inst_kernel<*, true>) over a ground, top level in LDS and in L2"""
    import whitted_scene
    monkeypatch.setenv("RTGO_WHITTED_MODE", mode)
    W, H = 112, 88
    meshes = [WI.ground(4.0, -0.4, normals=True), BM.displaced_torus(200, 100, texcoords=False)]
    inst = [(EYE, 0, 0), (EYE, 1, 1)]
    ctx = _scene_ctx(capi, meshes, inst, WI.materials(), WI.lights(), whitted_scene.camera(oracle, W, H, eye=(0.3, 2.0, 2.8), lookat=(0.0, -0.1, 0.0)))
    _splits_are_the_frame(ctx, capi, W, H, "clustered torus, mode " + mode)
    ctx.close()


@pytest.mark.gpu
def test_a_band_share_of_the_tori_against_the_instanced_oracle(capi, oracle):
    """rank 1 of a 3-way 4-row interleave of the instanced tori against oracle.whitted_render_instanced on the same rows"""
    import whitted_scene
    from raytracingo_amd import bands as B
    W, H = 96, 64
    meshes, inst = WI.tori_scene()
    mats, extra = WI.materials(), WI.lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.5, 4.0, 6.0), lookat=(0.0, 0.4, -0.5))
    ctx = _scene_ctx(capi, meshes, inst, mats, extra, cam)
    got = _share(ctx, capi, W, H, bands=(4, 3, 1), n=2)
    racc, rimg, _ = oracle.whitted_render_instanced(meshes, inst, mats, extra, cam, W, H, 2)
    rows = B.band_rows(H, 4, 3, 1)
    m = assert_parity(got[0], racc[rows], got[1], rimg[rows], what="tori, band share 1 of 3")
    print("tori band share 1/3 against the instanced oracle:", m)
    ctx.close()


@pytest.mark.gpu
def test_edge_cases_refusals_and_reserved_cus(capi, oracle):
    """a rank without rows enqueues nothing; every refusal is RTGO_E_INVALID and leaves the next valid launch's frame as it was;
    reserve_cus changes no pixel; state errors are rtgo_whitted_launch's"""
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
        assert L.rtgo_whitted_launch(bare._h, W, H, 0) == RTGO_E_STATE
        assert L.rtgo_whitted_launch_frame(bare._h, C.byref(capi.make_whitted_frame(W, H, 0))) == RTGO_E_STATE
    bare.close()

    ctx = _mesh_ctx(capi, mesh, cam)
    ref = _full(ctx, W, H)

    # a rank that owns no row: h = 4, G = 8, rank 7
    sentinel_a = torch.full((1, W, 4), 7.0, dtype=torch.float32, device="cuda")
    sentinel_i = torch.full((1, W, 4), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.bind_output(sentinel_a.data_ptr(), sentinel_i.data_ptr(), W)
    ctx.reset_stats()
    f = capi.make_whitted_frame(W, H, 0, window=(0, 10, W, 4), bands=(4, 8, 7))
    assert L.rtgo_whitted_launch_frame(ctx._h, C.byref(f)) == RTGO_OK
    ctx.sync()
    assert ctx.stats()["launches"] == 0 and ctx.stats()["rays_total"] == 0
    assert (sentinel_a.cpu().numpy() == 7.0).all() and (sentinel_i.cpu().numpy() == 7).all()

    # refusals between the subframes of a band share (rank 0 of 2, rows 4..67 of the window (3, 4, 100, 64))
    window, bands = (3, 4, 100, 64), (4, 2, 0)
    rows = capi.local_rows(64, 4, 2, 0)
    ctx.resize(rows * 100)
    refused = [capi.make_whitted_frame(W, H, 1, window=(W - 99, 4, 100, 64), bands=bands),    # window past the right edge
               capi.make_whitted_frame(W, H, 1, window=(3, H - 63, 100, 64), bands=bands),    # ... past the bottom
               capi.make_whitted_frame(W, H, 1, window=(0, 0, W + 1, 0), bands=bands),        # wider than the image
               capi.make_whitted_frame(W, H, 1, window=window, bands=(4, 2, 2)),              # rank >= n_ranks
               capi.make_whitted_frame(W, H, 1, window=window, bands=(4, 0, 1)),              # rank 1 of one rank
               capi.make_whitted_frame(W, H, 1, window=window, bands=(4, 1, 0)),              # 64 rows: beyond the output
               capi.make_whitted_frame(W, H, 1, window=(3, 4, 101, 64), bands=bands),         # 101 columns: beyond the output
               capi.make_whitted_frame(W, H, 1, window=window, bands=bands, reserve_cus=100000),   # no CU left
               capi.make_whitted_frame(0, H, 1)]                                               # empty image
    ctx.reset_stats()
    ctx.whitted_launch_frame(capi.make_whitted_frame(W, H, 0, window=window, bands=bands))
    for fr in refused:
        assert L.rtgo_whitted_launch_frame(ctx._h, C.byref(fr)) == RTGO_E_INVALID, [getattr(fr, k) for k in FIELDS]
    for sf in range(1, N_SUB):
        ctx.whitted_launch_frame(capi.make_whitted_frame(W, H, sf, window=window, bands=bands))
    ctx.sync()
    assert ctx.stats()["launches"] == N_SUB
    from raytracingo_amd import bands as B
    r = 4 + B.band_rows(64, 4, 2, 0)
    _same((ctx.read_accum(rows, 100), ctx.read_image(rows, 100)), (ref[0][r, 3:103], ref[1][r, 3:103]), "after refusals")

    # reserved CUs: the same frame
    for reserve in (8, 64, 200):
        got = _share(ctx, capi, W, H, reserve_cus=reserve)
        _same(got, ref, "reserve_cus %d" % reserve)
        assert got[2] == ref[2]
    ctx.close()
