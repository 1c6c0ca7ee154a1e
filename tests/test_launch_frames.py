"""rtgo_launch_frames on the MI355X: K progressive frames of a window or band share in one call -- one kernel launch where the batched
kernels (render_frames_kernel) apply, K launches otherwise -- must leave the accumulation buffer (compared as uint32) and the 8-bit image
that K calls of rtgo_launch with the frame counts in turn leave, bit for bit, and the ray counters their sums.

Every case plays a schedule of calls on one context and the same frames through rtgo_launch alone on another.  MI355X has 256 CUs:
units_per_wave4 = hot units / 4096 picks the variant, >= 3 the 5-waves kernels, below that the 4-waves ones.  The docstrings name the
instantiation each case runs (RTGO_DEBUG's line says which: frames per launch, waves/SIMD variant)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTGO_E_INVALID = 1
BATCHED_BIT = 128


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import capi as m
    m.load()
    return m


_tables = {}


def tables(name, W, H):
    from raytracingo_amd import scene
    if (name, W, H) not in _tables:
        _tables[(name, W, H)] = scene.tables(name, W, H)
    return _tables[(name, W, H)]


def context(capi, t, pixels, large=False, eye=None):
    ctx = capi.Context(0)
    (ctx.set_large_scene if large else ctx.set_scene)(t["type"], t["M"], t["mat"], t["aabb"])
    cam = t["cam"]
    ctx.set_camera(cam[0:3] if eye is None else np.asarray(eye, np.float32), cam[3:6], cam[6:9], cam[9:12])
    ctx.set_background(t["bg"])
    ctx.set_lights(t["lights"])
    ctx.resize(max(pixels, 1))
    return ctx


def play(capi, t, W, H, N, calls, path=True, ambient=False, window=None, bands=(4, 1, 0), stats=0, first=0, large=False, eye=None):
    """calls: the frames of each call in turn, 0 = one rtgo_launch, k >= 1 = rtgo_launch_frames of k frames; frame counts run on from
    `first`.  Returns the accumulation buffer, the image, the counters, and last_variant after every call."""
    x0, y0, w, h = window if window else (0, 0, W, H)
    rows = capi.local_rows(h, *bands)
    ctx = context(capi, t, rows * w, large, eye)
    f, variants = first, []
    for k in calls:
        fr = capi.make_frame(W, H, N, f, path, ambient, window, bands, stats=stats)
        if k == 0:
            ctx.launch(fr)
        else:
            ctx.launch_frames(fr, k)
        f += max(k, 1)
        variants.append(ctx.stats()["last_variant"])
    ctx.sync()
    out = (ctx.read_accum(rows, w), ctx.read_image(rows, w), ctx.stats(), variants)
    ctx.close()
    return out


def assert_same(got, ref, what):
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), (what, "accumulation buffers differ")
    assert np.array_equal(got[1], ref[1]), (what, "images differ")
    for k in ("rays_total", "rays_occlusion", "rays_culled"):
        assert got[2][k] == ref[2][k], (what, k, got[2][k], ref[2][k])


_references = {}


def reference(capi, name, W, H, N, frames, **kw):
    """`frames` calls of rtgo_launch on one context: rendered once per configuration, shared by the tests that compare against it"""
    key = (name, W, H, N, frames, tuple(sorted(kw.items())))
    if key not in _references:
        _references[key] = play(capi, tables(name, W, H), W, H, N, [0] * frames, **kw)
    return _references[key]


def check_batched(capi, name, W, H, N, K, what=None, **kw):
    """K frames in one batched launch against K launches"""
    t = tables(name, W, H)
    got = play(capi, t, W, H, N, [K], **kw)
    ref = reference(capi, name, W, H, N, K, **kw)
    assert_same(got, ref, what or (name, W, H, N, K, kw))
    assert got[3][-1] & BATCHED_BIT, got[3]
    assert got[2]["launches"] == 1 and ref[2]["launches"] == K
    assert got[2]["rays_total"] > 0
    return got, ref


# ---- 1. the 4-waves kernels, all three flavours -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,path,ambient", [("cornell", True, False), ("plateau", True, False), ("cornell", False, False), ("cornell", False, True)])
def test_four_waves_kernels(capi, name, path, ambient):
    """128 x 72, N = 2, frames 0-3: under one unit per wave, so render_frames_kernel<true, 4, true> (cornell: flat primitives, shading
    frames from LDS), <true, 4, false> (plateau: quadrics; most of its rectangle's strips are masked, the rest of the window is cold
    segments) and <false, 4, false> (distributed, without and with the ambient coefficient)"""
    got, _ = check_batched(capi, name, 128, 72, 2, 4, path=path, ambient=ambient)
    if name == "plateau":
        assert got[2]["rays_culled"] > 0   # the background pixels went through the four steps of their average too
    if not path:
        assert got[2]["rays_occlusion"] > 0


# ---- 2. the 5-waves kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,path", [("cornell", True), ("plateau", True), ("cornell", False)])
def test_five_waves_kernels(capi, name, path):
    """480 x 270, N = 4 (one unit = 4 pixels), frames 0-2: 3..8 units per wave, so render_frames_kernel<true, 5, true>, <true, 5, false> and
    <false, 5, false> (level records and the shadow ray's state in LDS)"""
    check_batched(capi, name, 480, 270, 4, 3, path=path)


# ---- 3. odd lane layouts and edges ----------------------------------------------------------------------------------------------------
def test_nine_samples_seven_pixels_per_unit(capi):
    """N = 3: 9 samples, 7 pixels per unit, lane 63 idle; 250 pixels a row: the last unit of a row is partial"""
    check_batched(capi, "cornell", 250, 141, 3, 3)


def test_one_sample_per_pixel(capi):
    """N = 1: 64 pixels per unit, one strip is one unit; 70 x 40"""
    check_batched(capi, "cornell", 70, 40, 1, 4)


def test_window(capi):
    check_batched(capi, "cornell", 160, 90, 2, 3, window=(13, 7, 97, 61))
    check_batched(capi, "plateau", 160, 90, 2, 3, window=(13, 7, 97, 61))


@pytest.mark.parametrize("bands", [(4, 2, 1), (4, 8, 3)])
def test_band_shares_into_compact_outputs(capi, bands):
    check_batched(capi, "cornell", 160, 90, 2, 3, bands=bands)
    check_batched(capi, "cornell", 160, 90, 2, 3, bands=bands, path=False)


def test_rank_without_rows(capi):
    """an 8-row window in 4-row bands over 4 ranks: rank 3 owns no row -- RTGO_OK, nothing enqueued, the counters do not move"""
    t = tables("cornell", 160, 90)
    assert capi.local_rows(8, 4, 4, 3) == 0
    ctx = context(capi, t, 1)
    ctx.launch_frames(capi.make_frame(160, 90, 2, 0, window=(0, 40, 160, 8), bands=(4, 4, 3)), 4)
    ctx.sync()
    st = ctx.stats()
    assert st["launches"] == 0 and st["rays_total"] == 0 and st["rays_culled"] == 0 and st["last_variant"] == 0, st
    ctx.close()


# ---- 4. start frame and chaining -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", [[2], [5],                 # from frame 0: the accumulation buffer is not read
                                   [0, 0, 0, 2], [0, 0, 0, 5],   # from frame 3, over what frames 0-2 left
                                   [4, 4],                   # frames 0-3, then 4-7
                                   [3, 0, 0], [0, 0, 3], [2, 0, 3, 0]])
@pytest.mark.parametrize("name,path", [("cornell", True), ("plateau", True), ("cornell", False)])
def test_chaining(capi, name, path, calls):
    t = tables(name, 128, 72)
    frames = sum(max(k, 1) for k in calls)
    got = play(capi, t, 128, 72, 2, calls, path=path)
    ref = reference(capi, name, 128, 72, 2, frames, path=path)
    assert_same(got, ref, (name, path, calls))
    for k, v in zip(calls, got[3]):
        assert bool(v & BATCHED_BIT) == (k > 1), (calls, got[3])
    assert got[2]["launches"] == len(calls)


def test_start_frame_is_the_frames_own(capi):
    """frames 3-5 over a buffer that never saw frames 0-2: the first step reads it like rtgo_launch at frame 3 does"""
    t = tables("cornell", 128, 72)
    got = play(capi, t, 128, 72, 2, [3], first=3)
    ref = play(capi, t, 128, 72, 2, [0, 0, 0], first=3)
    assert_same(got, ref, "from frame 3 over zeros")


def test_one_frame_is_rtgo_launch(capi):
    t = tables("cornell", 128, 72)
    got = play(capi, t, 128, 72, 2, [1, 1])
    ref = play(capi, t, 128, 72, 2, [0, 0])
    assert_same(got, ref, "K = 1")
    assert got[3] == ref[3] and all(v & BATCHED_BIT == 0 for v in got[3])
    for k in ("launches", "launches_trial", "launches_canonical"):
        assert got[2][k] == ref[2][k], k


# ---- 5. against the oracle --------------------------------------------------------------------------------------------------------------
def test_against_the_oracle(capi, oracle):
    """cornell 64 x 36, N = 2, path: frames 0-3 in one batched launch against the CPU oracle's four-frame chain, within the project's
    tolerance (parity.assert_parity: 1e-4 * max(1, |ref|) on >= 99 % of the pixels)"""
    from parity import assert_parity
    W, H, N = 64, 36, 2
    sc = oracle.scene("cornell", W, H)
    t = oracle.scene_tables(sc)
    got = play(capi, t, W, H, N, [4])
    assert got[3][-1] & BATCHED_BIT and got[2]["launches"] == 1
    racc = None
    for f in range(4):
        racc, rimg, _ = oracle.render(sc, oracle.frame(W, H, N, f, path=True, mode=1), accum_prev=racc)
    assert_parity(got[0], racc, got[1], rimg, what="frames 0-3 in one launch")


# ---- 6. stats -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,path", [("plateau", True), ("cornell", False)])
def test_ray_counters_are_the_sums(capi, name, path):
    t = tables(name, 160, 90)
    got = play(capi, t, 160, 90, 2, [5], path=path)
    singles = [play(capi, t, 160, 90, 2, [0], path=path, first=f)[2] for f in range(5)]
    for k in ("rays_total", "rays_occlusion", "rays_culled"):
        assert got[2][k] == sum(s[k] for s in singles), (k, got[2][k], [s[k] for s in singles])
    assert got[2]["rays_total"] > 0 and (path or got[2]["rays_occlusion"] > 0) and (name != "plateau" or got[2]["rays_culled"] > 0)
    assert got[2]["last_launch_ms"] > 0.0


# ---- 7. seeds -----------------------------------------------------------------------------------------------------------------------------
def seeds_flags(ctx):
    L = ctx._lib
    L.rtgo_debug_seeds.restype = C.c_int
    L.rtgo_debug_seeds.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    v = C.c_uint32(0)
    assert L.rtgo_debug_seeds(ctx._h, C.byref(v)) == 0
    return v.value


def test_seed_pass_around_a_batched_launch(capi):
    """cornell 1080p N = 4 runs the 6-waves kernel with the seed pass: rtgo_launch frame 0 (writes frame 1's seeds), rtgo_launch_frames
    frames 1-3 (reads none, leaves none), rtgo_launch frame 4 (hashes inline -- frame 1's seeds are stale -- and writes frame 5's)"""
    W, H, N = 1920, 1080, 4
    t = tables("cornell", W, H)
    ctx = context(capi, t, W * H)
    ctx.launch(capi.make_frame(W, H, N, 0))
    assert seeds_flags(ctx) == 2
    ctx.launch_frames(capi.make_frame(W, H, N, 1), 3)
    assert seeds_flags(ctx) == 0
    assert ctx.stats()["last_variant"] & BATCHED_BIT
    ctx.launch(capi.make_frame(W, H, N, 4))
    assert seeds_flags(ctx) == 2
    ctx.sync()
    acc, img = ctx.read_accum(H, W), ctx.read_image(H, W)
    ctx.close()
    # every frame on a fresh context, over the accumulation buffer the one before left
    racc = None
    for f in range(5):
        c = context(capi, t, W * H)
        if racc is not None:
            c.write_accum(racc)
        c.launch(capi.make_frame(W, H, N, f))
        assert seeds_flags(c) & 1 == 0
        c.sync()
        racc, rimg = c.read_accum(H, W), c.read_image(H, W)
        c.close()
    assert np.array_equal(acc.view(np.uint32), racc.view(np.uint32)) and np.array_equal(img, rimg)


# ---- 8. the launch-time trial ---------------------------------------------------------------------------------------------------------------
def test_trial_untouched(capi):
    """cornell 480 x 270 N = 4: the job's trial times its candidates over the first rtgo_launch calls.  Batched calls in between take no
    part: the trial launches are those of the rtgo_launch calls alone, the trial settles, and from then on a batched call walks the
    structure the trial chose"""
    W, H, N = 480, 270, 4
    t = tables("cornell", W, H)
    singles = 8
    alone = play(capi, t, W, H, N, [0] * singles)
    assert alone[2]["launches_trial"] > 0 and alone[3][-1] & 8 == 0, alone[3]   # there is a trial, and eight launches settle it
    calls = [0, 2] * singles
    mixed = play(capi, t, W, H, N, calls)
    assert mixed[2]["launches_trial"] == alone[2]["launches_trial"], (mixed[2], alone[2])
    for k, v in zip(calls, mixed[3]):
        assert not (k > 1 and v & 8), mixed[3]          # no batched call is a trial launch
        assert bool(v & BATCHED_BIT) == (k > 1), mixed[3]
    assert mixed[3][-2] & 8 == 0                          # settled
    assert mixed[3][-1] & 2 == mixed[3][-2] & 2           # ... and the batched call uses the choice
    ref = play(capi, t, W, H, N, [0] * (3 * singles))
    assert np.array_equal(mixed[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(mixed[1], ref[1])


# ---- 9. fallbacks ---------------------------------------------------------------------------------------------------------------------------
def check_fallback(capi, t, W, H, N, K, what, **kw):
    got = play(capi, t, W, H, N, [K], **kw)
    ref = play(capi, t, W, H, N, [0] * K, **kw)
    assert_same(got, ref, what)
    assert got[3][-1] & BATCHED_BIT == 0, (what, got[3])
    assert got[2]["launches"] == K, (what, got[2])
    return got


def test_fallback_more_than_16_spp(capi):
    check_fallback(capi, tables("cornell", 96, 54), 96, 54, 5, 3, "25 spp")


def test_fallback_collect_stats(capi):
    got = check_fallback(capi, tables("cornell", 96, 54), 96, 54, 2, 3, "collect_stats = 2", stats=2)
    assert got[2]["node_visits"] > 0 and got[2]["launches_canonical"] == 3


def test_fallback_beyond_the_far_field_guard(capi):
    got = check_fallback(capi, tables("cornell", 96, 54), 96, 54, 2, 3, "beyond the guard", eye=(0.0, 0.0, 510.0))
    assert got[2]["guard_reach"] > 500.0 and got[2]["launches_canonical"] == 3 and got[3][-1] & 4


def test_fallback_large_scene(capi):
    """a scene through rtgo_set_large_scene: 300 spheres, one at the centroid of every triangle of the 300-triangle fixture
    tests/golden/build_closure/sphere300.npz (every tenth an emitter), seen by cornell's camera"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "build_closure", "sphere300.npz"))
    pos, idx = z["in/positions"], z["in/indices"]
    cen = pos[idx].mean(axis=1).astype(np.float32)
    n = len(cen)
    assert n == 300
    t = dict(tables("cornell", 64, 36))
    M = np.zeros((n, 16), np.float32)
    M[:, 0] = M[:, 5] = M[:, 10] = 0.08
    M[:, 15] = 1.0
    M[:, 3], M[:, 7], M[:, 11] = cen[:, 0], cen[:, 1], cen[:, 2]
    mat = np.zeros((n, 10), np.float32)
    mat[:, 0:3] = (0.7, 0.6, 0.5)
    mat[::10, 7:10] = 1.0
    t.update(type=np.full(n, capi.SPHERE, np.int32), M=M, mat=mat, aabb=None)
    got = check_fallback(capi, t, 64, 36, 2, 3, "large scene", large=True)
    assert got[3][-1] & 32 and got[2]["rays_total"] > 0


# ---- 10. errors -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame_count,n_frames", [(0, 0), (7, 0), (0xFFFFFFFE, 3), (0xFFFFFFFF, 2)])
def test_invalid_frame_counts(capi, frame_count, n_frames):
    t = tables("cornell", 64, 36)
    ctx = context(capi, t, 64 * 36)
    fr = capi.make_frame(64, 36, 2, frame_count)
    assert ctx._lib.rtgo_launch_frames(ctx._h, C.byref(fr), n_frames) == RTGO_E_INVALID
    ctx.sync()
    st = ctx.stats()
    assert st["launches"] == 0 and st["rays_total"] == 0 and st["rays_culled"] == 0 and st["last_variant"] == 0, st
    assert not ctx.read_accum(36, 64).any()
    ctx.close()


def test_rtgo_launch_checks_apply(capi):
    t = tables("cornell", 64, 36)
    ctx = context(capi, t, 64 * 36)
    bad = capi.make_frame(64, 36, 2, 0, window=(10, 10, 64, 36))      # window outside the image
    assert ctx._lib.rtgo_launch_frames(ctx._h, C.byref(bad), 3) == ctx._lib.rtgo_launch(ctx._h, C.byref(bad)) == RTGO_E_INVALID
    bad = capi.make_frame(64, 36, 2, 0, bands=(4, 2, 2))              # rank >= n_ranks
    assert ctx._lib.rtgo_launch_frames(ctx._h, C.byref(bad), 3) == RTGO_E_INVALID
    assert ctx.stats()["launches"] == 0
    ctx.close()


# ---- 11. the C++ host ------------------------------------------------------------------------------------------------------------------------
def test_host_renderer_batched(capi):
    from raytracingo_amd import scene
    acc1, img1, st1 = scene.host_render("cornell", "path", 160, 90, sample=2, frames=7)
    acc3, img3, st3 = scene.host_render_batched("cornell", "path", 160, 90, sample=2, frames=7, frames_per_launch=3)
    assert np.array_equal(acc3.view(np.uint32), acc1.view(np.uint32)) and np.array_equal(img3, img1)
    assert st3["rays_total"] == st1["rays_total"]
    assert st1["launches"] == 7 and st3["launches"] == 3      # frames 0-2, 3-5, 6
    accd, imgd, std = scene.host_render_batched("cornell", "path", 160, 90, sample=2, frames=7, frames_per_launch=1)
    assert np.array_equal(accd.view(np.uint32), acc1.view(np.uint32)) and std["launches"] == 7


def test_host_multi_gpu_driver_batched(capi):
    """two shares on one GPU, 11 frames, presented every 5th, up to 4 frames per launch: launches of 4, 1, 4, 1, 1 frames per share"""
    from raytracingo_amd import scene
    W, H, n, frames = 200, 90, 2, 11
    acc1, img1, st1 = scene.host_render("mirror_spheres", "path", W, H, sample=n, frames=frames)
    acc2, img2, st2, _ = scene.host_render_multi_batched("mirror_spheres", "path", W, H, sample=n, frames=frames, devices=(0,),
                                                         launches_per_device=2, present_every=5, frames_per_launch=4)
    assert np.array_equal(img2, img1) and np.array_equal(acc2.view(np.uint32), acc1.view(np.uint32))
    assert st2["rays_total"] == st1["rays_total"] and st2["launches"] == 5


def test_cli_frames_per_launch(capi, tmp_path):
    exe = os.path.join(ROOT, "raytracingo_amd", "rtgo_engine")
    files = []
    for extra in ([], ["--frames-per-launch=3"]):
        ppm = str(tmp_path / ("o%d.ppm" % len(files)))
        r = subprocess.run([exe, "--scene=cornell", "--mode=path", "--dim=80x48", "--sample=2", "--frames=5", "--out=" + ppm] + extra,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        files.append(open(ppm, "rb").read())
    assert len(files[0]) > 80 * 48 * 3 and files[0] == files[1]
