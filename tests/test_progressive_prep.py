"""Progressive frames: a launch of the 6-waves lock-step kernel (launches of >= 8 units per wave) hashes the next frame's pixel seeds
when its queue runs dry, and the next launch on the same context reads them instead of hashing (rtgo_debug_seeds says which launches
did: bit 0 read, bit 1 wrote).  Frames must come out bit for bit as from contexts that never reuse anything: every frame below is
rendered again on a fresh context, into the same accumulation buffer.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def new_context(t, cam, out):
    from raytracingo_amd import capi
    ctx = capi.Context(0)
    ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
    ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])
    ctx.set_background(t["bg"])
    ctx.set_lights(t["lights"])
    acc, img = out
    ctx.bind_output(acc.data_ptr(), img.data_ptr(), acc.shape[0] * acc.shape[1])
    return ctx


def seeds_flags(ctx):
    L = ctx._lib
    L.rtgo_debug_seeds.restype = C.c_int
    L.rtgo_debug_seeds.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    v = C.c_uint32(0)
    assert L.rtgo_debug_seeds(ctx._h, C.byref(v)) == 0
    return v.value


def moved(cam):
    c = np.array(cam, dtype=np.float64).copy()
    c[0:3] += np.array([1.5, -1.0, 0.5])   # the eye moves far enough for the scene's screen rectangle (the strip layout) to move
    return c


def run(name, W, H, N, frames, bands=(4, 1, 0), camera_at=None, path=True, windows=None):
    """frames: the frame indices launched in turn; camera_at: from that launch on, the moved camera; windows: per launch, the window
    (None: the whole image).  Returns, per launch, the accumulation buffer and image of one context that renders the whole sequence
    and of fresh contexts, the seed flags, and the context's trial launches."""
    import torch
    from raytracingo_amd import bands as B, capi, scene
    t = scene.tables(name, W, H)
    band_h, n_ranks, rank = bands
    rows = B.max_local_rows(H, band_h, n_ranks) if n_ranks > 1 else H
    outs = [(torch.zeros((rows, W, 4), dtype=torch.float32, device="cuda"), torch.zeros((rows, W, 4), dtype=torch.uint8, device="cuda"))
            for _ in range(2)]
    torch.cuda.synchronize()   # (the contexts launch on streams of their own)
    wins = windows or [None] * len(frames)
    cams = [moved(t["cam"]) if (camera_at is not None and i >= camera_at) else t["cam"] for i in range(len(frames))]
    ctx = new_context(t, cams[0], outs[0])
    seq, flags = [], []
    for i, f in enumerate(frames):
        if i > 0 and cams[i] is not cams[i - 1]:
            c = cams[i]
            ctx.set_camera(c[0:3], c[3:6], c[6:9], c[9:12])
        ctx.launch(capi.make_frame(W, H, N, f, path, window=wins[i], bands=bands))
        flags.append(seeds_flags(ctx))
        ctx.sync()
        seq.append((outs[0][0].cpu().numpy().copy(), outs[0][1].cpu().numpy().copy()))
    trials = ctx.stats()["launches_trial"]
    ctx.close()
    fresh = []
    for i, f in enumerate(frames):
        c = new_context(t, cams[i], outs[1])
        c.launch(capi.make_frame(W, H, N, f, path, window=wins[i], bands=bands))
        assert seeds_flags(c) & 1 == 0
        c.sync()
        fresh.append((outs[1][0].cpu().numpy().copy(), outs[1][1].cpu().numpy().copy()))
        c.close()
    return seq, fresh, flags, trials


def assert_same(name, seq, fresh):
    for i, ((a, im), (ra, rim)) in enumerate(zip(seq, fresh)):
        assert np.array_equal(a.view(np.uint32), ra.view(np.uint32)), (name, i, "accumulation buffers differ")
        assert np.array_equal(im, rim), (name, i, "images differ")


@pytest.mark.parametrize("name,W,H,N", [("cornell", 1920, 1080, 4), ("cornell", 3840, 2160, 4), ("cornell", 1920, 1080, 3)])
def test_consecutive_frames_are_pre_seeded_and_unchanged(name, W, H, N):
    seq, fresh, flags, _ = run(name, W, H, N, [0, 1, 2, 3])
    assert_same(name, seq, fresh)
    assert flags[0] == 2, flags                 # the first launch hashes inline and writes the next frame's seeds
    assert flags[1:] == [3, 3, 3], flags        # launches 2..N read them


@pytest.mark.parametrize("name,W,H,N,path", [("cornell", 480, 270, 4, True), ("plateau", 480, 270, 4, True),
                                             ("checkered", 1920, 1080, 3, True), ("cornell", 480, 270, 2, False)])
def test_launches_without_the_seed_pass_are_unchanged(name, W, H, N, path):
    # few units per wave (a small frame), scenes whose LDS image or primitives keep them off the 6-waves kernel, distributed mode:
    # other kernel variants, which hash inline
    seq, fresh, flags, _ = run(name, W, H, N, [0, 1, 2], path=path)
    assert_same(name, seq, fresh)
    assert flags == [0, 0, 0], flags


def test_camera_change_mid_sequence():
    seq, fresh, flags, _ = run("cornell", 1920, 1080, 4, [0, 1, 2, 3, 4], camera_at=2)
    assert_same("cornell camera", seq, fresh)
    # the moved eye moves the strip layout: launch 3 hashes inline, the next ones read again
    assert flags == [2, 3, 2, 3, 3], flags


def test_window_change_mid_sequence():
    wins = [None, None, (64, 32, 1600, 900), (64, 32, 1600, 900), None]
    seq, fresh, flags, _ = run("cornell", 1920, 1080, 4, [0, 1, 2, 3, 4], windows=wins)
    assert_same("cornell window", seq, fresh)
    assert flags == [2, 3, 2, 3, 2], flags


def test_skipped_and_repeated_frame_index():
    seq, fresh, flags, _ = run("cornell", 1920, 1080, 4, [0, 1, 3, 4, 4, 5])
    assert_same("cornell skipped", seq, fresh)
    assert flags == [2, 3, 2, 3, 2, 3], flags


@pytest.mark.parametrize("bands,expect", [((4, 2, 1), [2, 3, 3]), ((4, 8, 3), [0, 0, 0])])
def test_band_shares(bands, expect):
    # a 1/8 share of the 1080p frame has ~3 strips per wave: it runs the 5-waves kernel, without the seed pass
    seq, fresh, flags, _ = run("cornell", 1920, 1080, 4, [0, 1, 2], bands=bands)
    assert_same("cornell bands %s" % (bands,), seq, fresh)
    assert flags == expect, flags


def test_launch_time_trial():
    # cornell's two fast-walk structures are candidates of the trial: both run the 6-waves kernel, so every launch after the first reads
    seq, fresh, flags, trials = run("cornell", 1920, 1080, 4, [0, 1, 2, 3, 4, 5])
    assert trials > 0
    assert_same("cornell trial", seq, fresh)
    assert flags == [2, 3, 3, 3, 3, 3], flags


def test_launch_time_trial_across_kernel_variants():
    # 64 spp: the trial also alternates the lock-step and streaming loops; a launch reads seeds only right after one that wrote them
    seq, fresh, flags, trials = run("cornell", 480, 270, 8, [0, 1, 2, 3, 4, 5])
    assert trials > 0
    assert_same("cornell trial 64 spp", seq, fresh)
    for i, fl in enumerate(flags):
        assert not (fl & 1) or (i > 0 and flags[i - 1] & 2), flags
