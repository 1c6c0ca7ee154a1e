"""developer tool: one GPU's share of a G-way row-band split of a whitted frame (rtgo_whitted_launch_frame), steady state
   python tools/whitted_share_perf.py small [W] [H]   tests/whitted_scene.build(40, 48) (3758 triangles, rtgo_whitted_set_mesh)
   python tools/whitted_share_perf.py big [W] [H]     whitted_inst_perf.py big's scene: a 1 M-triangle clustered torus on a ground
Rank 0's share at 1/2, 1/4 and 1/8 of a 4-, 8-, 16- and 32-row interleave: ms per launch (HIP events), and the kernel-only projection
full / share at 2, 4 and 8 GPUs; then the same counts of contiguous row blocks (the slowest block).  The floor line is one 8 x 8
window: one tile's latency and the fixed cost of a launch.  Last, the 1/8 share of the 4-row interleave with n = 2, 4, 8, 16 subframes to
a launch (rtgo_whitted_launch_frames).  DESIGN.md section 6 has the numbers."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import whitted_scene
import whitted_instances as WI
import whitted_big_meshes as BM
from raytracingo_amd import capi

what = sys.argv[1] if len(sys.argv) > 1 else "small"
W = int(sys.argv[2]) if len(sys.argv) > 2 else 1920
H = int(sys.argv[3]) if len(sys.argv) > 3 else 1080
K = 20


def frame(eye, look, fov=45.0):
    # pinhole frame like sutil::Camera::UVWFrame (float64 here: a timing tool, not a parity test)
    eye, look, up = np.array(eye, float), np.array(look, float), np.array([0.0, 1.0, 0.0])
    Wv = look - eye
    U = np.cross(Wv, up); U /= np.linalg.norm(U)
    V = np.cross(U, Wv); V /= np.linalg.norm(V)
    vlen = np.linalg.norm(Wv) * np.tan(0.5 * np.radians(fov))
    return [a.astype(np.float32) for a in (eye, U * vlen * W / H, V * vlen, Wv)]


def time_share(ctx, window=None, bands=(4, 1, 0)):
    h = window[3] if window else H
    w = window[2] if window else W
    ctx.resize(max(w * capi.local_rows(h, *bands), 1))
    for sf in range(3):
        ctx.whitted_launch_frame(capi.make_whitted_frame(W, H, sf, window=window, bands=bands))
    ctx.sync()
    ctx.reset_stats()
    for sf in range(K):
        ctx.whitted_launch_frame(capi.make_whitted_frame(W, H, 3 + sf, window=window, bands=bands))
    ctx.sync()
    st = ctx.stats()
    return st["total_launch_ms"] / K, st["rays_total"] / K


def time_share_frames(ctx, n, bands):
    """ms per SUBFRAME of the share with n subframes to a launch, over subframes 3 .. (K rounded up to whole launches)"""
    calls = (K + n - 1) // n
    ctx.resize(max(W * capi.local_rows(H, *bands), 1))
    ctx.whitted_launch_frames(capi.make_whitted_frame(W, H, 0, bands=bands), 3)
    ctx.sync()
    ctx.reset_stats()
    for k in range(calls):
        ctx.whitted_launch_frames(capi.make_whitted_frame(W, H, 3 + k * n, bands=bands), n)
    ctx.sync()
    st = ctx.stats()
    return st["total_launch_ms"] / (calls * n), st["rays_total"] / (calls * n)


ctx = capi.Context(0)
if what == "small":
    mesh = whitted_scene.build(n_lat=40, n_lon=48)
    ctx.whitted_set_mesh(mesh["positions"], mesh["normals"], mesh["indices"], mesh["tri_material"], mesh["materials"])
    lights, miss, cam = mesh["lights"], mesh["miss"], frame([0.5, 3.0, 7.0], [0.0, 1.0, 0.0])
    label = "%d triangles" % len(mesh["indices"])
else:
    big = BM.displaced_torus(1000, 500, R=1.0, r=0.35, amp=0.04, freq=(23, 11), texcoords=False)   # 1 000 000 triangles
    ctx.whitted_set_scene([WI.ground(4.0, -0.5, normals=True), big], [(np.eye(3, 4, dtype=np.float32), 0, 0), (np.eye(3, 4, dtype=np.float32), 1, 1)],
                          WI.materials())
    lt = WI.lights()
    lights, miss, cam = lt["lights"], lt["miss"], frame([0.4, 1.6, 2.6], [0.0, -0.1, 0.0], 45.0)
    label = "1 000 002 triangles (clustered)"
ctx.whitted_set_lights(lights)
ctx.whitted_set_miss_color(miss)
ctx.set_camera(*cam)

full_ms, full_rays = time_share(ctx)
floor_ms, _ = time_share(ctx, window=(W // 2, H // 2, 8, 8))
print("whitted %dx%d, %s: full frame %.4f ms (%.2f Gray/s); floor (one 8 x 8 window) %.4f ms" %
      (W, H, label, full_ms, full_rays / full_ms / 1e6, floor_ms))
for band_h in (4, 8, 16, 32):
    for G in (2, 4, 8):
        ms, rays = time_share(ctx, bands=(band_h, G, 0))
        print("  band_h %d share 1/%d (rank 0, %d rows): %.4f ms, %.2f Gray/s, %.1f %% of the rays; kernel-only projection at %d GPUs: %.2fx" %
              (band_h, G, capi.local_rows(H, band_h, G, 0), ms, rays / ms / 1e6, 100.0 * rays / full_rays, G, full_ms / ms))
# for comparison: G contiguous blocks of rows (a window each, no interleave); the slowest block sets the frame
for G in (2, 4, 8):
    per = [time_share(ctx, window=(0, g * H // G, W, (g + 1) * H // G - g * H // G)) for g in range(G)]
    slow = max(range(G), key=lambda g: per[g][0])
    print("  %d contiguous blocks: slowest (block %d) %.4f ms, %.1f %% of the rays, fastest %.4f ms; kernel-only projection at %d GPUs: %.2fx" %
          (G, slow, per[slow][0], 100.0 * per[slow][1] / full_rays, min(p[0] for p in per), G, full_ms / per[slow][0]))
# n subframes of one 1/8 share to a launch
one_ms, _ = time_share(ctx, bands=(4, 8, 0))
for n in (2, 4, 8, 16):
    ms, rays = time_share_frames(ctx, n, (4, 8, 0))
    print("  band_h 4 share 1/8, %2d subframes per launch (rtgo_whitted_launch_frames): %.4f ms/subframe, %.2f Gray/s, %.2fx the single launches (%.4f ms)" %
          (n, ms, rays / ms / 1e6, one_ms / ms, one_ms))
ctx.close()
