"""developer tool: rtgo_whitted_shade_rays against rtgo_whitted_launch on the same picture, steady state
   python tools/whitted_shade_perf.py [W] [H]
A W x H (1920 x 1080) pinhole view of the WaterBottle fixture (rtgo_whitted_set_mesh, three textures) and of whitted_instances.tori_scene()
(rtgo_whitted_set_scene, 21 instances), subframe 0: through the launch, and through the new call on the launch's own rays (the host raygen
of tests/whitted_shade_rays_ref.py) in raster order and in the order of the launch's 8 x 8 tiles (tile after tile, row-major in each).
HIP-event times on the context's stream, medians of 15 calls after 3.  Both orders are checked to leave the launch's two buffers bit for
bit.  The call does the launch's walks plus 32 B read and 20 B written per ray; DESIGN.md section 3.5 has the numbers."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import whitted_scene
import whitted_instances as WI
import whitted_shade_rays_ref as SR
from raytracingo_amd import capi

W = int(sys.argv[1]) if len(sys.argv) > 1 else 1920
H = int(sys.argv[2]) if len(sys.argv) > 2 else 1080
WARM, REPS = 3, 15


def frame(eye, look, fov):
    # pinhole frame like sutil::Camera::UVWFrame (float64 here: a timing tool, not a parity test)
    eye, look, up = np.array(eye, float), np.array(look, float), np.array([0.0, 1.0, 0.0])
    Wv = look - eye
    U = np.cross(Wv, up)
    U /= np.linalg.norm(U)
    V = np.cross(U, Wv)
    V /= np.linalg.norm(V)
    vlen = np.linalg.norm(Wv) * np.tan(0.5 * np.radians(fov))
    return np.concatenate([eye, U * vlen * W / H, V * vlen, Wv]).astype(np.float32)


def tile_order():
    """pixel indices of the W x H image, 8 x 8 tile after tile (tiles row-major, pixels row-major in each; edge tiles cut)"""
    idx = np.arange(W * H).reshape(H, W)
    return np.concatenate([idx[y:y + 8, x:x + 8].reshape(-1) for y in range(0, H, 8) for x in range(0, W, 8)])


def median_ms(stream, call):
    ms = []
    for k in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if k >= WARM:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms)


def case(name, ctx, cam, lights, miss, stream):
    ctx.set_stream(stream.cuda_stream)
    ctx.whitted_set_lights(lights)
    ctx.whitted_set_miss_color(miss)
    ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])
    ctx.resize(W * H)
    n = W * H
    o, d = SR.raygen32(cam, W, H, 0)
    rays = capi.make_rays(o, d, SR.TMIN, SR.TMAX)
    order = tile_order()
    d_acc = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
    d_img = torch.empty((n, 4), dtype=torch.uint8, device="cuda:0")
    launch_ms, launch_best = median_ms(stream, lambda: ctx.whitted_launch(W, H, 0))
    ctx.sync()
    acc, img = ctx.read_accum(H, W).reshape(n, 4), ctx.read_image(H, W).reshape(n, 4)
    hit = float((acc[:, :3] != np.float32(miss)).any(axis=1).mean())
    print("%s, %d x %d, %.1f %% of the pixels hit: rtgo_whitted_launch median %.4f ms (best %.4f), %.2f Gray/s primary" %
          (name, W, H, 100.0 * hit, launch_ms, launch_best, n / launch_ms / 1e6), flush=True)
    for what, perm in (("raster order", None), ("8 x 8-tile order", order)):
        r = rays if perm is None else rays[perm]
        d_rays = torch.from_numpy(r.view(np.float32).reshape(-1, 8)).to("cuda:0")
        stream.synchronize()

        def call():
            rc = ctx.whitted_shade_rays_raw(d_rays.data_ptr(), d_acc.data_ptr(), d_img.data_ptr(), n, 0)
            assert rc == 0, rc

        ms, best = median_ms(stream, call)
        ctx.sync()
        a, i = d_acc.cpu().numpy(), d_img.cpu().numpy()
        want_a, want_i = (acc, img) if perm is None else (acc[perm], img[perm])
        same = np.array_equal(a.view(np.uint32), want_a.view(np.uint32)) and np.array_equal(i, want_i)
        print("    rtgo_whitted_shade_rays, %-16s median %.4f ms (best %.4f)  %.2fx the launch  (the launch's buffers bit for bit: %s)" %
              (what + ":", ms, best, ms / launch_ms, same), flush=True)
        # without the 8-bit image: 16 B written per ray
        ms16, _ = median_ms(stream, lambda: ctx.whitted_shade_rays_raw(d_rays.data_ptr(), d_acc.data_ptr(), 0, n, 0))
        print("    %-42s median %.4f ms  %.2fx the launch" % ("  ... without the image:", ms16, ms16 / launch_ms), flush=True)
    ctx.close()


stream = torch.cuda.Stream(device="cuda:0")
with torch.cuda.stream(stream):
    print("whitted shade_rays against the launch, medians of %d calls after %d" % (REPS, WARM), flush=True)
    wb = whitted_scene.waterbottle()
    ctx = capi.Context(0)
    ctx.whitted_set_mesh(wb["positions"], wb["normals"], wb["indices"], None, wb["materials"])
    ctx.whitted_set_texcoords(wb["texcoords"])
    for mi, (bc, mr, nm) in wb["textures"].items():
        ctx.whitted_set_material_textures(mi, bc, mr, nm)
    case("WaterBottle (%d triangles, set_mesh)" % len(wb["indices"]), ctx, frame([0.12, 0.08, 0.42], [0.0, 0.0, 0.0], 40.0), wb["lights"], wb["miss"], stream)
    meshes, inst = WI.tori_scene()
    ctx = capi.Context(0)
    ctx.whitted_set_scene(meshes, inst, WI.materials())
    lt = WI.lights()
    case("tori (%d instances, set_scene)" % len(inst), ctx, frame([0.5, 4.0, 6.0], [0.0, 0.4, -0.5], 45.0), lt["lights"], lt["miss"], stream)
