"""developer tool: rtgo_shade_rays against rtgo_launch on the same picture, steady state
   python tools/shade_perf.py [W] [H] [log file]
A W x H (1920 x 1080) pinhole view of cornell and of balls, path and distributed mode, frame 0, sqrt_spp 1, max_trace_depth 5: through
rtgo_launch with collect_stats = 0 (the fast walk) and with collect_stats = 2 (the canonical walk, the one the new kernel takes; and,
for the record, with collect_stats = 1, the canonical walk over every pixel, culled ones included), and through rtgo_shade_rays on the launch's own rays and seeds (the host raygen of tests/shade_rays_ref.py).  At sqrt_spp 1 a unit of the
launch is 64 neighbouring pixels of a row, so for widths that are a multiple of 64 the launch's unit order IS the raster order: one
order serves both.  First the call's two buffers are checked against the launch's, bit for bit.  Then HIP-event times on the context's
stream: ROUNDS rounds, in each the three calls alternate, 3 warm-up turns and 15 timed ones, and a round's figure is the median of its
15; the spread of the rounds' medians is printed beside them, since "no slower than" only means something beyond it.  The call does the
instrumented launch's walks without its counters, plus 36 B read and 20 B written per ray.  DESIGN.md section 3.5.2 has the numbers."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import shade_rays_ref as R
from raytracingo_amd import capi, scene

W = int(sys.argv[1]) if len(sys.argv) > 1 else 1920
H = int(sys.argv[2]) if len(sys.argv) > 2 else 1080
LOG = open(sys.argv[3], "w") if len(sys.argv) > 3 else None
WARM, REPS, ROUNDS = 3, 15, 5
MAX_DEPTH = 5


def say(text):
    print(text, flush=True)
    if LOG:
        LOG.write(text + "\n")
        LOG.flush()


def timed(stream, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def case(name, path, stream):
    t = scene.tables(name, W, H)
    n = W * H
    ctx = capi.Context(0)
    ctx.set_stream(stream.cuda_stream)
    ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
    c = t["cam"]
    ctx.set_camera(c[0:3], c[3:6], c[6:9], c[9:12])
    ctx.set_background(t["bg"])
    ctx.set_lights(t["lights"])
    ctx.resize(n)
    o, d, seed = R.raygen32(c, W, H, 0)
    rays = capi.make_rays(o, d, R.T_MIN0, R.T_MAX0)
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).to("cuda:0")
    d_seed = torch.from_numpy(seed.view(np.int32)).to("cuda:0")
    d_acc = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
    d_img = torch.empty((n, 4), dtype=torch.uint8, device="cuda:0")
    opt = capi.ShadeOptions(MAX_DEPTH, int(path), 0, 0)
    frames = {k: capi.make_frame(W, H, 1, 0, path, False, max_depth=MAX_DEPTH, stats=k) for k in (0, 1, 2)}

    def shade():
        rc = ctx.shade_rays_raw(d_rays.data_ptr(), d_seed.data_ptr(), d_acc.data_ptr(), d_img.data_ptr(), n, opt)
        assert rc == 0, rc

    calls = {"rtgo_launch, collect_stats 0 (fast walk)": lambda: ctx.launch(frames[0]),
             "rtgo_launch, collect_stats 2 (canonical walk)": lambda: ctx.launch(frames[2]),
             # (for the record: the canonical launch that traces every pixel, as the call must -- 0 and 2 write the pixels no primary
             # ray of which can reach the scene's bounds without tracing them)
             "rtgo_launch, collect_stats 1 (every pixel)": lambda: ctx.launch(frames[1]), "rtgo_shade_rays": shade}
    # the buffers first: the launch's, bit for bit
    ctx.launch(frames[0])
    ctx.sync()
    acc, img = ctx.read_accum(H, W).reshape(n, 4), ctx.read_image(H, W).reshape(n, 4)
    stream.synchronize()
    shade()
    ctx.sync()
    same = np.array_equal(d_acc.cpu().numpy().view(np.uint32), acc.view(np.uint32)) and np.array_equal(d_img.cpu().numpy(), img)
    hit = float((acc[:, :3] != t["bg"]).any(axis=1).mean())
    say("%s, %s mode, %d x %d, %.1f %% of the pixels hit; the call's buffers are the launch's bit for bit: %s" %
        (name, "path" if path else "distributed", W, H, 100.0 * hit, same))
    assert same
    medians = {k: [] for k in calls}
    for r in range(ROUNDS):
        ms = {k: [] for k in calls}
        for turn in range(WARM + REPS):
            for k, call in calls.items():
                v = timed(stream, call)
                if turn >= WARM:
                    ms[k].append(v)
        for k in calls:
            medians[k].append(float(np.median(ms[k])))
    base = float(np.median(medians["rtgo_launch, collect_stats 2 (canonical walk)"]))
    for k in calls:
        m = medians[k]
        say("    %-46s median of %d rounds' medians %.4f ms  (rounds %s; spread %.4f ms = %.1f %%)  %.2fx the canonical launch" %
            (k + ":", ROUNDS, float(np.median(m)), " ".join("%.4f" % v for v in m), max(m) - min(m), 100.0 * (max(m) - min(m)) / float(np.median(m)),
             float(np.median(m)) / base))
    ctx.close()


stream = torch.cuda.Stream(device="cuda:0")
with torch.cuda.stream(stream):
    say("rtgo_shade_rays against rtgo_launch: %d rounds, each the median of %d alternating calls after %d" % (ROUNDS, REPS, WARM))
    for name in ("cornell", "balls"):
        for path in (True, False):
            case(name, path, stream)
