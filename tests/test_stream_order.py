"""The stream contract of include/rtgo.h on a caller's stream, on the MI355X.

The header promises, for every call that takes device buffers, that the caller's writes need only be "ordered on the context's stream
(rtgo_set_stream)", and for the ray calls and the launches that they are "asynchronous on the context's stream".  The rest of the suite
synchronises before every call and after it.  Here a context runs on a torch side stream that is backed up behind a delay
(tests/stream_order.py): inputs are written on that stream behind the delay, calls are made with no host wait, results are cloned on the
stream, and everything is compared bit for bit with the same calls made the waited way on a second context.  A third run without the
stream's writes shows that stale inputs would have given another answer.  Stale data is always valid data.

call -> test (2: inputs written on the stream; 3: outputs cloned on the stream; 4: returned at once, while the stall was pending)
  rtgo_set_scene_device, rtgo_set_large_scene_device   2 test_set_scene_device_reads_what_the_stream_wrote
  rtgo_update_prims_device                             2 test_update_prims_device_reads_what_the_stream_wrote, test_a_refusal_is_decided_on_what_the_stream_wrote,
                                                         test_a_refusal_is_read_after_the_check_of_a_million_entries, C
  rtgo_trace_rays, rtgo_whitted_trace_rays             2 3 4 test_trace_rays_on_the_stream; 4 test_the_unwaited_drag
  rtgo_shade_rays                                      2 3 4 test_shade_rays_on_the_stream; 4 test_the_unwaited_drag
  rtgo_whitted_shade_rays                              2 3 4 test_whitted_shade_rays_on_the_stream, test_the_unwaited_whitted_drag
  rtgo_whitted_set_scene_device, _set_mesh_device,
  rtgo_whitted_set_texcoords_device                    2 test_whitted_set_calls_read_what_the_stream_wrote
  rtgo_whitted_update_meshes_device                    2 test_whitted_update_meshes_device_reads_what_the_stream_wrote, C
  rtgo_whitted_set_instances_device                    2 test_whitted_set_instances_device_reads_what_the_stream_wrote, C
  rtgo_launch, rtgo_launch_frames, rtgo_whitted_launch,
  rtgo_whitted_launch_frames                           3 4 test_launch_outputs_are_ordered_on_the_stream
  rtgo_whitted_launch_frame                            3 4 test_two_contexts_on_two_streams
  rtgo_assemble_bands                                  3 4 test_assemble_bands_on_the_stream
  C test_the_chain   D test_the_unwaited_drag, test_the_unwaited_whitted_drag   E test_a_backlog_deeper_than_the_event_ring
  F test_set_stream_waits_and_moves_the_work, test_null_is_the_contexts_own_stream   G test_two_contexts_on_two_streams"""
import re

import numpy as np
import pytest

import shade_rays_ref as SR
import stream_order as SO
import test_prims_device as TP
import test_update_prims as TU
import test_whitted_instances_device as TI
import test_whitted_update_device as TWD
import test_whitted_update_meshes as TWM
from test_trace_rays import Knob
import trace_rays_ref as TR
import whitted_instances as WI

pytestmark = pytest.mark.gpu

W, H = 48, 36              # analytic frames
WW, WH = TWM.W, TWM.H      # whitted frames, 64 x 48
N_RAYS = 4096
E_INVALID = 1


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def capi(torch):
    from raytracingo_amd import capi as m
    m.load()
    if torch.cuda.is_available():
        torch.cuda.init()   # torch's HIP runtime up before this module's first context (the tests hand the library torch tensors)
    return m


@pytest.fixture(scope="module", autouse=True)
def host_times(torch):
    """after the module: the stall's calibration and the idle-stream host time of every asynchronous call (shown with -s)"""
    yield
    cal = {k: v for k, v in SO.calibrate(torch).items() if k != "m"}
    print("\nstall: %r, %g ms; idle-stream host times in ms: %s" % (cal, SO.STALL_MS, {k: round(v, 3) for k, v in sorted(SO.IDLE_MS.items())}))
    assert 20.0 * max(SO.IDLE_MS.values(), default=0.0) <= SO.STALL_MS, "the stall is no longer 20 x the slowest asynchronous call: measure again (DESIGN.md section 4)"


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
_made = {}


def analytic(oracle, name, w=W, h=H):
    key = (name, w, h)
    if key not in _made:
        _made[key] = oracle.scene_tables(oracle.scene(name, w, h))
    return _made[key]


def box_moved(oracle, t, which):
    """cornell with its short box (6-11) or its tall box (12-17) moved: (indices, tables)"""
    idx, d = (np.arange(6, 12), (-0.6, 0.0, 0.9)) if which == "short" else (np.arange(12, 18), (0.5, 0.0, -0.4))
    return idx, TU.edit(oracle, t, idx, M=TU.moved(t["M"][idx], d))


def shifted(cam, d):
    """the camera with its eye moved by d (U, V, W kept)"""
    cam = np.array(cam, np.float32)
    cam[0:3] += np.asarray(d, np.float32)
    return cam


def look(ctx, cam):
    ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])


def analytic_ctx(ctx, t, large=False):
    return TU.set_scene(ctx, t, large)


def whitted_small():
    """a 16 x 8 torus with normals and an octahedron without, five instances"""
    if "whitted" not in _made:
        rng = np.random.RandomState(3)
        meshes = [WI.torus(16, 8), WI.octahedron(0.3)]
        inst = [(WI.transform(WI.rotation(rng), [-0.7, 0.2, 0.1]), 0, 1), (WI.transform(WI.rotation(rng) @ np.diag([1.0, 0.6, 1.3]), [0.7, 0.3, 0.3]), 1, 0),
                (WI.transform(0.7 * WI.rotation(rng), [0.0, -0.4, 0.6]), 0, 2), (WI.transform(WI.mirror(rng), [0.1, 0.7, -0.5]), 1, 3),
                (WI.transform(np.eye(3), [0.0, 0.0, 0.0]), 1, 2)]
        _made["whitted"] = (meshes, inst)
    return _made["whitted"]


def whitted_ctx(capi, oracle, ctx, meshes, inst, view_of=None, set_scene=True):
    """ctx with the lights, miss colour and camera that show (view_of or meshes, inst), and the scene unless told otherwise: the camera"""
    cam, extra = TWM.world_view(oracle, view_of or meshes, inst)
    if set_scene:
        ctx.whitted_set_scene(meshes, inst, WI.materials())
    ctx.whitted_set_lights(extra["lights"])
    ctx.whitted_set_miss_color(extra["miss"])
    look(ctx, cam)
    return cam


def deformed(mesh, k=1.0):
    """(positions, normals or None) of the mesh bent: valid vertices that give another picture"""
    p = mesh["positions"].astype(np.float64)
    if mesh.get("normals") is None:
        return (p[:, [2, 0, 1]] * (1.0 + 0.4 * k)).astype(np.float32), None
    return (p + 0.08 * k * np.sin(9.0 * p[:, [2, 0, 1]]) * mesh["normals"] + 0.1 * k * np.array([1.0, 1.0, -1.0])).astype(np.float32), TWD.new_normals(mesh)


def frame(capi, f=0, w=W, h=H, **kw):
    return capi.make_frame(w, h, 1, f, True, False, **kw)


# ---- A. inputs ordered on the stream ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("large", [False, True], ids=["set_scene_device", "set_large_scene_device"])
def test_set_scene_device_reads_what_the_stream_wrote(capi, torch, oracle, large):
    t_a = analytic(oracle, "cornell")
    _, t_b = box_moved(oracle, t_a, "short")

    def case(R, stale):
        ctx = R.ctx
        TP.view(ctx, t_a)
        _, prims, boxes = R.keep(*TP.tensors(torch, capi, t_a)[0:3])
        _, new_prims, new_boxes = R.keep(*TP.tensors(torch, capi, t_b)[0:3])
        acc, img = R.bound(W * H)
        R.begin()
        with R.on():
            if not stale:
                prims.copy_(new_prims)
                boxes.copy_(new_boxes)
            SO.ok(capi, ctx, R.call(SO.raw_set_scene_device, capi, ctx, prims, boxes, large))
            R.call(ctx.launch, frame(capi))
            return {"accum": acc.clone(), "image": img.clone()}

    SO.wrote_all(SO.regimes(torch, capi, case), ["accum"])


@pytest.mark.parametrize("rebuild", [False, True], ids=["refit", "rebuild"])
@pytest.mark.parametrize("large", [False, True], ids=["resident", "large"])
def test_update_prims_device_reads_what_the_stream_wrote(capi, torch, oracle, large, rebuild):
    t0 = analytic(oracle, "cornell")
    idx_a, t_a = box_moved(oracle, t0, "short")
    idx_b, t_b = box_moved(oracle, t0, "tall")

    def case(R, stale):
        ctx = analytic_ctx(R.ctx, t0, large)
        acc, img = R.bound(W * H)
        ctx.launch(frame(capi))   # (a mask, seeds and a trial over the old scene)
        ctx.sync()
        bufs = R.keep(*TP.tensors(torch, capi, t_a, idx_a))
        new = R.keep(*TP.tensors(torch, capi, t_b, idx_b))
        R.begin()
        with R.on():
            if not stale:
                for dst, src in zip(bufs, new):
                    dst.copy_(src)
            SO.ok(capi, ctx, R.call(SO.raw_update_prims_device, capi, ctx, bufs[0], bufs[1], bufs[2], rebuild))
            R.call(ctx.launch, frame(capi))
            return {"accum": acc.clone(), "image": img.clone()}

    SO.wrote_all(SO.regimes(torch, capi, case), ["accum"])


@pytest.mark.parametrize("large", [False, True], ids=["resident", "large"])
def test_a_refusal_is_decided_on_what_the_stream_wrote(capi, torch, oracle, large):
    """the check kernel's verdict is read after the stream's writes: indices the stream spoils are refused (the verdict of the accepted
    call before it, or of the good indices they replace, would accept them), and good indices written over the spoiled ones are accepted"""
    t0 = analytic(oracle, "cornell")
    idx, t_a = box_moved(oracle, t0, "short")

    def case(R, stale):
        ctx = analytic_ctx(R.ctx, t0, large)
        acc, img = R.bound(W * H)
        i, rec, boxes = R.keep(*TP.tensors(torch, capi, t_a, idx))
        good = R.keep(i.clone())
        bad = R.keep(i.clone())
        bad[1] = bad[0]   # (an index named twice: refused, and valid data all the same)
        SO.ok(capi, ctx, SO.raw_update_prims_device(capi, ctx, i, rec, boxes, False))   # an accepted call first: its verdict is clean
        R.begin()
        with R.on():
            if not stale:
                i.copy_(bad)
            rc_spoiled = R.call(SO.raw_update_prims_device, capi, ctx, i, rec, boxes, False)
            twice = "another entry names" in capi.load().rtgo_last_error(ctx._h).decode() if rc_spoiled else False
            if not stale:
                i.copy_(good)
            rc_good = R.call(SO.raw_update_prims_device, capi, ctx, i, rec, boxes, False)
            R.call(ctx.launch, frame(capi))
            return {"spoiled": rc_spoiled, "named twice": twice, "good": rc_good, "accum": acc.clone()}

    res = SO.regimes(torch, capi, case)
    assert res["spoiled"] == E_INVALID and res["named twice"] and res["good"] == 0, (res["spoiled"], res["named twice"], res["good"])


def sphere_grid(torch, capi, side, shade):
    """side x side small spheres on a grid in the plane y = 0, as rtgo_prim records made on the device (no boxes: the CubeBox rule)"""
    n = side * side
    k = torch.arange(n, device="cuda")
    models = torch.zeros((n, 16), dtype=torch.float32, device="cuda")
    models[:, [0, 5, 10]] = 0.2
    models[:, 15] = 1.0
    models[:, 3], models[:, 11] = (k % side) * 0.5 - 0.25 * side, (k // side) * 0.5 - 0.25 * side
    materials = torch.zeros((n, 10), dtype=torch.float32, device="cuda")
    materials[:, 0:3] = shade
    return capi.prims_tensor(torch.full((n,), capi.SPHERE, dtype=torch.int32, device="cuda"), models, materials)


def test_a_refusal_is_read_after_the_check_of_a_million_entries(capi, torch, oracle):
    """the same over 2^20 entries, the count at which the check kernel outlasts a copy that did not wait for it: every device call
    first waits for its stream, so a verdict read without waiting for the check races nothing but the check itself"""
    side = 1024
    n = side * side
    t0 = analytic(oracle, "cornell")

    def case(R, stale):
        ctx = R.ctx
        TP.view(ctx, t0)
        acc, img = R.bound(W * H)
        scene, rec = R.keep(sphere_grid(torch, capi, side, 0.7), sphere_grid(torch, capi, side, 0.3))
        good = R.keep(torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda"))
        bad = R.keep(good.clone())
        bad[n - 1] = bad[n - 2]   # (an index named twice, by the last two entries)
        i = R.keep(good.clone())
        torch.cuda.synchronize()
        SO.ok(capi, ctx, SO.raw_set_scene_device(capi, ctx, scene, None, True))
        SO.ok(capi, ctx, SO.raw_update_prims_device(capi, ctx, i, scene, None, False))   # an accepted call first: its verdict is clean
        R.begin()
        with R.on():
            if not stale:
                i.copy_(bad)
            rc_spoiled = R.call(SO.raw_update_prims_device, capi, ctx, i, rec, None, False)
            twice = "another entry names" in capi.load().rtgo_last_error(ctx._h).decode() if rc_spoiled else False
            if not stale:
                i.copy_(good)
            rc_good = R.call(SO.raw_update_prims_device, capi, ctx, i, rec, None, False)
            R.call(ctx.launch, frame(capi))
            return {"spoiled": rc_spoiled, "named twice": twice, "good": rc_good, "accum": acc.clone()}

    res = SO.regimes(torch, capi, case)
    assert res["spoiled"] == E_INVALID and res["named twice"] and res["good"] == 0, (res["spoiled"], res["named twice"], res["good"])


def trace_inputs(capi, cam, whitted):
    o, d = TR.primaries(cam, 64, 64)
    return SO.rays_tensor(capi, o, d, TWM.TMIN if whitted else TU.TMIN, TWM.TMAX if whitted else TU.TMAX)


@pytest.mark.parametrize("flags", [0, 1], ids=["closest", "any-hit"])
@pytest.mark.parametrize("path", ["resident", "large", "whitted"])
def test_trace_rays_on_the_stream(capi, torch, oracle, path, flags):
    whitted = path == "whitted"
    t = analytic(oracle, "cornell")
    meshes, inst = whitted_small()

    def case(R, stale):
        ctx = R.ctx
        cam = whitted_ctx(capi, oracle, ctx, meshes, inst) if whitted else analytic_ctx(ctx, t, path == "large") and t["cam"]
        rays = R.dev(trace_inputs(capi, cam, whitted))
        new = R.dev(trace_inputs(capi, shifted(cam, (0.3, -0.2, 0.1)), whitted))
        hits = R.keep(torch.full((N_RAYS, 8), SO.SENTINEL, dtype=torch.float32, device="cuda"))
        R.begin()
        with R.on():
            if not stale:
                rays.copy_(new)
            SO.ok(capi, ctx, R.call(ctx.trace_rays_raw, rays.data_ptr(), hits.data_ptr(), N_RAYS, flags, whitted, asynchronous=True,
                                    name="rtgo_whitted_trace_rays" if whitted else "rtgo_trace_rays"))
            got = hits.clone()
            # any-hit: hit or miss is the answer, the other fields describe some accepted hit
            return {"hits": got.view(torch.int32)[:, 1] >= 0} if flags else {"hits": got}

    SO.regimes(torch, capi, case)


def test_shade_rays_on_the_stream(capi, torch, oracle):
    """rays, seeds and the mean of the sample before (sample_index 1) are written on the stream"""
    t = analytic(oracle, "cornell")
    prev_mean = np.random.RandomState(5).rand(N_RAYS, 4).astype(np.float32)

    def inputs(cam, f):
        o, d, seed = SR.raygen32(cam, 64, 64, f)
        return SO.rays_tensor(capi, o, d, TU.TMIN, TU.TMAX), seed

    def case(R, stale):
        ctx = analytic_ctx(R.ctx, t)
        ra, sa = inputs(t["cam"], 1)
        rb, sb = inputs(shifted(t["cam"], (0.2, 0.1, -0.3)), 2)
        rays, seeds, new_rays, new_seeds = R.dev(ra), R.dev(sa), R.dev(rb), R.dev(sb)
        acc, img = R.outputs(N_RAYS)
        acc.fill_(0.25)
        prev = R.dev(prev_mean)
        opt = capi.ShadeOptions(5, 1, 0, 1)
        R.begin()
        with R.on():
            if not stale:
                rays.copy_(new_rays)
                seeds.copy_(new_seeds)
                acc.copy_(prev)
            SO.ok(capi, ctx, R.call(ctx.shade_rays_raw, rays.data_ptr(), seeds.data_ptr(), acc.data_ptr(), img.data_ptr(), N_RAYS, opt, asynchronous=True,
                                    name="rtgo_shade_rays"))
            return {"accum": acc.clone(), "image": img.clone()}

    SO.wrote_all(SO.regimes(torch, capi, case), ["accum"])


def test_whitted_shade_rays_on_the_stream(capi, torch, oracle):
    meshes, inst = whitted_small()
    prev_mean = np.random.RandomState(6).rand(N_RAYS, 4).astype(np.float32)

    def case(R, stale):
        ctx = R.ctx
        cam = whitted_ctx(capi, oracle, ctx, meshes, inst)
        rays, new_rays = R.dev(trace_inputs(capi, cam, True)), R.dev(trace_inputs(capi, shifted(cam, (0.3, -0.2, 0.1)), True))
        acc, img = R.outputs(N_RAYS)
        acc.fill_(0.25)
        prev = R.dev(prev_mean)
        R.begin()
        with R.on():
            if not stale:
                rays.copy_(new_rays)
                acc.copy_(prev)
            SO.ok(capi, ctx, R.call(ctx.whitted_shade_rays_raw, rays.data_ptr(), acc.data_ptr(), img.data_ptr(), N_RAYS, 1, asynchronous=True,
                                    name="rtgo_whitted_shade_rays"))
            return {"accum": acc.clone(), "image": img.clone()}

    SO.wrote_all(SO.regimes(torch, capi, case), ["accum"])


def mesh_tensors(R, mesh):
    return {k: (None if mesh.get(k) is None else R.dev(mesh[k])) for k in ("positions", "normals", "texcoords", "indices", "tri_material")}


def other_mesh(mesh):
    """the mesh deformed, its triangles in another order and its two materials exchanged: valid, and another picture"""
    p, n = deformed(mesh)
    return dict(mesh, positions=p, normals=n, indices=np.roll(mesh["indices"], 5, axis=0),
                tri_material=None if mesh.get("tri_material") is None else (1 - mesh["tri_material"]).astype(np.uint32))


def overwrite(bufs, new):
    for k, dst in bufs.items():
        if dst is not None:
            dst.copy_(new[k])


@pytest.mark.parametrize("which", ["set_scene_device", "set_mesh_device", "set_texcoords_device"])
def test_whitted_set_calls_read_what_the_stream_wrote(capi, torch, oracle, which):
    meshes, inst = whitted_small()
    others = [other_mesh(m) for m in meshes]
    rng = np.random.RandomState(8)
    texture = rng.randint(0, 256, (16, 16, 4)).astype(np.uint8)
    uv_a, uv_b = (rng.rand(len(meshes[0]["positions"]), 2).astype(np.float32) for _ in range(2))
    one = [(TWM.EYE, 0, 0)]

    def case(R, stale):
        ctx = R.ctx
        acc, img = R.bound(WW * WH)
        if which == "set_scene_device":
            whitted_ctx(capi, oracle, ctx, meshes, inst, view_of=others, set_scene=False)
            bufs, new = [mesh_tensors(R, m) for m in meshes], [mesh_tensors(R, m) for m in others]
        else:
            whitted_ctx(capi, oracle, ctx, meshes[:1], one, view_of=others[:1], set_scene=False)
            bufs, new = [mesh_tensors(R, meshes[0])], [mesh_tensors(R, others[0])]
            if which == "set_texcoords_device":
                ctx.whitted_set_mesh(meshes[0]["positions"], meshes[0]["normals"], meshes[0]["indices"], meshes[0]["tri_material"], WI.materials())
                for m in range(len(WI.materials())):
                    ctx.whitted_set_material_textures(m, texture, None, None)
                bufs, new = [{"uv": R.dev(uv_a)}], [{"uv": R.dev(uv_b)}]
        R.begin()
        with R.on():
            if not stale:
                for b, n in zip(bufs, new):
                    overwrite(b, n)
            if which == "set_scene_device":
                R.call(ctx.whitted_set_scene_device, bufs, inst, WI.materials())
            elif which == "set_mesh_device":
                b = bufs[0]
                R.call(ctx.whitted_set_mesh_device, b["positions"], b["normals"], b["indices"], b["tri_material"], WI.materials())
            else:
                R.call(ctx.whitted_set_texcoords_device, bufs[0]["uv"])
            R.call(ctx.whitted_launch, WW, WH, 0)
            return {"accum": acc.clone(), "image": img.clone()}

    SO.wrote_all(SO.regimes(torch, capi, case), ["accum"])


@pytest.mark.parametrize("rebuild", [False, True], ids=["refit", "rebuild"])
def test_whitted_update_meshes_device_reads_what_the_stream_wrote(capi, torch, oracle, rebuild):
    """the small meshes and the clustered one of tests/test_whitted_update_device.py in one call, one of them with new normals"""
    meshes, inst, updates = TWD.several()
    new = TWD.moved(meshes, updates)

    def case(R, stale):
        ctx = R.ctx
        whitted_ctx(capi, oracle, ctx, meshes, inst, view_of=new)
        acc, img = R.bound(WW * WH)
        bufs = [(k, R.dev(meshes[k]["positions"]), None if n is None else R.dev(meshes[k]["normals"])) for k, _, n in updates]
        fresh = [(k, R.dev(p), None if n is None else R.dev(n)) for k, p, n in updates]
        R.begin()
        with R.on():
            if not stale:
                for (_, p, n), (_, new_p, new_n) in zip(bufs, fresh):
                    p.copy_(new_p)
                    if n is not None:
                        n.copy_(new_n)
            R.call(ctx.whitted_update_meshes_device, bufs, rebuild)
            R.call(ctx.whitted_launch, WW, WH, 0)
            return {"accum": acc.clone(), "image": img.clone()}

    SO.wrote_all(SO.regimes(torch, capi, case), ["accum"])


def moved_instances(inst, k=1.0):
    """the same meshes under other transforms and material offsets"""
    return [(np.asarray(tr, np.float32) + np.float32(k) * np.array([[0, 0, 0, 0.3], [0, 0, 0, -0.2], [0, 0, 0, 0.25]], np.float32), m, (off + 1) % 3)
            for tr, m, off in inst]


@pytest.mark.parametrize("refit", [False, True], ids=["rebuild", "refit"])
def test_whitted_set_instances_device_reads_what_the_stream_wrote(capi, torch, oracle, refit):
    meshes, inst = whitted_small()
    new = moved_instances(inst)

    def case(R, stale):
        ctx = R.ctx
        whitted_ctx(capi, oracle, ctx, meshes, inst)
        acc, img = R.bound(WW * WH)
        rec, new_rec = R.dev(TI.records(inst)), R.dev(TI.records(new))
        R.begin()
        with R.on():
            if not stale:
                rec.copy_(new_rec)
            R.call(ctx.whitted_set_instances_device, rec, refit)
            R.call(ctx.whitted_launch, WW, WH, 0)
            return {"accum": acc.clone(), "image": img.clone()}

    SO.wrote_all(SO.regimes(torch, capi, case), ["accum"])


# ---- B. outputs ordered on the stream -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["launch", "launch_frames", "whitted_launch", "whitted_launch_frames"])
def test_launch_outputs_are_ordered_on_the_stream(capi, torch, oracle, which):
    """the stream writes the output buffers behind the stall -- the mean a progressive frame continues from, or the sentinel -- then the
    launch is made and its buffers are cloned, all with no wait: a launch that ran anywhere else would be overwritten or read too early"""
    t = analytic(oracle, "cornell")
    meshes, inst = whitted_small()
    whitted = which.startswith("whitted")
    w, h = (WW, WH) if whitted else (W, H)
    prev_mean = np.random.RandomState(9).rand(w * h, 4).astype(np.float32)

    def case(R, stale):
        ctx = R.ctx
        if whitted:
            whitted_ctx(capi, oracle, ctx, meshes, inst)
        else:
            analytic_ctx(ctx, t)
        acc, img = R.bound(w * h)
        prev = R.dev(prev_mean)
        R.begin()
        with R.on():
            img.fill_(SO.IMAGE_SENTINEL - 1)
            if not stale:
                acc.copy_(prev)
            if which == "launch":
                R.call(ctx.launch, frame(capi, 1), asynchronous=True, name="rtgo_launch")
            elif which == "launch_frames":
                R.call(ctx.launch_frames, frame(capi, 1), 4, asynchronous=True, name="rtgo_launch_frames")
            elif which == "whitted_launch":
                R.call(ctx.whitted_launch, WW, WH, 1, asynchronous=True, name="rtgo_whitted_launch")
            else:
                R.call(ctx.whitted_launch_frames, capi.make_whitted_frame(WW, WH, 1), 5, asynchronous=True, name="rtgo_whitted_launch_frames")
            return {"accum": acc.clone(), "image": img.clone()}

    SO.wrote_all(SO.regimes(torch, capi, case), ["accum"])


@pytest.mark.parametrize("named", [False, True], ids=["hip_stream NULL", "hip_stream named"])
def test_assemble_bands_on_the_stream(capi, torch, oracle, named):
    """three contexts render the three band shares of a frame on one stream, torch gathers them on it, rtgo_assemble_bands follows"""
    t = analytic(oracle, "cornell")
    band_h, ranks = 5, 3
    rows = [capi.local_rows(H, band_h, ranks, g) for g in range(ranks)]
    rows_pad = max(rows)
    assert rows == [15, 11, 10]

    def case(R, stale):
        shares = []
        for g, ctx in enumerate(R.ctxs):
            analytic_ctx(ctx, t)
            shares.append(R.bound(rows_pad * W, ctx))
        full_acc, full_img = R.outputs(W * H)
        R.begin()
        with R.on():
            for g, ctx in enumerate(R.ctxs):
                R.call(ctx.launch, frame(capi, 0, bands=(band_h, ranks, g)), asynchronous=True, ctx=ctx, name="rtgo_launch")
            stream = R.stream.cuda_stream if (named and not R.waited) else None
            for k, (full, elem) in enumerate(((full_acc, 16), (full_img, 4))):
                gathered = R.keep(torch.cat([s[k] for s in shares]))
                SO.ok(capi, R.ctx, R.call(SO.assemble_bands, capi, R.ctx, stream, gathered, full, W, H, band_h, ranks, rows_pad, elem, asynchronous=True,
                                          name="rtgo_assemble_bands"))
            return {"accum": full_acc.clone(), "image": full_img.clone()}

    res = SO.regimes(torch, capi, case, n_ctx=3, differs=False)
    SO.wrote_all(res, ["accum"])
    whole = capi.Context(0)
    try:
        analytic_ctx(whole, t).resize(W * H)
        whole.launch(frame(capi))
        whole.sync()
        assert np.array_equal(whole.read_accum(H, W).view(np.uint8).reshape(-1), res["accum"].reshape(-1)), "the assembled shares are not the whole frame"
    finally:
        whole.close()


# ---- C. the chain -------------------------------------------------------------------------------------------------------------------------
def test_the_chain(capi, torch, oracle):
    """four simulation steps on one stream: every input is a torch expression of the step number, every call follows at once.  (The
    synchronous calls sit out the stall in step 0, and the analytic job's launch-time trial waits once at its fifth launch: what the
    chain shows is the order of the steps' writes, calls and clones, not a backlog)"""
    t = analytic(oracle, "cornell")
    idx, _ = box_moved(oracle, t, "short")
    meshes, inst = whitted_small()
    far = [deformed(m, 4.0)[0] for m in meshes]

    def case(R, stale):
        a, w = R.ctxs
        analytic_ctx(a, t)
        whitted_ctx(capi, oracle, w, meshes, inst, view_of=[dict(m, positions=np.concatenate([m["positions"], f])) for m, f in zip(meshes, far)])
        acc_a, img_a = R.bound(W * H, a)
        acc_w, img_w = R.bound(WW * WH, w)
        i, rec0, box0 = R.keep(*TP.tensors(torch, capi, t, idx))
        rec, box = R.keep(rec0.clone(), box0.clone())
        pos0 = [R.dev(m["positions"]) for m in meshes]
        pos = [R.keep(p.clone()) for p in pos0]
        inst0 = R.dev(TI.records(inst)).view(torch.float32)
        irec = R.keep(inst0.clone())
        out = {}
        R.begin()
        with R.on():
            for step in range(4):
                s = 0.0 if stale else 0.1 * (step + 1)
                for p, p0 in zip(pos, pos0):
                    p.copy_(p0 * (1.0 + s) + 0.5 * s)
                R.call(w.whitted_update_meshes_device, [(k, p, None) for k, p in enumerate(pos)], False, ctx=w)
                irec.copy_(inst0)
                irec[:, [3, 7, 11]] += s
                R.call(w.whitted_set_instances_device, irec, True, ctx=w)
                R.call(w.whitted_launch_frames, capi.make_whitted_frame(WW, WH, 0), 2, ctx=w)
                out["whitted %d" % step], out["whitted image %d" % step] = acc_w.clone(), img_w.clone()
                rec.copy_(rec0)
                box.copy_(box0)
                rec[:, 8] += s      # (model[7]: the y translation)
                box[:, [1, 4]] += s
                SO.ok(capi, a, R.call(SO.raw_update_prims_device, capi, a, i, rec, box, False, ctx=a))
                for f in (0, 1):
                    R.call(a.launch, frame(capi, f), ctx=a)
                out["analytic %d" % step], out["analytic image %d" % step] = acc_a.clone(), img_a.clone()
        return out

    res = SO.regimes(torch, capi, case, n_ctx=2)
    SO.wrote_all(res, [k for k in res if k.startswith(("whitted", "analytic")) and "image" not in k])
    assert len({res["analytic %d" % k].tobytes() for k in range(4)}) == 4 and len({res["whitted %d" % k].tobytes() for k in range(4)}) == 4, "the steps look alike"


# ---- D. the unwaited drag -----------------------------------------------------------------------------------------------------------------
WINDOWS = [(16, 12), (24, 18), (32, 24), (40, 30), (44, 33), (48, 36)]
DRAG_SPP = 4   # sqrt_spp of the drag: 16 samples per pixel make strips of 4 pixels, so a 16 x 12 window has 48 of them and the frame 432
STRIPS = re.compile(r"rtgo_launch: .* (\d+) strips of (\d+) px \((\d+) x (\d+) at (\d+),(\d+)\)")


def drag_cameras(cam, towards=0.0):
    """six cameras that drift sideways and back away from the scene, or with `towards` > 0 approach it by that share of W per step"""
    cam = np.asarray(cam, np.float32)
    return [shifted(cam, (towards * k if towards else -(1.0 + 0.5 * k)) * cam[9:12] + (0.01 if towards else 0.15) * k * cam[3:6]) for k in range(6)]


@pytest.mark.parametrize("interleaved", [False, True], ids=["launches", "launches and ray calls"])
def test_the_unwaited_drag(capi, torch, oracle, capfd, interleaved):
    """six camera moves towards plateau behind one stall, each with a larger window (grown from the frame's last corner, where sky and
    scene meet) and buffers of its own, at 16 samples per pixel (strips of 4 pixels).  What the library says of each launch (RTGO_DEBUG's line: the strips of the scene's screen rectangle; rays_culled) must
    show that every step takes a per-strip mask with cold strips in it and that the mask has more 32-bit words than the step before: it is
    rebuilt and regrown per step while the launches that were given the earlier ones are still queued, and six steps pass through its
    two staging slots three times"""
    t = analytic(oracle, "plateau")
    cams = drag_cameras(t["cam"], towards=0.05)
    o, d, seed = SR.raygen32(t["cam"], 64, 64, 0)
    rays_host = SO.rays_tensor(capi, o, d, TU.TMIN, TU.TMAX)
    culled = []   # the waited run's rays_culled after each step

    def case(R, stale):
        ctx = analytic_ctx(R.ctx, t)
        bufs = [R.outputs(w * h) for w, h in WINDOWS]
        rays, seeds = R.dev(rays_host), R.dev(seed)
        hits = [R.keep(torch.full((N_RAYS, 8), SO.SENTINEL, dtype=torch.float32, device="cuda")) for _ in WINDOWS]
        shaded = [R.outputs(N_RAYS) for _ in WINDOWS]
        opt = capi.ShadeOptions(5, 1, 0, 0)
        R.begin()
        with R.on():
            for k, ((w, h), (acc, img)) in enumerate(zip(WINDOWS, bufs)):
                first = k < 2   # (later steps may wait for a staging slot's copy or for the mask to regrow)
                look(ctx, cams[k])
                ctx.bind_output(acc.data_ptr(), img.data_ptr(), w * h)
                R.call(ctx.launch, capi.make_frame(W, H, DRAG_SPP, 0, True, False, window=(W - w, H - h, w, h)), asynchronous=first,
                       name="rtgo_launch")
                if R.waited:
                    culled.append(ctx.stats()["rays_culled"])
                if interleaved:
                    SO.ok(capi, ctx, R.call(ctx.trace_rays_raw, rays.data_ptr(), hits[k].data_ptr(), N_RAYS, 0, False, asynchronous=first, name="rtgo_trace_rays"))
                    SO.ok(capi, ctx, R.call(ctx.shade_rays_raw, rays.data_ptr(), seeds.data_ptr(), shaded[k][0].data_ptr(), shaded[k][1].data_ptr(), N_RAYS,
                                            opt, asynchronous=first, name="rtgo_shade_rays"))
            out = {}
            for k in range(6):
                out["accum %d" % k], out["image %d" % k] = bufs[k][0].clone(), bufs[k][1].clone()
                if interleaved:
                    out["hits %d" % k], out["shaded %d" % k] = hits[k].clone(), shaded[k][0].clone()
            return out

    capfd.readouterr()
    with Knob(RTGO_DEBUG=1):
        res = SO.regimes(torch, capi, case, differs=False)
    said = [tuple(int(x) for x in m.groups()) for m in map(STRIPS.search, capfd.readouterr().err.splitlines()) if m]
    SO.wrote_all(res, ["accum %d" % k for k in range(6)])
    assert res["counters 0"][2] > 0, "no ray was culled"
    assert len({res["accum %d" % k][:16 * 12 * 16].tobytes() for k in range(6)}) == 6, "the six cameras show the same picture"
    # the premise, from what the library reported: both regimes planned the same strips; step by step the waited run's mask had cold
    # strips (so it was staged and uploaded) and more words than the one before (so its buffer was grown)
    assert len(said) == 12 and said[:6] == said[6:], said
    words, before = [], 0
    for k, ((w, h), (n_hot, strip_px, hot_w, hot_h, hot_x0, _)) in enumerate(zip(WINDOWS, said)):
        assert strip_px == 4 and n_hot == hot_w * hot_h, said[k]
        outside = w * h - hot_h * (min((hot_x0 + hot_w) * strip_px, w) - hot_x0 * strip_px)   # pixels beside the scene's rectangle
        masked = (culled[k] - before) // DRAG_SPP ** 2 - outside
        before = culled[k]
        assert masked > 0, "step %d: no strip of the mask was cold, the launch took no mask: %r" % (k, said[k])
        words.append((n_hot + 31) // 32)
    assert all(a < b for a, b in zip(words, words[1:])), "the mask did not grow at every step: %r words" % words


def test_the_unwaited_whitted_drag(capi, torch, oracle):
    """the whitted twin: camera moves and launches alternate with rtgo_whitted_shade_rays, so the two sets of tile-queue heads change
    hands six times behind one stall"""
    meshes, inst = whitted_small()

    def case(R, stale):
        ctx = R.ctx
        cam = whitted_ctx(capi, oracle, ctx, meshes, inst)
        cams = drag_cameras(cam)
        bufs = [R.outputs(WW * WH) for _ in cams]
        rays = R.dev(trace_inputs(capi, cam, True))
        shaded = [R.outputs(N_RAYS) for _ in cams]
        R.begin()
        with R.on():
            for k, (acc, img) in enumerate(bufs):
                look(ctx, cams[k])
                ctx.bind_output(acc.data_ptr(), img.data_ptr(), WW * WH)
                R.call(ctx.whitted_launch, WW, WH, 0, asynchronous=k < 2, name="rtgo_whitted_launch")
                SO.ok(capi, ctx, R.call(ctx.whitted_shade_rays_raw, rays.data_ptr(), shaded[k][0].data_ptr(), shaded[k][1].data_ptr(), N_RAYS, 0,
                                        asynchronous=k < 2, name="rtgo_whitted_shade_rays"))
            out = {}
            for k in range(6):
                out["accum %d" % k], out["image %d" % k], out["shaded %d" % k] = bufs[k][0].clone(), bufs[k][1].clone(), shaded[k][0].clone()
            return out

    res = SO.regimes(torch, capi, case, differs=False)
    SO.wrote_all(res, ["accum %d" % k for k in range(6)] + ["shaded %d" % k for k in range(6)])
    assert len({res["accum %d" % k].tobytes() for k in range(6)}) == 6, "the six cameras show the same picture"


# ---- E. a backlog deeper than the event ring ----------------------------------------------------------------------------------------------
def test_a_backlog_deeper_than_the_event_ring(capi, torch, oracle):
    """70 progressive frames queued behind the stall.  The job has one candidate (RTGO_TREE pins the structure), so no launch-time trial
    waits at the fifth launch and drains the stall: the first 64 launches return at once, the stall still pending after the 64th, and the
    65th finds the ring of 64 event pairs full with its oldest pair not yet completed"""
    w, h, n = 32, 24, 70
    t = analytic(oracle, "cornell", w, h)

    def case(R, stale):
        ctx = analytic_ctx(R.ctx, t)
        acc, img = R.bound(w * h)
        R.begin()
        with R.on():
            for f in range(n):
                R.call(ctx.launch, frame(capi, f, w, h), asynchronous=f < 64, name="rtgo_launch")
            return {"accum": acc.clone(), "image": img.clone(), "trial launches": ctx.stats()["launches_trial"]}

    with Knob(RTGO_TREE=0):
        res = SO.regimes(torch, capi, case, differs=False)
    SO.wrote_all(res, ["accum"])
    assert res["counters 0"][3] == n and res["trial launches"] == 0


# ---- F. rtgo_set_stream itself ------------------------------------------------------------------------------------------------------------
def test_set_stream_waits_and_moves_the_work(capi, torch, oracle):
    """rtgo_set_stream first finishes the work on the previous stream; frames 0, 1 on one stream and 2, 3 on the next are frames 0 .. 3"""
    t = analytic(oracle, "cornell")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    moved, own = capi.Context(0), capi.Context(0)
    try:
        for ctx in (moved, own):
            analytic_ctx(ctx, t)
        R, R_own = SO.Run(torch, [moved], s1), SO.Run(torch, [own])
        out, want = R.bound(W * H), R_own.bound(W * H)
        R.begin()
        with R.on():
            for f in (0, 1):
                R.call(moved.launch, frame(capi, f), asynchronous=True, name="rtgo_launch")
        moved.set_stream(s2.cuda_stream)
        assert R.ev.query(), "rtgo_set_stream returned while the work on the previous stream was pending"
        with torch.cuda.stream(s2):
            for f in (2, 3):
                moved.launch(frame(capi, f))
            got = [x.clone() for x in out]
        torch.cuda.synchronize()
        moved.sync()
        for f in range(4):
            own.launch(frame(capi, f))
            own.sync()
        assert all(np.array_equal(SO.host(torch, {"x": g})["x"], SO.host(torch, {"x": x})["x"]) for g, x in zip(got, want)), "frames 0 .. 3 over two streams differ"
        sa, sb = moved.stats(), own.stats()
        assert [sa[f] for f in SO.COUNTERS] == [sb[f] for f in SO.COUNTERS]
    finally:
        torch.cuda.synchronize()
        moved.close()
        own.close()


def test_null_is_the_contexts_own_stream(capi, torch, oracle):
    """after rtgo_set_stream(NULL) a launch and rtgo_sync complete while the stream the context left is still stalled.  Streams share the
    device's hardware queues (four to a process unless GPU_MAX_HW_QUEUES says otherwise), and two streams on one queue wait for each
    other whatever they were told.  So the context leaves four streams in turn: where the runtime hands its queues out in turn, four
    streams taken one after the other lie on four queues and exactly one shares the own stream's, so three launches do not wait; the
    test asks for two, which leaves room for one more coincidence under another hand-out and is still far from the none of four that a
    launch left behind on the old stream gives"""
    t = analytic(oracle, "cornell")
    ctx = capi.Context(0)
    try:
        analytic_ctx(ctx, t).resize(W * H)
        pending = []
        for f in range(4):
            left = torch.cuda.Stream()
            ctx.set_stream(left.cuda_stream)
            ctx.launch(frame(capi, 2 * f))
            ctx.set_stream(None)
            torch.cuda.synchronize()
            ev = SO.stall(torch, left, SO.STALL_MS)
            ctx.launch(frame(capi, 2 * f + 1))
            ctx.sync()
            pending.append(not ev.query())
            ev.synchronize()
        assert sum(pending) >= 2, "launches after rtgo_set_stream(NULL) waited for the streams the context had left: %r" % pending
    finally:
        torch.cuda.synchronize()
        ctx.close()


# ---- G. two contexts on two streams -------------------------------------------------------------------------------------------------------
def test_two_contexts_on_two_streams(capi, torch, oracle):
    """cornell in path mode and the whitted scene, each on a stream of its own behind a stall of its own, four progressive frames each,
    enqueued in turn: every frame is what the context renders alone"""
    t = analytic(oracle, "cornell")
    meshes, inst = whitted_small()

    def case(runs, stale):
        Ra, Rw = runs
        analytic_ctx(Ra.ctx, t)
        whitted_ctx(capi, oracle, Rw.ctx, meshes, inst)
        acc_a, img_a = Ra.bound(W * H)
        acc_w, img_w = Rw.bound(WW * WH)
        out = {}
        Ra.begin()
        Rw.begin(synchronize=False)   # (a wait here would sit out the first stall)
        for f in range(4):
            with Ra.on():
                Ra.call(Ra.ctx.launch, frame(capi, f), asynchronous=f < 2, name="rtgo_launch")
                out["analytic %d" % f], out["analytic image %d" % f] = acc_a.clone(), img_a.clone()
            with Rw.on():
                Rw.call(Rw.ctx.whitted_launch_frame, capi.make_whitted_frame(WW, WH, f), asynchronous=f < 2, name="rtgo_whitted_launch_frame")
                out["whitted %d" % f], out["whitted image %d" % f] = acc_w.clone(), img_w.clone()
        return out

    res = SO.regimes(torch, capi, case, n_ctx=2, differs=False, separate=True)
    SO.wrote_all(res, [k for k in res if k.startswith(("whitted", "analytic")) and "image" not in k])
