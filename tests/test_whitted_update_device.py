"""rtgo_whitted_update_meshes_device on the MI355X: refits and rebuilds from vertex buffers that are on the device already.

One claim: after the call the context holds, array for array, what its host-pointer twin holds after the same vertices --
rtgo_whitted_update_meshes for RTGO_UPDATE_REFIT, rtgo_whitted_rebuild_meshes for RTGO_UPDATE_REBUILD.  So every comparison here is an
equality: the build digests span for span, the frames bit for bit with the top level in LDS and through L2.  A refused call leaves
digests, frames and the caller's tensors as they were.

Meshes, deformations and helpers are those of tests/test_whitted_update_meshes.py and tests/test_whitted_rebuild_meshes.py.  The shapes
are the smallest at which each kernel can go wrong: an octahedron (8 triangles), torus(16, 8) (256 triangles), the 8320-triangle mesh
(three clusters under a mid level of one leaf; 4160 vertices: thirteen workgroups of the check, so partial boxes, partial flags and
tails all occur); 64 x 48 frames."""
import numpy as np
import pytest

import accel_check as A
import whitted_instances as WI
import whitted_scene
from test_trace_rays import Knob
from test_whitted_rebuild_meshes import beside, moved, same_digests
from test_whitted_update_meshes import (E_INVALID, E_STATE, EYE, MODES, big, frames, layout, no_violations, permuted, same_frames, scene_ctx, sine,
                                        world_view)

pytestmark = pytest.mark.gpu
FLAGS = [False, True]   # rebuild: RTGO_UPDATE_REFIT against whitted_update_meshes, RTGO_UPDATE_REBUILD against whitted_rebuild_meshes


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


def on_device(torch, updates):
    """[(mesh, positions, normals or None)] with the arrays as device tensors, their uploads complete"""
    def dev(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    out = [(k, dev(p), dev(n)) for k, p, n in updates]
    torch.cuda.synchronize()
    return out


def device_call(torch, ctx, updates, rebuild):
    ctx.whitted_update_meshes_device(on_device(torch, updates), rebuild=rebuild)


def host_call(ctx, updates, rebuild):
    (ctx.whitted_rebuild_meshes if rebuild else ctx.whitted_update_meshes)(updates)


def same_scene(a, b, what):
    same_digests(a, b, what)
    for mode in MODES:
        with Knob(RTGO_WHITTED_MODE=mode):
            fa, fb = frames(a), frames(b)
        same_frames(fa, fb, "%s, RTGO_WHITTED_MODE=%d" % (what, mode))


def bits(t):
    return t.cpu().numpy().view(np.uint32).copy()


def new_normals(mesh):
    n = mesh["normals"].astype(np.float64) + 0.3 * np.sin(5.0 * mesh["positions"].astype(np.float64)[:, [1, 2, 0]])
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


# ---- cases 1 and 2: device = host -----------------------------------------------------------------------------------------------
def several():
    """a ground (not named), a torus, the clustered mesh and two octahedra, named in shuffled order: three small meshes for the one
    refit launch, one of them with new normals"""
    rng = np.random.RandomState(21)
    torus = WI.torus(16, 8)
    meshes = [WI.ground(3.0, -0.4), torus, big(8320), WI.octahedron(0.3), WI.octahedron(0.2)]
    inst = [(EYE, 0, 0), (WI.transform(WI.rotation(rng), [-1.2, 0.3, 0.2]), 1, 1), (WI.transform(np.eye(3), [0.2, 0.1, -0.2]), 2, 2),
            (WI.transform(WI.rotation(rng) @ np.diag([1.0, 0.6, 1.3]), [1.2, 0.3, 0.5]), 3, 0), (WI.transform(0.7 * WI.rotation(rng), [-0.3, 0.9, 0.8]), 4, 3)]
    p = torus["positions"].astype(np.float64)
    updates = [(3, meshes[3]["positions"] * np.float32(1.5), None),
               (2, sine(meshes[2], shift=np.float64([0.1, 0.05, -0.1])), None),
               (4, meshes[4]["positions"][:, [2, 0, 1]] * np.float32(1.3), None),
               (1, (p + 0.08 * np.sin(9.0 * p[:, [2, 0, 1]]) * torus["normals"] + [0.1, 0.1, -0.1]).astype(np.float32), new_normals(torus))]
    return meshes, inst, updates


def case(name):
    mesh = big(8320)
    if name == "several":
        return several()
    new = permuted(mesh) if name == "clustered, permuted" else sine(mesh)
    return [mesh, WI.octahedron(0.3)], beside(new), [(0, new, new_normals(mesh) if name == "clustered, new normals" else None)]


@pytest.mark.parametrize("rebuild", FLAGS)
@pytest.mark.parametrize("name", ["clustered, sine", "clustered, permuted", "clustered, new normals", "several"])
def test_the_device_call_leaves_what_the_host_call_leaves(capi, oracle, torch, name, rebuild):
    meshes, inst, updates = case(name)
    new = moved(meshes, updates)
    cam, extra = world_view(oracle, new, inst)
    host, dev = (scene_ctx(capi, meshes, inst, WI.materials(), cam, extra) for _ in range(2))
    fresh = None
    try:
        before = list(dev.build_digest(True))
        host_call(host, updates, rebuild)
        device_call(torch, dev, updates, rebuild)
        assert list(dev.build_digest(True)) != before
        what = "%s, rebuild=%r" % (name, rebuild)
        same_scene(host, dev, what)
        no_violations(A.check_instanced(dev.read_build(True), new, inst), what)
        if rebuild:
            fresh = scene_ctx(capi, new, inst, WI.materials(), cam, extra)
            same_digests(dev, fresh, what + ", against a fresh scene")
    finally:
        for c in (host, dev, fresh):
            if c is not None:
                c.close()


def test_a_device_refit_keeps_the_old_tree_and_a_device_rebuild_replaces_it(capi, oracle, torch):
    meshes, inst, updates = case("clustered, permuted")
    new = moved(meshes, updates)
    cam, extra = world_view(oracle, new, inst)
    ctx = scene_ctx(capi, meshes, inst, WI.materials(), cam, extra)
    fresh = scene_ctx(capi, new, inst, WI.materials(), cam, extra)
    try:
        device_call(torch, ctx, updates, False)
        assert list(ctx.build_digest(True)) != list(fresh.build_digest(True)), "a refit over permuted vertices came out as the fresh build: the comparison shows nothing"
        same_frames(frames(ctx), frames(fresh), "refitted")
        device_call(torch, ctx, updates, True)
        same_digests(ctx, fresh, "rebuilt after the refit")
        same_frames(frames(ctx), frames(fresh), "rebuilt after the refit")
    finally:
        ctx.close()
        fresh.close()


@pytest.mark.parametrize("rebuild", FLAGS)
def test_a_set_mesh_scene_takes_mesh_zero(capi, torch, rebuild):
    mesh = whitted_scene.build()
    p = mesh["positions"].astype(np.float64)
    new = (p + 0.15 * np.sin(3.0 * p[:, [1, 2, 0]])).astype(np.float32)
    host, dev = capi.Context(0), capi.Context(0)
    try:
        for ctx in (host, dev):
            ctx.whitted_set_mesh(mesh["positions"], mesh["normals"], mesh["indices"], mesh["tri_material"], mesh["materials"])
        before = list(dev.build_digest(True))
        for normals in (None, -mesh["normals"]):
            host_call(host, [(0, new, normals)], rebuild)
            device_call(torch, dev, [(0, new, normals)], rebuild)
            assert list(dev.build_digest(True)) == list(host.build_digest(True)) != before
        for bad in ([(1, new, None)], [(0, new, None), (0, new, None)], [(0, new[:-1], None)]):
            with pytest.raises(capi.RtgoError, match=E_INVALID):
                device_call(torch, dev, bad, rebuild)
            assert list(dev.build_digest(True)) == list(host.build_digest(True))
    finally:
        host.close()
        dev.close()


# ---- case 3: a tensor that never was on the host --------------------------------------------------------------------------------
@pytest.mark.parametrize("rebuild", FLAGS)
def test_vertices_computed_on_the_device(capi, oracle, torch, rebuild):
    meshes, inst = [big(8320), WI.torus(16, 8)], beside()
    shift = torch.tensor([0.1, -0.05, 0.2], dtype=torch.float32, device="cuda")
    made = [(k, torch.from_numpy(meshes[k]["positions"]).cuda() * 1.1 + shift, None) for k in (1, 0)]
    torch.cuda.synchronize()
    assert all(t.is_contiguous() and t.dtype == torch.float32 for _, t, _ in made)
    updates = [(k, t.cpu().numpy(), None) for k, t, _ in made]
    cam, extra = world_view(oracle, moved(meshes, updates), inst)
    host, dev = (scene_ctx(capi, meshes, inst, WI.materials(), cam, extra) for _ in range(2))
    try:
        host_call(host, updates, rebuild)
        torch.cuda.synchronize()
        dev.whitted_update_meshes_device(made, rebuild=rebuild)
        same_scene(host, dev, "computed on the device, rebuild=%r" % rebuild)
    finally:
        host.close()
        dev.close()


# ---- case 4: non-finite data ----------------------------------------------------------------------------------------------------
def refusal_scene(capi, oracle):
    """the clustered mesh, a torus, and an octahedron with a seventh vertex that no triangle names"""
    bigm, small = big(8320), WI.torus(16, 8)
    bare = WI.octahedron(0.3)
    bare = dict(bare, positions=np.concatenate([bare["positions"], np.float32([[0.1, 0.2, 0.1]])]))
    meshes = [bigm, small, bare]
    inst = [(EYE, 0, 0), (WI.transform(np.eye(3), [0.5, 0.5, 0.0]), 1, 0), (WI.transform(np.eye(3), [-0.5, 0.5, 0.0]), 2, 0)]
    cam, extra = world_view(oracle, meshes, inst)
    ok = [(0, sine(bigm), None), (1, small["positions"] * np.float32(1.1), small["normals"]), (2, bare["positions"] * np.float32(2.0), None)]
    return meshes, scene_ctx(capi, meshes, inst, WI.materials(), cam, extra), ok


@pytest.mark.parametrize("rebuild", FLAGS)
def test_non_finite_data_is_refused_wherever_it_hides(capi, oracle, torch, rebuild):
    (bigm, small, bare), ctx, ok = refusal_scene(capi, oracle)

    def poisoned(a, vertex, axis, value=np.nan):
        a = np.array(a, np.float32)
        a[vertex, axis] = value
        return a

    assert 3 * 2500 + 1 > 1024 and len(bigm["positions"]) > 2500
    assert 6 not in bare["indices"]
    refused = {
        "a NaN in the last float of the last entry of three": [ok[0], ok[2], (1, poisoned(ok[1][1], -1, 2), None)],
        "a NaN in a vertex that no triangle names": [(2, poisoned(ok[2][1], 6, 0), None)],
        "an infinity in the clustered mesh beyond the first workgroup's floats": [(0, poisoned(ok[0][1], 2500, 1, -np.inf), None)],
        "a NaN among the normals, the positions finite": [(0, ok[0][1], poisoned(bigm["normals"], 4000, 2)), ok[1]],
        "a NaN in entry 0, valid entries after it": [(2, poisoned(ok[2][1], 0, 0), None), ok[0], ok[1]],
    }
    try:
        before, shown = list(ctx.build_digest(True)), frames(ctx)
        for what, updates in refused.items():
            tensors = on_device(torch, updates)
            kept = [(bits(p), None if n is None else bits(n)) for _, p, n in tensors]
            with pytest.raises(capi.RtgoError, match=E_INVALID):
                ctx.whitted_update_meshes_device(tensors, rebuild=rebuild)
            assert list(ctx.build_digest(True)) == before, what
            same_frames(frames(ctx), shown, what)
            for (_, p, n), (kp, kn) in zip(tensors, kept):
                assert np.array_equal(bits(p), kp) and (n is None or np.array_equal(bits(n), kn)), what + ": the caller's tensors changed"
        device_call(torch, ctx, ok, rebuild)
        assert list(ctx.build_digest(True)) != before
    finally:
        ctx.close()


# ---- case 5: the other refusals -------------------------------------------------------------------------------------------------
def test_the_other_refusals(capi, oracle, torch):
    (bigm, small, bare), ctx, ok = refusal_scene(capi, oracle)
    none = capi.Context(0)
    try:
        for rebuild in FLAGS:
            with pytest.raises(capi.RtgoError, match=E_STATE):
                device_call(torch, none, [ok[0]], rebuild)
        before = list(ctx.build_digest(True))
        refused = {
            "a mesh named twice": [ok[0], ok[1], (0, bigm["positions"], None)],
            "a mesh index beyond the scene's": ok[:2] + [(3, bare["positions"], None)],
            "a vertex count not the mesh's own": [ok[0], (1, small["positions"][:-1], None)],
            "normals for a mesh set without": [ok[0], (2, bare["positions"], np.ones_like(bare["positions"]))],
        }
        for what, updates in refused.items():
            for rebuild in FLAGS:
                with pytest.raises(capi.RtgoError, match=E_INVALID):
                    device_call(torch, ctx, updates, rebuild)
                assert list(ctx.build_digest(True)) == before, what
        # decided on the host, before any launch: NULL updates with a count, NULL positions, a pointer off by two bytes, unknown flags
        fn = ctx._lib.rtgo_whitted_update_meshes_device
        (_, p, n), = on_device(torch, [ok[1]])
        entry = lambda pos, nrm: (capi.WhittedMeshUpdate * 1)(capi.WhittedMeshUpdate(1, pos, nrm, len(small["positions"])))
        for flags in (capi.UPDATE_REFIT, capi.UPDATE_REBUILD):
            assert fn(ctx._h, None, 2, flags) == 1
            assert fn(ctx._h, entry(None, None), 1, flags) == 1
            assert fn(ctx._h, entry(p.data_ptr() + 2, None), 1, flags) == 1
            assert fn(ctx._h, entry(p.data_ptr(), n.data_ptr() + 2), 1, flags) == 1
            assert fn(ctx._h, None, 0, flags) == 0
            assert fn(ctx._h, entry(p.data_ptr(), n.data_ptr()), 0, flags) == 0
        assert fn(ctx._h, entry(p.data_ptr(), n.data_ptr()), 1, 2) == 1
        assert fn(ctx._h, None, 0, 2) == 1
        ctx.whitted_update_meshes_device([])
        ctx.whitted_update_meshes_device([], rebuild=True)
        assert list(ctx.build_digest(True)) == before
        # the binding's own: a tensor that is not contiguous, not float32, not on the device
        wide = torch.zeros((len(small["positions"]), 4), dtype=torch.float32, device="cuda")
        for bad in (wide[:, :3], p.double(), p.cpu(), p.reshape(-1)):
            with pytest.raises(ValueError):
                ctx.whitted_update_meshes_device([(1, bad, None)])
            with pytest.raises(ValueError):
                ctx.whitted_update_meshes_device([(1, p, bad)])
        assert list(ctx.build_digest(True)) == before
        # a valid call still works
        assert fn(ctx._h, entry(p.data_ptr(), n.data_ptr()), 1, capi.UPDATE_REFIT) == 0
        assert list(ctx.build_digest(True)) != before
    finally:
        ctx.close()
        none.close()


# ---- case 6: a refusal after the work -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rebuild", FLAGS)
def test_a_refusal_after_the_work_puts_the_meshes_back(capi, oracle, torch, rebuild):
    """the 1e30-scaled instance of test_a_refusal_after_the_build_puts_the_meshes_back: the clustered mesh's box is known only after its
    refit or build, and positions x 1e10 then place that instance beyond the float range"""
    bigm, small = big(8320), WI.octahedron(0.3)
    inst = [(EYE, 0, 0), (EYE, 1, 0), (WI.transform(np.diag([1e30, 1.0, 1.0]), [0, 1, 0]), 0, 0)]
    cam, extra = world_view(oracle, [bigm, small], inst[:2])
    ctx = scene_ctx(capi, [bigm, small], inst, WI.materials(), cam, extra)
    try:
        before, shown = list(ctx.build_digest(True)), frames(ctx)
        assert (shown[0][..., :3] != np.float32(extra["miss"])).any(axis=-1).mean() > 0.05
        far = bigm["positions"] * np.float32(1e10)
        for updates in ([(0, far, None)], [(1, small["positions"] * np.float32(2.0), None), (0, far, -bigm["normals"])]):
            with pytest.raises(capi.RtgoError, match=E_INVALID):
                device_call(torch, ctx, updates, rebuild)
            assert list(ctx.build_digest(True)) == before
            same_frames(frames(ctx), shown, "after a refusal")
        doubled = [dict(bigm, positions=bigm["positions"] * np.float32(2.0)), dict(small, positions=small["positions"] * np.float32(2.0))]
        device_call(torch, ctx, [(1, doubled[1]["positions"], None), (0, doubled[0]["positions"], None)], rebuild)
        assert list(ctx.build_digest(True)) != before
        no_violations(A.check_instanced(ctx.read_build(True), doubled, inst), "after the refusals")
    finally:
        ctx.close()


# ---- case 7: afterwards ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rebuild", FLAGS)
def test_the_other_calls_work_afterwards(capi, oracle, torch, rebuild):
    mesh, small = big(8320), WI.torus(16, 8)
    first, second = sine(mesh), permuted(mesh)
    meshes, inst = [mesh, small], layout("two", first) + [(WI.transform(0.6 * np.eye(3), [-0.9, 0.4, 0.6]), 1, 2)]
    cam, extra = world_view(oracle, moved(meshes, [(0, first, None)]), inst)
    dev, host = (scene_ctx(capi, meshes, inst, WI.materials(), cam, extra) for _ in range(2))
    try:
        start = [(0, first, None), (1, small["positions"] * np.float32(0.9), None)]
        device_call(torch, dev, start, rebuild)
        host_call(host, start, rebuild)
        same_scene(dev, host, "the device call")
        rng = np.random.RandomState(4)
        again = [(WI.transform(WI.rotation(rng) @ np.diag([1.0, 0.7 + 0.2 * k, 1.0]), np.asarray(tr)[:, 3] + [0.1 * k, 0.0, 0.1]), m, off) for k, (tr, m, off) in enumerate(inst)]
        centre = np.float32(first.mean(axis=0))
        last = [(1, small["positions"] * np.float32(1.1), -small["normals"]), (0, first * np.float32(1.05), None)]
        steps = [("set_instances", lambda c: c.whitted_set_instances(again)),
                 ("update_mesh on the small mesh", lambda c: c.whitted_update_mesh(1, small["positions"] * np.float32(1.2))),
                 ("update_meshes", lambda c: c.whitted_update_meshes([(0, mesh["positions"] + centre, None), (1, small["positions"], None)])),
                 ("rebuild_meshes", lambda c: c.whitted_rebuild_meshes([(0, second + centre, None), (1, small["positions"], None)])),
                 ("a second device call", lambda c: device_call(torch, c, last, rebuild) if c is dev else host_call(c, last, rebuild)),
                 ("a device call with the other flag", lambda c: device_call(torch, c, start, not rebuild) if c is dev else host_call(c, start, not rebuild))]
        for what, step in steps:
            step(dev)
            step(host)
            same_digests(dev, host, what)
        same_scene(dev, host, "after every step")
        no_violations(A.check_instanced(dev.read_build(True), moved(meshes, start), again), "after every step")
    finally:
        dev.close()
        host.close()
