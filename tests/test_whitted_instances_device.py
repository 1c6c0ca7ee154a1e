"""rtgo_whitted_set_instances_device on the MI355X: the instances of an instanced scene set (RTGO_UPDATE_REBUILD) or refitted
(RTGO_UPDATE_REFIT) from a buffer that is on the device already.

REBUILD is the twin of rtgo_whitted_set_instances: afterwards the context holds, array for array, what that call holds after the same
instances, so the build digests are compared span for span and the frames bit for bit with the top level in LDS and through L2.  REFIT
keeps the top level's topology, so its arrays differ from a rebuilt top level's, but any tree over the same instances returns the same
closest hit (lowest (instance, triangle) on ties): frames, closest hits and shaded rays are compared bit for bit with a context that
took the same instances through rtgo_whitted_set_instances.  A refused call has the twin's code and message on the same data and leaves
digests, frames and the caller's tensor as they were.  Every comparison is an equality.

Shapes are the smallest at which each path can go wrong: 1 and 4 instances (a top level of one leaf, no records), 5 (the first records),
257 (two workgroups of inst_prepare_kernel, the second with one entry), 8192 (the cap); 64 x 48 frames."""
import numpy as np
import pytest

import accel_check as A
import trace_rays_ref as R
import whitted_instances as WI
from test_trace_rays import Knob
from test_whitted_rebuild_meshes import same_digests
from test_whitted_update_meshes import (E_INVALID, E_STATE, E_UNSUPPORTED, EYE, H, MODES, TMAX, TMIN, W, big, frames, no_violations, same_frames, same_rays,
                                        scene_ctx, world_view)

pytestmark = pytest.mark.gpu
NAME = "rtgo_whitted_set_instances_device"
REFITS = [False, True]   # RTGO_UPDATE_REBUILD, RTGO_UPDATE_REFIT


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


# ---- instances ------------------------------------------------------------------------------------------------------------------
def records(inst):
    """[(transform, mesh, material offset)] as rtgo_whitted_instance records: uint32 [n, 14]"""
    out = np.zeros((len(inst), 14), np.uint32)
    for i, (tr, mesh, off) in enumerate(inst):
        out[i, :12] = np.asarray(tr, np.float32).reshape(-1)[:12].view(np.uint32)
        out[i, 12], out[i, 13] = mesh, off
    return out


def on_device(torch, inst, dtype="uint8"):
    """... as a device tensor, its upload complete: uint8 [n, 56], int32 [n, 14] or float32 [n, 14]"""
    rec = np.ascontiguousarray(inst if isinstance(inst, np.ndarray) else records(inst))
    view = {"uint8": rec.view(np.uint8).reshape(-1, 56), "int32": rec.view(np.int32), "float32": rec.view(np.float32)}[dtype]
    t = torch.from_numpy(view.copy()).cuda()
    torch.cuda.synchronize()
    return t


def bits(t):
    return t.cpu().numpy().view(np.uint8).copy()


def mixed(n, n_meshes, seed, spacing=0.45):
    """n instances on a grid over mesh 0 (a ground, identity): rigid, non-uniformly scaled, mirrored (det < 0) and uniformly scaled ones
    in turn, over meshes 1 .. n_meshes - 1 and material offsets 0 .. 2"""
    rng = np.random.RandomState(seed)
    side = max(int(np.ceil(np.sqrt(n))), 1)
    inst = [(EYE, 0, 0)]
    for k in range(1, n):
        rot = WI.rotation(rng)
        lin = [rot, rot @ np.diag([1.4, 0.6, 1.0]), WI.mirror(rng), 0.7 * rot][k % 4]
        t = [spacing * (k % side - 0.5 * side), 0.3 + 0.25 * rng.rand(), spacing * (k // side - 0.5 * side)]
        inst.append((WI.transform(0.4 * lin, t), 1 + k % (n_meshes - 1), k % 3))
    return inst[:n]


def edge_transforms(inst):
    """... with, among them: a translation of 1e6, and box bounds that round to float32 denormals (scales (2e-38, 1e4, 1e4) over a mesh of
    extent below 1: x bounds of a few 1e-39, rounded outwards among the denormals; |det| = 2e-30 passes and the inverse's 5e37 is finite;
    the sheet this makes of the mesh lies far off the view).  The last entry, alone in inst_prepare_kernel's second workgroup at 257, is
    the denormal one."""
    inst = list(inst)
    inst[3] = (WI.transform(np.eye(3), [1e6, 2.0, -1e6]), inst[3][1], 1)
    inst[-1] = (WI.transform(np.diag([2e-38, 1e4, 1e4]), [0.0, 1e5, -1e5]), inst[-1][1], 2)
    return inst


def small_meshes():
    tor = WI.torus(16, 8)
    return [WI.ground(4.0, 0.0), tor, WI.octahedron(0.3)]


def case(name):
    """(meshes, the instances the scene is set with, the new instances, how many of the new instances place the camera)"""
    if name in ("1", "4", "5"):
        n = int(name)
        meshes = small_meshes()
        return meshes, mixed(7, 3, 1), mixed(n, 3, 2), n
    if name == "257":
        meshes = small_meshes()
        return meshes, mixed(9, 3, 4), edge_transforms(mixed(257, 3, 3)), 3
    if name == "8192":
        meshes, inst = WI.octahedra_scene(8191)
        return meshes, inst[:300], inst, 8192
    if name == "normals and texcoords beside none":
        tor = WI.torus(16, 8)
        tor = dict(tor, texcoords=np.random.RandomState(5).rand(len(tor["positions"]), 2).astype(np.float32))
        meshes = [WI.ground(4.0, 0.0), tor, WI.octahedron(0.3)]
        return meshes, mixed(6, 3, 6), mixed(23, 3, 7), 23
    if name == "a clustered mesh among the meshes":
        meshes = [WI.ground(4.0, -0.5), big(8320), WI.octahedron(0.3)]
        return meshes, mixed(4, 3, 8, spacing=1.5), mixed(9, 3, 9, spacing=1.5), 9
    raise KeyError(name)


def same_scene(a, b, what):
    same_digests(a, b, what)
    for mode in MODES:
        with Knob(RTGO_WHITTED_MODE=mode):
            fa, fb = frames(a), frames(b)
        same_frames(fa, fb, "%s, RTGO_WHITTED_MODE=%d" % (what, mode))


def same_results(capi, a, b, cam, what):
    """frames in both modes, closest hits, any-hit masks and shaded rays of two contexts whose top levels may differ"""
    for mode in MODES:
        with Knob(RTGO_WHITTED_MODE=mode):
            fa, fb = frames(a), frames(b)
        same_frames(fa, fb, "%s, RTGO_WHITTED_MODE=%d" % (what, mode))
    same_rays(capi, a, b, cam, what)
    o, d = R.primaries(cam, W, H)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    (acc_a, img_a), (acc_b, img_b) = a.whitted_shade_rays(rays), b.whitted_shade_rays(rays)
    assert np.array_equal(acc_a.view(np.uint32), acc_b.view(np.uint32)) and np.array_equal(img_a, img_b), what + ": shaded rays differ"


def sorted_walk(ctx):
    """the top.inst rows by their instance column"""
    rows = np.asarray(ctx.read_build(True)["top.inst"], np.uint32).reshape(-1, 16)
    return rows[np.argsort(rows[:, 15].view(np.int32), kind="stable")]


def depth_fields(ctx):
    """of top.meta: the build's depth, n_recs and walk_depth, then n_recs, n_instances, the scene's walk_depth and mesh_depth"""
    m = np.ascontiguousarray(ctx.read_build(True)["top.meta"]).view(np.int32)
    return m[[0, 1, 2, 9, 10, 11, 12]].tolist()


def span(ctx, name):
    names = list(ctx.read_build(True))
    return ctx.build_digest(True)[names.index(name)]


# ---- 1. REBUILD equals the host call --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1", "4", "5", "257", "8192", "normals and texcoords beside none", "a clustered mesh among the meshes"])
def test_a_device_rebuild_leaves_what_the_host_call_leaves(capi, oracle, torch, name):
    meshes, first, new, seen = case(name)
    cam, extra = world_view(oracle, meshes, new[:seen])
    host, dev = (scene_ctx(capi, meshes, first, WI.materials(), cam, extra) for _ in range(2))
    fresh = None
    try:
        before = list(dev.build_digest(True))
        t = on_device(torch, new, ["uint8", "int32", "float32"][len(new) % 3])
        kept = bits(t)
        host.whitted_set_instances(new)
        dev.whitted_set_instances_device(t)
        assert list(dev.build_digest(True)) != before
        assert np.array_equal(bits(t), kept), "the caller's tensor changed"
        n_recs = depth_fields(dev)[3]
        assert (n_recs == 0) == (len(new) <= 4), "a top level has records from five instances on"
        same_scene(host, dev, name)
        same_rays(capi, dev, host, cam, name)
        no_violations(A.check_instanced(dev.read_build(True), meshes, new), name)
        fresh = scene_ctx(capi, meshes, new, WI.materials(), cam, extra)
        same_digests(dev, fresh, name + ", against a fresh scene")
    finally:
        for c in (host, dev, fresh):
            if c is not None:
                c.close()


# ---- 2. REFIT equals the host call's results ------------------------------------------------------------------------------------
def refit_case(name):
    """(meshes, the scene's instances, the new ones): the same count and mesh choices"""
    meshes = small_meshes()
    n = {"n = 4": 4, "n = 257": 257}.get(name, 61)
    first = mixed(n, 3, 11)
    rng = np.random.RandomState(12)
    new = list(first)
    if name in ("a mild jitter", "n = 4", "n = 257"):
        for k in range(1, n):
            tr = np.array(first[k][0], np.float32)
            tr[:, 3] += np.float32(0.08 * rng.normal(size=3))
            new[k] = (tr, first[k][1], first[k][2])
    elif name == "permuted":
        for mesh in (1, 2):   # the transforms permuted among the instances of one mesh: far moves
            which = [k for k in range(n) if first[k][1] == mesh]
            for k, src in zip(which, rng.permutation(which)):
                new[k] = (first[src][0], mesh, first[k][2])
    elif name == "material offsets":
        new = [(tr, mesh, (off + 1) % 3) for tr, mesh, off in first]
    else:
        raise KeyError(name)
    return meshes, first, new


@pytest.mark.parametrize("name", ["a mild jitter", "permuted", "material offsets", "n = 4", "n = 257"])
def test_a_device_refit_gives_the_host_calls_results(capi, oracle, torch, name):
    meshes, first, new = refit_case(name)
    cam, extra = world_view(oracle, meshes, new)
    host, dev = (scene_ctx(capi, meshes, first, WI.materials(), cam, extra) for _ in range(2))
    try:
        depths, recs_before = depth_fields(dev), span(dev, "top.recs")
        assert (depths[3] == 0) == (name == "n = 4")
        t = on_device(torch, new, "float32")
        kept = bits(t)
        host.whitted_set_instances(new)
        dev.whitted_set_instances_device(t, refit=True)
        assert np.array_equal(bits(t), kept), "the caller's tensor changed"
        same_results(capi, dev, host, cam, name)
        assert np.array_equal(sorted_walk(dev), sorted_walk(host)), name + ": the InstWalk records differ"
        assert depth_fields(dev) == depths, name + ": a refit moved the depths"
        no_violations(A.check_instanced(dev.read_build(True), meshes, new), name)
        if name == "permuted":
            assert span(dev, "top.recs") != span(host, "top.recs"), "a refit over permuted transforms came out as the rebuilt top level: the comparison shows nothing"
        if name in ("a mild jitter", "permuted", "n = 257"):
            assert span(dev, "top.recs") != recs_before, name + ": the records did not move"
    finally:
        host.close()
        dev.close()


def test_a_refit_with_the_scenes_own_instances_reproduces_the_build_bit_for_bit(capi, oracle, torch):
    for n in (4, 61, 257):
        meshes, first = small_meshes(), mixed(n, 3, 11)
        cam, extra = world_view(oracle, meshes, first)
        ctx = scene_ctx(capi, meshes, first, WI.materials(), cam, extra)
        try:
            before = list(ctx.build_digest(True))
            ctx.whitted_set_instances_device(on_device(torch, first), refit=True)
            assert list(ctx.build_digest(True)) == before, n
            _, _, moved_inst = refit_case("a mild jitter" if n == 61 else "n = %d" % n)   # there and back
            ctx.whitted_set_instances_device(on_device(torch, moved_inst), refit=True)
            assert list(ctx.build_digest(True)) != before, n
            ctx.whitted_set_instances_device(on_device(torch, first), refit=True)
            assert list(ctx.build_digest(True)) == before, n
        finally:
            ctx.close()


def test_a_refit_works_after_the_host_call_and_after_a_device_rebuild(capi, oracle, torch):
    meshes, first, new = refit_case("a mild jitter")
    _, _, other = refit_case("permuted")
    cam, extra = world_view(oracle, meshes, new)
    host, dev = (scene_ctx(capi, meshes, mixed(9, 3, 4), WI.materials(), cam, extra) for _ in range(2))
    try:
        dev.whitted_set_instances(first)                                   # last set by the host call
        dev.whitted_set_instances_device(on_device(torch, new), refit=True)
        host.whitted_set_instances(new)
        same_results(capi, dev, host, cam, "a refit after the host call")
        dev.whitted_set_instances_device(on_device(torch, first))         # last set by a device rebuild
        host.whitted_set_instances(first)
        same_scene(dev, host, "the device rebuild")
        dev.whitted_set_instances_device(on_device(torch, other), refit=True)
        host.whitted_set_instances(other)
        same_results(capi, dev, host, cam, "a refit after a device rebuild")
        no_violations(A.check_instanced(dev.read_build(True), meshes, other), "a refit after a device rebuild")
    finally:
        host.close()
        dev.close()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def refusal_scene(capi, oracle, n=12):
    """a ground, a torus (material indices 0 and 1, four materials: a material offset of 3 is one too many) and an octahedron of
    extent 2"""
    meshes = [WI.ground(4.0, 0.0), WI.torus(16, 8), WI.octahedron(1.0)]
    inst = mixed(n, 3, 13)
    cam, extra = world_view(oracle, meshes, inst)
    return meshes, inst, cam, extra


def with_entry(inst, k, transform=None, mesh=None, off=None):
    out = list(inst)
    tr, m, o = out[k]
    out[k] = (tr if transform is None else np.asarray(transform, np.float32), m if mesh is None else mesh, o if off is None else off)
    return out


def poisoned(tr, r, c, value):
    tr = np.array(tr, np.float32)
    tr[r, c] = value
    return tr


def device_faults(inst):
    """name -> the instances with one fault of a kind inst_prepare_kernel decides (none changes a valid mesh choice: under
    RTGO_UPDATE_REFIT the same rule refuses them)"""
    eye3 = np.eye(3)
    torus_k = next(k for k in range(len(inst)) if inst[k][1] == 1)
    octa_k = next(k for k in range(len(inst)) if inst[k][1] == 2)
    return {
        "a mesh index beyond the meshes": with_entry(inst, 7, mesh=3),
        "a mesh index of 2^32 - 1": with_entry(inst, 2, mesh=0xFFFFFFFF),
        "material offset + the mesh's largest index beyond the table": with_entry(inst, torus_k, off=3),
        "a material offset of 2^32 - 1 (+ 1 wraps to 0 in 32 bits)": with_entry(inst, torus_k, off=0xFFFFFFFF),
        "a NaN in a transform": with_entry(inst, 4, transform=poisoned(inst[4][0], 1, 2, np.nan)),
        "an infinity in a translation": with_entry(inst, 9, transform=poisoned(inst[9][0], 2, 3, -np.inf)),
        "scales of 1e-11: |det| = 1e-33": with_entry(inst, 5, transform=WI.transform(1e-11 * eye3, [0, 1, 0])),
        "scales (1e-39, 1e5, 1e5): det 1e-29 passes, the inverse overflows": with_entry(inst, 6, transform=WI.transform(np.diag([1e-39, 1e5, 1e5]), [0, 1, 0])),
        "a box beyond the float range": with_entry(inst, octa_k, transform=WI.transform(1e38 * eye3, [3e38, 0, 0])),
    }


def refused_like_the_twin(capi, torch, dev, twin, inst, refit, what):
    """the device call on `inst` is refused with the code and message rtgo_whitted_set_instances gives `twin` on the same data"""
    t = on_device(torch, inst)
    kept = bits(t)
    with pytest.raises(capi.RtgoError) as host_err:
        twin.whitted_set_instances(inst)
    with pytest.raises(capi.RtgoError) as dev_err:
        dev.whitted_set_instances_device(t, refit=refit)
    assert str(dev_err.value) == str(host_err.value).replace("rtgo_whitted_set_instances", NAME), what
    assert np.array_equal(bits(t), kept), what + ": the caller's tensor changed"


@pytest.mark.parametrize("refit", REFITS)
def test_every_device_decided_fault_is_refused_as_the_host_call_refuses_it(capi, oracle, torch, refit):
    meshes, inst, cam, extra = refusal_scene(capi, oracle)
    dev, twin = (scene_ctx(capi, meshes, inst, WI.materials(), cam, extra) for _ in range(2))
    try:
        before, shown = list(dev.build_digest(True)), frames(dev)
        for what, bad in device_faults(inst).items():
            refused_like_the_twin(capi, torch, dev, twin, bad, refit, what)
            assert list(dev.build_digest(True)) == before, what
            same_frames(frames(dev), shown, what)
        same_digests(dev, twin, "after the refusals")
    finally:
        dev.close()
        twin.close()


@pytest.mark.parametrize("refit", REFITS)
def test_the_lowest_offending_instance_is_named_across_workgroups(capi, oracle, torch, refit):
    meshes, _, _, _ = refusal_scene(capi, oracle)
    inst = mixed(512, 3, 14, spacing=0.3)
    cam, extra = world_view(oracle, meshes, inst)
    dev, twin = (scene_ctx(capi, meshes, inst, WI.materials(), cam, extra) for _ in range(2))
    try:
        before = list(dev.build_digest(True))
        bad = with_entry(with_entry(inst, 300, mesh=9), 40, transform=poisoned(inst[40][0], 0, 0, np.nan))
        refused_like_the_twin(capi, torch, dev, twin, bad, refit, "300 and 40")
        with pytest.raises(capi.RtgoError, match=r"\(1\).*instance 40 has a non-finite or singular transform"):
            dev.whitted_set_instances_device(on_device(torch, bad), refit=refit)
        bad = with_entry(with_entry(inst, 300, transform=poisoned(inst[300][0], 0, 0, np.nan)), 40, off=0xFFFFFFFF)
        refused_like_the_twin(capi, torch, dev, twin, bad, refit, "300 and 40, the kinds exchanged")
        with pytest.raises(capi.RtgoError, match=r"\(1\).*instance 40: material offset"):
            dev.whitted_set_instances_device(on_device(torch, bad), refit=refit)
        assert list(dev.build_digest(True)) == before
    finally:
        dev.close()
        twin.close()


@pytest.mark.parametrize("refit", REFITS)
def test_what_the_host_call_accepts_at_the_edges_is_accepted(capi, oracle, torch, refit):
    """scales of 1e-9 (|det| = 1e-27); and a translation of 3e38 with a mesh of extent 2, whose box stays below FLT_MAX = 3.4e38 -- the
    host call accepts it (the box leaves the float range only with a scale on top: device_faults), so its device twin does"""
    meshes, inst, cam, extra = refusal_scene(capi, oracle)
    octa_k = next(k for k in range(len(inst)) if inst[k][1] == 2)
    edges = {"scales of 1e-9": with_entry(inst, 5, transform=WI.transform(1e-9 * np.eye(3), [0, 1, 0])),
             "a translation of 3e38": with_entry(inst, octa_k, transform=WI.transform(np.eye(3), [3e38, 0, 0]))}
    dev, twin = (scene_ctx(capi, meshes, inst, WI.materials(), cam, extra) for _ in range(2))
    try:
        for what, new in edges.items():
            twin.whitted_set_instances(new)
            dev.whitted_set_instances_device(on_device(torch, new), refit=refit)
            if refit:
                same_results(capi, dev, twin, cam, what)
                assert np.array_equal(sorted_walk(dev), sorted_walk(twin)), what
            else:
                same_scene(dev, twin, what)
    finally:
        dev.close()
        twin.close()


def test_a_refit_keeps_the_count_and_the_mesh_choices(capi, oracle, torch):
    meshes, inst, cam, extra = refusal_scene(capi, oracle)
    dev = scene_ctx(capi, meshes, inst, WI.materials(), cam, extra)
    try:
        before, shown = list(dev.build_digest(True)), frames(dev)
        swapped = with_entry(inst, 5, mesh=3 - inst[5][1])   # the torus for the octahedron or the other way: a valid instance, another mesh
        for what, bad, message in (("one instance fewer", inst[:-1], "instances"), ("one more", inst + [inst[1]], "instances"),
                                   ("a mesh changed", swapped, "instance 5 names another mesh")):
            t = on_device(torch, bad)
            kept = bits(t)
            with pytest.raises(capi.RtgoError, match=E_INVALID + ".*" + message):
                dev.whitted_set_instances_device(t, refit=True)
            assert list(dev.build_digest(True)) == before, what
            assert np.array_equal(bits(t), kept), what
        same_frames(frames(dev), shown, "after the refusals")
        dev.whitted_set_instances_device(on_device(torch, swapped))   # a rebuild takes it
        assert list(dev.build_digest(True)) != before
    finally:
        dev.close()


def test_the_refusals_the_host_decides(capi, oracle, torch):
    meshes, inst, cam, extra = refusal_scene(capi, oracle)
    dev = scene_ctx(capi, meshes, inst, WI.materials(), cam, extra)
    none, single = capi.Context(0), capi.Context(0)
    try:
        tor = meshes[1]
        single.whitted_set_mesh(tor["positions"], tor["normals"], tor["indices"], tor["tri_material"], WI.materials())
        before = list(dev.build_digest(True))
        t = on_device(torch, inst)
        wide = on_device(torch, mixed(8193, 3, 15))
        fn = dev._lib.rtgo_whitted_set_instances_device
        for flags in (capi.UPDATE_REFIT, capi.UPDATE_REBUILD):
            assert fn(dev._h, None, len(inst), flags) == 1                                  # a NULL pointer
            assert fn(dev._h, t[1:].reshape(-1)[1:].data_ptr(), len(inst) - 2, flags) == 1  # a pointer one byte off
            assert fn(none._h, t.data_ptr(), len(inst), flags) == 3                         # no scene
            assert fn(single._h, t.data_ptr(), len(inst), flags) == 3                       # a scene of rtgo_whitted_set_mesh
            assert fn(dev._h, t.data_ptr(), 0, flags) == 4                                  # n = 0
            assert fn(dev._h, wide.data_ptr(), 8193, flags) == 4                            # n = 8193
        assert fn(dev._h, t.data_ptr(), len(inst), 2) == 1                                  # flag 2
        assert fn(dev._h, t.data_ptr(), len(inst), 3) == 1
        with pytest.raises(capi.RtgoError, match=E_STATE):
            none.whitted_set_instances_device(t)
        with pytest.raises(capi.RtgoError, match=E_UNSUPPORTED):
            dev.whitted_set_instances_device(wide)
        with pytest.raises(capi.RtgoError, match=E_INVALID):
            dev.whitted_set_instances_device(t.reshape(-1)[1:1 + 56 * (len(inst) - 1)].reshape(-1, 56))
        for bad in (t.cpu(), t[:, :48], t.reshape(-1), t.to(torch.int16)):
            with pytest.raises(ValueError):
                dev.whitted_set_instances_device(bad)
        assert list(dev.build_digest(True)) == before
        assert fn(dev._h, t.data_ptr(), len(inst), capi.UPDATE_REFIT) == 0
        assert list(dev.build_digest(True)) == before   # (the scene's own instances)
    finally:
        for c in (dev, none, single):
            c.close()


# ---- 4. the context works afterwards as after the twin --------------------------------------------------------------------------
@pytest.mark.parametrize("refit", REFITS)
def test_the_other_calls_work_afterwards(capi, oracle, torch, refit):
    mesh, tor, octa = big(8320), WI.torus(16, 8), WI.octahedron(0.3)
    meshes = [WI.ground(4.0, -0.5), mesh, tor, octa]
    first = mixed(14, 4, 16, spacing=1.2)
    rng = np.random.RandomState(17)
    new = [(tr if k == 0 else WI.transform(np.asarray(tr)[:, :3] @ WI.rotation(rng), np.asarray(tr)[:, 3] + [0.1, 0.05, -0.1]), m, (off + 1) % 3)
           for k, (tr, m, off) in enumerate(first)]
    again = [(tr, m, (off + 2) % 3) for tr, m, off in new]
    cam, extra = world_view(oracle, meshes, new)
    dev, host = (scene_ctx(capi, meshes, first, WI.materials(), cam, extra) for _ in range(2))
    try:
        dev.whitted_set_instances_device(on_device(torch, new), refit=refit)
        host.whitted_set_instances(new)
        same_results(capi, dev, host, cam, "the device call")
        centre = np.float32([0.05, 0.1, -0.05])
        steps = [("update_mesh", lambda c: c.whitted_update_mesh(2, tor["positions"] * np.float32(1.2))),
                 ("update_meshes, a clustered entry included", lambda c: c.whitted_update_meshes([(1, mesh["positions"] + centre, None), (3, octa["positions"] * np.float32(1.5), None)])),
                 ("rebuild_meshes", lambda c: c.whitted_rebuild_meshes([(1, mesh["positions"] * np.float32(1.05), None), (2, tor["positions"], None)])),
                 ("set_instances", lambda c: c.whitted_set_instances(again)),
                 ("a second device call", lambda c: c.whitted_set_instances_device(on_device(torch, new), refit=refit) if c is dev else c.whitted_set_instances(new))]
        for what, step in steps:
            step(dev)
            step(host)
            # the mesh-update calls and the set calls build the top level again from the instances the context keeps: the same arrays
            # whichever call gave it those instances
            if what == "a second device call" and refit:
                same_results(capi, dev, host, cam, what)
            else:
                same_digests(dev, host, what)
        moved = [meshes[0], dict(mesh, positions=mesh["positions"] * np.float32(1.05)), tor, dict(octa, positions=octa["positions"] * np.float32(1.5))]
        no_violations(A.check_instanced(dev.read_build(True), moved, new), "after every step")
    finally:
        dev.close()
        host.close()


# ---- 5. a tensor that never was on the host -------------------------------------------------------------------------------------
@pytest.mark.parametrize("refit", REFITS)
def test_instances_packed_on_the_device(capi, oracle, torch, refit):
    meshes, first, new = refit_case("a mild jitter")
    cam, extra = world_view(oracle, meshes, new)
    shift = torch.tensor([0.0, 0.0, 0.0, 0.05, 0.0, 0.0, 0.0, 0.02, 0.0, 0.0, 0.0, -0.05], dtype=torch.float32, device="cuda")
    transforms = torch.from_numpy(np.stack([np.asarray(tr, np.float32).reshape(12) for tr, _, _ in new])).cuda() + shift
    t = capi.instances_tensor(transforms, torch.tensor([m for _, m, _ in new], device="cuda"), torch.tensor([o for _, _, o in new], device="cuda"))
    torch.cuda.synchronize()
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == (len(new), 14)
    kept = bits(t)
    made = [(row[:12].reshape(3, 4), int(m), int(o)) for row, (_, m, o) in zip(t.cpu().numpy(), new)]
    host, dev = (scene_ctx(capi, meshes, first, WI.materials(), cam, extra) for _ in range(2))
    try:
        host.whitted_set_instances(made)
        dev.whitted_set_instances_device(t, refit=refit)
        assert np.array_equal(bits(t), kept), "the caller's tensor changed"
        if refit:
            same_results(capi, dev, host, cam, "packed on the device")
        else:
            same_scene(dev, host, "packed on the device")
    finally:
        host.close()
        dev.close()
