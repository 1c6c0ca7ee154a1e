"""rtgo_whitted_set_scene_device, rtgo_whitted_set_mesh_device and rtgo_whitted_set_texcoords_device on the MI355X: a first build from
meshes that are on the device already.

Each call is the twin of its host-pointer call: afterwards the context holds, array for array, what the twin holds after the same data.
So every comparison is an equality against a second context that took the same data through the twin -- build digests span for span,
frames (64 x 48, the top level in LDS and through L2), closest hits, any-hit masks and shaded rays bit for bit -- and the calls that
follow (instances on host and device, mesh updates on the device) leave equal digests too, which pins what no digest span holds: the
largest material indices, the mesh boxes and the packed indices.  A refused call has the twin's code and the twin's message under its
own name and leaves digests, frames and the caller's tensors as they were.

Shapes are the smallest at which each path can go wrong: 1 triangle (a root that is a leaf), 2, three small meshes of which some lack
normals, texture coordinates or materials (zero-filled slices), 1025 vertices and triangles (mesh_check_kernel's second workgroup
holds one vertex and one triangle), 256 meshes (the cap, the table search), 8320 triangles (a clustered mesh), two meshes over the same
buffers."""
import numpy as np
import pytest

import whitted_instances as WI
from test_whitted_instances_device import mixed, on_device, same_results, same_scene
from test_whitted_rebuild_meshes import same_digests
from test_whitted_update_meshes import E_INVALID, E_STATE, E_UNSUPPORTED, EYE, H, W, big, checker, frames, layout, same_frames, same_rays, scene_ctx, world_view

pytestmark = pytest.mark.gpu
SCENE, MESH, UV = "rtgo_whitted_set_scene", "rtgo_whitted_set_mesh", "rtgo_whitted_set_texcoords"
ARRAYS = ("positions", "normals", "texcoords", "indices", "tri_material")


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


# ---- meshes ---------------------------------------------------------------------------------------------------------------------
def to_device(torch, meshes):
    """the meshes' arrays as device tensors, their uploads complete (one tensor per distinct array: meshes that share an array share it
    on the device too); indices and material words as int32 bits"""
    made = {}

    def put(a, dt):
        if a is None:
            return None
        if id(a) not in made:
            made[id(a)] = torch.from_numpy(np.ascontiguousarray(a, dt).view(np.int32 if dt == np.uint32 else dt).copy()).cuda()
        return made[id(a)]

    out = [{k: put(m.get(k), np.float32 if k in ARRAYS[:3] else np.uint32) for k in ARRAYS} for m in meshes]
    torch.cuda.synchronize()
    return out


def bits(dev_meshes):
    """the bytes of every tensor of the meshes (a tensor that several meshes share is read once)"""
    seen = {}
    for m in dev_meshes:
        for t in m.values():
            if t is not None and id(t) not in seen:
                seen[id(t)] = t.cpu().numpy().view(np.uint8).copy()
    return [None if t is None else seen[id(t)] for m in dev_meshes for t in m.values()]


def unchanged(dev_meshes, kept, what):
    for a, b in zip(bits(dev_meshes), kept):
        assert (a is None and b is None) or np.array_equal(a, b), what + ": a tensor of the caller's changed"


def device_ctx(capi, torch, meshes, inst, mats, cam, extra):
    """scene_ctx through rtgo_whitted_set_scene_device; returns (context, the tensors)"""
    ctx = capi.Context(0)
    dm = to_device(torch, meshes)
    kept = bits(dm)
    ctx.whitted_set_scene_device(dm, inst, mats)
    unchanged(dm, kept, "set_scene_device")
    for mi, (bc, mr, nm) in (extra.get("textures") or {}).items():
        ctx.whitted_set_material_textures(mi, bc, mr, nm)
    ctx.whitted_set_lights(extra["lights"])
    ctx.whitted_set_miss_color(extra["miss"])
    ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])
    ctx.resize(W * H)
    return ctx, dm


def with_uv(mesh, seed=5):
    return dict(mesh, texcoords=np.random.RandomState(seed).rand(len(mesh["positions"]), 2).astype(np.float32))


def one_triangle():
    return {"positions": np.float32([[-1, 0, -1], [0, 0, 1], [1, 0, -1]]), "normals": np.float32([[0, 1, 0]] * 3),
            "texcoords": np.float32([[0, 0], [0.5, 1], [1, 0]]), "indices": np.uint32([[0, 1, 2]]), "tri_material": np.uint32([1])}


def band(n=1025):
    """n vertices and n triangles with every array: a band that winds up a cylinder, triangle i over vertices i, i + 1, i + 2 (mod n)"""
    i = np.arange(n)
    a = 2 * np.pi * (i // 2) / 64.3
    p = np.stack([np.cos(a), 0.3 * (i % 2) + 0.01 * (i // 2), np.sin(a)], axis=1)
    nrm = np.stack([np.cos(a), np.zeros(n), np.sin(a)], axis=1)
    return {"positions": p.astype(np.float32), "normals": nrm.astype(np.float32), "texcoords": np.stack([(i // 2) / 16.0 % 1.0, i % 2], axis=1).astype(np.float32),
            "indices": np.stack([i, (i + 1) % n, (i + 2) % n], axis=1).astype(np.uint32), "tri_material": (i % 3).astype(np.uint32)}


def small_meshes():
    """a torus with normals, texture coordinates and materials; a ground and an octahedron with positions and indices alone"""
    return [WI.ground(4.0, 0.0), with_uv(WI.torus(16, 8)), WI.octahedron(0.3)]


def textures():
    return {k: (checker(), None, None) for k in range(4)}


def case(name):
    """(meshes, instances, textures or None)"""
    if name == "1 triangle":
        return [one_triangle()], [(EYE, 0, 0)], None
    if name == "2 triangles":
        return [WI.ground(1.0, 0.0)], [(EYE, 0, 2)], None
    if name == "three small meshes":
        return small_meshes(), mixed(7, 3, 1), None
    if name == "three small meshes, textured":
        return small_meshes(), mixed(7, 3, 1), textures()
    if name == "1025 vertices and triangles":
        return [band()], [(EYE, 0, 1)], textures()
    if name == "256 meshes":
        meshes = [WI.octahedron(0.05 + 0.0005 * k) for k in range(256)]
        return meshes, [(WI.transform(np.eye(3), [0.25 * (k % 16), 0.1 * (k % 3), 0.25 * (k // 16)]), k, k % 4) for k in range(256)], None
    if name == "a clustered mesh":
        return [big(8320, texcoords=True)], layout("two"), textures()
    if name == "two meshes over the same buffers":
        tor = with_uv(WI.torus(16, 8))
        return [tor, dict(tor)], [(WI.transform(np.eye(3), [-0.7, 0, 0]), 0, 0), (WI.transform(0.8 * np.eye(3), [0.7, 0.2, 0]), 1, 2)], textures()
    raise KeyError(name)


CASES = ["1 triangle", "2 triangles", "three small meshes", "three small meshes, textured", "1025 vertices and triangles", "256 meshes", "a clustered mesh",
         "two meshes over the same buffers"]


# ---- 1. equality with the twin --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_a_scene_from_device_buffers_is_the_host_calls_scene(capi, oracle, torch, name):
    meshes, inst, tex = case(name)
    cam, extra = world_view(oracle, meshes, inst)
    extra["textures"] = tex
    host = scene_ctx(capi, meshes, inst, WI.materials(), cam, extra)
    dev = None
    try:
        dev, dm = device_ctx(capi, torch, meshes, inst, WI.materials(), cam, extra)
        if name == "two meshes over the same buffers":
            assert dm[0]["positions"].data_ptr() == dm[1]["positions"].data_ptr() and dm[0]["indices"].data_ptr() == dm[1]["indices"].data_ptr()
        same_digests(host, dev, name)
        same_results(capi, dev, host, cam, name)
        if tex:   # ... and the packed texture coordinates show: the same scene without the textures differs
            bare, _ = device_ctx(capi, torch, meshes, inst, WI.materials(), cam, dict(extra, textures=None))
            try:
                assert not np.array_equal(frames(dev)[1], frames(bare)[1]), "the textures do not show in this frame"
            finally:
                bare.close()
    finally:
        host.close()
        if dev is not None:
            dev.close()


def single_ctx(capi, cam, extra):
    ctx = capi.Context(0)
    ctx.whitted_set_lights(extra["lights"])
    ctx.whitted_set_miss_color(extra["miss"])
    ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])
    ctx.resize(W * H)
    return ctx


def same_single(capi, a, b, cam, what):
    assert list(a.build_digest(True)) == list(b.build_digest(True)), what
    same_results(capi, a, b, cam, what)


@pytest.mark.parametrize("name", ["a torus", "bare"])
def test_set_mesh_device_then_texcoords_then_a_texture(capi, oracle, torch, name):
    mesh = with_uv(WI.torus(16, 8)) if name == "a torus" else dict(WI.octahedron(1.0), texcoords=np.random.RandomState(2).rand(6, 2).astype(np.float32))
    cam, extra = world_view(oracle, [mesh], [(EYE, 0, 0)])
    host, dev = single_ctx(capi, cam, extra), single_ctx(capi, cam, extra)
    try:
        dm = to_device(torch, [mesh])
        kept = bits(dm)
        d = dm[0]
        host.whitted_set_mesh(mesh["positions"], mesh["normals"], mesh["indices"], mesh["tri_material"], WI.materials())
        dev.whitted_set_mesh_device(d["positions"], d["normals"], d["indices"], d["tri_material"], WI.materials())
        same_single(capi, dev, host, cam, name + ": set_mesh_device")
        host.whitted_set_texcoords(mesh["texcoords"])
        dev.whitted_set_texcoords_device(d["texcoords"])
        for ctx in (host, dev):
            ctx.whitted_set_material_textures(0, checker(), None, None)
            ctx.whitted_set_material_textures(1, checker(4), None, None)
        same_single(capi, dev, host, cam, name + ": textured")
        shown = frames(dev)
        host.whitted_set_texcoords(None)
        dev.whitted_set_texcoords_device(None)
        same_single(capi, dev, host, cam, name + ": the coordinates removed")
        assert not np.array_equal(frames(dev)[1], shown[1]), "the texture coordinates did not show"
        # ... and the update calls take the scene as the twin's
        moved = (mesh["positions"] * np.float32(1.1)).astype(np.float32)
        dev.whitted_update_meshes_device([(0, torch.from_numpy(moved).cuda(), None)], rebuild=True)
        host.whitted_rebuild_meshes([(0, moved, None)])
        assert list(dev.build_digest(True)) == list(host.build_digest(True))
        unchanged(dm, kept, name)
    finally:
        host.close()
        dev.close()


# ---- 2. the calls afterwards ----------------------------------------------------------------------------------------------------
def test_the_calls_afterwards_behave_as_after_the_twin(capi, oracle, torch):
    """torus(16, 8) has material indices 0 and 1 and the table four entries: a material offset of 2 is the last that fits"""
    bigm, tor, octa = big(8320, texcoords=True), with_uv(WI.torus(16, 8)), WI.octahedron(0.3)
    meshes = [WI.ground(4.0, -0.5), bigm, tor, octa]
    first = mixed(14, 4, 16, spacing=1.2)
    cam, extra = world_view(oracle, meshes, first)
    host = scene_ctx(capi, meshes, first, WI.materials(), cam, extra)
    dev = None
    try:
        dev, dm = device_ctx(capi, torch, meshes, first, WI.materials(), cam, extra)
        kept = bits(dm)
        torus_k = next(k for k in range(len(first)) if first[k][1] == 2)
        fits = [(tr, m, 2 if k == torus_k else off) for k, (tr, m, off) in enumerate(first)]
        too_far = [(tr, m, 3 if k == torus_k else off) for k, (tr, m, off) in enumerate(first)]
        rng = np.random.RandomState(17)
        turned = [(tr if k == 0 else WI.transform(np.asarray(tr)[:, :3] @ WI.rotation(rng), np.asarray(tr)[:, 3] + [0.1, 0.05, -0.1]), m, off)
                  for k, (tr, m, off) in enumerate(fits)]
        nudged = [(tr if k == 0 else WI.transform(np.asarray(tr)[:, :3], np.asarray(tr)[:, 3] + [0.0, 0.1, 0.0]), m, off) for k, (tr, m, off) in enumerate(turned)]
        tor_moved = torch.from_numpy((tor["positions"] * np.float32(1.2)).astype(np.float32)).cuda()
        big_moved = torch.from_numpy((bigm["positions"] + np.float32([0.05, 0.1, -0.05])).astype(np.float32)).cuda()
        torch.cuda.synchronize()
        steps = [("set_instances, the largest offset that fits", lambda c: c.whitted_set_instances(fits)),
                 ("set_instances_device, rebuilt", lambda c: c.whitted_set_instances_device(on_device(torch, turned))),
                 ("set_instances_device, refitted", lambda c: c.whitted_set_instances_device(on_device(torch, nudged), refit=True)),
                 ("update_meshes_device, refitted", lambda c: c.whitted_update_meshes_device([(2, tor_moved, None), (1, big_moved, None)])),
                 ("update_meshes_device, rebuilt", lambda c: c.whitted_update_meshes_device([(1, big_moved, None), (2, tor_moved, None)], rebuild=True)),
                 ("a texture", lambda c: c.whitted_set_material_textures(2, checker(), None, None))]
        for what, step in steps:
            step(dev)
            step(host)
            same_scene(host, dev, what)
            if what.startswith("set_instances, "):   # one more does not fit: the same refusal
                errs = []
                for c in (host, dev):
                    with pytest.raises(capi.RtgoError, match=E_INVALID + ".*material offset") as e:
                        c.whitted_set_instances(too_far)
                    errs.append(str(e.value))
                assert errs[0] == errs[1]
                same_scene(host, dev, what + ", after the refusal")
        same_rays(capi, dev, host, cam, "after every step")
        unchanged(dm, kept, "after every step")
    finally:
        host.close()
        if dev is not None:
            dev.close()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def structs(capi, meshes, device):
    """rtgo_whitted_mesh[len(meshes)] over numpy arrays (device False) or tensors (True): (the array, what keeps the memory alive)"""
    ms = (capi.WhittedMesh * max(len(meshes), 1))()
    keep = []
    for k, m in enumerate(meshes):
        p = []
        for name in ARRAYS:
            a = m.get(name)
            if a is not None and not device:
                a = np.ascontiguousarray(a, np.float32 if name in ARRAYS[:3] else np.uint32)
            keep.append(a)
            p.append(None if a is None else a.data_ptr() if device else a.ctypes.data)
        ms[k] = capi.WhittedMesh(p[0], p[1], p[2], len(m["positions"]), p[3], p[4], len(m["indices"]))
    return ms, keep


def call(capi, ctx, device, ms, n_meshes, inst, mats, n_inst=None, n_mats=4):
    """the bare C call: (code, message).  mats: the material table, or None for a NULL pointer"""
    fn = getattr(ctx._lib, SCENE + ("_device" if device else ""))
    arr = None if inst is None else capi.whitted_instances(inst)
    mats = None if mats is None else np.ascontiguousarray(mats, np.float32)
    rc = fn(ctx._h, ms, n_meshes, arr, len(inst) if n_inst is None else n_inst, None if mats is None else mats.ctypes.data, n_mats)
    return rc, ctx._lib.rtgo_last_error(ctx._h).decode()


def refused_alike(capi, torch, dev, twin, meshes, inst, what, patch=None, n_meshes=None, null_materials=False, **counts):
    """both calls on the same data (patch: applied to both struct arrays) are refused with the same code, and the device call's message is
    the twin's under its own name; the caller's tensors stay"""
    mats = None if null_materials else WI.materials()
    dm = to_device(torch, meshes)
    kept = bits(dm)
    out = []
    for device, ctx, data in ((False, twin, meshes), (True, dev, dm)):
        ms, keep = structs(capi, data, device)
        if patch:
            patch(ms)
        out.append(call(capi, ctx, device, ms, len(meshes) if n_meshes is None else n_meshes, inst, mats, **counts))
    (host_rc, host_msg), (dev_rc, dev_msg) = out
    assert host_rc != 0, what + ": the twin accepted it"
    assert (dev_rc, dev_msg) == (host_rc, host_msg.replace(SCENE, SCENE + "_device")), what
    unchanged(dm, kept, what)
    return dev_rc, dev_msg


def refusal_meshes():
    """a torus with every array and one more vertex that no triangle names (the last floats of positions, normals and texcoords are its),
    a ground, an octahedron"""
    tor = with_uv(WI.torus(16, 8))
    tor = dict(tor, positions=np.concatenate([tor["positions"], np.float32([[0.1, 0.2, 0.3]])]), normals=np.concatenate([tor["normals"], np.float32([[0, 1, 0]])]),
               texcoords=np.concatenate([tor["texcoords"], np.float32([[0.5, 0.5]])]))
    return [tor, WI.ground(4.0, 0.0), WI.octahedron(0.3)]


def poisoned(mesh, name, where, value):
    a = np.array(mesh[name])
    a[where] = value
    return dict(mesh, **{name: a})


def data_faults(meshes):
    """name -> (the meshes with faults of the kinds the device decides, what the message says)"""
    tor, gnd, octa = meshes
    nv = len(tor["positions"])
    return {
        "an index equal to n_vertices in the first triangle of mesh 0": ([poisoned(tor, "indices", (0, 1), nv), gnd, octa], "mesh 0: index beyond"),
        "index 2^32 - 1 in the last triangle of the last mesh": ([tor, gnd, poisoned(octa, "indices", (-1, -1), 0xFFFFFFFF)], "mesh 2: index beyond"),
        "a NaN in the last position, which no triangle names": ([poisoned(tor, "positions", (-1, -1), np.nan), gnd, octa], "mesh 0: non-finite vertex data"),
        "+Inf in the last normal": ([poisoned(tor, "normals", (-1, -1), np.inf), gnd, octa], "mesh 0: non-finite vertex data"),
        "a NaN in the last texture coordinate": ([poisoned(tor, "texcoords", (-1, -1), np.nan), gnd, octa], "mesh 0: non-finite texture coordinate"),
        "a material index equal to n_materials": ([poisoned(tor, "tri_material", -1, 4), gnd, octa], "mesh 0: material index beyond"),
        "a bad material and a bad texture coordinate in one mesh": ([poisoned(poisoned(tor, "tri_material", 0, 9), "texcoords", (3, 0), np.nan), gnd, octa],
                                                                    "mesh 0: non-finite texture coordinate"),
        "a bad vertex and a bad index in one mesh": ([poisoned(poisoned(tor, "positions", (0, 0), -np.inf), "indices", (100, 2), nv + 7), gnd, octa],
                                                     "mesh 0: index beyond"),
        "faults in meshes 1 and 2": ([tor, poisoned(gnd, "positions", (2, 1), np.nan), poisoned(octa, "indices", (0, 0), 6)], "mesh 1: non-finite vertex data"),
    }


@pytest.fixture(scope="module")
def refusal_pair(capi, oracle, torch):
    """two contexts over the same valid scene, (device call's, twin's), with the scene's digests and frames"""
    meshes = refusal_meshes()
    inst = [(EYE, 1, 0), (WI.transform(np.eye(3), [0.0, 0.5, 0.0]), 0, 1), (WI.transform(np.eye(3), [1.2, 0.5, 0.3]), 2, 3)]
    cam, extra = world_view(oracle, meshes, inst)
    twin = scene_ctx(capi, meshes, inst, WI.materials(), cam, extra)
    dev, _ = device_ctx(capi, torch, meshes, inst, WI.materials(), cam, extra)
    yield dev, twin, meshes, inst, list(dev.build_digest(True)), frames(dev)
    dev.close()
    twin.close()


def as_it_was(pair, what):
    dev, twin, _, _, before, shown = pair
    assert list(dev.build_digest(True)) == before, what + ": the scene changed"
    same_frames(frames(dev), shown, what)


def test_every_fault_in_the_data_is_refused_as_the_twin_refuses_it(capi, torch, refusal_pair):
    dev, twin, meshes, inst = refusal_pair[:4]
    for what, (bad, says) in data_faults(meshes).items():
        rc, msg = refused_alike(capi, torch, dev, twin, bad, inst, what)
        assert rc == 1 and says in msg, (what, rc, msg)
        as_it_was(refusal_pair, what)
    same_digests(dev, twin, "after the refusals")


def test_the_twins_order_holds_between_host_and_device_decided_faults(capi, torch, refusal_pair):
    dev, twin, meshes, inst = refusal_pair[:4]
    tor, gnd, octa = meshes
    bad_octa = poisoned(octa, "positions", (0, 0), np.nan)

    def no_triangles(ms):
        ms[1].n_triangles = 0

    rc, msg = refused_alike(capi, torch, dev, twin, [tor, gnd, bad_octa], inst, "mesh 1's count, mesh 2's data", patch=no_triangles)
    assert rc == 4 and "mesh 1: triangle count" in msg, msg
    as_it_was(refusal_pair, "mesh 1's count, mesh 2's data")
    rc, msg = refused_alike(capi, torch, dev, twin, [poisoned(tor, "tri_material", 5, 4), gnd, bad_octa], inst, "mesh 0's data, mesh 1's count", patch=no_triangles)
    assert rc == 1 and "mesh 0: material index beyond" in msg, msg
    as_it_was(refusal_pair, "mesh 0's data, mesh 1's count")


def test_pointers_and_counts_are_refused_on_the_host(capi, torch, refusal_pair):
    dev, twin, meshes, inst = refusal_pair[:4]

    def field(k, name, value):
        def patch(ms):
            setattr(ms[k], name, value)
        return patch

    cases = {
        "NULL positions": (dict(patch=field(1, "positions", None)), 1, "mesh 1: NULL positions or indices"),
        "NULL indices": (dict(patch=field(2, "indices", None)), 1, "mesh 2: NULL positions or indices"),
        "no triangles": (dict(patch=field(0, "n_triangles", 0)), 4, "mesh 0: triangle count"),
        "a mesh beyond the triangle cap": (dict(patch=field(0, "n_triangles", (1 << 24) + 1)), 4, "mesh 0: triangle count"),
        "no vertices": (dict(patch=field(2, "n_vertices", 0)), 4, "mesh 2: triangle count"),
        "no meshes": (dict(n_meshes=0), 4, "mesh count"),
        "257 meshes": (dict(n_meshes=257), 4, "mesh count"),
        "no materials": (dict(n_mats=0), 4, "materials non-empty"),
        "no instances": (dict(n_inst=0), 4, "instance count"),
        "8193 instances": (dict(n_inst=8193), 4, "instance count"),
        "NULL materials": (dict(null_materials=True), 1, "NULL argument"),
    }
    for what, (kw, code, says) in cases.items():
        rc, msg = refused_alike(capi, torch, dev, twin, meshes, inst, what, **kw)
        assert rc == code and says in msg, (what, rc, msg)
        as_it_was(refusal_pair, what)
    # NULL meshes, NULL instances; an instance that the meshes refuse
    dm = to_device(torch, meshes)
    ms, keep = structs(capi, dm, True)
    assert call(capi, dev, True, None, 3, inst, WI.materials())[0] == 1
    assert call(capi, dev, True, ms, 3, None, WI.materials(), n_inst=3)[0] == 1
    for bad_inst, says in (([(EYE, 3, 0)], "names a mesh beyond"), ([(EYE, 0, 3)], "material offset + material index")):
        rc, msg = refused_alike(capi, torch, dev, twin, meshes, bad_inst, says)
        assert rc == 1 and says in msg, msg
    # a pointer two bytes off: no twin, the code and a message of its own; for every array
    for k, name in ((0, "positions"), (0, "normals"), (0, "texcoords"), (2, "indices"), (0, "material_of_triangle")):
        ms, keep = structs(capi, dm, True)
        setattr(ms[k], name, getattr(ms[k], name) + 2)
        rc, msg = call(capi, dev, True, ms, 3, inst, WI.materials())
        assert rc == 1 and msg == "%s_device: mesh %d: a pointer is not 4-byte aligned" % (SCENE, k), (name, rc, msg)
    as_it_was(refusal_pair, "pointers")
    # the Python binding refuses what the library could not read, before calling it
    d = dm[0]
    for bad in (dict(d, positions=meshes[0]["positions"]), dict(d, positions=d["positions"].cpu()), dict(d, positions=d["positions"].double()),
                dict(d, indices=d["indices"].reshape(-1)), dict(d, normals=d["normals"][:-1]), dict(d, texcoords=d["positions"][:, ::2]),
                dict(d, tri_material=d["tri_material"].float())):
        with pytest.raises(ValueError):
            dev.whitted_set_scene_device([bad], [(EYE, 0, 0)], WI.materials())
    as_it_was(refusal_pair, "the binding's refusals")


def test_the_scene_triangle_limit_is_the_twins(capi, torch, refusal_pair):
    """four meshes of 2^24 triangles fill the scene's limit, a fifth passes it: the four are checked first, by both calls (they name one
    buffer of 2^24 index triples, all vertex 0)"""
    dev, twin, meshes, inst = refusal_pair[:4]
    full = {"positions": np.float32([[0, 0, 0], [1, 0, 0], [0, 0, 1]]), "normals": None, "indices": np.zeros((1 << 24, 3), np.uint32), "tri_material": None}
    rc, msg = refused_alike(capi, torch, dev, twin, [full] * 4 + [meshes[2]], [(EYE, 4, 0)], "the scene's triangle limit")
    assert rc == 4 and "mesh 4: the meshes hold more than" in msg, msg
    as_it_was(refusal_pair, "the scene's triangle limit")


def test_set_mesh_device_and_set_texcoords_device_refuse_as_their_twins(capi, oracle, torch):
    mesh = refusal_meshes()[0]
    cam, extra = world_view(oracle, [mesh], [(EYE, 0, 0)])
    host, dev, none = single_ctx(capi, cam, extra), single_ctx(capi, cam, extra), capi.Context(0)
    try:
        d = to_device(torch, [mesh])[0]
        host.whitted_set_mesh(mesh["positions"], mesh["normals"], mesh["indices"], mesh["tri_material"], WI.materials())
        dev.whitted_set_mesh_device(d["positions"], d["normals"], d["indices"], d["tri_material"], WI.materials())
        before, shown = list(dev.build_digest(True)), frames(dev)
        nv = len(mesh["positions"])

        def alike(fn_host, fn_dev, name, what, stays=True):
            with pytest.raises(capi.RtgoError) as eh:
                fn_host()
            with pytest.raises(capi.RtgoError) as ed:
                fn_dev()
            assert str(ed.value) == str(eh.value).replace(name, name + "_device"), what
            if stays:
                assert list(dev.build_digest(True)) == before, what
                same_frames(frames(dev), shown, what)

        faults = data_faults(refusal_meshes())
        for what in ("an index equal to n_vertices in the first triangle of mesh 0", "a NaN in the last position, which no triangle names", "+Inf in the last normal",
                     "a material index equal to n_materials", "a bad vertex and a bad index in one mesh"):
            m = faults[what][0][0]
            t = to_device(torch, [m])[0]
            kept = bits([t])
            alike(lambda: host.whitted_set_mesh(m["positions"], m["normals"], m["indices"], m["tri_material"], WI.materials()),
                  lambda: dev.whitted_set_mesh_device(t["positions"], t["normals"], t["indices"], t["tri_material"], WI.materials()), MESH, what)
            unchanged([t], kept, what)
        octa = dict(WI.octahedron(0.3))
        octa["indices"] = poisoned(octa, "indices", (-1, -1), 0xFFFFFFFF)["indices"]
        t = to_device(torch, [octa])[0]
        alike(lambda: host.whitted_set_mesh(octa["positions"], None, octa["indices"], None, WI.materials()),
              lambda: dev.whitted_set_mesh_device(t["positions"], None, t["indices"], None, WI.materials()), MESH, "index 2^32 - 1 in the last triangle")
        # counts, NULL and alignment
        fn, mats = dev._lib.rtgo_whitted_set_mesh_device, WI.materials()
        p, n, i, tm, nt = d["positions"].data_ptr(), d["normals"].data_ptr(), d["indices"].data_ptr(), d["tri_material"].data_ptr(), len(mesh["indices"])
        assert fn(dev._h, None, n, nv, i, tm, nt, mats.ctypes.data, 4) == 1
        assert fn(dev._h, p, n, nv, None, tm, nt, mats.ctypes.data, 4) == 1
        assert fn(dev._h, p, n, nv, i, tm, nt, None, 4) == 1
        for args in ((p + 2, n, nv, i, tm, nt), (p, n + 2, nv, i, tm, nt), (p, n, nv, i + 2, tm, nt), (p, n, nv, i, tm + 2, nt)):
            assert fn(dev._h, *args, mats.ctypes.data, 4) == 1
            assert "4-byte aligned" in dev._lib.rtgo_last_error(dev._h).decode()
        for args in ((p, n, nv, i, tm, 0), (p, n, nv, i, tm, 8193), (p, n, 0, i, tm, nt)):
            assert fn(dev._h, *args, mats.ctypes.data, 4) == 4
        assert fn(dev._h, p, n, nv, i, tm, nt, mats.ctypes.data, 0) == 4
        hfn = host._lib.rtgo_whitted_set_mesh
        assert hfn(host._h, mesh["positions"].ctypes.data, None, nv, mesh["indices"].ctypes.data, None, 8193, mats.ctypes.data, 4) == 4
        assert fn(dev._h, p, None, nv, i, None, 8193, mats.ctypes.data, 4) == 4
        assert dev._lib.rtgo_last_error(dev._h).decode() == host._lib.rtgo_last_error(host._h).decode().replace(MESH, MESH + "_device")
        assert list(dev.build_digest(True)) == before
        # texture coordinates
        uv_bad = poisoned(mesh, "texcoords", (-1, -1), np.nan)["texcoords"]
        t_bad = torch.from_numpy(uv_bad).cuda()
        for uv, t, what in ((uv_bad, t_bad, "a NaN in the last coordinate"), (mesh["texcoords"][:-1], d["texcoords"][:-1], "one vertex fewer")):
            alike(lambda: host.whitted_set_texcoords(uv), lambda: dev.whitted_set_texcoords_device(t), UV, what)
        assert np.isnan(t_bad.cpu().numpy()[-1, -1]) and np.array_equal(t_bad.cpu().numpy()[:-1], uv_bad[:-1])
        ufn = dev._lib.rtgo_whitted_set_texcoords_device
        assert ufn(dev._h, d["texcoords"].data_ptr() + 2, nv) == 1
        assert ufn(none._h, d["texcoords"].data_ptr(), nv) == 3 and ufn(none._h, None, 0) == 3
        for bad in (mesh["texcoords"], d["texcoords"].cpu(), d["texcoords"].double(), d["positions"], d["texcoords"].reshape(-1)):
            with pytest.raises(ValueError):
                dev.whitted_set_texcoords_device(bad)
        # an instanced scene takes them per mesh
        for c, device in ((host, False), (dev, True)):
            ms, keep = structs(capi, to_device(torch, [mesh]) if device else [mesh], device)
            assert call(capi, c, device, ms, 1, [(EYE, 0, 0)], WI.materials())[0] == 0
        alike(lambda: host.whitted_set_texcoords(mesh["texcoords"]), lambda: dev.whitted_set_texcoords_device(d["texcoords"]), UV, "an instanced scene", stays=False)
    finally:
        for c in (host, dev, none):
            c.close()


def test_a_refused_first_call_leaves_no_scene(capi, torch):
    meshes = refusal_meshes()
    bad = to_device(torch, [poisoned(meshes[0], "indices", (7, 0), 1 << 20), meshes[1]])
    ctx = capi.Context(0)
    try:
        ctx.resize(W * H)
        with pytest.raises(capi.RtgoError, match=E_INVALID + ".*mesh 0: index beyond the vertex array"):
            ctx.whitted_set_scene_device(bad, [(EYE, 0, 0)], WI.materials())
        with pytest.raises(capi.RtgoError, match=E_STATE):
            ctx.whitted_launch(W, H, 0)
        d = bad[0]
        with pytest.raises(capi.RtgoError, match=E_INVALID + ".*index beyond the vertex array"):
            ctx.whitted_set_mesh_device(d["positions"], d["normals"], d["indices"], d["tri_material"], WI.materials())
        with pytest.raises(capi.RtgoError, match=E_STATE):
            ctx.whitted_launch(W, H, 0)
        with pytest.raises(capi.RtgoError, match=E_UNSUPPORTED):
            ctx.whitted_set_scene_device(bad[1:], [], WI.materials())
    finally:
        ctx.close()
