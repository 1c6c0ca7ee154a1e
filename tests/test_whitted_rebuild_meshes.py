"""rtgo_whitted_rebuild_meshes and the batched builds on the MI355X.

Two claims, both equalities (no comparison here has a tolerance):

* batched = sequential: rtgo_whitted_set_scene builds every structure of the call through one table (one workgroup per structure); with
  RTGO_WHITTED_SEQ_BUILD=1 it builds them one after another as it always did.  The two leave the same arrays, digest for digest over
  the spans of rtgo_debug_build_digest, and so the same frames.
* rebuild = fresh: after rtgo_whitted_rebuild_meshes the context holds what a fresh rtgo_whitted_set_scene (rtgo_whitted_set_mesh) with
  the new vertices holds, digest for digest -- stronger than "the same frame", which any tree gives (a refit gives it too: case 3
  asserts that a refit's digests differ, so the comparison bites).  A refused call leaves the digests and the frames as they were.

Meshes, deformations and helpers are those of tests/test_whitted_update_meshes.py: 8320 triangles (three clusters, a mid level of one
leaf), 16 512 (five clusters, the first mid level with records), 40 000 (ten clusters); 64 x 48 frames, subframes 0 and 1.

The Morton fallback (a surface-area tree deeper than the walk's stack gets its Morton records back): `repeated` below is the idiom of
test_gpu_parity's coincident-triangles test at cluster size -- a few distinct triangles, each repeated thousands of times, so that every
sweep of the surface-area pass ties.  It goes through case 1 like the other scenes; whether its clusters take the fallback is printed,
not asserted (ties go to the median, so the tree stays shallow: no input that reaches the fallback is known)."""
import numpy as np
import pytest

import accel_check as A
import whitted_instances as WI
import whitted_scene
from test_trace_rays import Knob
from test_whitted_update_meshes import (DEFORM, E_INVALID, E_STATE, EYE, H, MODES, W, big, checker, frames, layout, no_violations, same_frames, same_pixels,
                                        scene_ctx, sine, world_view)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import capi as m
    m.load()
    return m


def same_digests(a, b, what):
    """the build digests of two contexts, span for span (the names are read_build's, in the same order)"""
    da, db = list(a.build_digest(True)), list(b.build_digest(True))
    names = list(a.read_build(True))
    assert len(da) == len(db) == len(names), (what, len(da), len(db), len(names))
    assert da == db, "%s: spans differ: %s" % (what, [n for n, x, y in zip(names, da, db) if x != y])


def moved(meshes, updates):
    new = list(meshes)
    for k, pos, nrm in updates:
        new[k] = dict(new[k], positions=np.ascontiguousarray(pos, np.float32))
        if nrm is not None:
            new[k]["normals"] = nrm
    return new


def beside(positions=None):
    """mesh 0 under the "two" layout, mesh 1 (a small one) beside it"""
    return layout("two", positions) + [(WI.transform(0.6 * np.eye(3), [-0.9, 0.4, 0.6]), 1, 2)]


# ---- case 1: batched = sequential -----------------------------------------------------------------------------------------------
def repeated(n_each=3000):
    """three distinct triangles, each n_each times: 9000 triangles, three clusters whose leaves' boxes are all equal or nearly so.
    (The triangles lean out of their planes: a cluster of copies of one axis-aligned triangle has no extent on an axis, and its 16-bit
    grid's last cell then ends one float below the fp32 plane -- in the sequential build as in the batched one, so not this file's
    subject; accel_check reports it.)"""
    pos = np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.1], [0.0, 1.5, 0.3], [-2.0, 0.0, -1.0], [2.0, 0.0, -1.2], [0.0, 2.5, -0.8],
                    [-0.5, 0.2, 0.5], [0.5, 0.2, 0.6], [0.0, 0.9, 0.4]], np.float32)
    idx = np.concatenate([np.tile(np.uint32([[3 * k, 3 * k + 1, 3 * k + 2]]), (n_each, 1)) for k in range(3)])
    return {"positions": pos, "normals": None, "indices": idx, "tri_material": (np.arange(len(idx)) % 2).astype(np.uint32)}


def set_scene_case(name):
    if name == "two clustered and a small":
        meshes = [big(8320), WI.torus(16, 8), big(16512)]
        return meshes, layout("two") + [(WI.transform(np.eye(3), [-1.0, 0.3, 0.4]), 1, 1), (WI.transform(0.7 * np.eye(3), [0.9, 1.1, -0.6]), 2, 0)]
    if name == "repeated":
        return [repeated(), WI.octahedron(0.3)], [(EYE, 0, 0), (WI.transform(np.eye(3), [0.0, 0.5, 1.5]), 1, 2)]
    return [big(int(name)), WI.octahedron(0.3)], beside()


@pytest.mark.parametrize("no_sah", [None, 1])
@pytest.mark.parametrize("name", ["8320", "16512", "40000", "two clustered and a small", "repeated"])
def test_batched_set_scene_writes_what_the_sequential_one_writes(capi, oracle, name, no_sah):
    meshes, inst = set_scene_case(name)
    cam, extra = world_view(oracle, meshes, inst)
    with Knob(RTGO_WHITTED_NO_SAH=no_sah, RTGO_WHITTED_SEQ_BUILD=None):
        batched = scene_ctx(capi, meshes, inst, WI.materials(), cam, extra)
    with Knob(RTGO_WHITTED_NO_SAH=no_sah, RTGO_WHITTED_SEQ_BUILD=1):
        sequential = scene_ctx(capi, meshes, inst, WI.materials(), cam, extra)
    try:
        what = "%s, no_sah=%r" % (name, no_sah)
        same_digests(batched, sequential, what)
        same_frames(frames(batched), frames(sequential), what)
        no_violations(A.check_instanced(batched.read_build(True), meshes, inst), what)
        if name == "repeated" and no_sah is None:
            with Knob(RTGO_WHITTED_NO_SAH=1):
                morton = scene_ctx(capi, meshes, inst, WI.materials(), cam, extra)
            try:
                a, b = batched.read_build(True)["mesh0.recs"], morton.read_build(True)["mesh0.recs"]
                print("repeated: records equal to the Morton records (a fallback everywhere):", a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)))
            finally:
                morton.close()
    finally:
        batched.close()
        sequential.close()


# ---- case 2: rebuild = fresh ----------------------------------------------------------------------------------------------------
def rebuilt_against_fresh(capi, oracle, meshes, inst, updates, what, mats=None, textures=None, prepare=None):
    """the scene (meshes, inst) after rebuild_meshes(updates) against a fresh context over the updated meshes: digests, frames with the
    top level in LDS and through L2, the structure's closure.  prepare(ctx): run on the first context before the rebuild."""
    mats = WI.materials() if mats is None else mats
    new = moved(meshes, updates)
    cam, extra = world_view(oracle, new, inst)
    extra["textures"] = textures
    ctx = scene_ctx(capi, meshes, inst, mats, cam, extra)
    fresh = None
    try:
        if prepare is not None:
            prepare(ctx)
        ctx.whitted_rebuild_meshes(updates)
        fresh = scene_ctx(capi, new, inst, mats, cam, extra)
        same_digests(ctx, fresh, what)
        same_pixels(ctx, fresh, extra["miss"], what)
        no_violations(A.check_instanced(ctx.read_build(True), new, inst), what)
    finally:
        ctx.close()
        if fresh is not None:
            fresh.close()


@pytest.mark.parametrize("n_tri,deform", [(8320, "sine"), (8320, "flat"), (8320, "permuted"), (16512, "sine"), (16512, "permuted")])
def test_a_rebuilt_clustered_mesh_is_the_fresh_build(capi, oracle, n_tri, deform):
    mesh = big(n_tri)
    new = DEFORM[deform](mesh)
    rebuilt_against_fresh(capi, oracle, [mesh, WI.octahedron(0.3)], beside(new), [(0, new, None)], "%d triangles, %s" % (n_tri, deform))


def test_unchanged_vertices_give_the_digests_from_before(capi):
    mesh = big(16512)
    ctx = capi.Context(0)
    try:
        ctx.whitted_set_scene([mesh, WI.octahedron(0.3)], beside(), WI.materials())
        before = list(ctx.build_digest(True))
        ctx.whitted_rebuild_meshes([(0, mesh["positions"], None)])
        assert list(ctx.build_digest(True)) == before
        ctx.whitted_rebuild_meshes([(1, WI.octahedron(0.3)["positions"], None), (0, mesh["positions"], mesh["normals"])])
        assert list(ctx.build_digest(True)) == before
        assert ctx._lib.rtgo_whitted_rebuild_meshes(ctx._h, None, 0) == 0
        ctx.whitted_rebuild_meshes([])
        assert list(ctx.build_digest(True)) == before
    finally:
        ctx.close()


# ---- case 3: it really builds ---------------------------------------------------------------------------------------------------
def test_a_refit_keeps_the_old_tree_and_a_rebuild_replaces_it(capi, oracle):
    mesh = big(8320)
    new = DEFORM["permuted"](mesh)
    meshes, inst = [mesh, WI.octahedron(0.3)], beside(new)
    cam, extra = world_view(oracle, moved(meshes, [(0, new, None)]), inst)
    ctx = scene_ctx(capi, meshes, inst, WI.materials(), cam, extra)
    fresh = scene_ctx(capi, moved(meshes, [(0, new, None)]), inst, WI.materials(), cam, extra)
    try:
        ctx.whitted_update_meshes([(0, new, None)])
        assert list(ctx.build_digest(True)) != list(fresh.build_digest(True)), "a refit over permuted vertices came out as the fresh build: the comparison shows nothing"
        same_frames(frames(ctx), frames(fresh), "refitted")
        ctx.whitted_rebuild_meshes([(0, new, None)])
        same_digests(ctx, fresh, "rebuilt after the refit")
        same_frames(frames(ctx), frames(fresh), "rebuilt after the refit")
    finally:
        ctx.close()
        fresh.close()


# ---- case 4: one call, several meshes, textures kept ----------------------------------------------------------------------------
def several():
    """a ground (not named), a small torus, the 8320-triangle mesh with texture coordinates, an octahedron (not named); material 4 textured"""
    rng = np.random.RandomState(5)
    torus = WI.torus(16, 8)
    meshes = [WI.ground(3.0, -0.4), torus, big(8320, texcoords=True), WI.octahedron(0.2)]
    mats = np.concatenate([WI.materials(), np.array([[1.0, 1.0, 1.0, 1.0, 0.0, 0.5]], np.float32)])
    inst = [(EYE, 0, 0), (WI.transform(WI.rotation(rng), [-1.1, 0.1, 0.2]), 1, 1), (WI.transform(np.eye(3), [0.3, 0.0, -0.3]), 2, 3),
            (WI.transform(WI.rotation(rng), [1.1, 0.2, 0.4]), 3, 2), (WI.transform(0.8 * WI.rotation(rng), [-0.4, 0.5, 0.9]), 3, 1)]
    p = torus["positions"].astype(np.float64)
    updates = [(2, sine(meshes[2], shift=np.float64([0.05, 0.1, -0.05])), None),
               (1, (p + 0.08 * np.sin(9.0 * p[:, [2, 0, 1]]) * torus["normals"] + [0.1, 0.1, -0.1]).astype(np.float32), torus["normals"])]
    return meshes, inst, mats, {4: (checker(), None, None)}, updates


def test_several_meshes_in_one_call_and_the_textures_stay(capi, oracle):
    meshes, inst, mats, textures, updates = several()
    kept = {}

    def prepare(ctx):
        kept.update({k: v.copy() for k, v in ctx.read_build(True).items() if k.startswith(("mesh0.", "mesh3."))})

    rebuilt_against_fresh(capi, oracle, meshes, inst, updates, "several meshes", mats=mats, textures=textures, prepare=prepare)
    new = moved(meshes, updates)
    cam, extra = world_view(oracle, new, inst)
    ctx = scene_ctx(capi, meshes, inst, mats, cam, dict(extra, textures=textures))
    bare = scene_ctx(capi, new, inst, mats, cam, extra)
    try:
        ctx.whitted_rebuild_meshes(updates)
        after = ctx.read_build(True)
        assert len(kept) >= 10
        for k, v in kept.items():
            assert v.shape == after[k].shape and np.array_equal(v.view(np.uint32), after[k].view(np.uint32)), "the spans of a mesh not named changed: " + k
        # ... and the textures show: the same scene without them differs
        assert not np.array_equal(frames(ctx)[1], frames(bare)[1]), "the textures do not show in this frame"
    finally:
        ctx.close()
        bare.close()


# ---- case 5: a scene of rtgo_whitted_set_mesh ------------------------------------------------------------------------------------
def mesh_ctx(capi, mesh, cam, positions=None):
    ctx = capi.Context(0)
    ctx.whitted_set_mesh(mesh["positions"] if positions is None else positions, mesh.get("normals"), mesh["indices"], mesh.get("tri_material"), mesh["materials"])
    if mesh.get("texcoords") is not None:
        ctx.whitted_set_texcoords(mesh["texcoords"])
    for mi, (bc, mr, nm) in (mesh.get("textures") or {}).items():
        ctx.whitted_set_material_textures(mi, bc, mr, nm)
    ctx.whitted_set_lights(mesh["lights"])
    ctx.whitted_set_miss_color(mesh["miss"])
    ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])
    ctx.resize(W * H)
    return ctx


@pytest.mark.parametrize("which", ["textured quads", "sphere, box and ground"])
def test_a_set_mesh_scene_takes_mesh_zero(capi, oracle, which):
    mesh = whitted_scene.textured_quad() if which == "textured quads" else whitted_scene.build()
    p = mesh["positions"].astype(np.float64)
    new = (p + 0.15 * np.sin(3.0 * p[:, [1, 2, 0]])).astype(np.float32)
    cam = whitted_scene.camera(oracle, W, H, eye=(0.3, 1.4, 5.0), lookat=(0.0, 0.9, -1.0)) if which == "textured quads" else whitted_scene.camera(oracle, W, H)
    ctx, fresh = mesh_ctx(capi, mesh, cam), mesh_ctx(capi, mesh, cam, positions=new)
    try:
        before = list(ctx.build_digest(True))
        ctx.whitted_rebuild_meshes([(0, mesh["positions"], None)])
        assert list(ctx.build_digest(True)) == before
        ctx.whitted_rebuild_meshes([(0, new, None)])
        same_digests(ctx, fresh, which)
        same_frames(frames(ctx), frames(fresh), which)   # (texture coordinates and textures of ctx were set before the rebuild, and never again)
        for bad in ([(1, new, None)], [(0, new, None), (0, new, None)], [(0, new[:-1], None)]):
            with pytest.raises(capi.RtgoError, match=E_INVALID):
                ctx.whitted_rebuild_meshes(bad)
            same_digests(ctx, fresh, which + ", after a refusal")
        # ... and a refit works on the rebuilt mesh as on the fresh one
        ctx.whitted_update_mesh(0, mesh["positions"])
        fresh.whitted_update_mesh(0, mesh["positions"])
        same_digests(ctx, fresh, which + ", refitted")
    finally:
        ctx.close()
        fresh.close()


# ---- case 6: afterwards ---------------------------------------------------------------------------------------------------------
def test_the_other_calls_work_afterwards_as_after_a_fresh_scene(capi, oracle):
    mesh, small = big(8320), WI.torus(16, 8)
    first, second = sine(mesh), DEFORM["permuted"](mesh)
    meshes, inst = [mesh, small], layout("two", first) + [(WI.transform(0.6 * np.eye(3), [-0.9, 0.4, 0.6]), 1, 2)]
    new = moved(meshes, [(0, first, None)])
    cam, extra = world_view(oracle, new, inst)
    ctx = scene_ctx(capi, meshes, inst, WI.materials(), cam, extra)
    fresh = scene_ctx(capi, new, inst, WI.materials(), cam, extra)
    try:
        ctx.whitted_rebuild_meshes([(0, first, None)])
        same_digests(ctx, fresh, "rebuilt")
        rng = np.random.RandomState(4)
        again = [(WI.transform(WI.rotation(rng) @ np.diag([1.0, 0.7 + 0.2 * k, 1.0]), np.asarray(tr)[:, 3] + [0.1 * k, 0.0, 0.1]), m, off) for k, (tr, m, off) in enumerate(inst)]
        bigger = small["positions"] * np.float32(1.2)
        steps = [("set_instances", lambda c: c.whitted_set_instances(again)),
                 ("update_mesh on the small mesh", lambda c: c.whitted_update_mesh(1, bigger)),
                 ("update_meshes on the rebuilt mesh", lambda c: c.whitted_update_meshes([(0, mesh["positions"] + np.float32(first.mean(axis=0)), None)])),
                 ("a second rebuild", lambda c: c.whitted_rebuild_meshes([(0, second + np.float32(first.mean(axis=0)), None), (1, small["positions"], None)]))]
        for what, step in steps:
            step(ctx)
            step(fresh)
            same_digests(ctx, fresh, what)
            same_frames(frames(ctx), frames(fresh), what)
        final = moved(new, [(0, second + np.float32(first.mean(axis=0)), None)])
        no_violations(A.check_instanced(ctx.read_build(True), final, again), "after every step")
        # the second rebuild against a scene set afresh with its vertices
        scratch = scene_ctx(capi, final, again, WI.materials(), cam, extra)
        try:
            same_digests(ctx, scratch, "the second rebuild against a fresh scene")
        finally:
            scratch.close()
    finally:
        ctx.close()
        fresh.close()


# ---- case 7: refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_as_it_was(capi, oracle):
    bigm, small, bare = big(8320), WI.torus(16, 8), WI.octahedron(0.3)
    inst = [(EYE, 0, 0), (WI.transform(np.eye(3), [0.5, 0.5, 0.0]), 1, 0), (WI.transform(np.eye(3), [-0.5, 0.5, 0.0]), 2, 0)]
    none = capi.Context(0)
    try:
        with pytest.raises(capi.RtgoError, match=E_STATE):
            none.whitted_rebuild_meshes([(0, bigm["positions"], None)])
    finally:
        none.close()
    cam, extra = world_view(oracle, [bigm, small, bare], inst)
    ctx = scene_ctx(capi, [bigm, small, bare], inst, WI.materials(), cam, extra)
    try:
        before, shown = list(ctx.build_digest(True)), frames(ctx)
        ok = [(0, sine(bigm), None), (1, small["positions"] * np.float32(1.1), None), (2, bare["positions"] * np.float32(2.0), None)]
        nan_last = bare["positions"].copy()
        nan_last[5, 2] = np.nan
        inf_big = bigm["positions"].copy()
        inf_big[77, 0] = np.inf
        nan_normal = bigm["normals"].copy()
        nan_normal[3, 1] = np.nan
        refused = {
            "a NaN in the last of three entries": ok[:2] + [(2, nan_last, None)],
            "an infinity in a clustered mesh": [(0, inf_big, None)],
            "a NaN among the normals": [(0, bigm["positions"], nan_normal)],
            "a mesh named twice": [ok[0], ok[1], (0, bigm["positions"], None)],
            "a mesh index beyond the scene's": ok[:2] + [(3, bare["positions"], None)],
            "a vertex count not the mesh's own": [ok[0], (1, small["positions"][:-1], None)],
            "normals for a mesh set without": [ok[0], (2, bare["positions"], np.ones_like(bare["positions"]))],
        }
        for what, updates in refused.items():
            with pytest.raises(capi.RtgoError, match=E_INVALID):
                ctx.whitted_rebuild_meshes(updates)
            assert list(ctx.build_digest(True)) == before, what
        # NULL updates with a count, NULL positions
        assert ctx._lib.rtgo_whitted_rebuild_meshes(ctx._h, None, 2) == 1
        arr = (capi.WhittedMeshUpdate * 1)(capi.WhittedMeshUpdate(1, None, None, len(small["positions"])))
        assert ctx._lib.rtgo_whitted_rebuild_meshes(ctx._h, arr, 1) == 1
        assert list(ctx.build_digest(True)) == before
        same_frames(frames(ctx), shown, "after the refusals")
        # a valid call still works
        ctx.whitted_rebuild_meshes(ok)
        assert list(ctx.build_digest(True)) != before
    finally:
        ctx.close()


def test_a_refusal_after_the_build_puts_the_meshes_back(capi, oracle):
    """a clustered mesh under an instance scaled by 1e30, positions x 1e10: its box is known only after its build, and that places the
    instance beyond the float range -- everything the build wrote comes back (vertices, normals, records, triangles, qrecs, tidx: the
    digests and the frame of its identity instance stay), also for a small mesh rebuilt by the same call"""
    bigm, small = big(8320), WI.octahedron(0.3)
    inst = [(EYE, 0, 0), (EYE, 1, 0), (WI.transform(np.diag([1e30, 1.0, 1.0]), [0, 1, 0]), 0, 0)]
    cam, extra = world_view(oracle, [bigm, small], inst[:2])
    ctx = scene_ctx(capi, [bigm, small], inst, WI.materials(), cam, extra)
    try:
        before, shown = list(ctx.build_digest(True)), frames(ctx)
        assert (shown[0][..., :3] != np.float32(extra["miss"])).any(axis=-1).mean() > 0.05
        far = DEFORM["permuted"](bigm) * np.float32(1e10)
        for updates in ([(0, far, None)], [(1, small["positions"] * np.float32(2.0), None), (0, far, -bigm["normals"])]):
            with pytest.raises(capi.RtgoError, match=E_INVALID):
                ctx.whitted_rebuild_meshes(updates)
            assert list(ctx.build_digest(True)) == before
            same_frames(frames(ctx), shown, "after a refusal")
        doubled = [dict(bigm, positions=bigm["positions"] * np.float32(2.0)), dict(small, positions=small["positions"] * np.float32(2.0))]
        ctx.whitted_rebuild_meshes([(1, doubled[1]["positions"], None), (0, doubled[0]["positions"], None)])
        assert list(ctx.build_digest(True)) != before
        no_violations(A.check_instanced(ctx.read_build(True), doubled, inst), "after the refusals")
    finally:
        ctx.close()
