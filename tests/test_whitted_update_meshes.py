"""rtgo_whitted_update_meshes on the MI355X: clustered meshes (beyond RTGO_MAX_TRIANGLES) refitted to moved vertices, and several meshes
moved by one call, against the same scene set afresh with the new vertices.

Any tree whose boxes contain its triangles returns the same closest hit (smallest t, then lowest index), so a refitted scene renders bit
for bit like a freshly built one: every comparison here is an equality, none has a tolerance.  Over unchanged vertices the refit
reproduces the build's own arrays, so there the build digests are equal span for span.

The meshes are the smallest that reach each branch: displaced_torus(65, 64), 8320 triangles, three clusters under a mid level of one leaf
(no records); (129, 64), 16 512 triangles, five clusters, the first mid level with records; (200, 100), 40 000 triangles, ten clusters."""
import numpy as np
import pytest

import accel_check as A
import trace_rays_ref as R
import whitted_big_meshes as BM
import whitted_instances as WI
import whitted_scene
from test_trace_rays import Knob

pytestmark = pytest.mark.gpu

W, H = 64, 48
SHIFT = np.float64([37.0, -5.0, 11.0])
TMIN, TMAX = np.float32(0.01), np.float32(1e16)
MODES = (2, 0)   # the top level in LDS, and read through L2
E_INVALID, E_STATE, E_UNSUPPORTED = r"\(1\)", r"\(3\)", r"\(4\)"
EYE = np.eye(3, 4, dtype=np.float32)
SHAPES = {8320: (65, 64), 16512: (129, 64), 40000: (200, 100)}
_cache = {}


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import capi as m
    m.load()
    return m


def big(n_tri, texcoords=False):
    key = (n_tri, texcoords)
    if key not in _cache:
        _cache[key] = BM.displaced_torus(*SHAPES[n_tri], texcoords=texcoords)
        assert len(_cache[key]["indices"]) == n_tri
    return _cache[key]


# ---- deformations ---------------------------------------------------------------------------------------------------------------
def sine(mesh, shift=SHIFT):
    """a sine displacement along the normals, 3 % of the mesh's extent, and a translation: bounds, pads and 16-bit grids all move"""
    p = mesh["positions"].astype(np.float64)
    n = mesh["normals"].astype(np.float64) if mesh.get("normals") is not None else np.tile([0.0, 1.0, 0.0], (len(p), 1))
    ext = (p.max(axis=0) - p.min(axis=0)).max()
    d = 0.03 * ext * np.sin(9.0 * p[:, 0] + 7.0 * p[:, 2] + 5.0 * p[:, 1])
    return (p + d[:, None] * n + shift).astype(np.float32)


def flat(mesh):
    """all y = 0: no extent on an axis, coincident triangles (the tube's two sheets) -- the lowest index wins the ties in either tree"""
    p = mesh["positions"].copy()
    p[:, 1] = 0.0
    return p


def permuted(mesh):
    """the vertex positions permuted at random: the kept order means nothing any more and the boxes overlap everywhere"""
    return mesh["positions"][np.random.RandomState(11).permutation(len(mesh["positions"]))]


DEFORM = {"sine": sine, "flat": flat, "permuted": permuted}


def layout(name, positions=None):
    """the instances of mesh 0: one identity instance, or two under a rotation and a non-uniform scale, each placing the centre of
    `positions` (the origin without) where its translation says -- both stay in one frame wherever the vertices went"""
    if name == "one":
        return [(EYE, 0, 0)]
    rng = np.random.RandomState(9)
    c = np.zeros(3) if positions is None else 0.5 * (positions.astype(np.float64).min(axis=0) + positions.astype(np.float64).max(axis=0))
    A = [WI.rotation(rng) @ np.diag([1.6, 0.5, 1.0]), WI.rotation(rng) @ np.diag([0.7, 1.8, 1.2])]
    return [(WI.transform(A[0], [0.2, 1.0, -0.5] - A[0] @ c), 0, 0), (WI.transform(A[1], [1.8, 1.2, 0.8] - A[1] @ c), 0, 1)]


# ---- contexts and comparisons --------------------------------------------------------------------------------------------------
def world_view(oracle, meshes, inst):
    """a camera and the two lights placed by the world bounds of the instanced vertices: (cam, extra)"""
    pts = []
    for tr, m, _ in inst:
        p = meshes[int(m)]["positions"].astype(np.float64)
        box = np.array([[x, y, z] for x in (p[:, 0].min(), p[:, 0].max()) for y in (p[:, 1].min(), p[:, 1].max()) for z in (p[:, 2].min(), p[:, 2].max())])
        t = np.asarray(tr, np.float64).reshape(3, 4)
        pts.append(box @ t[:, :3].T + t[:, 3])
    pts = np.concatenate(pts)
    centre, ext = 0.5 * (pts.min(axis=0) + pts.max(axis=0)), (pts.max(axis=0) - pts.min(axis=0)).max()
    eye = centre + ext * np.array([0.25, 0.75, 1.1])
    cam = whitted_scene.camera(oracle, W, H, eye=tuple(np.float32(eye)), lookat=tuple(np.float32(centre)))
    extra = WI.lights()
    extra["lights"][:, 4:7] += np.float32(centre)
    return cam, extra


def scene_ctx(capi, meshes, inst, mats, cam, extra):
    ctx = capi.Context(0)
    ctx.whitted_set_scene(meshes, inst, mats)
    for mi, (bc, mr, nm) in (extra.get("textures") or {}).items():
        ctx.whitted_set_material_textures(mi, bc, mr, nm)
    ctx.whitted_set_lights(extra["lights"])
    ctx.whitted_set_miss_color(extra["miss"])
    ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])
    ctx.resize(W * H)
    return ctx


def frames(ctx):
    """subframes 0 and 1: accumulation buffer, image, (rays_total, rays_occlusion)"""
    ctx.reset_stats()
    for sf in range(2):
        ctx.whitted_launch(W, H, sf)
    ctx.sync()
    st = ctx.stats()
    return ctx.read_accum(H, W), ctx.read_image(H, W), (st["rays_total"], st["rays_occlusion"])


def same_frames(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), what + ": accumulation differs in %d pixels" % (
        (a[0].view(np.uint32) != b[0].view(np.uint32)).any(axis=-1).sum())
    assert np.array_equal(a[1], b[1]), what + ": image differs"
    assert a[2] == b[2], what + ": ray counts differ %r %r" % (a[2], b[2])


def same_pixels(refit, fresh, miss, what):
    for mode in MODES:
        with Knob(RTGO_WHITTED_MODE=mode):
            a, b = frames(refit), frames(fresh)
        same_frames(a, b, "%s, RTGO_WHITTED_MODE=%d" % (what, mode))
        hit = (b[0][..., :3] != np.float32(miss)).any(axis=-1).mean()
        assert hit > 0.05 and b[2][1] > 0, (what, "the frame shows too little of the scene", hit, b[2])


def same_rays(capi, refit, fresh, cam, what):
    o, d = R.primaries(cam, W, H)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    a, b = refit.whitted_trace_rays(rays), fresh.whitted_trace_rays(rays)
    for f in ("t", "prim", "instance", "u", "v", "n"):
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), (what, "closest hits differ in", f)
    assert (b["prim"] >= 0).mean() > 0.05, what
    x, y = refit.whitted_trace_rays(rays, capi.TRACE_ANY_HIT), fresh.whitted_trace_rays(rays, capi.TRACE_ANY_HIT)
    assert np.array_equal(x["prim"] >= 0, y["prim"] >= 0) and np.array_equal(x["prim"] >= 0, b["prim"] >= 0), (what, "any-hit mask")


def no_violations(v, what):
    assert len(v) == 0, "%s: %d violations, first: %s" % (what, len(v), list(v)[:5])


def refit_against_fresh(capi, oracle, meshes, inst, updates, what, mats=None, textures=None):
    """the scene (meshes, inst) after update_meshes(updates) against a fresh context over the updated meshes; returns the new meshes"""
    mats = WI.materials() if mats is None else mats
    new = list(meshes)
    for k, pos, nrm in updates:
        new[k] = dict(new[k], positions=np.ascontiguousarray(pos, np.float32))
        if nrm is not None:
            new[k]["normals"] = nrm
    cam, extra = world_view(oracle, new, inst)
    extra["textures"] = textures
    refit = scene_ctx(capi, meshes, inst, mats, cam, extra)
    fresh = None
    try:
        refit.whitted_update_meshes(updates)
        fresh = scene_ctx(capi, new, inst, mats, cam, extra)
        same_pixels(refit, fresh, extra["miss"], what)
        same_rays(capi, refit, fresh, cam, what)
        no_violations(A.check_instanced(refit.read_build(True), new, inst), what)
    finally:
        refit.close()
        if fresh is not None:
            fresh.close()
    return new


# ---- case 1: identity, there and back ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tri", list(SHAPES))
def test_unchanged_vertices_reproduce_the_build_bit_for_bit(capi, n_tri):
    mesh = big(n_tri)
    ctx = capi.Context(0)
    try:
        ctx.whitted_set_scene([mesh], layout("two"), WI.materials())
        info = A.mesh_info(ctx.read_build(True)["mesh0.info"])
        ncl = -(-n_tri // 4096)
        assert info["clustered"] == 1 and info["n_built"] == ncl + 1
        assert (info["built"][ncl]["n_recs"] > 0) == (n_tri > 16384), "the mid level has records from five clusters on"
        before = list(ctx.build_digest(True))
        ctx.whitted_update_meshes([(0, mesh["positions"], None)])
        assert list(ctx.build_digest(True)) == before
        ctx.whitted_update_meshes([(0, mesh["positions"], mesh["normals"])])
        assert list(ctx.build_digest(True)) == before
        # there and back
        ctx.whitted_update_meshes([(0, sine(mesh), None)])
        assert list(ctx.build_digest(True)) != before
        ctx.whitted_update_meshes([(0, mesh["positions"], None)])
        assert list(ctx.build_digest(True)) == before
    finally:
        ctx.close()


# ---- case 2: deformations -------------------------------------------------------------------------------------------------------
CASES = [(n, d, l) for n in SHAPES for d in ("sine", "flat") for l in ("one", "two")] + [(8320, "permuted", l) for l in ("one", "two")]


@pytest.mark.parametrize("n_tri,deform,instances", CASES)
def test_deformed_clustered_mesh_renders_like_a_fresh_build(capi, oracle, n_tri, deform, instances):
    mesh = big(n_tri)
    moved = DEFORM[deform](mesh)
    refit_against_fresh(capi, oracle, [mesh], layout(instances, moved), [(0, moved, None)], "%d triangles, %s, %s" % (n_tri, deform, instances))


# ---- case 3: normals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["new", "kept"])
def test_new_normals_and_kept_normals(capi, oracle, which):
    mesh = big(8320)
    n = mesh["normals"].astype(np.float64) + 0.3 * np.sin(5.0 * mesh["positions"].astype(np.float64)[:, [1, 2, 0]])
    new_normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    assert not np.array_equal(new_normals, mesh["normals"])
    new = refit_against_fresh(capi, oracle, [mesh], layout("one"), [(0, sine(mesh), new_normals if which == "new" else None)], which + " normals")
    assert np.array_equal(new[0]["normals"], new_normals if which == "new" else mesh["normals"])


# ---- case 4: the mixed scene of test_whitted_clustered -------------------------------------------------------------------------
def checker(n=8):
    t = np.zeros((n, n, 4), np.uint8)
    t[..., 3] = 255
    on = (np.arange(n)[:, None] + np.arange(n)[None, :]) % 2 == 0
    t[on] = [250, 240, 200, 255]
    t[~on] = [60, 120, 200, 255]
    return t


def mixed_scene():
    """small meshes (a torus with normals, octahedra, a ground) and the 40 000-triangle mesh with texture coordinates, material 4 textured"""
    rng = np.random.RandomState(5)
    meshes = [WI.ground(3.0, -0.4), WI.torus(), big(40000, texcoords=True), WI.octahedron(0.2)]
    mats = np.concatenate([WI.materials(), np.array([[1.0, 1.0, 1.0, 1.0, 0.0, 0.5]], np.float32)])
    inst = [(EYE, 0, 0), (WI.transform(WI.rotation(rng), [-1.1, 0.1, 0.2]), 1, 1), (WI.transform(np.eye(3), [0.3, 0.0, -0.3]), 2, 3),
            (WI.transform(WI.rotation(rng), [1.1, 0.2, 0.4]), 3, 2), (WI.transform(0.8 * WI.rotation(rng), [-0.4, 0.5, 0.9]), 3, 1)]
    return meshes, inst, mats, {4: (checker(), None, None)}


def test_mixed_scene_keeps_its_textures(capi, oracle):
    meshes, inst, mats, textures = mixed_scene()
    moved = sine(meshes[2], shift=np.float64([0.05, 0.1, -0.05]))
    new = refit_against_fresh(capi, oracle, meshes, inst, [(2, moved, None)], "mixed scene", mats=mats, textures=textures)
    # ... and they show: the same scene without them differs
    cam, extra = world_view(oracle, new, inst)
    refit = scene_ctx(capi, meshes, inst, mats, cam, dict(extra, textures=textures))
    bare = scene_ctx(capi, new, inst, mats, cam, extra)
    try:
        refit.whitted_update_meshes([(2, moved, None)])
        assert not np.array_equal(frames(refit)[1], frames(bare)[1]), "the textures do not show in this frame"
    finally:
        refit.close()
        bare.close()


# ---- case 5: batches ------------------------------------------------------------------------------------------------------------
def batch_scene():
    rng = np.random.RandomState(21)
    torus = WI.torus(16, 8)
    meshes = [WI.ground(3.0, -0.4, normals=True), torus, big(8320), WI.octahedron(0.3)]
    inst = [(EYE, 0, 0), (WI.transform(WI.rotation(rng), [-1.2, 0.3, 0.2]), 1, 1), (WI.transform(np.eye(3), [0.2, 0.1, -0.2]), 2, 2),
            (WI.transform(WI.rotation(rng) @ np.diag([1.0, 0.6, 1.3]), [1.2, 0.3, 0.5]), 3, 0), (WI.transform(0.7 * WI.rotation(rng), [-0.3, 0.9, 0.8]), 1, 0)]
    p = torus["positions"].astype(np.float64)
    updates = [(3, meshes[3]["positions"] * np.float32(1.5), None),
               (2, sine(meshes[2], shift=np.float64([0.1, 0.05, -0.1])), None),
               (1, (p + 0.08 * np.sin(9.0 * p[:, [2, 0, 1]]) * torus["normals"] + [0.1, 0.1, -0.1]).astype(np.float32), torus["normals"])]
    return meshes, inst, updates


def test_three_meshes_in_one_call(capi, oracle):
    meshes, inst, updates = batch_scene()
    new = refit_against_fresh(capi, oracle, meshes, inst, updates, "a batch of three")
    rng = np.random.RandomState(4)
    moved = [(WI.transform(WI.rotation(rng) @ np.diag([1.0, 0.7 + 0.2 * k, 1.0]), [0.8 * k - 1.6, 0.4, 0.3 * k]), m, off) for k, (_, m, off) in enumerate(inst)]
    moved[0] = inst[0]
    mats = WI.materials()
    cam, extra = world_view(oracle, new, moved)
    batch, single, fresh = (scene_ctx(capi, ms, inst, mats, cam, extra) for ms in (meshes, meshes, new))
    try:
        batch.whitted_update_meshes(updates)
        # the small meshes one by one: the arrays and the top level come out the same
        single.whitted_update_meshes([updates[1]])
        for k, pos, nrm in (updates[0], updates[2]):
            single.whitted_update_mesh(k, pos, nrm)
        assert list(batch.build_digest(True)) == list(single.build_digest(True))
        # the new boxes reached the host's tables: the next top level is built from them
        batch.whitted_set_instances(moved)
        fresh.whitted_set_instances(moved)
        same_pixels(batch, fresh, extra["miss"], "a batch, then set_instances")
        no_violations(A.check_instanced(batch.read_build(True), new, moved), "a batch, then set_instances")
        # ... and further updates work: back to the first vertices, in two calls
        batch.whitted_update_meshes([(k, meshes[k]["positions"], meshes[k].get("normals")) for k in (1, 2)])
        batch.whitted_update_mesh(3, meshes[3]["positions"])
        single.whitted_set_instances(moved)
        single.whitted_update_meshes([(k, meshes[k]["positions"], meshes[k].get("normals")) for k in (3, 2, 1)])
        assert list(batch.build_digest(True)) == list(single.build_digest(True))
    finally:
        for c in (batch, single, fresh):
            c.close()


def test_a_set_mesh_scene_takes_mesh_zero(capi):
    mesh = whitted_scene.build()
    p = mesh["positions"].astype(np.float64)
    moved = (p + 0.1 * np.sin(3.0 * p[:, [1, 2, 0]])).astype(np.float32)
    a, b = capi.Context(0), capi.Context(0)
    try:
        for ctx in (a, b):
            ctx.whitted_set_mesh(mesh["positions"], mesh["normals"], mesh["indices"], mesh["tri_material"], mesh["materials"])
        before = list(a.build_digest(True))
        a.whitted_update_meshes([(0, moved, None)])
        b.whitted_update_mesh(0, moved)
        assert list(a.build_digest(True)) == list(b.build_digest(True)) != before
        for bad in ([(1, moved, None)], [(0, moved, None), (0, moved, None)]):
            with pytest.raises(capi.RtgoError, match=E_INVALID):
                a.whitted_update_meshes(bad)
            assert list(a.build_digest(True)) == list(b.build_digest(True))
    finally:
        a.close()
        b.close()


# ---- case 6: refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_as_it_was(capi):
    bigm, small, bare = big(8320), WI.torus(16, 8), WI.octahedron(0.3)
    inst = [(EYE, 0, 0), (WI.transform(np.eye(3), [0.5, 0.5, 0.0]), 1, 0), (WI.transform(np.eye(3), [-0.5, 0.5, 0.0]), 2, 0)]
    ctx = capi.Context(0)
    try:
        with pytest.raises(capi.RtgoError, match=E_STATE):
            ctx.whitted_update_meshes([(0, bigm["positions"], None)])
        ctx.whitted_set_scene([bigm, small, bare], inst, WI.materials())
        before = list(ctx.build_digest(True))
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
                ctx.whitted_update_meshes(updates)
            assert list(ctx.build_digest(True)) == before, what
        # NULL updates with a count, NULL positions; no entries at all is a success that changes nothing
        assert ctx._lib.rtgo_whitted_update_meshes(ctx._h, None, 2) == 1
        arr = (capi.WhittedMeshUpdate * 1)(capi.WhittedMeshUpdate(1, None, None, len(small["positions"])))
        assert ctx._lib.rtgo_whitted_update_meshes(ctx._h, arr, 1) == 1
        assert ctx._lib.rtgo_whitted_update_meshes(ctx._h, None, 0) == 0
        ctx.whitted_update_meshes([])
        assert list(ctx.build_digest(True)) == before
        # a valid call still works
        ctx.whitted_update_meshes(ok)
        assert list(ctx.build_digest(True)) != before
    finally:
        ctx.close()


def test_a_refusal_after_the_clustered_refit_puts_the_mesh_back(capi, oracle):
    """a clustered mesh under an instance scaled by 1e30, positions x 1e10: its box is known only after its refit, and that places the
    instance beyond the float range -- the saved arrays come back (records, triangles, vertices and normals: the digests and the frame
    of its identity instance stay), also when a small mesh precedes it in the batch"""
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
                ctx.whitted_update_meshes(updates)
            assert list(ctx.build_digest(True)) == before
            same_frames(frames(ctx), shown, "after a refusal")
        doubled = [dict(bigm, positions=bigm["positions"] * np.float32(2.0)), dict(small, positions=small["positions"] * np.float32(2.0))]
        ctx.whitted_update_meshes([(1, doubled[1]["positions"], None), (0, doubled[0]["positions"], None)])
        assert list(ctx.build_digest(True)) != before
        no_violations(A.check_instanced(ctx.read_build(True), doubled, inst), "after the refusals")
    finally:
        ctx.close()
