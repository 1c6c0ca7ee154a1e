"""What the triangle path builds on the device, held to the reference build of tests/whitted_build_ref.py: each test sets a scene, reads
the structures back (capi.Context.read_build) and compares -- no frame is rendered.  tests/test_build_closure.py proves that every
structure is A valid tree over the triangles; these prove it is THE tree DESIGN.md 3.4 describes.

Held exactly, per structure (one mesh, a mesh of a batched call, a cluster, a mid level): the Morton order, the hierarchy's depth, the
leaves, the Morton records' topology, every record's child boxes, walk_depth.  Held to the derived cost bound
(whitted_build_ref.COST_MARGIN): the surface-area records' splits.  A clustered mesh's global sort is held exactly through the cut:
cluster c holds the triangles g[s:e] of the reference order g over the whole mesh, in the order of its own build over them.

Which records a structure must carry is the host's rule, asserted here: RTGO_WHITTED_NO_SAH or more than
whitted_build_ref.SAH_MAX_TRIANGLES triangles -> the Morton records; otherwise surface-area records, unless that tree came out deeper
than the walk's stack (kMaxWalkDepth) and the build went back to the Morton records.  The device does not keep the tree it dropped, so
that exception is accepted only where it can happen at all -- on inputs whose sweeps tie (`ties` below), with more units than a chain of
kMaxWalkDepth records holds -- and only when the records then ARE the Morton records, walk_depth included; it is printed.

NOT held: the top level's key order.  The float32 instance boxes its build sorts are not among the spans rtgo_debug_read_build returns
(test_read_build_returns_the_bytes_the_digest_hashes pins that list), so the top level gets the surface-area checks (b) to (d) only,
over units read from its own leaf children; the closure tests tie those boxes to the instances."""
import numpy as np
import pytest

import accel_check as A
import whitted_build_ref as R
from test_build_closure import MATERIALS, _mesh_cases, bumpy_sheet, first_triangles

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import capi as m
    m.load()
    return m


def clean(v, what):
    if v:
        print("%s: %d violations listed (%s)" % (what, len(v), ", ".join(A.tags(v))))
        for line in v[:10]:
            print("   ", line)
    assert not v, "%s: %s" % (what, list(v)[:3])


# ---------------------------------------------------------------------------------------------------------------- one structure
def hold(what, positions, indices, got_order, recs, meta, morton, ties=False, want_order=None):
    """one build over (positions, indices) against the reference: got_order = the items at its sorted positions (or the float4 rows of its
    sorted triangles), recs / meta = its records and WhittedBuildMeta, morton = the host's rule says Morton records.  want_order: what
    got_order must equal when it is not the reference order itself (a cluster: the mesh's own triangle numbers).  Returns violations."""
    ref = R.Reference(positions, indices)
    out = R.check_order(got_order, ref.order if want_order is None else np.asarray(want_order)[ref.order])
    R.check_depth(meta["depth"], ref.depth, out)
    n_recs = meta["n_recs"]
    if morton:
        v = R.check_morton_records(recs, n_recs, ref, ref.boxes, meta["walk_depth"] if n_recs else None)
    else:
        v = R.check_sah_records(recs, n_recs, ref.runs, ref.boxes, meta["walk_depth"] if n_recs else None)
        if v and ties and len(ref.runs) - 1 > A.MAX_WALK_DEPTH:
            m = R.check_morton_records(recs, n_recs, ref, ref.boxes, meta["walk_depth"])
            if not m:
                print("%s: the Morton records over %d units (walk_depth %d): the surface-area tree was dropped" % (what, len(ref.runs), meta["walk_depth"]))
                v = m
    R.report(what, v)
    out += v
    return out


def sah_rule(n, no_sah=False):
    return no_sah or n > R.SAH_MAX_TRIANGLES


def test_the_rule_is_the_hosts():
    """whitted_sah_lds(n) = 33 n + 16 <= 150 KiB"""
    assert R.SAH_MAX_TRIANGLES == 4654 and 33 * 4654 + 16 <= 150 * 1024 < 33 * 4655 + 16


# ---------------------------------------------------------------------------------------------------------------- one mesh
def unused_far_vertices():
    """a sheet and six vertices no triangle names, far outside it: keys and pad must not see them"""
    m = bumpy_sheet(301)
    far = np.array([[1e3, 0, 0], [-1e3, 0, 0], [0, 2e3, 0], [0, -2e3, 0], [0, 0, 3e3], [0.5, 0.5, -3e3]], np.float32)
    return dict(m, positions=np.concatenate([far[:3], m["positions"], far[3:]]), indices=(m["indices"] + 3).astype(np.uint32))


def point_at_the_upper_corner():
    """the last triangle is one point at the bounds' upper corner: its centroid is the corner, cell 1023 on every axis"""
    m = bumpy_sheet(203)
    used = m["positions"][np.unique(m["indices"])]
    v = len(m["positions"])
    return dict(m, positions=np.concatenate([m["positions"], used.max(axis=0)[None, :]]).astype(np.float32),
                indices=np.concatenate([m["indices"], [[v, v, v]]]).astype(np.uint32))


def one_centroid(n=64):
    """n triangles of many sizes around one centroid (a, b, -a - b about c): every code is the same, so order and hierarchy come from the
    index alone; the bounds are lopsided, so c is no cell boundary"""
    rng = np.random.RandomState(7)
    c = np.array([0.1, 0.2, 0.3])
    a, b = rng.uniform(-1, 1, (n, 3)) * rng.uniform(0.05, 1.0, (n, 1)), rng.uniform(-1, 1, (n, 3)) * rng.uniform(0.05, 1.0, (n, 1))
    pos = np.stack([c + a, c + b, c - a - b], axis=1).reshape(-1, 3).astype(np.float32)
    return {"positions": pos, "normals": None, "indices": np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)}


def test_the_one_centroid_mesh_has_one_code():
    m = one_centroid()
    order, codes = R.morton_order(m["positions"], m["indices"])
    assert len(set(codes.tolist())) == 1 and order.tolist() == list(range(64))


NEW_CASES = [("4654 triangles", lambda: bumpy_sheet(4654), False), ("4655 triangles", lambda: bumpy_sheet(4655), False),
             ("unused far vertices", unused_far_vertices, False), ("a point at the upper corner", point_at_the_upper_corner, False),
             ("64 triangles, one centroid", one_centroid, True)]
TIES = {"coincident"}   # of test_build_closure's cases: the sweeps of 200 copies of one triangle tie at every position


def mesh_cases():
    return [(what, make, what in TIES) for what, make in _mesh_cases()] + NEW_CASES


@pytest.mark.parametrize("no_sah", [False, True])
@pytest.mark.parametrize("case", range(16))
def test_one_mesh(capi, monkeypatch, case, no_sah):
    what, make, ties = mesh_cases()[case]
    mesh = make()
    if no_sah:
        monkeypatch.setenv("RTGO_WHITTED_NO_SAH", "1")
    else:
        monkeypatch.delenv("RTGO_WHITTED_NO_SAH", raising=False)
    ctx = capi.Context(0)
    try:
        ctx.whitted_set_mesh(mesh["positions"], mesh.get("normals"), mesh["indices"], None, MATERIALS)
        build = ctx.read_build(True)
    finally:
        ctx.close()
    n = len(np.asarray(mesh["indices"]).reshape(-1, 3))
    meta = A.whitted_meta(build["meta"])
    clean(hold("%s%s" % (what, ", NO_SAH" if no_sah else ""), mesh["positions"], mesh["indices"], build["tris"], build["recs"], meta, sah_rule(n, no_sah), ties), what)


def test_the_new_sizes_sit_either_side_of_the_rule():
    assert not sah_rule(4654) and sah_rule(4655) and [w for w, _, _ in mesh_cases()][:6] == ["%d triangles" % n for n in (1, 2, 4, 5, 8191, 8192)]


# ---------------------------------------------------------------------------------------------------------------- instanced scenes
def hold_scene(build, meshes, what, ties=()):
    """every structure of an instanced scene below the top level, mesh by mesh in object space, and the top level's records.  ties: the
    meshes whose sweeps tie.  (No RTGO_WHITTED_NO_SAH here: the rule is the size alone.)"""
    out = A._Out()
    clusters = np.asarray(build["clusters"], np.int32).reshape(-1, 4)
    for k, m in enumerate(meshes):
        tag = "mesh%d." % k
        info = A.mesh_info(build[tag + "info"])
        pos = np.asarray(m["positions"], np.float32).reshape(-1, 3)
        idx = np.asarray(m["indices"]).reshape(-1, 3).astype(np.int64)
        n = len(idx)
        recs_all = np.asarray(build[tag + "recs"], np.float32).reshape(-1, 4, 4)
        r_at = np.concatenate([[0], np.cumsum([b["n_recs"] for b in info["built"]])]).astype(int)   # (as check_instanced slices them)
        assert info["n_tris"] == n and info["clustered"] == (1 if n > A.MAX_TRIANGLES else 0), (what, k, info)
        if not info["clustered"]:
            b = info["built"][0]
            out += [tag + v for v in hold("%s mesh %d" % (what, k), pos, idx, build[tag + "tris"], recs_all[r_at[0]:r_at[1]], b["meta"], sah_rule(n), k in ties)]
            continue
        # a clustered mesh: the reference order over the whole mesh, cut at cluster_start; each cluster a build of its slice
        ncl = (n + A.CLUSTER_TRIS - 1) // A.CLUSTER_TRIS
        assert len(info["built"]) == ncl + 1, (what, k, info)
        g, _ = R.morton_order(pos, idx)
        which = R.triangle_at(build[tag + "tris"])
        starts = [A.cluster_start(n, ncl, c) for c in range(ncl + 1)]
        boxes = np.zeros((ncl, 2, 3), np.float32)
        for c in range(ncl):
            s, e = starts[c], starts[c + 1]
            b = info["built"][c]
            assert e - s <= A.CLUSTER_TRIS <= R.SAH_MAX_TRIANGLES and b["n_recs"] > 0
            rc = recs_all[r_at[c]:r_at[c + 1]]
            out += ["%sc%d.%s" % (tag, c, v) for v in hold("%s mesh %d cluster %d" % (what, k, c), pos, idx[g[s:e]], which[s:e], rc, b["meta"], False, k in ties,
                                                           want_order=g[s:e])]
            boxes[c, 0], boxes[c, 1] = np.minimum(rc[0, 0, 0:3], rc[0, 2, 0:3]), np.maximum(rc[0, 1, 0:3], rc[0, 3, 0:3])   # as big_cluster_boxes_kernel takes them
        # the mid level: item c is the degenerate triangle (lo, hi, lo) of cluster c's box; its order is the cluster table's
        tbase = (info["root"] - 1) >> 3
        by_rec = {info["built"][c]["rec0"]: c for c in range(ncl)}
        mid_order = np.array([by_rec.get(int(r), -1) for r in clusters[tbase:tbase + ncl, 0]], np.int64)
        mid = info["built"][ncl]
        mid_idx = np.array([[2 * c, 2 * c + 1, 2 * c] for c in range(ncl)], np.int64)
        out += [tag + "mid." + v for v in hold("%s mesh %d mid level" % (what, k), boxes.reshape(-1, 3), mid_idx, mid_order, recs_all[r_at[ncl]:r_at[ncl + 1]],
                                               mid["meta"], sah_rule(ncl))]
    # the top level: (b) to (d) over the units its own leaf children name
    top = np.ascontiguousarray(build["top.meta"]).view(np.int32)
    tmeta, n_top = A.whitted_meta(top[:9]), int(top[9])
    runs, ubox = R.units_of_records(build["top.recs"], n_top)
    assert n_top == 0 or sum(c for _, c in runs) == int(top[10]) <= R.SAH_MAX_TRIANGLES
    v = R.check_sah_records(build["top.recs"], n_top, runs, ubox, tmeta["walk_depth"] if n_top else None)
    R.report("%s top level" % what, v)
    out += ["top." + x for x in v]
    return out


def instanced(capi, what, meshes, instances, ties=()):
    import whitted_instances as WI
    ctx = capi.Context(0)
    try:
        ctx.whitted_set_scene(meshes, instances, WI.materials())
        build = ctx.read_build(True)
    finally:
        ctx.close()
    clean(hold_scene(build, meshes, what, ties), what)


def test_instanced_tori(capi):
    import whitted_instances as WI
    meshes, inst = WI.tori_scene()
    instanced(capi, "tori", meshes, inst)


def test_instanced_edges(capi):
    """test_build_closure's scene: meshes with records beside a mesh that is one leaf (three triangles, no records), six instances"""
    import whitted_instances as WI
    rng = np.random.RandomState(5)
    meshes = [WI.torus(16, 8), WI.octahedron(0.3), first_triangles(WI.octahedron(0.3), 3)]
    inst = [(WI.transform(WI.rotation(rng), [-1, 1, 0]), 0, 0), (WI.transform(0.6 * WI.rotation(rng), [0, 1, 0.5]), 1, 1),
            (WI.transform(WI.rotation(rng) @ np.diag([2.0, 0.4, 1.0]), [1, 0.5, 0]), 0, 1), (WI.transform(np.diag([1.5, 0.5, 1.0]), [2, 1, -1]), 2, 0),
            (WI.transform(WI.rotation(rng) @ np.diag([-0.7, 1.3, 0.9]), [0, 2, 1]), 1, 2), (WI.transform(np.eye(3), [300.0, -200.0, 100.0]), 0, 0)]
    instanced(capi, "edges", meshes, inst)
    instanced(capi, "edges, five", meshes, inst[:5])   # (kLeafTris instances and one more: the top level's first record)


@pytest.mark.parametrize("n", [8193, 16384, 16385, 40002])
def test_clustered_meshes(capi, n):
    """test_build_closure's sizes and meshes: two clusters, four full ones, the first fifth, ten (a mid level with records)"""
    import whitted_big_meshes as BM
    import whitted_instances as WI
    nu = {8193: 65, 16384: 128, 16385: 129, 40002: 200}[n]
    nv = {8193: 64, 16384: 64, 16385: 64, 40002: 101}[n]
    big = first_triangles(BM.displaced_torus(nu, nv), n)
    rng = np.random.RandomState(n)
    inst = [(WI.transform(np.eye(3), [0, 1, 0]), 0, 0), (WI.transform(WI.rotation(rng) @ np.diag([1.2, 0.7, 1.0]), [2, 1, 0]), 0, 1),
            (WI.transform(np.eye(3), [0, 2, 0]), 1, 0)]
    instanced(capi, "clustered %d" % n, [big, WI.octahedron(0.2)], inst)


def test_coincident_copies_across_clusters(capi):
    """test_whitted_clustered's mesh with 5000 copies of its last triangle appended: their keys differ in the index alone, so the
    stability of the global sort decides which cluster a copy lands in, and clusters made of copies tie in every sweep"""
    from test_whitted_clustered import EYE, _torus_and_ground
    mesh = _torus_and_ground(200, 100)
    dup = dict(mesh, indices=np.concatenate([mesh["indices"], np.tile(mesh["indices"][-1], (5000, 1))]),
               tri_material=np.concatenate([mesh["tri_material"], np.full(5000, 3, np.uint32)]))
    instanced(capi, "coincident copies", [dup], [(EYE, 0, 0)], ties={0})


# ---------------------------------------------------------------------------------------------------------------- after a rebuild
def test_rebuilt_meshes_are_the_reference_over_the_new_vertices(capi):
    """rtgo_whitted_rebuild_meshes of a small and a clustered mesh to displaced vertices: every structure is then the reference build
    over the NEW vertices.  (Refit, rebuild and their device twins are held to a fresh set call array for array by their own tests.)"""
    import whitted_instances as WI
    from test_whitted_update_meshes import big, sine
    meshes = [big(8320), WI.torus(16, 8)]
    inst = [(WI.transform(np.eye(3), [0, 1, 0]), 0, 0), (WI.transform(0.6 * np.eye(3), [-0.9, 0.4, 0.6]), 1, 2), (WI.transform(np.eye(3), [1.5, 0.4, 0.0]), 1, 1)]
    new = [sine(meshes[0]), sine(meshes[1], shift=np.array([0.05, -0.02, 0.03]))]
    assert not np.array_equal(R.morton_order(new[0], meshes[0]["indices"])[0], R.morton_order(meshes[0]["positions"], meshes[0]["indices"])[0])
    ctx = capi.Context(0)
    try:
        ctx.whitted_set_scene(meshes, inst, WI.materials())
        before = hold_scene(ctx.read_build(True), meshes, "before the rebuild")
        ctx.whitted_rebuild_meshes([(0, new[0], None), (1, new[1], None)])
        build = ctx.read_build(True)
    finally:
        ctx.close()
    clean(before, "before the rebuild")
    moved = [dict(m, positions=p) for m, p in zip(meshes, new)]
    clean(hold_scene(build, moved, "rebuilt"), "rebuilt")
    stale = A.tags(hold_scene(build, meshes, "rebuilt, against the old vertices"))   # (the comparison bites: the old order is gone)
    assert any(t.endswith("order.morton") for t in stale), stale
