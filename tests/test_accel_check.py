"""The validators of tests/accel_check.py bite: recorded structures (tests/golden/build_closure, written on an MI355X by make_fixtures.py
there) have no violation, and each mutation of a COPY of their arrays makes the validator it targets report the invariant it breaks.
Nothing here touches a device; mutated arrays never leave the host.

The grid, and the instanced / clustered structures, are too large to record; their mutation targets are numpy restatements
(accel_check.numpy_grid, toy_scene below): targets for the mutations only, never a reference for the device."""
import os

import numpy as np
import pytest

import accel_check as A

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_closure")


def i2f(v):
    return np.array([v], np.int32).view(np.float32)[0]


def inward(a, index, lower):
    """the fp32 plane a[index] moved in by one ulp (a lower plane up, an upper plane down)"""
    a[index] = np.nextafter(a[index], np.float32(np.inf if lower else -np.inf))


# ---------------------------------------------------------------------------------------------------------------- the analytic fixture
@pytest.fixture(scope="module")
def cornell():
    return A.load(os.path.join(GOLD, "cornell.npz"))


def fast_tree(build, inputs, k=0):
    """check_fast_tree's arguments for tree k of a recorded analytic build, as a dict of copies"""
    return dict(fnodes=build["tree%d.fnodes" % k].copy(), fprims=build["tree%d.fprims" % k].copy(), meta=A.build_meta(build["tree%d.meta" % k]),
                prims6=build["prims"].copy(), tight=build["tight"].copy(), aabb=build["aabb"].copy(), types=inputs["types"].copy(), M=inputs["M"].copy(),
                big_frac=A.BIG_FRAC[k], nodes=build["nodes"].copy())


def test_the_recorded_cornell_has_no_violation(cornell):
    build, inputs = cornell
    assert A.check_analytic(build, inputs["types"], inputs["M"]) == []
    a = fast_tree(build, inputs)
    # the fixture has what the mutations below need: a root over two certified six-record leaves, and a paired up-front list
    assert a["meta"]["n_fnodes"] == 3 and a["meta"]["n_small"] == 12 and a["meta"]["cuboid_leaves"] == 2 and a["meta"]["list_group"] == (3 | 2 << 8)
    assert A.build_meta(build["tree1.meta"])["n_small"] == 0 and len(build["tree1.fnodes"]) == 0


def _leaf_link(a, k, count=None, pairs=None, cub=None):
    fn = a["fnodes"].reshape(-1, 2, 4)
    v = -int(fn[k, 1, 3:4].view(np.int32)[0])
    c, p, q = v & 0xFFF, (v >> 12) & 0xFF, v >> 20
    c, p, q = (c if count is None else count), (p if pairs is None else pairs), (q if cub is None else cub)
    fn[k, 1, 3] = i2f(-(c | p << 12 | q << 20))


def _swap_records(a, i, j, rows=slice(0, 4)):
    fp = a["fprims"].reshape(-1, 4, 4)
    fp[[i, j], rows] = fp[[j, i], rows]


def _set(a, key, value):
    a["meta"][key] = value


FAST_TREE_MUTATIONS = {
    # (node 0 is the root, nodes 1 and 2 its leaves of records [0, 6) and [6, 12), records [12, 19) the up-front list)
    "containment.node: a root plane one ulp in": (lambda a: inward(a["fnodes"].reshape(-1, 2, 4), (0, 0, 1), True), {"containment.node"}),
    "containment.node: an upper root plane one ulp in": (lambda a: inward(a["fnodes"].reshape(-1, 2, 4), (0, 1, 2), False), {"containment.node"}),
    "containment.leaf: a leaf plane one ulp in": (lambda a: inward(a["fnodes"].reshape(-1, 2, 4), (1, 1, 0), False), {"containment.leaf"}),
    "containment.leaf: two records swapped across leaves": (lambda a: _swap_records(a, 0, 6), {"containment.leaf", "groups.opposite"}),
    "records.rows: two records' rows swapped, not their indices": (lambda a: _swap_records(a, 0, 6, slice(0, 3)), {"records.rows"}),
    "records.permutation: an SBT index twice": (lambda a: a["fprims"].reshape(-1, 4, 4).__setitem__((3, 3, 1), a["fprims"].reshape(-1, 4, 4)[4, 3, 1]), {"records.permutation"}),
    "records.type: a type word changed": (lambda a: a["fprims"].reshape(-1, 4, 4).__setitem__((3, 3, 0), i2f(A.DISK)), {"records.type"}),
    "shape.tile: a leaf count decremented": (lambda a: _leaf_link(a, 1, count=5), {"shape.tile"}),
    "shape.tile: a leaf count incremented": (lambda a: _leaf_link(a, 1, count=7), {"shape.tile"}),
    "shape.leaf_count: an empty leaf": (lambda a: _leaf_link(a, 2, count=0), {"shape.leaf_count", "shape.tile"}),
    "shape.reach: a link pointed at the sibling": (lambda a: a["fnodes"].reshape(-1, 2, 4).__setitem__((0, 0, 3), i2f(2)), {"shape.reach", "shape.tile"}),
    "shape.links: a link beyond the tree": (lambda a: a["fnodes"].reshape(-1, 2, 4).__setitem__((0, 1, 3), i2f(3)), {"shape.links", "shape.reach", "shape.tile"}),
    "shape.odd: an even node count": (lambda a: (_set(a, "n_fnodes", 2), a.__setitem__("fnodes", a["fnodes"][:4])), {"shape.odd", "shape.links", "shape.tile"}),
    "shape.big: the first big record counted into the tree": (lambda a: _set(a, "n_small", 13), {"shape.big", "shape.tile", "groups.opposite"}),
    "meta.walk_depth: one short": (lambda a: _set(a, "walk_depth", a["meta"]["walk_depth"] - 1), {"meta.walk_depth"}),
    "meta.cuboid_leaves: one more": (lambda a: _set(a, "cuboid_leaves", 3), {"meta.cuboid_leaves"}),
    "meta.tree_types: a type the tree does not hold": (lambda a: _set(a, "tree_types", 4 | 8), {"meta.tree_types"}),
    "meta.canonical_depth: one short": (lambda a: _set(a, "canonical_depth", a["meta"]["canonical_depth"] - 1), {"meta.canonical_depth"}),
    "groups.count: more pairs than records": (lambda a: _leaf_link(a, 1, pairs=4), {"groups.count"}),
    "groups.cuboid: a certificate over two pairs": (lambda a: _leaf_link(a, 1, pairs=2), {"groups.cuboid"}),
    "groups.opposite: neighbours of different pairs exchanged": (lambda a: _swap_records(a, 1, 2), {"groups.opposite"}),
    "groups.opposite: in the up-front list": (lambda a: _swap_records(a, 13, 14), {"groups.opposite"}),
    "groups.rectangles: a disk in a pair": (lambda a: (a["types"].__setitem__(int(a["fprims"].reshape(-1, 4, 4)[0, 3, 1:2].view(np.int32)[0]), A.DISK),
                                                       a["fprims"].reshape(-1, 4, 4).__setitem__((0, 3, 0), i2f(A.DISK))), {"groups.rectangles", "meta.tree_types"}),
}


@pytest.mark.parametrize("name", sorted(FAST_TREE_MUTATIONS))
def test_fast_tree_mutations(cornell, name):
    mutate, expect = FAST_TREE_MUTATIONS[name]
    a = fast_tree(*cornell)
    assert A.check_fast_tree(**a) == []
    mutate(a)
    got = set(A.tags(A.check_fast_tree(**a)))
    print(name, "->", sorted(got))
    assert name.split(":")[0] in got and got == expect, (name, got)


def test_tight_box_mutations(cornell):
    build, inputs = cornell
    meta = A.build_meta(build["tree0.meta"])
    types, M = inputs["types"], inputs["M"]
    assert A.check_tight(build["tight"], build["aabb"], types, M, meta) == []
    # a rectangle's box carries the reference's pad of 1e-3: moved in by twice that it no longer holds the rectangle
    t = build["tight"].copy()
    t[5, 0] += np.float32(2e-3)
    assert "tight.rectangle" in A.tags(A.check_tight(t, build["aabb"], types, M, meta))
    # the same box read as a disk's (radius 1 under M: wider than the rectangle's half extent on its long axes)
    ty = types.copy()
    ty[5] = A.DISK
    assert "tight.disk" in A.tags(A.check_tight(build["tight"], build["aabb"], ty, M, meta))
    # ... and as a sphere's, whose tight box is its reference box bit for bit
    ty[5] = A.SPHERE
    assert "tight.quadric" in A.tags(A.check_tight(build["tight"], build["aabb"], ty, M, meta))
    m2 = dict(meta, tight_bounds=meta["tight_bounds"].copy())
    inward(m2["tight_bounds"], 4, False)
    assert A.tags(A.check_tight(build["tight"], build["aabb"], types, M, m2)) == ["tight.bounds"]


# ---------------------------------------------------------------------------------------------------------------- the grid
@pytest.fixture(scope="module")
def lattice():
    """64 spheres of radius 0.6 on a 4 x 4 x 4 lattice of spacing 2, binned into 3 x 3 x 3 cells (numpy_grid): cells list several spheres"""
    c = np.stack(np.meshgrid(*[np.arange(4) * 2.0] * 3, indexing="ij"), -1).reshape(-1, 3)
    tight = np.concatenate([c - 0.6, c + 0.6], axis=1).astype(np.float32)
    fprims = np.zeros((64, 4, 4), np.float32)
    fprims[:, 3, 1] = np.arange(64, dtype=np.int32)[::-1].copy().view(np.float32)   # (record k holds primitive 63 - k)
    image, gp = A.numpy_grid(tight[::-1], (3, 3, 3))
    return image, gp, fprims, tight


def _grid_parts(img, gp):
    return A.grid_lists(img, gp)   # views into img


def _first_cell(img, gp, min_items=1):
    table, recs, items = _grid_parts(img, gp)
    for z, y, x in np.argwhere(table != 0):
        r = int(table[z, y, x]) - 1
        if int(recs[r, 3:4].view(np.uint32)[0]) >> 16 >= min_items:
            return (z, y, x), r
    raise AssertionError("no such cell")


def _recount(img, gp, r, delta):
    recs = _grid_parts(img, gp)[1]
    recs[r, 3:4].view(np.uint32)[0] += np.uint32(delta << 16) if delta > 0 else np.uint32(0)
    if delta < 0:
        recs[r, 3:4].view(np.uint32)[0] -= np.uint32((-delta) << 16)


def _grid_mutations():
    def border(img, gp):
        _grid_parts(img, gp)[0][0, 1, 1] = 1

    def record(img, gp):
        table, recs, _ = _grid_parts(img, gp)
        table[_first_cell(img, gp)[0]] = len(recs) + 1

    def items(img, gp):
        recs, it = _grid_parts(img, gp)[1:]
        recs[len(recs) - 1, 3:4].view(np.uint32)[0] = (len(it) - 1) | (3 << 16)

    def item_range(img, gp):
        recs, it = _grid_parts(img, gp)[1:]
        it[int(recs[0, 3:4].view(np.uint32)[0]) & 0xFFFF] = 64

    def item_repeat(img, gp):
        recs, it = _grid_parts(img, gp)[1:]
        r = _first_cell(img, gp, 2)[1]
        first = int(recs[r, 3:4].view(np.uint32)[0]) & 0xFFFF
        it[first + 1] = it[first]

    def deleted(img, gp):
        _recount(img, gp, _first_cell(img, gp, 2)[1], -1)

    def box(img, gp):
        recs = _grid_parts(img, gp)[1]
        recs[0, 0] = 0.5 * (recs[0, 0] + recs[0, 4])   # (the record's box carries the binning's pad: one ulp does not reach the shapes)

    return {"grid.border": (border, {"grid.border"}), "grid.record": (record, {"grid.record", "grid.complete"}), "grid.items": (items, {"grid.items", "grid.complete"}),
            "grid.item_range": (item_range, {"grid.item_range", "grid.complete"}), "grid.item_repeat": (item_repeat, {"grid.item_repeat", "grid.complete"}),
            "grid.complete": (deleted, {"grid.complete"}), "grid.box": (box, {"grid.box"})}


@pytest.mark.parametrize("name", sorted(_grid_mutations()))
def test_grid_mutations(lattice, name):
    image, gp, fprims, tight = lattice
    assert A.check_grid(image, gp, fprims, tight, 64) == []
    assert gp["entries"] > 64   # (spheres straddle cell walls: the lists are not trivial)
    mutate, expect = _grid_mutations()[name]
    img = image.copy()
    mutate(img, gp)
    got = set(A.tags(A.check_grid(img, gp, fprims, tight, 64)))
    print(name, "->", sorted(got))
    assert got == expect, (name, got)


def test_grid_layout_is_checked_first(lattice):
    image, gp, fprims, tight = lattice
    assert A.tags(A.check_grid(image[:-32], gp, fprims, tight, 64)) == ["grid.layout"]
    assert A.tags(A.check_grid(image, dict(gp, n_cells=gp["n_cells"] - 1), fprims, tight, 64)) == ["grid.layout"]


# ---------------------------------------------------------------------------------------------------------------- the whitted fixture
@pytest.fixture(scope="module")
def sphere():
    build, inputs = A.load(os.path.join(GOLD, "sphere300.npz"))
    return {k: {n[len(k) + 1:]: v for n, v in build.items() if n.startswith(k + "/")} for k in ("sah", "morton")}, inputs


def whitted_args(b, inputs):
    return dict(recs=b["recs"].copy(), qrecs=b["qrecs"].copy(), tris=b["tris"].copy(), tidx=b["tidx"].copy(), meta=A.whitted_meta(b["meta"]),
                positions=inputs["positions"], indices=inputs["indices"])


def test_the_recorded_sphere_has_no_violation(sphere):
    builds, inputs = sphere
    for k in ("sah", "morton"):
        assert A.check_mesh(builds[k], inputs) == [], k
        assert A.whitted_meta(builds[k]["meta"])["n_recs"] > 50
    assert not np.array_equal(builds["sah"]["recs"], builds["morton"]["recs"])   # (two different trees over the same leaves)


def _links(a):
    """[record, child] links and where they sit in recs [n, 4, 4]"""
    rc = a["recs"].reshape(-1, 4, 4)
    return np.stack([rc[:, 0, 3], rc[:, 2, 3]], axis=1).view(np.int32)


def _find(a, want):
    """the first (record, child) whose child is a record (want = "record") or a leaf of fewer than four / exactly four / more than one triangles"""
    link = _links(a)
    for r in range(len(link)):
        for c in (0, 1):
            cnt = ((-1 - int(link[r, c])) >> A.LEAF_SHIFT) + 1
            if (want == "record" and link[r, c] > 0) or (link[r, c] < 0 and ((want == "short" and 1 < cnt < 4) or (want == "full" and cnt == 4) or (want == "leaf" and cnt > 1))):
                return r, c
    raise AssertionError("no %s child" % want)


def _set_link(a, r, c, v):
    a["recs"].reshape(-1, 4, 4)[r, 2 * c, 3] = i2f(v)
    a["qrecs"].reshape(-1, 2, 4)[r, c, 3] = np.array([v], np.int32).view(np.uint32)[0]


def _recount_leaf(a, want, delta):
    r, c = _find(a, want)
    _set_link(a, r, c, int(_links(a)[r, c]) - (delta << A.LEAF_SHIFT))


def _cell(a, upper, delta):
    """one cell of an ordinary quantised plane (not clamped to the grid's ends, a whole cell to two outside its fp32 plane) moved by delta"""
    q, rc = a["qrecs"].reshape(-1, 2, 4), a["recs"].reshape(-1, 4, 4)
    g0, gs = A.f64(a["meta"]["grid_lo"]), A.f64(a["meta"]["grid_step"])
    for r, c, axis in np.ndindex(a["meta"]["n_recs"], 2, 3):
        cell = (int(q[r, c, axis]) >> 16) if upper else (int(q[r, c, axis]) & 0xFFFF)
        x = (float(rc[r, 2 * c + (1 if upper else 0), axis]) - g0[axis]) / gs[axis]
        if 0 < cell < 65535 and 1.0 <= (cell - x if upper else x - cell) < 1.9:
            break
    else:
        raise AssertionError("no ordinary plane")
    q[r, c, axis] = np.uint32(int(q[r, c, axis]) + (delta << 16 if upper else delta))


def _sibling(a):
    r, c = _find(a, "record")
    _set_link(a, r, 1 - c, int(_links(a)[r, c]))


def _plane_in(a):
    """the box of a child that is a record: one plane one ulp in (that child's own boxes reach it exactly)"""
    r, c = _find(a, "record")
    inward(a["recs"].reshape(-1, 4, 4), (r, 2 * c, 0), True)


def _leaf_plane_in(a):
    """a leaf's box moved in past the build's pad (1e-4 of the extent: 2.4e-4 here) -- one ulp stays outside the triangles"""
    r, c = _find(a, "leaf")
    a["recs"].reshape(-1, 4, 4)[r, 2 * c + 1, 1] -= np.float32(1e-3)


WHITTED_MUTATIONS = {
    "containment.record: a plane one ulp in": (_plane_in, {"containment.record"}),
    "containment.items: a leaf's plane moved in past the pad": (_leaf_plane_in, {"containment.items"}),
    "shape.tile: a leaf count decremented": (lambda a: _recount_leaf(a, "leaf", -1), {"shape.tile"}),
    "shape.tile: a leaf count incremented": (lambda a: _recount_leaf(a, "short", 1), {"shape.tile"}),
    "shape.leaf: a leaf of five": (lambda a: _recount_leaf(a, "full", 1), {"shape.leaf", "shape.tile"}),
    "shape.reach: a link pointed at the sibling": (_sibling, {"shape.reach", "shape.tile"}),
    "shape.links: a link beyond the records": (lambda a: _set_link(a, *_find(a, "record"), a["meta"]["n_recs"]), {"shape.links", "shape.reach", "shape.tile"}),
    "shape.n_recs: no records over 300 triangles": (lambda a: a["meta"].__setitem__("n_recs", 0), {"shape.n_recs"}),
    "meta.walk_depth: one short": (lambda a: a["meta"].__setitem__("walk_depth", a["meta"]["walk_depth"] - 1), {"meta.walk_depth"}),
    "meta.walk_depth_max: beyond the walk's stack": (lambda a: a["meta"].__setitem__("walk_depth", A.MAX_WALK_DEPTH + 1), {"meta.walk_depth_max"}),
    "meta.depth: too shallow for 300 leaves": (lambda a: a["meta"].__setitem__("depth", 8), {"meta.depth"}),
    "quant.margin: a lower cell moved in by one": (lambda a: _cell(a, False, 1), {"quant.margin"}),
    "quant.margin: an upper cell moved in by one": (lambda a: _cell(a, True, -1), {"quant.margin"}),
    "quant.lower: a lower cell moved in by three": (lambda a: _cell(a, False, 3), {"quant.lower", "quant.margin"}),
    "quant.upper: an upper cell moved in by three": (lambda a: _cell(a, True, -3), {"quant.upper", "quant.margin"}),
    "quant.order: the two cells of a slab exchanged": (lambda a: a["qrecs"].reshape(-1, 2, 4).__setitem__((2, 0, 0), np.uint32((int(a["qrecs"].reshape(-1, 2, 4)[2, 0, 0]) >> 16) | (int(a["qrecs"].reshape(-1, 2, 4)[2, 0, 0]) & 0xFFFF) << 16)),
                                                       {"quant.order", "quant.lower", "quant.upper", "quant.margin"}),
    "quant.links: a quantised link changed alone": (lambda a: a["qrecs"].reshape(-1, 2, 4).__setitem__((3, 1, 3), a["qrecs"].reshape(-1, 2, 4)[3, 0, 3]), {"quant.links"}),
    "triangles.permutation: a triangle index twice": (lambda a: a["tris"].reshape(-1, 3, 4).__setitem__((7, 0, 3), a["tris"].reshape(-1, 3, 4)[8, 0, 3]), {"triangles.permutation"}),
    "triangles.vertices: a vertex one ulp off": (lambda a: inward(a["tris"].reshape(-1, 3, 4), (7, 1, 2), True), {"triangles.vertices"}),
    "triangles.tidx: a packed vertex index changed": (lambda a: a["tidx"].reshape(-1, 2).__setitem__((7, 0), a["tidx"].reshape(-1, 2)[7, 0] ^ np.uint32(1)), {"triangles.tidx"}),
}


@pytest.mark.parametrize("tree", ["sah", "morton"])
@pytest.mark.parametrize("name", sorted(WHITTED_MUTATIONS))
def test_whitted_mutations(sphere, name, tree):
    builds, inputs = sphere
    mutate, expect = WHITTED_MUTATIONS[name]
    a = whitted_args(builds[tree], inputs)
    assert A.check_whitted(**a) == []
    mutate(a)
    got = set(A.tags(A.check_whitted(**a)))
    print(name, tree, "->", sorted(got))
    assert name.split(":")[0] in got and got <= expect, (name, got)


# ---------------------------------------------------------------------------------------------------------------- instanced and clustered
def toy_records(lo, hi, leaf_max):
    """records in the walk's layout over items in leaf order with fp32 bounds lo / hi [n, 3]: median splits of the index range, boxes the
    exact bounds.  Returns (recs [n_recs, 4, 4] float32, the longest chain of records)."""
    recs, depth = [], [0]

    def node(a, b, d):
        """-> (link, lo, hi) of the items [a, b)"""
        blo, bhi = lo[a:b].min(axis=0), hi[a:b].max(axis=0)
        if b - a <= leaf_max:
            return -1 - (a | (b - a - 1) << A.LEAF_SHIFT), blo, bhi
        r = len(recs)
        recs.append(np.zeros((4, 4), np.float32))
        depth[0] = max(depth[0], d)
        m = (a + b) // 2
        for c, (x, y) in enumerate(((a, m), (m, b))):
            link, clo, chi = node(x, y, d + 1)
            recs[r][2 * c, :3], recs[r][2 * c + 1, :3], recs[r][2 * c, 3] = clo, chi, i2f(link)
        return r, blo, bhi

    if len(lo) > leaf_max:
        node(0, len(lo), 1)
    return np.array(recs, np.float32).reshape(-1, 4, 4), depth[0]


def toy_meta(n, n_recs, walk_depth, glo=(0, 0, 0), gstep=(1, 1, 1)):
    return np.concatenate([np.array([int(np.ceil(np.log2(max(n, 1)))), n_recs, walk_depth], np.int32), np.array(list(glo) + list(gstep), np.float32).view(np.int32)])


def toy_mesh_build(pos, idx, which, leaf_max=A.LEAF_TRIS):
    """one build over the triangles `which` of a mesh, in that order: (recs, qrecs, tris, tidx, meta words)"""
    v = pos[idx[which]]
    tris = np.zeros((len(which), 3, 4), np.float32)
    tris[:, :, :3] = v
    tris[:, 0, 3] = np.asarray(which, np.int32).view(np.float32)
    recs, chain = toy_records(v.min(axis=1), v.max(axis=1), leaf_max)
    glo = (pos.min(axis=0) - np.float32(1e-3)).astype(np.float32)
    gstep = ((pos.max(axis=0) - pos.min(axis=0) + np.float32(2e-3)) / np.float32(65533)).astype(np.float32)
    q = np.zeros((len(recs), 2, 4), np.uint32)
    for c in (0, 1):
        cl = np.clip(np.floor((A.f64(recs[:, 2 * c, :3]) - glo) / gstep) - 1, 0, 65535).astype(np.uint32)
        ch = np.clip(np.ceil((A.f64(recs[:, 2 * c + 1, :3]) - glo) / gstep) + 1, 0, 65535).astype(np.uint32)
        q[:, c, :3] = cl | ch << 16
        q[:, c, 3] = recs[:, 2 * c, 3].view(np.uint32)
    i = idx[which].astype(np.uint32)
    tidx = np.stack([i[:, 0] | i[:, 1] << 16, i[:, 2] | np.asarray(which, np.uint32) << 16], axis=1)
    return recs, q, tris, tidx, toy_meta(len(which), len(recs), chain, glo, gstep)


def outward(lo, hi):
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    lo32 = np.where(lo32 > lo, np.nextafter(lo32, np.float32(-np.inf)), lo32)
    hi32 = np.where(hi32 < hi, np.nextafter(hi32, np.float32(np.inf)), hi32)
    return lo32, hi32


MAX_TRI, CLUSTER = 64, 16   # the toy scene's stand-ins for kMaxTriangles and kClusterTris


def toy_scene():
    """an instanced scene in read_build's layout: mesh 0 of 24 triangles, mesh 1 of 3 (one leaf, no records), mesh 2 of 100 triangles,
    clustered (beyond MAX_TRI: seven clusters of at most CLUSTER and a mid level with records), nine instances"""
    import whitted_instances as WI
    rng = np.random.RandomState(2)

    def strip(n):
        p = np.stack([np.arange(n + 2) * 0.1, rng.uniform(0, 0.3, n + 2), rng.uniform(0, 0.3, n + 2)], axis=1).astype(np.float32)
        return {"positions": p, "indices": np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], axis=1).astype(np.uint32)}

    meshes = [strip(24), strip(3), strip(100)]
    build, infos, table, base = {}, [], [], 0
    for k, m in enumerate(meshes):
        pos, idx, n = m["positions"], m["indices"].astype(np.int64), len(m["indices"])
        head = dict(rec_base=base, tri_base=base, vert_base=0, root=0, depth=0, clustered=int(n > MAX_TRI), n_tris=n)
        if n <= MAX_TRI:
            recs, q, tris, tidx, meta = toy_mesh_build(pos, idx, np.arange(n))
            head.update(root=0 if len(recs) else -1 - ((n - 1) << A.LEAF_SHIFT), depth=int(meta[2]) if len(recs) else 0)
            built = [np.concatenate([[base, len(recs), base], meta])]
            parts = ([recs], [q], [tris], tidx)
        else:
            ncl = (n + CLUSTER - 1) // CLUSTER
            order = rng.permutation(n)   # (the mesh's "sorted" order: any permutation cut into runs)
            starts = [A.cluster_start(n, ncl, c) for c in range(ncl + 1)]
            rec, built, R, Q, T, clo, chi, cdepth = base + ncl - 1, [], [], [], [], [], [], 0
            for c in range(ncl):
                which = np.sort(order[starts[c]:starts[c + 1]])
                recs, q, tris, _, meta = toy_mesh_build(pos, idx, which)
                built.append(np.concatenate([[rec, len(recs), base + starts[c]], meta]))
                table.append([rec, base + starts[c], 0, 0])
                rec += len(recs)
                cdepth = max(cdepth, int(meta[2]))
                R.append(recs); Q.append(q); T.append(tris)
                v = tris[:, :, :3].reshape(-1, 3)
                clo.append(v.min(axis=0)); chi.append(v.max(axis=0))
            mid, chain = toy_records(np.array(clo), np.array(chi), A.LEAF_TRIS)
            built.append(np.concatenate([[base, len(mid), -1], toy_meta(ncl, len(mid), chain)]))
            head.update(root=1 + ((len(table) - ncl) << 3 | A.MID_HAS_RECORDS), depth=chain + cdepth)
            parts = (R + [mid], Q, T, np.zeros((n, 2), np.uint32))
        tag = "mesh%d." % k
        build[tag + "recs"] = np.concatenate(parts[0]).reshape(-1, 4)
        build[tag + "qrecs"] = np.concatenate(parts[1]).reshape(-1, 4)
        build[tag + "tris"] = np.concatenate(parts[2]).reshape(-1, 4)
        build[tag + "tidx"] = parts[3]
        build[tag + "info"] = np.concatenate([np.array([head[f] for f in ("rec_base", "tri_base", "vert_base", "root", "depth", "clustered", "n_tris")] + [len(built)])] + built).astype(np.int32)
        infos.append(head)
        base += n
    build["clusters"] = np.array(table, np.int32)
    inst = [(WI.transform(WI.rotation(rng) @ np.diag(rng.uniform(0.5, 2.0, 3)), rng.uniform(-5, 5, 3)), k % 3, 0) for k in range(9)]
    lo, hi = np.zeros((9, 3)), np.zeros((9, 3))
    for i, (tr, mk, _) in enumerate(inst):
        t = np.asarray(tr, np.float32).astype(np.float64)
        w = A.f64(meshes[mk]["positions"]) @ t[:, :3].T + t[:, 3]
        lo[i], hi[i] = w.min(axis=0), w.max(axis=0)
    order = np.argsort(lo[:, 0])
    tlo, thi = outward(lo[order], hi[order])
    top, chain = toy_records(tlo, thi, A.LEAF_TRIS)
    walk = np.zeros((9, 16), np.uint32)
    for p, i in enumerate(order):
        h = infos[inst[i][1]]
        walk[p, 12:16] = np.array([h["rec_base"], h["tri_base"], h["root"], i], np.int32).view(np.uint32)
    mesh_depth = max(h["depth"] for h in infos)
    build.update({"top.recs": top.reshape(-1, 4), "top.inst": walk,
                  "top.meta": np.concatenate([toy_meta(9, len(top), chain), np.array([len(top), 9, chain + mesh_depth, mesh_depth], np.int32)])})
    return build, meshes, inst


def _check_toy(build, meshes, inst):
    return A.check_instanced(build, meshes, inst, max_triangles=MAX_TRI, cluster_tris=CLUSTER)


def test_the_toy_instanced_scene_has_no_violation():
    build, meshes, inst = toy_scene()
    assert _check_toy(build, meshes, inst) == []
    info = A.mesh_info(build["mesh2.info"])
    assert info["clustered"] == 1 and len(info["built"]) == 8 and info["built"][7]["n_recs"] > 0 and len(build["top.recs"]) > 0


def _top_rec(b):
    return b["top.recs"].reshape(-1, 4, 4)


INSTANCED_MUTATIONS = {
    "top.inst.permutation: an instance twice": (lambda b: b["top.inst"].__setitem__((3, 15), b["top.inst"][4, 15]), {"top.inst.permutation"}),
    "top.inst.bases: a record base of another mesh": (lambda b: b["top.inst"].__setitem__((3, 12), b["top.inst"][3, 12] + np.uint32(1)), {"top.inst.bases"}),
    "top.inst.bases: a root of another mesh": (lambda b: b["top.inst"].__setitem__((3, 14), b["top.inst"][3, 14] ^ np.uint32(8)), {"top.inst.bases"}),
    "top.containment.items: a top-level plane one ulp in": (lambda b: inward(_top_rec(b), (len(_top_rec(b)) - 1, 0, 0), True), {"top.containment.items"}),
    "top.shape.tile: a top-level leaf one instance short": (lambda b: _top_rec(b).__setitem__((len(_top_rec(b)) - 1, 0, 3), i2f(int(_top_rec(b)[len(_top_rec(b)) - 1, 0, 3:4].view(np.int32)[0]) + (1 << A.LEAF_SHIFT))),
                                                            {"top.shape.tile"}),
    "top.meta.walk_depth: one short": (lambda b: b["top.meta"].__setitem__(11, b["top.meta"][11] - 1), {"top.meta.walk_depth"}),
    "mesh2.clusters.tile: a clusters row shifted by one triangle": (lambda b: b["clusters"].__setitem__((2, 1), b["clusters"][2, 1] + 1), {"mesh2.clusters.tile"}),
    "mesh2.clusters.table: a clusters row of another cluster's records": (lambda b: b["clusters"].__setitem__((2, 0), b["clusters"][3, 0]), {"mesh2.clusters.table"}),
    "mesh2.mid.root: the mid level's root bits": (lambda b: b["mesh2.info"].__setitem__(3, b["mesh2.info"][3] ^ A.MID_HAS_RECORDS), {"mesh2.mid.root", "top.inst.bases"}),
    "mesh2.mid.containment.items: a mid-level plane one ulp in": (lambda b: inward(b["mesh2.recs"].reshape(-1, 4, 4), (len(b["mesh2.recs"]) // 4 - 1, 1, 1), False), {"mesh2.mid.containment.items"}),
    "mesh2.c3.shape.tile: a cluster's leaf one triangle short": (lambda b: _shorten_cluster_leaf(b, 3), {"mesh2.c3.shape.tile"}),
    "mesh2.c0.triangles.vertices: a cluster's vertex one ulp off": (lambda b: inward(b["mesh2.tris"].reshape(-1, 3, 4), (2, 1, 1), True), {"mesh2.c0.triangles.vertices"}),
    "mesh0.containment.record: a mesh's plane one ulp in": (lambda b: inward(b["mesh0.recs"].reshape(-1, 4, 4), (0, 0, 0), True), {"mesh0.containment.record", "mesh0.containment.items"}),   # (the toy boxes have no pad)
    "mesh1.info: a one-leaf mesh's root code": (lambda b: b["mesh1.info"].__setitem__(3, -1 - (1 << A.LEAF_SHIFT)), {"mesh1.info", "top.inst.bases"}),
}


def _shorten_cluster_leaf(b, c):
    info = A.mesh_info(b["mesh2.info"])
    r0 = sum(q["n_recs"] for q in info["built"][:c])
    rc = b["mesh2.recs"].reshape(-1, 4, 4)
    for r in range(r0, r0 + info["built"][c]["n_recs"]):
        link = int(rc[r, 0, 3:4].view(np.int32)[0])
        if link < 0 and (-1 - link) >> A.LEAF_SHIFT > 0:
            rc[r, 0, 3] = i2f(link + (1 << A.LEAF_SHIFT))
            b["mesh2.qrecs"].reshape(-1, 2, 4)[r, 0, 3] = np.array([link + (1 << A.LEAF_SHIFT)], np.int32).view(np.uint32)[0]
            return
    raise AssertionError("no leaf of several triangles")


@pytest.mark.parametrize("name", sorted(INSTANCED_MUTATIONS))
def test_instanced_mutations(name):
    build, meshes, inst = toy_scene()
    build = {k: v.copy() for k, v in build.items()}
    mutate, expect = INSTANCED_MUTATIONS[name]
    mutate(build)
    got = set(A.tags(_check_toy(build, meshes, inst)))
    print(name, "->", sorted(got))
    assert name.split(":")[0] in got and got <= expect, (name, got)
