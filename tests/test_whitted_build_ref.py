"""The reference build of tests/whitted_build_ref.py and its checks, against the device builds recorded in
tests/golden/build_closure/sphere300.npz (300 triangles, built with the surface-area records, "sah/", and with RTGO_WHITTED_NO_SAH,
"morton/"): the reference reproduces the recorded order, depth and leaves exactly, the checks are clean on the records they belong to,
the surface-area check tells the Morton records from surface-area records, and each mutation of a COPY of the recorded arrays is
reported under its own tag.  Nothing here touches a device."""
import os

import numpy as np
import pytest

import accel_check as A
import whitted_build_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_closure")
F = np.float32


def i2f(v):
    return np.array([v], np.int32).view(np.float32)[0]


def leaf_link(first, count):
    return -1 - (first | (count - 1) << A.LEAF_SHIFT)


@pytest.fixture(scope="module")
def sphere():
    build, inputs = A.load(os.path.join(GOLD, "sphere300.npz"))
    return build, R.Reference(inputs["positions"], inputs["indices"])


def arrays(sphere, key):
    """copies of one recorded build's records and triangles, with its meta"""
    build, ref = sphere
    meta = A.whitted_meta(build[key + "meta"])
    return {"recs": build[key + "recs"].reshape(-1, 4, 4).copy(), "tris": build[key + "tris"].copy(), "n_recs": meta["n_recs"], "depth": meta["depth"],
            "walk_depth": meta["walk_depth"]}


def sah(a, ref):
    return R.check_sah_records(a["recs"], a["n_recs"], ref.runs, ref.boxes, a["walk_depth"])


def morton(a, ref):
    return R.check_morton_records(a["recs"], a["n_recs"], ref, ref.boxes, a["walk_depth"])


# ---------------------------------------------------------------------------------------------------------------- the recorded builds
@pytest.mark.parametrize("key", ["sah/", "morton/"])
def test_order_depth_and_leaves_are_exact(sphere, key):
    build, ref = sphere
    a = arrays(sphere, key)
    assert R.check_order(a["tris"], ref.order) == []
    assert R.check_depth(a["depth"], ref.depth) == [] and ref.depth == 10
    _, link, _ = R._links(a["recs"], a["n_recs"])
    assert sorted(R.leaf_of(k) for k in link.reshape(-1) if k < 0) == ref.runs and len(ref.runs) == 104
    assert sum(c for _, c in ref.runs) == 300 and max(c for _, c in ref.runs) <= A.LEAF_TRIS


def test_the_morton_records_are_the_reference_hierarchy_cut_at_the_runs(sphere):
    v = morton(arrays(sphere, "morton/"), sphere[1])
    assert v == [] and v.stats["records"] == 103


def test_the_surface_area_records_pass_with_no_excess(sphere):
    v = sah(arrays(sphere, "sah/"), sphere[1])
    R.report("sphere300, recorded", v)
    assert v == [] and v.stats["excess"] == 0.0 and sum(v.stats["axes"]) == 103 and all(v.stats["axes"])


def test_the_checks_tell_the_two_kinds_of_records_apart(sphere):
    """the Morton records split where a key bit flips, up to 0.93 of the cheapest split above it; the surface-area records are no
    left-to-right ranges"""
    v = sah(arrays(sphere, "morton/"), sphere[1])
    assert A.tags(v) == ["sah.cost"] and 0.9 < v.stats["excess"] < 0.95
    assert "morton.range" in A.tags(morton(arrays(sphere, "sah/"), sphere[1]))


# ---------------------------------------------------------------------------------------------------------------- mutations
def swap_triangles_of_different_codes(a, ref):
    codes = ref.codes[ref.order]
    i = int(np.flatnonzero(codes[1:] != codes[:-1])[0])
    t = a["tris"].reshape(-1, 3, 4)
    t[[i, i + 1]] = t[[i + 1, i]]


def split_a_leaf_run(a, ref):
    """a leaf of four triangles becomes a record over two leaves of two"""
    rc = a["recs"]
    r, c = next((r, c) for r in range(a["n_recs"]) for c in (0, 1) if R.bits(rc[r, 2 * c, 3:4])[0] < 0 and R.leaf_of(R.bits(rc[r, 2 * c, 3:4])[0])[1] == 4)
    first, _ = R.leaf_of(R.bits(rc[r, 2 * c, 3:4])[0])
    new = np.zeros((1, 4, 4), F)
    new[0, 0:2, 0:3] = new[0, 2:4, 0:3] = rc[r, 2 * c:2 * c + 2, 0:3]
    new[0, 0, 3], new[0, 2, 3] = i2f(leaf_link(first, 2)), i2f(leaf_link(first + 2, 2))
    rc[r, 2 * c, 3] = i2f(a["n_recs"])
    a["recs"] = np.concatenate([rc[:a["n_recs"]], new])
    a["n_recs"] += 1


def three_unit_records(a, ref):
    """(record, leaf child, units in the order of the axis it split on): records over three units, one a leaf and two below a record of
    two leaves"""
    got = R.record_units(a["recs"], a["n_recs"], ref.runs, A._Out(), "")
    order, chain, link, box, below = got
    ub64, key32, w = A.f64(ref.boxes), (ref.boxes[:, 0:3] + ref.boxes[:, 3:6]).astype(F), np.array([c for _, c in ref.runs], np.float64)
    for r in order:
        U = np.sort(np.concatenate([below[(r, 0)], below[(r, 1)]]))
        leaf = [c for c in (0, 1) if link[r, c] < 0]
        if len(U) != 3 or len(leaf) != 1:
            continue
        orders, costs = R.sweep_costs(ub64, key32, w, U)
        for ax in range(3):
            o = orders[ax]
            if (leaf[0] == 0 and o[0] == below[(r, 0)][0]) or (leaf[0] == 1 and o[2] == below[(r, 1)][0]):
                yield r, leaf[0], o, costs[ax]
                break


def move_a_split(a, ref, min_change):
    """record r over units (x, y, z) sorted on its axis, split x | y z (or x y | z), becomes x y | z (x | y z): the leaf child swaps
    sides with the far unit of the inner record, which keeps the middle one.  Chooses a record where that changes the cost by more
    than min_change of it; returns the record."""
    rc = a["recs"]
    for r, leaf, o, costs in three_unit_records(a, ref):
        if abs(costs[1] - costs[0]) <= min_change * costs.min() or costs[1 - leaf] <= costs[leaf]:
            continue
        q = int(R.bits(rc[r, 2 * (1 - leaf), 3:4])[0])                      # the inner record, over the other two units
        rows = {}                                                           # unit -> its two rows (box and leaf link)
        for rec, c in ((r, leaf), (q, 0), (q, 1)):
            run = R.leaf_of(R.bits(rc[rec, 2 * c, 3:4])[0])
            rows[ref.runs.index(run)] = rc[rec, 2 * c:2 * c + 2].copy()
        x, y, z = (rows[int(u)] for u in o)
        inner, alone, side = ((x, y), z, 0) if leaf == 0 else ((y, z), x, 1)   # side: where the inner record goes
        rc[q, 0:2], rc[q, 2:4] = inner
        rc[r, 2 * (1 - side):2 * (1 - side) + 2] = alone
        rc[r, 2 * side, 0:3], rc[r, 2 * side + 1, 0:3] = np.minimum(inner[0][0, 0:3], inner[1][0, 0:3]), np.maximum(inner[0][1, 0:3], inner[1][1, 0:3])
        rc[r, 2 * side, 3], rc[r, 2 * side + 1, 3] = i2f(q), 0.0
        return r
    raise AssertionError("the fixture has no record over three units whose two splits differ by %g" % min_change)


def repartition_off_every_axis(a, ref):
    """a record over two records of two leaves each exchanges one leaf of the left with one of the right, such that the new left pair is
    a prefix of the four units on no axis; returns the record"""
    rc = a["recs"]
    _, _, link, _, below = R.record_units(a["recs"], a["n_recs"], ref.runs, A._Out(), "")
    ub64, key32, w = A.f64(ref.boxes), (ref.boxes[:, 0:3] + ref.boxes[:, 3:6]).astype(F), np.array([c for _, c in ref.runs], np.float64)
    for r in range(a["n_recs"]):
        if link[r, 0] < 0 or link[r, 1] < 0 or len(below[(r, 0)]) != 2 or len(below[(r, 1)]) != 2:
            continue
        ql, qr = int(link[r, 0]), int(link[r, 1])
        U = np.sort(np.concatenate([below[(r, 0)], below[(r, 1)]]))
        orders, _ = R.sweep_costs(ub64, key32, w, U)
        for cl in (0, 1):
            for cr in (0, 1):
                newl = {int(below[(ql, 1 - cl)][0]), int(below[(qr, cr)][0])}
                if any(set(o[:2].tolist()) == newl for o in orders):
                    continue
                a_rows, b_rows = slice(2 * cl, 2 * cl + 2), slice(2 * cr, 2 * cr + 2)
                rc[ql, a_rows], rc[qr, b_rows] = rc[qr, b_rows].copy(), rc[ql, a_rows].copy()
                for c, q in ((0, ql), (1, qr)):
                    rc[r, 2 * c, 0:3] = np.minimum(rc[q, 0, 0:3], rc[q, 2, 0:3])
                    rc[r, 2 * c + 1, 0:3] = np.maximum(rc[q, 1, 0:3], rc[q, 3, 0:3])
                return r
    raise AssertionError("the fixture has no record over two pairs of leaves that can be re-partitioned off every axis")


def grow_a_box(a, ref):
    a["recs"][5, 3, 1] = np.nextafter(a["recs"][5, 3, 1], F(np.inf))


SAH_MUTATIONS = {
    "order.morton: two triangles of different codes swapped": (swap_triangles_of_different_codes, {"order.morton"}),
    "sah.leaves: a leaf run split in two": (split_a_leaf_run, {"sah.leaves"}),
    "sah.cost: a split moved one position": (lambda a, ref: move_a_split(a, ref, 1e-3), {"sah.cost"}),
    "sah.prefix: children re-partitioned off every axis": (repartition_off_every_axis, {"sah.prefix", "sah.cost"}),
    "sah.box: a child box grown by one ulp": (grow_a_box, {"sah.box"}),
    "morton.depth: meta.depth one more": (lambda a, ref: a.__setitem__("depth", a["depth"] + 1), {"morton.depth"}),
    "morton.depth: meta.depth one short": (lambda a, ref: a.__setitem__("depth", a["depth"] - 1), {"morton.depth"}),
    "sah.walk_depth: one more": (lambda a, ref: a.__setitem__("walk_depth", a["walk_depth"] + 1), {"sah.walk_depth"}),
}


def everything(a, ref, records):
    out = R.check_order(a["tris"], ref.order)
    R.check_depth(a["depth"], ref.depth, out)
    out += records(a, ref)
    return out


@pytest.mark.parametrize("name", sorted(SAH_MUTATIONS))
def test_mutations_of_the_surface_area_build(sphere, name):
    mutate, expect = SAH_MUTATIONS[name]
    a, ref = arrays(sphere, "sah/"), sphere[1]
    assert everything(a, ref, sah) == []
    mutate(a, ref)
    got = set(A.tags(everything(a, ref, sah)))
    print(name, "->", sorted(got))
    assert name.split(":")[0] in got and got <= expect, (name, got)


def test_a_moved_split_is_reported_at_its_record_alone(sphere):
    a, ref = arrays(sphere, "sah/"), sphere[1]
    r = move_a_split(a, ref, 1e-3)
    v = sah(a, ref)
    assert len(v) == 1 and v[0].startswith("sah.cost: record %d:" % r), v
    assert v.stats["excess"] > 1e-3


MORTON_MUTATIONS = {
    "morton.leaves: a leaf run split in two": (split_a_leaf_run, {"morton.leaves"}),
    "morton.box: a child box grown by one ulp": (grow_a_box, {"morton.box"}),
    "morton.walk_depth: one short": (lambda a, ref: a.__setitem__("walk_depth", a["walk_depth"] - 1), {"morton.walk_depth"}),
}


@pytest.mark.parametrize("name", sorted(MORTON_MUTATIONS))
def test_mutations_of_the_morton_records(sphere, name):
    mutate, expect = MORTON_MUTATIONS[name]
    a, ref = arrays(sphere, "morton/"), sphere[1]
    assert everything(a, ref, morton) == []
    mutate(a, ref)
    got = set(A.tags(everything(a, ref, morton)))
    print(name, "->", sorted(got))
    assert got == expect, (name, got)


def test_a_morton_split_one_position_off_is_no_reference_node(sphere):
    """x | y z over adjacent runs becomes x y | z (or the reverse): contiguous ranges still, with a split the hierarchy does not have"""
    a, ref = arrays(sphere, "morton/"), sphere[1]
    rc = a["recs"]
    _, _, link, _, below = R.record_units(rc, a["n_recs"], ref.runs, A._Out(), "")
    r = next(r for r in range(a["n_recs"]) if link[r, 0] < 0 and link[r, 1] >= 0 and len(below[(r, 1)]) == 2)
    q = int(link[r, 1])
    # r: (x | q: (y | z))  ->  r: (q: (x | y) | z)
    x, y, z = rc[r, 0:2].copy(), rc[q, 0:2].copy(), rc[q, 2:4].copy()
    rc[q, 0:2], rc[q, 2:4] = x, y
    rc[r, 2:4] = z
    rc[r, 0, 0:3], rc[r, 1, 0:3], rc[r, 0, 3] = np.minimum(x[0, 0:3], y[0, 0:3]), np.maximum(x[1, 0:3], y[1, 0:3]), i2f(q)
    assert A.tags(morton(a, ref)) == ["morton.records"]


# ---------------------------------------------------------------------------------------------------------------- hand-made inputs
def points(*p):
    """one degenerate triangle per point (all three corners the point), and the vertices"""
    pos = np.array(p, F)
    return pos, np.repeat(np.arange(len(pos), dtype=np.uint32), 3).reshape(-1, 3)


def test_a_centroid_on_the_upper_bound_lands_in_cell_1023():
    """bounds [0, 1]^3.  The centroid of three copies of 1 is ((1 + 1) + 1) * float32(1/3) = 3 * 0.3333333432674408 = 1.00000003, which
    rounds to 1: u = 1, u * 1024 = 1024, held to 1023 on every axis, all thirty bits set.  (0.5, 0.25, 0) likewise gives exactly 0.5 and
    0.25: cells 512 = bit 9 of x -> bit 29, 256 = bit 8 of y -> bit 25, 0."""
    pos, idx = points((1.0, 1.0, 1.0), (0.5, 0.25, 0.0), (0.0, 0.0, 0.0))
    order, codes = R.morton_order(pos, idx)
    assert codes.tolist() == [(1 << 30) - 1, (1 << 29) | (1 << 25), 0] and order.tolist() == [2, 1, 0]
    assert R.morton_cells(np.array([[1.0, 1.0, 1.0]], F), np.zeros(3, F), np.ones(3, F)).tolist() == [[1023, 1023, 1023]]


def test_a_zero_extent_gives_cell_0():
    """all z = 5: no extent on z, cell 0 there whatever the coordinate; x and y of the far corner in cell 1023: bits 3 b + 2 and 3 b + 1
    for b = 0 .. 9 = 6 * (8^10 - 1) / 7"""
    pos, idx = points((1.0, 1.0, 5.0), (0.0, 0.0, 5.0))
    order, codes = R.morton_order(pos, idx)
    assert codes.tolist() == [6 * ((8 ** 10 - 1) // 7), 0] == [920350134, 0] and order.tolist() == [1, 0]
    # and a mesh that is one point: every cell 0, the order is the index
    pos, idx = points((2.0, 3.0, 4.0))
    order, codes = R.morton_order(pos, np.tile(idx, (5, 1)))
    assert codes.tolist() == [0] * 5 and order.tolist() == [0, 1, 2, 3, 4]


def test_unused_vertices_do_not_move_the_bounds():
    pos, idx = points((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (-50.0, 70.0, 1e6))
    lo, hi = R.used_bounds(pos, idx[:2])
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [1, 1, 1]
    assert R.morton_order(pos, idx[:2])[1].tolist() == [(1 << 30) - 1, 0]


def test_the_hierarchy_splits_where_the_highest_differing_bit_flips():
    """keys (0, 0) (0, 1) (5, 2) (7, 3): the root's ends differ first in code bit 2, set from position 2 on; positions 0 and 1 share a code
    and differ in bit 0 of the position; 5 = 101 and 7 = 111 differ in code bit 1"""
    nodes, depth = R.hierarchy(np.array([0, 0, 5, 7], np.uint64))
    assert sorted(nodes) == [(0, 1, 1), (0, 2, 3), (2, 3, 3)] and depth == 2
    assert R.hierarchy(np.array([9], np.uint64)) == ([], 0)
    # 64 equal codes: the tree over the positions' six bits, cut into 16 runs of four
    nodes, depth = R.hierarchy(np.zeros(64, np.uint64))
    assert depth == 6 and len(nodes) == 63 and (0, 32, 63) in nodes and (16, 24, 31) in nodes
    assert R.leaf_runs(nodes, 64, 4) == [(4 * k, 4) for k in range(16)] and len(R.cut_nodes(nodes, 4)) == 15
    # five positions: 0 .. 3 | 4; leaves of at most four triangles: one run of four and one of one, one record
    nodes, depth = R.hierarchy(np.zeros(5, np.uint64))
    assert depth == 3 and R.leaf_runs(nodes, 5, 4) == [(0, 4), (4, 1)] and R.cut_nodes(nodes, 4) == {(0, 4, 4)}
    assert R.leaf_runs([], 1, 4) == [(0, 1)] and R.leaf_runs(R.hierarchy(np.zeros(4, np.uint64))[0], 4, 4) == [(0, 4)]


def test_unit_boxes_are_the_exact_bounds_moved_out_by_the_pad():
    """bounds [0, 2] x [0, 1] x [0, 0]: maxext 2, reach 2; the pad is float32(float32(2 * 1e-4f) + 1e-6f), far above 2 * 2^-22"""
    pos = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [2, 1, 0]], F)
    idx = np.array([[0, 1, 2], [1, 3, 2]], np.uint32)
    pad = F(F(F(2) * F(1e-4)) + F(1e-6))
    assert R.box_pad(np.zeros(3, F), np.array([2, 1, 0], F)) == pad
    b = R.unit_boxes(pos, idx, [0, 1], [(0, 1), (1, 1)])
    assert b.dtype == np.float32 and np.array_equal(b, np.array([[-pad, -pad, -pad, F(2) + pad, F(1) + pad, pad], [-pad, -pad, -pad, F(2) + pad, F(1) + pad, pad]], F))
    assert np.array_equal(R.unit_boxes(pos, idx, [0, 1], [(0, 2)]), b[:1])
    # far from the origin the second term takes over: two floats at the largest coordinate
    assert R.box_pad(np.full(3, 1e4, F), np.full(3, 1e4 + 1, F)) == F(F(1e4 + 1) * F(2.3841858e-7)) > F(1e-4) + F(1e-6)
