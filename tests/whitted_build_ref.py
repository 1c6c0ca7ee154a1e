"""A reference build of the triangle ("whitted") path's structures, in numpy, and the checks that hold what the device built to it.

accel_check.py proves that a build is A valid structure (a permutation, a tiling, conservative boxes).  This file states WHICH structure
DESIGN.md 3.4 describes and compares the device's arrays with it:

  exactly      the Morton order (morton_order), the Morton hierarchy and its depth (hierarchy), the leaves (leaf_runs), the boxes the
               surface-area pass reads (unit_boxes), the Morton records' topology, every record's child boxes, walk_depth
  to a bound   the surface-area records: every record splits its units at a position of one of the three sorts sah_build documents, and in
               float64 that split costs at most (1 + COST_MARGIN) times the cheapest position of any of them

The recipe is restated from the formulas, not from the kernels' control flow: a sort is numpy's argsort of the keys (whatever bitonic
or radix passes produce it on the device), the hierarchy is a recursive split at the highest differing key bit (not Karras' searches),
the sweep is a pair of accumulate() calls.  Everything that decides is done in float32, operation for operation (the library is
compiled without contraction, so a float32 numpy expression of the same operations gives the same bits).

Positions in a structure are SORTED positions; a node is (first, split, last): it holds the sorted triangles [first, last], its left
child [first, split), its right child [split, last].  A unit is a leaf run (first, count): a maximal subtree of at most leaf_tris
triangles.  Record layout: accel_check.py."""
import numpy as np

from accel_check import LEAF_SHIFT, LEAF_TRIS, _Out, bits, f64

COST_MARGIN = 2e-6   # see check_sah_records
SAH_MAX_TRIANGLES = (150 * 1024 - 16) // 33   # the host's rule: the surface-area pass's LDS is 33 n + 16 bytes, at most 150 KiB (4654)
F = np.float32


# ------------------------------------------------------------------------------------------------------------------ the reference build
def used_bounds(positions, indices):
    """float32 (lo, hi) over the vertices the triangles name (a vertex no triangle names does not count)"""
    pos = np.asarray(positions, F).reshape(-1, 3)
    used = pos[np.unique(np.asarray(indices).reshape(-1))]
    return used.min(axis=0), used.max(axis=0)


def box_pad(lo, hi):
    """the pad of every box a build writes, from the build's bounds: max(maxext * 1e-4 + 1e-6, reach * 2^-22) in float32"""
    maxext = F((hi - lo).astype(F).max())
    reach = F(max(np.abs(lo).max(), np.abs(hi).max()))
    return max(F(F(maxext * F(1e-4)) + F(1e-6)), F(reach * F(2.3841858e-7)))


def morton_cells(c, lo, ext):
    """the 10-bit cell of float32 coordinates c [n, 3] on the grid of the bounds [lo, lo + ext]; 0 on an axis without extent"""
    with np.errstate(divide="ignore", invalid="ignore"):
        u = ((c - lo).astype(F) / ext).astype(F)
    u = np.where(ext > 0, u, F(0)).astype(F)
    return np.minimum(np.maximum((u * F(1024)).astype(F), F(0)), F(1023)).astype(np.uint32)


def interleave(cells):
    """30-bit Morton code of cells [n, 3]: bit b of x, y, z goes to bits 3 b + 2, 3 b + 1, 3 b"""
    q = np.asarray(cells, np.uint64)
    code = np.zeros(len(q), np.uint64)
    for b in range(10):
        for a in range(3):
            code |= ((q[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    return code


def morton_order(positions, indices):
    """(order, codes): order[p] = the triangle at sorted position p, codes[t] = triangle t's Morton code (uint64).  The order is the one
    order of the unique keys code << 32 | triangle."""
    pos = np.asarray(positions, F).reshape(-1, 3)
    idx = np.asarray(indices).reshape(-1, 3).astype(np.int64)
    lo, hi = used_bounds(pos, idx)
    ext = (hi - lo).astype(F)
    p0, p1, p2 = pos[idx[:, 0]], pos[idx[:, 1]], pos[idx[:, 2]]
    c = (((p0 + p1).astype(F) + p2).astype(F) * F(1.0 / 3.0)).astype(F)
    codes = interleave(morton_cells(c, lo, ext))
    key = (codes << np.uint64(32)) | np.arange(len(idx), dtype=np.uint64)
    return np.argsort(key, kind="stable").astype(np.int64), codes


def hierarchy(sorted_codes):
    """the binary radix tree over the keys code << 32 | sorted position: (nodes, depth).  nodes: every internal node as (first, split,
    last); depth: edges from the root to the deepest single triangle."""
    codes = np.asarray(sorted_codes, np.uint64)
    n = len(codes)
    keys = ((codes << np.uint64(32)) | np.arange(n, dtype=np.uint64)).tolist()
    karr = np.array(keys, np.uint64)
    nodes, depth, stack = [], 0, [(0, n - 1, 0)]
    while stack:
        first, last, d = stack.pop()
        if first == last:
            depth = max(depth, d)
            continue
        b = (keys[first] ^ keys[last]).bit_length() - 1          # the highest bit in which the range's keys differ ...
        flip = ((keys[first] >> b) | 1) << b                     # ... and the smallest key with the range's prefix and that bit set
        split = first + int(np.searchsorted(karr[first:last + 1], np.uint64(flip), side="left"))
        nodes.append((first, split, last))
        stack += [(first, split - 1, d + 1), (split, last, d + 1)]
    return nodes, depth


def leaf_runs(nodes, n, leaf_tris=LEAF_TRIS):
    """the maximal subtrees of at most leaf_tris triangles as (first, count), in sorted positions, ascending"""
    if n <= leaf_tris:
        return [(0, n)]
    runs = []
    for first, split, last in nodes:
        if last - first + 1 > leaf_tris:
            for a, b in ((first, split - 1), (split, last)):
                if b - a + 1 <= leaf_tris:
                    runs.append((a, b - a + 1))
    return sorted(runs)


def cut_nodes(nodes, leaf_tris=LEAF_TRIS):
    """the nodes above the leaf runs: those of more than leaf_tris triangles (one record each)"""
    return {nd for nd in nodes if nd[2] - nd[0] + 1 > leaf_tris}


def unit_boxes(positions, indices, order, runs):
    """float32 [n_units, 6] (lo, hi): per leaf run the exact min / max of its triangles' vertices, moved out by the build's pad"""
    pos = np.asarray(positions, F).reshape(-1, 3)
    idx = np.asarray(indices).reshape(-1, 3).astype(np.int64)
    pad = box_pad(*used_bounds(pos, idx))
    v = pos[idx[np.asarray(order, np.int64)]]                    # [sorted position, corner, axis]
    starts = np.array([r[0] for r in runs], np.int64)
    lo = np.minimum.reduceat(v.min(axis=1), starts, axis=0)
    hi = np.maximum.reduceat(v.max(axis=1), starts, axis=0)
    return np.concatenate([(lo - pad).astype(F), (hi + pad).astype(F)], axis=1)


class Reference:
    """the reference build of one structure: order, codes, nodes, depth, runs, boxes (of the runs)"""

    def __init__(self, positions, indices, leaf_tris=LEAF_TRIS):
        self.n = len(np.asarray(indices).reshape(-1, 3))
        self.leaf_tris = leaf_tris
        self.order, self.codes = morton_order(positions, indices)
        self.nodes, self.depth = hierarchy(self.codes[self.order])
        self.runs = leaf_runs(self.nodes, self.n, leaf_tris)
        self.boxes = unit_boxes(positions, indices, self.order, self.runs)


# ------------------------------------------------------------------------------------------------------------------ reading records
def _links(recs, n_recs):
    rc = np.asarray(recs, F).reshape(-1, 4, 4)[:n_recs]
    link = np.stack([bits(rc[:, 0, 3].copy()), bits(rc[:, 2, 3].copy())], axis=1).astype(np.int64)
    box = np.concatenate([rc[:, [0, 2], 0:3], rc[:, [1, 3], 0:3]], axis=2)      # [record, child, 6]
    return rc, link, box


def leaf_of(link):
    code = -1 - int(link)
    return code & ((1 << LEAF_SHIFT) - 1), (code >> LEAF_SHIFT) + 1


def reachable(link, n_recs, out, tag):
    """the records reachable from record 0, parents before children, with the number of records on the chain down to each; None when
    the links do not form a tree (accel_check's closure reports the details)"""
    order, chain, seen, stack = [], {}, set(), [(0, 1)]
    while stack:
        r, d = stack.pop()
        if r in seen or not 0 <= r < n_recs:
            out.add(tag + "shape", "record %d is reached twice or lies outside the %d records" % (r, n_recs))
            return None
        seen.add(r)
        order.append(r)
        chain[r] = d
        for c in (0, 1):
            if link[r, c] >= 0:
                stack.append((int(link[r, c]), d + 1))
    return order, chain


def record_units(recs, n_recs, runs, out, tag):
    """per reachable record and child, the units (indices into `runs`) below it: (order, chain, link, box, below) with below[(r, c)] a
    sorted int array; None when a leaf link is no run of `runs` or the links are no tree"""
    rc, link, box = _links(recs, n_recs)
    got = reachable(link, n_recs, out, tag)
    if got is None:
        return None
    order, chain = got
    unit_of = {run: u for u, run in enumerate(runs)}
    leaves = [leaf_of(link[r, c]) for r in order for c in (0, 1) if link[r, c] < 0]
    if sorted(leaves) != sorted(runs):
        extra, missing = sorted(set(leaves) - set(runs)), sorted(set(runs) - set(leaves))
        out.add(tag + "leaves", "%d leaf links, %d reference runs; links that are no run: %s, runs without a link: %s" % (len(leaves), len(runs), extra[:4], missing[:4]))
        return None
    below = {}
    for r in reversed(order):
        for c in (0, 1):
            k = link[r, c]
            below[(r, c)] = np.array([unit_of[leaf_of(k)]], np.int64) if k < 0 else np.sort(np.concatenate([below[(int(k), 0)], below[(int(k), 1)]]))
    return order, chain, link, box, below


def _check_boxes(order, box, below, unit_box, out, tag):
    """(b): each child's box is bitwise the union of its units' boxes"""
    for r in order:
        for c in (0, 1):
            u = below[(r, c)]
            want = np.concatenate([unit_box[u, 0:3].min(axis=0), unit_box[u, 3:6].max(axis=0)])
            if not np.array_equal(bits(want), bits(box[r, c])):
                out.add(tag + "box", "record %d child %d: box %s, the union of its %d units' boxes %s" % (r, c, box[r, c], len(u), want))


def _check_walk_depth(chain, walk_depth, out, tag):
    if walk_depth is not None and walk_depth != max(chain.values()):
        out.add(tag + "walk_depth", "walk_depth %d, the longest chain of records has %d" % (walk_depth, max(chain.values())))


# ------------------------------------------------------------------------------------------------------------------ the checks
def triangle_at(tris):
    """tris[3 i].w: the triangle at sorted position i"""
    return bits(np.asarray(tris, F).reshape(-1, 3, 4)[:, 0, 3].copy()).astype(np.int64)


def check_order(tris, ref_order, out=None, tag=""):
    """tris[3 i].w, the triangle at sorted position i, must be the reference order.  tris: the float4 rows of the sorted triangles, or
    (an integer array) the items at the sorted positions as read elsewhere -- a cluster's slice of triangle_at(), a mid level's clusters"""
    out = _Out() if out is None else out
    got = np.asarray(tris).astype(np.int64) if np.issubdtype(np.asarray(tris).dtype, np.integer) else triangle_at(tris)
    want = np.asarray(ref_order, np.int64)
    if len(got) != len(want):
        out.add(tag + "order.morton", "%d sorted triangles, the reference orders %d" % (len(got), len(want)))
        return out
    out.each(tag + "order.morton", got != want, lambda i: "sorted position %d holds triangle %d, the reference order has %d" % (i, got[i], want[i]))
    return out


def check_depth(meta_depth, ref_depth, out=None, tag=""):
    out = _Out() if out is None else out
    if meta_depth != ref_depth:
        out.add(tag + "morton.depth", "meta.depth %d, the reference hierarchy's is %d" % (meta_depth, ref_depth))
    return out


def check_morton_records(recs, n_recs, ref, unit_box=None, walk_depth=None, out=None, tag=""):
    """the records are the reference hierarchy cut at the leaf runs, up to record numbering: the set of (first, split, last) over the
    records reachable from record 0 is the set of the reference's nodes of more than leaf_tris triangles (the left child covering
    [first, split)), the leaf links are the runs, each child's box is the union of its units' (unit_box given), walk_depth the longest
    chain.  ref: a Reference, or anything with nodes, runs, n, leaf_tris.  out.stats: counts for the report."""
    out = _Out() if out is None else out
    out.stats = {"kind": "morton", "triangles": ref.n, "units": len(ref.runs), "records": n_recs}
    want = cut_nodes(ref.nodes, ref.leaf_tris)
    if n_recs == 0 or not want:
        if n_recs != len(want):
            out.add(tag + "morton.records", "%d records, the reference cut has %d nodes" % (n_recs, len(want)))
        return out
    got = record_units(recs, n_recs, ref.runs, out, tag + "morton.")
    if got is None:
        return out
    order, chain, link, box, below = got
    runs = ref.runs
    have = set()
    for r in order:
        lu, ru = below[(r, 0)], below[(r, 1)]
        # Morton units are consecutive runs: a child that covers units a .. b covers the sorted triangles from a's first to b's last
        if lu[-1] - lu[0] + 1 != len(lu) or ru[-1] - ru[0] + 1 != len(ru) or ru[0] != lu[-1] + 1:
            out.add(tag + "morton.range", "record %d: its children hold units %s.. and %s.., no two adjacent ranges left to right" % (r, lu[:4].tolist(), ru[:4].tolist()))
            continue
        have.add((runs[lu[0]][0], runs[ru[0]][0], runs[ru[-1]][0] + runs[ru[-1]][1] - 1))
    if have != want:
        out.add(tag + "morton.records", "%d of the records' (first, split, last) are no reference node: %s; %d reference nodes have no record: %s"
                % (len(have - want), sorted(have - want)[:4], len(want - have), sorted(want - have)[:4]))
    if unit_box is not None:
        _check_boxes(order, box, below, unit_box, out, tag + "morton.")
    _check_walk_depth(chain, walk_depth, out, tag + "morton.")
    return out


def _area(lo, hi):
    e = hi - lo
    return e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0]


def sweep_costs(ubox64, key32, weight, units):
    """float64 costs A(L) W(L) + A(R) W(R) of every split position 1 .. m - 1 of `units` sorted by (key32 on an axis, unit number), for the
    three axes: (orders [3][m], costs [3, m - 1])"""
    orders, costs = [], []
    for a in range(3):
        o = units[np.lexsort((units, key32[units, a]))]
        lo, hi, w = ubox64[o, 0:3], ubox64[o, 3:6], weight[o]
        plo, phi, pw = np.minimum.accumulate(lo, axis=0), np.maximum.accumulate(hi, axis=0), np.cumsum(w)
        slo, shi, sw = np.minimum.accumulate(lo[::-1], axis=0)[::-1], np.maximum.accumulate(hi[::-1], axis=0)[::-1], np.cumsum(w[::-1])[::-1]
        costs.append(_area(plo[:-1], phi[:-1]) * pw[:-1] + _area(slo[1:], shi[1:]) * sw[1:])
        orders.append(o)
    return orders, np.array(costs)


def split_cost(ubox64, weight, left, right):
    c = 0.0
    for u in (left, right):
        c += float(_area(ubox64[u, 0:3].min(axis=0), ubox64[u, 3:6].max(axis=0)) * weight[u].sum())
    return c


def check_sah_records(recs, n_recs, runs, unit_box, walk_depth=None, out=None, tag=""):
    """the surface-area records over the units `runs` (leaf runs, numbered by Morton position; weights: their triangle counts) with the
    float32 boxes unit_box [n_units, 6].  Per record reachable from record 0, over the units U below it:
      sah.leaves      (a) the leaf links under the whole tree are exactly the runs
      sah.box         (b) each child's box is bitwise the union of its units' boxes
      sah.prefix      (c) on some axis the left child's units are a proper prefix of U sorted by (float32(lo + hi) on that axis, unit)
      sah.cost        (d) in float64 the split's cost A(L) W(L) + A(R) W(R) is at most (1 + COST_MARGIN) times the minimum over the three
                          axes and every position of those sorts
      sah.walk_depth  walk_depth is the longest chain of records
    Which of several equal costs wins is not checked.  COST_MARGIN is derived, not measured: the device forms a cost in float32 from 3
    differences, 3 products and 2 sums of non-negative terms, times a weight, plus a second such term -- a relative error under 5e-7;
    two costs it ordered wrongly differ by under 1e-6 of themselves, and 2e-6 doubles that.
    out.stats: units, records, the largest cost excess (cost / minimum - 1) and how many records split on each axis (the first axis on
    which the left child is a prefix)."""
    out = _Out() if out is None else out
    runs = [tuple(int(x) for x in r) for r in runs]
    stats = out.stats = {"kind": "sah", "triangles": sum(r[1] for r in runs), "units": len(runs), "records": n_recs, "excess": 0.0, "axes": [0, 0, 0]}
    if n_recs == 0 or len(runs) < 2:
        if n_recs != max(len(runs) - 1, 0):
            out.add(tag + "sah.leaves", "%d records over %d units" % (n_recs, len(runs)))
        return out
    got = record_units(recs, n_recs, runs, out, tag + "sah.")
    if got is None:
        return out
    order, chain, link, box, below = got
    ub = np.asarray(unit_box, F).reshape(-1, 6)
    _check_boxes(order, box, below, ub, out, tag + "sah.")
    key32 = (ub[:, 0:3] + ub[:, 3:6]).astype(F)
    ub64, weight = f64(ub), np.array([r[1] for r in runs], np.float64)
    for r in order:
        L, R = below[(r, 0)], below[(r, 1)]
        U = np.sort(np.concatenate([L, R]))
        orders, costs = sweep_costs(ub64, key32, weight, U)
        axes = [a for a in range(3) if np.array_equal(np.sort(orders[a][:len(L)]), L)]
        if not axes:
            out.add(tag + "sah.prefix", "record %d: its left child's %d units of %d are a prefix of no axis' order" % (r, len(L), len(U)))
        else:
            stats["axes"][axes[0]] += 1
        best, cost = float(costs.min()), split_cost(ub64, weight, L, R)
        excess = 0.0 if cost <= best else (cost / best - 1.0 if best > 0 else np.inf)
        stats["excess"] = max(stats["excess"], excess)
        if not cost <= best * (1.0 + COST_MARGIN):
            out.add(tag + "sah.cost", "record %d: its split of %d units costs %.9g, the cheapest sweep position %.9g (excess %.3g)" % (r, len(U), cost, best, excess))
    _check_walk_depth(chain, walk_depth, out, tag + "sah.")
    return out


def units_of_records(recs, n_recs):
    """(runs, boxes) read from the records' own leaf children (the top level: its units' boxes are the instances', which the closure
    checks tie to the instances)"""
    rc, link, box = _links(recs, n_recs)
    found = sorted((leaf_of(link[r, c]), r, c) for r in range(n_recs) for c in (0, 1) if link[r, c] < 0)
    return [f[0] for f in found], np.array([box[r, c] for _, r, c in found], F).reshape(-1, 6)


def report(what, out):
    """one line per structure: triangles, units, records, and for surface-area records the largest cost excess and the axes chosen"""
    s = out.stats
    line = "%-44s %-6s %6d triangles %5d units %5d records" % (what, s["kind"], s["triangles"], s["units"], s["records"])
    if s["kind"] == "sah":
        line += "  excess %.3g  axes x %d y %d z %d" % (s["excess"], s["axes"][0], s["axes"][1], s["axes"][2])
    print(line)
    return line
