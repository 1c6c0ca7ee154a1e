"""Structural validators for every acceleration structure the build kernels write, in numpy (no GPU call anywhere in this file except
record()).  Inputs are the arrays of capi.Context.read_build plus the scene's inputs; every function returns a list of violations, each a
string "<invariant>: <which node / record / cell / primitive and what>".  The invariant names are the keys of the mutation tests
(tests/test_accel_check.py).

Geometry is done in float64 on the exact values of the fp32 words, and containment is an exact <= / >= with zero slack: boxes are fp32
min / max of fp32 numbers and every pad in the builds is added, never subtracted, so a correct build satisfies containment exactly.
Where a check restates a DECISION the build takes in fp32 (which primitives are big, which rectangles pair up) it says so below.

Layouts (rtgo_device.h, rtgo_build.h, rtgo_whitted.h, rtgo_whitted_inst.h, rtgo_whitted_host.h's WhittedBuildTarget, rtgo_capi.hip's
build_grid):
  fnodes   2 float4 per node: (lo, left) (hi, right); a leaf: left = first record, right = -(count | pairs << 12 | cuboid << 20)
  fprims   4 float4 per record: rows 0..2 of M^-1, (bits(type), bits(SBT index), 0, 0); [0, n_small) in the tree, the rest up front
  recs     4 float4 per record: (left lo, left link) (left hi, -) (right lo, right link) (right hi, -); link >= 0: a record,
           < 0: the leaf -1 - (first | (count - 1) << 13)
  qrecs    2 uint4 per record: per child x, y, z as (lower cell | upper cell << 16), link
  grid     [table: n_cells words, 0 or 1 + record][records: 8 floats (lo, first | count << 16, hi, 0)][items: 16 bit]"""
import numpy as np

LEAF_SHIFT = 13          # whitted::kLeafShift
LEAF_TRIS = 4            # whitted::kLeafTris
MAX_TRIANGLES = 8192     # whitted::kMaxTriangles: beyond it a mesh is clustered
MAX_WALK_DEPTH = 40      # whitted::kMaxWalkDepth
CLUSTER_TRIS = 4096      # whitted::kClusterTris
MID_HAS_RECORDS = 4      # whitted::kMidHasRecords
CYLINDER, DISK, RECTANGLE, SPHERE = 0, 1, 2, 3
BIG_FRAC = (np.float32(36) * np.float32(0.01), np.float32(0.15))   # build_kernel's big_frac for tree[0] and tree[1] (rtgo_set_scene)
MAX_REPORT = 50          # violations listed per invariant (the count is in the last one)


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class _Out(list):
    """a violation list that stops listing an invariant after MAX_REPORT entries"""

    def __init__(self):
        super().__init__()
        self.count = {}

    def add(self, tag, msg):
        k = self.count.get(tag, 0)
        self.count[tag] = k + 1
        if k < MAX_REPORT:
            self.append("%s: %s" % (tag, msg))

    def each(self, tag, where, fmt):
        for i in np.flatnonzero(where):
            self.add(tag, fmt(int(i)))


def tags(violations):
    return sorted({v.split(":")[0] for v in violations})


# ---------------------------------------------------------------------------------------------------------------- analytic path
def build_meta(words):
    """BuildMeta's 15 words (rtgo_build.h)"""
    w = np.ascontiguousarray(words).view(np.int32)
    f = w.view(np.float32)
    return {"canonical_depth": int(w[0]), "walk_depth": int(w[1]), "n_small": int(w[2]), "tight_bounds": f[3:9].copy(), "list_group": int(w[9]),
            "n_fnodes": int(w[10]), "cub_a": float(f[11]), "cub_b": float(f[12]), "cuboid_leaves": int(w[13]), "tree_types": int(w[14])}


def canonical_depth(nodes):
    """depth of the canonical LBVH (`nodes`: 2 float4 per node, leaves carry right = -1): the largest number of internal ancestors of a leaf"""
    nd = np.asarray(nodes, np.float32).reshape(-1, 2, 4)
    left, right = bits(nd[:, 0, 3].copy()), bits(nd[:, 1, 3].copy())
    depth, best, stack = 0, 0, [(0, 0)]
    while stack:
        k, d = stack.pop()
        if right[k] < 0:
            best = max(best, d)
        else:
            stack += [(int(left[k]), d + 1), (int(right[k]), d + 1)]
    return best


def rect_normals(M):
    """unit world normals of unit rectangles under the model matrices M [n, 16] in float64: row 1 of the inverse of the 3 x 3 part
    (TransformNormal of (0, 1, 0))"""
    A = f64(M).reshape(-1, 4, 4)[:, :3, :3]
    r = np.linalg.inv(A)[:, 1, :]
    return r / np.linalg.norm(r, axis=1, keepdims=True)


def check_tight(tight, aabb, types, M, meta):
    """the per-primitive boxes the fast walk culls with, and their bounds"""
    out = _Out()
    tight32, aabb32 = np.asarray(tight, np.float32).reshape(-1, 6), np.asarray(aabb, np.float32).reshape(-1, 6)
    types = np.asarray(types).astype(np.int64)
    t, Mm = f64(tight32), f64(M).reshape(-1, 4, 4)
    quad = (types == SPHERE) | (types == CYLINDER)
    out.each("tight.quadric", quad & np.any(bits(tight32) != bits(aabb32), axis=1), lambda i: "primitive %d: tight box is not its aabb row" % i)
    mx, mz, c = Mm[:, :3, 0], Mm[:, :3, 2], Mm[:, :3, 3]
    for ty, e, tag in ((RECTANGLE, (np.abs(mx) + np.abs(mz)) / 2, "tight.rectangle"), (DISK, np.sqrt(mx * mx + mz * mz), "tight.disk")):
        bad = (types == ty) & (np.any(t[:, 0:3] > c - e, axis=1) | np.any(t[:, 3:6] < c + e, axis=1))
        out.each(tag, bad, lambda i: "primitive %d: box %s does not contain centre %s +- %s" % (i, tight32[i], c[i], e[i]))
    want = np.concatenate([tight32[:, 0:3].min(axis=0), tight32[:, 3:6].max(axis=0)])
    if not np.array_equal(bits(want), bits(np.asarray(meta["tight_bounds"], np.float32))):
        out.add("tight.bounds", "tight_bounds %s, min / max of the tight rows %s" % (meta["tight_bounds"], want))
    return out


def big_flags(tight, big_frac):
    """build_kernel's decision (tight_boxes_and_big), restated in fp32 as it takes it: a primitive is big when its box spans at least
    big_frac of the scene's tight bounds on two axes"""
    t = np.asarray(tight, np.float32).reshape(-1, 6)
    ext = (t[:, 3:6] - t[:, 0:3]).astype(np.float32)
    scene = (t[:, 3:6].max(axis=0) - t[:, 0:3].min(axis=0)).astype(np.float32)
    return (ext >= (np.float32(big_frac) * scene).astype(np.float32)).sum(axis=1) >= 2


def check_fast_tree(fnodes, fprims, meta, prims6, tight, aabb, types, M, big_frac=BIG_FRAC[0], nodes=None):
    """one fast-walk structure of rtgo_set_scene: tree `fnodes`, records `fprims`, BuildMeta `meta` (build_meta()), against the canonical
    records `prims6`, the tight boxes, the reference boxes `aabb` and the scene's types and model matrices M [n, 16].  nodes: the
    canonical LBVH, for meta.canonical_depth."""
    out = _Out()
    types = np.asarray(types).astype(np.int64)
    n = len(types)
    fp = np.asarray(fprims, np.float32).reshape(-1, 4, 4)
    p6 = np.asarray(prims6, np.float32).reshape(-1, 6, 4)
    tight32 = np.asarray(tight, np.float32).reshape(-1, 6)
    n_small, n_fnodes = meta["n_small"], meta["n_fnodes"]
    fn = np.asarray(fnodes, np.float32).reshape(-1, 2, 4)
    if len(fp) != n or len(p6) != n or len(fn) != n_fnodes or not 0 <= n_small <= n:
        out.add("shape.sizes", "%d fprims, %d prims, %d fnodes for n %d, n_small %d, n_fnodes %d" % (len(fp), len(p6), len(fn), n, n_small, n_fnodes))
        return out
    # ---- records
    orig, ftype = bits(fp[:, 3, 1].copy()).astype(np.int64), bits(fp[:, 3, 0].copy()).astype(np.int64)
    perm_ok = np.array_equal(np.sort(orig), np.arange(n))
    if not perm_ok:
        out.add("records.permutation", "the SBT indices of fprims are not a permutation of 0..%d" % (n - 1))
        return out
    out.each("records.rows", np.any(bits(fp[:, 0:3, :]) != bits(p6[orig, 0:3, :]), axis=(1, 2)), lambda i: "record %d: rows differ from primitive %d's" % (i, orig[i]))
    out.each("records.type", ftype != types[orig], lambda i: "record %d: type %d, primitive %d has %d" % (i, ftype[i], orig[i], types[orig[i]]))
    # ---- which records are up front (the build's own fp32 decision)
    big = big_flags(tight32, big_frac)
    if set(orig[n_small:].tolist()) != set(np.flatnonzero(big).tolist()):
        out.add("shape.big", "records [n_small, n) hold primitives %s, the big ones are %s" % (sorted(orig[n_small:].tolist())[:8], np.flatnonzero(big)[:8].tolist()))
    # ---- shape
    left, right = bits(fn[:, 0, 3].copy()).astype(np.int64), bits(fn[:, 1, 3].copy()).astype(np.int64)
    lo, hi = f64(fn[:, 0, 0:3]), f64(fn[:, 1, 0:3])
    if (n_small == 0) != (n_fnodes == 0) or (n_fnodes > 0 and n_fnodes % 2 == 0):
        out.add("shape.odd", "n_fnodes %d with n_small %d" % (n_fnodes, n_small))
    leaf = right < 0
    count, pairs, cub = (-right) & 0xFFF, ((-right) >> 12) & 0xFF, (-right) >> 20
    visits, anc = np.zeros(n_fnodes, np.int64), np.zeros(n_fnodes, np.int64)
    shape_ok = n_fnodes > 0
    stack = [(0, 0)] if n_fnodes > 0 else []
    while stack:
        k, d = stack.pop()
        visits[k] += 1
        anc[k] = d
        if visits[k] > 1 or leaf[k]:
            continue
        for c in (left[k], right[k]):
            if 0 <= c < n_fnodes:
                stack.append((int(c), d + 1))
            else:
                out.add("shape.links", "node %d: child link %d outside [0, %d)" % (k, c, n_fnodes))
                shape_ok = False
    out.each("shape.reach", visits != 1, lambda k: "node %d reached %d times from the root" % (k, visits[k]))
    shape_ok = shape_ok and bool(np.all(visits == 1))
    lv = np.flatnonzero(leaf & (visits > 0))
    out.each("shape.leaf_count", leaf & (visits > 0) & (count < 1), lambda k: "leaf %d: count %d" % (k, count[k]))
    cover = np.zeros(max(n_small, 1) + 1, np.int64)
    for k in lv:
        a, b = int(left[k]), int(left[k] + count[k])
        if a < 0 or b > n_small:
            out.add("shape.tile", "leaf %d: range [%d, %d) outside [0, %d)" % (k, a, b, n_small))
            shape_ok = False
        else:
            cover[a:b] += 1
    bad = np.flatnonzero(cover[:n_small] != 1)
    if len(bad):
        out.add("shape.tile", "%d records of [0, %d) are not in exactly one leaf, first: record %d in %d leaves" % (len(bad), n_small, bad[0], cover[bad[0]]))
        shape_ok = False
    # ---- containment
    tb = f64(tight32)[orig]   # per record
    if shape_ok:
        for k in lv:
            r = slice(int(left[k]), int(left[k] + count[k]))
            if np.any(lo[k] > tb[r, 0:3]) or np.any(hi[k] < tb[r, 3:6]):
                j = int(left[k]) + int(np.flatnonzero(np.any(lo[k] > tb[r, 0:3], axis=1) | np.any(hi[k] < tb[r, 3:6], axis=1))[0])
                out.add("containment.leaf", "leaf %d: box %s %s does not contain record %d's tight box %s" % (k, fn[k, 0, :3], fn[k, 1, :3], j, tight32[orig[j]]))
        inner = np.flatnonzero(~leaf)
        for c in (left, right):
            ch = c[inner]
            bad = np.any(lo[inner] > lo[ch], axis=1) | np.any(hi[inner] < hi[ch], axis=1)
            for k, q in zip(inner[bad], ch[bad]):
                out.add("containment.node", "node %d: box does not contain child %d's" % (k, q))
        # ---- meta
        want = int(anc[lv].max()) if len(lv) else 0
        if meta["walk_depth"] != want:
            out.add("meta.walk_depth", "walk_depth %d, the deepest leaf has %d internal ancestors" % (meta["walk_depth"], want))
        if meta["cuboid_leaves"] != int(np.sum(cub[lv] != 0)):
            out.add("meta.cuboid_leaves", "cuboid_leaves %d, leaves with a certificate %d" % (meta["cuboid_leaves"], int(np.sum(cub[lv] != 0))))
    elif n_fnodes == 0 and (meta["walk_depth"] != 0 or meta["cuboid_leaves"] != 0):
        out.add("meta.walk_depth", "walk_depth %d, cuboid_leaves %d without a tree" % (meta["walk_depth"], meta["cuboid_leaves"]))
    want = int(np.bitwise_or.reduce(1 << types[orig[:n_small]])) if n_small else 0
    if meta["tree_types"] != want:
        out.add("meta.tree_types", "tree_types %d, the tree's records have %d" % (meta["tree_types"], want))
    if nodes is not None and meta["canonical_depth"] != canonical_depth(nodes):
        out.add("meta.canonical_depth", "canonical_depth %d, the canonical tree's is %d" % (meta["canonical_depth"], canonical_depth(nodes)))
    # ---- groups: multi-record leaves with pairs or a certificate, and the up-front list
    normals = rect_normals(M)
    groups = [("list", n_small, n - n_small, meta["list_group"] & 0xFF, meta["list_group"] >> 8)]
    if shape_ok:
        groups += [("leaf %d" % k, int(left[k]), int(count[k]), int(pairs[k]), int(cub[k])) for k in lv if pairs[k] > 0 or cub[k] != 0]
    for name, first, cnt, npairs, cert in groups:
        if 2 * npairs > cnt:
            out.add("groups.count", "%s: %d pairs in %d records" % (name, npairs, cnt))
            continue
        if cert != 0 and npairs != 3:
            out.add("groups.cuboid", "%s: certificate %d over %d pairs" % (name, cert, npairs))
        for k in range(npairs):
            a, b = int(orig[first + 2 * k]), int(orig[first + 2 * k + 1])
            if types[a] != RECTANGLE or types[b] != RECTANGLE:
                out.add("groups.rectangles", "%s: pair %d holds primitives %d, %d of types %d, %d" % (name, k, a, b, types[a], types[b]))
            # pair_test's precondition: the two world normals are opposite, so that at most one of the two one-sided rectangles faces a
            # ray (both pass its sign test only through rounding, which it handles).  The build pairs on dot < -0.9999 of the fp32
            # normalised rows; restated in float64 from M, with 1e-5 for that fp32 arithmetic (a handful of roundings of 6e-8 on unit
            # vectors and the fp32 inverse's own error, well below it for the suite's scales).
            elif float(normals[a] @ normals[b]) >= -0.9999 + 1e-5:
                out.add("groups.opposite", "%s: pair %d (primitives %d, %d): normals' dot %.9f" % (name, k, a, b, float(normals[a] @ normals[b])))
    return out


def grid_params(words):
    """GridParams' 16 words, then {bytes, list entries} (the grid.params span)"""
    w = np.ascontiguousarray(words).view(np.int32)
    f = w.view(np.float32)
    return {"min": f[0:3].copy(), "cs": f[3:6].copy(), "ics": f[6:9].copy(), "dim": w[9:12].copy(), "n_cells": int(w[12]), "rec_off4": int(w[13]),
            "items_off4": int(w[14]), "margin": float(f[15]), "bytes": int(w[16]), "entries": int(w[17])}


def grid_lists(image, gp):
    """(table [NZ, NY, NX] words, records [n_rec, 8] float32, items uint16) of a grid image"""
    img = np.ascontiguousarray(image, np.uint8)
    NX, NY, NZ = (int(d) + 2 for d in gp["dim"])
    table = img[:4 * gp["n_cells"]].view(np.uint32).reshape(NZ, NY, NX)
    recs = img[16 * gp["rec_off4"]:16 * gp["items_off4"]].view(np.float32).reshape(-1, 8)
    items = img[16 * gp["items_off4"]:].view(np.uint16)
    return table, recs, items


def check_grid(image, gp, fprims, tight, n_small):
    """the uniform grid image build_grid assembles over tree[0]'s small primitives (gp: grid_params())"""
    out = _Out()
    img = np.ascontiguousarray(image, np.uint8)
    nx, ny, nz = (int(d) for d in gp["dim"])
    NX, NY, NZ = nx + 2, ny + 2, nz + 2
    if gp["n_cells"] != NX * NY * NZ or len(img) != gp["bytes"] or not 4 * gp["n_cells"] <= 16 * gp["rec_off4"] <= 16 * gp["items_off4"] <= len(img):
        out.add("grid.layout", "n_cells %d for %d x %d x %d, offsets %d, %d in %d bytes (params say %d)" % (gp["n_cells"], nx, ny, nz, gp["rec_off4"], gp["items_off4"], len(img), gp["bytes"]))
        return out
    table, recs, items = grid_lists(img, gp)
    fp = np.asarray(fprims, np.float32).reshape(-1, 4, 4)
    orig = bits(fp[:, 3, 1].copy()).astype(np.int64)
    tb = f64(np.asarray(tight, np.float32).reshape(-1, 6))[orig[:n_small]]   # per record position
    border = np.ones((NZ, NY, NX), bool)
    border[1:-1, 1:-1, 1:-1] = False
    for z, y, x in np.argwhere(border & (table != 0)):
        out.add("grid.border", "border cell (%d, %d, %d) holds %d" % (x - 1, y - 1, z - 1, table[z, y, x]))
    gmin, cs = f64(gp["min"]), f64(gp["cs"])
    listed = np.zeros((nz, ny, nx, max(n_small, 1)), bool)
    for z, y, x in np.argwhere(~border & (table != 0)):
        r = int(table[z, y, x]) - 1
        cell = "cell (%d, %d, %d)" % (x - 1, y - 1, z - 1)
        if r >= len(recs):
            out.add("grid.record", "%s: record %d of %d" % (cell, r, len(recs)))
            continue
        fc = int(recs[r, 3:4].view(np.uint32)[0])
        first, cnt = fc & 0xFFFF, fc >> 16
        if first + cnt > len(items) or cnt < 1:
            out.add("grid.items", "%s: items [%d, %d) of %d" % (cell, first, first + cnt, len(items)))
            continue
        it = items[first:first + cnt].astype(np.int64)
        if np.any(it >= n_small):
            out.add("grid.item_range", "%s lists record %d, n_small %d" % (cell, int(it.max()), n_small))
            continue
        if len(np.unique(it)) != cnt:
            out.add("grid.item_repeat", "%s lists a record twice: %s" % (cell, it.tolist()))
        listed[z - 1, y - 1, x - 1, it] = True
        clo = gmin + cs * np.array([x - 1, y - 1, z - 1], np.float64)
        chi = gmin + cs * np.array([x, y, z], np.float64)
        ilo, ihi = np.maximum(tb[it, 0:3], clo), np.minimum(tb[it, 3:6], chi)
        real = np.all(ilo <= ihi, axis=1)   # (a shape listed through the pad alone has nothing inside the cell)
        bad = real & (np.any(f64(recs[r, 0:3]) > ilo, axis=1) | np.any(f64(recs[r, 4:7]) < ihi, axis=1))
        for j in np.flatnonzero(bad):
            out.add("grid.box", "%s: its box %s %s does not contain record %d's part of the cell %s %s" % (cell, recs[r, 0:3], recs[r, 4:7], it[j], ilo[j], ihi[j]))
    # completeness: the cells whose geometric box a primitive's tight box overlaps (closed intervals, float64, no pad)
    for p in range(n_small):
        rng = []
        for a, m in enumerate((nx, ny, nz)):
            i = np.arange(m, dtype=np.float64)
            rng.append((tb[p, a] <= gmin[a] + (i + 1) * cs[a]) & (tb[p, 3 + a] >= gmin[a] + i * cs[a]))
        need = rng[2][:, None, None] & rng[1][None, :, None] & rng[0][None, None, :]
        for z, y, x in np.argwhere(need & ~listed[:, :, :, p]):
            out.add("grid.complete", "cell (%d, %d, %d) does not list record %d, whose tight box %s touches it" % (x, y, z, p, tb[p]))
    return out


# ---------------------------------------------------------------------------------------------------------------- whitted path
def whitted_meta(words):
    """WhittedBuildMeta's nine words"""
    w = np.ascontiguousarray(words).view(np.int32)[:9]
    f = w.view(np.float32)
    return {"depth": int(w[0]), "n_recs": int(w[1]), "walk_depth": int(w[2]), "grid_lo": f[3:6].copy(), "grid_step": f[6:9].copy()}


def _leaf_minmax(first, cnt, item_lo, item_hi):
    """exact bounds of the items [first, first + cnt) for arrays of leaves (cnt <= a handful)"""
    lo, hi = item_lo[first].copy(), item_hi[first].copy()
    for k in range(1, int(cnt.max()) if len(cnt) else 0):
        j = first + np.minimum(k, cnt - 1)
        lo, hi = np.minimum(lo, item_lo[j]), np.maximum(hi, item_hi[j])
    return lo, hi


def check_records(recs, n_recs, n_items, item_lo, item_hi, leaf_max, out, tag=""):
    """the shape and containment rules of one record tree over n_items items in leaf order (triangles, instances, clusters), whose exact
    float64 bounds are item_lo / item_hi [n_items, 3].  Returns the largest number of records on a root-to-record chain (0 without
    records), or -1 when the shape is broken."""
    rc = np.asarray(recs, np.float32).reshape(-1, 4, 4)[:max(n_recs, 0)]
    if (n_recs == 0) != (n_items <= leaf_max) or len(rc) != n_recs:
        out.add(tag + "shape.n_recs", "%d records (%d present) over %d items, leaves hold %d" % (n_recs, len(rc), n_items, leaf_max))
        return -1
    if n_recs == 0:
        return 0
    link = np.stack([bits(rc[:, 0, 3].copy()), bits(rc[:, 2, 3].copy())], axis=1).astype(np.int64)   # [record, child]
    blo, bhi = f64(rc[:, [0, 2], 0:3]), f64(rc[:, [1, 3], 0:3])                                      # [record, child, axis]
    is_leaf = link < 0
    code = -1 - link
    first, cnt = code & ((1 << LEAF_SHIFT) - 1), (code >> LEAF_SHIFT) + 1
    ok = True
    out_of = ~is_leaf & (link >= n_recs)
    for r, c in np.argwhere(out_of):
        out.add(tag + "shape.links", "record %d child %d: link %d of %d records" % (r, c, link[r, c], n_recs))
        ok = False
    # reach: every record exactly once from record 0
    visits, chain, order = np.zeros(n_recs, np.int64), np.zeros(n_recs, np.int64), []
    stack = [(0, 1)]
    while stack:
        r, d = stack.pop()
        visits[r] += 1
        if visits[r] > 1:
            continue
        chain[r] = d
        order.append(r)
        for c in (0, 1):
            if not is_leaf[r, c] and link[r, c] < n_recs:
                stack.append((int(link[r, c]), d + 1))
    out.each(tag + "shape.reach", visits != 1, lambda r: "record %d reached %d times from record 0" % (r, visits[r]))
    ok = ok and bool(np.all(visits == 1))
    # leaves tile the items
    lr, lc = np.nonzero(is_leaf & (visits[:, None] > 0))
    lf, ln = first[lr, lc], cnt[lr, lc]
    bad = (ln > leaf_max) | (ln < 1) | (lf + ln > n_items)
    for k in np.flatnonzero(bad):
        out.add(tag + "shape.leaf", "record %d child %d: leaf [%d, %d) of %d items, at most %d each" % (lr[k], lc[k], lf[k], lf[k] + ln[k], n_items, leaf_max))
    cover = np.zeros(n_items + 1, np.int64)
    np.add.at(cover, np.clip(lf, 0, n_items), 1)
    np.add.at(cover, np.clip(lf + ln, 0, n_items), -1)
    cover = np.cumsum(cover)[:n_items]
    if np.any(cover != 1):
        j = int(np.flatnonzero(cover != 1)[0])
        out.add(tag + "shape.tile", "%d items are not in exactly one leaf, first: item %d in %d" % (int(np.sum(cover != 1)), j, cover[j]))
        ok = False
    if not ok or np.any(bad):
        return -1
    # containment, bottom-up: the exact bounds of the items below each child, and below each record
    sub_lo, sub_hi = np.full((n_recs, 2, 3), np.inf), np.full((n_recs, 2, 3), -np.inf)
    l_lo, l_hi = _leaf_minmax(lf, ln, item_lo, item_hi)
    sub_lo[lr, lc], sub_hi[lr, lc] = l_lo, l_hi
    for r in reversed(order):   # (children come after their parent in `order`)
        for c in (0, 1):
            if not is_leaf[r, c]:
                q = link[r, c]
                sub_lo[r, c], sub_hi[r, c] = sub_lo[q].min(axis=0), sub_hi[q].max(axis=0)
    bad = np.any(blo > sub_lo, axis=2) | np.any(bhi < sub_hi, axis=2)
    for r, c in np.argwhere(bad):
        out.add(tag + "containment.items", "record %d child %d: box %s %s does not contain the items below it, %s %s" % (r, c, rc[r, 2 * c, :3], rc[r, 2 * c + 1, :3], sub_lo[r, c], sub_hi[r, c]))
    for c in (0, 1):
        rr = np.flatnonzero(~is_leaf[:, c])
        q = link[rr, c]
        bad = np.any(blo[rr, c][:, None, :] > blo[q], axis=(1, 2)) | np.any(bhi[rr, c][:, None, :] < bhi[q], axis=(1, 2))
        for r, k in zip(rr[bad], q[bad]):
            out.add(tag + "containment.record", "record %d child %d: box does not contain record %d's boxes" % (r, c, k))
    return int(chain.max())


def check_qrecs(recs, qrecs, n_recs, grid_lo, grid_step, out, tag=""):
    """the 16-bit quantised twins of the first n_recs records"""
    rc = np.asarray(recs, np.float32).reshape(-1, 4, 4)[:n_recs]
    q = np.asarray(qrecs, np.uint32).reshape(-1, 2, 4)[:n_recs]
    if len(q) != n_recs or len(rc) != n_recs:
        out.add(tag + "quant.count", "%d quantised records for %d" % (len(q), n_recs))
        return
    link = np.stack([bits(rc[:, 0, 3].copy()), bits(rc[:, 2, 3].copy())], axis=1)
    for r, c in np.argwhere(q[:, :, 3].view(np.int32) != link):
        out.add(tag + "quant.links", "record %d child %d: link %d, the fp32 record's %d" % (r, c, q[r, c, 3].view(np.int32), link[r, c]))
    cl, ch = (q[:, :, 0:3] & 0xFFFF).astype(np.int64), (q[:, :, 0:3] >> 16).astype(np.int64)
    for r, c, a in np.argwhere(cl > ch):
        out.add(tag + "quant.order", "record %d child %d axis %d: cells %d > %d" % (r, c, a, cl[r, c, a], ch[r, c, a]))
    g0, gs = f64(grid_lo), f64(grid_step)
    plo, phi = f64(rc[:, [0, 2], 0:3]), f64(rc[:, [1, 3], 0:3])
    for r, c, a in np.argwhere(g0 + cl * gs > plo):
        out.add(tag + "quant.lower", "record %d child %d axis %d: cell %d = %.9g above the fp32 plane %.9g" % (r, c, a, cl[r, c, a], g0[a] + cl[r, c, a] * gs[a], plo[r, c, a]))
    for r, c, a in np.argwhere(g0 + ch * gs < phi):
        out.add(tag + "quant.upper", "record %d child %d axis %d: cell %d = %.9g below the fp32 plane %.9g" % (r, c, a, ch[r, c, a], g0[a] + ch[r, c, a] * gs[a], phi[r, c, a]))
    # The builder moves every plane out by a WHOLE cell (floor(c) - 1, ceil(c) + 1 of c = (plane - grid_lo) / grid_step in fp32, clamped to
    # [0, 65535]): the walk dequantises in fp32 and must stay conservative.  plane - grid_lo is one correctly rounded subtraction of fp32
    # inputs and the quotient one more rounding, so c is good to 2^-23 of its value, under 0.01 cell at 65535.  An unclamped lower cell
    # is therefore at most c - 0.99, an unclamped upper cell at least c + 0.99.
    for r, c, a in np.argwhere((cl > 0) & (g0 + (cl + 0.99) * gs > plo)):
        out.add(tag + "quant.margin", "record %d child %d axis %d: lower cell %d is less than a cell below the fp32 plane %.9g" % (r, c, a, cl[r, c, a], plo[r, c, a]))
    for r, c, a in np.argwhere((ch < 65535) & (g0 + (ch - 0.99) * gs < phi)):
        out.add(tag + "quant.margin", "record %d child %d axis %d: upper cell %d is less than a cell above the fp32 plane %.9g" % (r, c, a, ch[r, c, a], phi[r, c, a]))


def check_triangles(tris, tidx, positions, indices, out, tag="", tri_index=None, check_tidx=True):
    """the Morton-ordered triangles of one build against the mesh.  tri_index: the mesh triangles this build holds (a cluster's), default
    all of them; check_tidx: tidx carries this build's own numbering (not a cluster's).  Returns (ok, lo, hi): float64 bounds per triangle."""
    t = np.asarray(tris, np.float32).reshape(-1, 3, 4)
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    idx = np.asarray(indices).reshape(-1, 3).astype(np.int64)
    want = np.arange(len(idx)) if tri_index is None else np.asarray(tri_index, np.int64)
    which = bits(t[:, 0, 3].copy()).astype(np.int64)
    v = f64(t[:, :, 0:3])
    if len(t) != len(want) or not np.array_equal(np.sort(which), np.sort(want)):
        out.add(tag + "triangles.permutation", "tris[3i].w over %d triangles is not a permutation of the build's %d" % (len(t), len(want)))
        return False, v.min(axis=1), v.max(axis=1)
    out.each(tag + "triangles.vertices", np.any(bits(t[:, :, 0:3]) != bits(pos[idx[which]]), axis=(1, 2)),
             lambda i: "sorted triangle %d: vertices differ from triangle %d's" % (i, which[i]))
    if check_tidx and tidx is not None and int(idx.max()) < 65536 and len(t) <= 65536:
        ti = np.asarray(tidx, np.uint32).reshape(-1, 2)
        got = np.stack([ti[:, 0] & 0xFFFF, ti[:, 0] >> 16, ti[:, 1] & 0xFFFF, ti[:, 1] >> 16], axis=1).astype(np.int64)
        exp = np.concatenate([idx[which], which[:, None]], axis=1)
        out.each(tag + "triangles.tidx", np.any(got != exp, axis=1), lambda i: "sorted triangle %d: tidx %s, expected %s" % (i, got[i].tolist(), exp[i].tolist()))
    return True, v.min(axis=1), v.max(axis=1)


def check_whitted(recs, qrecs, tris, tidx, meta, positions, indices, leaf_tris=LEAF_TRIS, tag="", tri_index=None, check_tidx=True, out=None):
    """one mesh of rtgo_whitted_set_mesh, or one build of an instanced mesh in object space (meta: whitted_meta())"""
    out = _Out() if out is None else out
    ok, lo, hi = check_triangles(tris, tidx, positions, indices, out, tag, tri_index, check_tidx)
    n, n_recs = len(lo), meta["n_recs"]
    chain = check_records(recs, n_recs, n, lo, hi, leaf_tris, out, tag)
    if n_recs > 0 and qrecs is not None:
        check_qrecs(recs, qrecs, n_recs, meta["grid_lo"], meta["grid_step"], out, tag)
    if chain >= 0 and meta["walk_depth"] < chain:
        out.add(tag + "meta.walk_depth", "walk_depth %d, a chain of %d records exists" % (meta["walk_depth"], chain))
    if meta["walk_depth"] > MAX_WALK_DEPTH:
        out.add(tag + "meta.walk_depth_max", "walk_depth %d beyond %d" % (meta["walk_depth"], MAX_WALK_DEPTH))
    # the Morton hierarchy is a binary tree over n leaves: its depth lies in [ceil(log2 n), n - 1]
    if not int(np.ceil(np.log2(max(n, 1)))) <= meta["depth"] <= max(n - 1, 0):
        out.add(tag + "meta.depth", "depth %d of a binary tree over %d leaves" % (meta["depth"], n))
    return out


def mesh_info(words):
    """one mesh<k>.info span of an instanced scene"""
    w = np.ascontiguousarray(words).view(np.int32)
    keys = ("rec_base", "tri_base", "vert_base", "root", "depth", "clustered", "n_tris", "n_built")
    info = {k: int(v) for k, v in zip(keys, w[:8])}
    info["built"] = []
    for b in range(info["n_built"]):
        q = w[8 + 12 * b:8 + 12 * (b + 1)]
        info["built"].append(dict(rec0=int(q[0]), n_recs=int(q[1]), tri0=int(q[2]), meta=whitted_meta(q[3:12])))
    return info


def cluster_start(n, ncl, c):
    q, r = n // ncl, n % ncl
    return c * q + min(c, r)


def inst_walk(words):
    """the top.inst span: per entry w2o [3, 4] (float32), rec_base, tri_base, root, instance"""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1, 16)
    i = w.view(np.int32)
    return {"w2o": w[:, :12].view(np.float32).reshape(-1, 3, 4), "rec_base": i[:, 12], "tri_base": i[:, 13], "root": i[:, 14], "instance": i[:, 15]}


def check_instanced(build, meshes, instances, leaf_tris=LEAF_TRIS, max_triangles=MAX_TRIANGLES, cluster_tris=CLUSTER_TRIS):
    """an instanced scene (rtgo_whitted_set_scene): `build` = read_build(True), meshes = the mesh dicts, instances = [(transform, mesh,
    material offset)].  Mesh-level invariants carry the prefix "mesh<k>." (a cluster's "mesh<k>.c<j>."), the mid level's "mesh<k>.mid.",
    the top level's "top.".  max_triangles, cluster_tris: the library's constants (the mutation tests cluster a small mesh)."""
    out = _Out()
    clusters = np.asarray(build["clusters"], np.int32).reshape(-1, 4)
    infos, vbounds = [], []
    for k, m in enumerate(meshes):
        info = mesh_info(build["mesh%d.info" % k])
        infos.append(info)
        tag = "mesh%d." % k
        pos = np.asarray(m["positions"], np.float32).reshape(-1, 3)
        idx = np.asarray(m["indices"]).reshape(-1, 3).astype(np.int64)
        vbounds.append(f64(pos[np.unique(idx)]))
        recs_all = np.asarray(build[tag + "recs"], np.float32).reshape(-1, 4, 4)
        q_all = np.asarray(build[tag + "qrecs"], np.uint32).reshape(-1, 2, 4)
        tris, tidx = np.asarray(build[tag + "tris"], np.float32).reshape(-1, 3, 4), build[tag + "tidx"]
        n = len(idx)
        if info["n_tris"] != n or info["clustered"] != (1 if n > max_triangles else 0):
            out.add(tag + "info", "n_tris %d, clustered %d for a mesh of %d triangles" % (info["n_tris"], info["clustered"], n))
            continue
        r_at = np.concatenate([[0], np.cumsum([b["n_recs"] for b in info["built"]])]).astype(int)          # where each build's records start in recs_all
        q_at = np.concatenate([[0], np.cumsum([b["n_recs"] if b["tri0"] >= 0 else 0 for b in info["built"]])]).astype(int)
        if not info["clustered"]:
            b = info["built"][0]
            check_whitted(recs_all[r_at[0]:r_at[1]], q_all[q_at[0]:q_at[1]], tris, tidx, b["meta"], pos, idx, leaf_tris, tag, out=out)
            want_root = 0 if b["n_recs"] > 0 else -1 - ((n - 1) << LEAF_SHIFT)
            if info["root"] != want_root or b["rec0"] != info["rec_base"] or b["tri0"] != info["tri_base"]:
                out.add(tag + "info", "root %d (expected %d), build at record %d / triangle %d, bases %d / %d" % (info["root"], want_root, b["rec0"], b["tri0"], info["rec_base"], info["tri_base"]))
            continue
        # a clustered mesh: clusters of consecutive sorted triangles, each a build of its own; a mid level over them
        ncl = (n + cluster_tris - 1) // cluster_tris
        if len(info["built"]) != ncl + 1 or info["root"] <= 0:
            out.add(tag + "info", "%d builds, root %d" % (len(info["built"]), info["root"]))
            continue
        which = bits(tris[:, 0, 3].copy()).astype(np.int64)
        if not np.array_equal(np.sort(which), np.arange(n)):
            out.add(tag + "triangles.permutation", "tris[3i].w is not a permutation of the mesh's %d triangles" % n)
            continue
        c_lo, c_hi = np.zeros((ncl, 3)), np.zeros((ncl, 3))
        starts = [cluster_start(n, ncl, c) for c in range(ncl + 1)]
        for c in range(ncl):
            b, s, e = info["built"][c], starts[c], starts[c + 1]
            ctag = "%sc%d." % (tag, c)
            if b["tri0"] != info["tri_base"] + s:
                out.add(tag + "clusters.tile", "cluster %d starts at triangle %d, expected %d" % (c, b["tri0"] - info["tri_base"], s))
                continue
            check_whitted(recs_all[r_at[c]:r_at[c + 1]], q_all[q_at[c]:q_at[c + 1]], tris[s:e], None, b["meta"], pos, idx, leaf_tris, ctag,
                          tri_index=which[s:e], check_tidx=False, out=out)
            v = f64(tris[s:e, :, 0:3]).reshape(-1, 3)
            c_lo[c], c_hi[c] = v.min(axis=0), v.max(axis=0)
        # the mesh's slice of the cluster table, in the mid level's leaf order
        bits3 = info["root"] - 1
        tbase, mid_bits = bits3 >> 3, bits3 & 7
        mid = info["built"][ncl]
        table = clusters[tbase:tbase + ncl]
        if len(table) != ncl:
            out.add(tag + "clusters.table", "table rows [%d, %d) of %d" % (tbase, tbase + ncl, len(clusters)))
            continue
        by_rec = {info["built"][c]["rec0"]: c for c in range(ncl)}
        order = [by_rec.get(int(r), -1) for r in table[:, 0]]
        if sorted(order) != list(range(ncl)):
            out.add(tag + "clusters.table", "the table's record bases %s are not the clusters'" % table[:, 0].tolist()[:8])
            continue
        for pos_k, c in enumerate(order):
            want = (info["built"][c]["rec0"], info["tri_base"] + starts[c], 0 if info["built"][c]["n_recs"] > 0 else -1 - ((starts[c + 1] - starts[c] - 1) << LEAF_SHIFT))
            if tuple(int(v) for v in table[pos_k, :3]) != want:
                out.add(tag + "clusters.tile", "table row %d: %s, cluster %d is %s" % (pos_k, table[pos_k, :3].tolist(), c, list(want)))
        if (mid["n_recs"] > 0) != bool(mid_bits & MID_HAS_RECORDS) or (mid["n_recs"] == 0 and (mid_bits & 3) != ncl - 1) or mid["rec0"] != info["rec_base"]:
            out.add(tag + "mid.root", "root bits %d for a mid level of %d records over %d clusters at record %d" % (mid_bits, mid["n_recs"], ncl, mid["rec0"]))
        chain = check_records(recs_all[r_at[ncl]:r_at[ncl + 1]], mid["n_recs"], ncl, c_lo[order], c_hi[order], leaf_tris, out, tag + "mid.")
        cdepth = max(b["meta"]["walk_depth"] if b["n_recs"] > 0 else 0 for b in info["built"][:ncl])
        if chain >= 0 and info["depth"] < chain + cdepth:
            out.add(tag + "mid.meta.walk_depth", "depth %d, the mid level's chain %d + the clusters' %d" % (info["depth"], chain, cdepth))
    # ---- the top level and the InstWalk array
    iw = inst_walk(build["top.inst"])
    n_inst = len(instances)
    top = np.ascontiguousarray(build["top.meta"]).view(np.int32)
    tmeta, n_top, walk_depth = whitted_meta(top[:9]), int(top[9]), int(top[11])
    if len(iw["instance"]) != n_inst or int(top[10]) != n_inst or not np.array_equal(np.sort(iw["instance"]), np.arange(n_inst)):
        out.add("top.inst.permutation", "InstWalk.instance over %d entries is not a permutation of the %d instances" % (len(iw["instance"]), n_inst))
        return out
    i_lo, i_hi = np.zeros((n_inst, 3)), np.zeros((n_inst, 3))
    for p, i in enumerate(iw["instance"]):
        tr, mk = np.asarray(instances[i][0], np.float32).reshape(-1)[:12].astype(np.float64).reshape(3, 4), int(instances[i][1])
        if mk >= len(infos) or len(infos[mk].get("built", [])) == 0:
            continue
        info = infos[mk]
        if (int(iw["rec_base"][p]), int(iw["tri_base"][p]), int(iw["root"][p])) != (info["rec_base"], info["tri_base"], info["root"]):
            out.add("top.inst.bases", "entry %d (instance %d): bases %d, %d root %d, mesh %d has %d, %d root %d" % (p, i, iw["rec_base"][p], iw["tri_base"][p], iw["root"][p], mk, info["rec_base"], info["tri_base"], info["root"]))
        w = vbounds[mk] @ tr[:, :3].T + tr[:, 3]
        i_lo[p], i_hi[p] = w.min(axis=0), w.max(axis=0)
    chain = check_records(build["top.recs"], n_top, n_inst, i_lo, i_hi, leaf_tris, out, "top.")
    mesh_depth = max([f["depth"] for f in infos] + [0])
    if chain >= 0 and walk_depth < max(chain + mesh_depth, 1):
        out.add("top.meta.walk_depth", "walk_depth %d, the top level's chain %d + the deepest mesh's %d" % (walk_depth, chain, mesh_depth))
    if tmeta["n_recs"] != n_top:
        out.add("top.meta.n_recs", "the build reported %d records, the top level keeps %d" % (tmeta["n_recs"], n_top))
    return out


def check_analytic(build, types, M, aabb=None):
    """everything rtgo_set_scene built: both fast-walk structures, the tight boxes and the grid when there is one.  `build` =
    read_build(False); aabb: the caller's boxes (None: the device's own, which read_build returns)."""
    out = _Out()
    n = len(types)
    box = build["aabb"] if aabb is None else aabb
    if aabb is not None and not np.array_equal(bits(np.asarray(aabb, np.float32).reshape(-1, 6)), bits(build["aabb"])):
        out.add("aabb.given", "the device's boxes are not the caller's")
    metas = {}
    for k in (0, 1):
        if len(build["tree%d.fprims" % k]) == 0:
            continue
        metas[k] = meta = build_meta(build["tree%d.meta" % k])
        if k == 0:
            out += ["tree0." + v for v in check_tight(build["tight"], box, types, M, meta)]
        out += ["tree%d." % k + v for v in check_fast_tree(build["tree%d.fnodes" % k], build["tree%d.fprims" % k], meta, build["prims"], build["tight"], box,
                                                           types, M, BIG_FRAC[k], build["nodes"])]
    gp = grid_params(build["grid.params"])
    if int(np.ascontiguousarray(build["scene.info"]).view(np.int32)[3]):
        out += check_grid(build["grid.image"], gp, build["tree0.fprims"], build["tight"], metas[0]["n_small"])
    return out


def check_mesh(build, mesh, leaf_tris=LEAF_TRIS):
    """everything rtgo_whitted_set_mesh built (`build` = read_build(True))"""
    w = np.ascontiguousarray(build["meta"]).view(np.int32)
    meta = whitted_meta(w[:9])
    out = check_whitted(build["recs"], build["qrecs"], build["tris"], build["tidx"], meta, mesh["positions"], mesh["indices"], leaf_tris)
    counts = np.ascontiguousarray(build["counts"]).view(np.int32)
    if int(counts[0]) != meta["n_recs"] or int(counts[1]) != max(meta["walk_depth"], 1) or int(w[9]) != len(np.asarray(mesh["indices"]).reshape(-1, 3)):
        out.add("meta.kept", "the context keeps n_recs %d, walk_depth %d, %d triangles; the build reported %d, %d" % (counts[0], counts[1], w[9], meta["n_recs"], meta["walk_depth"]))
    if not np.array_equal(bits(build["grid"].view(np.float32)), bits(np.concatenate([meta["grid_lo"], meta["grid_step"]]))):
        out.add("meta.kept", "the context's grid differs from the build's")
    return out


# ---------------------------------------------------------------------------------------------------------------- fixtures
def numpy_grid(tight, dims, n_small=None):
    """build_grid's binning restated in numpy for given cell counts `dims` (the cost search is not restated), over tight boxes in record
    order: a mutation target for the tests of check_grid, NOT a reference for the device.  Returns (image, grid_params dict)."""
    t = np.asarray(tight, np.float32).reshape(-1, 6)
    ns = len(t) if n_small is None else n_small
    t = t[:ns]
    f = np.float32
    lo, hi = t[:, 0:3].min(axis=0), t[:, 3:6].max(axis=0)
    ext = (hi - lo).astype(f)
    dims = np.asarray(dims, np.int64)
    reach = f(4) * f(np.abs(np.concatenate([lo, hi])).max())
    pad = f(f(2e-3) * (ext / dims.astype(f)).max() + f(1e-4) * reach)
    gmin = (lo - f(2) * pad).astype(f)
    gcs = ((ext + f(4) * pad) / dims.astype(f)).astype(f)
    gics = (f(1) / gcs).astype(f)
    NX, NY, NZ = (int(d) + 2 for d in dims)
    lists = {}
    a0 = np.clip(np.floor((t[:, 0:3] - pad - gmin) * gics).astype(np.int64), 0, None)
    a1 = np.minimum(np.floor((t[:, 3:6] + pad - gmin) * gics).astype(np.int64), dims - 1)
    for p in range(ns):
        for z in range(a0[p, 2], a1[p, 2] + 1):
            for y in range(a0[p, 1], a1[p, 1] + 1):
                for x in range(a0[p, 0], a1[p, 0] + 1):
                    lists.setdefault(((z + 1) * NY + (y + 1)) * NX + (x + 1), []).append(p)
    n_cells = NX * NY * NZ
    total = sum(len(l) for l in lists.values())
    table_bytes = (n_cells * 4 + 15) // 16 * 16
    rec_bytes = len(lists) * 32
    nbytes = (table_bytes + rec_bytes + total * 2 + 31) // 32 * 32
    img = np.zeros(nbytes, np.uint8)
    cells, recs, items = img[:4 * n_cells].view(np.uint32), img[table_bytes:table_bytes + rec_bytes].view(np.float32).reshape(-1, 8), img[table_bytes + rec_bytes:].view(np.uint16)
    at = 0
    for r, k in enumerate(sorted(lists)):
        l = lists[k]
        cells[k] = r + 1
        kk = np.array([k % NX - 1, (k // NX) % NY - 1, k // (NX * NY) - 1]).astype(f)
        recs[r, 0:3] = np.maximum((t[l, 0:3] - pad).min(axis=0), gmin + gcs * kk - pad)
        recs[r, 4:7] = np.minimum((t[l, 3:6] + pad).max(axis=0), gmin + gcs * (kk + f(1)) + pad)
        recs[r, 3:4].view(np.uint32)[0] = at | (len(l) << 16)
        items[at:at + len(l)] = l
        at += len(l)
    gp = {"min": gmin, "cs": gcs, "ics": gics, "dim": dims.astype(np.int32), "n_cells": n_cells, "rec_off4": table_bytes // 16,
          "items_off4": (table_bytes + rec_bytes) // 16, "margin": float(f(0.5) * pad), "bytes": nbytes, "entries": total}
    return img, gp


def record(path, build, **inputs):
    """store a read_build() dict and the scene's inputs as one .npz (keys 'build/<span>' and 'in/<name>'; None inputs are left out)"""
    data = {"build/" + k: v for k, v in build.items()}
    data.update({"in/" + k: np.asarray(v) for k, v in inputs.items() if v is not None})
    np.savez_compressed(path, **data)


def load(path):
    """record()'s file back: (build dict, inputs dict)"""
    z = np.load(path)
    return ({k[6:]: z[k] for k in z.files if k.startswith("build/")}, {k[3:]: z[k] for k in z.files if k.startswith("in/")})


def sphere300(offset=(0.0, 0.0, 0.0)):
    """the sphere of tests/whitted_scene.build(n_lat=6, n_lon=30) alone: 300 triangles over its own vertices, moved by `offset` in fp32"""
    import whitted_scene
    m = whitted_scene.build(n_lat=6, n_lon=30)
    ix = m["indices"][m["tri_material"] == 1]
    v0, v1 = int(ix.min()), int(ix.max()) + 1
    return {"positions": (m["positions"][v0:v1] + np.asarray(offset, np.float32)).astype(np.float32), "normals": m["normals"][v0:v1],
            "indices": (ix - v0).astype(np.uint32), "tri_material": None, "materials": m["materials"]}
