"""Rays aimed where a cull that is not conservative changes the answer, and the meshes they are aimed at (numpy only).

tests/test_whitted_trace_rays.py compares the triangle walks with the oracle on rays a float64 brute force finds clear: pixel centres and
uniformly random rays, which meet no vertex, no edge, no silhouette and no box face.  The families here are those rays.  Every generator is
seeded, takes at most MAX_RAYS rays a call and returns (o [n, 3] float32, d [n, 3] float32, not normalised, tag [n] of dtype TAG); an aimed
ray meets its target at t = 1.  tests/test_oracle_adversarial_rays.py checks that each family is what it says, in float64;
tests/test_whitted_adversarial_rays.py holds the device to the oracle's brute force on all of them.

  edge, vertex   the target is a point of an edge two triangles share / a vertex, rounded to float32.  piercing: the direction lies in a
                 cone around minus the mean of the adjacent face normals (the ray enters the solid there); grazing: it is perpendicular to
                 that mean (tangent at the silhouette)
  box_face       axis-parallel: two direction components are exactly +0.0f or -0.0f, and the origin has one coordinate of a vertex, bit for
                 bit -- for half of the rays a vertex that attains the mesh's extreme on that axis, so the ray lies in the face plane of a
                 box that is tight there; both signs of the free component
  in_plane       d = a e1 + b e2 of one triangle for small integers a, b, where that sum is exact in float32 (det = 0 for that triangle),
                 through the triangle's interior
  far            piercing edge and vertex rays from 1e2 and 1e4 extents away
  on_surface     the origin IS a vertex or an edge point, tmin = 1e-4, directions into both half spaces: the occlusion rays' situation
  interior       the control: points well inside triangles, from either side"""
import numpy as np

import trace_rays_ref as R
import whitted_big_meshes as BM
import whitted_instances as WI

F = np.float32
MAX_RAYS = 2048
TMIN, TMIN_SURFACE, TMAX = F(0.01), F(1e-4), F(1e16)
TAG = np.dtype([("family", "U12"), ("variant", "U12"), ("elem", "<i4"), ("closed", "?"), ("dist", "<f8"), ("axis", "<i4"), ("shared", "<i4"),
                ("target", "<f4", (3,))])
# rtgo_hit as raytracingo_amd.capi.HIT_DTYPE lays it out (the oracle's hits are written in the device's form, to be compared as bytes)
HIT = np.dtype([("t", "<f4"), ("prim", "<i4"), ("instance", "<i4"), ("u", "<f4"), ("v", "<f4"), ("n", "<f4", (3,))])
EYE = np.eye(3, 4, dtype=F)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def sliver_fan(n=32, aspect=1e4, seed=3):
    """n triangles of aspect `aspect` that share their sharp vertex: spokes of length 1, 1 / aspect apart at the rim, lifted out of
    their common plane by a tenth of that and turned into a generic position (no edge along an axis)"""
    rng = np.random.RandomState(seed)
    th = np.arange(n + 1) / aspect
    rim = np.stack([np.cos(th), np.sin(th), 0.1 / aspect * np.sin(1.7 * np.arange(n + 1))], axis=1)
    p = np.concatenate([[[0.0, 0.0, 0.0]], rim]) @ WI.rotation(rng).T + [0.21, -0.13, 0.17]
    tris = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 2 + np.arange(n)], axis=1)
    return {"positions": p.astype(F), "normals": None, "indices": tris.astype(np.uint32), "tri_material": None}


def plus_one_triangle(mesh):
    """mesh with one more triangle below it (the first size a clustered mesh has)"""
    tri = np.array([[-1.5, -0.4, -1.5], [0.0, -0.4, 1.5], [1.5, -0.4, -1.5]], F)
    nv = len(mesh["positions"])
    return {"positions": np.concatenate([mesh["positions"], tri]), "normals": None,
            "indices": np.concatenate([mesh["indices"], np.array([[nv, nv + 1, nv + 2]], np.uint32)]), "tri_material": None}


def _bare(mesh):
    return {"positions": mesh["positions"], "normals": None, "indices": mesh["indices"], "tri_material": None}


def _octahedron():
    return WI.octahedron(0.5)


def _half_octahedron():
    m = WI.octahedron(0.5)
    return dict(m, indices=m["indices"][:4])


def _torus256():
    return _bare(BM.displaced_torus(16, 8, texcoords=False))


def _torus256_far():
    m = _torus256()
    return dict(m, positions=(m["positions"] + F(1e4)).astype(F))


def _torus8192():
    return _bare(BM.displaced_torus(64, 64, texcoords=False))


# name -> builder.  half_octahedron: one leaf, no records; grid: a box of zero thickness; torus256_far: ulp(1e4) ~ 1e-3 is above the
# build's pad of 1e-4 extent; torus8192: the last size of one build; torus8193: the first clustered size (instanced scenes only)
MESHES = {"octahedron": _octahedron, "half_octahedron": _half_octahedron, "torus256": _torus256, "grid": lambda: BM.flat_sheet(16),
          "slivers": sliver_fan, "torus256_far": _torus256_far, "torus8192": _torus8192, "torus8193": lambda: plus_one_triangle(_torus8192())}
CLOSED = ("octahedron", "torus256")


def twist(mesh):
    """the vertices turned about the y axis through the mesh's centre by an angle that grows to a half turn with height (tools/
    whitted_refit_perf.py's `twist`): what a refit's boxes fit worst"""
    p = mesh["positions"].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    c = 0.5 * (lo + hi)
    a = np.pi * (p[:, 1] - lo[1]) / max(hi[1] - lo[1], 1e-9)
    q = p - c
    return (np.stack([np.cos(a) * q[:, 0] + np.sin(a) * q[:, 2], q[:, 1], -np.sin(a) * q[:, 0] + np.cos(a) * q[:, 2]], axis=1) + c).astype(F)


# ---- topology ----------------------------------------------------------------------------------------------------------------------
def topology(mesh):
    """what the aimed families need of a mesh: corners P [T, 3, 3] and unit face normals fn [T, 3] in float64, the edges two triangles
    share (shared [E, 2] vertices, shared_faces [E, 2]), per used vertex its faces (vfaces: dict) and whether they close a fan around it
    (closed: set), and the largest extent of the bounds"""
    pos = np.asarray(mesh["positions"], F).astype(np.float64)
    ix = np.asarray(mesh["indices"], np.int64).reshape(-1, 3)
    P = pos[ix]
    fn = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    edges, vfaces, vedges = {}, {}, {}
    for f, (a, b, c) in enumerate(ix.tolist()):
        for x, y in ((a, b), (b, c), (c, a)):
            e = (min(x, y), max(x, y))
            edges.setdefault(e, []).append(f)
            vedges.setdefault(x, set()).add(e)
            vedges.setdefault(y, set()).add(e)
        for x in (a, b, c):
            vfaces.setdefault(x, []).append(f)
    two = sorted(e for e, fs in edges.items() if len(fs) == 2)
    closed = {v for v, es in vedges.items() if all(len(edges[e]) == 2 for e in es)}
    return {"pos": pos, "ix": ix, "P": P, "fn": fn, "shared": np.array(two, np.int64).reshape(-1, 2),
            "shared_faces": np.array([edges[e] for e in two], np.int64).reshape(-1, 2), "vfaces": vfaces, "closed": closed,
            "used": np.array(sorted(vfaces), np.int64), "ext": float((pos[ix.reshape(-1)].max(0) - pos[ix.reshape(-1)].min(0)).max())}


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _mean_normal(topo, faces):
    m = topo["fn"][faces].sum(0)
    return topo["fn"][faces[0]] if np.linalg.norm(m) < 1e-6 else m / np.linalg.norm(m)


def _perp(rng, axis):
    """a unit vector perpendicular to each row of `axis` (unit), uniform in that plane"""
    r = rng.normal(size=axis.shape)
    r -= (r * axis).sum(-1, keepdims=True) * axis
    return _unit(r)


def _cone(rng, axis, half):
    """unit vectors within `half` radians of each row of `axis` (unit)"""
    ang = half * np.sqrt(rng.rand(len(axis), 1))
    return np.cos(ang) * axis + np.sin(ang) * _perp(rng, axis)


def _aim(target, w, dist):
    """rays that meet `target` (float32) at t = 1 from `dist` away along -w: the origin rounded to float32, then d = target - o rounded
    (each component within 2^-24 relative, so the ray passes its target within 2^-24 |d|)"""
    t64 = np.asarray(target, F).astype(np.float64)
    o = (t64 - np.reshape(dist, (-1, 1)) * w).astype(F)
    return o, (t64 - o.astype(np.float64)).astype(F)


def _tags(n, family, variant, elem, closed, dist, target, axis=-1, shared=-1):
    tag = np.zeros(n, TAG)
    tag["family"], tag["variant"], tag["elem"], tag["closed"], tag["dist"], tag["target"] = family, variant, elem, closed, dist, target
    tag["axis"], tag["shared"] = axis, shared
    return tag


def _directions(rng, topo, faces_of, variant):
    """piercing / grazing directions for targets whose adjacent faces are faces_of[k]"""
    nbar = np.array([_mean_normal(topo, f) for f in faces_of])
    if variant == "grazing":
        return _perp(rng, nbar)
    assert variant == "piercing", variant
    w = _cone(rng, -nbar, 0.4)
    for k, f in enumerate(faces_of):   # every adjacent face is entered from its front: else straight down the mean normal
        if (topo["fn"][f] @ w[k]).max() > -0.05:
            w[k] = -nbar[k]
    return w


def _pick_edges(rng, topo, n):
    e = rng.randint(0, len(topo["shared"]), n)
    s = np.where(rng.rand(n) < 0.125, 0.5, rng.uniform(0.02, 0.98, n))[:, None]
    a, b = topo["pos"][topo["shared"][e, 0]], topo["pos"][topo["shared"][e, 1]]
    return e, ((1.0 - s) * a + s * b).astype(F), [topo["shared_faces"][k] for k in e]


def _pick_vertices(rng, topo, n):
    closed = np.array(sorted(topo["closed"]), np.int64)
    v = topo["used"][rng.randint(0, len(topo["used"]), n)]
    if len(closed):   # three in four at a vertex whose triangles close a fan around it
        v = np.where(rng.rand(n) < 0.75, closed[rng.randint(0, len(closed), n)], v)
    return v, topo["pos"][v].astype(F), [np.array(topo["vfaces"][k], np.int64) for k in v.tolist()]


def edge(mesh, n, seed, variant="piercing", dist=2.0, topo=None, family="edge"):
    """n rays at points of shared edges from `dist` extents away"""
    assert n <= MAX_RAYS
    topo = topo or topology(mesh)
    rng = np.random.RandomState(seed)
    e, target, faces = _pick_edges(rng, topo, n)
    o, d = _aim(target, _directions(rng, topo, faces, variant), dist * topo["ext"])
    return o, d, _tags(n, family, variant, e, True, dist, target)


def vertex(mesh, n, seed, variant="piercing", dist=2.0, topo=None, family="vertex"):
    """n rays at vertices from `dist` extents away (tag `closed`: the vertex's triangles close a fan around it)"""
    assert n <= MAX_RAYS
    topo = topo or topology(mesh)
    rng = np.random.RandomState(seed)
    v, target, faces = _pick_vertices(rng, topo, n)
    o, d = _aim(target, _directions(rng, topo, faces, variant), dist * topo["ext"])
    return o, d, _tags(n, family, variant, v, np.isin(v, sorted(topo["closed"])), dist, target)


def interior(mesh, n, seed, dist=2.0, topo=None):
    """the control: n rays at points well inside triangles (barycentrics from Dirichlet(4, 4, 4)), within 0.4 rad of the face normal's
    opposite or, every other ray, of the normal itself.  On a mesh whose other families are all unclear by construction (a flat sheet)
    these are the rays float64 and float32 must agree on."""
    assert n <= MAX_RAYS
    topo = topo or topology(mesh)
    rng = np.random.RandomState(seed)
    f = rng.randint(0, len(topo["P"]), n)
    target = (rng.dirichlet([4, 4, 4], n)[:, :, None] * topo["P"][f]).sum(1).astype(F)
    side = np.where(np.arange(n) % 2 == 0, -1.0, 1.0)[:, None]
    o, d = _aim(target, _cone(rng, side * topo["fn"][f], 0.4), dist * topo["ext"])
    return o, d, _tags(n, "interior", "", f, False, dist, target)


def far(mesh, n, seed, topo=None):
    """piercing edge and vertex rays from 1e2 and 1e4 extents away, a quarter of n each"""
    assert n <= MAX_RAYS
    topo = topo or topology(mesh)
    q = [n // 4, n // 4, n // 4, n - 3 * (n // 4)]
    parts = [edge(mesh, q[0], seed, "piercing", 1e2, topo, "far"), edge(mesh, q[1], seed + 1, "piercing", 1e4, topo, "far"),
             vertex(mesh, q[2], seed + 2, "piercing", 1e2, topo, "far"), vertex(mesh, q[3], seed + 3, "piercing", 1e4, topo, "far")]
    for k, p in enumerate(parts):
        p[2]["variant"] = ("edge", "vertex")[k // 2]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def box_face(mesh, n, seed, dist=2.0, topo=None):
    """n axis-parallel rays.  Free axis `axis` (tag), direction +-(the distance) there, +-0.0 on the other two; the origin has coordinate
    `shared` of vertex `elem` bit for bit -- for every other ray a vertex that attains the mesh's minimum or maximum on that axis -- and on
    the third axis either that vertex's coordinate too (one ray in four: the ray goes through the vertex) or a point up to 0.3 extents off"""
    assert n <= MAX_RAYS
    topo = topo or topology(mesh)
    rng = np.random.RandomState(seed)
    pos = topo["pos"].astype(F)
    used = topo["used"]
    o, d = np.zeros((n, 3), F), np.zeros((n, 3), F)
    tag = _tags(n, "box_face", "", 0, False, dist, 0.0)
    for k in range(n):
        a = int(rng.randint(3))
        b = (a + 1 + int(rng.randint(2))) % 3
        c = 3 - a - b
        if k % 2 == 0:
            ext = used[np.argmin(pos[used, b])] if rng.rand() < 0.5 else used[np.argmax(pos[used, b])]
            v = int(ext)
        else:
            v = int(used[rng.randint(len(used))])
        sign = 1.0 if rng.rand() < 0.5 else -1.0
        o[k, b] = pos[v, b]
        o[k, c] = pos[v, c] if rng.rand() < 0.25 else F(float(pos[v, c]) + rng.uniform(-0.3, 0.3) * topo["ext"])
        o[k, a] = F(float(pos[v, a]) - sign * dist * topo["ext"])
        d[k, a] = F(float(pos[v, a]) - float(o[k, a]))
        d[k, b] = F(-0.0) if rng.rand() < 0.5 else F(0.0)
        d[k, c] = F(-0.0) if rng.rand() < 0.5 else F(0.0)
        tag["variant"][k], tag["elem"][k], tag["axis"][k], tag["shared"][k] = "xyz"[a] + ("+" if sign > 0 else "-"), v, a, b
        tag["target"][k] = (o[k].astype(np.float64) + d[k].astype(np.float64)).astype(F)
    return o, d, tag


_COMBOS = [(1, 0), (0, 1), (1, -1), (1, 1), (2, 1), (1, 2), (2, -1), (-1, 2), (3, 1), (1, 3), (3, -1), (-1, 3), (3, 2), (2, 3), (3, -2), (-2, 3)]


def in_plane(mesh, n, seed, dist=2.0, topo=None):
    """up to n rays in a triangle's plane: d = a e1 + b e2 with (a, b) from a short list of small integers, kept where that sum (exact in
    float64: the corners are float32) is a float32 vector as it stands, either sign -- det = e1 . (d x e2) is then zero for triangle `elem`
    -- from about `dist` extents before a point of the triangle's interior.  Fewer than n where too few triangles have such a sum."""
    assert n <= MAX_RAYS
    topo = topo or topology(mesh)
    rng = np.random.RandomState(seed)
    P = topo["P"]
    o, d, elem, target = [], [], [], []
    for _ in range(20 * n):
        if len(o) == n:
            break
        f = int(rng.randint(len(P)))
        e1, e2 = P[f, 1] - P[f, 0], P[f, 2] - P[f, 0]
        for j in rng.permutation(len(_COMBOS)):
            d64 = (_COMBOS[j][0] * e1 + _COMBOS[j][1] * e2) * (1.0 if rng.rand() < 0.5 else -1.0)
            if np.array_equal(d64.astype(F).astype(np.float64), d64) and np.linalg.norm(d64) > 0:
                break
        else:
            continue
        q = rng.dirichlet([2, 2, 2]) @ P[f]
        steps = np.round(dist * topo["ext"] / np.linalg.norm(d64))
        o.append((q - steps * d64).astype(F))
        d.append(d64.astype(F))
        elem.append(f)
        target.append(q.astype(F))
    m = len(o)
    return (np.array(o, F).reshape(m, 3), np.array(d, F).reshape(m, 3),
            _tags(m, "in_plane", "", np.array(elem, np.int32), False, dist, np.array(target, F).reshape(m, 3)))


def on_surface(mesh, n, seed, topo=None):
    """n rays that START on a vertex (every other one) or on a point of a shared edge: directions up to 1.35 rad off the mean normal
    (variant `out`) or off its opposite (`in`), of a length between a quarter of and a whole extent.  For tmin = TMIN_SURFACE."""
    assert n <= MAX_RAYS
    topo = topo or topology(mesh)
    rng = np.random.RandomState(seed)
    nv = (n + 1) // 2
    v, tv, fv = _pick_vertices(rng, topo, nv)
    e, te, fe = _pick_edges(rng, topo, n - nv)
    target = np.concatenate([tv, te])
    nbar = np.array([_mean_normal(topo, f) for f in fv + fe])
    side = np.where(np.arange(n) % 4 < 2, 1.0, -1.0)
    w = _cone(rng, side[:, None] * nbar, 1.35)
    d = (w * rng.uniform(0.25, 1.0, (n, 1)) * topo["ext"]).astype(F)
    tag = _tags(n, "on_surface", "", np.concatenate([v, e]), False, 0.0, target)
    tag["variant"] = np.where(side > 0, "out", "in")
    return target.copy(), d, tag


def family_rays(mesh, n=256, seed=100):
    """every family over one mesh, n rays each (in_plane: up to n): {name: (o, d, tag, tmin)} in a fixed order"""
    topo = topology(mesh)
    out = {}
    for k, variant in enumerate(("piercing", "grazing")):
        out["edge/" + variant] = edge(mesh, n, seed + k, variant, topo=topo) + (TMIN,)
        out["vertex/" + variant] = vertex(mesh, n, seed + 10 + k, variant, topo=topo) + (TMIN,)
    out["box_face"] = box_face(mesh, n, seed + 20, topo=topo) + (TMIN,)
    out["in_plane"] = in_plane(mesh, n, seed + 30, topo=topo) + (TMIN,)
    out["far"] = far(mesh, n, seed + 40, topo=topo) + (TMIN,)
    out["on_surface"] = on_surface(mesh, n, seed + 50, topo=topo) + (TMIN_SURFACE,)
    out["interior"] = interior(mesh, n // 2, seed + 60, topo=topo) + (TMIN,)
    return out


def all_rays(fams):
    """family_rays' families back to back: o, d, tmin [n], family name [n]"""
    o = np.concatenate([f[0] for f in fams.values()])
    d = np.concatenate([f[1] for f in fams.values()])
    tmin = np.concatenate([np.full(len(f[0]), f[3], F) for f in fams.values()])
    name = np.concatenate([np.full(len(f[0]), k, "U16") for k, f in fams.items()])
    return o, d, tmin, name


def to_world(transform, o, d):
    """object-space rays through a 3x4 object-to-world transform (float64, rounded to float32 once)"""
    M = WI.as34(np.asarray(transform, F))
    return (o.astype(np.float64) @ M[:, :3].T + M[:, 3]).astype(F), (d.astype(np.float64) @ M[:, :3].T).astype(F)


def placements(seed=31):
    """name -> 3x4 transform: a rotation, a non-uniform scale under a rotation, a mirror, and uniform scales of 1e-3 and of 1e3 (the last
    1e4 from the origin)"""
    rng = np.random.RandomState(seed)
    return {"rotated": WI.transform(WI.rotation(rng), [0.4, 0.3, -0.2]),
            "scaled": WI.transform(WI.rotation(rng) @ np.diag([1.7, 0.45, 1.1]), [-0.5, 0.2, 0.6]),
            "mirrored": WI.transform(WI.mirror(rng), [0.1, -0.6, 0.3]),
            "milli": WI.transform(1e-3 * WI.rotation(rng), [0.3, -0.2, 0.1]),
            "kilo": WI.transform(1e3 * WI.rotation(rng), [1e4, -1e4, 1e4])}


# ---- references --------------------------------------------------------------------------------------------------------------------
def oracle_hits(sc, o, d, tmin, tmax=TMAX):
    """oracle_py.InstancedScene.trace for every ray, as rtgo_whitted_trace_rays writes its hits (HIT; a miss: t = tmax, prim -1, the
    rest zero)"""
    tmin, tmax = np.broadcast_to(F(tmin), len(o)), np.broadcast_to(F(tmax), len(o))
    out = np.zeros(len(o), HIT)
    for k in range(len(o)):
        h = sc.trace(o[k], d[k], float(tmin[k]), float(tmax[k]))
        if h is None:
            out["t"][k], out["prim"][k] = tmax[k], -1
        else:
            out["instance"][k], out["prim"][k], out["t"][k], out["u"][k], out["v"][k] = h
    return out


def differing(a, b):
    """the rows in which two HIT arrays differ in any bit"""
    return np.nonzero((a.view(np.uint32).reshape(len(a), -1) != b.view(np.uint32).reshape(len(b), -1)).any(axis=1))[0]


def box_pad(mesh):
    """whitted::box_pad over a mesh, in float32 as the builds compute it: 1e-4 of the largest extent + 1e-6, at least 2^-22 of the largest
    coordinate"""
    used = np.asarray(mesh["positions"], F)[np.asarray(mesh["indices"], np.int64).reshape(-1)]
    lo, hi = used.min(0), used.max(0)
    maxext, reach = (hi - lo).max(), np.maximum(np.abs(lo), np.abs(hi)).max()
    return max(F(F(maxext * F(1e-4)) + F(1e-6)), F(reach * F(2.3841858e-7)))


def is_phantom(c, ray, instance, prim, t):
    """Whether the hit (instance, prim, t) the intersector reports on ray `ray` of case `c` is a PHANTOM: in the instance's object space
    and in float64, the ray does not meet the triangle's own bounds, grown by the builds' pad, anywhere in [tmin, t (1 + 1e-6)].
    tri_intersect accepts such hits where |det| is rounding noise -- a ray within rounding of the triangle's plane, a triangle of aspect
    1e4 -- and u, v, t are quotients of noise.  Every box of every tree contains its triangles' padded bounds, so a ray that meets those
    before t meets every box on the way to the triangle before t, and no conservative cull may lose the hit; a phantom's ray misses the
    triangle's own leaf-level bounds, and a walk finds the hit only if the ray happens to cross the larger boxes above."""
    tr, mi, _ = c["inst"][instance]
    M = WI.as34(np.asarray(tr, F))
    Binv = np.linalg.inv(M[:, :3])
    mesh = c["meshes"][int(mi)]
    oo, od = (c["o"][ray].astype(np.float64) - M[:, 3]) @ Binv.T, c["d"][ray].astype(np.float64) @ Binv.T
    P = np.asarray(mesh["positions"], F).astype(np.float64)[np.asarray(mesh["indices"], np.int64).reshape(-1, 3)[prim]]
    pad = float(box_pad(mesh))
    lo, hi = P.min(0) - pad, P.max(0) + pad
    a, b = float(c["tmin"][ray]), float(t) * (1 + 1e-6)
    for k in range(3):
        if od[k] == 0.0:
            if not lo[k] <= oo[k] <= hi[k]:
                return True
            continue
        t0, t1 = (lo[k] - oo[k]) / od[k], (hi[k] - oo[k]) / od[k]
        a, b = max(a, min(t0, t1)), min(b, max(t0, t1))
    return bool(a > b)


def only_phantoms_lost(sc, c, ray, got, limit=64):
    """Ray `ray` of case `c`, on which the device's record `got` is not the brute force's.  Walks the oracle's hits (sc: the case's
    InstancedScene without cull) in ascending t, each query starting at the t of the hit before, up to the device's: None if every hit
    on the way is a phantom and the next one is the device's record bit for bit (or, for a device miss, none is left) -- else what is
    wrong."""
    o, d, tmin, tmax = c["o"][ray], c["d"][ray], float(c["tmin"][ray]), float(TMAX)
    for _ in range(limit):
        h = sc.trace(o, d, tmin, tmax)
        if h is None:
            return None if got["prim"] < 0 else "the device reports a hit the brute force does not have beyond t = %r" % tmin
        rec = np.zeros(1, HIT)
        rec["instance"], rec["prim"], rec["t"], rec["u"], rec["v"] = h
        if got["prim"] >= 0 and rec.tobytes() == np.asarray(got).reshape(1).view(HIT).tobytes():
            return None
        if not is_phantom(c, ray, h[0], h[1], h[2]):
            return "lost a hit inside its triangle's padded bounds: instance %d triangle %d t %r" % (h[0], h[1], h[2])
        tmin = h[2]
    return "more than %d phantom hits on one ray" % limit


def _mt64(P, o, d):
    """Moeller-Trumbore over triangles P [T, 3, 3] and rays o, d [n, 3] in float64: t, u, v, det [n, T] (NaN where det = 0) and the
    condition number kappa = max(|o - P0|, |e1|) |d| max(|e1|, |e2|) / |det| of the barycentrics"""
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    pv = np.cross(d[:, None, :], e2[None])
    det = (e1[None] * pv).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(det != 0, 1.0 / det, np.nan)
        tv = o[:, None, :] - P[None, :, 0]
        u = (tv * pv).sum(-1) * inv
        qv = np.cross(tv, e1[None])
        v = (d[:, None, :] * qv).sum(-1) * inv
        t = (e2[None] * qv).sum(-1) * inv
        l1, l2 = np.linalg.norm(e1, axis=1)[None], np.linalg.norm(e2, axis=1)[None]
        kappa = np.maximum(np.linalg.norm(tv, axis=-1), l1) * np.linalg.norm(d, axis=1)[:, None] * np.maximum(l1, l2) / np.abs(det)
    return t, u, v, det, kappa


RESOLVE = 32 * 2.0 ** -24


def brute64(meshes, inst, o, d, tmin, chunk=64):
    """float64 brute force over every (instance, triangle), object-space Moeller-Trumbore as trace_rays_ref.clear_triangle_rays states it.
    Returns dict(hit, clear, strict, resolved [n] bool, key [n, 2] = the winner's (instance, triangle), t [n] = its t (inf on a miss),
    kappa [n] = its condition number).
    clear: clear_triangle_rays' rule -- it hits, the runner-up is at least 1e-5 relative further, the winner's barycentrics are at least
    1e-5 inside.
    strict: clear, and no (instance, triangle) whose plane the ray meets before t (1 + 1e-5) of the winner is met within 1e-5 of its
    border, inside or outside (smallest barycentric in [-1e-5, 1e-5]): float64 may just miss a triangle at a grazed vertex that float32
    accepts.
    resolved: strict with every 1e-5 above replaced by max(1e-5, RESOLVE kappa) of the triangle in question, and no triangle near the
    ray whose det float32 cannot sign.  1e-5 is a margin in barycentric units, and float32 resolves a barycentric to about 13 roundings
    of 2^-24 times kappa = max(|o - P0|, |e1|) |d| max(|e1|, |e2|) / |det| (u = (tv . pv) / det: three roundings in each component of
    pv, one in tv, five in the dot product, as many again in det, one each for the reciprocal and the product; 1 - u - v doubles it; 32
    covers both).  From 2 extents at a well shaped triangle kappa is about 10 and 1e-5 stands; from 1e4 extents, or at a triangle of
    aspect 1e4, RESOLVE kappa is 1e-2 and more, and a margin of 1e-5 says nothing about what float32 decides."""
    n = len(o)
    tmin = np.broadcast_to(np.float64(tmin), n)
    hit, clear, strict, resolved = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    key, tw, kappa_w = np.full((n, 2), -1, np.int64), np.full(n, np.inf), np.zeros(n)
    prep = []
    for tr, mi, _ in inst:
        M = WI.as34(np.asarray(tr, F))
        mesh = meshes[int(mi)]
        P = np.asarray(mesh["positions"], F).astype(np.float64)[np.asarray(mesh["indices"], np.int64).reshape(-1, 3)]
        centre = P.mean(axis=1)
        prep.append((M[:, 3], np.linalg.inv(M[:, :3]), P, centre, np.linalg.norm(P - centre[:, None], axis=2).max(axis=1)))
    for s in range(0, n, chunk):
        rows = slice(s, min(s + chunk, n))
        o64, d64, tm = np.asarray(o[rows], np.float64), np.asarray(d[rows], np.float64), tmin[rows, None]
        m = len(o64)
        tb, t2, mb, kw = np.full(m, np.inf), np.full(m, np.inf), np.zeros(m), np.zeros(m)
        tg, tg_r, unsigned = np.full(m, np.inf), np.full(m, np.inf), np.zeros(m, bool)
        kb = np.full((m, 2), -1, np.int64)
        for ii, (shift, Binv, P, centre, radius) in enumerate(prep):
            oo, od = (o64 - shift) @ Binv.T, d64 @ Binv.T
            with np.errstate(invalid="ignore", divide="ignore"):
                t, u, v, det, kappa = _mt64(P, oo, od)
                margin = np.minimum(np.minimum(u, v), 1 - u - v)
                ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tm)
                ahead = t > tm * (1 - 1e-5)
                grazed = (np.abs(margin) <= 1e-5) & ahead
                grazed_r = (np.abs(margin) <= np.maximum(1e-5, RESOLVE * kappa)) & ahead
                # a triangle whose det float32 cannot sign, within whose bounding sphere the ray's line passes
                off = np.linalg.norm(np.cross(centre[None] - oo[:, None, :], od[:, None, :]), axis=-1) / np.linalg.norm(od, axis=1)[:, None]
                unsigned |= (~(RESOLVE * kappa < 1.0) & (off <= radius[None] * 1.001)).any(axis=1)
            tg = np.minimum(tg, np.where(grazed, t, np.inf).min(axis=1))
            tg_r = np.minimum(tg_r, np.where(grazed_r, t, np.inf).min(axis=1))
            t = np.where(ok, t, np.inf)
            k = np.arange(m)
            b = np.argmin(t, axis=1)           # (the first of equal minima: the lowest triangle)
            t_first = t[k, b]
            t[k, b] = np.inf
            t_second = t.min(axis=1) if t.shape[1] > 1 else np.full(m, np.inf)
            better = t_first < tb
            t2 = np.where(better, np.minimum(tb, t_second), np.minimum(t2, t_first))
            mb = np.where(better, margin[k, b], mb)
            kw = np.where(better, kappa[k, b], kw)
            kb[better] = np.stack([np.full(m, ii), b], 1)[better]
            tb = np.where(better, t_first, tb)
        thr = np.maximum(1e-5, RESOLVE * kw)
        hit[rows] = np.isfinite(tb)
        clear[rows] = hit[rows] & (t2 >= tb * (1 + 1e-5)) & (mb >= 1e-5)
        strict[rows] = clear[rows] & ~(tg < tb * (1 + 1e-5))
        resolved[rows] = hit[rows] & (t2 >= tb * (1 + thr)) & (mb >= thr) & ~(tg_r < tb * (1 + thr)) & ~unsigned
        key[rows], tw[rows], kappa_w[rows] = kb, tb, kw
    return {"hit": hit, "clear": clear, "strict": strict, "resolved": resolved & strict, "key": key, "t": tw, "kappa": kappa_w}


def strict_clear(meshes, inst, o, d, tmin=0.01):
    """clear_triangle_rays with brute64's stricter rule: (hit [n], strictly clear [n], key [n, 2])"""
    b = brute64(meshes, inst, o, d, tmin)
    return b["hit"], b["strict"], b["key"]


def entry64(mesh, o, d, window=1e-3, eps=1e-12):
    """whether float64 finds a triangle of `mesh` (object space) within `window` of t = 1, the aimed rays' target.  (eps: a ray whose
    origin and direction were representable as they stood meets its vertex exactly, where float64's own rounding decides the
    barycentrics' signs.)"""
    P = np.asarray(mesh["positions"], F).astype(np.float64)[np.asarray(mesh["indices"], np.int64).reshape(-1, 3)]
    out = np.zeros(len(o), bool)
    for s in range(0, len(o), 64):
        with np.errstate(invalid="ignore"):
            t, u, v = _mt64(P, np.asarray(o[s:s + 64], np.float64), np.asarray(d[s:s + 64], np.float64))[:3]
            out[s:s + 64] = ((u >= -eps) & (v >= -eps) & (u + v <= 1 + eps) & (np.abs(t - 1.0) <= window)).any(axis=1)
    return out


# ---- the cases both test modules share ---------------------------------------------------------------------------------------------
WAYS = ("identity", "three", "milli", "kilo")
_cases, _references = {}, {}


def case(name, way, n=256):
    """mesh `name` placed the way `way` says, and every family's rays over it in world space (built once a session):
    identity  one identity instance (what rtgo_whitted_set_mesh draws too)
    three     a rotated, a non-uniformly scaled and a mirrored instance in one scene, every third ray aimed at each
    milli, kilo   one instance under a uniform scale of 1e-3 / of 1e3
    twisted   the mesh with its vertices twisted, one identity instance, the rays aimed at the twisted mesh
    Returns dict(meshes, inst, o, d, tmin [n], family [n], fams: the object-space families)."""
    if (name, way) not in _cases:
        mesh = MESHES[name]()
        if way == "twisted":
            mesh = dict(mesh, positions=twist(mesh))
        fams = family_rays(mesh, n)
        o, d, tmin, family = all_rays(fams)
        place = placements()
        trs = {"identity": [EYE], "twisted": [EYE], "three": [place["rotated"], place["scaled"], place["mirrored"]]}.get(way) or [place[way]]
        for k, tr in enumerate(trs):
            if tr is not EYE:
                o[k::len(trs)], d[k::len(trs)] = to_world(tr, o[k::len(trs)], d[k::len(trs)])
        _cases[name, way] = {"meshes": [mesh], "inst": [(tr, 0, 0) for tr in trs], "o": o, "d": d, "tmin": tmin, "family": family, "fams": fams}
    return _cases[name, way]


def reference(oracle, name, way):
    """the oracle's brute force (no cull) over case(name, way), as HIT records (computed once a session, never changed)"""
    if (name, way) not in _references:
        c = case(name, way)
        hits = oracle_hits(oracle.InstancedScene(c["meshes"], c["inst"], WI.materials(), cull=False), c["o"], c["d"], c["tmin"])
        hits.setflags(write=False)
        _references[name, way] = hits
    return _references[name, way]


# ---- the lattice -------------------------------------------------------------------------------------------------------------------
LATTICE_COLOURS = [(0.9, 0.1, 0.1), (0.1, 0.9, 0.1), (0.1, 0.1, 0.9), (0.9, 0.9, 0.1), (0.9, 0.1, 0.9), (0.1, 0.9, 0.9), (0.95, 0.95, 0.95),
                   (0.3, 0.3, 0.3)]


def lattice_primaries(cam, W, H):
    """the primary rays of subframe 0 of a W x H launch, operation for operation (raygen: no jitter at subframe 0, the pixel's corner:
    dx = 2 (x / W) - 1, d = (U dx + V dy + W) scaled by 1 / sqrt(d . d), float32, one rounding each)"""
    cam = np.asarray(cam, F)
    eye, U, V, Wv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    x, y = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    dx = (F(2) * (x / F(W)) - F(1))[..., None]
    dy = (F(2) * (y / F(H)) - F(1))[..., None]
    d = ((U * dx) + (V * dy)) + Wv
    dot = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d = d * (F(1) / np.sqrt(dot))[..., None]
    return np.tile(eye, (W * H, 1)), d.reshape(-1, 3).astype(F)


def lattice_mesh(cam, W, H, seed, band=0.04):
    """A mesh whose every vertex lies on a subframe-0 primary ray of a W x H launch of camera `cam` (eye, U, V, W; W and H powers of two,
    so that dx_i = 2 i / W - 1 and dy_j are exact): positions[j W + i] = fl32(eye + s_ij (U dx_i + V dy_j + W)) with s_ij within `band` of
    1 (a smooth ridge plus seeded noise: the sheet shadows itself under a light from the side).  Two triangles a cell, the diagonal
    alternating, wound to face the eye, no vertex normals.  The eight triangles that can meet at a vertex have eight different materials
    (cell parity x half), of well separated base colours: another triangle at a pixel is another colour, far beyond 1e-4.  Returns a mesh
    dict with materials, two point lights (one beside the eye, one low at the side) and a miss colour."""
    assert W & (W - 1) == 0 and H & (H - 1) == 0
    rng = np.random.RandomState(seed)
    c = np.asarray(cam, F).astype(np.float64)
    eye, U, V, Wv = c[0:3], c[3:6], c[6:9], c[9:12]
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    dx, dy = 2.0 * (i / W) - 1.0, 2.0 * (j / H) - 1.0
    s = 1.0 + band * (0.6 * np.sin(5.0 * dx + 2.0 * dy) * np.cos(3.0 * dy) + 0.4 * (2.0 * rng.rand(H, W) - 1.0))
    pos = eye + s[..., None] * (U * dx[..., None] + V * dy[..., None] + Wv)
    ci, cj = np.meshgrid(np.arange(W - 1), np.arange(H - 1))
    a = cj * W + ci
    b, cc, dd = a + 1, a + W + 1, a + W
    even = ((ci + cj) % 2 == 0)[..., None]
    t0 = np.where(even, np.stack([a, b, cc], -1), np.stack([a, b, dd], -1))
    t1 = np.where(even, np.stack([a, cc, dd], -1), np.stack([b, cc, dd], -1))
    tris = np.stack([t0, t1], axis=2).reshape(-1, 3)
    tmat = (np.stack([np.zeros_like(a), np.ones_like(a)], axis=2) + (2 * (ci % 2) + 4 * (cj % 2))[..., None]).reshape(-1)
    mats = np.array([list(rgb) + [1.0, 0.0, 0.7] for rgb in LATTICE_COLOURS], F)
    lights = np.zeros((2, 8), F)
    lights[0] = [1.0, 0.95, 0.9, 2.0] + list(eye + 0.3 * U + 0.4 * V) + [0]
    lights[1] = [0.7, 0.8, 1.0, 3.0] + list(eye + 0.93 * Wv + 1.6 * U + 0.2 * V) + [0]
    return {"positions": pos.reshape(-1, 3).astype(F), "normals": None, "indices": tris.astype(np.uint32), "tri_material": tmat.astype(np.uint32),
            "materials": mats, "lights": lights, "miss": np.array([0.02, 0.03, 0.05], F)}


LATTICE = dict(W=64, H=32, eye=(0.4, 1.1, 3.0), lookat=(0.1, 0.2, 0.0), seed=17)


def lattice(oracle):
    """the camera and the lattice mesh of the render tests: a 64 x 32 launch"""
    import whitted_scene
    cam = whitted_scene.camera(oracle, LATTICE["W"], LATTICE["H"], eye=LATTICE["eye"], lookat=LATTICE["lookat"])
    return cam, lattice_mesh(cam, LATTICE["W"], LATTICE["H"], LATTICE["seed"])
