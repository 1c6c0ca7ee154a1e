"""The adversarial ray families of tests/adversarial_rays.py on the CPU: each family is what it says (judged in float64 or exactly), the
oracle's own cull changes no answer on any of them, the float32 oracle names the float64 winner wherever float64 is strictly clear, and
a census of the rays on which plain float32 Moeller-Trumbore (oracle_tri_intersect, the device's tri_intersect) lets a ray through a
shared edge or vertex.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import adversarial_rays as AR
import trace_rays_ref as R
import whitted_instances as WI

F = np.float32
AIM = 4 * 2.0 ** -24     # an aimed ray passes its target within this much of |o| + |target| (o and d = target - o are rounded once each)
# the resolved rays (brute64) of a mesh's families together: what the committed seeds give on the CPU (identity placement) is, in MESHES'
# order, 190, 150, 502, 128, 129, 810, 111, 186; the floors are nine tenths of that, so that a family that lost its rays shows
RESOLVED_FLOOR = {"octahedron": 171, "half_octahedron": 135, "torus256": 451, "grid": 115, "slivers": 116, "torus256_far": 729, "torus8192": 99,
                  "torus8193": 167}
BIG_STEP = 4             # the float64 brute force of the strict-clear rule takes every fourth ray of the meshes beyond 8000 triangles


def line_distance(o, d, p):
    o, d, p = (np.asarray(a, F).astype(np.float64) for a in (o, d, p))
    return np.linalg.norm(np.cross(p - o, d), axis=1) / np.linalg.norm(d, axis=1)


def exact_det(P, d):
    """e1 . (d x e2) of one triangle in rational arithmetic"""
    p0, p1, p2 = ([Fraction(float(x)) for x in row] for row in P)
    dd = [Fraction(float(x)) for x in d]
    e1, e2 = [a - b for a, b in zip(p1, p0)], [a - b for a, b in zip(p2, p0)]
    pv = [dd[1] * e2[2] - dd[2] * e2[1], dd[2] * e2[0] - dd[0] * e2[2], dd[0] * e2[1] - dd[1] * e2[0]]
    return sum(a * b for a, b in zip(e1, pv))


# ---- the generators ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(AR.MESHES))
def test_every_family_is_what_it_says(name):
    mesh = AR.MESHES[name]()
    topo = AR.topology(mesh)
    fams = AR.family_rays(mesh, 256)
    again = AR.family_rays(mesh, 256)
    pos32 = np.asarray(mesh["positions"], F)
    for k, (o, d, tag, tmin) in fams.items():
        assert o.dtype == F and d.dtype == F and 0 < len(o) <= AR.MAX_RAYS and len(o) == len(d) == len(tag), k
        assert np.isfinite(o).all() and np.isfinite(d).all() and (d != 0).any(axis=1).all(), k
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again[k][:2], (o, d))), (k, "not seeded")
    for k in ("edge/piercing", "edge/grazing", "vertex/piercing", "vertex/grazing", "far"):
        o, d, tag, _ = fams[k]
        dist = line_distance(o, d, tag["target"])
        bound = AIM * (np.linalg.norm(o.astype(np.float64), axis=1) + np.linalg.norm(tag["target"].astype(np.float64), axis=1))
        assert (dist <= bound).all(), (k, float((dist / bound).max()))
        # the targets themselves: a vertex bit for bit, a point within rounding of its edge
        vert = (tag["family"] == "vertex") | ((tag["family"] == "far") & (tag["variant"] == "vertex"))
        assert np.array_equal(tag["target"][vert].view(np.uint32), pos32[tag["elem"][vert]].view(np.uint32)), k
        ea, eb = topo["pos"][topo["shared"][tag["elem"][~vert], 0]], topo["pos"][topo["shared"][tag["elem"][~vert], 1]]
        off = np.linalg.norm(np.cross(tag["target"][~vert].astype(np.float64) - ea, eb - ea), axis=1) / np.linalg.norm(eb - ea, axis=1)
        assert (off <= 2.0 ** -23 * np.abs(topo["pos"]).max()).all(), k
        w = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
        faces = [topo["shared_faces"][e] if not v else np.array(topo["vfaces"][e]) for e, v in zip(tag["elem"].tolist(), vert.tolist())]
        nbar = np.array([AR._mean_normal(topo, f) for f in faces])
        along = (w * nbar).sum(1)
        if k.endswith("grazing"):
            # (w was perpendicular in float64; o and d = target - o are rounded from it, each to 2^-24 of its size)
            assert (np.abs(along) <= 1e-6 + bound / np.linalg.norm(d.astype(np.float64), axis=1)).all(), (k, "not tangent")
        else:
            assert (along < -0.5).all(), (k, "not against the mean normal")
            # a piercing ray enters: float64 finds the surface at t = 1 (at a vertex only where its triangles close a fan around it;
            # from 1e4 extents the aim is off by up to 2^-24 of that, 6e-4 extents, wider than a sliver)
            judged = tag["closed"] & (tag["dist"] < (1e3 if name == "slivers" else 1e9))
            assert judged.sum() >= len(o) // 4 or (k.startswith("vertex") and not topo["closed"]), (k, "too few rays whose entry can be judged")
            assert AR.entry64(mesh, o, d)[judged].all(), (k, "float64 finds no entry at t = 1")
    assert set(fams["far"][2]["dist"].tolist()) == {1e2, 1e4} and (fams["edge/piercing"][2]["dist"] == 2.0).all()
    # box_face
    o, d, tag, _ = fams["box_face"]
    n = np.arange(len(o))
    a, b = tag["axis"], tag["shared"]
    c = 3 - a - b
    assert (d[n, b] == 0).all() and (d[n, c] == 0).all() and (d[n, a] != 0).all()
    assert np.signbit(d[n, b]).any() and (~np.signbit(d[n, b])).any() and np.signbit(d[n, c]).any() and (~np.signbit(d[n, c])).any(), "both zeros"
    assert (d[n, a] > 0).sum() > len(o) // 4 and (d[n, a] < 0).sum() > len(o) // 4, "both signs of the free component"
    assert np.array_equal(o[n, b].view(np.uint32), pos32[tag["elem"], b].view(np.uint32)), "the shared coordinate"
    used = pos32[topo["used"]]
    extreme = (o[n, b] == used.min(0)[b]) | (o[n, b] == used.max(0)[b])
    assert extreme[0::2].all() and (o[n, c] == pos32[tag["elem"], c]).sum() >= len(o) // 8
    assert set(a.tolist()) == {0, 1, 2}
    # in_plane
    o, d, tag, _ = fams["in_plane"]
    assert len(o) >= 128, len(o)
    P = topo["P"][tag["elem"]]
    area2 = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
    for k in range(len(o)):
        det = exact_det(P[k], d[k])
        assert abs(det) < Fraction(2.0 ** -40 * float(np.linalg.norm(d[k].astype(np.float64))) * float(area2[k])), (k, float(det))
    q = tag["target"].astype(np.float64) - P[:, 0]
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    uv = np.array([np.linalg.lstsq(np.stack([x, y], 1), z, rcond=None)[0] for x, y, z in zip(e1, e2, q)])
    assert (uv.min(1) > 0.0).all() and (uv.sum(1) < 1.0).all(), "through the interior"
    assert (line_distance(o, d, tag["target"]) <= AIM * 64 * (np.linalg.norm(o, axis=1) + 1.0)).all()
    # on_surface
    o, d, tag, tmin = fams["on_surface"]
    assert tmin == AR.TMIN_SURFACE and np.array_equal(o.view(np.uint32), tag["target"].view(np.uint32))
    nv = (len(o) + 1) // 2
    assert np.array_equal(o[:nv].view(np.uint32), pos32[tag["elem"][:nv]].view(np.uint32)), "on a vertex"
    assert set(tag["variant"].tolist()) == {"in", "out"} and (tag["variant"][:nv] == "in").any() and (tag["variant"][nv:] == "out").any()
    faces = [np.array(topo["vfaces"][e]) for e in tag["elem"][:nv].tolist()] + [topo["shared_faces"][e] for e in tag["elem"][nv:].tolist()]
    along = (d.astype(np.float64) * np.array([AR._mean_normal(topo, f) for f in faces])).sum(1)
    assert ((along > 0) == (tag["variant"] == "out")).all()


def test_the_meshes_are_the_regimes_they_stand_for():
    m = {k: f() for k, f in AR.MESHES.items()}
    assert [len(m[k]["indices"]) for k in AR.MESHES] == [8, 4, 256, 512, 32, 256, 8192, 8193]
    assert (m["grid"]["positions"][:, 1] == 0).all()
    P = m["slivers"]["positions"].astype(np.float64)[m["slivers"]["indices"].astype(np.int64)]
    longest = np.max([np.linalg.norm(P[:, i] - P[:, j], axis=1) for i, j in ((0, 1), (1, 2), (2, 0))], axis=0)
    height = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1) / longest
    assert (longest / height > 0.9e4).all() and len(set(m["slivers"]["indices"][:, 0].tolist())) == 1
    far = m["torus256_far"]["positions"]
    ext = float((far.max(0) - far.min(0)).max())
    assert np.spacing(far.min()) > 1e-4 * ext + 1e-6, "the build's pad is below one ulp of the coordinates"
    assert (far.min(0) - F(1e-4 * ext + 1e-6) == far.min(0)).all(), "lo - pad rounds back to lo"
    tw = AR.twist(m["torus256"])
    assert tw.shape == m["torus256"]["positions"].shape and np.abs(tw - m["torus256"]["positions"]).max() > 0.5


# ---- the oracle's cull against its brute force ---------------------------------------------------------------------------------------
CULL_CASES = [(name, "identity") for name in AR.MESHES] + [(name, way) for name in AR.CLOSED for way in ("three", "milli", "kilo")] + [("torus256", "twisted")]


@pytest.mark.parametrize("name,way", CULL_CASES)
def test_the_oracles_cull_changes_no_answer(oracle, name, way):
    """miss or hit, and (instance, triangle, t, u, v) bit for bit, on every ray of every family"""
    c = AR.case(name, way)
    brute = AR.reference(oracle, name, way)
    culled = AR.oracle_hits(oracle.InstancedScene(c["meshes"], c["inst"], WI.materials(), cull=True), c["o"], c["d"], c["tmin"])
    diff = AR.differing(culled, brute)
    for fam in c["fams"]:
        m = c["family"] == fam
        print("%s, %s, %-15s %4d rays, %4d hit, %d differ between cull and brute force" % (name, way, fam, m.sum(), (brute["prim"][m] >= 0).sum(), m[diff].sum()))
    assert len(diff) == 0, diff[:10]
    assert len({i for i in brute["instance"][brute["prim"] >= 0].tolist()}) == len(c["inst"]), "an instance no ray meets"


# ---- strictly clear rays ---------------------------------------------------------------------------------------------------------------
def test_brute64_states_clear_as_clear_triangle_rays_does(oracle):
    c = AR.case("torus256", "three")
    b = AR.brute64(c["meshes"], c["inst"], c["o"], c["d"], c["tmin"])
    for tmin in (AR.TMIN, AR.TMIN_SURFACE):
        m = c["tmin"] == tmin
        hit, clear, key = R.clear_triangle_rays(c["meshes"], c["inst"], c["o"][m], c["d"][m], float(tmin))
        assert np.array_equal(hit, b["hit"][m]) and np.array_equal(clear, b["clear"][m]) and np.array_equal(key[hit], b["key"][m][hit])
    assert (b["resolved"] <= b["strict"]).all() and (b["strict"] <= b["clear"]).all() and (b["clear"] <= b["hit"]).all()
    assert b["resolved"].any() and (b["strict"] & ~b["resolved"]).any() and (b["clear"] & ~b["strict"]).any()
    s = AR.strict_clear(c["meshes"], c["inst"], c["o"][:64], c["d"][:64], float(AR.TMIN))
    assert np.array_equal(s[0], b["hit"][:64]) and np.array_equal(s[1], b["strict"][:64]) and np.array_equal(s[2], b["key"][:64])


@pytest.mark.parametrize("name", list(AR.MESHES))
def test_the_oracle_names_the_float64_winner_where_float32_resolves_the_margins(oracle, name):
    """On every ray that is strictly clear AND resolved (adversarial_rays.brute64) the float32 oracle names the float64 winner.  The
    strict rule's 1e-5 alone does not carry to every family: measured here with the committed seeds, the oracle names another triangle
    (or none) on 77 of torus256's 149 strictly clear `far` rays, on 427 of the sliver fan's 990 strictly clear rays and on 1 in-plane
    ray of torus256 -- rays from 1e2 and 1e4 extents, triangles of aspect 1e4 and a ray in a triangle's own plane, where float32
    resolves a barycentric to 1e-3 .. 1e-1, not to 1e-5.  Those counts are printed per family and held to nothing; the resolved rule
    sets them aside from the formats' precision, never from what the oracle answers."""
    c = AR.case(name, "identity")
    step = BIG_STEP if len(c["meshes"][0]["indices"]) > 8000 else 1
    rows = np.arange(0, len(c["o"]), step)
    got = AR.reference(oracle, name, "identity")[rows]
    b = AR.brute64(c["meshes"], c["inst"], c["o"][rows], c["d"][rows], c["tmin"][rows])
    other = (got["prim"] != b["key"][:, 1]) | (got["instance"] != np.maximum(b["key"][:, 0], 0))
    s = b["resolved"]
    assert (s <= b["strict"]).all()
    for fam in c["fams"]:
        m = c["family"][rows] == fam
        print("%s, %-15s %4d rays: float64 hits %4d, clear %4d (another triangle in float32: %3d), strictly clear %4d = %.3f (%3d), resolved %4d = %.3f (%d)"
              % (name, fam, m.sum(), b["hit"][m].sum(), b["clear"][m].sum(), (b["clear"] & other)[m].sum(), b["strict"][m].sum(), b["strict"][m].mean(),
                 (b["strict"] & other)[m].sum(), s[m].sum(), s[m].mean(), (s & other)[m].sum()))
    print("%s: %d strictly clear and %d resolved rays of %d" % (name, b["strict"].sum(), s.sum(), len(rows)))
    assert s.sum() >= RESOLVED_FLOOR[name], (s.sum(), RESOLVED_FLOOR[name])
    assert not (s & other).any(), np.nonzero(s & other)[0][:10]
    assert (np.abs(got["t"][s] - b["t"][s]) <= np.maximum(1e-5, AR.RESOLVE * b["kappa"][s]) * b["t"][s]).all()   # (t's roundings are the barycentrics')


# ---- how watertight float32 Moeller-Trumbore is NOT --------------------------------------------------------------------------------------
def test_leak_census(oracle):
    """Piercing rays at shared edges and at vertices of the two closed meshes, from 2 and from 100 extents: float64 finds the entry at
    t = 1 on every one (asserted: the census counts what it says); the float32 oracle reports nothing within 1e-3 of it on a share of
    them (printed, DESIGN.md section 4: a measurement of oracle_tri_intersect / tri_intersect, held to no threshold)."""
    for name in AR.CLOSED:
        mesh = AR.MESHES[name]()
        topo = AR.topology(mesh)
        sc = oracle.InstancedScene([mesh], [(AR.EYE, 0, 0)], WI.materials(), cull=False)
        for gen in (AR.edge, AR.vertex):
            for dist in (2.0, 100.0):
                o, d, tag = gen(mesh, 1024, 7, "piercing", dist, topo)
                assert tag["closed"].all() and AR.entry64(mesh, o, d).all(), (name, gen.__name__, dist)
                window = AR.oracle_hits(sc, o, d, F(1.0 - 1e-3), F(1.0 + 1e-3))
                leaks = (window["prim"] < 0).sum()
                print("leak census: %-10s %-6s from %5.0f extents: %4d of %d rays (%.1f %%)" % (name, gen.__name__, dist, leaks, len(o), 100.0 * leaks / len(o)))


# ---- the lattice ---------------------------------------------------------------------------------------------------------------------
def test_lattice_mesh(oracle):
    W, H = AR.LATTICE["W"], AR.LATTICE["H"]
    cam, mesh = AR.lattice(oracle)
    o, d = AR.lattice_primaries(cam, W, H)
    pos, ix = mesh["positions"], mesh["indices"].astype(np.int64)
    assert len(pos) == W * H and len(ix) == 2 * (W - 1) * (H - 1)
    # every vertex lies on its pixel's subframe-0 primary
    dist = line_distance(o, d, pos)
    assert (dist <= AIM * (np.linalg.norm(o.astype(np.float64), axis=1) + np.linalg.norm(pos.astype(np.float64), axis=1))).all(), float(dist.max())
    # the triangles at a vertex have different materials, of well separated colours
    at = {}
    for f, tri in enumerate(ix.tolist()):
        for v in tri:
            at.setdefault(v, []).append(int(mesh["tri_material"][f]))
    assert all(len(set(ms)) == len(ms) for ms in at.values()) and max(len(ms) for ms in at.values()) == 8
    rgb = mesh["materials"][:, :3].astype(np.float64)
    assert len(rgb) >= 4 and min(np.abs(rgb[i] - rgb[j]).max() for i in range(len(rgb)) for j in range(i)) >= 0.5
    # lattice_primaries is raygen: the oracle's frame misses exactly where its brute force misses these rays
    acc, img, rays = oracle.whitted_render(mesh, cam, W, H, 1)
    sc = oracle.InstancedScene([mesh], [(AR.EYE, 0, 0)], mesh["materials"], cull=False)
    hits = AR.oracle_hits(sc, o, d, AR.TMIN)
    miss = (acc[..., :3] == mesh["miss"]).all(axis=-1).reshape(-1)
    assert np.array_equal(miss, hits["prim"] < 0)
    inner = np.ones((H, W), bool)
    inner[:, -1] = inner[-1, :] = False
    print("lattice: %d of %d pixels hit, %d of the %d inside the sheet's border; %d occlusion rays" % ((~miss).sum(), W * H, (~miss)[inner.reshape(-1)].sum(), inner.sum(), rays["rays_occlusion"]))
    assert (~miss).sum() >= 0.8 * W * H
    # part of the sheet shadows the rest under the second light, and the first one reaches most of it
    for li, (lo, hi) in enumerate(((0.0, 0.3), (0.1, 0.9))):
        L = mesh["lights"][li, 4:7].astype(np.float64)
        to = L - pos.astype(np.float64)
        ln = np.linalg.norm(to, axis=1, keepdims=True)
        sh = AR.oracle_hits(sc, pos, (to / ln).astype(F), F(1e-3), (ln[:, 0] - 1e-3).astype(F))
        share = (sh["prim"] >= 0).mean()
        print("lattice: light %d is occluded at %.3f of the vertices" % (li, share))
        assert lo <= share <= hi, (li, share)
