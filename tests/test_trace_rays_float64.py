"""rtgo_trace_rays on the MI355X held to tests/analytic_ref64.py, the float64 reference written from the geometry, with the constants
tests/test_oracle_float64.py measured from the oracle on the CPU: random scenes of all four primitive types under plain and sheared model
matrices, non-unit directions, origins inside primitives; every form of the scene set-up; the hand-placed rays; axis-parallel rays; a
primitive beyond the box rule's +-50 seed; the acceptance window; what the build wrote (boxes, inverses); and the render kernels' fast walk
against the canonical walk on the same matrices."""
import numpy as np
import pytest

import analytic_ref64 as A
import trace_rays_ref as R
from test_oracle_float64 import (INVERSE_BOUND, NAMES, N_BOUND_SINE, T_BOUND_UNITS, check_known, check_units, deviations, inverse_residual,
                                 one_primitive)
from test_trace_rays import Knob, same_hits

pytestmark = pytest.mark.gpu

TMIN, TMAX = np.float32(1e-3), np.float32(1e16)
UNCLEAR_CAP = 0.15
# name: (primitives, half-width of the box of centres, rays, seed)
# (the unclear share of a 48-primitive scene of this family runs from 0.09 to 0.16 over seeds 13 .. 20; the cap is a condition on the
# inputs, so the seed is one that meets it with room: 0.099 here)
SCENES = {"k16a": (16, 8.0, 4096, 11), "k16b": (16, 8.0, 4096, 12), "k48": (48, 12.0, 4096, 16), "k1": (1, 8.0, 4096, 14)}
# the scenes that are also rendered: scales in [1/2, 2] and centres within +-4, so that with the floor, the ceiling and cornell's eye at
# (0, 0, 14) the launch stays inside the far-field guard (D^2 smax / smin^2 <= 8000 over the quadrics) and the timed kernel IS the fast walk
RENDERED = {"r16a": (16, 4.0, 2048, 31, (0.5, 2.0)), "r16b": (16, 4.0, 2048, 32, (0.5, 2.0))}
LARGE = (600, 25.0, 2048, 15)      # beyond RTGO_MAX_PRIMS: rtgo_set_large_scene alone, walked from global memory
FORMS = ("device boxes", "oracle boxes", "large scene")


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import capi as m
    m.load()
    return m


def materials(n):
    mat = np.zeros((n, 10), np.float32)
    mat[:, 0:3], mat[:, 6] = 0.6, 1.0
    return mat


def random_scene(n, box, n_rays, seed, scales=(0.25, 4.0), near=False):
    """n primitives, type i % 4, plain and sheared alternating within each type, centres in the box of +-`box`; n_rays rays, each aimed
    at a random point of the 1.2 x unit cube's image of a random primitive, from origins in 1.3 x the box (near: a quarter inside the
    aimed-at primitive, the rest 1 to 30 units from its centre, as in the one-primitive families), |d| log-uniform in [0.1, 10]"""
    rng = np.random.RandomState(seed)
    types = np.arange(n) % 4
    M = np.stack([A.random_matrix(rng, bool((i // 4 + i) % 2), spread=box, scales=scales) for i in range(n)])
    target = rng.randint(0, n, n_rays)
    origins = rng.uniform(-1.3 * box, 1.3 * box, (n_rays, 3))
    o, d = np.zeros((n_rays, 3), np.float32), np.zeros((n_rays, 3), np.float32)
    for p in range(n):
        rows = np.nonzero(target == p)[0]
        o[rows], d[rows] = A.aimed_rays(rng, types[p], M[p], len(rows), None if near else origins[rows])
    return types, M, o, d


def oracle_boxes(oracle, M):
    bb = np.zeros((len(M), 6), np.float32)
    for i in range(len(M)):
        oracle.lib().oracle_prim_aabb(oracle.fptr(np.ascontiguousarray(M[i], np.float32)), oracle.fptr(bb[i]))
    return bb


def context(capi, form, types, M, boxes=None):
    ctx = capi.Context(0)
    if form == "large scene":
        ctx.set_large_scene(types, M, materials(len(types)), None)
    else:
        ctx.set_scene(types, M, materials(len(types)), boxes if form == "oracle boxes" else None)
    return ctx


def scene_case(capi, oracle, name, _cases):
    """the scene, its rays, the float64 reference, the oracle's brute force and one context per form with the hits it gave, made once"""
    if name not in _cases:
        types, M, o, d = random_scene(*SCENES[name])
        ref = A.closest(types, M, o, d, TMIN, TMAX)
        sc = oracle.scene_from_tables(types, M, materials(len(types)), np.zeros((0, 16), np.float32), np.zeros(12, np.float32))
        brute = np.zeros(len(o), capi.HIT_DTYPE)
        for k in range(len(o)):
            p, t, n, _ = R.brute(oracle, sc, o[k], d[k], TMIN, TMAX)
            brute["prim"][k], brute["t"][k], brute["n"][k] = p, t, n
        brute["instance"] = np.where(brute["prim"] >= 0, -1, 0)
        boxes = oracle_boxes(oracle, M)
        rays = capi.make_rays(o, d, TMIN, TMAX)
        ctxs = {form: context(capi, form, types, M, boxes) for form in FORMS}
        with Knob(RTGO_TRACE_MODE=None, RTGO_TRACE_BLOCKS=None):
            hits = {form: ctxs[form].trace_rays(rays) for form in FORMS}
        _cases[name] = dict(types=types, M=M, o=o, d=d, ref=ref, brute=brute, boxes=boxes, rays=rays, ctx=ctxs, hits=hits)
    return _cases[name]


@pytest.fixture(scope="module")
def cases(capi, oracle):
    """scene_case by name; the contexts are closed when the module is done"""
    made = {}
    yield lambda name: scene_case(capi, oracle, name, made)
    for c in made.values():
        for ctx in c["ctx"].values():
            ctx.close()


def hold_to_reference(what, capi, types, M, o, d, ref, hits, tmax=TMAX, cap=UNCLEAR_CAP):
    """the assertions on clear rays: the reference's primitive; hit point and normal within the CPU-measured bounds of the winner's type;
    a miss carries tmax.  Prints the unclear share and the deviations per type."""
    clear = ref["clear"]
    share = 1 - clear.mean()
    hit = clear & (ref["prim"] >= 0)
    dt, dn = np.zeros(len(o)), np.zeros(len(o))
    figures = []
    wrong = np.nonzero(clear & (hits["prim"] != ref["prim"]))[0]
    agree = hit & (hits["prim"] == ref["prim"])
    for ty in sorted(NAMES):
        rows = np.nonzero(agree & (types[np.maximum(ref["prim"], 0)] == ty))[0]
        for p in np.unique(ref["prim"][rows]):
            k = rows[ref["prim"][rows] == p]
            dt[k], dn[k] = deviations(ty, M[p], o[k], d[k], ref["t"][k], ref["n"][k], hits["t"][k], hits["n"][k])
        figures.append("%s %.1f units / sine %.3g" % (NAMES[ty], dt[rows].max(initial=0), dn[rows].max(initial=0)))
    print("%s: %d rays, %d clear hits, unclear %.4f, wrong primitive on clear rays %d; %s" % (what, len(o), hit.sum(), share, len(wrong), "; ".join(figures)))
    assert share <= cap, share
    assert len(wrong) == 0, (wrong[:10], hits["prim"][wrong[:10]], ref["prim"][wrong[:10]])
    for ty in NAMES:
        rows = hit & (types[np.maximum(ref["prim"], 0)] == ty)
        assert dt[rows].max(initial=0) <= T_BOUND_UNITS[ty] and dn[rows].max(initial=0) <= N_BOUND_SINE[ty], (NAMES[ty], dt[rows].max(), dn[rows].max())
    assert ((hits["n"][hit].astype(np.float64) * ref["n"][hit]).sum(-1) > 0).all()
    miss = hits["prim"] == capi.HIT_MISS
    assert (hits["prim"] >= -1).all() and np.array_equal(hits["t"][miss], np.broadcast_to(np.float32(tmax), (len(o),))[miss])
    return hit


@pytest.mark.parametrize("name", list(SCENES))
def test_random_scenes_against_float64(capi, cases, name):
    c = cases(name)
    hits = c["hits"]["device boxes"]
    hit = hold_to_reference(name, capi, c["types"], c["M"], c["o"], c["d"], c["ref"], hits)
    assert hit.sum() >= 300 and (c["ref"]["clear"] & (c["ref"]["prim"] < 0)).sum() >= 300
    # the oracle's brute force runs the device's roundings: every ray, clear or not, bit for bit
    b = c["brute"]
    differ = np.nonzero((hits["prim"] != b["prim"]) | (hits["t"] != b["t"]) | (hits["n"] != b["n"]).any(-1))[0]
    both = (hits["prim"] >= 0) & (b["prim"] >= 0)
    print("%s: device against the oracle's brute force: %d of %d rays differ, largest deviation of t %.3g, of n %.3g"
          % (name, len(differ), len(hits), R.rel_dev(hits["t"][both], b["t"][both]), R.rel_dev(hits["n"][both], b["n"][both])))
    assert len(differ) == 0, (differ[:10], hits[differ[:10]], b[differ[:10]])
    assert same_hits(hits, b)


@pytest.mark.parametrize("name", list(SCENES))
def test_forms_agree_bitwise(cases, name):
    """the device's own boxes under shear, the oracle's boxes, rtgo_set_large_scene; the scene in global memory and in LDS"""
    c = cases(name)
    base = c["hits"]["device boxes"]
    for form in FORMS:
        assert same_hits(c["hits"][form], base), form
        for mode in (0, 1):
            with Knob(RTGO_TRACE_MODE=mode):
                assert same_hits(c["ctx"][form].trace_rays(c["rays"]), base), (form, mode)


def test_large_scene_from_global_memory(capi):
    n, box, n_rays, seed = LARGE
    assert n > capi.RTGO_MAX_PRIMS
    # (origins near the aimed-at primitive, as in the one-primitive families: a box of +-25 would put them up to 56 units off)
    types, M, o, d = random_scene(n, box, n_rays, seed, near=True)
    ref = A.closest(types, M, o, d, TMIN, TMAX)
    ctx = context(capi, "large scene", types, M)
    hits = ctx.trace_rays(capi.make_rays(o, d, TMIN, TMAX))
    ctx.close()
    # (no cap here: a ray is unclear as soon as one of the primitives it passes before its winner decides narrowly, and it passes many
    # times more of them than in the small scenes -- 43 % of these rays; what is needed is enough clear rays of both kinds)
    hit = hold_to_reference("%d primitives" % n, capi, types, M, o, d, ref, hits, cap=1.0)
    assert hit.sum() >= 600 and len(np.unique(ref["prim"][hit])) >= 300 and (ref["clear"] & (ref["prim"] < 0)).sum() >= 100


def three_primitive_scene(ty, M):
    """the primitive under test at index 1 between two small ones far off"""
    far0, far1 = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    far0[:3, :3] *= 0.5
    far1[:3, :3] *= 0.5
    far0[:3, 3], far1[:3, 3] = (31.0, 37.0, -29.0), (-33.0, -28.0, 35.0)
    return np.array([A.SPHERE, ty, A.DISK]), np.stack([far0.reshape(16), np.asarray(M, np.float32).reshape(16), far1.reshape(16)])


@pytest.mark.parametrize("which", ["identity", "sheared"])
def test_known_answers_on_the_device(capi, which):
    M = A.IDENTITY if which == "identity" else A.SHEARED
    outcomes = set()
    for ty in sorted(NAMES):
        types, Ms = three_primitive_scene(ty, M)
        ctx = context(capi, "device boxes", types, Ms)
        known = [k for k in A.KNOWN if k[1] == ty]
        units = [(u, s) for u in A.UNITS if u[0] == ty for s in A.SCALES]
        world = [A.to_world(M, k[2], k[3]) for k in known] + [A.to_world(M, u[1], np.asarray(u[2], np.float64) * s) for u, s in units]
        o, d = np.stack([w[0] for w in world]), np.stack([w[1] for w in world])
        hits = ctx.trace_rays(capi.make_rays(o, d, 0.0, TMAX))     # (tmin = 0: the intersectors' own thresholds decide)
        assert np.isin(hits["prim"], (capi.HIT_MISS, 1)).all(), (NAMES[ty], hits["prim"])
        assert np.isfinite(hits["t"]).all() and np.isfinite(hits["n"]).all()
        for k, (name, _, _, _, answer) in enumerate(known):
            check_known(name, ty, M, o[k], d[k], answer, hits["prim"][k] == 1, hits["t"][k], hits["n"][k])
        for k, (u, s) in enumerate(units, len(known)):
            t1 = one_primitive(ty, M, *[v[None] for v in A.to_world(M, u[1], u[2])])[1][0]
            outcomes.add(check_units(ty, M, o[k], d[k], s, hits["prim"][k] == 1, hits["t"][k], t1))
        ctx.close()
    assert outcomes == {True, False}


def test_axis_parallel_rays(capi, oracle):
    """two direction components exactly zero (the slab test's 1 / 0), at primitives whose boxes straddle all three origin planes"""
    rng = np.random.RandomState(21)
    types = np.arange(8) % 4
    M = np.stack([A.random_matrix(rng, i >= 4, spread=0.2) for i in range(8)])
    ctx = context(capi, "device boxes", types, M)
    aabb = ctx.read_bvh()[3]
    assert (aabb[:, :3] < 0).all() and (aabb[:, 3:] > 0).all(), aabb
    n = 1536
    axis, sign = np.arange(n) % 3, np.where((np.arange(n) // 3) % 2, 1.0, -1.0)
    o = rng.uniform(-2.0, 2.0, (n, 3))
    o[np.arange(n), axis] = -sign * rng.uniform(6.0, 12.0, n)
    d = np.zeros((n, 3))
    d[np.arange(n), axis] = sign * np.exp(rng.uniform(np.log(0.1), np.log(10.0), n))
    o, d = o.astype(np.float32), d.astype(np.float32)
    assert ((d == 0).sum(1) == 2).all()
    ref = A.closest(types, M, o, d, TMIN, TMAX)
    hits = ctx.trace_rays(capi.make_rays(o, d, TMIN, TMAX))
    hit = hold_to_reference("axis-parallel", capi, types, M, o, d, ref, hits)
    assert hit.sum() >= 300
    sc = oracle.scene_from_tables(types, M, materials(8), np.zeros((0, 16), np.float32), np.zeros(12, np.float32))
    for k in range(0, n, 4):
        p, t, nn, _ = R.brute(oracle, sc, o[k], d[k], TMIN, TMAX)
        assert hits["prim"][k] == p and hits["t"][k] == t and (p < 0 or np.array_equal(hits["n"][k], nn)), (k, hits[k], p, t, nn)


def test_primitive_beyond_the_box_seed(capi, oracle):
    """the box rule seeds its minimum with +50 and its maximum with -50: a primitive centred at (70, 0, 0) gets a box stretched back to
    x = 50, which still holds it, and it is still hit"""
    rng = np.random.RandomState(22)
    types = np.array([A.DISK, A.SPHERE, A.CYLINDER])
    M = np.stack([A.random_matrix(rng, True, spread=3.0) for _ in range(3)])
    M[1].reshape(4, 4)[:3, 3] = (70.0, 0.0, 0.0)
    ctx = context(capi, "device boxes", types, M)
    aabb = ctx.read_bvh()[3]
    assert np.array_equal(aabb.view(np.uint32), oracle_boxes(oracle, M).view(np.uint32))
    assert aabb[1, 0] == np.float32(50.0) - np.float32(0.001) and aabb[1, 3] > 70.0
    origins = np.array([70.0, 0.0, 0.0]) + rng.uniform(-20.0, 20.0, (1024, 3))     # (reach stays under 40)
    o, d = A.aimed_rays(rng, A.SPHERE, M[1], 1024, origins)
    ref = A.closest(types, M, o, d, TMIN, TMAX)
    hits = ctx.trace_rays(capi.make_rays(o, d, TMIN, TMAX))
    hit = hold_to_reference("sphere at x = 70", capi, types, M, o, d, ref, hits)
    assert (hit & (ref["prim"] == 1)).sum() >= 200


def test_window_at_the_devices_own_t(capi, cases):
    """t is in units of dir in the window too: with tmax at the device's own t the hit is refused, one step above it the hit is back"""
    c = cases("k16a")
    first = c["hits"]["device boxes"]
    rows = np.nonzero(c["ref"]["clear"] & (first["prim"] >= 0))[0]
    o, d, first = c["o"][rows], c["d"][rows], first[rows]
    assert len(rows) >= 300 and (np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1) > 1e-3).all()
    ctx = c["ctx"]["device boxes"]
    th = first["t"]
    got = ctx.trace_rays(capi.make_rays(o, d, TMIN, th))
    assert (got["prim"] == capi.HIT_MISS).all() and np.array_equal(got["t"], th)
    assert same_hits(ctx.trace_rays(capi.make_rays(o, d, TMIN, np.nextafter(th, np.float32(np.inf)))), first)


def surface_points(ty, n=256):
    """n object-space points of the primitive's surface, by parameter (edges and rims included)"""
    k = int(np.sqrt(n))
    u, v = [g.reshape(-1) for g in np.meshgrid(np.linspace(0, 1, k), np.linspace(0, 1, k))]
    phi = 2 * np.pi * u
    if ty == A.SPHERE:
        th = np.pi * v
        return np.stack([np.sin(th) * np.cos(phi), np.cos(th), np.sin(th) * np.sin(phi)], 1)
    if ty == A.CYLINDER:
        return np.stack([np.cos(phi), 2 * v - 1, np.sin(phi)], 1)
    if ty == A.DISK:
        return np.stack([v * np.cos(phi), 0 * v, v * np.sin(phi)], 1)
    return np.stack([u - 0.5, 0 * v, v - 0.5], 1)


@pytest.mark.parametrize("name", ["k16a", "k48", "k1"])
def test_what_the_build_wrote(cases, name):
    """rtgo_read_bvh after set_scene(aabbs=None): every primitive's surface lies inside the box the device derived for it, and the
    device's inverse is M's inverse within what its arithmetic loses"""
    c = cases(name)
    boxes, links, inv, aabb = c["ctx"]["device boxes"].read_bvh()
    lo, hi = aabb[:, :3].astype(np.float64), aabb[:, 3:].astype(np.float64)
    worst = 0.0
    for p, ty in enumerate(c["types"]):
        M = c["M"][p].astype(np.float64).reshape(4, 4)
        pts = surface_points(ty) @ M[:3, :3].T + M[:3, 3]
        assert len(pts) == 256 and (pts >= lo[p]).all() and (pts <= hi[p]).all(), (p, NAMES[ty])
        full = np.concatenate([inv[p].astype(np.float64).reshape(3, 4), [[0, 0, 0, 1]]])
        res, cond = inverse_residual(M, full)
        worst = max(worst, res / cond)
        assert res <= INVERSE_BOUND * cond, (p, res, cond)
    assert (boxes[0, :3] <= aabb[:, :3].min(0)).all() and (boxes[0, 3:] >= aabb[:, 3:].max(0)).all()   # the root holds every box
    print("%s: largest inverse residual / cond %.3g (bound %.3g)" % (name, worst, INVERSE_BOUND))


@pytest.mark.parametrize("name", list(RENDERED))
def test_fast_walk_is_the_canonical_walk_under_shear(capi, oracle, name):
    """the render kernels' own intersectors on these matrices: a floor, an emissive ceiling with its light and cornell's camera around the
    scene; 80 x 60 at 4 spp in the three modes; the timed kernel's accumulation buffer equals the instrumented canonical walk's bit for bit,
    and the timed launches did take the fast walk (inside the far-field guard).  The same context answers ray queries as the float64
    reference does, which ties the render kernels' intersectors to the anchored walk."""
    W, H = 80, 60
    n, box, n_rays, seed, scales = RENDERED[name]
    c = dict(zip(("types", "M", "o", "d"), random_scene(n, box, n_rays, seed, scales)))
    L = oracle.lib()

    def mat(fn, *a):
        m = np.zeros(16, np.float32)
        fn(*a, oracle.fptr(m))
        return m

    def mul(a, b):
        m = np.zeros(16, np.float32)
        L.oracle_mat_mul(oracle.fptr(a), oracle.fptr(b), oracle.fptr(m))
        return m

    floor = mul(mat(L.oracle_mat_translate, 0.0, -4.0, 0.0), mat(L.oracle_mat_scale, 14.0, 1.0, 14.0))
    ceil = mul(mul(mat(L.oracle_mat_translate, 0.0, 4.5, 0.0), mat(L.oracle_mat_rotate, np.float32(np.pi), 1.0, 0.0, 0.0)),
               mat(L.oracle_mat_scale, 6.0, 1.0, 6.0))
    types = np.concatenate([[A.RECTANGLE, A.RECTANGLE], c["types"]])
    M = np.concatenate([np.stack([floor, ceil]), c["M"]])
    m = materials(len(types))
    rng = np.random.RandomState(5)
    m[:, 0:3] = rng.uniform(0.1, 1.0, (len(types), 3))
    m[:, 3:6] = rng.uniform(0.0, 0.8, (len(types), 1))
    m[:, 6] = rng.choice([0.0, 1.0, 100.0, 10000.0], len(types))
    m[0] = [0.7, 0.7, 0.7, 0.3, 0.3, 0.3, 1.0, 0, 0, 0]
    m[1] = [0, 0, 0, 0, 0, 0, 1.0, 12.0, 12.0, 12.0]
    cam = oracle.scene_tables(oracle.scene("cornell", W, H))["cam"]
    ctx = capi.Context(0)
    ctx.set_scene(types, M, m, None)
    ctx.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12])
    ctx.set_background((0.05, 0.07, 0.1))
    ctx.set_lights(oracle.light_from_matrix(ceil, falloff=0.02)[None])
    ctx.resize(W * H)
    for path, ambient in ((True, False), (False, False), (False, True)):
        out = []
        for stats in (True, False):
            ctx.launch(capi.make_frame(W, H, 2, 0, path, ambient, stats=stats))
            ctx.sync()
            out.append(ctx.read_accum(H, W))
        assert np.isfinite(out[0]).all() and out[0][..., :3].max() > 0
        assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32)), "fast walk != canonical walk (path=%s, ambient=%s)" % (path, ambient)
        st = ctx.stats()
        assert st["guard_quadric"] <= 8000.0 and st["guard_reach"] <= 500.0, (st["guard_quadric"], st["guard_reach"])
    st = ctx.stats()
    print("%s: guard quadric %.0f, reach %.1f, launches %d of which canonical %d" % (name, st["guard_quadric"], st["guard_reach"], st["launches"], st["launches_canonical"]))
    assert st["launches"] == 6 and st["launches_canonical"] == 3, "the un-instrumented launches must have taken the fast walk"
    ref = A.closest(types, M, c["o"], c["d"], TMIN, TMAX)
    hits = ctx.trace_rays(capi.make_rays(c["o"], c["d"], TMIN, TMAX))
    ctx.close()
    hit = hold_to_reference(name, capi, types, M.reshape(-1, 16), c["o"], c["d"], ref, hits)
    assert hit.sum() >= 300
