"""rtgo_whitted_trace_rays on the MI355X: caller-supplied rays against one mesh, instanced and clustered scenes -- held to the instanced
oracle's single-ray trace on the rays a float64 brute force finds clear, and the structures and forms against each other bit for bit."""
import numpy as np
import pytest

import trace_rays_ref as R
import whitted_big_meshes as BM
import whitted_instances as WI
from test_trace_rays import Knob, same_hits

pytestmark = pytest.mark.gpu

EYE = np.eye(3, 4, dtype=np.float32)
TMIN, TMAX = np.float32(0.01), np.float32(1e16)
# Largest relative deviation of the device's t, u and v from oracle_whitted_trace_instanced's over the clear rays of the two scenes below,
# as measured on an MI355X: 0, 0 and 0 -- the walk's arithmetic is the oracle's, operation for operation, one IEEE rounding
# each (no contraction; div_cr is the correctly rounded quotient in its range).  The bounds are 4 x that: equality.
T_BOUND, UV_BOUND = 4 * 0.0, 4 * 0.0
UNCLEAR_CAP = 0.01


@pytest.fixture(scope="module")
def capi():
    import torch
    from raytracingo_amd import capi as m
    m.load()
    if torch.cuda.is_available():
        torch.cuda.init()   # torch's HIP runtime up before this module's first context (some tests hand the library torch buffers)
    return m


def scene_rays(oracle, meshes, inst, eye, lookat, n_random=512, W=48, H=32):
    """W x H pixel-centre primaries of a camera at `eye` plus n_random rays with a uniform origin in the scene's bounds (seed 7)"""
    import whitted_scene
    cam = whitted_scene.camera(oracle, W, H, eye=eye, lookat=lookat)
    pos = WI.flatten([dict(m, normals=None, texcoords=None) for m in meshes], inst)["positions"]
    o1, d1 = R.primaries(cam, W, H)
    o2, d2 = R.random_rays(pos.min(0), pos.max(0) + np.float32([0, 1, 0]), n_random)
    return np.concatenate([o1, o2]), np.concatenate([d1, d2])


def inst_ctx(capi, meshes, inst, mats=None):
    ctx = capi.Context(0)
    ctx.whitted_set_scene(meshes, inst, WI.materials() if mats is None else mats)
    return ctx


CASES = {"tori": (lambda: WI.tori_scene(), (0.5, 4.0, 6.0), (0.0, 0.4, -0.5)),
         "octahedra": (lambda: WI.mirrored_scene(False, scale=(1.4, 0.6, 1.0)), (0.3, 3.5, 5.5), (0.0, 0.5, -0.3))}


@pytest.mark.parametrize("name", list(CASES))
def test_triangle_path_against_the_oracle(capi, oracle, name):
    make, eye, lookat = CASES[name]
    meshes, inst = make()
    o, d = scene_rays(oracle, meshes, inst, eye, lookat)
    hit64, clear, key = R.clear_triangle_rays(meshes, inst, o, d, float(TMIN))
    share = 1.0 - clear.sum() / max(hit64.sum(), 1)
    sc = oracle.InstancedScene(meshes, inst, WI.materials(), WI.lights())
    hits = inst_ctx(capi, meshes, inst).whitted_trace_rays(capi.make_rays(o, d, TMIN, TMAX))
    ks = np.nonzero(clear)[0]
    want = np.array([sc.trace(o[k], d[k], float(TMIN), float(TMAX)) for k in ks], np.float64)   # (instance, triangle, t, u, v)
    got = hits[ks]
    dt = R.rel_dev(got["t"], want[:, 2])
    duv = max(R.rel_dev(got["u"], want[:, 3]), R.rel_dev(got["v"], want[:, 4]))
    print("%s: %d rays, %d hit in float64, unclear share of them %.4f, t deviation %.3g, u / v deviation %.3g" % (name, len(o), hit64.sum(), share, dt, duv))
    assert hit64.sum() > 0.4 * len(o) and share <= UNCLEAR_CAP
    assert np.array_equal(want[:, :2].astype(np.int64), key[ks]), "the oracle against float64"
    assert np.array_equal(got["instance"], want[:, 0].astype(np.int32)) and np.array_equal(got["prim"], want[:, 1].astype(np.int32))
    assert dt <= T_BOUND and duv <= UV_BOUND, (dt, duv)
    # the rest of the record
    miss = hits["prim"] == capi.HIT_MISS
    assert (hits["prim"] >= -1).all() and (hits["n"] == 0).all()
    assert np.array_equal(hits["t"][miss], np.full(miss.sum(), TMAX)) and not hits[miss].view(np.uint32).reshape(-1, 8)[:, 2:].any()
    assert (hits["instance"][~miss] >= 0).all() and (hits["instance"][~miss] < len(inst)).all()


def test_forms_agree_bitwise(capi, oracle):
    """top level in LDS or read through L2, any batch size, any grid, permuted rays; any-hit gives the closest walk's hit / miss mask"""
    make, eye, lookat = CASES["tori"]
    meshes, inst = make()
    o, d = scene_rays(oracle, meshes, inst, eye, lookat)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    ctx = inst_ctx(capi, meshes, inst)
    with Knob(RTGO_TRACE_MODE=0, RTGO_TRACE_BLOCKS=None):
        base = ctx.whitted_trace_rays(rays)
    assert (base["prim"] >= 0).sum() > 500
    perm = np.random.RandomState(1).permutation(len(rays))
    for mode in (None, 0, 1):
        with Knob(RTGO_TRACE_MODE=mode):
            assert same_hits(ctx.whitted_trace_rays(rays), base), mode
            assert same_hits(ctx.whitted_trace_rays(rays[perm]), base[perm]), "permuted rays"
            for n in (1, 63, 64, 65, 256, 257):
                assert same_hits(ctx.whitted_trace_rays(rays[:n]), base[:n]), "batch of %d" % n
            with Knob(RTGO_TRACE_BLOCKS=2):   # workgroups of 256 lanes: two passes and one ray
                assert same_hits(ctx.whitted_trace_rays(rays[:1025]), base[:1025]), "grid-stride loop"
            any_hit = ctx.whitted_trace_rays(rays, capi.TRACE_ANY_HIT)
            assert np.array_equal(any_hit["prim"] >= 0, base["prim"] >= 0), "any-hit mask"
            h = any_hit["prim"] >= 0
            assert (any_hit["t"][h] >= base["t"][h]).all() and (any_hit["t"][h] < TMAX).all()


def test_one_mesh_equals_one_identity_instance(capi, oracle):
    import whitted_scene
    mesh = whitted_scene.build()
    o, d = scene_rays(oracle, [mesh], [(EYE, 0, 0)], (0.5, 3.0, 7.0), (0.0, 1.0, 0.0))
    rays = capi.make_rays(o, d, TMIN, TMAX)
    ctx = capi.Context(0)
    ctx.whitted_set_mesh(mesh["positions"], mesh["normals"], mesh["indices"], mesh["tri_material"], mesh["materials"])
    a = ctx.whitted_trace_rays(rays)
    b = inst_ctx(capi, [mesh], [(EYE, 0, 0)], mesh["materials"]).whitted_trace_rays(rays)
    assert (a["prim"] >= 0).sum() > 500 and (a["instance"] == 0).all()
    assert same_hits(a, b)
    any_hit = ctx.whitted_trace_rays(rays, capi.TRACE_ANY_HIT)
    assert np.array_equal(any_hit["prim"] >= 0, a["prim"] >= 0)
    with Knob(RTGO_TRACE_BLOCKS=1):
        assert same_hits(ctx.whitted_trace_rays(rays[:700]), a[:700])
    # a mesh of one leaf (no records at all)
    small = WI.octahedron(0.5)
    small = dict(small, indices=small["indices"][:4])
    so, _ = R.random_rays([-1, -1, -1], [1, 1, 1], 256)
    rng = np.random.RandomState(4)   # (aimed at points of the four triangles: random directions hardly ever meet them)
    corners = small["positions"][small["indices"][rng.randint(0, 4, 256)]]
    sd = ((rng.dirichlet([1, 1, 1], 256)[:, :, None] * corners).sum(1) - so).astype(np.float32)
    ctx.whitted_set_mesh(small["positions"], None, small["indices"], None, WI.materials())
    one = ctx.whitted_trace_rays(capi.make_rays(so, sd, TMIN, TMAX))
    assert (one["prim"] >= 0).sum() > 200 and (one["prim"] < 4).all() and set(np.unique(one["prim"])) >= {0, 1, 2, 3}
    assert same_hits(one, inst_ctx(capi, [small], [(EYE, 0, 0)]).whitted_trace_rays(capi.make_rays(so, sd, TMIN, TMAX)))


@pytest.mark.parametrize("n_tri", [8193, 16385])
def test_clustered_mesh_equals_the_callers_cut(capi, oracle, n_tri):
    """8193 triangles: a mid level without records; 16385: the first with.  One identity instance of the clustered mesh against its cut
    into identity instances of at most 8192 triangles, (instance, triangle) mapped back to the mesh's own index"""
    from test_whitted_clustered import _plus_one_triangle
    mesh = _plus_one_triangle(BM.displaced_torus(64 if n_tri < 16384 else 128, 64, texcoords=False))
    assert len(mesh["indices"]) == n_tri
    inst = [(EYE, 0, 0)]
    o, d = scene_rays(oracle, [mesh], inst, (0.6, 1.5, 2.2), (0.0, -0.1, 0.0))
    rays = capi.make_rays(o, d, TMIN, TMAX)
    cmeshes, cinst = BM.chunked_scene([mesh], inst, big={0})
    cut = inst_ctx(capi, cmeshes, cinst).whitted_trace_rays(rays)
    h = cut["prim"] >= 0
    assert h.sum() > 500 and len(np.unique(cut["instance"][h])) == len(cinst)
    want = cut.copy()
    want["prim"][h] = cut["instance"][h] * 8192 + cut["prim"][h]
    want["instance"][h] = 0
    ctx = inst_ctx(capi, [mesh], inst)
    for mode in (None, 0, 1):
        with Knob(RTGO_TRACE_MODE=mode):
            got = ctx.whitted_trace_rays(rays)
            assert same_hits(got, want), mode
            any_hit = ctx.whitted_trace_rays(rays, capi.TRACE_ANY_HIT)
            assert np.array_equal(any_hit["prim"] >= 0, h)


def test_ties_keep_the_lower_instance(capi, oracle):
    """nine copies of one triangle under one transform among other instances: more than two top-level leaves hold them (a leaf has at most
    four), and the lowest index among them is reported"""
    tri = {"positions": np.array([[-1, 0, -1], [1, 0, -1], [0, 0, 1]], np.float32), "normals": None, "indices": np.array([[0, 2, 1]], np.uint32),
           "tri_material": None}
    rng = np.random.RandomState(2)
    T = WI.transform(WI.rotation(rng) * 0.8, [0.3, 0.5, -0.2])
    copies = list(range(3, 21, 2))
    inst = [(T, 0, 0) if k in copies else (WI.transform(WI.rotation(rng), [3.0 + (k % 5), 4.0, 2.0 + k // 5]), 1, 0) for k in range(24)]
    assert len(copies) == 9
    M = WI.as34(T)
    b = rng.dirichlet([2, 2, 2], 128)
    pts = (b @ tri["positions"][[0, 2, 1]].astype(np.float64)) @ M[:, :3].T + M[:, 3]
    nrm = M[:, :3] @ np.array([0.0, 1.0, 0.0])
    o = (pts + 1.5 * nrm / np.linalg.norm(nrm)).astype(np.float32)
    d = np.tile(-nrm / np.linalg.norm(nrm), (128, 1)).astype(np.float32)
    ctx = inst_ctx(capi, [tri, WI.octahedron(0.2)], inst)
    for mode in (0, 1):
        with Knob(RTGO_TRACE_MODE=mode):
            hits = ctx.whitted_trace_rays(capi.make_rays(o, d, TMIN, TMAX))
            assert (hits["instance"] == copies[0]).all() and (hits["prim"] == 0).all(), (hits["instance"], hits["prim"])


def test_invalid_rays_and_window(capi, oracle):
    make, eye, lookat = CASES["octahedra"]
    meshes, inst = make()
    o, d = scene_rays(oracle, meshes, inst, eye, lookat, n_random=64)
    rays = capi.make_rays(o, d, TMIN, TMAX)
    ctx = inst_ctx(capi, meshes, inst)
    alone = ctx.whitted_trace_rays(rays)
    bad = rays.copy()
    nan = np.float32(np.nan)
    ks = np.array([0, 63, 64, 65, 700])
    bad["dir"][0] = 0
    bad["origin"][63] = (0, nan, 0)
    bad["tmax"][64] = bad["tmin"][64]
    bad["tmin"][65] = -1
    bad["tmax"][700] = nan
    got = ctx.whitted_trace_rays(bad)
    assert (got["prim"][ks] == capi.HIT_INVALID).all()
    assert not got[ks].view(np.uint32).reshape(len(ks), 8)[:, [0, 2, 3, 4, 5, 6, 7]].any()
    keep = np.ones(len(rays), bool)
    keep[ks] = False
    assert same_hits(got[keep], alone[keep])
    # the window at the GPU's own t
    h = alone["prim"] >= 0
    th = alone["t"][h]
    assert (ctx.whitted_trace_rays(capi.make_rays(o[h], d[h], TMIN, th))["prim"] == capi.HIT_MISS).all()
    assert same_hits(ctx.whitted_trace_rays(capi.make_rays(o[h], d[h], TMIN, np.nextafter(th, np.float32(np.inf)))), alone[h])
    assert same_hits(ctx.whitted_trace_rays(capi.make_rays(o[h], d[h], np.nextafter(th, np.float32(0)), TMAX)), alone[h])
    behind = ctx.whitted_trace_rays(capi.make_rays(o[h], d[h], th, TMAX))
    b = behind["prim"] >= 0
    assert (behind["t"][b] > th[b]).all() and b.any() and (~b).any()
    s0 = ctx.stats()
    ctx.whitted_trace_rays(rays[:77], capi.TRACE_ANY_HIT)
    ctx.whitted_trace_rays(rays[:23])
    s1 = ctx.stats()
    assert s1["rays_total"] == s0["rays_total"] + 100 and s1["rays_occlusion"] == s0["rays_occlusion"] + 77 and s1["launches"] == s0["launches"]
