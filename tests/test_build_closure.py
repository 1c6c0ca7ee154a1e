"""Structural closure of everything the build kernels write: each test sets a scene, reads the structures back (capi.Context.read_build)
and runs the validators of tests/accel_check.py over them -- no frame is rendered.  A violation names the broken invariant and the node,
record, cell or primitive; it holds for every ray at once, where pixel parity only sees the rays a test frame shoots."""
import importlib.util
import os

import numpy as np
import pytest

import accel_check as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64
ALL_SCENES = ["cornell", "slide", "mirror_spheres", "plateau", "window", "checkered", "balls", "soft_mirrors"]
MATERIALS = np.array([[0.8, 0.8, 0.75, 1.0, 0.0, 0.9]], np.float32)


def _module(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def capi():
    from raytracingo_amd import capi as m
    m.load()
    return m


@pytest.fixture(scope="module")
def tg():
    """tests/test_gpu_parity.py, for its scene builders (as tools/build_digest.py takes them)"""
    return _module("tg_scenes", "tests/test_gpu_parity.py")


def no_violations(v, what):
    if v:
        print("%s: %d violations listed (%s)" % (what, len(v), ", ".join(A.tags(v))))
        for line in v[:10]:
            print("   ", line)
    assert not v, "%s: %s" % (what, v[:3])


def has_grid(ctx):
    import ctypes as C
    out = (C.c_int32 * 6)()
    ctx._lib.rtgo_debug_grid.restype = C.c_int
    ctx._lib.rtgo_debug_grid.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    assert ctx._lib.rtgo_debug_grid(ctx._h, out) == 0
    return list(out)


def analytic(capi, what, types, M, mat, aabb, expect_grid=None):
    ctx = capi.Context(0)
    try:
        ctx.set_scene(types, M, mat, aabb)
        build = ctx.read_build(False)
        grid = has_grid(ctx)
    finally:
        ctx.close()
    info = np.ascontiguousarray(build["scene.info"]).view(np.int32)
    assert info[0] == len(types) and info[3] == grid[0] and len(build["tree1.fprims"]) > 0, (what, info, grid)   # (both trees are built by default)
    if grid[0]:
        gp = A.grid_params(build["grid.params"])
        assert list(gp["dim"]) == grid[1:4] and gp["entries"] == grid[4] and gp["bytes"] == grid[5] == len(build["grid.image"]), (what, gp, grid)
    if expect_grid is not None:
        assert bool(grid[0]) == expect_grid, (what, grid)
    no_violations(A.check_analytic(build, types, M, aabb), what)
    return build


# ---------------------------------------------------------------------------------------------------------------- analytic scenes
@pytest.mark.parametrize("name", ALL_SCENES)
def test_reference_scenes(capi, oracle, name):
    t = oracle.scene_tables(oracle.scene(name, W, H))
    for bb in (t["aabb"], None):
        analytic(capi, "%s, %s boxes" % (name, "the caller's" if bb is not None else "the device's"), t["type"], t["M"], t["mat"], bb,
                 expect_grid=(name == "balls"))


@pytest.mark.parametrize("k", [1, 2, 7])
def test_slide_prefixes(capi, oracle, k):
    t = oracle.scene_tables(oracle.scene("slide", W, H))
    analytic(capi, "slide[:%d]" % k, t["type"][:k], t["M"][:k], t["mat"][:k], None)


@pytest.mark.parametrize("seed", range(100, 112))
def test_random_scenes(capi, oracle, tg, seed):
    _, t = tg._random_scene(oracle, seed, W, H)
    analytic(capi, "random %d" % seed, t["type"], t["M"], t["mat"], None if seed % 2 else t["aabb"])


@pytest.mark.parametrize("seed", range(100, 112))
def test_box_scenes(capi, oracle, tg, seed):
    _, t = tg._box_scene(oracle, seed, W, H, (1, 6, 40)[seed % 3], bool(seed & 1), bool(seed & 2))
    analytic(capi, "boxes %d" % seed, t["type"], t["M"], t["mat"], None if (seed // 3) % 2 else t["aabb"])


def test_capacity_scene(capi):
    types, M, mat = _module("build_digest_scenes", "tools/build_digest.py").capacity_scene(7, 512)
    analytic(capi, "capacity", types, M, mat, None)


def _spheres(n, spacing, radius=0.6):
    """n equal spheres on a 4 x 4 x 5 lattice"""
    k = np.arange(n)
    c = np.stack([k % 4, (k // 4) % 4, k // 16], axis=1) * spacing
    M = np.zeros((n, 4, 4), np.float32)
    M[:, 0, 0] = M[:, 1, 1] = M[:, 2, 2] = radius
    M[:, 3, 3] = 1.0
    M[:, :3, 3] = c
    mat = np.zeros((n, 10), np.float32)
    mat[:, 0:3], mat[:, 6] = 0.7, 1.0
    return np.full(n, A.SPHERE), M.reshape(n, 16), mat


@pytest.mark.parametrize("n,spacing", [(63, 3.0), (64, 3.0), (65, 3.0), (64, 2.0)])
def test_equal_spheres_either_side_of_the_grid_threshold(capi, n, spacing):
    """63 small primitives get no grid, 64 and 65 (RTGO_GRID_MIN = 64) may; at spacing 2 every sphere spans more than 15 % of the scene, so
    the second structure holds all of them up front and has no tree at all"""
    build = analytic(capi, "%d spheres, spacing %g" % (n, spacing), *_spheres(n, spacing), None, expect_grid=False if n < 64 else None)
    m0, m1 = A.build_meta(build["tree0.meta"]), A.build_meta(build["tree1.meta"])
    assert m0["n_small"] == n and m1["n_small"] == (n if spacing == 3.0 else 0), (m0, m1)


# ---------------------------------------------------------------------------------------------------------------- whitted, one mesh
def bumpy_sheet(n, seed=1):
    """n triangles: the first n of a grid of quads over [-1, 1]^2 with random heights"""
    q = int(np.ceil(np.sqrt(n / 2.0)))
    rng = np.random.RandomState(seed)
    g = np.linspace(-1.0, 1.0, q + 1)
    X, Z = np.meshgrid(g, g, indexing="ij")
    p = np.stack([X, 0.2 * rng.uniform(-1, 1, X.shape), Z], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = np.arange(q)[:, None], np.arange(q)[None, :]
    a, b, c, d = i * (q + 1) + j, (i + 1) * (q + 1) + j, (i + 1) * (q + 1) + j + 1, i * (q + 1) + j + 1
    tris = np.stack([np.stack([a, c, b], -1), np.stack([a, d, c], -1)], axis=2).reshape(-1, 3)[:n]
    return {"positions": p, "normals": None, "indices": tris.astype(np.uint32)}


def coincident():
    """test_whitted_coincident_triangles' mesh: 200 copies of one triangle and two others (every split of the surface-area sweep ties)"""
    base = np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.5, 0.0]], np.float32)
    extra = np.array([[-2.0, 0.0, -1.0], [2.0, 0.0, -1.0], [0.0, 2.5, -1.0], [-0.5, 0.2, 0.5], [0.5, 0.2, 0.5], [0.0, 0.9, 0.5]], np.float32)
    return {"positions": np.concatenate([base, extra]), "normals": None, "indices": np.array([[0, 1, 2]] * 200 + [[3, 4, 5], [6, 7, 8]], np.uint32)}


def _mesh_cases():
    import whitted_big_meshes as BM
    import whitted_scene
    cases = [("%d triangles" % n, (lambda n=n: bumpy_sheet(n))) for n in (1, 2, A.LEAF_TRIS, A.LEAF_TRIS + 1, 8191, 8192)]
    cases += [("sphere300", A.sphere300), ("coincident", coincident), ("waterbottle", whitted_scene.waterbottle), ("flat sheet", lambda: BM.flat_sheet(12)),
              ("sphere300 far", lambda: A.sphere300((400.0, -400.0, 400.0)))]
    return cases


@pytest.mark.parametrize("no_sah", [False, True])
@pytest.mark.parametrize("case", range(11))
def test_one_mesh(capi, monkeypatch, case, no_sah):
    what, make = _mesh_cases()[case]
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
    no_violations(A.check_mesh(build, mesh), "%s%s" % (what, ", Morton records" if no_sah else ""))


# ---------------------------------------------------------------------------------------------------------------- instanced, clustered
def first_triangles(mesh, n):
    m = dict(mesh)
    m["indices"] = np.ascontiguousarray(np.asarray(mesh["indices"]).reshape(-1, 3)[:n])
    if m.get("tri_material") is not None:
        m["tri_material"] = np.ascontiguousarray(m["tri_material"][:n])
    return m


def instanced(capi, what, meshes, instances, then=None):
    import whitted_instances as WI
    ctx = capi.Context(0)
    try:
        ctx.whitted_set_scene(meshes, instances, WI.materials())
        no_violations(A.check_instanced(ctx.read_build(True), meshes, instances), what)
        if then is not None:
            ctx.whitted_set_instances(then)
            no_violations(A.check_instanced(ctx.read_build(True), meshes, then), what + ", after rtgo_whitted_set_instances")
    finally:
        ctx.close()


def test_instanced_tori_and_a_rebuilt_top_level(capi):
    import whitted_instances as WI
    meshes, inst = WI.tori_scene()
    rng = np.random.RandomState(3)
    moved = [(WI.transform(WI.rotation(rng) @ np.diag([1.0, 0.5 + k % 3, 1.0]), [k - 5.0, 1.0, 0.3 * k]), m, off) for k, (_, m, off) in enumerate(inst[:13])]
    instanced(capi, "tori", meshes, inst, then=moved)


def test_instanced_edges(capi):
    """one instance (no top-level records); a rotation, a uniform and a non-uniform scale; a mesh of one leaf among meshes with records"""
    import whitted_instances as WI
    rng = np.random.RandomState(5)
    instanced(capi, "one instance", [WI.torus()], [(WI.transform(WI.rotation(rng), [0.5, 1.0, -2.0]), 0, 0)])
    meshes = [WI.torus(16, 8), WI.octahedron(0.3), first_triangles(WI.octahedron(0.3), 3)]
    inst = [(WI.transform(WI.rotation(rng), [-1, 1, 0]), 0, 0), (WI.transform(0.6 * WI.rotation(rng), [0, 1, 0.5]), 1, 1),
            (WI.transform(WI.rotation(rng) @ np.diag([2.0, 0.4, 1.0]), [1, 0.5, 0]), 0, 1), (WI.transform(np.diag([1.5, 0.5, 1.0]), [2, 1, -1]), 2, 0),
            (WI.transform(WI.rotation(rng) @ np.diag([-0.7, 1.3, 0.9]), [0, 2, 1]), 1, 2), (WI.transform(np.eye(3), [300.0, -200.0, 100.0]), 0, 0)]
    instanced(capi, "transforms", meshes, inst)
    instanced(capi, "transforms, four", meshes, inst[:4])     # (kLeafTris instances: one leaf) ...
    instanced(capi, "transforms, five", meshes, inst[:5])     # ... and one more: the first record


def test_instanced_2400_octahedra(capi):
    import whitted_instances as WI
    meshes, inst = WI.octahedra_scene(2400)
    instanced(capi, "2400 octahedra", meshes, inst)


@pytest.mark.parametrize("n", [8193, 16384, 16385, 40002])
def test_clustered_meshes(capi, n):
    import whitted_big_meshes as BM
    import whitted_instances as WI
    nu = {8193: 65, 16384: 128, 16385: 129, 40002: 200}[n]
    nv = {8193: 64, 16384: 64, 16385: 64, 40002: 101}[n]
    big = first_triangles(BM.displaced_torus(nu, nv), n)
    rng = np.random.RandomState(n)
    meshes = [big, WI.octahedron(0.2)]
    inst = [(WI.transform(np.eye(3), [0, 1, 0]), 0, 0), (WI.transform(WI.rotation(rng) @ np.diag([1.2, 0.7, 1.0]), [2, 1, 0]), 0, 1),
            (WI.transform(np.eye(3), [0, 2, 0]), 1, 0)]
    instanced(capi, "clustered %d" % n, meshes, inst, then=inst[:2] if n == 8193 else None)


def _fnv(a):
    h = 0xCBF29CE484222325
    for b in np.ascontiguousarray(a).view(np.uint8).reshape(-1).tolist():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_read_build_returns_the_bytes_the_digest_hashes(capi, oracle):
    """rtgo_debug_read_build and rtgo_debug_build_digest walk one list of spans: span for span, the bytes read back hash to the digest"""
    import whitted_instances as WI
    t = oracle.scene_tables(oracle.scene("cornell", W, H))
    ctx = capi.Context(0)
    try:
        ctx.set_scene(t["type"], t["M"], t["mat"], t["aabb"])
        build, digest = ctx.read_build(False), ctx.build_digest(False)
        assert len(build) == len(digest) == 16 and [_fnv(v) for v in build.values()] == digest
        mesh = A.sphere300()
        ctx.whitted_set_mesh(mesh["positions"], mesh["normals"], mesh["indices"], None, MATERIALS)
        build, digest = ctx.read_build(True), ctx.build_digest(True)
        assert list(build)[:6] == ["recs", "qrecs", "tris", "tidx", "grid", "counts"] and [_fnv(v) for v in build.values()] == digest
        meshes = [WI.torus(8, 4), WI.octahedron(0.3)]
        ctx.whitted_set_scene(meshes, [(WI.transform(np.eye(3), [k, 0, 0]), k % 2, 0) for k in range(6)], WI.materials())
        build, digest = ctx.read_build(True), ctx.build_digest(True)
        assert len(build) == 5 * 2 + 3 + 2 + 1 and [_fnv(v) for v in build.values()] == digest
    finally:
        ctx.close()
