"""tests/adversarial_cameras.py on the CPU: what the oracle's brute force says about rays that lie in the planes of cornell's geometry
(the counts DESIGN.md section 4 states), that the oracle renders such frames without a pixel that is not finite, and the helpers
themselves.  No GPU."""
import numpy as np
import pytest

import accel_check as AC
import adversarial_cameras as A
import shade_rays_ref as R

W, H = 48, 36
TMIN, TMAX = R.T_MIN0, R.T_MAX0
MODES = {"path": (True, False), "distributed": (False, False), "ambient": (False, True)}
# cornell at 48 x 36, frame 0, U = e_a, V = e_b, W = (0.35, 0.15) on (a, b): (axis, c, eye_ab) -> (rays that hit, of them on a
# rectangle's edge, primitives hit).  In the plane of the floor and of the ceiling every hit is an edge hit and most rays leave the closed
# room; in the planes of the boxes' tops and of the lamp every top edge is missed; from (0.7, 3.3) in a wall's plane nothing is hit,
# from the eyes of A.CORNELL_PLANES the wall itself is.  (0.3: on no plane.)
TABLE = {(1, -4.0, (0.7, 3.3)): (340, 340, [0, 10]), (1, 4.0, (0.7, 3.3)): (152, 152, [2]), (1, -2.0, (0.7, 3.3)): (1728, 0, [0, 1, 2, 3, 16]),
         (1, 0.0, (0.7, 3.3)): (1728, 0, [0, 1, 2, 3]), (1, 3.95, (0.7, 3.3)): (1728, 0, [0, 1, 2, 3]), (1, 0.3, (0.7, 3.3)): (1728, 0, [0, 1, 2, 3]),
         (0, -4.0, (0.7, 3.3)): (0, 0, []), (0, 4.0, (0.7, 3.3)): (0, 0, []), (2, -4.0, (0.7, 3.3)): (0, 0, []),
         (0, -4.0, (-3.3, -0.7)): (574, 0, [2]), (0, 4.0, (-3.3, -0.7)): (574, 0, [3]), (2, -4.0, (-0.7, -3.3)): (418, 0, [0]),
         (2, 4.0, (-0.7, -3.3)): (418, 0, [1])}
_cache = {}


def cornell(oracle):
    if "cornell" not in _cache:
        sc = oracle.scene("cornell", W, H)
        _cache["cornell"] = (sc, oracle.scene_tables(sc))
    return _cache["cornell"]


def brute(oracle, cam, w=W, h=H, frame=0):
    """(o, d, the brute force's records) of the camera's primaries over cornell, computed once per camera"""
    key = (np.asarray(cam, np.float32).tobytes(), w, h, frame)
    if key not in _cache:
        sc, _ = cornell(oracle)
        o, d, _ = A.rays(cam, w, h, frame)
        _cache[key] = (o, d, A.brute_hits(oracle, sc, o, d, TMIN, TMAX))
    return _cache[key]


def test_the_geometry_plane_cases_are_in_the_table():
    assert all((axis, c, eye_ab) in TABLE and w_ab == (0.35, 0.15) for axis, c, eye_ab, w_ab, _ in A.CORNELL_PLANES)


@pytest.mark.parametrize("key", sorted(TABLE), ids=lambda v: str(v))
def test_brute_force_in_the_planes_of_cornell(oracle, key):
    axis, c, eye_ab = key
    hits, edge, prims = TABLE[key]
    cam = A.in_plane(axis, c, eye_ab)
    assert cam[axis] == np.float32(c) and A.zero_axes(cam) == [axis]
    o, d, ref = brute(oracle, cam)             # (A.rays asserts the exact zero of every direction on the axis)
    assert (o == cam[0:3]).all() and not np.signbit(d[:, axis]).any()
    hit = ref["prim"] >= 0
    on_edge = A.edge_hits(cornell(oracle)[1], o, d, ref)
    print(key, "hits", int(hit.sum()), "edge", int(on_edge.sum()), "prims", np.unique(ref["prim"][hit]).tolist())
    if axis == 1 and abs(c) == 4.0:
        assert hit.any() and (~hit).any() and (on_edge == hit).all()
    assert (int(hit.sum()), int(on_edge.sum()), np.unique(ref["prim"][hit]).tolist()) == (hits, edge, prims)
    # the records: a miss carries tmax and nothing else, a hit a t inside the window and a normal
    assert (ref["t"][~hit] == TMAX).all() and (ref["instance"][~hit] == 0).all() and not ref["n"][~hit].any()
    assert ((ref["t"][hit] > TMIN) & (ref["t"][hit] < TMAX)).all() and (ref["instance"][hit] == -1).all()
    assert np.isfinite(ref["n"][hit]).all() and (ref["u"] == 0).all() and (ref["v"] == 0).all()


def test_float64_calls_every_in_plane_ray_unclear(oracle):
    """why the brute force is the yardstick here: analytic_ref64.closest, under its clear rule as it stands, has no verdict on any of
    these rays -- the camera on no plane (0.3) included: a ray with an exact zero runs parallel to two walls of the room"""
    import analytic_ref64
    _, t = cornell(oracle)
    for axis, c, eye_ab in sorted(TABLE):
        o, d, _ = brute(oracle, A.in_plane(axis, c, eye_ab))
        got = analytic_ref64.closest(t["type"], t["M"].reshape(-1, 4, 4), o, d, TMIN, TMAX)
        assert not got["clear"].any(), (axis, c, eye_ab, float(got["clear"].mean()))


@pytest.mark.parametrize("max_depth", [0, 3])
@pytest.mark.parametrize("mode", list(MODES))
def test_the_oracle_renders_in_plane_cameras(oracle, mode, max_depth):
    """at one sample per pixel a pixel's primary is A.rays' ray: a pixel whose primary misses is the background, and no pixel is NaN or
    infinite -- in the planes where rounding decides every ray"""
    sc, t = cornell(oracle)
    path, amb = MODES[mode]
    bg = np.append(np.float32(t["bg"]), np.float32(1.0))
    cams = [A.in_plane(axis, c, eye_ab) for axis, c, eye_ab in sorted(TABLE)] + [A.one_ray((-4.0, -4.0, 3.0), (0.0, 0.0, -1.0))]
    missed = 0
    try:
        for cam in cams:
            _, _, ref = brute(oracle, cam)
            sc.eye[:], sc.U[:], sc.V[:], sc.W[:] = [[float(v) for v in cam[3 * k:3 * k + 3]] for k in range(4)]
            acc, img, _ = oracle.render(sc, oracle.frame(W, H, 1, 0, path=path, ambient=amb, mode=1, max_depth=max_depth))
            assert np.isfinite(acc).all(), cam
            miss = (ref["prim"] < 0).reshape(H, W)
            assert np.array_equal(acc[miss].view(np.uint32), np.tile(bg, (int(miss.sum()), 1)).view(np.uint32)), cam
            missed += int(miss.sum())
    finally:
        cam = t["cam"]
        sc.eye[:], sc.U[:], sc.V[:], sc.W[:] = [[float(v) for v in cam[3 * k:3 * k + 3]] for k in range(4)]
    assert missed > 5000


@pytest.mark.parametrize("d", [(0.0, 0.0, -1.0), (0.0, -1.0, 0.0), (-0.0, -1.0, -0.0), (0.3, 0.0, -0.4), (1.0, 2.0, 2.0)])
def test_one_ray_is_the_same_primary_in_every_pixel(oracle, d):
    eye = (-4.0, -4.0, 3.0)
    cam = A.one_ray(eye, d)
    want = (np.float32(d) * (np.float32(1.0) / np.sqrt(np.float32(sum(np.float32(x) * np.float32(x) for x in d))))).astype(np.float32)
    seeds = []
    for frame in (0, 7):
        o, dd, seed = A.rays(cam, 8, 8, frame)
        assert (o == np.float32(eye)).all() and (dd == want).all(), (frame, dd[0], want)
        assert all((dd[:, k] == 0).all() for k in range(3) if d[k] == 0)
        seeds.append(seed)
        ref = brute(oracle, cam, 8, 8, frame)[2]
        assert (ref.view(np.uint32).reshape(-1, 8) == ref.view(np.uint32).reshape(-1, 8)[0]).all()
    assert not np.array_equal(seeds[0], seeds[1]) and len(np.unique(seeds[0])) == 64     # (the seeds differ: the ray does not depend on them)
    if np.signbit(d[0]) and d[0] == 0:
        assert np.signbit(dd[:, 0]).any() and not np.signbit(dd[:, 0]).all(), "a zero of W = -0 takes the sign of the pixel offsets' zeros"


def test_in_plane_is_the_zero_component_test_s_camera():
    """tests/test_gpu_parity.py::test_rays_with_an_exactly_zero_direction_component's camera, with its plane as a parameter"""
    for axis in range(3):
        a, b = [k for k in range(3) if k != axis]
        eye = np.zeros(3, np.float32); eye[axis] = 0.3; eye[a] = 0.2; eye[b] = -0.4
        U, V, Wv = [np.zeros(3, np.float32) for _ in range(3)]
        U[a], V[b] = 1.0, 1.0
        Wv[a], Wv[b] = 0.35, 0.15
        assert np.array_equal(A.in_plane(axis, 0.3, (0.2, -0.4)).view(np.uint32), np.concatenate([eye, U, V, Wv]).view(np.uint32))
    neg = A.in_plane(1, 2.0, (0.0, 0.0), zero=-0.0)
    assert np.signbit(neg[10]) and neg[10] == 0 and A.zero_axes(neg) == [1]
    d = A.rays(neg, 8, 6, 0)[1]
    assert np.signbit(d[:, 1]).reshape(6, 8)[:3, :4].all() and not np.signbit(d[:, 1]).reshape(6, 8)[3:].any() and not np.signbit(d[:, 1]).reshape(6, 8)[:, 4:].any()


def test_planes_of_a_build():
    """planes() over a hand-made read_build dict: every structure's faces, and the grid's planes as min + cs * (float)k in float32"""
    f = np.float32
    tight = np.array([[0, 0, 0, 1, 2, 3], [0.5, -1, 0, 4, 2, 6]], f)
    aabb = tight + np.array([-1, -1, -1, 1, 1, 1], f) * f(0.25)
    nodes = np.array([[-1, -2, -3, 0], [5, 6, 7, 0], [0, 0, 0, 0], [1, 2, 3, 0], [0.5, -1, 0, 0], [4, 2, 6, 0]], f)
    words = np.zeros(18, np.int32)
    words.view(f)[0:3] = (f(-0.7), f(0.1), f(3.3))
    words.view(f)[3:6] = (f(0.3), f(0.7), f(1.1))
    words[9:12] = (3, 2, 1)
    build = {"tight": tight, "aabb": aabb, "nodes": nodes, "tree0.fnodes": nodes[:2] * f(0.5), "tree1.fnodes": np.zeros((0, 4), f),
             "scene.info": np.array([2, 0, 0, 1], np.int32), "grid.params": words}
    for axis in range(3):
        p = A.planes(build, axis)
        assert all(v.dtype == f for v in p.values())
        assert np.array_equal(p["tight"], np.unique(tight[:, [axis, 3 + axis]])) and np.array_equal(p["aabb"], np.unique(aabb[:, [axis, 3 + axis]]))
        assert np.array_equal(p["nodes"], np.unique(nodes[:, axis])) and np.array_equal(p["tree0"], np.unique(nodes[:2, axis] * f(0.5))) and len(p["tree1"]) == 0
        gmin, cs, n = words.view(f)[axis], words.view(f)[3 + axis], int(words[9 + axis])
        want = [f(gmin + f(cs * f(k))) for k in range(n + 1)]
        assert np.array_equal(p["grid"].view(np.uint32), np.array(want, f).view(np.uint32))
    assert f(f(-0.7) + f(f(0.3) * f(3))) != f(-0.7 + 0.3 * 3), "the case tells one rounding per operation from one rounding in all"
    build["scene.info"] = np.array([2, 0, 0, 0], np.int32)
    assert len(A.planes(build, 0)["grid"]) == 0
    # straddlers: strictly inside; most_straddled: the lowest of the planes with the most
    assert A.straddlers(tight, 0, 0.5).tolist() == [True, False] and A.straddlers(tight, 0, 0.75).tolist() == [True, True]
    best, count = A.most_straddled(tight, 0, [3.0, 0.75, 0.9, 0.25])
    assert (float(best), count) == (0.75, 2)
    assert AC.grid_params(words)["dim"].tolist() == [3, 2, 1]
