"""Cameras whose rays lie in the planes of a scene's geometry and of its acceleration structures, numpy only (no GPU call anywhere in
this file): what tests/test_adversarial_cameras_ref.py (CPU) and tests/test_analytic_adversarial_cameras.py (MI355X) share.

A camera whose U, V and W have an exact 0 on one axis shoots rays with an exact 0 there, and with the eye in a plane of the scene -- a
wall, a box's face, a face of a node box of either fast-walk tree or of the canonical LBVH, a cell plane or a bound of the uniform grid --
every primary ray runs INSIDE that plane: slab parameters are 0 * 1e30 or a rounding residue times 1e30, rectangles are met on their
edges, and rounding decides each ray.  float64 calls all of these rays unclear (analytic_ref64.closest), so the yardstick is the brute
force over the oracle's float32 intersection programs on every ray (trace_rays_ref.brute), which is what the canonical walk computes."""
import numpy as np

import accel_check as AC
import shade_rays_ref
import trace_rays_ref

F = np.float32
# rtgo_hit as a numpy record: raytracingo_amd.capi.HIT_DTYPE restated (this module does not load the library)
HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<i4"), ("instance", "<i4"), ("u", "<f4"), ("v", "<f4"), ("n", "<f4", (3,))])
HIT_MISS = -1


# cornell, the planes of its geometry: (axis, c, eye_ab, w_ab, least number of primaries that miss).  Axis y with the eye inside the room:
# the floor and both boxes' bottoms, the short box's top, the tall box's top, the lamp, the ceiling (the brute force's counts at 48 x 36,
# frame 0: tests/test_adversarial_cameras_ref.py).  Axes x and z with the eye ON a wall plane: from (0.7, 3.3) no ray hits anything, from
# the eyes below the rays that run inside the wall's own plane hit that wall, at whatever t its 0 / 0 of rounding residues gives.
CORNELL_PLANES = [(1, -4.0, (0.7, 3.3), (0.35, 0.15), 100), (1, -2.0, (0.7, 3.3), (0.35, 0.15), 0), (1, 0.0, (0.7, 3.3), (0.35, 0.15), 0),
                  (1, 3.95, (0.7, 3.3), (0.35, 0.15), 0), (1, 4.0, (0.7, 3.3), (0.35, 0.15), 100),
                  (0, -4.0, (-3.3, -0.7), (0.35, 0.15), 100), (0, 4.0, (-3.3, -0.7), (0.35, 0.15), 100),
                  (2, -4.0, (-0.7, -3.3), (0.35, 0.15), 100), (2, 4.0, (-0.7, -3.3), (0.35, 0.15), 100)]


def others(axis):
    """the two axes that are not `axis`, ascending"""
    return [k for k in range(3) if k != axis]


def in_plane(axis, c, eye_ab, w_ab=(0.35, 0.15), zero=0.0):
    """cam[12] (eye, U, V, W) of test_rays_with_an_exactly_zero_direction_component with the plane as a parameter: eye[axis] = c, the
    eye's other two coordinates eye_ab; U and V the unit vectors of the other two axes, W = w_ab on them.  U, V and W are exactly 0 on
    `axis`; zero = -0.0 puts the negative zero into W there (the ray's component is then -0 where both pixel offsets are negative, +0
    elsewhere: one frame holds both signs)."""
    a, b = others(axis)
    cam = np.zeros(12, F)
    cam[axis], cam[a], cam[b] = c, eye_ab[0], eye_ab[1]
    cam[3 + a] = 1.0
    cam[6 + b] = 1.0
    cam[9 + a], cam[9 + b] = w_ab
    cam[9 + axis] = zero
    return cam


def one_ray(eye, d):
    """cam[12] with U = V = 0 and W = d: every pixel shoots the ray (eye, normalize(d)); no projection is involved.  The zero components
    of d stay exactly zero (of either sign: 0 * offset + 0 * offset + 0)."""
    cam = np.zeros(12, F)
    cam[0:3] = eye
    cam[9:12] = d
    return cam


def zero_axes(cam):
    """the axes on which U, V and W are all exactly zero"""
    cam = np.asarray(cam, F)
    return [k for k in range(3) if cam[3 + k] == 0 and cam[6 + k] == 0 and cam[9 + k] == 0]


def rays(cam, w, h, frame):
    """shade_rays_ref.raygen32: (o [h w, 3], d [h w, 3], seed [h w]) of the launch's own primaries at one sample per pixel.  On every
    axis on which the camera's U, V and W are zero the direction must be exactly zero."""
    o, d, seed = shade_rays_ref.raygen32(cam, w, h, frame)
    for k in zero_axes(cam):
        assert (d[:, k] == 0).all(), "axis %d: %d rays leave the plane" % (k, int((d[:, k] != 0).sum()))
    return o, d, seed


def brute_hits(oracle, scene, o, d, tmin, tmax):
    """trace_rays_ref.brute over all rays, as the records rtgo_trace_rays writes: a hit is (t, prim, instance -1, 0, 0, n), a miss
    (tmax, -1, 0, 0, 0, 0)"""
    out = np.zeros(len(o), HIT_DTYPE)
    for k in range(len(o)):
        p, t, n, _ = trace_rays_ref.brute(oracle, scene, o[k], d[k], tmin, tmax)
        out["prim"][k], out["t"][k] = p, t
        if p >= 0:
            out["instance"][k], out["n"][k] = -1, n
    return out


def grid_planes(gp, axis):
    """the uniform grid's bound and cell planes on `axis` as fast_grid forms them: min + cs * (float)k, k = 0 .. dim, one rounding per
    operation (the build contracts nothing)"""
    k = np.arange(int(gp["dim"][axis]) + 1).astype(F)
    p = (F(gp["min"][axis]) + (F(gp["cs"][axis]) * k).astype(F)).astype(F)
    assert p.dtype == F
    return p


def has_grid(build):
    return bool(np.ascontiguousarray(build["scene.info"]).view(np.int32)[3])


def planes(build, axis):
    """the exact float32 coordinates on `axis` of every face the walks test a ray against, by structure, each sorted and without
    repeats: "tight" (the boxes the fast walk culls with), "tree0" / "tree1" (leaf and inner boxes of the two fast-walk trees),
    "nodes" (the canonical LBVH), "aabb" (the reference's boxes) and "grid" (its bounds and cell planes; empty without a grid).
    build: Context.read_build(False)."""
    out = {}
    for name in ("tight", "aabb"):
        b = np.asarray(build[name], F).reshape(-1, 6)
        out[name] = np.unique(np.concatenate([b[:, axis], b[:, 3 + axis]]))
    for name, span in (("tree0", "tree0.fnodes"), ("tree1", "tree1.fnodes"), ("nodes", "nodes")):
        nd = np.asarray(build.get(span, np.zeros((0, 4), F)), F).reshape(-1, 2, 4)
        out[name] = np.unique(nd[:, :, axis].reshape(-1))
    out["grid"] = np.unique(grid_planes(AC.grid_params(build["grid.params"]), axis)) if has_grid(build) else np.zeros(0, F)
    return out


def straddlers(tight, axis, c):
    """which tight boxes have the plane `axis` = c strictly inside"""
    b = np.asarray(tight, F).reshape(-1, 6)
    return (b[:, axis] < F(c)) & (F(c) < b[:, 3 + axis])


def most_straddled(tight, axis, candidates):
    """(plane, count): the candidate plane that the most tight boxes straddle, the lowest on ties"""
    cand = np.unique(np.asarray(candidates, F))
    counts = np.array([int(straddlers(tight, axis, c).sum()) for c in cand])
    k = int(np.argmax(counts))
    return cand[k], int(counts[k])


def edge_hits(tables, o, d, hits, tol=1e-5):
    """of the rays that hit a rectangle: which meet it on an edge, |(|u| - 1/2)| < tol for u either in-plane object coordinate of the hit
    point (float64 from the model matrix)"""
    M = np.asarray(tables["M"], np.float64).reshape(-1, 4, 4)
    on = np.zeros(len(o), bool)
    for k in np.flatnonzero((hits["prim"] >= 0)):
        p = int(hits["prim"][k])
        if int(tables["type"][p]) != AC.RECTANGLE:
            continue
        w = np.asarray(o[k], np.float64) + float(hits["t"][k]) * np.asarray(d[k], np.float64)
        q = np.linalg.solve(M[p], np.append(w, 1.0))
        on[k] = min(abs(abs(q[0]) - 0.5), abs(abs(q[2]) - 0.5)) < tol
    return on
