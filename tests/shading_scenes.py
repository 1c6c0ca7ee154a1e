"""Scenes built for tests/analytic_shading_ref64.py's whole-pipeline checks, as the tables the C ABI and oracle_py.scene_from_tables take
(type, M [n, 16] row-major float32, mat [n, 10] = kd kr specularity Le, lights [nl, 16] = corner v1 v2 normal colour falloff, cam [12] = eye U V W,
bg).  Numpy only; no file and no scene of the reference.  A rectangle is the unit square y = 0 seen from +y only, a disk the unit disk y = 0
seen from both sides, a sphere |p| = 1, a cylinder x^2 + z^2 = 1, |y| < 1 (tests/analytic_ref64.py)."""
import numpy as np

CYLINDER, DISK, RECTANGLE, SPHERE = 0, 1, 2, 3

# kd, kr, specularity, Le.  The three surface kinds the shader tells apart: specularity < 0.5 (a diffuse lobe about N), a glossy lobe about the
# mirror direction, and an exponent so large that the lobe is a mirror's
DIFFUSE = (0.8, 0.8, 0.8, 0.3, 0.3, 0.3, 0.0, 0, 0, 0)
MATTE = (0.8, 0.8, 0.8, 0.3, 0.3, 0.3, 1.0, 0, 0, 0)     # specularity 1: a wide lobe about the mirror direction, and a child under ambient light too
RED = (0.9, 0.1, 0.1, 0.3, 0.3, 0.3, 1.0, 0, 0, 0)
GREEN = (0.1, 0.9, 0.1, 0.3, 0.3, 0.3, 1.0, 0, 0, 0)
GLOSSY = (0.5, 0.4, 0.1, 0.5, 0.5, 0.5, 30.0, 0, 0, 0)
MIRROR = (0.05, 0.05, 0.05, 1.0, 1.0, 1.0, 100000.0, 0, 0, 0)
LAMP = (0, 0, 0, 0, 0, 0, 1.0, 15.0, 15.0, 15.0)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def frame_about(normal, spin=0.0):
    """a right-handed rotation whose y column is `normal`; `spin` turns it about that normal"""
    n = _unit(normal)
    h = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.array([0.0, 0.0, 1.0])
    a = _unit(h - n * (h @ n))
    b = np.cross(a, n)
    a, b = np.cos(spin) * a + np.sin(spin) * b, np.cos(spin) * b - np.sin(spin) * a
    return np.stack([a, n, b], 1)


def model(centre, R, scale):
    M = np.eye(4)
    M[:3, :3] = np.asarray(R, np.float64) @ np.diag(np.broadcast_to(np.asarray(scale, np.float64), (3,)))
    M[:3, 3] = centre
    return M.astype(np.float32).reshape(16)


def flat(centre, normal, size, spin=0.0):
    """the model matrix of a rectangle of edge `size` (or a disk of radius `size`) at `centre` facing `normal`"""
    return model(centre, frame_about(normal, spin), (size, 1.0, size))


def box(centre, half, turn):
    """six outward rectangles of a box with half-extents `half`, turned by `turn` about y"""
    c, s = np.cos(turn), np.sin(turn)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    out = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            n = np.zeros(3)
            n[axis] = sign
            F = frame_about(n)
            # the rectangle's own x and z run along the two other axes of the box: scale each by that axis' extent
            ext = [2 * float(np.abs(F[:, k]) @ np.asarray(half, np.float64)) for k in (0, 2)]
            M = np.eye(4)
            M[:3, :3] = R @ F @ np.diag([ext[0], 1.0, ext[1]])
            M[:3, 3] = np.asarray(centre, np.float64) + R @ (n * np.asarray(half, np.float64))
            out.append(M.astype(np.float32).reshape(16))
    return out


def light_record(M, falloff, colour=(1.0, 1.0, 1.0)):
    """the surface light of a unit rectangle under M: corner = M (-1/2, 0, 1/2, 1), v1 = M (1, 0, 0, 0), v2 = M (0, 0, -1, 0), normal = normalize(v1 x v2)"""
    M = np.asarray(M, np.float64).reshape(4, 4)
    corner = M[:3, :3] @ np.array([-0.5, 0.0, 0.5]) + M[:3, 3]
    v1, v2 = M[:3, 0], -M[:3, 2]
    return np.concatenate([corner, v1, v2, _unit(np.cross(v1, v2)), colour, [falloff]]).astype(np.float32)


def camera(eye, lookat, up, fovy, aspect):
    eye, lookat, up = (np.asarray(v, np.float64) for v in (eye, lookat, up))
    W = lookat - eye
    U = _unit(np.cross(W, up))
    V = _unit(np.cross(U, W))
    vlen = np.linalg.norm(W) * np.tan(0.5 * np.radians(fovy))
    return np.concatenate([eye, U * vlen * aspect, V * vlen, W]).astype(np.float32)


def _tables(prims, lights, cam, bg):
    return {"type": np.array([p[0] for p in prims], np.int32), "M": np.array([p[1] for p in prims], np.float32).reshape(-1, 16),
            "mat": np.array([p[2] for p in prims], np.float32).reshape(-1, 10), "lights": np.array(lights, np.float32).reshape(-1, 16),
            "cam": cam, "bg": np.array(bg, np.float32)}


def shell(centre, half, materials, skip=()):
    """the inward rectangles of a cube of half-edge `half` about `centre`, one material per face in the order -x +x -y +y -z +z (the face named is
    the one the rectangle lies on); `skip` leaves faces out"""
    faces = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    return [(RECTANGLE, flat(np.asarray(centre, np.float64) + half * np.asarray(f, np.float64), [-c for c in f], 2 * half), m)
            for k, (f, m) in enumerate(zip(faces, materials)) if k not in skip]


def room(aspect=48 / 36):
    """a closed box of rectangles, flat primitives only: an emitter under the ceiling with its light record 0.02 below it and two thirds
    its size (so that an occlusion ray's window ends clear of the emitter, and its line clear of the emitter's edges), a diffuse and a glossy box, both turned, and a mirror-like disk"""
    h = 4.0
    prims = shell((0, 0, 0), h, (RED, GREEN, MATTE, MATTE, MATTE, DIFFUSE))
    lamp = flat((-2.6, h - 0.05, -2.4), (0, -1, 0), 1.6, spin=0.3)
    prims.append((RECTANGLE, flat((-2.6, h - 0.05, -2.4), (0, -1, 0), 2.4, spin=0.3), LAMP))
    prims += [(RECTANGLE, M, DIFFUSE) for M in box((-1.2, -h + 2.2, -0.6), (0.9, 2.2, 0.9), 0.4)]
    prims += [(RECTANGLE, M, GLOSSY) for M in box((1.7, -h + 2.0, -1.8), (0.7, 2.0, 0.7), -0.3)]
    prims.append((DISK, flat((0.8, 2.0, -0.4), (0.2, 0.3, 1.0), 0.5), MIRROR))
    below = np.asarray(lamp, np.float64).copy()
    below[7] -= 0.02
    lights = [light_record(below, 0.1), light_record(below, 0.1)]   # two records: the index rule never draws the last
    return _tables(prims, lights, camera((0.2, 0.3, 3.8), (0.0, -0.8, -1.0), (0, 1, 0), 70.0, aspect), (0.0, 0.0, 0.0))


def two_lights(aspect=48 / 36):
    """an open floor under three surface lights of distinct falloff -- the index rule can draw the first two only -- with blockers whose Le
    lies below and above 1 in different channels: a shadowed point carries min(Le, 1) of its blocker.  Light 2 hangs low over the middle
    of the floor: were it ever drawn, the floor there would be far brighter."""
    prims = [(RECTANGLE, flat((0, 0, 0), (0, 1, 0), 14.0), DIFFUSE),
             (RECTANGLE, flat((0, 2.0, -7.0), (0, 0, 1), 14.0), GLOSSY)]
    prims[0] = (RECTANGLE, prims[0][1], MATTE)
    spots = [((-2.5, 5.0, -1.0), 0.0), ((2.5, 5.5, 0.5), 0.35), ((0.0, 1.2, 0.0), 2.0)]
    lights = [light_record(flat(c, (0, -1, 0), 1.5, spin=0.2 * k), f) for k, (c, f) in enumerate(spots)]
    # blockers: both are "emitters" by length(Le) > 0.01, so a primary ray that sees one returns white; what they pass on as occluders differs
    prims.append((DISK, flat((-1.6, 2.2, -0.6), (0.1, 1, 0.1), 1.5), (0, 0, 0, 0, 0, 0, 1.0, 0.25, 0.5, 2.0)))
    prims.append((RECTANGLE, flat((1.8, 2.4, 0.4), (0, -1, 0), 2.6, spin=0.5), (0, 0, 0, 0, 0, 0, 1.0, 3.0, 0.125, 0.5)))
    prims += shell((0, 8.0, 0), 10.0, (RED, GREEN, MATTE, MATTE, MATTE, MATTE), skip=(3, 4))     # no ceiling, no far wall: the background shows there
    return _tables(prims, lights, camera((0.5, 6.0, 7.5), (0.0, 0.3, -0.5), (0, 1, 0), 55.0, aspect), (0.1, 0.2, 0.4))


def quadrics(aspect=48 / 36):
    """a sphere and a cylinder, each at least 40 pixels across at 48 x 36, over a floor, under one drawable light"""
    prims = [(RECTANGLE, flat((0, -1.5, 0), (0, 1, 0), 30.0), MATTE),
             (SPHERE, model((-0.9, 0.0, 0.6), np.eye(3), 1.5), GLOSSY),
             (CYLINDER, model((1.2, 0.6, -1.6), frame_about((1.0, 0.25, 0.1)), (1.1, 2.6, 1.1)), RED),
             (SPHERE, model((2.2, -0.7, 1.4), np.eye(3), (0.8, 0.8, 0.8)), MIRROR)]
    prims += shell((0, 6.0, 0), 9.0, (RED, GREEN, MATTE, MATTE, MATTE, MATTE), skip=(3,))
    L = flat((0.5, 6.0, 2.0), (0, -1, 0), 2.0)
    lights = [light_record(L, 0.05), light_record(L, 0.05)]
    return _tables(prims, lights, camera((0.3, 0.8, 5.2), (0.2, -0.1, 0.0), (0, 1, 0), 50.0, aspect), (0.3, 0.4, 0.6))


PATCHES = 8          # per edge of each of the detector's six faces


def patch_colours():
    """the colour of each of the detector's 6 x 8 x 8 patches: (1, 1 + a / 16, 1 + b / 32) with a = u + 8 (face % 2) in 0 .. 15 and
    b = v + 8 (face // 2) in 0 .. 23 -- exact in float32, the first channel > 0.01, and the two channel ratios of a pixel name its patch"""
    f, u, v = [a.reshape(-1) for a in np.mgrid[0:6, 0:PATCHES, 0:PATCHES]]
    c = np.stack([np.ones(len(f)), 1.0 + (u + 8 * (f % 2)) / 16.0, 1.0 + (v + 8 * (f // 2)) / 32.0], 1)
    unit = c / np.linalg.norm(c, axis=1, keepdims=True)
    assert (unit @ unit.T - 2.0 * np.eye(len(c))).max() < np.cos(1e-3)      # a thousand times a pixel's bound away from each other
    assert (c.astype(np.float32) == c).all()
    return c


DETECTOR_POSES = {"axis": ((0, 0, 1), 0.0), "rotated": ((0.3, -0.5, 0.8), 0.7), "tilted": ((0, 0.5, np.cos(np.radians(30.0))), 0.0)}


def detector(pose, specularity=None, aspect=48 / 36):
    """a target rectangle that fills the frame inside a closed cube (half-edge 6) of 6 x 8 x 8 patches, each of its own colour.
    specularity None: for path mode -- a diffuse target, emissive patches (Le = the colour), camera nearly head on: a pixel at max_depth 1 is
    kd (N . Ra) Le_patch.  Else for distributed mode, where an emitter would return white: the patches do not emit and carry the colour as kd,
    one surface light hangs in front of the target (it lights every patch a bounce can reach, and the target cannot come between), the target
    has kd = 0 and kr = 1 with that specularity, and the camera is oblique, so that Rr is not N: a pixel at max_depth 1 is the direct term
    of the patch its lobe's ray met.  Returns the tables and the target's weight (kd or kr)."""
    normal, spin = DETECTOR_POSES[pose]
    path = specularity is None
    weight = (0.75, 0.5, 0.625) if path else (1.0, 1.0, 1.0)
    target = weight + (0, 0, 0, 0, 0, 0, 0) if path else (0, 0, 0) + weight + (float(specularity), 0, 0, 0)
    prims = [(RECTANGLE, flat((0, 0, 0), normal, 3.0 if path else 7.0, spin), target)]
    colour = patch_colours()
    half, edge = 6.0, 12.0 / PATCHES
    k = 0
    for f in [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]:
        F = frame_about([-c for c in f])
        for iu in range(PATCHES):
            for iv in range(PATCHES):
                centre = half * np.asarray(f, np.float64) + F[:, 0] * (iu + 0.5 - PATCHES / 2) * edge + F[:, 2] * (iv + 0.5 - PATCHES / 2) * edge
                mat = (0, 0, 0, 0, 0, 0, 1.0) + tuple(colour[k]) if path else tuple(colour[k]) + (0, 0, 0, 1.0, 0, 0, 0)
                prims.append((RECTANGLE, flat(centre, [-c for c in f], edge), mat))
                k += 1
    n = _unit(normal)
    if path:
        lights = np.zeros((1, 16), np.float32)
        cam = camera(2.2 * n + np.array([0.3, 0.2, 0.0]), (0, 0, 0), (0, 1, 0), 40.0, aspect)
    else:
        lights = [light_record(flat(1.5 * n + np.array([-0.4, 0.3, 0.2]), -n, 0.5), 0.2)]
        cam = camera(2.6 * n + np.array([1.6, 0.9, 0.0]), (0, 0, 0), (0, 1, 0), 30.0, aspect)
    return _tables(prims, lights, cam, (0, 0, 0)), np.array(weight, np.float32)


SCENES = {"room": room, "two_lights": two_lights, "quadrics": quadrics}
