"""A float64 reference for the four analytic primitives, written from their geometry (numpy only: nothing of the oracle or the product is
imported here, so a slip the two share does not reach this file).

A primitive is a canonical shape in object space under a row-major 4 x 4 model matrix M (float32 values, widened).  A world ray (o, d)
becomes the object ray o' = inv(M) (o, 1), d' = inv(M) (d, 0); d is used as given, so t is in units of d and is the same number in both
spaces.  An object-space normal n' becomes the world direction transpose(inv(M)) n'.  The shapes and their rules:

  SPHERE     |p| = 1.  Only the NEAR root of |o' + t d'|^2 = 1 counts: a hit iff the discriminant is > 0 and that root is > 1e-4, so an
             origin inside the sphere sees nothing.  n' = o' + t d'.
  CYLINDER   x^2 + z^2 = 1, open, |y| < 1 (strict).  With a = d'x^2 + d'z^2, b = 2 (o'x d'x + o'z d'z), c = o'x^2 + o'z^2 - 1 the discriminant
             b^2 - 4ac must be > 1e-3 -- an absolute figure, so it scales with |d'|^2 -- and the hit is the smaller of the roots that are
             > 1e-3 and land at |y| < 1: from inside, or through an open end, that is the far wall.  n' = (x, 0, z), never flipped.
  DISK       y = 0, |p'|^2 < 1, seen from both sides; no hit when |d'y| < 0.01 (unnormalised: a short d never hits); t > 1e-4; n' = (0, 1, 0)
             from either side.
  RECTANGLE  y = 0, |x| < 1/2, |z| < 1/2 (open); t > 1e-4; seen only from the front, d'y < 0; n' = (0, 1, 0).

Every rule is a comparison, and float32 code may land on the other side of one that float64 decides narrowly.  So each comparison also
yields a MARGIN: its distance from the boundary, relative to the magnitude of what the compared quantity is summed from (the larger of
two cancelling terms, not their small difference).  With O = |o'| and D = |d'| the componentwise magnitudes of the object-space ray (the
cancellation inside inv(M) (o, 1) itself is not counted: the tests keep origins within ~40 units):
  discriminant against its threshold    relative to max(B^2, 4 A C) with A, B, C the quadratic's coefficients summed from O and D (+ 1 in C)
  a quadric's root against its threshold relative to (B + sqrt(max(B^2, 4 A C))) / 2a
  a plane's t = -o'y / d'y                relative to 2 max(|t|, threshold) (one relative error from o'y, one from d'y)
  |y| against 1, |x|, |z| against 1/2     relative to max(that bound, O + |t| D of the component)
  |p'|^2 against 1                        relative to max(1, |O + |t| D|^2)
  |d'y| against 0.01 or against 0         relative to max(D_y, 0.01)
Only the comparisons that decide the outcome count (a cylinder's far root is looked at only where the near one was refused).  The margin of
a (ray, primitive) pair is the smallest of them.

A ray is CLEAR (closest) when the winner's runner-up is at least 1e-4 max(1 / |d|, t) behind it, the winner is at least 1e-4 (relative) from
tmin and from tmax, and the margin of every primitive that could change the answer is at least 1e-4.  A primitive cannot change it when
the first t at which the ray could meet it at all -- a quadric's near root, the double root -b / 2a where the line misses it, a plane's t -- lies
5 % and the runner-up's lead behind the winner: however its comparisons fall, what it reports loses.  (Without this a ray is unclear as soon as it
passes ANY primitive narrowly, also behind its hit point: 16 to 23 % of the rays of a 48-primitive scene and 85 % of a 600-primitive scene's.)  A ray that
misses everything has no winner, and every primitive counts."""
import numpy as np

CYLINDER, DISK, RECTANGLE, SPHERE = 0, 1, 2, 3
T_EPS, T_EPS_CYLINDER, DISCR_EPS_CYLINDER, DISK_PARALLEL = 1e-4, 1e-3, 1e-3, 0.01
BEHIND = 1.05
CLEAR = 1e-4   # a ray is clear when every margin is at least this, and so are the winner's lead and its distance from the window's ends


def _rel(q, bound, scale):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(q - bound) / scale


def _object_rays(M, o, d):
    """M [p, 4, 4], o, d [r, 3] -> inv [p, 4, 4], o', d', O, D each [r, p, 3]"""
    inv = np.linalg.inv(M)
    A = inv[:, :3, :3]
    oo = np.einsum("pij,rj->rpi", A, o) + inv[None, :, :3, 3]
    dd = np.einsum("pij,rj->rpi", A, d)
    O, D = np.abs(oo), np.abs(dd)
    return inv, oo, dd, O, D


def _quadratic(a, b, c, A, B, Cm, discr_eps):
    """discriminant test and both roots: ok, near root, far root, margin of the discriminant, scale of a root's error, and the first t at
    which the quadric could be met at all (see `first` in intersect)"""
    discr = b * b - 4.0 * a * c
    big = np.maximum(np.maximum(B * B, 4.0 * A * Cm), discr_eps)
    m = _rel(discr, discr_eps, big)
    ok = discr > discr_eps
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(np.where(ok, discr, 0.0))
        near = np.where(ok, (-b - s) / (2.0 * a), np.inf)    # (a > 0 wherever ok: a = 0 gives b = 0 and discr = 0)
        far = np.where(ok, (-b + s) / (2.0 * a), np.inf)
        tscale = np.where(ok, (B + np.sqrt(big)) / (2.0 * a), 1.0)
        first = np.where(ok, near, np.where(a > 0.0, -b / (2.0 * a), -np.inf))    # the double root where the line misses
    return ok, near, far, m, tscale, first


def _sphere(oo, dd, O, D):
    a, b, c = (dd * dd).sum(-1), 2.0 * (oo * dd).sum(-1), (oo * oo).sum(-1) - 1.0
    ok, near, _, m, tscale, first = _quadratic(a, b, c, (D * D).sum(-1), 2.0 * (O * D).sum(-1), (O * O).sum(-1) + 1.0, 0.0)
    m = np.where(ok, np.minimum(m, _rel(near, T_EPS, np.maximum(tscale, T_EPS))), m)
    hit = ok & (near > T_EPS)
    t = np.where(hit, near, np.inf)
    n = oo + np.where(hit, t, 0.0)[..., None] * dd
    return t, n, m, first


def _cylinder(oo, dd, O, D):
    x, z = 0, 2
    a = dd[..., x] ** 2 + dd[..., z] ** 2
    b = 2.0 * (oo[..., x] * dd[..., x] + oo[..., z] * dd[..., z])
    c = oo[..., x] ** 2 + oo[..., z] ** 2 - 1.0
    ok, near, far, m, tscale, first = _quadratic(a, b, c, D[..., x] ** 2 + D[..., z] ** 2, 2.0 * (O[..., x] * D[..., x] + O[..., z] * D[..., z]),
                                          O[..., x] ** 2 + O[..., z] ** 2 + 1.0, DISCR_EPS_CYLINDER)

    def root(t):
        """is this root a hit, and how narrowly"""
        tf = np.where(np.isfinite(t), t, 0.0)
        mt = _rel(tf, T_EPS_CYLINDER, np.maximum(tscale, T_EPS_CYLINDER))
        y = oo[..., 1] + tf * dd[..., 1]
        my = _rel(np.abs(y), 1.0, np.maximum(1.0, O[..., 1] + np.abs(tf) * D[..., 1]))
        front = tf > T_EPS_CYLINDER
        return front & (np.abs(y) < 1.0), np.where(front, np.minimum(mt, my), mt)

    h_near, m_near = root(near)
    h_far, m_far = root(far)
    m = np.where(ok, np.minimum(m, np.where(h_near, m_near, np.minimum(m_near, m_far))), m)
    hit = ok & (h_near | h_far)
    t = np.where(hit, np.where(h_near, near, far), np.inf)
    p = oo + np.where(hit, t, 0.0)[..., None] * dd
    n = p * np.array([1.0, 0.0, 1.0])
    return t, n, m, first


def _plane(oo, dd):
    """t of y = 0 and the margin of t > 1e-4 (d'y = 0: no t; the callers' own test of d'y refuses such a ray first)"""
    oy, dy = oo[..., 1], dd[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dy != 0.0, -oy / dy, np.inf)
    tf = np.where(np.isfinite(t), t, 0.0)
    return t, tf, _rel(tf, T_EPS, 2.0 * np.maximum(np.abs(tf), T_EPS))


def _disk(oo, dd, O, D):
    dy = dd[..., 1]
    m = _rel(np.abs(dy), DISK_PARALLEL, np.maximum(D[..., 1], DISK_PARALLEL))
    facing = np.abs(dy) >= DISK_PARALLEL     # (the miss is |d'y| < 0.01)
    t, tf, mt = _plane(oo, dd)
    m = np.where(facing, np.minimum(m, mt), m)
    front = facing & (t > T_EPS)
    p = oo + tf[..., None] * dd
    P = O + np.abs(tf)[..., None] * D
    r2 = (p * p).sum(-1)
    m = np.where(front, np.minimum(m, _rel(r2, 1.0, np.maximum(1.0, (P * P).sum(-1)))), m)
    hit = front & (r2 < 1.0)
    n = np.broadcast_to(np.array([0.0, 1.0, 0.0]), oo.shape)
    return np.where(hit, t, np.inf), n, m, np.where(np.isfinite(t), t, -np.inf)


def _rectangle(oo, dd, O, D):
    dy = dd[..., 1]
    m = _rel(dy, 0.0, np.maximum(D[..., 1], DISK_PARALLEL))
    facing = dy < 0.0
    t, tf, mt = _plane(oo, dd)
    m = np.where(facing, np.minimum(m, mt), m)
    front = facing & (t > T_EPS)
    inside = front
    for k in (0, 2):
        q = oo[..., k] + tf * dd[..., k]
        m = np.where(front, np.minimum(m, _rel(np.abs(q), 0.5, np.maximum(0.5, O[..., k] + np.abs(tf) * D[..., k]))), m)
        inside = inside & (np.abs(q) < 0.5)
    n = np.broadcast_to(np.array([0.0, 1.0, 0.0]), oo.shape)
    return np.where(inside, t, np.inf), n, m, np.where(np.isfinite(t), t, -np.inf)


_SHAPES = {CYLINDER: _cylinder, DISK: _disk, RECTANGLE: _rectangle, SPHERE: _sphere}


def intersect(types, M, o, d):
    """every ray against every primitive.  types [p], M [p, 16] or [p, 4, 4], o, d [r, 3] -> t [r, p] (inf: no hit), the unit world normal
    [r, p, 3] (zero: no hit), the margin [r, p], and `first` [r, p]: the smallest t at which the primitive could be met if its narrow
    comparisons fell the other way -- a quadric's near root (where the line misses it, the double root -b / 2a), a plane's t; -inf where
    there is no such t"""
    types = np.asarray(types).reshape(-1)
    M = np.asarray(M, np.float64).reshape(-1, 4, 4)
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    inv, oo, dd, O, D = _object_rays(M, o, d)
    t = np.full((len(o), len(types)), np.inf)
    n = np.zeros((len(o), len(types), 3))
    m = np.zeros((len(o), len(types)))
    first = np.full((len(o), len(types)), -np.inf)
    for ty, shape in _SHAPES.items():
        cols = np.nonzero(types == ty)[0]
        if not len(cols):
            continue
        tt, nn, mm, ff = shape(oo[:, cols], dd[:, cols], O[:, cols], D[:, cols])
        nw = np.einsum("pji,rpj->rpi", inv[cols][:, :3, :3], nn)     # transpose(inv(M)) n'
        with np.errstate(divide="ignore", invalid="ignore"):
            nw = nw / np.linalg.norm(nw, axis=-1, keepdims=True)
        t[:, cols], m[:, cols], first[:, cols] = tt, mm, ff
        n[:, cols] = np.where(np.isfinite(tt)[..., None], nw, 0.0)
    return t, n, m, first


def closest(types, M, o, d, tmin=1e-3, tmax=1e16):
    """the scene-level answer: a hit is accepted iff tmin < t < tmax, the smallest t wins, ties go to the lowest index.  tmin, tmax: scalars
    or [r].  Returns dict(prim [r] (-1: miss), t [r] (inf: miss), n [r, 3], second [r] (the runner-up's t, inf: none), margin [r, p],
    clear [r])."""
    t, n, m, first = intersect(types, M, o, d)
    r = np.arange(len(t))
    tmin = np.broadcast_to(np.asarray(tmin, np.float64), (len(t),))
    tmax = np.broadcast_to(np.asarray(tmax, np.float64), (len(t),))
    found = np.isfinite(t)
    tw = np.where(found & (t > tmin[:, None]) & (t < tmax[:, None]), t, np.inf)
    prim = np.argmin(tw, axis=1)              # (the first of equal minima: the lowest index)
    best = tw[r, prim]
    rest = tw.copy()
    rest[r, prim] = np.inf
    second = rest.min(axis=1)
    hit = np.isfinite(best)
    # how narrowly the window itself decided, for every primitive the ray meets at all
    with np.errstate(invalid="ignore", divide="ignore"):
        win = np.where(found, np.minimum(np.abs(t - tmin[:, None]), np.abs(t - tmax[:, None])) / np.maximum(np.abs(t), 1e-300), np.inf)
    dlen = np.linalg.norm(np.asarray(d, np.float64).reshape(-1, 3), axis=1)
    tb = np.where(hit, best, 0.0)
    lead_ok = ~hit | (second - tb >= CLEAR * np.maximum(1.0 / dlen, tb))
    # a narrow comparison counts only where it can change the answer: not for a primitive that the ray can first meet well behind the winner
    # (BEHIND: 5 %, as a discriminant within 1e-4 of its larger term moves a root by up to 1 % of -b / 2a)
    behind = hit[:, None] & (first >= BEHIND * tb[:, None] + CLEAR * np.maximum(1.0 / dlen, tb)[:, None])
    behind[r, prim] = False
    counted = np.where(behind, np.inf, m)
    clear = (counted.min(axis=1) >= CLEAR) & lead_ok & (np.where(behind, np.inf, win).min(axis=1) >= CLEAR)
    return {"prim": np.where(hit, prim, -1), "t": best, "n": np.where(hit[:, None], n[r, prim], 0.0), "second": second, "margin": m,
            "counted": counted, "clear": clear}


def normal_sine(a, b):
    """sine of the angle between the directions a and b ([n, 3] each; neither needs unit length)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.linalg.norm(np.cross(a, b), axis=-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def reach(M, o):
    """|o - centre| + the spectral norm of M's 3 x 3 part: the length a relative rounding error of the hit point scales with.  M one
    matrix, o [r, 3] -> [r]"""
    M = np.asarray(M, np.float64).reshape(4, 4)
    return np.linalg.norm(np.asarray(o, np.float64) - M[:3, 3], axis=-1) + np.linalg.norm(M[:3, :3], 2)


# ---- inputs: model matrices, rays aimed at a primitive, hand-placed rays with known answers (shared by the CPU and the GPU tests) ----
def random_matrix(rng, sheared, spread=5.0, scales=(0.25, 4.0)):
    """M = T R [H] S as float32 [16], row-major: scales log-uniform in `scales` ([1/4, 4]) per axis, H a unit-diagonal shear with three off-diagonal
    entries in [-1/2, 1/2] (which three is drawn too), R a uniform rotation, the translation within +-spread"""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    A = q
    if sheared:
        H = np.eye(3)
        slots = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
        for k in rng.choice(6, 3, replace=False):
            H[slots[k]] = rng.uniform(-0.5, 0.5)
        A = A @ H
    A = A @ np.diag(np.exp(rng.uniform(np.log(scales[0]), np.log(scales[1]), 3)))
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = A, rng.uniform(-spread, spread, 3)
    return M.astype(np.float32).reshape(16)


def _interior(rng, ty, n):
    """n object-space points inside the primitive (the flat ones have no inside: points of the box around them, on either side)"""
    if ty == SPHERE:
        v = rng.normal(size=(n, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0, 1, (n, 1)) ** (1 / 3)
    if ty == CYLINDER:
        a, r = rng.uniform(0, 2 * np.pi, n), np.sqrt(rng.uniform(0, 1, n))
        return np.stack([r * np.cos(a), rng.uniform(-1, 1, n), r * np.sin(a)], 1)
    half = 1.0 if ty == DISK else 0.5
    return np.stack([rng.uniform(-half, half, n), rng.uniform(-1, 1, n), rng.uniform(-half, half, n)], 1)


def aimed_rays(rng, ty, M, n, origins=None):
    """n float32 rays, each aimed at a random point of the image of the 1.2 x unit cube under M; a quarter of the origins inside the
    primitive's image, the rest 1 to 30 units from its centre (or the given origins); |d| log-uniform in [0.1, 10]"""
    M = np.asarray(M, np.float64).reshape(4, 4)
    target = rng.uniform(-1.2, 1.2, (n, 3)) @ M[:3, :3].T + M[:3, 3]
    if origins is None:
        v = rng.normal(size=(n, 3))
        origins = M[:3, 3] + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(1.0, 30.0, (n, 1))
        k = n // 4
        origins[:k] = _interior(rng, ty, k) @ M[:3, :3].T + M[:3, 3]
    d = target - origins
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * np.exp(rng.uniform(np.log(0.1), np.log(10.0), (n, 1)))
    return origins.astype(np.float32), d.astype(np.float32)


IDENTITY = np.eye(4, dtype=np.float32).reshape(16)
# one sheared, non-uniformly scaled matrix for the hand-placed rays: rotation about (1, 2, 3) by 0.7, shear, scale (2, 0.5, 1.25)
def _sheared_matrix():
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K
    H = np.array([[1, 0.4, 0], [0, 1, -0.3], [0.25, 0, 1]])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R @ H @ np.diag([2.0, 0.5, 1.25]), [1.5, -2.0, 0.75]
    return M.astype(np.float32).reshape(16)


SHEARED = _sheared_matrix()
_S2 = np.sqrt(0.5)
# (name, type, object-space origin, object-space direction, the answer: None for a miss, else (t, n'));  every origin is at least 1e-2
# off every surface, t is the same number in world space
KNOWN = [
    ("sphere: origin inside", SPHERE, (0.2, 0.1, -0.3), (0, 0, 1), None),
    ("sphere: outside, pointing away", SPHERE, (0, 0, 3), (0, 0, 1), None),
    ("sphere: outside, pointing at it: the near root", SPHERE, (0, 0, 3), (0, 0, -1), (2.0, (0, 0, 1))),
    ("sphere: off-centre, the near root", SPHERE, (0.6, 0, 3), (0, 0, -1), (3 - 0.8, (0.6, 0, 0.8))),
    ("cylinder: origin inside: the far wall, normal outward", CYLINDER, (0.5, 0.2, 0), (1, 0, 0), (0.5, (1, 0, 0))),
    ("cylinder: through the open end: the near root lands at y = 2, the far root at y = 0", CYLINDER, (-2, 3, 0), (1, -1, 0), (3.0, (1, 0, 0))),
    ("cylinder: from above the open end, inside the bore: the far wall", CYLINDER, (0, 2, 0), (0.5, -1, 0), (2.0, (1, 0, 0))),
    ("cylinder: along the axis", CYLINDER, (0.3, -3, 0.2), (0, 1, 0), None),
    ("cylinder: both roots beyond the ends", CYLINDER, (-3, 4, 0), (1, -0.2, 0), None),
    ("cylinder: from outside: the near root", CYLINDER, (3, 0.5, 0), (-1, 0, 0), (2.0, (1, 0, 0))),
    ("cylinder: a near root of 5e-4 in units of d is refused: the far wall", CYLINDER, (1.01, 0.3, 0), (-20, 0, 0), (2.01 / 20, (-1, 0, 0))),
    ("sphere: a near root of 5e-5 in units of d: a miss", SPHERE, (0, 0, 1.01), (0, 0, -200), None),
    ("sphere: a near root of 5e-4 in units of d: a hit", SPHERE, (0, 0, 1.01), (0, 0, -20), (5e-4, (0, 0, 1))),
    ("disk: from above", DISK, (0.3, 2, 0.2), (0, -1, 0), (2.0, (0, 1, 0))),
    ("disk: from below, the same normal", DISK, (0.3, -2, 0.2), (0, 1, 0), (2.0, (0, 1, 0))),
    ("disk: |d'y| = 0.009: a miss", DISK, (-0.5, 0.009, 0), (np.sqrt(1 - 0.009 ** 2), -0.009, 0), None),
    ("disk: |d'y| = 0.011: a hit", DISK, (-0.5, 0.011, 0), (np.sqrt(1 - 0.011 ** 2), -0.011, 0), (1.0, (0, 1, 0))),
    ("disk: outside the rim", DISK, (0.8, 1, 0.7), (0, -1, 0), None),
    ("disk: hits with |d| = 1", DISK, (0.1, 1.5, -0.2), (0, -1, 0), (1.5, (0, 1, 0))),
    ("disk: the same ray, d x 0.005: a miss", DISK, (0.1, 1.5, -0.2), (0, -0.005, 0), None),
    ("rectangle: from the front", RECTANGLE, (0.2, 1, -0.3), (0, -1, 0), (1.0, (0, 1, 0))),
    ("rectangle: the same line from the back", RECTANGLE, (0.2, -1, -0.3), (0, 1, 0), None),
    ("rectangle: 1e-2 outside an edge", RECTANGLE, (0.51, 1, 0), (0, -1, 0), None),
    ("rectangle: 1e-2 inside an edge, slanted", RECTANGLE, (0.49 + 0.5, 1, -0.49 - 0.25), (-0.5, -1, 0.25), (1.0, (0, 1, 0))),
]
# one hitting ray per type for the units of dir: (o, s d) for s in SCALES gives t / s, or misses where a threshold in units of d says so
SCALES = (0.01, 1.0, 100.0)
UNITS = [
    (SPHERE, (0.3, 0.2, 3), (0, 0, -1)),
    (CYLINDER, (3, 0.4, 0), (-1, 0, 0)),             # discriminant 4 s^2: 4e-4 at s = 0.01, under the cylinder's 1e-3
    (DISK, (0.2, 2, 0.1), (0.1, -0.8, 0.1)),        # |d'y| = 0.008 at s = 0.01, under the disk's 0.01
    (RECTANGLE, (0.1, 2, 0.1), (0.05, -1, -0.05)),
]


def to_world(M, o_obj, d_obj):
    """an object-space ray as the float32 world ray under M"""
    M = np.asarray(M, np.float64).reshape(4, 4)
    return ((M[:3, :3] @ np.asarray(o_obj, np.float64) + M[:3, 3]).astype(np.float32), (M[:3, :3] @ np.asarray(d_obj, np.float64)).astype(np.float32))
