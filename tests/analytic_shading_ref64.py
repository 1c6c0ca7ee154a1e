"""A float64 statement of what the analytic path does around its intersectors: the random numbers, the primary ray, the lobe sampler, the
closest-hit program in its three modes, the occlusion program, the miss colour, the mean, the running average and the byte.  Numpy only; the
hits come from tests/analytic_ref64.py, and nothing of the oracle or the product is imported, so a slip those two share does not reach this
file.  Float32 appears only where a rule says so: the draws (k / 2^24, exact), the stored scene and camera, pi as the float32 constant, the
light index (one float32 product, see light_index), the reciprocals of the mean and of the running average, and the byte.

THE RULES
  random numbers   seed = tea<16>(width * py + px, frame_count); lcg: s <- 1664525 s + 1013904223 mod 2^32, k = s & 0xFFFFFF; rnd = k / 2^24.
  primary ray      for sample (i, j), i outer: r0, r1 = rnd, rnd (x first); dx = 2 (px + (i + r0) / n) / width - 1, dy likewise with j, r1, height;
                   o = eye, d = normalize(dx U + dy V + W), window [0.05, 1e16], depth 0, and the seed as it stands after the two draws -- by
                   value: what the path draws never comes back, the next sample goes on from the caller's copy.
  lobe             hemisphere(normal, direction, c, seed): per draw r1, r2 = rnd, rnd; phi = 2 pi_f r1; theta = acos((1 - r2)^(1 / (c + 1)));
                   Y = normalize(direction), X = normalize(Y.y - Y.z, -Y.x, Y.x), Z = Y x X; ray = sin theta cos phi X + cos theta Y - sin theta sin phi Z;
                   repeat while normal . ray < 0, at most 1024 draws (the last is kept).  |(Y.y - Y.z, -Y.x, Y.x)| < 1e-6 is DEGENERATE: X is
                   whatever rounding leaves (0 / 0 in exact arithmetic: a NaN ray, which ends the loop because NaN < 0 is false).
  closest hit      N = normalize(n), x = o + t normalize(d), V = normalize(o - x), N flipped where N . V < 0, rayEpsilon = 1e-6 max(t^2, 1).
    path           Le.x > 0.01: Le.  Else at depth < max: Ra = lobe(N, N, 0), child from x over [rayEpsilon, 1e6] at depth + 1 with the seed after
                   the draws, payload kd (N . Ra) child; at depth == max: black.
    distributed    length(Le) > 0.01: white.  l = int(rnd (n_lights - 1)), then r_a, r_b; samplingPos = corner + r_a v1 + r_b v2;
                   Lm = normalize(samplingPos - x), lightDistance = |samplingPos - x|; the occlusion ray (x, Lm) over
                   [rayEpsilon, lightDistance - rayEpsilon] draws nothing and returns min(Le, 1) of what it hits, (1, 1, 1) on a miss;
                   direct = |Lm . n_light| illumination max(N . Lm, 0) kd / (1 + falloff lightDistance) (the light's colour is not used).
                   At depth < max, with Rr = d^ - 2 (N . d^) N:  without ambient one child, weight kr: lobe(N, N, 0) when specularity < 0.5, else
                   lobe(N, Rr, specularity);  with ambient a child only when specularity > 0.5, and 0.1 kd is added (not at depth == max).
  miss             the background.   mean: sum of the n^2 payloads times float32(1 / n^2).   running average: prev + (cur - prev) float32(1 / (frame + 1)).
  byte             int(clamp(c, 0, 1) * 255), truncated.

MARGINS.  Every rule that is a comparison names how narrowly it was decided, so that a test can set aside the cases float32 may decide the
other way (CLEAR):
  a lobe draw      |normal . ray| / |normal| against HEMI_CLEAR direction_units (kappa_h plus the frame's term, below), kappa_h = 1 + 1 / max(sin theta, 2^-12): u = (1 - r2)^(1 / (c + 1)) is placed
                   by float32 to 2^-24 u, so theta to 2^-24 u / sin theta, and phi to 2^-22; a direction is judged in units of 2^-23 kappa_h.
  the flip         |N . V| >= 1e-5, plus the noise of V itself, 2^-21 (|o| + |x|) / t (V = normalize(o - x) is rounding noise when t is tiny
                   against the coordinates).
  Le.x > 0.01, specularity against 0.5: stored float32 values against float32 constants: exact, no margin.
  length(Le) > 0.01: |length - 0.01| >= 1e-5 x 0.01.
  the light index: rnd is k / 2^24 exactly and n_lights - 1 is a small integer, so the float32 product is ONE correctly rounded operation on
                   exact operands: computing it in float32 here gives the same bits on any IEEE machine, and there is nothing to be narrow
                   about.  (It is not the real product: k (n - 1) can need 28 bits, and 9 (1 - 2^-24) rounds to 9.0.)
  an occlusion ray is clear by analytic_ref64.closest's rule on its window: a clear hit well inside, or nothing that comes close WITHIN the
                   window (_occluders); and it need not be clear where N . Lm < -1e-4, as the direct term is zero there whatever it meets.

KAPPA of a pixel: one term per factor that cancels, weighted by the share of the colour it carries.  Each bounce adds to everything beyond it
1 / sin theta of its lobe (acos' condition: the child sets off in a direction placed to 2^-23 kappa_h, and what it meets moves with it -- a
mirror's lobe has kappa_h in the hundreds) and, in path mode, 1 / (N . Ra) (1 / (1 - r2) for the diffuse lobe); each direct term carries
1 / (N . Lm), 1 / |Lm . n_light| and (|samplingPos| + |x|) / lightDistance of its own, stated as the size of what each factor's rounding moves
so that a point where N . Lm is zero to rounding (one computation sees the light, the other does not) is weighed like its neighbours.
A hit on a sphere or a cylinder adds (|o - centre| + ||M||) / sigma_min(M) / (N . V)^2 to itself and to everything beyond (curved_hit_kappa).
kappa = 1 + sum_k share_k (bounces before k + the direct term's own).  What no local factor states is the lever arm of a direction's
last bit on the NEXT hit point (a bounce off a small sphere multiplies it by 2 d / r): the whole-pipeline figures of DESIGN.md 4 show what that
leaves, and check_nodes, which judges every node from its own logged inputs, is not subject to it."""
import numpy as np

import analytic_ref64 as A

UNIT = 2.0 ** -23
PI_F = float(np.float32(np.pi))
HEMI_MAX_DRAWS = 1024
HEMI_CLEAR = 16 * UNIT     # a rejection draw is clear when |normal . ray| >= 16 x 2^-23 direction_units |normal|: twice the loosest lobe bound
FLIP_CLEAR = 1e-5
NLM_NEAR = 1e-4            # N . Lm below -NLM_NEAR: float32 cannot see the light from there either
DEGENERATE = 1e-6
LE_PATH = float(np.float32(0.01))
RADIANCE, OCCLUSION = 0, 1
T_MIN0, T_MAX0, T_MAX_CHILD = float(np.float32(0.05)), float(np.float32(1e16)), 1e6
_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ random numbers
def tea16(v0, v1):
    v0, v1 = np.asarray(v0, np.uint64) & _M32, np.asarray(v1, np.uint64) & _M32
    v0, v1 = np.broadcast_arrays(v0, v1)
    v0, v1 = v0.copy(), v1.copy()
    s0 = np.uint64(0)
    for _ in range(16):
        s0 = (s0 + np.uint64(0x9E3779B9)) & _M32
        v0 = (v0 + ((((v1 << np.uint64(4)) + np.uint64(0xA341316C)) & _M32) ^ ((v1 + s0) & _M32) ^ (((v1 >> np.uint64(5)) + np.uint64(0xC8013EA4)) & _M32))) & _M32
        v1 = (v1 + ((((v0 << np.uint64(4)) + np.uint64(0xAD90777D)) & _M32) ^ ((v0 + s0) & _M32) ^ (((v0 >> np.uint64(5)) + np.uint64(0x7E95761E)) & _M32))) & _M32
    return v0.astype(np.uint32)


def lcg(seed):
    """seed [n] uint32 -> (the next seed, its low 24 bits)"""
    s = (np.asarray(seed, np.uint64) * np.uint64(1664525) + np.uint64(1013904223)) & _M32
    return s.astype(np.uint32), (s & np.uint64(0xFFFFFF)).astype(np.int64)


def rnd(seed):
    """-> (the next seed, k / 2^24 as float64: an exact float32)"""
    s, k = lcg(seed)
    return s, k / 16777216.0


def lcg_back(seed):
    """the seed whose successor is `seed` (1664525 is odd, so the step is a bijection of 2^32)"""
    inv = pow(1664525, -1, 1 << 32)
    return np.uint32(((int(seed) - 1013904223) * inv) & 0xFFFFFFFF)


def seed_for_draws(ks, high=0):
    """a seed whose first draw is ks[0] / 2^24 (the top byte of the state after that draw is `high`); for more than one k the following
    draws are searched over `high`: returns the seed or None"""
    ks = list(ks)
    for h in ([high] if len(ks) == 1 else range(256)):
        state = np.uint32((h << 24) | ks[0])
        s, ok = state, True
        for k in ks[1:]:
            s, got = lcg(s)
            ok = ok and int(got) == k
        if ok:
            return lcg_back(state)
    return None


# ------------------------------------------------------------------------------------------------ vectors
def _dot(a, b):
    return (a * b).sum(-1)


def _unit(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / np.linalg.norm(a, axis=-1, keepdims=True)


def _cond(a, b):
    """sum |a_i b_i|: what a rounding of the dot product a . b scales with"""
    return (np.abs(a) * np.abs(b)).sum(-1)


# ------------------------------------------------------------------------------------------------ the primary ray
def primary_rays(cam, width, height, px, py, n, frame_count):
    """cam: 12 float32 (eye, U, V, W); px, py [p] -> o [p, n^2, 3], d [p, n^2, 3] (unit), seed [p, n^2] as handed to the path"""
    cam = np.asarray(cam, np.float64)
    eye, U, V, W = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    seed = tea16(width * py + px, np.full(len(px), frame_count))
    ds, seeds = [], []
    for i in range(n):
        for j in range(n):
            seed, r0 = rnd(seed)
            seed, r1 = rnd(seed)
            dx = 2.0 * ((px + (i + r0) / n) / width) - 1.0
            dy = 2.0 * ((py + (j + r1) / n) / height) - 1.0
            ds.append(_unit(dx[:, None] * U + dy[:, None] * V + W))
            seeds.append(seed.copy())
    d = np.stack(ds, 1)
    return np.broadcast_to(eye, d.shape).copy(), d, np.stack(seeds, 1)


# ------------------------------------------------------------------------------------------------ the lobe
def kappa_h(theta):
    return 1.0 + 1.0 / np.maximum(np.sin(theta), 2.0 ** -12)


def direction_units(theta, frame):
    """what a lobe direction is judged in, over 2^-23: kappa_h, and sin theta / |(Y.y - Y.z, -Y.x, Y.x)| for the frame: X = normalize of that
    vector takes the rounding of Y's components, 2^-24 each, divided by its length (sqrt(1 + Y.x^2 - 2 Y.y Y.z) >= 0.7 away from (0, a, a))"""
    return kappa_h(theta) + np.sin(theta) * frame


def hemisphere(normal, direction, c, seed):
    """normal, direction [n, 3], c [n] or scalar, seed [n] uint32 -> dict(ray, seed, draws, theta, margin (the smallest over the draws, already
    divided by direction_units |normal|), degenerate, exhausted, clear, frame: 1 / |(Y.y - Y.z, -Y.x, Y.x)|)"""
    normal, direction = np.asarray(normal, np.float64).reshape(-1, 3), np.asarray(direction, np.float64).reshape(-1, 3)
    n = len(normal)
    c = np.broadcast_to(np.asarray(c, np.float64), (n,))
    seed = np.array(seed, np.uint32).reshape(n).copy()
    Y = _unit(direction)
    Xr = np.stack([Y[:, 1] - Y[:, 2], -Y[:, 0], Y[:, 0]], 1)
    xl = np.linalg.norm(Xr, axis=1)
    degenerate = ~(xl >= DEGENERATE)
    with np.errstate(invalid="ignore", divide="ignore"):
        X = Xr / xl[:, None]
    Z = np.cross(Y, X)
    nl = np.linalg.norm(normal, axis=1)
    ray, theta = np.zeros((n, 3)), np.zeros(n)
    draws, margin, active = np.zeros(n, np.int64), np.full(n, np.inf), np.ones(n, bool)
    for _ in range(HEMI_MAX_DRAWS):
        k = np.nonzero(active)[0]
        if not len(k):
            break
        s, r1 = rnd(seed[k])
        s, r2 = rnd(s)
        seed[k] = s
        phi = 2.0 * PI_F * r1
        th = np.arccos((1.0 - r2) ** (1.0 / (c[k] + 1.0)))
        st, ct = np.sin(th), np.cos(th)
        r = (st * np.cos(phi))[:, None] * X[k] + ct[:, None] * Y[k] - (st * np.sin(phi))[:, None] * Z[k]
        dn = _dot(normal[k], r)
        with np.errstate(invalid="ignore", divide="ignore"):
            margin[k] = np.fmin(margin[k], np.abs(dn) / (direction_units(th, 1.0 / xl[k]) * nl[k]))
            active[k] = dn < 0.0
        ray[k], theta[k] = r, th
        draws[k] += 1
    clear = (margin >= HEMI_CLEAR) & ~degenerate & ~active
    return {"ray": ray, "seed": seed, "draws": draws, "theta": theta, "margin": margin, "degenerate": degenerate, "exhausted": active,
            "clear": clear, "frame": 1.0 / np.maximum(xl, 1e-300)}


# ------------------------------------------------------------------------------------------------ the closest-hit program
def light_index(r, n_lights):
    """int(rnd * (n_lights - 1)) as ONE float32 product of exact operands (see the docstring): never the last light once there are two"""
    return (np.asarray(r, np.float32) * np.float32(n_lights - 1)).astype(np.int64)


def closest_hit(o, d, t, n, mat, depth, seed, lights, path, ambient, max_depth):
    """One node per row: the ray (o, d), its hit (t, the unnormalised n), the material row (kd, kr, specularity, Le), depth and the seed as
    the program received it; lights [nl, 16] (corner, v1, v2, normal, colour, falloff).  Returns what the program does next: N, x, eps,
    `final` (the payload is `value` and nothing is traced), the occlusion ray (occ, Lm, dist, sp, light), the radiance child (rad, rad_dir,
    rad_seed, theta), `clear`, and the terms payload() needs."""
    o, d, n = (np.asarray(a, np.float64).reshape(-1, 3) for a in (o, d, n))
    t, mat = np.asarray(t, np.float64).reshape(-1), np.asarray(mat, np.float64).reshape(-1, 10)
    depth, seed = np.asarray(depth, np.int64).reshape(-1), np.array(seed, np.uint32).reshape(-1).copy()
    m = len(t)
    kd, kr, spec, Le = mat[:, 0:3], mat[:, 3:6], mat[:, 6], mat[:, 7:10]
    dn = _unit(d)
    x = o + t[:, None] * dn
    V = -dn                                     # normalize(o - x) with t > 0
    N = _unit(n)
    nv = _dot(N, V)
    N = np.where((nv < 0.0)[:, None], -N, N)
    with np.errstate(divide="ignore", invalid="ignore"):
        clear = np.abs(nv) >= FLIP_CLEAR + 4 * UNIT * (np.linalg.norm(o, axis=1) + np.linalg.norm(x, axis=1)) / t
    eps = 1e-6 * np.maximum(t * t, 1.0)
    out = {"N": N, "x": x, "eps": eps, "kd": kd, "kr": kr, "value": np.zeros((m, 3)), "ambient": np.zeros((m, 3)),
           "occ": np.zeros(m, bool), "Lm": np.zeros((m, 3)), "dist": np.zeros(m), "sp": np.zeros((m, 3)), "light": np.zeros(m, np.int64),
           "nl": np.zeros((m, 3)), "falloff": np.zeros(m), "theta": np.zeros(m), "frame": np.ones(m), "hemi_draws": np.zeros(m, np.int64),
           "rad_dir": np.zeros((m, 3)), "rad_seed": seed.copy(), "path": bool(path)}
    more = depth < max_depth
    if path:
        emit = Le[:, 0] > LE_PATH
        out["value"][emit] = Le[emit]
        rad = ~emit & more
        lobe_dir, lobe_c = N.copy(), np.zeros(m)
    else:
        ll = np.linalg.norm(Le, axis=1)
        emit = ll > 0.01
        clear &= np.abs(ll - 0.01) >= 1e-5 * 0.01
        out["value"][emit] = 1.0
        lights = np.asarray(lights, np.float64).reshape(-1, 16)
        seed, r = rnd(seed)
        li = light_index(r, len(lights))
        seed, ra = rnd(seed)
        seed, rb = rnd(seed)
        L = lights[li]
        sp = L[:, 0:3] + ra[:, None] * L[:, 3:6] + rb[:, None] * L[:, 6:9]
        dist = np.linalg.norm(sp - x, axis=1)
        out.update(occ=~emit, Lm=_unit(sp - x), dist=dist, sp=sp, light=li, nl=L[:, 9:12], falloff=L[:, 15])
        Rr = dn - 2.0 * _dot(N, dn)[:, None] * N
        glossy = spec > 0.5 if ambient else ~(spec < 0.5)
        rad = ~emit & more & (glossy if ambient else True)
        if ambient:
            out["ambient"][~emit & more] = 0.1 * kd[~emit & more]
        lobe_dir, lobe_c = np.where(glossy[:, None], Rr, N), np.where(glossy, spec, 0.0)
    k = np.nonzero(rad)[0]
    h = hemisphere(N[k], lobe_dir[k], lobe_c[k], seed[k])
    out["rad_dir"][k], out["theta"][k], out["hemi_draws"][k], out["frame"][k] = h["ray"], h["theta"], h["draws"], h["frame"]
    seed[k] = h["seed"]
    clear[k] &= h["clear"]
    out.update(final=emit, rad=rad, rad_seed=seed, clear=clear, degenerate=np.zeros(m, bool), exhausted=np.zeros(m, bool))
    out["degenerate"][k], out["exhausted"][k] = h["degenerate"], h["exhausted"]
    return out


def payload(node, rad_dir, rad_payload, Lm, illumination):
    """the program's formula on a node of closest_hit, with the child directions and child payloads the caller names (the reference's own, or
    float32 values from a log).  Returns (payload [m, 3], scale [m, 3]: the payload's rounding scales with 2^-23 scale -- the sum of every term
    times the condition numbers of its dot products -- and the direct term alone [m, 3])"""
    N, kd, kr = node["N"], node["kd"], node["kr"]
    rad, occ = node["rad"], node["occ"]
    m = len(N)
    value, scale, direct = node["value"].copy(), np.abs(node["value"]), np.zeros((m, 3))
    if node["path"]:
        c, s = _dot(N, rad_dir), _cond(N, rad_dir)
        value[rad] = (kd * c[:, None] * rad_payload)[rad]
        scale[rad] = (kd * s[:, None] * np.abs(rad_payload))[rad]
        return value, scale, direct
    a, sa = np.abs(_dot(Lm, node["nl"])), _cond(Lm, node["nl"])
    b, sb = np.maximum(_dot(N, Lm), 0.0), _cond(N, Lm)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = 1.0 / (1.0 + node["falloff"] * node["dist"])
        reach = (np.linalg.norm(node["sp"], axis=1) + np.linalg.norm(node["x"], axis=1)) / node["dist"]
    direct[occ] = ((a * b * f)[:, None] * illumination * kd)[occ]
    dscale = ((sa * b + a * sb + a * b * (1.0 + reach)) * f)[:, None] * illumination * kd
    value[occ] = direct[occ]
    scale[occ] = dscale[occ]
    value[rad] += (kr * rad_payload)[rad]
    scale[rad] += np.abs(kr * rad_payload)[rad]
    value += node["ambient"]
    scale += node["ambient"]
    return value, scale, direct


def occlusion_payload(Le):
    return np.minimum(np.asarray(Le, np.float64), 1.0)


# ------------------------------------------------------------------------------------------------ raygen's tail
def mean(total, n):
    """the sum of the n^2 payloads times the float32 reciprocal"""
    return np.asarray(total, np.float64) * float(np.float32(1.0) / np.float32(n * n))


def running_average(prev, cur, frame_count):
    if frame_count == 0:
        return np.asarray(cur, np.float64)
    prev = np.asarray(prev, np.float64)
    return prev + (cur - prev) * float(np.float32(1.0) / np.float32(frame_count + 1))


def byte(c):
    """make_color's truncation; also how far c * 255 is from an integer (a test compares exactly only beyond 1e-3)"""
    v = np.clip(np.asarray(c, np.float64), 0.0, 1.0) * 255.0
    v = np.where(np.isnan(v), 255.0, v)       # clamp is fmaxf(0, fminf(c, 1)), and fminf(NaN, 1) is 1
    return np.floor(v).astype(np.int64), np.abs(v - np.round(v))


# ------------------------------------------------------------------------------------------------ drivers
PLANE_UNITS = 16.0       # 4 x what the case that showed this needed (a wall 0.01 under the origin of a ray along it, reach 24: t off by 1.2e-3)


def _skims_a_plane(scene, o, d, tmin, tmax, best, winner):
    """analytic_ref64's margins leave one cancellation out, as its docstring says: the object-space origin inv(M) (o, 1) itself.  For a flat
    primitive that matters when the origin lies close above its plane without lying on it -- a hit point next to a room's corner: the
    height o'y is then a small difference of coordinates, and t = -o'y / d'y is placed to 2^-23 reach / height only, times the inverse's own
    few dozen units.  A ray is set aside when such a plane's t (height above 1e-5 of the reach: not the surface the ray leaves) comes within
    PLANE_UNITS x 2^-23 reach / height, relative, of what it is compared with: the window's ends and the t of a winner other than itself (`best`, inf: none)."""
    types, M = np.asarray(scene["type"]).reshape(-1), np.asarray(scene["M"], np.float64).reshape(-1, 4, 4)
    out = np.zeros(len(o), bool)
    lo, hi = np.broadcast_to(tmin, (len(o),)), np.broadcast_to(tmax, (len(o),))
    for p in np.nonzero((types == A.DISK) | (types == A.RECTANGLE))[0]:
        inv = np.linalg.inv(M[p])
        oy = o @ inv[1, :3] + inv[1, 3]
        dy = d @ inv[1, :3]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -oy / dy
            reach = A.reach(M[p], o)
            height = np.abs(oy) / np.linalg.norm(inv[1, :3])
            band = PLANE_UNITS * UNIT * reach / height
            near = np.zeros(len(o), bool)
            for b in (lo, hi, np.where(winner == p, np.inf, best)):
                near |= np.isfinite(b) & (np.abs(t - b) < band * np.abs(t)) & (np.abs(t - b) > 0)
        out |= (height > 1e-5 * reach) & (t > 0) & near
        if types[p] == A.DISK:
            # a ray that leaves a disk it lies on: float32 places the origin some 2^-23 reach off the plane, on either side, and a disk is
            # met from both: at a grazing angle the plane is met again beyond tmin (a rectangle is met from the front only, which a ray
            # that leaves it never faces; one that enters it has N . Lm < 0 and adds nothing)
            with np.errstate(divide="ignore", invalid="ignore"):
                again = 8.0 * UNIT * reach / (np.abs(dy) / np.linalg.norm(inv[1, :3]))
            out |= (height <= 1e-5 * reach) & (again > lo)
    return out


def _closest(scene, o, d, tmin, tmax, chunk=4096):
    r = _closest_raw(scene, o, d, tmin, tmax, chunk)
    if len(o):
        r["clear"] = r["clear"] & ~_skims_a_plane(scene, o, d, tmin, tmax, r["t"], r["prim"])
    return r


def _closest_raw(scene, o, d, tmin, tmax, chunk=4096):
    parts = [A.closest(scene["type"], scene["M"], o[k:k + chunk], d[k:k + chunk], np.broadcast_to(tmin, (len(o),))[k:k + chunk],
                       np.broadcast_to(tmax, (len(o),))[k:k + chunk]) for k in range(0, len(o), chunk)]
    if not parts:
        return {"prim": np.zeros(0, np.int64), "t": np.zeros(0), "n": np.zeros((0, 3)), "clear": np.zeros(0, bool)}
    return {key: np.concatenate([p[key] for p in parts]) for key in ("prim", "t", "n", "clear")}


def _occluders(scene, o, d, tmin, tmax):
    """_closest for an occlusion ray.  analytic_ref64.closest counts, for a ray that misses, every primitive the ray's LINE passes narrowly,
    however far beyond the window; here a primitive that the ray can first meet 5 % beyond tmax is left out, as one behind a winner is
    there: however its comparisons fall, what it reports is outside the window."""
    r = _closest_raw(scene, o, d, tmin, tmax)
    skims = _skims_a_plane(scene, o, d, tmin, tmax, r["t"], r["prim"])
    redo = np.nonzero((r["prim"] < 0) & ~r["clear"])[0]
    if len(redo):
        t, _, m, first = A.intersect(scene["type"], scene["M"], o[redo], d[redo])
        lo, hi = np.broadcast_to(tmin, (len(o),))[redo][:, None], np.broadcast_to(tmax, (len(o),))[redo][:, None]
        beyond = first >= A.BEHIND * hi
        with np.errstate(invalid="ignore", divide="ignore"):
            win = np.where(np.isfinite(t), np.minimum(np.abs(t - lo), np.abs(t - hi)) / np.maximum(np.abs(t), 1e-300), np.inf)
        r["clear"][redo] = (np.where(beyond, np.inf, m).min(1) >= A.CLEAR) & (np.where(beyond, np.inf, win).min(1) >= A.CLEAR)
    r["clear"] = r["clear"] & ~skims
    return r


def curved_hit_kappa(scene, prim, o, node):
    """what a sphere's or a cylinder's hit adds to kappa: N is read off the hit point, so the intersector's placement of x -- some units of
    2^-23 reach (tests/test_oracle_float64.py) -- turns N by that over the radius of curvature, at most the smallest scale of M; and the
    near root of the quadratic is found through b^2 - 4ac, which cancels as 1 / (N . V)^2 towards the silhouette.  Zero for the flat ones."""
    types, M = np.asarray(scene["type"]).reshape(-1), np.asarray(scene["M"], np.float64).reshape(-1, 4, 4)
    out = np.zeros(len(prim))
    for p in np.unique(prim):
        if types[p] in (A.SPHERE, A.CYLINDER):
            q = prim == p
            nv = np.abs(_dot(node["N"][q], _unit(o[q] - node["x"][q])))
            out[q] = A.reach(M[p], o[q]) / np.linalg.svd(M[p][:3, :3], compute_uv=False).min() / np.maximum(nv, 1e-3) ** 2
    return out


def render(scene, frame, prev=None):
    """scene: dict(type, M, mat, lights, cam, bg) as the C ABI takes them; frame: dict(width, height, sqrt_spp, max_depth, frame_count, path,
    ambient).  Follows every path in float64.  Returns dict: accum [h, w, 3] (after the running average over prev [h, w, 3 or 4]), sample
    [h, w, n^2, 3], byte, byte_slack, clear [h, w], kappa [h, w], chain (per pixel and sample: the list of (primitive, kind)), hits
    [h, w, n^2] (hits on the radiance chain), lit / shadowed [h, w] (distributed: a primary hit's occlusion ray missed / was blocked, in any sample),
    rays_radiance [depth] and rays_occlusion as (clear, unclear) counts -- a ray is counted unclear when its path had stopped being clear before it
    was traced -- and clear_paths [h w n^2]; clear_chain [h, w]: clear, and every occlusion ray clear and leaving its surface (N . Lm > 1e-4): one that enters it
    adds nothing to the colour, but float32 may meet the surface again where float64 starts on it."""
    W, H, n, md = frame["width"], frame["height"], frame["sqrt_spp"], frame["max_depth"]
    path, ambient = bool(frame["path"]), bool(frame.get("ambient", False))
    py, px = [a.reshape(-1) for a in np.mgrid[0:H, 0:W]]
    o, d, seed = primary_rays(scene["cam"], W, H, px, py, n, frame["frame_count"])
    P = o.shape[0] * o.shape[1]
    o, d, seed = o.reshape(P, 3), d.reshape(P, 3), seed.reshape(P)
    mat, bg = np.asarray(scene["mat"], np.float64).reshape(-1, 10), np.asarray(scene["bg"], np.float64)
    colour, through = np.zeros((P, 3)), np.ones((P, 3))
    share_k, bounce = np.zeros(P), np.zeros(P)      # sum of |term| x its kappa; 1 / (N . Ra) gathered along the path
    clear, hits, strict = np.ones(P, bool), np.zeros(P, np.int64), np.ones(P, bool)
    lit, shadowed = np.zeros(P, bool), np.zeros(P, bool)
    chain = [[] for _ in range(P)]
    rays_radiance = np.zeros((md + 2, 2), np.int64)
    rays_occlusion = np.zeros(2, np.int64)
    first = {"cos": np.zeros(P), "cond": np.zeros(P), "units": np.zeros(P)}      # the primary hit's bounce: N . Ra, sum |N_i Ra_i|, direction_units
    why = {"ray": 0, "node": 0, "occlusion": 0}      # how many radiance rays, nodes and occlusion rays were not clear
    alive = np.arange(P)
    tmin, tmax, depth = np.full(P, T_MIN0), np.full(P, T_MAX0), np.zeros(P, np.int64)

    def add(k, term, kap):
        colour[k] += term
        share_k[k] += np.abs(term).sum(-1) * kap

    for level in range(md + 2):
        if not len(alive):
            break
        k = alive
        np.add.at(rays_radiance[level], (~clear[k]).astype(int), 1)
        r = _closest(scene, o[k], d[k], tmin[k], tmax[k])
        why["ray"] += int((~r["clear"]).sum())
        clear[k] &= r["clear"]
        miss = r["prim"] < 0
        add(k[miss], through[k[miss]] * bg, bounce[k[miss]])
        k, prim, t, nn = k[~miss], r["prim"][~miss], r["t"][~miss], r["n"][~miss]
        for q, p in zip(k, prim):
            chain[q].append((int(p), RADIANCE))
        hits[k] += 1
        node = closest_hit(o[k], d[k], t, nn, mat[prim], depth[k], seed[k], scene["lights"], path, ambient, md)
        why["node"] += int((~node["clear"]).sum())
        clear[k] &= node["clear"]
        bounce[k] += curved_hit_kappa(scene, prim, o[k], node)
        illum = np.ones((len(k), 3))
        oc = np.nonzero(node["occ"])[0]
        if len(oc):
            np.add.at(rays_occlusion, (~clear[k[oc]]).astype(int), 1)
            ro = _occluders(scene, node["x"][oc], node["Lm"][oc], node["eps"][oc], node["dist"][oc] - node["eps"][oc])
            # (where N . Lm < 0 the direct term is zero whatever the ray meets: its narrow decisions change nothing)
            strict[k[oc]] &= ro["clear"] & (_dot(node["N"], node["Lm"])[oc] > NLM_NEAR)
            occ_clear = ro["clear"] | (_dot(node["N"], node["Lm"])[oc] < -NLM_NEAR)
            why["occlusion"] += int((~occ_clear).sum())
            clear[k[oc]] &= occ_clear
            blocked = ro["prim"] >= 0
            illum[oc[blocked]] = occlusion_payload(mat[ro["prim"][blocked], 7:10])
            for q, p in zip(k[oc[blocked]], ro["prim"][blocked]):
                chain[q].append((int(p), OCCLUSION))
            if level == 0:
                lit[k[oc[~blocked]]], shadowed[k[oc[blocked]]] = True, True
        own, _, direct = payload(node, node["rad_dir"], np.zeros((len(k), 3)), node["Lm"], illum)
        # the direct term's own kappa, as the size of what each of its factors' rounding moves: N . Lm (counted on either side of zero, where
        # max(., 0) hides the term from one of the two computations), |Lm . n_light|, and lightDistance and Lm through (|samplingPos| + |x|) / lightDistance
        nlm, a = _dot(node["N"], node["Lm"]), np.abs(_dot(node["Lm"], node["nl"]))
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(node["occ"], 1.0 / (1.0 + node["falloff"] * node["dist"]), 0.0)
            reach = np.where(node["occ"], (np.linalg.norm(node["sp"], axis=1) + np.linalg.norm(node["x"], axis=1)) / node["dist"], 0.0)
        moved = (np.where(nlm > -NLM_NEAR, a, 0.0) + np.maximum(nlm, 0.0) + a * np.maximum(nlm, 0.0) * reach) * f
        share_k[k] += (through[k] * moved[:, None] * illum * node["kd"]).sum(-1)
        add(k, through[k] * own, bounce[k])
        rad = node["rad"]
        if level == 0:
            first["cos"][k], first["cond"][k] = _dot(node["N"], node["rad_dir"]), _cond(node["N"], node["rad_dir"])
            first["units"][k] = direction_units(node["theta"], node["frame"])
        if path:
            c = _dot(node["N"], node["rad_dir"])
            through[k[rad]] *= (node["kd"] * c[:, None])[rad]
            with np.errstate(divide="ignore"):
                bounce[k[rad]] += 1.0 / np.maximum(c[rad], 1e-300)
        else:
            through[k[rad]] *= node["kr"][rad]
        bounce[k[rad]] += kappa_h(node["theta"][rad]) - 1.0      # acos' own condition: the child starts off in a direction placed to 2^-23 kappa_h
        kr_ = k[rad]
        o[kr_], d[kr_], seed[kr_] = node["x"][rad], node["rad_dir"][rad], node["rad_seed"][rad]
        tmin[kr_], tmax[kr_], depth[kr_] = node["eps"][rad], T_MAX_CHILD, depth[kr_] + 1
        alive = kr_
    S = n * n
    sample = colour.reshape(H, W, S, 3)
    cur = mean(sample.sum(2), n)
    accum = running_average(None if prev is None else np.asarray(prev)[..., :3], cur, frame["frame_count"])
    b, slack = byte(accum)
    tot = np.abs(colour).sum(-1).reshape(H, W, S).sum(2)
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = 1.0 + np.where(tot > 0, share_k.reshape(H, W, S).sum(2) / tot, 0.0)
    return {"accum": accum, "sample": sample, "byte": b, "byte_slack": slack, "clear": clear.reshape(H, W, S).all(2), "kappa": kappa,
            "chain": [chain[q * S:(q + 1) * S] for q in range(H * W)], "hits": hits.reshape(H, W, S),
            "lit": lit.reshape(H, W, S).any(2), "shadowed": shadowed.reshape(H, W, S).any(2),
            "rays_radiance": rays_radiance, "rays_occlusion": rays_occlusion, "unclear_by": why, "clear_paths": clear,
            "first": {key: v.reshape(H, W, S) for key, v in first.items()},
            "clear_chain": (clear & strict).reshape(H, W, S).all(2)}


# ------------------------------------------------------------------------------------------------ the oracle's ray log, node by node
LOG_DTYPE = np.dtype([("parent", "<i4"), ("kind", "<i4"), ("depth", "<i4"), ("seed", "<u4"), ("o", "<f4", 3), ("d", "<f4", 3), ("tmin", "<f4"),
                      ("tmax", "<f4"), ("hit", "<i4"), ("prim", "<i4"), ("t", "<f4"), ("n", "<f4", 3), ("payload", "<f4", 3)])
# the constants tests/test_oracle_float64.py holds the oracle's intersectors to (hit point in units of 2^-23 reach, the normals' sine)
HIT_T_UNITS = {A.CYLINDER: 448.0, A.DISK: 288.0, A.RECTANGLE: 132.0, A.SPHERE: 356.0}
HIT_N_SINE = {A.CYLINDER: 2.4e-3, A.DISK: 3.0e-7, A.RECTANGLE: 2.68e-7, A.SPHERE: 2.16e-3}


def check_nodes(log, pixel, scene, frame, bounds, accum=None, image=None, prev=None):
    """log: LOG_DTYPE records of a launch in call order, `parent` indexing the same array (-1: raygen), pixel [records]: the flat pixel index
    of each (py * w + px over the launch); bounds: dict(lobe_units(c) -> units of 2^-23 kappa_h, origin_units, occ_dir_units, window_units,
    payload_units).  Every node is judged locally from the float32 values logged.  Returns dict(failures: a list of strings (empty: all
    well), figures: the largest deviation per family, counts)."""
    L = np.asarray(log)
    R = len(L)
    fails, fig = [], {}
    path, ambient, md = bool(frame["path"]), bool(frame.get("ambient", False)), frame["max_depth"]
    mat = np.asarray(scene["mat"], np.float64).reshape(-1, 10)
    types = np.asarray(scene["type"]).reshape(-1)
    o, d = L["o"].astype(np.float64), L["d"].astype(np.float64)

    def fail(what, idx):
        idx = np.atleast_1d(idx)
        if len(idx):
            fails.append("%s: %d nodes, first %s" % (what, len(idx), idx[:5].tolist()))

    # -- the hit, on clear rays
    ref = _closest(scene, o, d, L["tmin"].astype(np.float64), L["tmax"].astype(np.float64))
    cl = ref["clear"]
    rhit = ref["prim"] >= 0
    fail("hit/miss differs on a clear ray", np.nonzero(cl & (rhit != (L["hit"] != 0)))[0])
    both = cl & rhit & (L["hit"] != 0)
    fail("primitive differs on a clear ray", np.nonzero(both & (ref["prim"] != L["prim"]))[0])
    same = np.nonzero(both & (ref["prim"] == L["prim"]))[0]
    if len(same):
        Ms = np.asarray(scene["M"], np.float64).reshape(-1, 4, 4)[L["prim"][same]]
        reach = np.linalg.norm(o[same] - Ms[:, :3, 3], axis=1) + np.linalg.norm(Ms[:, :3, :3], 2, axis=(1, 2))
        dt = np.abs(L["t"][same] - ref["t"][same]) * np.linalg.norm(d[same], axis=1) / (UNIT * reach)
        dn = A.normal_sine(L["n"][same], ref["n"][same])
        ty = types[L["prim"][same]]
        fail("hit point beyond the intersector's bound", same[dt > np.vectorize(HIT_T_UNITS.get)(ty)])
        fail("normal beyond the intersector's bound", same[dn > np.vectorize(HIT_N_SINE.get)(ty)])
        fig["hit_t_units"], fig["hit_n_sine"] = float(dt.max()), float(dn.max())

    # -- the children of every radiance hit
    child = {RADIANCE: np.full(R, -1), OCCLUSION: np.full(R, -1)}
    nchild = {RADIANCE: np.zeros(R, np.int64), OCCLUSION: np.zeros(R, np.int64)}
    has_parent = np.nonzero(L["parent"] >= 0)[0]
    for kind in (RADIANCE, OCCLUSION):
        k = has_parent[L["kind"][has_parent] == kind]
        child[kind][L["parent"][k]] = k
        np.add.at(nchild[kind], L["parent"][k], 1)
    fail("an occlusion ray or a miss has children", np.nonzero(((L["kind"] == OCCLUSION) | (L["hit"] == 0)) & (nchild[RADIANCE] + nchild[OCCLUSION] > 0))[0])
    hk = np.nonzero((L["kind"] == RADIANCE) & (L["hit"] != 0))[0]
    node = closest_hit(o[hk], d[hk], L["t"][hk], L["n"][hk], mat[L["prim"][hk]], L["depth"][hk], L["seed"][hk], scene["lights"], path, ambient, md)
    ncl = node["clear"]
    fail("number of radiance children", hk[ncl & (nchild[RADIANCE][hk] != node["rad"])])
    fail("number of occlusion children", hk[ncl & (nchild[OCCLUSION][hk] != node["occ"])])
    xs = UNIT * (np.linalg.norm(o[hk], axis=1) + L["t"][hk].astype(np.float64))
    for kind, have, want_dir, scale_name in ((RADIANCE, node["rad"], node["rad_dir"], "lobe"), (OCCLUSION, node["occ"], node["Lm"], "occ")):
        sel = np.nonzero(ncl & have & (nchild[kind][hk] == 1))[0]
        if not len(sel):
            continue
        c = child[kind][hk[sel]]
        fail("child depth (kind %d)" % kind, c[L["depth"][c] != L["depth"][hk[sel]] + (1 if kind == RADIANCE else 0)])
        if kind == RADIANCE:
            fail("child seed", c[L["seed"][c] != node["rad_seed"][sel]])
        dev = np.linalg.norm(o[c] - node["x"][sel], axis=1) / xs[sel]
        fig["origin_units"] = max(fig.get("origin_units", 0.0), float(dev.max()))
        fail("child origin", c[dev > bounds["origin_units"]])
        if kind == RADIANCE:
            unit = UNIT * direction_units(node["theta"][sel], node["frame"][sel])
            dev = np.linalg.norm(d[c] - want_dir[sel], axis=1) / unit
            cls = lobe_class(node, sel, mat[L["prim"][hk[sel]]], path, ambient)
            for name in np.unique(cls):
                q = cls == name
                fig["lobe_units_" + name] = max(fig.get("lobe_units_" + name, 0.0), float(dev[q].max()))
                fail("child direction (%s lobe)" % name, c[q][dev[q] > bounds["lobe_units"][name]])
            wmax = np.full(len(sel), T_MAX_CHILD)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                unit = UNIT * (np.linalg.norm(node["sp"][sel], axis=1) + np.linalg.norm(node["x"][sel], axis=1)) / node["dist"][sel]
            dev = np.linalg.norm(d[c] - want_dir[sel], axis=1) / unit
            fig["occ_dir_units"] = max(fig.get("occ_dir_units", 0.0), float(dev.max()))
            fail("occlusion direction", c[dev > bounds["occ_dir_units"]])
            wmax = node["dist"][sel] - node["eps"][sel]
            # the window's end inherits lightDistance's placement
            dev = np.abs(L["tmax"][c] - wmax) / (unit * node["dist"][sel] + UNIT * np.abs(wmax))
            fig["occ_tmax_units"] = max(fig.get("occ_tmax_units", 0.0), float(dev.max()))
            fail("occlusion tmax", c[dev > bounds["occ_dir_units"] + bounds["window_units"]])
        dev = np.abs(L["tmin"][c] - node["eps"][sel]) / (UNIT * node["eps"][sel])
        fail("child tmin", c[dev > bounds["window_units"]])
        if kind == RADIANCE:
            fail("child tmax", c[L["tmax"][c] != np.float32(1e6)])

    # -- the payload, from the logged child directions and payloads
    okc = ncl & (nchild[RADIANCE][hk] == node["rad"]) & (nchild[OCCLUSION][hk] == node["occ"])
    cr, co = child[RADIANCE][hk], child[OCCLUSION][hk]
    rd = np.where((cr >= 0)[:, None], d[np.maximum(cr, 0)], 0.0)
    rp = np.where((cr >= 0)[:, None], L["payload"][np.maximum(cr, 0)].astype(np.float64), 0.0)
    lm = np.where((co >= 0)[:, None], d[np.maximum(co, 0)], 0.0)
    il = np.where((co >= 0)[:, None], L["payload"][np.maximum(co, 0)].astype(np.float64), 1.0)
    want, scale, _ = payload(node, rd, rp, lm, il)
    got = L["payload"][hk].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        dev = np.where(scale > 0, np.abs(got - want) / (UNIT * scale), np.where(got == want, 0.0, np.inf)).max(-1)
    dev = np.where(okc, dev, 0.0)
    fig["payload_units"] = float(dev.max(initial=0.0))
    fail("payload", hk[dev > bounds["payload_units"]])
    # an occlusion ray returns min(Le, 1) of what it hit and (1, 1, 1) otherwise; a radiance miss returns the background: exact
    ok = np.nonzero(L["kind"] == OCCLUSION)[0]
    want = np.where((L["hit"][ok] != 0)[:, None], np.minimum(mat[np.maximum(L["prim"][ok], 0), 7:10], 1.0), 1.0)
    fail("occlusion payload", ok[(L["payload"][ok] != want).any(-1)])
    ms = np.nonzero((L["kind"] == RADIANCE) & (L["hit"] == 0))[0]
    fail("miss payload", ms[(L["payload"][ms] != np.asarray(scene["bg"], np.float32)).any(-1)])

    # -- raygen: the primaries, the seed chain across the samples, the mean, the running average, the byte
    W, H, n = frame["width"], frame["height"], frame["sqrt_spp"]
    prim_k = np.nonzero(L["parent"] < 0)[0]
    pix = np.asarray(pixel)[prim_k]
    npix = int(pix.max()) + 1 if len(pix) else 0
    S = n * n
    if len(prim_k) != npix * S or (np.bincount(pix, minlength=npix) != S).any():
        fails.append("primaries per pixel: expected %d each" % S)
    else:
        w = frame.get("w", W)
        x0, y0 = frame.get("x0", 0), frame.get("y0", 0)
        upix = np.arange(npix)
        po, pd, ps = primary_rays(scene["cam"], W, H, x0 + upix % w, y0 + upix // w, n, frame["frame_count"])
        order = np.argsort(pix, kind="stable")          # call order within a pixel is kept
        k = prim_k[order].reshape(npix, S)
        fail("primary seed", k[L["seed"][k] != ps])
        fail("primary origin", k[(L["o"][k] != po.astype(np.float32)).any(-1)])
        dev = np.linalg.norm(d[k] - pd, axis=-1) / UNIT
        fig["primary_dir_units"] = float(dev.max())
        fail("primary direction", k[dev > bounds["origin_units"]])
        fail("primary window or depth", k[(L["tmin"][k] != np.float32(0.05)) | (L["tmax"][k] != np.float32(1e16)) | (L["depth"][k] != 0)
                                          | (L["kind"][k] != RADIANCE)])
        if accum is not None:
            tot = L["payload"][k].astype(np.float64).sum(1)
            cur = mean(tot, n)
            pv = None if prev is None else np.asarray(prev, np.float64).reshape(-1, 4)[:npix, :3]
            want = running_average(pv, cur, frame["frame_count"])
            got = np.asarray(accum, np.float64).reshape(-1, 4)[:npix]
            mag = np.abs(L["payload"][k].astype(np.float64)).sum(1) * float(np.float32(1.0) / np.float32(S)) + (0 if pv is None else np.abs(pv))
            with np.errstate(divide="ignore", invalid="ignore"):
                dev = np.where(mag > 0, np.abs(got[:, :3] - want) / (UNIT * mag), np.where(got[:, :3] == want, 0.0, np.inf)).max(-1)
            fig["accum_units"] = float(dev.max())
            fail("mean / running average", np.nonzero(dev > S + 4)[0])       # S - 1 additions, a product, the lerp's three operations
            fail("alpha", np.nonzero(got[:, 3] != 1.0)[0])
            if image is not None:
                b, _ = byte(got[:, :3])                                          # the byte of the float32 value itself: exact
                img = np.asarray(image).reshape(-1, 4)[:npix]
                fail("byte", np.nonzero((img[:, :3] != b).any(-1) | (img[:, 3] != 255))[0])
    return {"failures": fails, "figures": fig, "nodes": R, "hits_with_child": int((nchild[RADIANCE][hk] + nchild[OCCLUSION][hk] > 0).sum())}


def lobe_class(node, sel, mats, path, ambient):
    """the exponent class of each radiance child: 'diffuse' (c = 0: u is exact), 'glossy' (0.5 < c <= 64), 'mirror' (c > 64)"""
    spec = mats[:, 6]
    glossy = np.zeros(len(sel), bool) if path else ((spec > 0.5) if ambient else ~(spec < 0.5))
    return np.where(~glossy, "diffuse", np.where(spec <= 64.0, "glossy", "mirror"))
