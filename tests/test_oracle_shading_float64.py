"""The oracle's shading held to tests/analytic_shading_ref64.py, a float64 statement of the rules written apart from it: the lobe sampler on
seeded families and on seeds chosen so that the draws are known, every node of the oracle's ray log judged locally (its hit, its children's
kinds, depths, seeds, origins, directions and windows, its payload), whole frames of scenes built for this against whole float64 paths, and
answers worked out by hand.  tests/test_shading_float64.py holds the device to the same reference and the same constants."""
import ctypes as C

import numpy as np
import pytest

import analytic_shading_ref64 as S
import shading_scenes as SC

UNIT = S.UNIT
ALL_SCENES = ["cornell", "slide", "mirror_spheres", "plateau", "window", "checkered", "balls", "soft_mirrors"]
MODES = {"path": (True, False), "distributed": (False, False), "ambient": (False, True)}
# every specularity of the pinned material table (oracle/rtgo_oracle_scenes.c; 0 and 1 are among the first five)
EXPONENTS = [0.0, 1.0, 3.0, 30.0, 300.0, 100.0, 1000.0, 5000.0, 10000.0, 50000.0, 100000.0, 500000.0]

# ---- measured on the CPU: the oracle's largest deviation from the float64 reference over the clear cases of each family.
# The bounds are 4 x these, and the device is held to the same constants.
# lobe direction per exponent class, in units of 2^-23 direction_units (kappa_h + the frame's term); the three hemisphere families and
# every logged node of the launches below
MEASURED_LOBE_UNITS = {"diffuse": 1.08, "glossy": 1.10, "mirror": 0.55}
MEASURED_ORIGIN_UNITS = 1.26         # child origin (and the primary direction), in units of 2^-23 (|o| + t |d|)
MEASURED_OCC_DIR_UNITS = 2.81        # occlusion direction, in units of 2^-23 (|samplingPos| + |x|) / lightDistance
MEASURED_PAYLOAD_UNITS = {"path": 1.72, "distributed": 0.93, "ambient": 1.03}     # node payload, in units of 2^-23 x the terms' condition numbers
# whole-pipeline dev = |c32 - c64| / (kappa max(|c64|, 1e-3)) in units of 2^-23, per scene and mode (48 x 36, every depth and sample count below)
MEASURED_DEV_UNITS = {("room", "path"): 0.48, ("room", "distributed"): 5.47, ("room", "ambient"): 5.18,
                      ("two_lights", "path"): 0.61, ("two_lights", "distributed"): 4.93, ("two_lights", "ambient"): 3.47,
                      ("quadrics", "path"): 0.49, ("quadrics", "distributed"): 22.31, ("quadrics", "ambient"): 20.08,
                      ("detector", "path"): 0.99, ("detector", "distributed"): 2.20}
LOBE_BOUND = {k: 4 * v for k, v in MEASURED_LOBE_UNITS.items()}
DEV_BOUND = {k: 4 * v for k, v in MEASURED_DEV_UNITS.items()}
WINDOW_UNITS = 4.0                   # "a few 2^-23 relative": rayEpsilon is a product and a max, lightDistance - rayEpsilon one more subtraction
LENGTH_UNITS = 8.0                   # | |ray| - 1 |: three normalised axes, three products and two sums, half a unit each at the most


def node_bounds(mode):
    return {"lobe_units": LOBE_BOUND, "origin_units": 4 * MEASURED_ORIGIN_UNITS, "occ_dir_units": 4 * MEASURED_OCC_DIR_UNITS,
            "window_units": WINDOW_UNITS, "payload_units": 4 * MEASURED_PAYLOAD_UNITS[mode]}


def lobe_class(c):
    return "diffuse" if c == 0 else ("glossy" if c <= 64 else "mirror")


# ------------------------------------------------------------------------------------------------ the lobe
def oracle_lobes(oracle, normal, direction, c, seed):
    L = oracle.lib()
    normal, direction = oracle.f32(normal), oracle.f32(direction)
    rays, seeds = np.zeros((len(seed), 3), np.float32), np.zeros(len(seed), np.uint32)
    for k in range(len(seed)):
        s = C.c_uint32(int(seed[k]))
        L.oracle_hemisphere(oracle.fptr(normal[k]), oracle.fptr(direction[k]), float(c[k]), C.byref(s), oracle.fptr(rays[k]))
        seeds[k] = s.value
    return rays, seeds


def _sphere(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _at_angle(rng, axis, lo, hi):
    """unit vectors at an angle in [lo, hi] degrees from each axis"""
    t = np.cross(axis, _sphere(rng, len(axis)))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    a = np.radians(rng.uniform(lo, hi, len(axis)))[:, None]
    return np.cos(a) * axis + np.sin(a) * t


FAMILIES = ["direction is the normal", "grazing", "sphere"]
CASES = 4000


def family_inputs(name):
    """float32 (normal, direction, c, seed) of a family"""
    rng = np.random.RandomState(7000 + FAMILIES.index(name))
    c = np.array([EXPONENTS[k % len(EXPONENTS)] for k in range(CASES)])
    seed = rng.randint(0, 2 ** 32, CASES, dtype=np.uint64).astype(np.uint32)
    if name == "direction is the normal":
        normal = _sphere(rng, CASES)
        direction = normal
    elif name == "grazing":     # the lobe's axis within 80 to 95 degrees of the normal: the loop really rejects
        normal = _sphere(rng, CASES)
        direction = _at_angle(rng, normal, 80.0, 95.0)
    else:
        direction = _sphere(rng, CASES)
        k = CASES // 10
        axes = np.eye(3)[rng.randint(0, 3, k)] * rng.choice([-1.0, 1.0], (k, 1))
        direction[:k] = axes + 1e-3 * _sphere(rng, k) * rng.uniform(0, 1, (k, 1))
        # Y.x small and Y.y close to Y.z: the frame's X is the normalised difference of nearly equal numbers
        small, gap = 10.0 ** rng.uniform(-3, -1, k), 10.0 ** rng.uniform(-3, -1, k) * rng.choice([-1.0, 1.0], k)
        direction[k:2 * k] = np.stack([small * rng.choice([-1.0, 1.0], k), 1.0 + gap, np.ones(k)], 1) * rng.choice([-1.0, 1.0], (k, 1))
        normal = _at_angle(rng, direction / np.linalg.norm(direction, axis=1, keepdims=True), 0.0, 60.0)
    direction = direction * rng.uniform(0.5, 2.0, (CASES, 1))     # (the program normalises it)
    return normal.astype(np.float32), direction.astype(np.float32), c, seed


_families = {}


def family(oracle, name, lobes=None):
    """the family's inputs, the reference's answers and the answers under test (the oracle's unless `lobes` computes them), once"""
    key = (name, lobes)
    if key not in _families:
        normal, direction, c, seed = family_inputs(name)
        ref = S.hemisphere(normal, direction, c, seed)
        rays, seeds = (lobes or (lambda *a: oracle_lobes(oracle, *a)))(normal, direction, c, seed)
        _families[key] = (c, ref, np.asarray(rays, np.float64), seeds)
    return _families[key]


def family_figures(f):
    """per family: the unclear share, the share with more than one draw, seeds that differ on clear cases, the largest direction deviation per
    exponent class and the largest | |ray| - 1 |, both in units of 2^-23 (x direction_units for the former)"""
    c, ref, rays, seeds = f
    clear = (ref["margin"] >= S.HEMI_CLEAR) & ~ref["degenerate"]      # (a loop that runs to its bound is as determinate as one that ends)
    dev = np.linalg.norm(rays - ref["ray"], axis=1) / (UNIT * S.direction_units(ref["theta"], ref["frame"]))
    cls = np.array([lobe_class(x) for x in c])
    return {"unclear": 1 - clear.mean(), "rejecting": (ref["draws"] > 1).mean(), "exhausted": int(ref["exhausted"].sum()),
            "seed_differs": np.nonzero(clear & (seeds != ref["seed"]))[0],
            "dev": {k: float(dev[clear & (cls == k)].max()) for k in LOBE_BOUND},
            "length": float((np.abs(np.linalg.norm(rays[clear], axis=1) - 1.0) / UNIT).max())}


def check_family(name, fig):
    print(name, fig)
    assert fig["unclear"] <= 0.02
    assert len(fig["seed_differs"]) == 0, fig["seed_differs"][:10]       # the same seed afterwards: the same number of draws
    for k, v in fig["dev"].items():
        assert v <= LOBE_BOUND[k], (k, v)
    assert fig["length"] <= LENGTH_UNITS
    if name == "grazing":
        assert fig["rejecting"] >= 0.20


@pytest.mark.parametrize("name", FAMILIES)
def test_lobe_family(oracle, name):
    check_family(name, family_figures(family(oracle, name)))


def seed_with(first=None, second=None):
    """a seed whose first draw is first / 2^24, or whose second draw is second / 2^24 (the other one is whatever follows: returned too).
    The LCG's step is a bijection of 2^32 and a draw is the state's low 24 bits, so a state with the wanted low bits is stepped back."""
    if first is not None:
        state1 = np.uint32((0x5A << 24) | first)
        seed = S.lcg_back(state1)
    else:
        state2 = np.uint32((0xC3 << 24) | second)
        seed = S.lcg_back(S.lcg_back(state2))
    s, k1 = S.lcg(seed)
    _, k2 = S.lcg(s)
    return seed, int(k1) / 2.0 ** 24, int(k2) / 2.0 ** 24


def lobe_known_answers():
    """(what, normal, direction, c, seed, the expected direction in float64 worked out here, expected seed steps)"""
    rng = np.random.RandomState(99)
    out = []
    for c in (0.0, 3.0, 30.0, 1000.0):
        Y = _sphere(rng, 1)[0].astype(np.float32).astype(np.float64)
        Yn = Y / np.linalg.norm(Y)
        X = np.array([Yn[1] - Yn[2], -Yn[0], Yn[0]])
        X /= np.linalg.norm(X)
        Z = np.cross(Yn, X)
        seed, r1, r2 = seed_with(second=0)                         # r2 = 0: theta = 0, the ray is Y itself
        assert r2 == 0.0
        out.append(("r2 = 0, c = %g" % c, Y, Y, c, seed, Yn, 2))
        seed, r1, r2 = seed_with(first=0)                          # r1 = 0: phi = 0, sin theta X + cos theta Y
        th = np.arccos((1.0 - r2) ** (1.0 / (c + 1.0)))
        out.append(("r1 = 0, c = %g" % c, Y, Y, c, seed, np.sin(th) * X + np.cos(th) * Yn, 2))
        seed, r1, r2 = seed_with(first=1 << 22)                    # r1 = 1/4: phi = pi_f / 2, cos theta Y - sin theta Z up to cos(pi_f / 2)
        assert r1 == 0.25
        th = np.arccos((1.0 - r2) ** (1.0 / (c + 1.0)))
        want = np.cos(th) * Yn - np.sin(th) * Z
        assert abs(np.cos(S.PI_F / 2)) < 5e-8
        out.append(("r1 = 1/4, c = %g" % c, Y, Y, c, seed, want + np.sin(th) * np.cos(S.PI_F / 2) * X, 2))
    return out


def check_lobe_known(what, normal, direction, c, seed, want, steps, ray, seed_after):
    """the reference gives the hand-worked direction (to float64 rounding), and (ray, seed_after) -- the code under test -- agrees with the
    reference within the family bounds"""
    ref = S.hemisphere(normal[None], direction[None], c, np.array([seed], np.uint32))
    assert np.abs(ref["ray"][0] - want).max() <= 1e-12, what
    s = np.uint32(seed)
    for _ in range(steps):
        s, _k = S.lcg(s)
    assert int(ref["seed"][0]) == int(s) and int(seed_after) == int(s), what
    dev = np.linalg.norm(np.asarray(ray, np.float64) - ref["ray"][0]) / (UNIT * S.direction_units(ref["theta"][0], ref["frame"][0]))
    assert dev <= LOBE_BOUND[lobe_class(c)], (what, dev)


def test_lobe_known_answers(oracle):
    for what, normal, direction, c, seed, want, steps in lobe_known_answers():
        ray, after = oracle_lobes(oracle, normal[None], direction[None], [c], [seed])
        check_lobe_known(what, normal, direction, c, seed, want, steps, ray[0], after[0])


def test_lobe_below_the_horizon_stops_at_its_bound(oracle):
    """normal = -direction, c = 0: normal . ray = -cos theta <= 0 for every draw (zero needs r2 = 1, which rnd never gives), so the loop runs
    to its 1024th draw and the seed has moved by exactly 2048 steps"""
    Y = np.array([0.3, -0.5, 0.8], np.float32)
    seed, _, r2 = seed_with(second=0)
    ref = S.hemisphere(-Y[None], Y[None], 0.0, np.array([seed], np.uint32))
    s = np.uint32(seed)
    for _ in range(2048):
        s, _k = S.lcg(s)
    assert ref["draws"][0] == 1024 and ref["exhausted"][0] and int(ref["seed"][0]) == int(s)
    ray, after = oracle_lobes(oracle, -Y[None], Y[None], [0.0], [seed])
    assert int(after[0]) == int(s)
    dev = np.linalg.norm(ray[0].astype(np.float64) - ref["ray"][0]) / (UNIT * S.direction_units(ref["theta"][0], ref["frame"][0]))
    assert dev <= LOBE_BOUND["diffuse"]


DEGENERATE_SEED = 20261018


def test_degenerate_frame(oracle):
    """direction = (0, a, a): Y.y - Y.z = 0 and Y.x = 0, X = 0 / 0.  IEEE arithmetic makes the ray NaN, NaN < 0 is false, and the loop ends
    after one draw of r1 and r2: two steps of the seed.  Pinned for the oracle; the reference flags the frame instead of returning a number."""
    for a in (1.0, 0.5, -2.0):
        d = np.array([0.0, a, a], np.float32)
        ref = S.hemisphere(d[None], d[None], 0.0, np.array([DEGENERATE_SEED], np.uint32))
        assert ref["degenerate"][0] and not ref["clear"][0]
        ray, after = oracle_lobes(oracle, d[None], d[None], [0.0], [DEGENERATE_SEED])
        s, _k = S.lcg(np.uint32(DEGENERATE_SEED))
        s, _k = S.lcg(s)
        assert np.isnan(ray[0]).all() and int(after[0]) == int(s)


def tilted_plane(angle_deg=45.0):
    """one rectangle tilted about x under a bright background, seen head on: at exactly 45 degrees the float32 cosine and sine are equal"""
    a = np.float32(np.radians(angle_deg))
    c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
    if angle_deg == 45.0:
        c = s = np.float32(np.sqrt(0.5))
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] = np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float32) @ np.diag([6, 1, 6]).astype(np.float32)
    mat = np.array([[0.8, 0.6, 0.4, 0, 0, 0, 0, 0, 0, 0]], np.float32)
    cam = SC.camera((0, 0.5, 5.0), (0, 0, 0), (0, 1, 0), 40.0, 16 / 12)
    return {"type": np.array([SC.RECTANGLE], np.int32), "M": M.reshape(1, 16), "mat": mat, "lights": np.zeros((1, 16), np.float32), "cam": cam,
            "bg": np.array([0.5, 0.75, 1.0], np.float32)}


def test_degenerate_plane_renders_nan(oracle):
    """a plane tilted by exactly 45 degrees about x has N = (0, a, a): in path mode every bounce off it is the NaN ray, which meets nothing,
    and kd (N . NaN) background is NaN: the accumulation buffer holds NaN and the byte is clamp's answer to it, fmaxf(0, fminf(NaN, 1)) = 1,
    so 255.  (DESIGN.md 4 says what that means for a scene.)"""
    t = tilted_plane()
    N = (t["M"].reshape(4, 4)[:3, :3].astype(np.float64) @ [0, 1, 0])
    assert N[0] == 0 and N[1] == N[2]
    W, H = 16, 12
    acc, img, _ = oracle.render(scene_of(oracle, t), oracle.frame(W, H, 1, 0, path=True, mode=1, max_depth=1))
    ref = S.render(t, frame_of(W, H, 1, 1, 0, "path"))
    hit = (ref["hits"] > 0).all(-1)
    assert hit.mean() > 0.5
    assert np.isnan(acc[hit][:, :3]).all() and (acc[..., 3] == 1.0).all()
    assert (img[hit][:, :3] == 255).all()
    assert (acc[~hit][:, :3] == t["bg"]).all()


# ------------------------------------------------------------------------------------------------ helpers over scenes and frames
def scene_of(oracle, t):
    return oracle.scene_from_tables(t["type"], t["M"], t["mat"], t["lights"], t["cam"], t["bg"])


def frame_of(W, H, n, md, fc, mode):
    path, amb = MODES[mode]
    return {"width": W, "height": H, "sqrt_spp": n, "max_depth": md, "frame_count": fc, "path": path, "ambient": amb}


def oracle_frames(oracle, sc, W, H, n, md, mode, upto):
    """the oracle's accumulation buffer after frames 0 .. upto - 1 (None for upto = 0)"""
    path, amb = MODES[mode]
    acc = None
    for fc in range(upto):
        acc, _, _ = oracle.render(sc, oracle.frame(W, H, n, fc, path=path, ambient=amb, mode=1, max_depth=md), acc)
    return acc


# ------------------------------------------------------------------------------------------------ logged nodes
# (sqrt_spp, frame_count, max_depth): every value the issue names, each with each of the others at least once
NODE_LAUNCHES = [(1, 0, 0), (2, 2, 1), (1, 2, 3), (2, 0, 5), (1, 0, 5), (2, 2, 0), (1, 2, 1), (2, 0, 3)]


FULL_W, FULL_H, WIN_W, WIN_H = 128, 96, 32, 24
_windows = {}


def busiest_window(oracle, name):
    """the 32 x 24 window of the scene's 128 x 96 frame in which most primary rays hit something (several scenes are mostly sky), by the
    reference's own primaries: (width, height, (x0, y0, w, h))"""
    if name not in _windows:
        for scale in (1, 2):          # a scene too thin for that is looked at twice as closely
            fw, fh = FULL_W * scale, FULL_H * scale
            t = oracle.scene_tables(oracle.scene(name, fw, fh))
            py, px = [a.reshape(-1) for a in np.mgrid[0:fh, 0:fw]]
            o, d, _ = S.primary_rays(t["cam"], fw, fh, px, py, 1, 0)
            hit = (S._closest_raw(t, o[:, 0], d[:, 0], S.T_MIN0, S.T_MAX0)["prim"] >= 0).reshape(fh, fw)
            c = np.pad(hit.astype(np.int64).cumsum(0).cumsum(1), ((1, 0), (1, 0)))
            best = max(((c[y + WIN_H, x + WIN_W] - c[y, x + WIN_W] - c[y + WIN_H, x] + c[y, x], -y, -x)
                        for y in range(0, fh - WIN_H + 1, 4) for x in range(0, fw - WIN_W + 1, 4)))
            _windows[name] = (fw, fh, (-best[2], -best[1], WIN_W, WIN_H))
            if best[0] >= 0.9 * WIN_W * WIN_H:
                break
    return _windows[name]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ALL_SCENES)
def test_logged_nodes(oracle, name, mode):
    W, H, win = busiest_window(oracle, name)
    sc = oracle.scene(name, W, H)
    t = oracle.scene_tables(sc)
    path, amb = MODES[mode]
    nodes = with_child = 0
    worst = {}
    for n, fc, md in NODE_LAUNCHES:
        prev = None
        for f in range(fc):
            prev, _, _ = oracle.render(sc, oracle.frame(W, H, n, f, path=path, ambient=amb, window=win, mode=1, max_depth=md), prev)
        log, pixel, acc, img = oracle.log_launch(sc, oracle.frame(W, H, n, fc, path=path, ambient=amb, window=win, mode=1, max_depth=md), prev)
        fr = dict(frame_of(W, H, n, md, fc, mode), x0=win[0], y0=win[1], w=win[2])
        res = S.check_nodes(log, pixel, t, fr, node_bounds(mode), acc, img, prev)
        assert not res["failures"], (name, mode, (n, fc, md), res["failures"])
        for k, v in res["figures"].items():
            worst[k] = max(worst.get(k, 0.0), v)
        nodes += res["nodes"]
        with_child += res["hits_with_child"]
    print(name, mode, win, {k: float("%.3g" % v) for k, v in worst.items()}, "hits with a child: %.3f of %d nodes" % (with_child / nodes, nodes))
    assert with_child >= 0.30 * nodes


def test_log_reproduces_the_render(oracle):
    """oracle_log_pixel writes what oracle_render writes, and the hook changes nothing: same accumulation buffer, same bytes, and as many
    records as the render counted rays"""
    W, H = 32, 24
    sc = oracle.scene("cornell", W, H)
    for mode, (path, amb) in MODES.items():
        fr = oracle.frame(W, H, 2, 0, path=path, ambient=amb, mode=1, max_depth=5)
        acc, img, ctr = oracle.render(sc, fr)
        log, pixel, lacc, limg = oracle.log_launch(sc, fr)
        assert acc.tobytes() == lacc.tobytes() and img.tobytes() == limg.tobytes()
        assert len(log) == ctr["rays_total"] and int((log["kind"] == S.OCCLUSION).sum()) == ctr["rays_occlusion"]
        assert int((log["hit"] != 0).sum()) == ctr["hits"]


def test_seed_flow_between_depths(oracle):
    """max_depth 1 against max_depth 2: everything traced at depth <= 1 is the same ray with the same seed; only the child's child is new"""
    W, H = 16, 12
    t = SC.room(W / H)
    sc = scene_of(oracle, t)
    for mode, (path, amb) in MODES.items():
        logs = []
        for md in (1, 2):
            log, pixel, _, _ = oracle.log_launch(sc, oracle.frame(W, H, 2, 0, path=path, ambient=amb, mode=1, max_depth=md))
            keep = log["depth"] <= 1          # (an occlusion ray carries the depth of the hit that traced it)
            logs.append((log[keep], pixel[keep]))
        a, b = logs
        # a depth-1 hit traces its occlusion ray at either max_depth, so the depth <= 1 sub-logs align one to one
        assert len(a[0]) == len(b[0]) and (a[1] == b[1]).all()
        for field in ("kind", "depth", "seed", "o", "d", "tmin", "tmax", "hit", "prim", "t", "n"):
            assert a[0][field].tobytes() == b[0][field].tobytes(), (mode, field)
        assert (logs[1][0]["payload"] != logs[0][0]["payload"]).any()      # ... and the child's child shows


# ------------------------------------------------------------------------------------------------ whole frames
W48, H36 = 48, 36
UNCLEAR_CAP = {"room": 0.05, "two_lights": 0.05, "quadrics": 0.25}
DEPTHS = {"room": (1, 3, 5), "two_lights": (1, 3, 5), "quadrics": (1, 2)}
_reference = {}


def reference(name, mode, md, n, frames=1):
    """the float64 frames of a scene, accumulated over `frames` progressive frames; computed once and shared"""
    key = (name, mode, md, n, frames)
    if key not in _reference:
        t = SC.SCENES[name](W48 / H36)
        prev, out = None, []
        for fc in range(frames):
            r = S.render(t, frame_of(W48, H36, n, md, fc, mode), prev)
            if out:      # a pixel is as clear, and as ill-conditioned, as the worst of its frames
                r["clear"] = r["clear"] & out[-1]["clear"]
                r["clear_chain"] = r["clear_chain"] & out[-1]["clear_chain"]
                r["kappa"] = np.maximum(r["kappa"], out[-1]["kappa"])
                r["hits"] = np.maximum(r["hits"], out[-1]["hits"])          # (a pixel misses when it misses in every frame)
                r["rays_radiance"] = r["rays_radiance"] + out[-1]["rays_radiance"]
                r["rays_occlusion"] = r["rays_occlusion"] + out[-1]["rays_occlusion"]
            r["paths_unclear"] = int((~r["clear_paths"]).sum()) + (out[-1]["paths_unclear"] if out else 0)
            out.append(r)
            prev = r["accum"]
        _reference[key] = (t, out[-1])
    return _reference[key]


def reference_frame(name, mode, md, n, fc, prev):
    """frame `fc` alone, and its running average over the buffer `prev` [h, w, 3 or 4] that the code under test held before it: each frame is
    then judged on its own clear pixels through the recurrence prev -> cur, whatever the earlier frames' pixels were"""
    key = (name, mode, md, n, "frame", fc)
    if key not in _reference:
        t = SC.SCENES[name](W48 / H36)
        r = S.render(t, frame_of(W48, H36, n, md, fc, mode))
        r["paths_unclear"] = int((~r["clear_paths"]).sum())
        _reference[key] = (t, r)
    t, r = _reference[key]
    r = dict(r)
    if fc > 0:
        r["accum"] = S.running_average(np.asarray(prev, np.float64)[..., :3], S.mean(r["sample"].sum(2), n), fc)
        r["byte"], r["byte_slack"] = S.byte(r["accum"])
        r["prev_is_background"] = (np.asarray(prev)[..., :3] == t["bg"]).all(-1)
    return t, r


def check_frame(name, mode, md, n, ref, acc, img, rays_radiance=None, rays_occlusion=None, rays_total=None, chains=None):
    """one frame of the code under test (acc [h, w, 4] float32, img [h, w, 4] uint8, its ray counts where it has them) against the
    reference's: the caps and floors of the reference itself, then deviation, bytes, background, alpha and ray counts.  Returns the figures."""
    t, r = ref
    clear = r["clear"]
    hit = (r["hits"] > 0).any(-1)
    unclear = (~clear & hit).sum() / max(hit.sum(), 1)
    two = (clear & (r["hits"] >= 2).all(-1)).mean()
    fig = {"unclear": float(unclear), "two_hits": float(two), "lit": float(r["lit"].mean()), "shadowed": float(r["shadowed"].mean())}
    assert unclear <= UNCLEAR_CAP[name], fig
    assert two >= 0.40, fig
    if mode != "path":
        assert fig["shadowed"] >= 0.10 and fig["lit"] >= 0.30, fig
    c64, c32 = r["accum"], np.asarray(acc, np.float64)[..., :3]
    dev = (np.abs(c32 - c64) / (r["kappa"][..., None] * np.maximum(np.abs(c64), 1e-3))).max(-1) / UNIT
    fig["dev"] = float(dev[clear].max())
    print(name, mode, "max_depth", md, "sqrt_spp", n, fig)
    assert fig["dev"] <= DEV_BOUND[(name, mode)], fig
    b = np.asarray(img)[..., :3].astype(np.int64)
    exact = r["byte_slack"] >= 1e-3
    assert (b[clear] == r["byte"][clear])[exact[clear]].all() and (np.abs(b[clear] - r["byte"][clear]) <= 1).all()
    miss = clear & ~hit & r.get("prev_is_background", True)      # (a later frame: where the buffer held the background before it)
    assert (np.asarray(acc)[miss][:, :3] == t["bg"]).all()
    assert (np.asarray(acc)[..., 3] == 1.0).all() and (np.asarray(img)[..., 3] == 255).all()
    # a ray counted clear is traced by both; one on a path that was no longer clear may or may not be, and such a path may run on where the
    # reference's ended: one more ray per depth and kind at the most
    spare = r["paths_unclear"]
    if rays_radiance is not None:
        for depth in range(md + 1):
            lo = int(r["rays_radiance"][depth, 0])
            assert lo <= rays_radiance[depth] <= lo + spare, (depth, rays_radiance, r["rays_radiance"].tolist())
    if rays_occlusion is not None:
        lo = int(r["rays_occlusion"][0])
        assert lo <= rays_occlusion <= lo + spare * (md + 1), (rays_occlusion, r["rays_occlusion"].tolist())
    if rays_total is not None:
        lo = int(r["rays_radiance"][:, 0].sum() + r["rays_occlusion"][0])
        assert lo <= rays_total <= lo + 2 * spare * (md + 1), (rays_total, lo, spare)
    if chains is not None:
        bad = [q for q in np.nonzero(r["clear_chain"].reshape(-1))[0] if chains[q] != r["chain"][q]]
        assert not bad, (bad[:5], chains[bad[0]], r["chain"][bad[0]])
    return fig


def chains_of(log, pixel, n_pixels, samples):
    """the (primitive, kind) of every hit in call order, per pixel and sample, from a ray log"""
    out = [[[] for _ in range(samples)] for _ in range(n_pixels)]
    sample = -1
    last = -1
    for k in range(len(log)):
        if pixel[k] != last:
            last, sample = pixel[k], -1
        if log["parent"][k] < 0:
            sample += 1
        if log["hit"][k]:
            out[pixel[k]][sample].append((int(log["prim"][k]), int(log["kind"][k])))
    return out


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(SC.SCENES))
def test_whole_frames(oracle, name, mode, n):
    path, amb = MODES[mode]
    for md in DEPTHS[name]:
        ref = reference(name, mode, md, n)
        sc = scene_of(oracle, ref[0])
        fr = oracle.frame(W48, H36, n, 0, path=path, ambient=amb, mode=1, max_depth=md)
        acc, img, ctr = oracle.render(sc, fr)
        chains = None
        if md == DEPTHS[name][-1]:
            log, pixel, _, _ = oracle.log_launch(sc, fr)
            chains = chains_of(log, pixel, W48 * H36, n * n)
        check_frame(name, mode, md, n, ref, acc, img, ctr["rays_radiance"], ctr["rays_occlusion"], ctr["rays_total"], chains)


# ------------------------------------------------------------------------------------------------ answers worked out here
def wall_scene(material, bg=(1.0, 1.0, 1.0), lights=None):
    """a single wall z = 0 facing +z, 20 units wide, seen head on from (0, 0, 6)"""
    M = SC.flat((0, 0, 0), (0, 0, 1), 20.0)
    return {"type": np.array([SC.RECTANGLE], np.int32), "M": M.reshape(1, 16), "mat": np.array([material], np.float32),
            "lights": np.zeros((1, 16), np.float32) if lights is None else lights, "cam": SC.camera((0, 0, 6.0), (0, 0, 0), (0, 1, 0), 45.0, 16 / 12),
            "bg": np.array(bg, np.float32)}


def stream(W, px, py, frame_count, count):
    """the first `count` draws of a pixel's seed, from the integers"""
    s = S.tea16(W * py + px, frame_count)
    out = []
    for _ in range(count):
        s, k = S.lcg(s)
        out.append(int(k) / 2.0 ** 24)
    return out


def test_known_path_single_wall(oracle):
    """path mode, max_depth 1, a white background: each sample is kd (N . Ra) with N . Ra = cos theta = 1 - r2 (c = 0: u = 1 - r2 exactly, and
    direction = normal accepts the first draw).  The sample's draws are the jitter's two, then r1, r2; the next sample goes on from the seed
    after the jitter alone (by value), so sample k reads draws 2k + 2 and 2k + 3 ... of which r2 is the second"""
    W, H, n = 16, 12, 2
    kd = np.array([0.8, 0.5, 0.25], np.float32)
    t = wall_scene([*kd, 0, 0, 0, 0, 0, 0, 0])
    acc, img, ctr = oracle.render(scene_of(oracle, t), oracle.frame(W, H, n, 0, path=True, mode=1, max_depth=1))
    ref = S.render(t, frame_of(W, H, n, 1, 0, "path"))
    assert ctr["rays_radiance"][:3] == [W * H * n * n, W * H * n * n, 0]
    for py, px in [(0, 0), (5, 7), (11, 15)]:
        d = stream(W, px, py, 0, 2 * n * n + 2)
        # sample k: jitter = draws 2k, 2k + 1; its path then reads 2k + 2 (r1) and 2k + 3 (r2) -- the next sample's jitter, read twice
        want = sum(kd.astype(np.float64) * (1.0 - d[2 * k + 3]) for k in range(n * n)) * float(np.float32(1.0) / np.float32(n * n))
        assert np.abs(ref["accum"][py, px] - want).max() <= 1e-12
        assert np.abs(acc[py, px, :3] - want).max() <= 8 * UNIT * kd.max()


def test_known_emitter_thresholds(oracle):
    """Le = (0, 5, 5): not an emitter in path mode (Le.x > 0.01 fails: it is shaded as a surface), white in distributed mode"""
    W, H = 16, 12
    t = wall_scene([0.5, 0.5, 0.5, 0, 0, 0, 0, 0.0, 5.0, 5.0])
    sc = scene_of(oracle, t)
    acc, _, _ = oracle.render(sc, oracle.frame(W, H, 1, 0, path=True, mode=1, max_depth=1))
    for py, px in [(3, 4), (8, 11)]:
        d = stream(W, px, py, 0, 4)
        assert np.abs(acc[py, px, :3] - 0.5 * (1.0 - d[3])).max() <= 8 * UNIT
    acc, _, _ = oracle.render(sc, oracle.frame(W, H, 1, 0, path=False, mode=1, max_depth=1))
    assert (acc[..., :3] == 1.0).all()
    ref = S.render(t, frame_of(W, H, 1, 1, 0, "distributed"))
    assert (ref["accum"] == 1.0).all()


def one_light():
    return SC.light_record(SC.flat((1.0, 2.0, 4.0), (0.2, -0.3, -1.0), 1.5, spin=0.4), 0.25)[None]


@pytest.mark.parametrize("mode", ["distributed", "ambient"])
def test_known_direct_term_alone(oracle, mode):
    """max_depth 0 in distributed mode with one light: the direct term alone, by hand -- and under ambient light no 0.1 kd, as
    depth == max_depth.  x is where the primary ray meets z = 0; the draws after the jitter are the light's index (n_lights - 1 = 0: light 0),
    r_a, r_b"""
    W, H = 16, 12
    kd = np.array([0.8, 0.5, 0.25], np.float32).astype(np.float64)
    t = wall_scene([0.8, 0.5, 0.25, 0.3, 0.3, 0.3, 1.0, 0, 0, 0], lights=one_light())
    path, amb = MODES[mode]
    acc, _, ctr = oracle.render(scene_of(oracle, t), oracle.frame(W, H, 1, 0, path=path, ambient=amb, mode=1, max_depth=0))
    assert ctr["rays_radiance"][:2] == [W * H, 0] and ctr["rays_occlusion"] == W * H
    ref = S.render(t, frame_of(W, H, 1, 0, 0, mode))
    L = t["lights"][0].astype(np.float64)
    cam = t["cam"].astype(np.float64)
    for py, px in [(2, 3), (6, 8), (10, 14)]:
        d = stream(W, px, py, 0, 5)
        dx, dy = 2 * (px + d[0]) / W - 1, 2 * (py + d[1]) / H - 1
        ray = dx * cam[3:6] + dy * cam[6:9] + cam[9:12]
        x = cam[0:3] - ray * cam[2] / ray[2]                       # z = 0
        sp = L[0:3] + d[3] * L[3:6] + d[4] * L[6:9]
        dist = np.linalg.norm(sp - x)
        Lm = (sp - x) / dist
        want = abs(Lm @ L[9:12]) * max(Lm[2], 0.0) * kd / (1.0 + L[15] * dist)      # N = (0, 0, 1); nothing occludes
        assert np.abs(ref["accum"][py, px] - want).max() <= 1e-9
        assert np.abs(acc[py, px, :3] - want).max() <= 4 * MEASURED_DEV_UNITS[("room", mode)] * UNIT * ref["kappa"][py, px] * np.maximum(want, 1e-3).max()


def test_known_occlusion_window_end(oracle):
    """the occlusion ray covers [rayEpsilon, lightDistance - rayEpsilon]: a blocker inside the last rayEpsilon before the sampled point does not
    shadow, one a few rayEpsilon before it does, and what it passes on is min(Le, 1).  The camera is 10 above the floor, so rayEpsilon =
    1e-6 t^2 is at least 1e-4; the light hangs 2 above the floor, a blocker d below the light moves the hit d lightDistance / 2 before the
    sample: d = 2.5e-5 stays inside rayEpsilon for every lightDistance below 8, d = 2e-3 is 10 rayEpsilon out at the least"""
    W, H = 16, 12
    floor = (SC.RECTANGLE, SC.flat((0, 0, 0), (0, 1, 0), 8.0), SC.MATTE)
    cam = SC.camera((0, 10.0, 0.01), (0, 0, 0), (0, 0, -1), 30.0, W / H)
    light = SC.light_record(SC.flat((0.5, 2.0, -0.5), (0, -1, 0), 1.0), 0.3)[None]
    Le = (0.5, 2.0, 0.25)

    def frame(gap):
        prims = [floor] + ([] if gap is None else [(SC.RECTANGLE, SC.flat((0, 2.0 - gap, 0), (0, -1, 0), 30.0), (0, 0, 0, 0, 0, 0, 1.0) + Le)])
        t = SC._tables(prims, light, cam, (0, 0, 0))
        acc, _, _ = oracle.render(scene_of(oracle, t), oracle.frame(W, H, 1, 0, path=False, mode=1, max_depth=0))
        return acc[..., :3], S.render(t, frame_of(W, H, 1, 0, 0, "distributed"))["accum"]

    open32, open64 = frame(None)
    near32, near64 = frame(2.5e-5)
    far32, far64 = frame(2e-3)
    assert open64.min() > 1e-3
    assert (near64 == open64).all() and near32.tobytes() == open32.tobytes()
    assert np.abs(far64 / open64 - np.minimum(Le, 1.0)).max() <= 1e-12
    assert np.abs(far32 / open32 - np.minimum(Le, 1.0)).max() <= 4 * UNIT


# ------------------------------------------------------------------------------------------------ the detector
# (pose, the target's specularity; None: path mode).  Distributed mode: a diffuse lobe about N (0), the lobe about Rr at the exponents 1, 30
# and 300 -- the camera is oblique there, so Rr is not N
DETECTOR_CASES = [("axis", None), ("rotated", None), ("tilted", None), ("rotated", 0), ("rotated", 1), ("rotated", 30), ("rotated", 300)]
DETECTOR_FRAMES = (0, 1, 2, 3)
_detector = {}


def detector_mode(spec):
    return "path" if spec is None else "distributed"


def detector_reference(pose, spec, fc):
    """the detector scene, its target's weight and the reference's frame `fc` rendered over a zeroed buffer (so the buffer holds the frame
    itself times float32(1 / (fc + 1))); computed once"""
    key = (pose, spec, fc)
    if key not in _detector:
        t, weight = SC.detector(pose, spec, W48 / H36)
        _detector[key] = (t, weight, S.render(t, frame_of(W48, H36, 1, 1, fc, detector_mode(spec)), np.zeros((H36, W48, 3))))
    return _detector[key]


def second_hit(r):
    """the primitive each pixel's bounce ray met (-1: none), of a one-sample frame"""
    out = []
    for c in r["chain"]:
        hits = [p for p, kind in c[0] if kind == S.RADIANCE]
        out.append(hits[1] if len(hits) > 1 else -1)
    return np.array(out).reshape(r["clear"].shape)


def check_detector(pose, spec, fc, acc):
    """acc: the buffer of the code under test after frame `fc` alone on a zeroed buffer.  Every pixel is weight x level x colour of the patch
    its bounce ray met (path mode: kd (N . Ra) Le_patch; distributed: kr x the patch's direct term, whose kd is the colour): the patch read off
    the channel ratios must be the reference's on every clear pixel, at most 2 % of the target's pixels may be unclear, the level is held to
    the reference's within the scene's bound, and in path mode N . Ra itself within the node bounds (the payload's times the dot product's
    condition number, plus the lobe's).  Returns dev in units."""
    t, weight, r = detector_reference(pose, spec, fc)
    colour = SC.patch_colours()
    mode = detector_mode(spec)
    target = np.array([c[0][0][0] if c[0] else -1 for c in r["chain"]]).reshape(H36, W48) == 0
    assert target.mean() >= 0.95, "the target no longer fills the frame"
    assert (~r["clear"] & target).sum() <= 0.02 * target.sum()
    patch = second_hit(r) - 1
    ok = r["clear"] & target & (patch >= 0)
    assert ok.mean() >= 0.90
    seen = np.asarray(acc, np.float64)[..., :3] / weight.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = seen / np.linalg.norm(seen, axis=-1, keepdims=True)
    named = np.argmax(np.nan_to_num(unit) @ (colour / np.linalg.norm(colour, axis=1, keepdims=True)).T, axis=-1)
    wrong = np.nonzero(ok & (named != patch))
    assert len(wrong[0]) == 0, (pose, spec, fc, list(zip(*wrong))[:5])
    assert len(np.unique(patch[ok])) >= 30          # the bounce rays really spread over the patches
    ratio = float(np.float32(1.0) / np.float32(fc + 1))
    if mode == "path":
        cos32 = (seen / colour[np.maximum(patch, 0)]).mean(-1) / ratio
        f = r["first"]
        tol = UNIT * (4 * MEASURED_PAYLOAD_UNITS["path"] * f["cond"][..., 0] + LOBE_BOUND["diffuse"] * f["units"][..., 0] + 2.0)   # (+ the lerp's and the mean's roundings)
        worst = (np.abs(cos32 - f["cos"][..., 0]) / tol)[ok].max()
        print("detector", pose, "frame", fc, "cosine: largest deviation %.3f of its bound" % worst)
        assert worst <= 1.0
    c64 = r["accum"]
    dev = (np.abs(np.asarray(acc, np.float64)[..., :3] - c64) / (r["kappa"][..., None] * np.maximum(np.abs(c64), 1e-3 * ratio))).max(-1) / UNIT
    print("detector", pose, spec, "frame", fc, "largest dev %.2f units, %d patches" % (dev[ok].max(), len(np.unique(patch[ok]))))
    assert dev[ok].max() <= DEV_BOUND[("detector", mode)]
    return float(dev[ok].max())


def detector_average(pose, spec, frames):
    """the reference's running average over frames 0 .. frames - 1, its kappa and the pixels clear in every one"""
    acc, ok, kappa = None, True, 0.0
    for fc in range(frames):
        t, weight, r = detector_reference(pose, spec, fc)
        cur = r["accum"] / float(np.float32(1.0) / np.float32(fc + 1)) if fc else r["accum"]
        acc = S.running_average(acc, cur, fc)
        ok = ok & r["clear"] & (second_hit(r) >= 1)
        kappa = np.maximum(kappa, r["kappa"])
    return acc, kappa, ok


@pytest.mark.parametrize("fc", DETECTOR_FRAMES)
@pytest.mark.parametrize("pose,spec", DETECTOR_CASES, ids=lambda v: str(v))
def test_detector(oracle, pose, spec, fc):
    """the oracle through the detector: where MEASURED_DEV_UNITS["detector", ...] come from, and the proof that the scene reads what it
    says it reads (tests/test_shading_float64.py holds the device to it)"""
    t, weight, r = detector_reference(pose, spec, fc)
    path, amb = MODES[detector_mode(spec)]
    acc, _, _ = oracle.render(scene_of(oracle, t), oracle.frame(W48, H36, 1, fc, path=path, ambient=amb, mode=1, max_depth=1),
                              np.zeros((H36, W48, 4), np.float32))
    check_detector(pose, spec, fc, acc)


def test_log_layout_is_the_oracle_s(oracle):
    assert S.LOG_DTYPE == oracle.RAY_RECORD_DTYPE
