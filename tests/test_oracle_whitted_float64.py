"""The oracle of the triangle path's shading (oracle/rtgo_oracle_whitted.c) against tests/whitted_ref64.py, a float64 statement of
cuda/whitted.cu and cuda/LocalGeometry.h that shares no text with it: the closest-hit program alone on a seeded sweep
(oracle_whitted_shade_point), known answers worked out by hand, and the whole pipeline on the three scenes of
tests/whitted_shading_scenes.py.  tests/test_whitted_shading_float64.py holds the device to the same reference with the same constants."""
import functools

import numpy as np
import pytest

import whitted_ref64 as R
import whitted_shading_scenes as S

# The largest dev (whitted_ref64.dev: |c32 - c64| / (kappa max(|c64|, 1e-3)) in units of 2^-23, over clear cases / pixels) measured on
# the CPU, per family; the bounds are 4 x that, the convention of test_oracle_float64.py: room for another libm,
# none for a wrong term.
MEASURED = {"untextured": 3.50, "textured": 2.53, "normal-mapped": 3.02, "pipeline": 18.65}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
# the share of hit pixels that may be unclear, and what a scene must show
UNCLEAR_CAP = {"sweep": 0.05, "instanced": 0.05, "textured": 0.15, "textured_nouv": 0.15}
MIN_LIT, MIN_SHADOW = 0.40, 0.05


# ---- the closest-hit sweep ----------------------------------------------------------------------------------------------------------
def _sphere(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _around(rng, axis, cos_lo, cos_hi):
    """unit vectors whose cosine to `axis` [n, 3] is uniform in [cos_lo, cos_hi], at a uniform azimuth"""
    n = len(axis)
    t = np.cross(axis, _sphere(rng, n))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(axis, t)
    c = cos_lo + (cos_hi - cos_lo) * rng.rand(n)
    s, phi = np.sqrt(np.maximum(0.0, 1.0 - c * c)), 2 * np.pi * rng.rand(n)
    return c[:, None] * axis + (s * np.cos(phi))[:, None] * t + (s * np.sin(phi))[:, None] * b


@functools.lru_cache(maxsize=None)
def _sweep_textures():
    rng = np.random.RandomState(77)
    rgba = lambda h, w: rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
    return {"bc": rgba(5, 7), "mr": rgba(4, 4), "nm_up": S.normal_map(rng, 5, 7), "nm_any": rgba(4, 4)}


def sweep_cases(n, textured, seed):
    """n seeded cases of the closest-hit program, every input a float32 number: N uniform on the sphere; V and one to three L uniform
    over N's hemisphere; a tenth of the cases with one of them below it (the gate); a fifth within 2 degrees of grazing in N.V or N.L; a
    fifth with H within 1 degree of N (the highlight); roughness log-uniform in [0.05, 1], metallic 0, 1 or uniform, the base colour
    uniform; light distance log-uniform in [0.1, 100], intensity in [0.1, 10]; corner UVs and UV in [-2, 3].  textured: each case reads
    a non-empty choice of the three textures (7 x 5, 4 x 4), its normal map with z >= 0.5 in three quarters of them."""
    rng = np.random.RandomState(seed)
    N = _sphere(rng, n)
    V = _around(rng, N, 0.0, 1.0)
    L = np.stack([_around(rng, N, 0.0, 1.0) for _ in range(3)], 1)
    kind = rng.rand(n)
    graze = _around(rng, N, 0.0, np.cos(np.radians(88.0)))
    below = _around(rng, N, -1.0, 0.0)
    which = rng.randint(0, 2, n).astype(bool)
    g, b = kind < 0.2, (kind >= 0.4) & (kind < 0.5)
    V[g & which], L[g & ~which, 0] = graze[g & which], graze[g & ~which]
    V[b & which], L[b & ~which, 0] = below[b & which], below[b & ~which]
    h = (kind >= 0.2) & (kind < 0.4)
    Hh = _around(rng, N, np.cos(np.radians(1.0)), 1.0)
    L[h, 0] = (2.0 * (V * Hh).sum(-1, keepdims=True) * Hh - V)[h]
    n_lights = rng.randint(1, 4, n)
    P = rng.uniform(-3, 3, (n, 3))
    dist = 0.1 * 1000.0 ** rng.rand(n, 3)
    lights = np.zeros((n, 3, 8))
    lights[..., 0:3] = rng.uniform(0.2, 1.0, (n, 3, 3))
    lights[..., 3] = rng.uniform(0.1, 10.0, (n, 3))
    lights[..., 4:7] = P[:, None] + dist[..., None] * L
    mats = np.ones((n, 6))
    mats[:, 0:3] = rng.rand(n, 3)
    m = rng.rand(n)
    mats[:, 4] = np.where(m < 1 / 3, 0.0, np.where(m < 2 / 3, 1.0, rng.rand(n)))
    mats[:, 5] = 0.05 * 20.0 ** rng.rand(n)
    corners = P[:, None] + rng.uniform(-1, 1, (n, 3, 3))
    cuv, uv = rng.uniform(-2, 3, (n, 3, 2)), rng.uniform(-2, 3, (n, 2))
    rd = -V * rng.uniform(0.5, 2.0, (n, 1))
    tex = np.zeros((n, 3), np.int64)       # (base colour, metallic-roughness, normal map: 0 none, 1 z >= 0.5, 2 unrestricted)
    if textured:
        pick = rng.randint(1, 8, n)
        tex[:, 0], tex[:, 1], tex[:, 2] = pick & 1, (pick >> 1) & 1, ((pick >> 2) & 1) * np.where(rng.rand(n) < 0.75, 1, 2)
    f = lambda a: np.asarray(a, np.float32)
    return {"P": f(P), "N": f(N), "C": f(corners), "CUV": f(cuv), "UV": f(uv), "rd": f(rd), "mats": f(mats), "lights": f(lights),
            "n_lights": n_lights, "tex": tex, "kind": kind}


def _triple(tex_row):
    t = _sweep_textures()
    return (t["bc"] if tex_row[0] else None, t["mr"] if tex_row[1] else None, {0: None, 1: t["nm_up"], 2: t["nm_any"]}[int(tex_row[2])])


def sweep_reference(c):
    """whitted_ref64.shade over the cases, grouped by light count and texture choice: color, clear, kappa [n, 3], gate-passing lights [n]"""
    n = len(c["P"])
    color, kappa, clear, gates = np.zeros((n, 3)), np.ones((n, 3)), np.zeros(n, bool), np.zeros(n, np.int64)
    groups = {}
    for k in range(n):
        groups.setdefault((int(c["n_lights"][k]),) + tuple(int(x) for x in c["tex"][k]), []).append(k)
    for (nl, *tx), rows in groups.items():
        r = np.array(rows)
        g = {k: c[k][r].astype(np.float64) for k in ("P", "N", "C", "CUV", "UV")}
        sh = R.shade(g, c["rd"][r].astype(np.float64), c["mats"][r], _triple(tx), c["lights"][r][:, :nl])
        color[r], kappa[r], clear[r], gates[r] = sh["color"], sh["kappa"], sh["clear"], (sh["state"] != R.GATED).sum(axis=1)
    return color, clear, kappa, gates


def sweep_oracle(oracle, c):
    n = len(c["P"])
    color, gates = np.zeros((n, 3), np.float32), np.zeros(n, np.int64)
    for k in range(n):
        tx = _triple(c["tex"][k])
        color[k], gates[k] = oracle.whitted_shade_point(c["P"][k], c["N"][k], c["C"][k], c["CUV"][k], c["UV"][k], c["rd"][k], c["mats"][k],
                                                        c["lights"][k, :c["n_lights"][k]], textures=tx)
    return color, gates


@pytest.mark.parametrize("textured", [False, True], ids=["untextured", "textured"])
def test_closest_hit_sweep(oracle, textured):
    """20 000 cases without textures, 5 000 with: the same gate on every clear case, dev within the family's bound"""
    n = 5000 if textured else 20000
    c = sweep_cases(n, textured, seed=5 if textured else 3)
    want, clear, kappa, gates = sweep_reference(c)
    got, got_gates = sweep_oracle(oracle, c)
    k = c["kind"]
    assert clear.mean() > 0.8 and (want[clear] > 0).any(axis=1).mean() > 0.7
    assert ((k < 0.2) & clear).sum() > 0.15 * n and ((k >= 0.2) & (k < 0.4) & clear).sum() > 0.15 * n      # grazing, highlight
    assert (gates[clear] < c["n_lights"][clear]).mean() > 0.05                                                # the gate closes
    assert np.array_equal(got_gates[clear], gates[clear]), "gate"
    d = R.dev(got, want, kappa).max(axis=1)
    fam = np.where(c["tex"][:, 2] > 0, "normal-mapped", np.where(c["tex"][:, :2].any(axis=1), "textured", "untextured"))
    for name in sorted(set(fam)):
        rows = clear & (fam == name)
        worst = d[rows].max()
        print("closest hit, %s: %d clear cases, largest dev %.2f (bound %.1f), largest kappa %.0f" % (name, rows.sum(), worst, BOUND[name], kappa[rows].max()))
        assert worst <= BOUND[name], (name, worst, int(np.argmax(np.where(rows, d, 0))))
    if textured:
        loose = clear & (c["tex"][:, 2] == 2)
        assert loose.sum() > 300 and (kappa[loose].max(axis=1) > 2 * kappa[clear & (c["tex"][:, 2] == 1)].max(axis=1).mean()).any()


# ---- known answers --------------------------------------------------------------------------------------------------------------------
PI = float(np.float32(np.pi))      # M_PIf
TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
TRI_UV = np.array([[0, 0], [1, 0], [0, 1]], np.float32)


def _point(oracle, mat, light_dir=(0, 0, 1), view_dir=(0, 0, 1), textures=None, corner_uv=TRI_UV, uv=(0.3, 0.3), dist=2.0, color=(1.0, 0.5, 0.25),
           intensity=2.0, N=(0, 0, 1)):
    """the shade of the point (0, 0, 0) of the triangle TRI with normal N, seen from view_dir, under one light at dist along light_dir"""
    light = np.array([list(color) + [intensity] + list(dist * np.asarray(light_dir, np.float64)) + [0]], np.float32)
    return oracle.whitted_shade_point([0, 0, 0], N, TRI, corner_uv, uv, -np.asarray(view_dir, np.float32), mat, light, textures=textures)[0].astype(np.float64)


def _close(got, want, rel=1e-6, absolute=0.0):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert (np.abs(got - want) <= rel * np.abs(want) + absolute).all(), (got, want)


LC = 2.0 * np.array([1.0, 0.5, 0.25])    # the light's colour times its intensity
BASE = np.array([0.8, 0.6, 0.25])


def test_known_normal_incidence_dielectric(oracle):
    """L = V = N, roughness 1: alpha = 1, so D = 1 / pi and vis = 1; V.H = 1, so F = F0 = 0.04; diff = (1 - 0.04) base 0.96 / pi"""
    got = _point(oracle, [0.8, 0.6, 0.25, 1, 0.0, 1.0])
    _close(got, LC * ((1 - 0.04) * BASE * 0.96 / PI + 0.04 * 1.0 * (1 / PI)))


def test_known_normal_incidence_metal(oracle):
    """the same on a metal: no diffuse term, F = base"""
    got = _point(oracle, [0.8, 0.6, 0.25, 1, 1.0, 1.0])
    _close(got, LC * BASE / PI)


def test_known_fresnel_at_v_dot_h_zero(oracle):
    """V.H -> 0 makes F -> 1 whatever the material.  V.H = 0 itself needs L = -V (no half vector), so: V and L mirror images at the cosine
    c = 2^-12 to N, the light at distance 2 (L.x = -V.x exactly, so H = N): N.L = N.V = V.H = c, N.H = 1; at roughness 1 D = 1 / pi,
    vis = 2 c c / (c + c) = c, F = s + (1 - s) (1 - c)^5: radiance = lc c (F c / pi + (1 - F) diffuse / pi)"""
    c = 2.0 ** -12
    sx = np.sqrt(1 - c * c)
    out = []
    for metallic in (0.0, 1.0):
        got = _point(oracle, [0.8, 0.6, 0.25, 1, metallic, 1.0], light_dir=(-sx, 0, c), view_dir=(sx, 0, c))
        s = 0.04 + (BASE - 0.04) * metallic
        Fr = s + (1 - s) * (1 - c) ** 5
        # (1 - F is formed in float32 from an F next to 1, so it carries F's rounding, 2^-24, as an absolute error: that of the diffuse term)
        _close(got, LC * c * (Fr * c / PI + (1 - Fr) * BASE * 0.96 * (1 - metallic) / PI), absolute=2.0 ** -23 * LC * c * BASE * 0.96 * (1 - metallic) / PI)
        out.append(got)
    # F -> 1 on both: of the dielectric's diffuse term, 4096 times the specular term at F = F0, 1 - F = 0.96 (5 c) is left
    assert (out[0] <= LC * c * (c / PI + 5 * c * BASE * 0.96 / PI) * (1 + 1e-6)).all() and (out[1] <= LC * c * c / PI * (1 + 1e-6)).all(), out


def _uniform(rgba):
    return np.tile(np.array(rgba, np.uint8), (4, 4, 1))


def test_known_roughness_and_metallic_channels(oracle):
    """a metallic-roughness texture's green scales the roughness and nothing else, its blue the metallic and nothing else, its red
    (occlusion) nothing at all"""
    mat = [0.8, 0.6, 0.25, 1, 0.9, 0.8]
    Ld, Vd = (0.3, 0.2, 0.93), (-0.4, 0.1, 0.9)
    with_rough = _point(oracle, mat, Ld, Vd, textures=(None, _uniform([255, 102, 255, 255]), None))
    _close(with_rough, _point(oracle, [0.8, 0.6, 0.25, 1, 0.9, 0.8 * 102 / 255], Ld, Vd))
    with_metal = _point(oracle, mat, Ld, Vd, textures=(None, _uniform([255, 255, 51, 255]), None))
    _close(with_metal, _point(oracle, [0.8, 0.6, 0.25, 1, 0.9 * 51 / 255, 0.8], Ld, Vd))
    assert (np.abs(with_rough - with_metal) > 0.05 * with_metal).any()                # (the two are not the same picture)
    plain = _point(oracle, mat, Ld, Vd)
    assert np.array_equal(_point(oracle, mat, Ld, Vd, textures=(None, _uniform([17, 255, 255, 99]), None)), plain)


def test_known_flatnormal_map(oracle):
    """(128, 128, 255) is (1 / 255, 1 / 255, 1): N moves by the 8-bit step.  On TRI dp/du = (1, 0, 0), dp/dv = (0, 1, 0), so
    N' = (a, a, 1) / sqrt(1 + 2 a^2), a = 1 / 255; with L = V = (0, 0, 1), roughness 1: N'.L = N'.V = 1 / sqrt(1 + 2 a^2) = nl, vis = nl,
    D = 1 / pi, F = F0"""
    mat = [0.8, 0.6, 0.25, 1, 0.0, 1.0]
    got = _point(oracle, mat, textures=(None, None, _uniform([128, 128, 255, 255])))
    a = 1 / 255
    nl = 1 / np.sqrt(1 + 2 * a * a)
    _close(got, LC * nl * (0.96 * BASE * 0.96 / PI + 0.04 * nl / PI))
    _close(got, _point(oracle, mat), rel=2 * a * a * 1.5)          # N within the 8-bit step: the cosine within a^2


def test_known_normal_map_of_plus_x_follows_dpdu(oracle):
    """(255, 128, 128) is (1, a, a), a = 1 / 255: N' = normalize(T + a B + a N), T = normalize(dp/du), B = normalize(dp/dv).  TRI's UVs
    sheared -- UV0 = (0, 0), UV1 = (1, 1/2), UV2 = (0, 1) -- give P1 - P0 = dp/du + dp/dv / 2 and P2 - P0 = dp/dv: dp/dv = (0, 1, 0),
    dp/du = (1, -1/2, 0), which is no edge of the triangle.  Seen and lit along D = (2, -1, 1) / sqrt(6) at roughness 1: V.H = 1, F = F0,
    N'.L = N'.V = nl, vis = nl, D = 1 / pi"""
    mat = [0.8, 0.6, 0.25, 1, 0.0, 1.0]
    uvs = np.array([[0, 0], [1, 0.5], [0, 1]], np.float32)
    D = np.array([2.0, -1.0, 1.0]) / np.sqrt(6.0)
    got = _point(oracle, mat, D, D, textures=(None, None, _uniform([255, 128, 128, 255])), corner_uv=uvs)
    a = 1 / 255
    Nn = np.array([2.0, -1.0, 0.0]) / np.sqrt(5.0) + a * np.array([0.0, 1.0, 0.0]) + a * np.array([0.0, 0.0, 1.0])
    nl = (Nn / np.linalg.norm(Nn)) @ D
    _close(got, LC * nl * (0.96 * BASE * 0.96 / PI + 0.04 * nl / PI))
    swapped = np.array([0.0, 1.0, 0.0]) + a * np.array([2.0, -1.0, 0.0]) / np.sqrt(5.0) + a * np.array([0.0, 0.0, 1.0])     # dp/dv in dp/du's place
    assert (swapped / np.linalg.norm(swapped)) @ D < 0         # ... would be gated: black


def test_known_occlusion_window(oracle):
    """an occlusion ray runs over 0.001 < t < L_dist - 0.001.  The point (0, 0, 0) under a light at (0, 0, 2) with the triangle of the
    corners across the ray at height z: at z = 0.0005 (before the window) and z = 2 - 0.0005 (past its end, in front of the light) the point
    is lit as without it; at z = 0.002, 1 and 2 - 0.002 it is black"""
    mat = [0.8, 0.6, 0.25, 1, 0.0, 1.0]
    light = np.array([[1.0, 0.5, 0.25, 2.0, 0, 0, 2.0, 0]], np.float32)
    lit = LC * ((1 - 0.04) * BASE * 0.96 / PI + 0.04 / PI)
    for z, want in ((0.0005, lit), (2 - 0.0005, lit), (0.002, 0 * lit), (1.0, 0 * lit), (2 - 0.002, 0 * lit)):
        tri = np.array([[-1, -1, z], [2, -1, z], [-1, 2, z]], np.float32)
        got, n = oracle.whitted_shade_point([0, 0, 0], [0, 0, 1], tri, TRI_UV, (0.3, 0.3), [0, 0, -1], mat, light, occlusion=True)
        assert n == 1
        _close(got, want)


# ---- the whole pipeline ---------------------------------------------------------------------------------------------------------------
def scene(name):
    return S.textured(texcoords=False) if name == "textured_nouv" else S.SCENES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """whitted_ref64.render of the scene, subframes 0 .. 2 (computed once; nobody writes to it)"""
    return R.render(scene(name), S.W, S.H, S.SUBFRAMES)


def check_conditions(name, ref):
    """what the scene must show, from the reference alone; returns the unclear share of the hit pixels"""
    hit = ref[0]["hit"]
    lit = (ref[0]["state"] == R.LIT).any(axis=-1).mean()
    shadow = (ref[0]["state"] == R.SHADOWED).any(axis=-1).mean()
    unclear = (hit & ~ref[-1]["clear"]).sum() / hit.sum()
    assert lit >= MIN_LIT and shadow >= MIN_SHADOW and unclear <= UNCLEAR_CAP[name], (name, lit, shadow, unclear)
    assert 0.02 < (~hit).mean() and (name != "sweep" or (ref[0]["state"] == R.GATED).all(axis=-1).mean() > 0.05)    # the gate closes on whole pixels
    return lit, shadow, unclear


def check_light_pattern(name, acc0, r0):
    """subframe 0: which lights reach each clear pixel, judged from its colour -- of all sums of a subset of the reference's per-light
    terms, the one nearest to the colour is the reference's own (subsets whose sums differ by less than 1e-3 of the pixel count as one)"""
    terms, state = r0["terms"], r0["state"]
    nl = terms.shape[2]
    c = acc0[..., :3].astype(np.float64)
    own = (terms * (state == R.LIT)[..., None]).sum(axis=2)
    best = np.abs(c - own).sum(axis=-1)
    scale = 1e-3 * np.maximum(np.abs(own).sum(axis=-1), 1e-3)
    rows = r0["clear"] & r0["hit"]
    wrong = np.zeros_like(rows)
    for subset in range(1 << nl):
        pick = np.array([(subset >> l) & 1 for l in range(nl)], bool)
        other = terms[:, :, pick].sum(axis=2)
        distinct = np.abs(other - own).sum(axis=-1) > scale
        wrong |= rows & distinct & (np.abs(c - other).sum(axis=-1) <= best)
    assert not wrong.any(), (name, "light pattern", np.argwhere(wrong)[:5])
    assert ((state == R.SHADOWED).any(axis=-1) & rows).sum() > 50


def check_frame(name, acc, img, r, miss, what):
    """one accumulated frame against the reference after as many subframes: returns (largest dev, share of bit-exact 8-bit pixels)"""
    clear = r["clear"]
    assert (acc[..., 3] == 1.0).all() and (img[..., 3] == 255).all(), (name, what, "alpha")
    d = np.where(clear[..., None], R.dev(acc[..., :3], r["color"], r["kappa"]), 0.0)
    worst = float(d.max())
    at = np.unravel_index(np.argmax(d), d.shape)
    assert worst <= BOUND["pipeline"], (name, what, worst, at, acc[at[0], at[1]], r["color"][at[0], at[1]], r["kappa"][at[0], at[1]])
    diff = np.abs(img[..., :3].astype(np.int64) - r["byte"].astype(np.int64))
    exact = r["byte_exact"] & clear[..., None]
    assert (diff[exact] == 0).all() and (diff[clear] <= 1).all(), (name, what, "8-bit image", np.argwhere(exact & (diff != 0))[:5])
    return worst, float((diff == 0).all(axis=-1).mean())


def check_miss(name, frames, ref, miss):
    """pixels every subframe so far misses clearly are exactly the miss colour"""
    missed = np.ones_like(ref[0]["hit"])
    for s, (acc, _) in enumerate(frames):
        missed &= ~ref[s]["hit"]
        rows = missed & ref[s]["clear"]
        assert rows.sum() > 30 and (acc[rows][:, :3] == np.float32(miss)).all(), (name, s, "miss pixels")


def oracle_frames(oracle, sc):
    """[(accum, image)] after 1, 2, 3 subframes, and subframe 0's ray counts"""
    acc, img = np.zeros((S.H, S.W, 4), np.float32), np.zeros((S.H, S.W, 4), np.uint8)
    out, rays0 = [], None
    flat = len(sc["instances"]) == 1
    for n in range(1, S.SUBFRAMES + 1):      # (the oracle keeps no state: n subframes from the start each time)
        if flat:
            acc, img, rays = oracle.whitted_render(S.flat_mesh(sc), sc["cam"], S.W, S.H, n)
        else:
            acc, img, rays = oracle.whitted_render_instanced(sc["meshes"], sc["instances"], sc["materials"], S.extra(sc), sc["cam"], S.W, S.H, n)
        rays0 = rays0 or rays
        out.append((acc, img))
    return out, rays0


def occlusion_ray_bounds(r0):
    """subframe 0's count of gate-passing (pixel, light) pairs: (over the pairs whose gate is clear, that plus the unclear pairs)"""
    passing = (r0["state"] == R.SHADOWED) | (r0["state"] == R.LIT)
    sure = int((passing & r0["gate_clear"]).sum())
    return sure, sure + int((~r0["gate_clear"]).sum())      # (an unclear pair may go either way, on an unclear miss too)


@pytest.mark.parametrize("name", ["sweep", "textured", "textured_nouv", "instanced"])
def test_pipeline_against_float64(oracle, name):
    sc, ref = scene(name), reference(name)
    lit, shadow, unclear = check_conditions(name, ref)
    frames, rays0 = oracle_frames(oracle, sc)
    # the same (instance, triangle) on subframe 0's clear primaries
    o, d = R.primaries32(sc["cam"], S.W, S.H)
    isc = oracle.InstancedScene(sc["meshes"], sc["instances"], sc["materials"], S.extra(sc))
    rows = np.nonzero((ref[0]["clear"] & ref[0]["hit"]).reshape(-1))[0]
    got = np.array([isc.trace(o[k], d[k])[:2] for k in rows], np.int64)
    assert np.array_equal(got, ref[0]["key"].reshape(-1, 2)[rows]), "closest hit"
    check_light_pattern(name, frames[0][0], ref[0])
    lo, hi = occlusion_ray_bounds(ref[0])
    assert rays0["rays_total"] - S.W * S.H == rays0["rays_occlusion"] and lo <= rays0["rays_occlusion"] <= hi, (rays0, lo, hi)
    check_miss(name, frames, ref, sc["miss"])
    for s, (acc, img) in enumerate(frames):
        worst, same8 = check_frame(name, acc, img, ref[s], sc["miss"], "subframes 0 .. %d" % s)
        print("%s, subframes 0 .. %d: lit %.3f, shadowed %.3f, unclear %.4f of the hit pixels, largest dev %.2f (bound %.1f), 8-bit identical %.4f"
              % (name, s, lit, shadow, unclear, worst, BOUND["pipeline"], same8))
