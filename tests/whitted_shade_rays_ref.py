"""What the tests of rtgo_whitted_shade_rays share (test_whitted_shade_rays_ref.py on the CPU, test_whitted_shade_rays.py on the device).
Numpy only.

  raygen32      whitted::raygen on the host, in float32, operation for operation: the rays rtgo_whitted_launch traces for a subframe.  The
                library is compiled without contraction and its quotient and square root are the correctly rounded ones, so these are the
                device's rays bit for bit -- the bitwise tests rest on that, and a pixel that differs is a slip HERE.
  ortho_rays    an orthographic view of a scene of tests/whitted_shading_scenes.py with directions that are not unit length: a camera the
                launches do not have.
  reference     tests/whitted_ref64.py on arbitrary rays: _Scene.closest, local_geometry and shade composed as whitted_ref64.render
                composes them for one subframe, shaped for test_oracle_whitted_float64.check_frame."""
import functools

import numpy as np

import whitted_ref64 as R
import whitted_shading_scenes as S
import test_oracle_whitted_float64 as T

F = np.float32
TMIN, TMAX = F(0.01), F(1e16)       # the primary ray's window in whitted.cu (whitted_ref64.T_MIN, T_MAX: what _Scene.closest accepts)
# half the width of the orthographic view, per scene
HALF = {"sweep": 3.0, "textured": 3.0, "textured_nouv": 3.0, "instanced": 2.2}


def raygen32(cam, W, H, subframe):
    """float32 origins [W H, 3] and directions [W H, 3] of __raygen__pinhole at `subframe`, raster order"""
    cam = np.asarray(cam, F)
    eye, U, V, Wv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    j = R.jitter(W, H, subframe)                                # float32: (0, 0) at subframe 0
    idx = np.arange(W * H)
    x, y = (idx % W).astype(F), (idx // W).astype(F)
    dx = F(2) * ((x + j[:, 0]) / F(W)) - F(1)
    dy = F(2) * ((y + j[:, 1]) / F(H)) - F(1)
    d = (dx[:, None] * U + dy[:, None] * V) + Wv
    dot = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    inv = F(1) / np.sqrt(dot)
    d = d * inv[:, None]
    assert d.dtype == F and dx.dtype == F and inv.dtype == F
    return np.tile(eye, (W * H, 1)).astype(F), d


def ortho_rays(cam, W, H, half, seed=1):
    """origins eye + sx U^ + sy V^ over the pixel centres (sx = (2 (i + .5) / W - 1) half, sy = (2 (j + .5) / H - 1) half H / W), directions
    W^ 2^u with u uniform in [-2, 2]: everything rounded to float32"""
    cam = np.asarray(cam, F).astype(np.float64)
    eye, U, V, Wv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    Uh, Vh, Wh = (a / np.linalg.norm(a) for a in (U, V, Wv))
    idx = np.arange(W * H)
    sx = (2.0 * ((idx % W) + 0.5) / W - 1.0) * half
    sy = (2.0 * ((idx // W) + 0.5) / H - 1.0) * half * H / W
    o = eye + sx[:, None] * Uh + sy[:, None] * Vh
    u = np.random.RandomState(seed).uniform(-2.0, 2.0, W * H)
    d = Wh[None] * (2.0 ** u)[:, None]
    return o.astype(F), d.astype(F)


def reference(scene, o, d, shape):
    """the float64 radiance of the float32 rays (o, d) over 0.01 < t < 1e16, as one sample (sample_index 0).  Returns a dict shaped
    shape + (...): color, kappa [.., 3], clear, hit [..], byte, byte_exact [.., 3], state, state_clear, gate_clear [.., nl], key [.., 2]"""
    sc = R._Scene(scene)
    nl = len(sc.lights)
    o, d = np.asarray(o, F).astype(np.float64), np.asarray(d, F).astype(np.float64)
    n = len(o)
    hit, clear, key, t, u, v, berr = sc.closest(o, d)
    color = np.tile(sc.miss, (n, 1))
    kappa = np.ones((n, 3))
    state, state_clear = np.full((n, nl), R.MISS, np.int64), np.ones((n, nl), bool)
    gate_clear = np.tile(clear[:, None], (1, nl))
    r = np.nonzero(hit)[0]
    g = sc.local_geometry(key[r], u[r], v[r], berr[r])
    for mi in np.unique(g["material"]):
        q = np.nonzero(g["material"] == mi)[0]
        gq = {k: a[q] for k, a in g.items()}
        sh = R.shade(gq, d[r[q]], np.tile(sc.materials[mi], (len(q), 1)), sc.textures.get(int(mi)), sc.lights, sc.occluded)
        rows = r[q]
        color[rows], kappa[rows], state[rows], state_clear[rows] = sh["color"], sh["kappa"], sh["state"], sh["state_clear"]
        gate_clear[rows] &= sh["gate_clear"]
        clear[rows] &= sh["clear"]
    byte, exact = R.make_color(color)
    sh = tuple(shape)
    return {"color": color.reshape(sh + (3,)), "kappa": kappa.reshape(sh + (3,)), "clear": clear.reshape(sh), "hit": hit.reshape(sh),
            "byte": byte.reshape(sh + (3,)), "byte_exact": exact.reshape(sh + (3,)), "state": state.reshape(sh + (nl,)),
            "state_clear": state_clear.reshape(sh + (nl,)), "gate_clear": gate_clear.reshape(sh + (nl,)), "key": key.reshape(sh + (2,))}


@functools.lru_cache(maxsize=None)
def ortho_case(name):
    """(scene, origins, directions, reference) of the orthographic view of scene `name` (computed once; nobody writes to it)"""
    sc = T.scene(name)
    o, d = ortho_rays(sc["cam"], S.W, S.H, HALF[name])
    return sc, o, d, reference(sc, o, d, (S.H, S.W))


def conditions(ref):
    """(lit, shadowed: share of the rays some light reaches / some occlusion ray shadows; unclear share of the hits; share of clear misses)"""
    hit = ref["hit"]
    lit = (ref["state"] == R.LIT).any(axis=-1).mean()
    shadow = (ref["state"] == R.SHADOWED).any(axis=-1).mean()
    unclear = (hit & ~ref["clear"]).sum() / max(hit.sum(), 1)
    return float(lit), float(shadow), float(unclear), float((~hit & ref["clear"]).mean())
