"""A float64 reference for the triangle ("whitted") path after the hit: what cuda/whitted.cu and cuda/LocalGeometry.h compute, as real
numbers (numpy only: nothing of the oracle or the product is imported here, so a slip the two share does not reach this file).  Written
from whitted.cu:52-85, 165-174, 183-337, LocalGeometry.h:53-137 and the definitions: the GGX distribution D = a^2 / (pi x^2) with
x = (N.H)^2 (a^2 - 1) + 1, the height-correlated Smith visibility in the form the file writes it (2 NL NV / (NL sqrt(NV^2 (1 - a^2) + a^2)
+ NV sqrt(NL^2 (1 - a^2) + a^2))), Schlick's Fresnel F = F0 + (1 - F0) (1 - V.H)^5 and the glTF metallic-roughness split with F0 = 0.04
(diffuse = base (1 - F0) (1 - metallic), specular F0 = lerp(0.04, base, metallic), a = roughness^2).  The file's float literals (0.04f,
2.2f, M_PIf, 0.01f, 0.001f, 1e16f, the float exponent 1 / 2.2f of make_color) are the float32 numbers they are, widened.

Per pixel of a W x H launch at a subframe:
  1. the primary ray from the float32 camera and the jitter: tea<4>, lcg, rnd in integers (exact), jitter = the float32 rnd - 0.5;
  2. the closest hit by brute force over (instance, triangle): the ray goes to object space through numpy.linalg.inv of the float32
     transform, not renormalised (t is the same number in both spaces), Moeller-Trumbore's t, u, v as triple products, 0.01 < t < 1e16;
  3. getLocalGeometry: P the object-space barycentric point through O2W; Ng = normalize(cross) in object space, then W2O^T, NOT
     renormalised; N = Ng without vertex normals (so N is not unit length under a non-rigid transform: the reference's rule), otherwise
     normalize(W2O^T interp); UV interpolated, or the barycentrics against the corners (0,0), (0,1), (1,0); dp/du, dp/dv from the
     object-space corners;
  4. the three texture branches, tex2D as DESIGN.md 3.4 states it: wrap addressing, x_B = u N - 0.5, texel floor(x_B), a weight of 8
     fractional bits rounded to nearest (the hardware's rounding is unpublished: round to nearest is this project's rule), the blend exact;
  5. the light loop: the N.L > 0 && N.V > 0 gate, an any-hit occlusion ray over 0.001 < t < L_dist - 0.001 by brute force, the sum;
  6. the running average over subframes 0 .. s, lerp(prev, new, 1 / (s + 1));
  7. make_color: the byte is the TRUNCATION of pow(clamp(c, 0, 1), 1 / 2.2) 255.

Every comparison on that way can fall the other way in float32, so a pixel is CLEAR only when each has a margin:
  the closest hit   the winner's barycentrics at least 1e-5 inside, its t at least 1e-5 (relative) past tmin, and no other triangle that
                    hits or misses by less than 1e-5 in its barycentrics within 1e-5 (relative) of the winner's t or before it
                    (tests/trace_rays_ref.clear_triangle_rays' constants); a miss is clear when no triangle comes that close;
  occlusion rays    the DECISION has a margin: some triangle is hit at least 1e-5 inside with t at least 1e-5 (relative) from both ends
                    of the window, or none is hit or missed by less than that;
  the gate          |N.L| and |N.V| at least 1e-5;
  texture weights   x_B 256 at least 0.01 from a rounding boundary (k + 1/2) and x_B at least 0.01 / 256 from an integer, both axes,
                    every texture read (float32 places u N to about 0.003 of a weight step at u <= 3, N <= 16) -- and at least as far
                    as float32 can place the interpolated UV itself: the barycentrics' uncertainty (closest()) times the spread of the
                    triangle's corner UVs, which exceeds 0.01 of a step where one triangle spans a whole wrap (a seam) or most of a texture;
  the byte          compared exactly only where pow(c, 1 / 2.2) 255 lies at least 1e-3 from an integer; within 1 elsewhere.

A deviation is judged against what float32 can deliver at that pixel: the condition number kappa >= 1, per channel the colour-weighted
mean over the contributing lights (and subframes) of 1 + 2 / x_l + |N| (2 / N.L + 1 / N.V) (+ 1 / |n| where a normal map is blended, n the
unnormalised blend): D goes as x^-2, and x is formed by cancellation from terms of size 1; the radiance goes as N.L (the cosine) to N.L^2
(the cosine times a visibility term that vanishes with it) and at most as N.V, and each is a dot product of vectors of size |N| and 1
that float32 places to about 2^-24 |N| whatever its own size -- without the grazing terms a pixel at N.L = 1e-3 shows 1e-4 relative, a
few hundred units.  dev() is |c32 - c64| / (kappa max(|c64|, 1e-3)) in units of 2^-23."""
import numpy as np

F = np.float32


def _w(x):
    return float(F(x))


PI_F, F0, GAMMA = _w(3.14159265358979323846), _w(0.04), _w(2.2)
INV_GAMMA = _w(1.0 / _w(2.2))
T_MIN, T_MAX, OCC_EPS = _w(0.01), _w(1e16), _w(0.001)
BARY_MARGIN = 1e-5      # clear_triangle_rays' constants
T_MARGIN = 1e-5
GATE_MARGIN = 1e-5
WEIGHT_MARGIN = 0.01    # of a weight step (1 / 256 of a texel)
BARY_ULPS = 4.0         # float32 Moeller-Trumbore places u and v to about this many 2^-24 of |o - P0| |d| max|e| / |det|: see closest()
BYTE_MARGIN = 1e-3
UNIT = 2.0 ** -23
MISS, GATED, SHADOWED, LIT = -1, 0, 1, 2


# ---- cuda/random.h:30-66 in integers ----
def tea4(v0, v1):
    m = np.uint64(0xFFFFFFFF)
    v0 = np.asarray(v0, np.uint64) & m
    v1 = (np.zeros_like(v0) + np.uint64(v1)) & m
    s0 = np.uint64(0)
    for _ in range(4):
        s0 = (s0 + np.uint64(0x9E3779B9)) & m
        v0 = (v0 + ((((v1 << np.uint64(4)) & m) + np.uint64(0xA341316C)) ^ (v1 + s0) ^ ((v1 >> np.uint64(5)) + np.uint64(0xC8013EA4)))) & m
        v1 = (v1 + ((((v0 << np.uint64(4)) & m) + np.uint64(0xAD90777D)) ^ (v0 + s0) ^ ((v0 >> np.uint64(5)) + np.uint64(0x7E95761E)))) & m
    return v0


def lcg(prev):
    prev = (np.uint64(1664525) * prev + np.uint64(1013904223)) & np.uint64(0xFFFFFFFF)
    return prev, prev & np.uint64(0x00FFFFFF)


def jitter(W, H, subframe):
    """[H W, 2] float32: (0, 0) at subframe 0, else (rnd - 0.5, rnd - 0.5), x drawn first"""
    if subframe == 0:
        return np.zeros((W * H, 2), F)
    seed = tea4(np.arange(W * H, dtype=np.uint64), subframe)
    seed, a = lcg(seed)
    seed, b = lcg(seed)
    return np.stack([a.astype(F) / F(0x01000000) - F(0.5), b.astype(F) / F(0x01000000) - F(0.5)], 1)


def primaries(cam, W, H, subframe):
    """float64 origins [n, 3] and unit directions [n, 3] of __raygen__pinhole, raster order"""
    cam = np.asarray(cam, F).astype(np.float64)
    eye, U, V, Wv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    j = jitter(W, H, subframe).astype(np.float64)
    idx = np.arange(W * H)
    dx = 2.0 * (((idx % W) + j[:, 0]) / W) - 1.0
    dy = 2.0 * (((idx // W) + j[:, 1]) / H) - 1.0
    d = dx[:, None] * U + dy[:, None] * V + Wv
    return np.tile(eye, (W * H, 1)), _normalize(d)


def primaries32(cam, W, H):
    """subframe 0's primaries in float32 (for single-ray traces): origins [n, 3], directions [n, 3]"""
    cam = np.asarray(cam, F)
    eye, U, V, Wv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    idx = np.arange(W * H)
    dx = (F(2) * ((idx % W).astype(F) / F(W)) - F(1)).astype(F)
    dy = (F(2) * ((idx // W).astype(F) / F(H)) - F(1)).astype(F)
    d = ((dx[:, None] * U + dy[:, None] * V) + Wv).astype(F)
    dot = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(F)
    d = (d * (F(1) / np.sqrt(dot))[:, None]).astype(F)
    return np.tile(eye, (W * H, 1)).astype(F), d


def _normalize(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _dot(a, b):
    return (a * b).sum(-1)


# ---- triangles ----
class _Mesh:
    def __init__(self, mesh):
        pos = np.asarray(mesh["positions"], F).astype(np.float64).reshape(-1, 3)
        self.ix = np.asarray(mesh["indices"], np.int64).reshape(-1, 3)
        self.P = pos[self.ix]                                                  # [T, 3 corners, 3]
        self.e1, self.e2 = self.P[:, 1] - self.P[:, 0], self.P[:, 2] - self.P[:, 0]
        self.n = np.cross(self.e1, self.e2)
        self.p0n = _dot(self.P[:, 0], self.n)
        self.e1xp0, self.e2xp0 = np.cross(self.e1, self.P[:, 0]), np.cross(self.e2, self.P[:, 0])
        self.normals = None if mesh.get("normals") is None else np.asarray(mesh["normals"], F).astype(np.float64).reshape(-1, 3)
        self.uv = None if mesh.get("texcoords") is None else np.asarray(mesh["texcoords"], F).astype(np.float64).reshape(-1, 2)
        tm = mesh.get("tri_material")
        self.tm = np.zeros(len(self.ix), np.int64) if tm is None else np.asarray(tm, np.int64)

    def mt(self, o, d):
        """Moeller-Trumbore's t, u, v [n, T] of rays [n, 3] as triple products: det = e1 . (d x e2) = -d . n, t = (o - P0) . n / det,
        u = e2 . ((o - P0) x d) / det, v = -e1 . ((o - P0) x d) / det; det = 0 gives no hit"""
        c = np.cross(o, d)
        det = -(d @ self.n.T)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(det != 0, 1.0 / det, np.nan)
            t = (o @ self.n.T - self.p0n[None]) * inv
            u = (c @ self.e2.T - d @ self.e2xp0.T) * inv
            v = -(c @ self.e1.T - d @ self.e1xp0.T) * inv
        return t, u, v


class _Scene:
    def __init__(self, scene):
        self.meshes = [_Mesh(m) for m in scene["meshes"]]
        self.inst = []
        for tr, mi, off in scene["instances"]:
            M = np.asarray(tr, F).astype(np.float64).reshape(-1)[:12].reshape(3, 4)
            inv = np.linalg.inv(np.concatenate([M, [[0.0, 0.0, 0.0, 1.0]]]))
            self.inst.append((M, inv[:3], self.meshes[int(mi)], int(off)))
        self.materials = np.asarray(scene["materials"], F).astype(np.float64).reshape(-1, 6)
        self.textures = scene.get("textures") or {}
        self.lights = np.asarray(scene["lights"], F).astype(np.float64).reshape(-1, 8)
        self.miss = np.asarray(scene["miss"], F).astype(np.float64)

    def to_object(self, k, o, d):
        inv = self.inst[k][1]
        return o @ inv[:, :3].T + inv[:, 3], d @ inv[:, :3].T

    def closest(self, o, d):
        """(hit [n], clear [n], key [n, 2] (instance, triangle), t, u, v [n], bary_err [n]).  bary_err is what float32 can place the
        winner's u and v to: u = (o - P0) . (d x e2) / det is a sum of products of size |o - P0| |d| |e2|, rounded in the cross product (1 to 2
        half-ulps), in the dot product (1 to 2) and in the object-space ray itself (1), over det -- BARY_ULPS 2^-24 |o - P0| |d| max(|e1|, |e2|) / |det|.
        It decides nothing here; local_geometry() turns it into the uncertainty of the interpolated UV."""
        n = len(o)
        bt, second = np.full(n, np.inf), np.full(n, np.inf)
        bu, bv, bm, berr = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        key = np.full((n, 2), -1, np.int64)
        k = np.arange(n)
        for ii in range(len(self.inst)):
            oo, od = self.to_object(ii, o, d)
            t, u, v = self.inst[ii][2].mt(oo, od)
            with np.errstate(invalid="ignore"):
                m = np.minimum(np.minimum(u, v), 1.0 - u - v)
                strict = (m >= 0) & (t > T_MIN) & (t < T_MAX)
                cand = (m >= -BARY_MARGIN) & (t > T_MIN * (1 - T_MARGIN)) & (t < T_MAX)
            ts = np.where(strict, t, np.inf)
            b = np.argmin(ts, axis=1)                  # (the first of equal minima: the lowest triangle)
            tb = ts[k, b]
            tc = np.where(cand, t, np.inf)
            tc[k, b] = np.where(np.isfinite(tb), np.inf, tc[k, b])
            c2 = tc.min(axis=1)
            better = tb < bt                           # (an equal t keeps the lower instance)
            second = np.where(better, np.minimum(np.minimum(bt, second), c2), np.minimum(second, np.minimum(tb, c2)))
            bu, bv, bm = np.where(better, u[k, b], bu), np.where(better, v[k, b], bv), np.where(better, m[k, b], bm)
            mesh = self.inst[ii][2]
            norm = lambda a: np.sqrt(_dot(a, a))
            with np.errstate(divide="ignore", invalid="ignore"):
                err = BARY_ULPS * 2.0 ** -24 * norm(oo - mesh.P[b, 0]) * norm(od) * np.maximum(norm(mesh.e1[b]), norm(mesh.e2[b])) / np.abs(_dot(od, mesh.n[b]))
            berr = np.where(better, err, berr)
            key[better] = np.stack([np.full(n, ii), b], 1)[better]
            bt = np.where(better, tb, bt)
        hit = np.isfinite(bt)
        clear = np.where(hit, (second >= bt * (1 + T_MARGIN)) & (bm >= BARY_MARGIN) & (bt >= T_MIN * (1 + T_MARGIN)), ~np.isfinite(second))
        return hit, clear, key, bt, bu, bv, berr

    def occluded(self, o, d, tmax, chunk=4096):
        """any hit over OCC_EPS < t < tmax: (occluded [n], clear [n])"""
        n = len(o)
        occ, sure, maybe = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
        for a in range(0, n, chunk):
            s = slice(a, a + chunk)
            tm = tmax[s, None]
            for ii in range(len(self.inst)):
                oo, od = self.to_object(ii, o[s], d[s])
                t, u, v = self.inst[ii][2].mt(oo, od)
                with np.errstate(invalid="ignore"):
                    m = np.minimum(np.minimum(u, v), 1.0 - u - v)
                    occ[s] |= ((m >= 0) & (t > OCC_EPS) & (t < tm)).any(axis=1)
                    sure[s] |= ((m >= BARY_MARGIN) & (t >= OCC_EPS * (1 + T_MARGIN)) & (t <= tm * (1 - T_MARGIN))).any(axis=1)
                    maybe[s] |= ((m >= -BARY_MARGIN) & (t >= OCC_EPS * (1 - T_MARGIN)) & (t <= tm * (1 + T_MARGIN))).any(axis=1)
        return occ, sure | ~maybe

    def local_geometry(self, key, u, v, bary_err=None):
        """getLocalGeometry of the hits key [n, 2] with barycentrics u, v: dict of P, N, corners C [n, 3, 3], corner UVs [n, 3, 2], UV,
        material, and UV_err [n, 2]: bary_err (|UV1 - UV0| + |UV2 - UV0|), what float32 can place UV to"""
        n = len(key)
        g = {"P": np.zeros((n, 3)), "N": np.zeros((n, 3)), "C": np.zeros((n, 3, 3)), "CUV": np.zeros((n, 3, 2)), "UV": np.zeros((n, 2)),
             "material": np.zeros(n, np.int64), "UV_err": np.zeros((n, 2))}
        for ii, (M, inv, mesh, off) in enumerate(self.inst):
            r = np.nonzero(key[:, 0] == ii)[0]
            if not len(r):
                continue
            tri = key[r, 1]
            C = mesh.P[tri]
            w0, bu, bv = (1.0 - u[r] - v[r])[:, None], u[r][:, None], v[r][:, None]
            g["P"][r] = (w0 * C[:, 0] + bu * C[:, 1] + bv * C[:, 2]) @ M[:, :3].T + M[:, 3]
            w2o = inv[:, :3]
            N = _normalize(np.cross(C[:, 1] - C[:, 0], C[:, 2] - C[:, 0])) @ w2o          # W2O^T Ng, not renormalised
            if mesh.normals is not None:
                vn = mesh.normals[mesh.ix[tri]]
                N = _normalize((w0 * vn[:, 0] + bu * vn[:, 1] + bv * vn[:, 2]) @ w2o)
            g["N"][r] = N
            if mesh.uv is not None:
                cuv = mesh.uv[mesh.ix[tri]]
                g["CUV"][r] = cuv
                g["UV"][r] = w0 * cuv[:, 0] + bu * cuv[:, 1] + bv * cuv[:, 2]
            else:
                g["CUV"][r] = np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0]])
                g["UV"][r] = np.concatenate([bu, bv], 1)
            g["C"][r] = C
            if bary_err is not None:
                g["UV_err"][r] = bary_err[r][:, None] * (np.abs(g["CUV"][r][:, 1] - g["CUV"][r][:, 0]) + np.abs(g["CUV"][r][:, 2] - g["CUV"][r][:, 0]))
            g["material"][r] = off + mesh.tm[tri]
        return g


# ---- tex2D<float4> ----
def tex2d(tex, u, v, uv_err=None):
    """(rgba [n, 4], clear [n]) of a uint8 [h, w, 4] texture at normalised coordinates u, v [n]; uv_err [n, 2]: what float32 can place
    (u, v) to (the margin is the larger of WEIGHT_MARGIN and that, in weight steps)"""
    tex = np.asarray(tex, np.uint8)
    h, w = tex.shape[:2]
    T = tex.astype(np.float64) / 255.0

    def axis(x, N, err):
        xb = x * N - 0.5
        f = np.floor(xb)
        q = (xb - f) * 256.0
        a = np.floor(q + 0.5) / 256.0
        margin = np.maximum(WEIGHT_MARGIN, err * N * 256.0)
        clear = (np.abs(q - np.floor(q) - 0.5) >= margin) & (np.minimum(q, 256.0 - q) >= margin)
        i0 = np.mod(f.astype(np.int64), N)
        return i0, np.mod(i0 + 1, N), a, clear

    uv_err = np.zeros((len(u), 2)) if uv_err is None else uv_err
    i0, i1, a, cx = axis(np.asarray(u, np.float64), w, uv_err[:, 0])
    j0, j1, b, cy = axis(np.asarray(v, np.float64), h, uv_err[:, 1])
    a, b = a[:, None], b[:, None]
    out = (1 - a) * (1 - b) * T[j0, i0] + a * (1 - b) * T[j0, i1] + (1 - a) * b * T[j1, i0] + a * b * T[j1, i1]
    return out, cx & cy


# ---- __closesthit__radiance ----
def shade(g, rd, materials, textures, lights, occluded=None):
    """the closest-hit program on hits g (local_geometry's dict: P, N, C, CUV, UV [n, ...]) seen along rd [n, 3] (not necessarily unit).
    materials [n, 6] per hit; textures: one (base_color, metallic_roughness, normal) triple for all hits, each uint8 [h, w, 4] or None;
    lights [nl, 8] or [n, nl, 8]; occluded(o, d, tmax) -> (occluded, clear) or None (nothing occludes).  Returns a dict:
    color [n, 3]; clear [n]; kappa [n, 3]; state [n, nl] (GATED, SHADOWED, LIT); state_clear [n, nl]; gate_clear [n, nl] (whether the
    gate alone is decided with a margin: the texture weights behind N, N.L, N.V); terms [n, nl, 3], each light's unoccluded contribution
    (zero where gated); N [n, 3]; roughness, metallic [n]; x [n, nl]"""
    n = len(rd)
    P, N = g["P"], g["N"].copy()
    mats = np.asarray(materials, np.float64).reshape(n, 6)
    base = mats[:, 0:3].copy()
    mr_y, mr_z = np.ones(n), np.ones(n)
    clear = np.ones(n, bool)
    extra = np.zeros(n)
    bc_tex, mr_tex, n_tex = textures if textures is not None else (None, None, None)
    if bc_tex is not None:
        tc, c = tex2d(bc_tex, g["UV"][:, 0], g["UV"][:, 1], g.get("UV_err"))
        base = base * tc[:, :3] ** GAMMA
        clear &= c
    if mr_tex is not None:
        tc, c = tex2d(mr_tex, g["UV"][:, 0], g["UV"][:, 1], g.get("UV_err"))
        mr_y, mr_z = tc[:, 1], tc[:, 2]             # (occlusion, roughness, metallic)
        clear &= c
    if n_tex is not None:
        UV0, UV1, UV2 = g["CUV"][:, 0], g["CUV"][:, 1], g["CUV"][:, 2]
        du1, du2, dv1, dv2 = UV0[:, 0] - UV2[:, 0], UV1[:, 0] - UV2[:, 0], UV0[:, 1] - UV2[:, 1], UV1[:, 1] - UV2[:, 1]
        dp1, dp2 = g["C"][:, 0] - g["C"][:, 2], g["C"][:, 1] - g["C"][:, 2]
        invdet = (1.0 / (du1 * dv2 - dv1 * du2))[:, None]
        dpdu = (dv2[:, None] * dp1 - dv1[:, None] * dp2) * invdet
        dpdv = (-du2[:, None] * dp1 + du1[:, None] * dp2) * invdet
        tc, c = tex2d(n_tex, g["UV"][:, 0], g["UV"][:, 1], g.get("UV_err"))
        NN = 2.0 * tc - 1.0
        blend = NN[:, 0:1] * _normalize(dpdu) + NN[:, 1:2] * _normalize(dpdv) + NN[:, 2:3] * N
        length = np.sqrt(_dot(blend, blend))
        N = blend / length[:, None]
        extra = 1.0 / length
        clear &= c
    metallic, roughness = mats[:, 4] * mr_z, mats[:, 5] * mr_y
    diff_color = base * (1.0 - F0) * (1.0 - metallic)[:, None]
    spec_color = F0 + (base - F0) * metallic[:, None]
    alpha = roughness * roughness
    a2 = alpha * alpha
    lights = np.asarray(lights, np.float64)
    if lights.ndim == 2:
        lights = np.broadcast_to(lights[None], (n,) + lights.shape)
    nl = lights.shape[1]
    V = -_normalize(np.asarray(rd, np.float64))
    NV = _dot(N, V)
    Nlen = np.sqrt(_dot(N, N))
    color, knum = np.zeros((n, 3)), np.zeros((n, 3))
    state, state_clear, gate_clear = np.zeros((n, nl), np.int64), np.ones((n, nl), bool), np.ones((n, nl), bool)
    terms, xs = np.zeros((n, nl, 3)), np.ones((n, nl))
    for l in range(nl):
        toL = lights[:, l, 4:7] - P
        Ld = np.sqrt(_dot(toL, toL))
        L = toL / Ld[:, None]
        H = _normalize(L + V)
        NL, NH, VH = _dot(N, L), _dot(N, H), _dot(V, H)
        gate = (NL > 0) & (NV > 0)
        state_clear[:, l] = gate_clear[:, l] = clear & (np.abs(NL) >= GATE_MARGIN) & (np.abs(NV) >= GATE_MARGIN)
        r = np.nonzero(gate)[0]
        occ = np.zeros(n, bool)
        if occluded is not None and len(r):
            o_r, c_r = occluded(P[r], L[r], Ld[r] - OCC_EPS)
            occ[r] = o_r
            state_clear[r, l] &= c_r
        with np.errstate(divide="ignore", invalid="ignore"):
            Fr = spec_color + (1.0 - spec_color) * ((1.0 - VH) ** 5.0)[:, None]
            g0 = NL * np.sqrt(NV * NV * (1.0 - a2) + a2)
            g1 = NV * np.sqrt(NL * NL * (1.0 - a2) + a2)
            G = 2.0 * NL * NV / (g0 + g1)
            x = NH * NH * (a2 - 1.0) + 1.0
            D = a2 / (PI_F * x * x)
            diff = (1.0 - Fr) * diff_color / PI_F
            spec = Fr * (G * D)[:, None]
            term = lights[:, l, 0:3] * lights[:, l, 3:4] * NL[:, None] * (diff + spec)
            kap = 1.0 + 2.0 / x + extra + Nlen * (2.0 / NL + 1.0 / NV)
        term = np.where(gate[:, None], term, 0.0)
        lit = gate & ~occ
        terms[:, l], xs[:, l] = term, x
        state[:, l] = np.where(lit, LIT, np.where(gate, SHADOWED, GATED))
        color += np.where(lit[:, None], term, 0.0)
        knum += np.where(lit[:, None], term * kap[:, None], 0.0)
    clear &= state_clear.all(axis=1)
    kappa = np.where(color > 0, knum / np.where(color > 0, color, 1.0), 1.0)
    return {"color": color, "clear": clear, "kappa": kappa, "state": state, "state_clear": state_clear, "gate_clear": gate_clear, "terms": terms, "N": N,
            "roughness": roughness, "metallic": metallic, "x": xs}


# ---- the whole pipeline ----
def make_color(c):
    """(byte [..., 3] uint8, exact [..., 3] bool: where the byte is to be compared exactly)"""
    y = np.clip(c, 0.0, 1.0) ** INV_GAMMA * 255.0
    return np.floor(y).astype(np.uint8), np.abs(y - np.round(y)) >= BYTE_MARGIN


def render(scene, W, H, subframes):
    """`scene`: dict(meshes, instances [(3x4 transform, mesh, material_offset)], materials [n, 6], textures {material: triple} or None,
    lights [nl, 8], miss (3,), cam (12,)).  Returns one dict per subframe count 1 .. subframes (the state after that many subframes):
    color [H, W, 3] the running average, byte, byte_exact, clear [H, W] (every subframe so far clear), kappa [H, W, 3]; and of that
    subframe alone: hit [H, W], key [H, W, 2], state [H, W, nl] (MISS on a miss pixel), state_clear, gate_clear [H, W, nl] (the hit or
    miss and the gate of that light are decided with a margin: whether the pixel sends that occlusion ray), terms [H, W, nl, 3]."""
    S = _Scene(scene)
    nl = len(S.lights)
    n = W * H
    out = []
    avg, knum, kden, all_clear = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.ones(n, bool)
    for s in range(subframes):
        o, d = primaries(scene["cam"], W, H, s)
        hit, clear, key, t, u, v, berr = S.closest(o, d)
        color = np.tile(S.miss, (n, 1))
        kappa = np.ones((n, 3))
        state, state_clear = np.full((n, nl), MISS, np.int64), np.ones((n, nl), bool)
        gate_clear = np.tile(clear[:, None], (1, nl))
        terms = np.zeros((n, nl, 3))
        r = np.nonzero(hit)[0]
        g = S.local_geometry(key[r], u[r], v[r], berr[r])
        for mi in np.unique(g["material"]):
            q = np.nonzero(g["material"] == mi)[0]
            gq = {k: a[q] for k, a in g.items()}
            sh = shade(gq, d[r[q]], np.tile(S.materials[mi], (len(q), 1)), S.textures.get(int(mi)), S.lights, S.occluded)
            rows = r[q]
            color[rows], kappa[rows], state[rows], state_clear[rows], terms[rows] = sh["color"], sh["kappa"], sh["state"], sh["state_clear"], sh["terms"]
            gate_clear[rows] &= sh["gate_clear"]
            clear[rows] &= sh["clear"]
        avg = color if s == 0 else avg + (color - avg) * (1.0 / (s + 1))
        knum, kden = knum + color * kappa, kden + color
        all_clear = all_clear & clear
        byte, exact = make_color(avg)
        out.append({"color": avg.reshape(H, W, 3).copy(), "byte": byte.reshape(H, W, 3), "byte_exact": exact.reshape(H, W, 3),
                    "clear": all_clear.reshape(H, W).copy(), "kappa": np.where(kden > 0, knum / np.where(kden > 0, kden, 1.0), 1.0).reshape(H, W, 3),
                    "hit": hit.reshape(H, W), "key": key.reshape(H, W, 2), "state": state.reshape(H, W, nl),
                    "state_clear": state_clear.reshape(H, W, nl), "gate_clear": gate_clear.reshape(H, W, nl), "terms": terms.reshape(H, W, nl, 3)})
    return out


def dev(c32, c64, kappa):
    """|c32 - c64| / (kappa max(|c64|, 1e-3)) in units of 2^-23"""
    c32, c64 = np.asarray(c32, np.float64), np.asarray(c64, np.float64)
    return np.abs(c32 - c64) / (kappa * np.maximum(np.abs(c64), 1e-3)) / UNIT
