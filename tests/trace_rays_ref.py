"""Rays and CPU references for the ray-query tests (rtgo_trace_rays, rtgo_whitted_trace_rays).

Analytic path: the reference is oracle_intersect over ALL primitives with the acceptance rule of include/rtgo.h (tmin < t < tmax, ties to
the lowest SBT index).  A ray is UNCLEAR when that reference itself is not stable: its runner-up lies within 1e-4 max(1, t) of its
winner, or its winner (or miss) changes when one direction component moves by +-1e-5.
Triangle path: the clear-ray rule of tests/test_oracle_whitted_instances.py -- a float64 brute force whose runner-up is at least 1e-5
relative further and whose barycentrics are at least 1e-5 inside the triangle."""
import ctypes as C

import numpy as np

import whitted_instances as WI

F = np.float32


def primaries(cam, W, H, step=1):
    """the rays through the centres of the pixels of a W x H image (every step-th pixel in raster order):
    dir = normalize((2 (x + .5) / W - 1) U + (2 (y + .5) / H - 1) V + W), float32 throughout.  Returns origins [n, 3], dirs [n, 3]."""
    cam = np.asarray(cam, F)
    eye, U, V, Wv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    x, y = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    fx = F(2) * (x + F(0.5)) / F(W) - F(1)
    fy = F(2) * (y + F(0.5)) / F(H) - F(1)
    d = (U * fx[..., None] + V * fy[..., None]) + Wv
    d = d / np.sqrt((d * d).sum(-1, keepdims=True, dtype=F))
    d = d.reshape(-1, 3)[::step].astype(F)
    return np.tile(eye, (len(d), 1)), d


def random_rays(lo, hi, n, seed=7):
    """n rays with a uniform origin in the box [lo, hi] and a uniform direction"""
    rng = np.random.RandomState(seed)
    o = (np.asarray(lo, np.float64) + rng.rand(n, 3) * (np.asarray(hi, np.float64) - np.asarray(lo, np.float64))).astype(F)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    return o, d


def scene_rays(tables, W=32, H=24, n_random=768, step=1):
    aabb = np.asarray(tables["aabb"], F)
    o1, d1 = primaries(tables["cam"], W, H, step)
    o2, d2 = random_rays(aabb[:, :3].min(0), aabb[:, 3:].max(0), n_random)
    return np.concatenate([o1, o2]), np.concatenate([d1, d2])


def brute(oracle, sc, o, d, tmin, tmax):
    """oracle_intersect over every primitive of the oracle Scene `sc` for one ray: (prim, t, n[3], runner-up t) under the acceptance rule;
    prim -1 and t = tmax on a miss; runner-up inf when there is none"""
    L = oracle.lib()
    o, d = oracle.f32(o), oracle.f32(d)
    po, pd = oracle.fptr(o), oracle.fptr(d)
    t, n = C.c_float(0), (C.c_float * 3)()
    best, bt, bn, second = -1, F(tmax), (0.0, 0.0, 0.0), np.inf
    for i in range(sc.n_prims):
        if not L.oracle_intersect(C.byref(sc.prims[i]), po, pd, C.byref(t), n):
            continue
        tv = F(t.value)
        if not (tv > F(tmin) and tv < F(tmax)):
            continue
        if best < 0 or tv < bt:    # (ascending i: an equal t keeps the lower index)
            if best >= 0:
                second = min(second, float(bt))
            best, bt, bn = i, tv, (n[0], n[1], n[2])
        else:
            second = min(second, float(tv))
    return best, bt, np.array(bn, F), second


def reference(oracle, sc, o, d, tmin=1e-3, tmax=1e16):
    """brute() for every ray, and which rays are unclear.  Returns dict(prim [n], t [n], n [n, 3], unclear [n] bool)"""
    m = len(o)
    prim, t, nn, unclear = np.zeros(m, np.int32), np.zeros(m, F), np.zeros((m, 3), F), np.zeros(m, bool)
    for k in range(m):
        p, tv, nv, second = brute(oracle, sc, o[k], d[k], tmin, tmax)
        prim[k], t[k], nn[k] = p, tv, nv
        if p >= 0 and second - float(tv) <= 1e-4 * max(1.0, float(tv)):
            unclear[k] = True
            continue
        for axis in range(3):
            for s in (-1e-5, 1e-5):
                dd = d[k].copy()
                dd[axis] = F(dd[axis] + F(s))
                if brute(oracle, sc, o[k], dd, tmin, tmax)[0] != p:
                    unclear[k] = True
                    break
            if unclear[k]:
                break
    return {"prim": prim, "t": t, "n": nn, "unclear": unclear}


def rel_dev(a, b):
    """largest |a - b| / max(1, |b|) (float64)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) if a.size else 0.0


# ---- triangle path ----
def _mt64(P, o, d):
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    pv = np.cross(d[:, None, :], e2[None])
    det = (e1[None] * pv).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(det != 0, 1.0 / det, np.nan)
        tv = o[:, None, :] - P[None, :, 0]
        u = (tv * pv).sum(-1) * inv
        qv = np.cross(tv, e1[None])
        v = (d[:, None, :] * qv).sum(-1) * inv
        t = (e2[None] * qv).sum(-1) * inv
    return t, u, v


def clear_triangle_rays(meshes, inst, o, d, tmin=0.01):
    """float64 brute force over every (instance, triangle): (hit [n] bool, clear [n] bool, key [n, 2] = the float64 winner's (instance,
    triangle)) -- clear: it hits, the runner-up is at least 1e-5 relative further and the barycentrics are at least 1e-5 inside"""
    n = len(o)
    o64, d64 = np.asarray(o, np.float64), np.asarray(d, np.float64)
    tb = np.full(n, np.inf)
    t2 = np.full(n, np.inf)
    mb = np.zeros(n)
    key = np.full((n, 2), -1, np.int64)
    for ii, (tr, mi, _) in enumerate(inst):
        M = WI.as34(np.asarray(tr, np.float32))
        Binv = np.linalg.inv(M[:, :3])
        oo = (o64 - M[:, 3]) @ Binv.T
        od = d64 @ Binv.T
        mesh = meshes[mi]
        P = np.asarray(mesh["positions"], np.float64)[np.asarray(mesh["indices"], np.int64)]
        # only the rays whose line comes within the mesh's bounding sphere (object space, a little grown) can hit it
        c = 0.5 * (P.reshape(-1, 3).min(0) + P.reshape(-1, 3).max(0))
        rad = np.linalg.norm(P.reshape(-1, 3) - c, axis=1).max() * 1.001 + 1e-9
        near = np.linalg.norm(np.cross(c - oo, od), axis=1) <= rad * np.linalg.norm(od, axis=1)
        rows = np.nonzero(near)[0]
        if not len(rows):
            continue
        t, u, v = _mt64(P, oo[rows], od[rows])
        ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tmin)
        t = np.where(ok, t, np.inf)
        margin = np.minimum(np.minimum(u, v), 1 - u - v)
        k = np.arange(len(rows))
        b = np.argmin(t, axis=1)           # (the first of equal minima: the lowest triangle)
        t_first = t[k, b]
        t[k, b] = np.inf
        t_second = t.min(axis=1) if t.shape[1] > 1 else np.full(len(rows), np.inf)
        better = t_first < tb[rows]
        t2[rows] = np.where(better, np.minimum(tb[rows], t_second), np.minimum(t2[rows], t_first))
        mb[rows] = np.where(better, margin[k, b], mb[rows])
        key[rows[better]] = np.stack([np.full(len(rows), ii), b], 1)[better]
        tb[rows] = np.where(better, t_first, tb[rows])
    hit = np.isfinite(tb)
    clear = hit & (t2 >= tb * (1 + 1e-5)) & (mb >= 1e-5)
    return hit, clear, key
