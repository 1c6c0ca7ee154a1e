"""What the tests of rtgo_shade_rays share, numpy only: the launch's raygen in float32 (the rays a caller must hand over to get the
launch's own buffers back), the lat-long camera the launches do not have, and tests/analytic_shading_ref64.py's float64 paths over rays
of the caller's own."""
from unittest import mock

import numpy as np

import analytic_shading_ref64 as S

T_MIN0, T_MAX0 = np.float32(0.05), np.float32(1e16)
F = np.float32


def raygen32(cam, width, height, frame_count):
    """rtgo_start_sample.inc for sqrt_spp 1 in float32, operation for operation (the build contracts nothing, div_cr and sqrt_cr are
    correctly rounded, as numpy's float32 quotient and root are): cam [12] float32 (eye, U, V, W) -> o [h w, 3], d [h w, 3] float32 and
    seed [h w] uint32 as it stands after the two jitter draws, in raster order"""
    cam = np.asarray(cam, F)
    eye, U, V, W = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    py, px = [a.reshape(-1) for a in np.mgrid[0:height, 0:width]]
    seed = S.tea16(width * py + px, np.full(len(px), frame_count))
    seed, k0 = S.lcg(seed)
    seed, k1 = S.lcg(seed)
    r0, r1 = k0.astype(F) / F(16777216.0), k1.astype(F) / F(16777216.0)      # rnd(): (float)(s & 0xFFFFFF) / (float)0x1000000
    inc = F(1.0) / F(1.0)
    dx = F(2.0) * ((px.astype(F) + (F(0.0) + r0) * inc) / F(width)) - F(1.0)
    dy = F(2.0) * ((py.astype(F) + (F(0.0) + r1) * inc) / F(height)) - F(1.0)
    v = (U[None] * dx[:, None] + V[None] * dy[:, None]) + W[None]
    assert v.dtype == F
    inv = F(1.0) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])      # vnormalize: 1 / sqrt(dot), then three products
    d = v * inv[:, None]
    assert d.dtype == F and inv.dtype == F
    return np.broadcast_to(eye, d.shape).copy(), d, seed.astype(np.uint32)


def latlong(cam, width, height, tilt_deg=0.0):
    """a lat-long window about the camera's axis: origin the eye, d = cos p (cos y f + sin y r) + sin p u with f, r, u the unit W, U, V,
    y = (2 (i + 1/2) / width - 1) atan(|U| / |W|), p = (2 (j + 1/2) / height - 1) atan(|V| / |W|) - tilt; computed in float64, rounded to
    float32.  -> o [h w, 3], d [h w, 3] float32, raster order"""
    cam = np.asarray(cam, np.float64)
    eye, U, V, W = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    nU, nV, nW = (np.linalg.norm(a) for a in (U, V, W))
    r, u, f = U / nU, V / nV, W / nW
    j, i = [a.reshape(-1) for a in np.mgrid[0:height, 0:width]]
    y = (2.0 * (i + 0.5) / width - 1.0) * np.arctan(nU / nW)
    p = (2.0 * (j + 0.5) / height - 1.0) * np.arctan(nV / nW) - np.radians(tilt_deg)
    d = np.cos(p)[:, None] * (np.cos(y)[:, None] * f + np.sin(y)[:, None] * r) + np.sin(p)[:, None] * u
    d = d.astype(F)
    return np.broadcast_to(eye.astype(F), d.shape).copy(), d


def index_seeds(n, sample_index):
    """tea<16>(i, sample_index): what rtgo_shade_rays gives ray i when no seeds are handed over"""
    return S.tea16(np.arange(n), np.full(n, sample_index)).astype(np.uint32)


def render_rays(scene, frame, o, d, seed, prev=None):
    """S.render over rays of the caller's own: o, d [h w, 3], seed [h w] stand in for the module's primary rays (one sample per result:
    frame["sqrt_spp"] must be 1) for the call's duration.  render writes into the arrays it is given: it gets fresh float64 copies"""
    assert frame["sqrt_spp"] == 1 and len(o) == frame["width"] * frame["height"]
    P = len(o)

    def rays(cam, width, height, px, py, n, frame_count):
        return (np.array(o, np.float64).reshape(P, 1, 3), np.array(d, np.float64).reshape(P, 1, 3), np.array(seed, np.uint32).reshape(P, 1))

    with mock.patch.object(S, "primary_rays", rays):
        return S.render(scene, frame, prev)
