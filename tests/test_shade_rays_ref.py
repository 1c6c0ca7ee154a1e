"""The references tests/test_shade_rays.py holds rtgo_shade_rays to, checked without a GPU (tests/shade_rays_ref.py): the float32 raygen
gives the oracle's depth-0 rays and seeds bit for bit, the float64 paths over caller-supplied rays are S.render's own when the rays are
S.render's own, and the lat-long rays of the test meet, in the reference alone, every condition T.check_frame puts on a reference."""
import numpy as np
import pytest

import analytic_shading_ref64 as S
import shade_rays_ref as R
import shading_scenes as SC
import test_oracle_shading_float64 as T

W, H = T.W48, T.H36
TILT = {"room": 10.0, "two_lights": 0.0, "quadrics": 0.0}      # room without the tilt: shadowed 0.091, under check_frame's floor of 0.10
# the reference's own figures over these rays, every mode and every depth of T.DEPTHS: (unclear at most, two-hit share at least, lit at
# least, shadowed at least)
LATLONG_FIGURES = {"room": (0.013, 0.78, 0.82, 0.18), "two_lights": (0.006, 0.72, 0.73, 0.195), "quadrics": (0.018, 0.87, 0.82, 0.178)}
_latlong = {}


def latlong_reference(name, mode, md):
    """(scene tables, S.render's result, o, d, seeds) of the lat-long window of scene `name`; computed once and shared with the GPU test"""
    key = (name, mode, md)
    if key not in _latlong:
        t = SC.SCENES[name](W / H)
        o, d = R.latlong(t["cam"], W, H, TILT[name])
        seed = R.index_seeds(W * H, 0)
        r = R.render_rays(t, T.frame_of(W, H, 1, md, 0, mode), o, d, seed)
        r["paths_unclear"] = int((~r["clear_paths"]).sum())
        _latlong[key] = (t, r, o, d, seed)
    return _latlong[key]


@pytest.mark.parametrize("fc", [0, 3])
@pytest.mark.parametrize("name", list(SC.SCENES))
def test_raygen32_is_the_oracle_s_raygen(oracle, name, fc):
    t = SC.SCENES[name](W / H)
    o, d, seed = R.raygen32(t["cam"], W, H, fc)
    log, pixel, _, _ = oracle.log_launch(T.scene_of(oracle, t), oracle.frame(W, H, 1, fc, path=True, mode=1, max_depth=0))
    first = log[(log["parent"] < 0) & (log["depth"] == 0) & (log["kind"] == S.RADIANCE)]
    assert len(first) == W * H and np.array_equal(pixel[(log["parent"] < 0)], np.arange(W * H))
    assert first["o"].tobytes() == o.tobytes()
    assert first["d"].tobytes() == d.tobytes(), np.nonzero((first["d"] != d).any(1))[0][:10]
    assert np.array_equal(first["seed"], seed)
    assert (first["tmin"] == R.T_MIN0).all() and (first["tmax"] == R.T_MAX0).all()


@pytest.mark.parametrize("mode", list(T.MODES))
def test_render_rays_is_render(mode):
    """handed S.primary_rays' own rays, render_rays is S.render to the bit, and neither the module nor the arrays handed over are changed;
    handed raygen32's -- the same rays rounded to float32 -- it stays within the float32 pipeline's own bound on the pixels clear in both"""
    name, md = "room", 3
    t, ref = T.reference(name, mode, md, 1)
    fr = T.frame_of(W, H, 1, md, 0, mode)
    py, px = [a.reshape(-1) for a in np.mgrid[0:H, 0:W]]
    original = S.primary_rays
    o, d, seed = S.primary_rays(t["cam"], W, H, px, py, 1, 0)
    o, d, seed = o[:, 0], d[:, 0], seed[:, 0]
    keep = (o.copy(), d.copy(), seed.copy())
    r = R.render_rays(t, fr, o, d, seed)
    assert S.primary_rays is original
    assert all(np.array_equal(a, b) for a, b in zip(keep, (o, d, seed)))
    assert r["accum"].tobytes() == ref["accum"].tobytes() and np.array_equal(r["clear"], ref["clear"]) and r["chain"] == ref["chain"]
    o32, d32, seed32 = R.raygen32(t["cam"], W, H, 0)
    assert np.array_equal(seed32, seed)
    r32 = R.render_rays(t, fr, o32, d32, seed32)
    both = r32["clear"] & ref["clear"]
    assert both.mean() >= 0.9
    dev = (np.abs(r32["accum"] - ref["accum"]) / (ref["kappa"][..., None] * np.maximum(np.abs(ref["accum"]), 1e-3))).max(-1) / S.UNIT
    print("render_rays over float32 primaries,", mode, "largest dev %.2f units" % dev[both].max())
    assert dev[both].max() <= T.DEV_BOUND[(name, mode)]


@pytest.mark.parametrize("name", list(SC.SCENES))
def test_latlong_rays_meet_the_reference_s_own_conditions(name):
    t = SC.SCENES[name](W / H)
    o, d = R.latlong(t["cam"], W, H, TILT[name])
    d64 = d.astype(np.float64)
    assert np.abs((d64 * d64).sum(1) - 1.0).max() <= 1.1e-7
    assert (o == t["cam"][0:3]).all()
    unclear_most, two_least, lit_least, shadowed_least = LATLONG_FIGURES[name]
    for mode in T.MODES:
        for md in T.DEPTHS[name]:
            _, r, _, _, _ = latlong_reference(name, mode, md)
            clear, hit = r["clear"], (r["hits"] > 0).any(-1)
            unclear = (~clear & hit).sum() / max(hit.sum(), 1)
            two = (clear & (r["hits"] >= 2).all(-1)).mean()
            lit, shadowed = r["lit"].mean(), r["shadowed"].mean()
            print(name, mode, md, "unclear %.4f two-hit %.3f lit %.3f shadowed %.3f" % (unclear, two, lit, shadowed))
            # check_frame's own conditions, exactly ...
            assert unclear <= T.UNCLEAR_CAP[name] and two >= 0.40
            if mode != "path":
                assert lit >= 0.30 and shadowed >= 0.10
            # ... and the figures as recorded, which are rounded to the digits shown (room's two-hit share is 0.7795 under ambient light)
            assert unclear <= unclear_most
            assert two >= two_least - 5e-3
            if mode != "path":
                assert lit >= lit_least - 5e-3 and shadowed >= shadowed_least - 5e-3
