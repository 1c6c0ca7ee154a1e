"""The cases tests/test_whitted_shade_rays.py holds rtgo_whitted_shade_rays to, checked from the reference alone (no GPU, no library): the
orthographic views of tests/whitted_shade_rays_ref.py show lit, shadowed and missed rays in the shares the shading tests ask of a scene
(test_oracle_whitted_float64's constants, unchanged), and the host raygen is whitted_ref64's at subframe 0.

Measured on the CPU (lit, shadowed, unclear share of the hits; clear misses): sweep 0.60, 0.07, 0; 0.29.  textured 0.54, 0.14, 0.036; 0.39.
textured_nouv 0.53, 0.14, 0.034; 0.39.  instanced 0.55, 0.10, 0.0085; 0.43."""
import numpy as np
import pytest

import whitted_ref64 as R
import whitted_shading_scenes as S
import whitted_shade_rays_ref as SR
import test_oracle_whitted_float64 as T


@pytest.mark.parametrize("name", ["sweep", "textured", "textured_nouv", "instanced"])
def test_orthographic_case_conditions(name):
    sc, o, d, ref = SR.ortho_case(name)
    lit, shadow, unclear, missed = SR.conditions(ref)
    print("%s: lit %.3f, shadowed %.3f, unclear %.4f of the hit rays, clear misses %.3f" % (name, lit, shadow, unclear, missed))
    assert lit >= T.MIN_LIT and shadow >= T.MIN_SHADOW and unclear <= T.UNCLEAR_CAP[name], (name, lit, shadow, unclear)
    assert missed > 0.02, (name, missed)
    # the rays are what the docstring says: float32, every direction along W, none of unit length, lengths over [1/4, 4]
    assert o.dtype == np.float32 and d.dtype == np.float32 and len(o) == S.W * S.H
    length = np.linalg.norm(d.astype(np.float64), axis=1)
    w = sc["cam"][9:12].astype(np.float64)
    assert np.allclose(d / length[:, None], w / np.linalg.norm(w), atol=1e-6)
    assert length.min() < 0.3 and length.max() > 3.5 and (np.abs(length - 1.0) > 1e-4).all()


@pytest.mark.parametrize("name", ["sweep", "instanced"])
def test_host_raygen_is_the_references(name):
    cam = T.scene(name)["cam"]
    o, d = SR.raygen32(cam, S.W, S.H, 0)
    o0, d0 = R.primaries32(cam, S.W, S.H)
    assert np.array_equal(o.view(np.uint32), o0.view(np.uint32)) and np.array_equal(d.view(np.uint32), d0.view(np.uint32))
    for s in (1, 2):
        o, d = SR.raygen32(cam, S.W, S.H, s)
        _, d64 = R.primaries(cam, S.W, S.H, s)
        assert np.abs(d.astype(np.float64) - d64).max() < 4e-7 and not np.array_equal(d, d0)
