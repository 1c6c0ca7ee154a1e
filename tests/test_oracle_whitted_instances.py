"""The instanced oracle (oracle_whitted_render_instanced / oracle_whitted_trace_instanced, oracle/rtgo_oracle_whitted.c) on the CPU:
against the single-mesh oracle where an instanced scene is exactly a flat one, against the flattened scene where it is approximately
one, against a float64 restatement of the hits, and against its committed fixture."""
import os

import numpy as np
import pytest

import whitted_instances as WI
import whitted_scene
from parity import compare

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bitwise(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), what + ": accumulation differs"
    assert np.array_equal(a[1], b[1]), what + ": image differs"
    assert a[2] == b[2], what + ": ray counts differ %r %r" % (a[2], b[2])


def _near(acc, img, racc, rimg, what):
    """the thresholds the GPU tests hold the kernel to against the flattened oracle"""
    a, r = acc[..., :3].astype(np.float64), racc[..., :3].astype(np.float64)
    within = (np.abs(a - r) <= 1e-3 * np.maximum(1.0, np.abs(r))).all(axis=-1).mean()
    same8 = (img[..., :3] == rimg[..., :3]).all(axis=-1).mean()
    print(what, "within 1e-3: %.4f, 8-bit identical: %.4f" % (within, same8), compare(acc, racc))
    assert within >= 0.99 and same8 >= 0.99, (what, within, same8)


def test_identity_instances_are_bitwise_the_flat_oracle(oracle):
    """whitted_scene.build()'s sphere, box and ground as three identity instances: accumulation, image and ray counts are bitwise the
    flat oracle's, with the box cull on and off"""
    W, H = 96, 64
    mesh = whitted_scene.build()
    cam = whitted_scene.camera(oracle, W, H)
    ref = oracle.whitted_render(mesh, cam, W, H, 2)
    meshes, inst = WI.split_scene(mesh)
    for cull in (True, False):
        _bitwise(oracle.whitted_render_instanced(meshes, inst, mesh["materials"], mesh, cam, W, H, 2, cull=cull), ref, "identity, cull %s" % cull)
    assert ref[2]["rays_occlusion"] > 0


def test_half_turn_waterbottle_is_bitwise_the_flat_oracle(oracle):
    """the WaterBottle un-rotated exactly and instanced under diag(-1, 1, -1), with its base-colour and metallic-roughness textures:
    Moeller-Trumbore and the shading arithmetic are exact under the sign flip, so the frame is bitwise the flat oracle's"""
    W, H = 80, 60
    wb = whitted_scene.waterbottle()
    flip = np.array([-1, 1, -1], np.float32)
    obj = dict(wb, positions=wb["positions"] * flip, normals=wb["normals"] * flip)
    half_turn = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 0]], np.float32)
    bc, mr, _ = wb["textures"][0]
    wb = dict(wb, textures={0: (bc, mr, None)})
    cam = whitted_scene.camera(oracle, W, H, eye=(0.12, 0.08, 0.42), lookat=(0.0, 0.0, 0.0), fov=40.0)
    ref = oracle.whitted_render(wb, cam, W, H, 2)
    got = oracle.whitted_render_instanced([obj], [(half_turn, 0, 0)], wb["materials"], wb, cam, W, H, 2)
    _bitwise(got, ref, "half-turn WaterBottle")
    assert (ref[0][..., :3] != wb["miss"]).any(axis=-1).mean() > 0.1


def test_rigid_and_scaled_tori_agree_with_the_flattened_scene(oracle):
    """the 21-instance scene of the GPU test (rotated, uniformly and non-uniformly scaled tori with vertex normals): the two formulations
    -- object-space intersection through the rounded W2O, and world-space triangles rounded from float64 -- agree"""
    W, H = 96, 64
    meshes, inst = WI.tori_scene()
    mats, extra = WI.materials(), WI.lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.5, 4.0, 6.0), lookat=(0.0, 0.4, -0.5))
    acc, img, rc = oracle.whitted_render_instanced(meshes, inst, mats, extra, cam, W, H, 2)
    racc, rimg, rr = oracle.whitted_render(dict(WI.flatten(meshes, inst), materials=mats, **extra), cam, W, H, 2)
    _near(acc, img, racc, rimg, "tori")
    assert abs(rc["rays_total"] - rr["rays_total"]) <= 0.01 * rr["rays_total"]


@pytest.mark.parametrize("smooth", [True, False], ids=["smooth", "faceted"])
def test_mirrored_instances_agree_with_the_flattened_scene(oracle, smooth):
    """rigid transforms with det = -1.  With vertex normals the flattened scene is the same scene.  Without them N = W2O^T Ng points
    opposite to the flattened triangle's own normal: the flattened scene agrees once its winding is swapped (and not before: then the
    mirrored octahedra are lit from the wrong side)"""
    W, H = 96, 64
    meshes, inst = WI.mirrored_scene(smooth)
    mats, extra = WI.materials(), WI.lights()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.3, 3.5, 5.5), lookat=(0.0, 0.5, -0.3))
    acc, img, rc = oracle.whitted_render_instanced(meshes, inst, mats, extra, cam, W, H, 2)
    assert all(np.linalg.det(WI.as34(tr)[:, :3]) < 0 for tr, m, _ in inst if m == 0)
    flat_meshes = meshes if smooth else [WI.swap_winding(meshes[0]), meshes[1]]
    racc, rimg, rr = oracle.whitted_render(dict(WI.flatten(flat_meshes, inst), materials=mats, **extra), cam, W, H, 2)
    _near(acc, img, racc, rimg, "mirrored " + ("smooth" if smooth else "faceted"))
    assert abs(rc["rays_total"] - rr["rays_total"]) <= 0.01 * rr["rays_total"]
    if not smooth:
        wacc, _, _ = oracle.whitted_render(dict(WI.flatten(meshes, inst), materials=mats, **extra), cam, W, H, 2)
        assert (np.abs(wacc - acc)[..., :3] > 1e-2).any(axis=-1).mean() > 0.02


def test_the_box_cull_changes_nothing(oracle):
    """the per-instance box cull only skips instances the triangle test cannot hit: cull on and off give bitwise one frame, on scaled,
    mirrored and many-instance scenes"""
    W, H = 48, 32
    mats, extra = WI.materials(), WI.lights()
    for name, (meshes, inst) in (("small", WI.small_scene()), ("tori", WI.tori_scene()), ("octahedra", WI.octahedra_scene(511))):
        cam = whitted_scene.camera(oracle, W, H, eye=(0.4, 3.0, 4.5), lookat=(0.0, 0.4, -0.5))
        on = oracle.whitted_render_instanced(meshes, inst, mats, extra, cam, W, H, 2, cull=True)
        off = oracle.whitted_render_instanced(meshes, inst, mats, extra, cam, W, H, 2, cull=False)
        _bitwise(on, off, name)


def _primary_rays(cam, W, H):
    """subframe 0's primary rays as the oracle makes them (no jitter), as float32: eye, directions [H, W, 3]"""
    f = np.float32
    eye, U, V, Wv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    x, y = np.meshgrid(np.arange(W, dtype=f), np.arange(H, dtype=f))
    dx = f(2) * (x / f(W)) - f(1)
    dy = f(2) * (y / f(H)) - f(1)
    d = (U * dx[..., None] + V * dy[..., None]) + Wv
    d = (d / np.sqrt((d.astype(np.float64) ** 2).sum(-1, keepdims=True))).astype(f)
    return eye.astype(f), d


def _mt64(P, o, d):
    """float64 Moeller-Trumbore of rays o + t d [n, 3] against triangles P [m, 3, 3]: t, u, v [n, m] (nan where the plane is parallel)"""
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


def test_hits_against_a_float64_reference(oracle):
    """a float64 restatement of the hits -- world rays, the transform's inverse (numpy), object-space Moeller-Trumbore, brute-force
    closest hit -- on rotated, scaled and mirrored tori and octahedra: on every pixel where the float64 answer is clear (runner-up at least
    1e-5 relative further, barycentrics at least 1e-5 inside the triangle) oracle_whitted_trace_instanced hits the same (instance,
    triangle), and its world P agrees within 1e-5 relative; such pixels are at least 90 % of the pixels that hit"""
    W, H = 48, 32
    meshes, inst = WI.small_scene()
    cam = whitted_scene.camera(oracle, W, H, eye=(0.4, 2.4, 3.6), lookat=(0.0, 0.5, -0.2))
    sc = oracle.InstancedScene(meshes, inst, WI.materials(), WI.lights(), cam)
    eye, d32 = _primary_rays(cam, W, H)
    d = d32.reshape(-1, 3).astype(np.float64)
    n = len(d)
    # every (instance, triangle) hit in float64, in object space
    cand = []   # (t [n, m], inside margin [n, m], instance, local triangle index)
    for ii, (tr, mi, _) in enumerate(inst):
        M = WI.as34(np.asarray(tr, np.float32))
        Binv = np.linalg.inv(M[:, :3])
        oo = (Binv @ (eye.astype(np.float64) - M[:, 3]))[None].repeat(n, 0)
        od = d @ Binv.T
        mesh = meshes[mi]
        P = np.asarray(mesh["positions"], np.float64)[np.asarray(mesh["indices"], np.int64)]
        t, u, v = _mt64(P, oo, od)
        ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0.01)
        t = np.where(ok, t, np.inf)
        margin = np.minimum(np.minimum(u, v), 1 - u - v)
        cand.append((t, margin, ii))
    t_all = np.concatenate([c[0] for c in cand], axis=1)
    m_all = np.concatenate([c[1] for c in cand], axis=1)
    key = np.concatenate([np.stack([np.full(c[0].shape[1], c[2]), np.arange(c[0].shape[1])], 1) for c in cand])
    order = np.argsort(t_all, axis=1, kind="stable")
    best, second = order[:, 0], order[:, 1]
    rows = np.arange(n)
    tb, t2 = t_all[rows, best], t_all[rows, second]
    hit = np.isfinite(tb)
    clear = hit & (t2 >= tb * (1 + 1e-5)) & (m_all[rows, best] >= 1e-5)
    assert hit.sum() > 0.5 * n
    assert clear.sum() >= 0.9 * hit.sum(), (clear.sum(), hit.sum())
    P64 = eye.astype(np.float64) + tb[:, None] * d
    checked = 0
    for k in np.nonzero(clear)[0]:
        got = sc.trace(eye, d32.reshape(-1, 3)[k])
        assert got is not None, ("pixel", k, "float64 hits", key[best[k]])
        ii, tri, t, u, v = got
        assert (ii, tri) == tuple(key[best[k]]), ("pixel", k, got, key[best[k]])
        tr, mi, _ = inst[ii]
        M = WI.as34(np.asarray(tr, np.float32))
        c = np.asarray(meshes[mi]["positions"], np.float32)[np.asarray(meshes[mi]["indices"])[tri]]
        f = np.float32
        Pobj = (c[0] * (f(1) - f(u) - f(v)) + c[1] * f(u)) + c[2] * f(v)
        Pw = M[:, :3] @ Pobj.astype(np.float64) + M[:, 3]
        assert np.abs(Pw - P64[k]).max() <= 1e-5 * max(1.0, np.abs(P64[k]).max()), ("pixel", k, Pw, P64[k])
        checked += 1
    # and where float64 sees nothing at all, nor does the oracle
    for k in np.nonzero(~hit)[0][:200]:
        assert sc.trace(eye, d32.reshape(-1, 3)[k]) is None, ("pixel", k)
    print("float64 reference: %d pixels hit, %d clear and checked" % (hit.sum(), checked))


def test_committed_instanced_render_reproduces_bitwise(oracle):
    """tests/golden/oracle_whitted_instances.npz (oracle/gen_golden.py): the instanced oracle reproduces its own committed frame"""
    import gen_golden
    z = np.load(os.path.join(GOLD, "oracle_whitted_instances.npz"))
    meshes, inst, mats, extra = gen_golden.whitted_instances_scene(z)
    W, H = int(z["size"][0]), int(z["size"][1])
    acc, img, rc = oracle.whitted_render_instanced(meshes, inst, mats, extra, z["cam"], W, H, int(z["subframes"]), threads=1)
    assert np.array_equal(acc.view(np.uint32), z["accum"].view(np.uint32))
    assert np.array_equal(img, z["image"])
    assert [rc["rays_total"], rc["rays_occlusion"]] == z["rays"].tolist()
    acc4, _, _ = oracle.whitted_render_instanced(meshes, inst, mats, extra, z["cam"], W, H, int(z["subframes"]), threads=4)
    assert np.array_equal(acc4.view(np.uint32), z["accum"].view(np.uint32))
