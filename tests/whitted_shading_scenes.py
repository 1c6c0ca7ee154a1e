"""The three scenes of the shading tests (test_oracle_whitted_float64.py on the CPU, test_whitted_shading_float64.py on the device), and
the forms the oracle, the C ABI and tests/whitted_ref64.py take them in.  Numpy only.

A scene is a dict: meshes (mesh dicts: positions, normals or None, texcoords or None, indices, tri_material or None), instances
[(3x4 transform, mesh, material_offset)], materials [n, 6], textures {material: (base_color, metallic_roughness, normal)} or None,
lights [nl, 8], miss (3,), cam (12,) = eye, U, V, W."""
import numpy as np

import whitted_instances as WI

W, H, SUBFRAMES = 64, 48, 3
EYE34 = np.eye(3, 4, dtype=np.float32)


def camera(eye, lookat, fov, aspect, up=(0.0, 1.0, 0.0)):
    """a pinhole camera's eye, U, V, W (12 floats): W towards lookat, |V| = |W| tan(fov / 2), |U| = |V| aspect"""
    eye, lookat, up = (np.asarray(a, np.float64) for a in (eye, lookat, up))
    Wv = lookat - eye
    U = np.cross(Wv, up)
    U /= np.linalg.norm(U)
    V = np.cross(U, Wv)
    V /= np.linalg.norm(V)
    vlen = np.linalg.norm(Wv) * np.tan(0.5 * np.radians(fov))
    return np.concatenate([eye, U * vlen * aspect, V * vlen, Wv]).astype(np.float32)


def _lights(rows):
    ls = np.zeros((len(rows), 8), np.float32)
    for k, (color, intensity, position) in enumerate(rows):
        ls[k, 0:3], ls[k, 3], ls[k, 4:7] = color, intensity, position
    return ls


def _grid(nx, nz, x0, x1, z0, z1, y=0.0):
    """(nx + 1)(nz + 1) vertices of a grid of nx x nz quads in the plane y, facing +y, two triangles per quad; quad q = iz nx + ix"""
    xs, zs = np.linspace(x0, x1, nx + 1), np.linspace(z0, z1, nz + 1)
    X, Z = np.meshgrid(xs, zs)
    pos = np.stack([X, np.full_like(X, y), Z], -1).reshape(-1, 3)
    tris, quad = [], []
    for iz in range(nz):
        for ix in range(nx):
            a, b, c, d = iz * (nx + 1) + ix, iz * (nx + 1) + ix + 1, (iz + 1) * (nx + 1) + ix + 1, (iz + 1) * (nx + 1) + ix
            tris += [(a, c, b), (a, d, c)]
            quad += [iz * nx + ix] * 2
    return pos, np.array(tris, np.uint32), np.array(quad, np.uint32)


def _hash01(k, salt):
    """a fixed pseudo-random number in [0, 1) per integer"""
    x = (np.asarray(k, np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15) & np.uint64(0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(29)
    x = x * np.uint64(0xBF58476D1CE4E5B9) & np.uint64(0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(32)
    return (x & np.uint64(0xFFFFFF)).astype(np.float64) / float(1 << 24)


def material_table(n=192):
    """metallic 0 / 1/2 / 1 in turn, roughness on a log ladder from 0.05 to 1 over the table, hashed base colours"""
    k = np.arange(n)
    rough = 0.05 * (1.0 / 0.05) ** ((k // 3) / (n // 3 - 1.0))
    mats = np.zeros((n, 6), np.float32)
    for c in range(3):
        mats[:, c] = 0.15 + 0.8 * _hash01(k, 101 + c)
    mats[:, 3] = 1.0
    mats[:, 4] = (k % 3) * 0.5
    mats[:, 5] = rough
    return mats


def _blockers(tris, n_materials):
    """floating triangles (their own vertices, normals along their geometric normal, the table's first materials)"""
    pos = np.array(tris, np.float64).reshape(-1, 3)
    nrm = np.repeat([np.cross(t[1] - t[0], t[2] - t[0]) for t in np.array(tris, np.float64)], 3, axis=0)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return pos, nrm, np.arange(len(pos), dtype=np.uint32).reshape(-1, 3), (np.arange(len(tris)) % n_materials).astype(np.uint32)


def sweep():
    """a 16 x 12 grid of quads (384 triangles) seen at 20 to 80 degrees from its normal, each quad its own material of material_table(),
    vertex normals tilted by a smooth bump field of up to 20 degrees, three point lights -- one 0.3 above the plane, one far, one BELOW
    the plane (gated: it contributes nothing) -- two floating blocker triangles, a third just in front of the far light (inside the last
    0.001 of every occlusion ray to it), and the miss colour above the horizon"""
    pos, tris, quad = _grid(16, 12, -4.0, 4.0, -3.5, 2.5)
    x, z = pos[:, 0], pos[:, 2]
    nrm = np.stack([0.25 * np.sin(1.3 * x + 0.4) * np.cos(0.9 * z), np.ones_like(x), 0.25 * np.cos(1.1 * x) * np.sin(1.7 * z + 0.2)], -1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    far = np.array([5.0, 9.0, 3.0])
    # a small triangle 0.0004 in front of the far light, across every ray from the plane to it: those rays meet it between the occlusion
    # window's end, L_dist - 0.001, and the light, so it shadows nothing (a window that ends at L_dist makes it shadow the whole plane)
    axis = (far - np.array([0.0, 0.0, -0.5])) / np.linalg.norm(far - np.array([0.0, 0.0, -0.5]))
    t1 = np.cross(axis, [0.0, 0.0, 1.0]) / np.linalg.norm(np.cross(axis, [0.0, 0.0, 1.0]))
    t2 = np.cross(axis, t1)
    c = far - 0.0004 * axis
    cap = [tuple(c + 0.03 * t1), tuple(c - 0.015 * t1 + 0.026 * t2), tuple(c - 0.015 * t1 - 0.026 * t2)]
    bp, bn, bi, bm = _blockers([[(-2.6, 0.9, -1.4), (-0.2, 1.3, -2.2), (-1.2, 1.1, 0.4)], [(0.6, 0.5, -0.3), (2.9, 0.8, -1.0), (1.9, 0.7, 1.2)], cap], 192)
    mesh = {"positions": np.concatenate([pos, bp]).astype(np.float32), "normals": np.concatenate([nrm, bn]).astype(np.float32), "texcoords": None,
            "indices": np.concatenate([tris, bi + np.uint32(len(pos))]), "tri_material": np.concatenate([quad, bm + np.uint32(40)])}
    lights = _lights([((1.0, 0.9, 0.8), 0.9, (-1.1, 0.3, 0.7)), ((0.8, 0.9, 1.0), 1.6, tuple(far)), ((1.0, 1.0, 1.0), 5.0, (1.0, -2.0, 0.0))])
    return {"meshes": [mesh], "instances": [(EYE34, 0, 0)], "materials": material_table(), "textures": None, "lights": lights,
            "miss": np.array([0.12, 0.17, 0.3], np.float32), "cam": camera((0.3, 2.0, 2.0), (0.0, 0.0, -1.2), 60.0, W / H)}


def normal_map(rng, h, w):
    t = np.zeros((h, w, 4), np.uint8)
    t[..., 0:2] = rng.randint(40, 216, (h, w, 2))
    t[..., 2] = rng.randint(192, 256, (h, w))       # z = 2 t - 1 >= 0.5
    t[..., 3] = 255
    return t


def textured(texcoords=True):
    """8 x 6 quads with all three textures, 7 x 5 and 16 x 16 texels, on two materials and only two of them on a third; per-vertex UVs
    from -1.3 to 2.6 (both wraps), or none (UV = the barycentrics); no vertex normals (N = Ng); two lights and a blocker"""
    rng = np.random.RandomState(12)
    pos, tris, quad = _grid(8, 6, -3.0, 3.0, -3.0, 1.5)
    uv = np.stack([-1.3 + 3.9 * (pos[:, 0] + 3.0) / 6.0, -1.3 + 3.9 * (pos[:, 2] + 3.0) / 4.5], -1)
    bp, _, bi, _ = _blockers([[(-1.8, 0.7, -1.6), (0.9, 1.0, -2.0), (-0.3, 0.8, 0.3)]], 1)
    mesh = {"positions": np.concatenate([pos, bp]).astype(np.float32), "normals": None,
            "texcoords": np.concatenate([uv, [[0.1, 0.2], [0.8, 0.3], [0.4, 0.9]]]).astype(np.float32) if texcoords else None,
            "indices": np.concatenate([tris, bi + np.uint32(len(pos))]), "tri_material": np.concatenate([quad % 3, [3]]).astype(np.uint32)}
    rgba = lambda h, w: rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
    # (one size per material: a second size doubles the pixels whose weights round unclearly)
    textures = {0: (rgba(5, 7), rgba(5, 7), normal_map(rng, 5, 7)), 1: (rgba(16, 16), rgba(16, 16), normal_map(rng, 16, 16)),
                2: (None, rgba(5, 7), normal_map(rng, 5, 7))}
    mats = np.array([[0.9, 0.8, 0.7, 1.0, 1.0, 1.0], [0.6, 0.9, 0.8, 1.0, 0.7, 0.8], [0.8, 0.5, 0.4, 1.0, 0.4, 0.9], [0.5, 0.5, 0.6, 1.0, 0.0, 0.6]], np.float32)
    lights = _lights([((1.0, 0.95, 0.9), 1.8, (2.5, 4.0, 3.0)), ((0.7, 0.8, 1.0), 1.2, (-3.0, 2.5, 1.0))])
    return {"meshes": [mesh], "instances": [(EYE34, 0, 0)], "materials": mats, "textures": textures, "lights": lights,
            "miss": np.array([0.1, 0.1, 0.12], np.float32), "cam": camera((0.3, 2.6, 2.4), (0.0, 0.0, -0.9), 56.0, W / H)}


def _torus_uv(n_u=20, n_v=15):
    """WI.torus(n_u, n_v) with texture coordinates that run 2.3 times round the ring and 1.7 times round the tube, sheared (u also
    grows along the tube), so dp/du is not an edge of any triangle"""
    m = WI.torus(n_u, n_v, R=0.38, r=0.14)
    i, j = np.divmod(np.arange(n_u * n_v), n_v)
    m["texcoords"] = np.stack([2.3 * i / n_u + 0.45 * j / n_v - 0.6, 1.7 * j / n_v - 0.4], -1).astype(np.float32)
    return m


def instanced():
    """six instances of two meshes -- a faceted octahedron (no normals, no texcoords: N = Ng, UV = barycentrics) and a smooth,
    normal-mapped torus of 600 triangles -- under a rotation, a uniform scale of 2.5, a non-uniform scale (1.4, 0.6, 1.0), a mirror, a
    shear and the identity, with material offsets 0 and 3"""
    rng = np.random.RandomState(4)
    meshes = [WI.octahedron(0.8), _torus_uv()]
    shear = np.array([[1.0, 0.45, 0.0], [0.0, 1.0, 0.0], [0.2, 0.3, 1.0]])
    inst = [(WI.transform(2.5 * np.eye(3), [0.0, -0.1, -2.4]), 0, 3),                                 # a uniform scale of 2.5: the backdrop
            (WI.transform(WI.rotation(rng), [-1.15, 0.95, 0.3]), 1, 0),                              # a rotation
            (EYE34, 0, 0),                                                                            # the identity
            (WI.transform(WI.rotation(rng) @ np.diag([1.4, 0.6, 1.0]), [1.0, 0.9, 0.2]), 1, 3),       # a non-uniform scale
            (WI.transform(WI.mirror(rng), [1.2, -0.55, 0.8]), 1, 0),                                  # a mirror
            (WI.transform(0.5 * shear @ WI.rotation(rng), [-1.2, -0.5, 0.8]), 0, 0)]                        # a shear
    nm = normal_map(rng, 8, 8)
    rgba = lambda h, w: rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
    mats = np.array([[0.85, 0.8, 0.7, 1.0, 0.0, 0.7], [0.9, 0.3, 0.25, 1.0, 0.3, 0.4], [0.5, 0.5, 0.5, 1.0, 0.5, 0.5],
                     [0.4, 0.6, 0.9, 1.0, 0.2, 0.6], [0.95, 0.8, 0.35, 1.0, 1.0, 0.3]], np.float32)
    textures = {1: (rgba(8, 8), None, nm), 4: (None, rgba(8, 8), nm)}
    lights = _lights([((1.0, 0.95, 0.9), 1.6, (2.5, 3.5, 4.0)), ((0.6, 0.7, 1.0), 1.1, (-3.5, 1.5, 3.0))])
    return {"meshes": meshes, "instances": inst, "materials": mats, "textures": textures, "lights": lights,
            "miss": np.array([0.1, 0.15, 0.25], np.float32), "cam": camera((0.2, 0.8, 3.9), (0.0, 0.1, 0.0), 40.0, W / H)}


SCENES = {"sweep": sweep, "textured": textured, "instanced": instanced}


def flat_mesh(scene):
    """a one-mesh, identity-instance scene as the mesh dict oracle.whitted_render and rtgo_whitted_set_mesh take"""
    assert len(scene["meshes"]) == 1 and len(scene["instances"]) == 1 and np.array_equal(scene["instances"][0][0], EYE34)
    return dict(scene["meshes"][0], materials=scene["materials"], textures=scene["textures"], lights=scene["lights"], miss=scene["miss"])


def extra(scene):
    """the `extra` of oracle_py.InstancedScene"""
    return {"lights": scene["lights"], "miss": scene["miss"], "textures": scene["textures"]}
