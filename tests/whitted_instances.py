"""Instanced scenes for the whitted path (rtgo_whitted_set_scene) and their flattened equivalents.

The instanced oracle (oracle_py.whitted_render_instanced) draws an instanced scene with the kernel's own arithmetic.  The flattened
scene is a second, independent formulation: every instance's mesh taken to world space in float64 (positions through the object-to-world
matrix, vertex normals through W2O^T without renormalisation: the oracle normalises after interpolating, as LocalGeometry.h:112 does after
transforming), rounded to float32 and concatenated in instance order -- and rendered by oracle.whitted_render.  Concatenating in instance
order keeps the tie rule: the lowest (instance, triangle) is the lowest index of the flattened mesh."""
import numpy as np


def as34(transform):
    m = np.asarray(transform, dtype=np.float64)
    return m.reshape(-1)[:12].reshape(3, 4)


def _apply(M, X):
    """rows of X (float64) through the columns of M: M X^T, summing only the terms whose coefficient is non-zero (a signed zero stays as
    it was under a permutation or sign flip)"""
    out = np.zeros((len(X), M.shape[0]), np.float64)
    for r in range(M.shape[0]):
        terms = [M[r, k] * X[:, k] for k in range(M.shape[1]) if M[r, k] != 0.0]
        if terms:
            acc = terms[0]
            for t in terms[1:]:
                acc = acc + t
            out[:, r] = acc
    return out


def flatten(meshes, instances):
    """meshes: list of mesh dicts (positions, normals or None, indices, tri_material or None, optional texcoords); instances: list of
    (3x4 transform, mesh, material_offset).  Returns one mesh dict in world space (normals None if any instanced mesh has none;
    texcoords None unless every instanced mesh has them)."""
    pos, nrm, uv, idx, tm = [], [], [], [], []
    base = 0
    with_normals = all(meshes[int(m)].get("normals") is not None for _, m, _ in instances)
    with_uv = all(meshes[int(m)].get("texcoords") is not None for _, m, _ in instances)
    for tr, mi, off in instances:
        mesh = meshes[int(mi)]
        M = as34(np.asarray(tr, dtype=np.float32))
        A, t = M[:, :3], M[:, 3]
        p = np.asarray(mesh["positions"], dtype=np.float32).astype(np.float64)
        pos.append(_apply(M, np.concatenate([p, np.ones((len(p), 1))], axis=1)).astype(np.float32))
        if with_normals:
            n = np.asarray(mesh["normals"], dtype=np.float32).astype(np.float64)
            nrm.append(_apply(np.linalg.inv(A).T, n).astype(np.float32))      # W2O^T n
        if with_uv:
            uv.append(np.asarray(mesh["texcoords"], dtype=np.float32))
        ix = np.asarray(mesh["indices"], dtype=np.uint32).reshape(-1, 3)
        idx.append(ix + np.uint32(base))
        t_m = mesh.get("tri_material")
        tm.append((np.zeros(len(ix), np.uint32) if t_m is None else np.asarray(t_m, dtype=np.uint32)) + np.uint32(off))
        base += len(p)
    return {"positions": np.concatenate(pos), "normals": np.concatenate(nrm) if with_normals else None,
            "texcoords": np.concatenate(uv) if with_uv else None, "indices": np.concatenate(idx), "tri_material": np.concatenate(tm)}


def split_scene(mesh):
    """tests/whitted_scene.build()'s sphere, box and ground as three meshes (contiguous runs of one material; each drawn by an identity
    instance whose material offset is that material) -- concatenated in this order they are the original mesh"""
    tmat = mesh["tri_material"]
    starts = [0] + [i for i in range(1, len(tmat)) if tmat[i] != tmat[i - 1]] + [len(tmat)]
    meshes, instances = [], []
    eye = np.eye(3, 4, dtype=np.float32)
    for a, b in zip(starts[:-1], starts[1:]):
        ix = mesh["indices"][a:b]
        v0, v1 = int(ix.min()), int(ix.max()) + 1
        meshes.append({"positions": mesh["positions"][v0:v1], "normals": None if mesh["normals"] is None else mesh["normals"][v0:v1],
                       "indices": (ix - v0).astype(np.uint32), "tri_material": None})
        instances.append((eye, len(meshes) - 1, int(tmat[a])))
    return meshes, instances


def torus(n_u=30, n_v=15, R=0.5, r=0.18):
    """a torus around the y axis with smooth vertex normals: 2 n_u n_v triangles"""
    u = 2 * np.pi * np.arange(n_u) / n_u
    v = 2 * np.pi * np.arange(n_v) / n_v
    U, V = np.meshgrid(u, v, indexing="ij")
    n = np.stack([np.cos(V) * np.cos(U), np.sin(V), np.cos(V) * np.sin(U)], axis=-1)
    c = np.stack([R * np.cos(U), np.zeros_like(U), R * np.sin(U)], axis=-1)
    p = c + r * n
    tris = []
    for i in range(n_u):
        for j in range(n_v):
            a, b, cc, d = i * n_v + j, ((i + 1) % n_u) * n_v + j, ((i + 1) % n_u) * n_v + (j + 1) % n_v, i * n_v + (j + 1) % n_v
            tris += [(a, d, b), (b, d, cc)]
    return {"positions": p.reshape(-1, 3).astype(np.float32), "normals": n.reshape(-1, 3).astype(np.float32),
            "indices": np.array(tris, np.uint32), "tri_material": (np.arange(len(tris)) // (2 * n_v) % 2).astype(np.uint32)}


def octahedron(size=0.1):
    """8 triangles, no vertex normals (faceted: N = Ng)"""
    p = np.array([[size, 0, 0], [-size, 0, 0], [0, size, 0], [0, -size, 0], [0, 0, size], [0, 0, -size]], np.float32)
    tris = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return {"positions": p, "normals": None, "indices": np.array(tris, np.uint32), "tri_material": None}


def ground(g=6.0, y=0.0, normals=False):
    """a quad facing +y (with vertex normals (0, 1, 0) when asked: a flattened scene has normals for all vertices or none)"""
    return {"positions": np.array([[-g, y, -g], [g, y, -g], [g, y, g], [-g, y, g]], np.float32),
            "normals": np.tile(np.array([0, 1, 0], np.float32), (4, 1)) if normals else None,
            "indices": np.array([(0, 2, 1), (0, 3, 2)], np.uint32), "tri_material": None}


def rotation(rng):
    """a random rotation (uniform quaternion)"""
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def transform(A, t):
    return np.concatenate([np.asarray(A, np.float64), np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(np.float32)


def materials():
    """four materials: dielectric rough, dielectric glossy, mixed, metal"""
    return np.array([[0.8, 0.8, 0.75, 1.0, 0.0, 0.9], [0.9, 0.25, 0.2, 1.0, 0.1, 0.35], [0.3, 0.5, 0.9, 1.0, 0.6, 0.3],
                     [0.95, 0.8, 0.3, 1.0, 1.0, 0.25]], np.float32)


def lights():
    """two point lights and a miss colour (the `extra` of oracle_py.whitted_render_instanced)"""
    ls = np.zeros((2, 8), dtype=np.float32)
    ls[0] = [1.0, 0.95, 0.9, 2.5, 1.0, 6.0, 2.0, 0]
    ls[1] = [0.6, 0.7, 1.0, 1.0, -4.0, 3.0, -1.0, 0]
    return {"lights": ls, "miss": np.array([0.1, 0.15, 0.25], np.float32)}


def tori_scene():
    """20 instances of a 900-triangle torus with vertex normals under random rotations and translations, five of them uniformly and five
    non-uniformly scaled, over a ground with normals (21 instances, 18 002 triangles)"""
    rng = np.random.RandomState(7)
    meshes = [torus(), ground(normals=True)]
    inst = [(transform(np.eye(3), [0, 0, 0]), 1, 0)]
    for k in range(20):
        A = rotation(rng)
        if 5 <= k < 10:
            A = 0.7 * A
        elif 10 <= k < 15:
            A = A @ np.diag([1.4, 0.6, 1.0]) @ rotation(rng)
        t = [-2.4 + 1.2 * (k % 5), 0.45 + 0.35 * (k // 10), -2.0 + 1.0 * (k // 5)]
        inst.append((transform(A, t), 0, 1 + k % 2))
    return meshes, inst


def octahedra_scene(n=4095):
    """n rigid instances of an 8-triangle octahedron without vertex normals on a 64-wide grid over a ground"""
    rng = np.random.RandomState(11)
    meshes = [octahedron(0.09), ground(8.0)]
    inst = [(transform(np.eye(3), [0, 0, 0]), 1, 0)]
    for k in range(n):
        t = [-3.2 + 0.1 * (k % 64), 0.15 + 0.4 * rng.rand(), -3.2 + 0.1 * (k // 64)]
        inst.append((transform(rotation(rng), t), 0, 1 + k % 3))
    return meshes, inst


def mirror(rng):
    """a random rotation composed with a reflection (det -1)"""
    return rotation(rng) @ np.diag([1.0, -1.0, 1.0])


def mirrored_scene(smooth, n=12, scale=None, seed=5):
    """n tori (smooth: with vertex normals) or octahedra (faceted) under rotation x reflection transforms (det < 0), optionally scaled by
    diag(scale) before the rotation, over a ground (instance 0, identity)"""
    rng = np.random.RandomState(seed)
    meshes = [torus() if smooth else octahedron(0.35), ground(normals=smooth)]
    inst = [(transform(np.eye(3), [0, 0, 0]), 1, 0)]
    for k in range(n):
        A = mirror(rng)
        if scale is not None:
            A = A @ np.diag(scale)
        t = [-2.4 + 1.2 * (k % 5), 0.5 + 0.2 * (k % 3), -1.5 + 1.1 * (k // 5)]
        inst.append((transform(A, t), 0, 1 + k % 2))
    return meshes, inst


def swap_winding(mesh):
    """the same triangles with their second and third corners exchanged (the geometric normal flips)"""
    ix = np.asarray(mesh["indices"], np.uint32)
    return dict(mesh, indices=np.ascontiguousarray(ix[:, [0, 2, 1]]))


def small_scene():
    """a few tori (with normals) and octahedra (faceted) under rotations, uniform and non-uniform scales and reflections, over a ground:
    the float64 hit reference's scene and oracle_whitted_instances.npz's"""
    rng = np.random.RandomState(23)
    meshes = [torus(16, 8), octahedron(0.3), ground(3.0)]
    inst = [(transform(np.eye(3), [0, 0, 0]), 2, 0)]
    shapes = [np.eye(3), 0.6 * np.eye(3), np.diag([1.5, 0.5, 1.0]), np.diag([1.0, -1.0, 1.0]), np.diag([-0.7, 1.3, 0.9]), np.diag([2.0, 1.0, 0.4])]
    for k, S in enumerate(shapes):
        for mi in (0, 1):
            A = rotation(rng) @ S
            t = [-1.5 + 0.6 * k, 0.45 + 0.5 * mi, -0.4 + 0.8 * mi - 0.1 * k]
            inst.append((transform(A, t), mi, 1 + k % (2 + mi)))
    return meshes, inst
