"""Procedural meshes beyond RTGO_MAX_TRIANGLES for the clustered-mesh tests (tests/test_whitted_clustered.py) and tools/whitted_inst_perf.py,
and the caller's cut the library replaces: a mesh split into contiguous index ranges of at most RTGO_MAX_TRIANGLES triangles, each drawn
by its own instance.  Concatenated in order, the chunks are the mesh again, so the chunked scene's closest-hit order (instance, triangle)
is the clustered mesh's (instance, the mesh's own triangle)."""
import numpy as np

import whitted_instances as WI


def displaced_torus(n_u, n_v, R=0.6, r=0.22, amp=0.03, freq=(7, 5), texcoords=True):
    """a torus around the y axis with its tube radius displaced by amp sin(f_u u) cos(f_v v): 2 n_u n_v triangles, analytic vertex normals
    of the displaced surface, texture coordinates (u, v) in [0, 1)^2 and two materials in bands along u"""
    u = 2 * np.pi * np.arange(n_u) / n_u
    v = 2 * np.pi * np.arange(n_v) / n_v
    U, V = np.meshgrid(u, v, indexing="ij")
    fu, fv = freq
    rr = r + amp * np.sin(fu * U) * np.cos(fv * V)
    drdu = amp * fu * np.cos(fu * U) * np.cos(fv * V)
    drdv = -amp * fv * np.sin(fu * U) * np.sin(fv * V)
    nrm0 = np.stack([np.cos(V) * np.cos(U), np.sin(V), np.cos(V) * np.sin(U)], axis=-1)
    c = np.stack([R * np.cos(U), np.zeros_like(U), R * np.sin(U)], axis=-1)
    p = c + rr[..., None] * nrm0
    # partial derivatives of p for the normal
    dc_du = np.stack([-R * np.sin(U), np.zeros_like(U), R * np.cos(U)], axis=-1)
    dn_du = np.stack([-np.cos(V) * np.sin(U), np.zeros_like(U), np.cos(V) * np.cos(U)], axis=-1)
    dn_dv = np.stack([-np.sin(V) * np.cos(U), np.cos(V), -np.sin(V) * np.sin(U)], axis=-1)
    pu = dc_du + drdu[..., None] * nrm0 + rr[..., None] * dn_du
    pv = drdv[..., None] * nrm0 + rr[..., None] * dn_dv
    n = np.cross(pv, pu)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    i = np.arange(n_u)[:, None]
    j = np.arange(n_v)[None, :]
    a = i * n_v + j
    b = ((i + 1) % n_u) * n_v + j
    cc = ((i + 1) % n_u) * n_v + (j + 1) % n_v
    d = i * n_v + (j + 1) % n_v
    tris = np.stack([np.stack([a, d, b], -1), np.stack([b, d, cc], -1)], axis=2).reshape(-1, 3)
    mesh = {"positions": p.reshape(-1, 3).astype(np.float32), "normals": n.reshape(-1, 3).astype(np.float32),
            "indices": tris.astype(np.uint32), "tri_material": ((np.arange(len(tris)) // (2 * n_v)) * 8 // n_u % 2).astype(np.uint32)}
    if texcoords:
        mesh["texcoords"] = np.stack([U / (2 * np.pi), V / (2 * np.pi)], axis=-1).reshape(-1, 2).astype(np.float32)
    return mesh


def flat_sheet(n, size=1.0):
    """an n x n grid of quads in the plane y = 0 (2 n^2 triangles, no normals): seen edge-on, every ray grazes its bounds"""
    g = np.linspace(-size, size, n + 1, dtype=np.float64)
    X, Z = np.meshgrid(g, g, indexing="ij")
    p = np.stack([X, np.zeros_like(X), Z], axis=-1).reshape(-1, 3).astype(np.float32)
    i = np.arange(n)[:, None]
    j = np.arange(n)[None, :]
    a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
    tris = np.stack([np.stack([a, c, b], -1), np.stack([a, d, c], -1)], axis=2).reshape(-1, 3)   # (wound so that Ng is +y)
    return {"positions": p, "normals": None, "indices": tris.astype(np.uint32), "tri_material": None}


def chunks(mesh, size=8192):
    """the caller's cut: contiguous runs of at most `size` triangles, each with the vertex range its indices span (re-based to 0).
    Returns a list of (mesh dict, vertex offset) in order."""
    ix = np.asarray(mesh["indices"], np.uint32).reshape(-1, 3)
    out = []
    for a in range(0, len(ix), size):
        part = ix[a:a + size]
        v0, v1 = int(part.min()), int(part.max()) + 1
        m = {"positions": mesh["positions"][v0:v1], "indices": (part - np.uint32(v0)).astype(np.uint32),
             "normals": None if mesh.get("normals") is None else mesh["normals"][v0:v1],
             "tri_material": None if mesh.get("tri_material") is None else mesh["tri_material"][a:a + size]}
        if mesh.get("texcoords") is not None:
            m["texcoords"] = mesh["texcoords"][v0:v1]
        out.append((m, v0))
    return out


def unchunk(parts):
    """the chunks of chunks() put back together: the mesh's indices, triangle materials and (per chunk) vertex data"""
    idx = np.concatenate([m["indices"] + np.uint32(v0) for m, v0 in parts])
    tm = None if parts[0][0]["tri_material"] is None else np.concatenate([m["tri_material"] for m, _ in parts])
    return idx, tm


def chunked_scene(meshes, instances, big, size=8192):
    """meshes / instances (WI's (transform, mesh, material_offset)) with every mesh whose index is in `big` replaced by its chunks, each
    drawn under the instance's transform: the scene a caller builds today.  Instance order is kept (a chunked instance becomes a run of
    instances), so the lowest (instance, triangle) is the same triangle in both scenes."""
    out_meshes, where = [], {}
    for k, m in enumerate(meshes):
        if k in big:
            parts = chunks(m, size)
            where[k] = list(range(len(out_meshes), len(out_meshes) + len(parts)))
            out_meshes += [p for p, _ in parts]
        else:
            where[k] = [len(out_meshes)]
            out_meshes.append(m)
    out_inst = [(tr, mi, off) for tr, m, off in instances for mi in where[int(m)]]
    return out_meshes, out_inst
