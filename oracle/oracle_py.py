"""ctypes view of oracle/liboracle.so -- TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this module; nothing under
raytracingo_amd/ may (tests/test_layout_rules.py enforces it).
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liboracle.so")
REF_PROBE_PATH = os.path.join(HERE, "_ref", "libref_probe.so")

MAX_PRIMS = 512
MAX_LIGHTS = 10
SCENES = ["cornell", "slide", "mirror_spheres", "plateau", "window", "checkered", "balls", "soft_mirrors"]
CYLINDER, DISK, RECTANGLE, SPHERE = 0, 1, 2, 3


class Prim(C.Structure):
    _fields_ = [("type", C.c_int32), ("M", C.c_float * 16), ("kd", C.c_float * 3), ("kr", C.c_float * 3),
                ("specularity", C.c_float), ("Le", C.c_float * 3)]


class Light(C.Structure):
    _fields_ = [("corner", C.c_float * 3), ("v1", C.c_float * 3), ("v2", C.c_float * 3), ("normal", C.c_float * 3),
                ("color", C.c_float * 3), ("falloff", C.c_float)]


class Scene(C.Structure):
    _fields_ = [("n_prims", C.c_int32), ("n_lights", C.c_int32), ("prims", Prim * MAX_PRIMS),
                ("aabb", (C.c_float * 6) * MAX_PRIMS), ("lights", Light * MAX_LIGHTS), ("eye", C.c_float * 3),
                ("U", C.c_float * 3), ("V", C.c_float * 3), ("W", C.c_float * 3), ("bg", C.c_float * 3)]


class Frame(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("sqrt_spp", C.c_int32), ("max_depth", C.c_int32),
                ("frame_count", C.c_uint32), ("path_tracing", C.c_int32), ("use_ambient", C.c_int32),
                ("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("band_h", C.c_uint32),
                ("n_ranks", C.c_uint32), ("rank", C.c_uint32), ("mode", C.c_int32), ("threads", C.c_int32),
                ("host_double_trig", C.c_int32)]


class Counters(C.Structure):
    _fields_ = [("rays_radiance", C.c_uint64 * 8), ("rays_occlusion", C.c_uint64), ("rays_total", C.c_uint64),
                ("node_visits", C.c_uint64), ("prim_tests", C.c_uint64), ("hits", C.c_uint64)]

    def as_dict(self):
        return {"rays_radiance": list(self.rays_radiance), "rays_occlusion": int(self.rays_occlusion),
                "rays_total": int(self.rays_total), "node_visits": int(self.node_visits),
                "prim_tests": int(self.prim_tests), "hits": int(self.hits)}


class RayRecord(C.Structure):
    _fields_ = [("parent", C.c_int32), ("kind", C.c_int32), ("depth", C.c_int32), ("seed", C.c_uint32), ("o", C.c_float * 3),
                ("d", C.c_float * 3), ("tmin", C.c_float), ("tmax", C.c_float), ("hit", C.c_int32), ("prim", C.c_int32), ("t", C.c_float),
                ("n", C.c_float * 3), ("payload", C.c_float * 3)]


RAY_RECORD_DTYPE = np.dtype([("parent", "<i4"), ("kind", "<i4"), ("depth", "<i4"), ("seed", "<u4"), ("o", "<f4", 3), ("d", "<f4", 3),
                             ("tmin", "<f4"), ("tmax", "<f4"), ("hit", "<i4"), ("prim", "<i4"), ("t", "<f4"), ("n", "<f4", 3),
                             ("payload", "<f4", 3)])
assert RAY_RECORD_DTYPE.itemsize == C.sizeof(RayRecord)


class Node(C.Structure):
    _fields_ = [("bmin", C.c_float * 3), ("bmax", C.c_float * 3), ("left", C.c_int32), ("right", C.c_int32)]


class WhittedScene(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("normals", C.c_void_p), ("indices", C.c_void_p), ("tri_material", C.c_void_p),
                ("materials", C.c_void_p), ("lights", C.c_void_p), ("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32),
                ("n_materials", C.c_uint32), ("n_lights", C.c_uint32), ("eye", C.c_float * 3), ("U", C.c_float * 3),
                ("V", C.c_float * 3), ("W", C.c_float * 3), ("miss", C.c_float * 3), ("texcoords", C.c_void_p), ("mat_tex", C.c_void_p)]


class WhittedMesh(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("normals", C.c_void_p), ("texcoords", C.c_void_p), ("indices", C.c_void_p),
                ("tri_material", C.c_void_p), ("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32)]


class WhittedInstance(C.Structure):
    _fields_ = [("transform", C.c_float * 12), ("mesh", C.c_uint32), ("material_offset", C.c_uint32)]


class WhittedIScene(C.Structure):
    _fields_ = [("meshes", C.c_void_p), ("instances", C.c_void_p), ("materials", C.c_void_p), ("lights", C.c_void_p), ("mat_tex", C.c_void_p),
                ("n_meshes", C.c_uint32), ("n_instances", C.c_uint32), ("n_materials", C.c_uint32), ("n_lights", C.c_uint32),
                ("eye", C.c_float * 3), ("U", C.c_float * 3), ("V", C.c_float * 3), ("W", C.c_float * 3), ("miss", C.c_float * 3),
                ("cull", C.c_int32)]


class Tex(C.Structure):
    _fields_ = [("px", C.c_void_p), ("w", C.c_uint32), ("h", C.c_uint32)]


class MatTex(C.Structure):
    _fields_ = [("base_color", Tex), ("metallic_roughness", Tex), ("normal", Tex)]


def build(force=False):
    """Compile the oracle (and the reference probe when /root/reference is mounted). Building the checker is not using it."""
    if force or not os.path.exists(LIB_PATH) or any(
            os.path.getmtime(os.path.join(HERE, f)) > os.path.getmtime(LIB_PATH)
            for f in ("rtgo_oracle.c", "rtgo_oracle_scenes.c", "rtgo_oracle_whitted.c", "rtgo_oracle.h")):
        subprocess.check_call(["make", "-C", HERE, "-s", "all"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        L = C.CDLL(LIB_PATH)
        fp = C.POINTER(C.c_float)
        u32p = C.POINTER(C.c_uint32)
        L.oracle_tea16.restype = C.c_uint32
        L.oracle_tea16.argtypes = [C.c_uint32, C.c_uint32]
        L.oracle_lcg.restype = C.c_uint32
        L.oracle_lcg.argtypes = [u32p]
        L.oracle_rnd.restype = C.c_float
        L.oracle_rnd.argtypes = [u32p]
        L.oracle_mat_mul.argtypes = [fp, fp, fp]
        L.oracle_mat_vec4.argtypes = [fp, fp, fp]
        L.oracle_mat_transpose.argtypes = [fp, fp]
        L.oracle_mat_det.restype = C.c_float
        L.oracle_mat_det.argtypes = [fp]
        L.oracle_mat_inverse.argtypes = [fp, fp]
        L.oracle_mat_rotate.argtypes = [C.c_float] * 4 + [fp]
        L.oracle_mat_translate.argtypes = [C.c_float] * 3 + [fp]
        L.oracle_mat_scale.argtypes = [C.c_float] * 3 + [fp]
        L.oracle_normalize3.argtypes = [fp, fp]
        L.oracle_camera_uvw.argtypes = [fp, fp, fp, C.c_float, C.c_float, fp, fp, fp]
        L.oracle_prim_aabb.argtypes = [fp, fp]
        L.oracle_light_from_matrix.argtypes = [fp, fp, C.c_float, C.POINTER(Light)]
        L.oracle_intersect.restype = C.c_int
        L.oracle_intersect.argtypes = [C.POINTER(Prim), fp, fp, fp, fp]
        L.oracle_hemisphere.argtypes = [fp, fp, C.c_float, u32p, fp]
        L.oracle_scene_create.restype = C.c_int
        L.oracle_scene_create.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(Scene)]
        L.oracle_tea4.restype = C.c_uint32
        L.oracle_tea4.argtypes = [C.c_uint32, C.c_uint32]
        L.oracle_tri_intersect.restype = C.c_int
        L.oracle_tri_intersect.argtypes = [fp, fp, fp, fp, fp, C.c_float, C.c_float, fp, fp, fp]
        L.oracle_whitted_render.restype = C.c_int
        L.oracle_whitted_render.argtypes = [C.POINTER(WhittedScene), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_uint64), C.c_int]
        L.oracle_whitted_render_instanced.restype = C.c_int
        L.oracle_whitted_render_instanced.argtypes = [C.POINTER(WhittedIScene), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                      C.POINTER(C.c_uint64), C.c_int]
        L.oracle_whitted_trace_instanced.restype = C.c_int
        L.oracle_whitted_trace_instanced.argtypes = [C.POINTER(WhittedIScene), fp, fp, C.c_float, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                     fp, fp, fp]
        L.oracle_whitted_shade_point.restype = C.c_int
        L.oracle_whitted_shade_point.argtypes = [fp, fp, fp, fp, fp, fp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, fp]
        L.oracle_tex2d.restype = None
        L.oracle_tex2d.argtypes = [C.POINTER(Tex), C.c_float, C.c_float, fp]
        L.oracle_material.restype = C.c_int
        L.oracle_material.argtypes = [C.c_char_p, fp]
        L.oracle_lbvh_build.restype = C.c_int
        L.oracle_lbvh_build.argtypes = [C.c_void_p, C.c_int, C.POINTER(Node), u32p, C.POINTER(C.c_int32)]
        L.oracle_render.restype = C.c_int
        L.oracle_render.argtypes = [C.POINTER(Scene), C.POINTER(Frame), C.c_void_p, C.c_void_p, C.POINTER(Counters)]
        L.oracle_log_pixel.restype = C.c_int
        L.oracle_log_pixel.argtypes = [C.POINTER(Scene), C.POINTER(Frame), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.oracle_local_rows.restype = C.c_uint32
        L.oracle_local_rows.argtypes = [C.c_uint32] * 4
        _lib = L
    return _lib


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def scene(name, width, height):
    sc = Scene()
    if lib().oracle_scene_create(name.encode(), width, height, C.byref(sc)) != 0:
        raise ValueError("unknown scene %r" % name)
    return sc


def material(name):
    """engine/materials.h constant `name` as the oracle states it: kd[3], kr[3], Le[3], specularity (None: unknown name)"""
    v = np.zeros(10, dtype=np.float32)
    return v if lib().oracle_material(name.encode(), fptr(v)) == 0 else None


def scene_tables(sc):
    """numpy views of a Scene: dict(type[n], M[n,16], mat[n,10] (kd,kr,spec,Le), aabb[n,6], lights[nl,16], cam[12], bg[3])"""
    n = sc.n_prims
    t = np.array([sc.prims[i].type for i in range(n)], dtype=np.int32)
    M = np.array([list(sc.prims[i].M) for i in range(n)], dtype=np.float32)
    mat = np.array([list(sc.prims[i].kd) + list(sc.prims[i].kr) + [sc.prims[i].specularity] + list(sc.prims[i].Le)
                    for i in range(n)], dtype=np.float32)
    aabb = np.array([list(sc.aabb[i]) for i in range(n)], dtype=np.float32)
    lights = np.array([list(L.corner) + list(L.v1) + list(L.v2) + list(L.normal) + list(L.color) + [L.falloff]
                       for L in list(sc.lights)[:sc.n_lights]], dtype=np.float32)
    cam = np.array(list(sc.eye) + list(sc.U) + list(sc.V) + list(sc.W), dtype=np.float32)
    return {"type": t, "M": M, "mat": mat, "aabb": aabb, "lights": lights, "cam": cam,
            "bg": np.array(list(sc.bg), dtype=np.float32)}


def frame(width, height, sqrt_spp=1, frame_count=0, path=True, ambient=False, window=None, bands=(1, 1, 0), mode=1,
          threads=0, max_depth=5, host_double_trig=False):
    x0, y0, w, h = window if window is not None else (0, 0, width, height)
    band_h, n_ranks, rank = bands
    return Frame(width, height, sqrt_spp, max_depth, frame_count, int(path), int(ambient), x0, y0, w, h, band_h,
                 n_ranks, rank, mode, threads, int(host_double_trig))


def local_rows(h, band_h, n_ranks, rank):
    return int(lib().oracle_local_rows(h, band_h, n_ranks, rank))


def render(sc, fr, accum_prev=None):
    """returns (accum float32 [rows,w,4], image uint8 [rows,w,4], counters dict)"""
    rows = local_rows(fr.h, fr.band_h or 1, fr.n_ranks or 1, fr.rank)
    accum = np.zeros((rows, fr.w, 4), dtype=np.float32) if accum_prev is None else np.array(accum_prev, dtype=np.float32)
    assert accum.shape == (rows, fr.w, 4)
    image = np.zeros((rows, fr.w, 4), dtype=np.uint8)
    ctr = Counters()
    lib().oracle_render(C.byref(sc), C.byref(fr), accum.ctypes.data, image.ctypes.data, C.byref(ctr))
    return accum, image, ctr.as_dict()


def log_launch(sc, fr, accum_prev=None):
    """oracle_log_pixel over every pixel of fr's window, row by row: (records: RAY_RECORD_DTYPE in call order, `parent` indexing this
    array, -1 for raygen's own calls; pixel [records]: the flat index of each record's pixel in the window; accum [h, w, 4]; image [h, w, 4])"""
    accum = np.zeros((fr.h, fr.w, 4), dtype=np.float32) if accum_prev is None else np.array(accum_prev, dtype=np.float32)
    image = np.zeros((fr.h, fr.w, 4), dtype=np.uint8)
    cap = 4 * fr.sqrt_spp * fr.sqrt_spp * (fr.max_depth + 2)       # a path: one radiance and at most one occlusion call per depth
    buf = np.zeros(cap, dtype=RAY_RECORD_DTYPE)
    parts, pixel, base = [], [], 0
    for y in range(fr.h):
        for x in range(fr.w):
            n = lib().oracle_log_pixel(C.byref(sc), C.byref(fr), fr.x0 + x, fr.y0 + y, accum[y, x].ctypes.data, image[y, x].ctypes.data,
                                       buf.ctypes.data, cap)
            assert 0 < n <= cap
            r = buf[:n].copy()
            r["parent"][r["parent"] >= 0] += base
            parts.append(r)
            pixel.append(np.full(n, y * fr.w + x))
            base += n
    return np.concatenate(parts), np.concatenate(pixel), accum, image


def lbvh(aabb):
    aabb = f32(aabb)
    n = aabb.shape[0]
    nodes = (Node * (2 * n))()
    code = np.zeros(n, dtype=np.uint32)
    order = np.zeros(n, dtype=np.int32)
    lib().oracle_lbvh_build(aabb.ctypes.data, n, nodes, code.ctypes.data_as(C.POINTER(C.c_uint32)),
                            order.ctypes.data_as(C.POINTER(C.c_int32)))
    arr = np.zeros((2 * n - 1, 8), dtype=np.float32)
    links = np.zeros((2 * n - 1, 2), dtype=np.int32)
    for i in range(2 * n - 1):
        arr[i, :3] = list(nodes[i].bmin)
        arr[i, 3:6] = list(nodes[i].bmax)
        links[i] = (nodes[i].left, nodes[i].right)
    return arr[:, :6], links, code, order


def scene_from_tables(types, M, mat, lights16, cam12, bg=(0.0, 0.0, 0.0), aabb=None):
    """build an oracle Scene from flattened tables (the same arrays the C ABI takes); AABBs default to the CubeBox rule"""
    sc = Scene()
    n = len(types)
    assert n <= MAX_PRIMS
    sc.n_prims = n
    M = f32(M).reshape(n, 16)
    mat = f32(mat).reshape(n, 10)
    for i in range(n):
        p = sc.prims[i]
        p.type = int(types[i])
        p.M[:] = M[i].tolist()
        p.kd[:] = mat[i, 0:3].tolist()
        p.kr[:] = mat[i, 3:6].tolist()
        p.specularity = float(mat[i, 6])
        p.Le[:] = mat[i, 7:10].tolist()
        if aabb is None:
            bb = np.zeros(6, dtype=np.float32)
            lib().oracle_prim_aabb(fptr(M[i].copy()), fptr(bb))
        else:
            bb = f32(aabb[i])
        sc.aabb[i][:] = bb.tolist()
    lights16 = f32(lights16).reshape(-1, 16)
    sc.n_lights = lights16.shape[0]
    for i in range(sc.n_lights):
        r = lights16[i].tolist()
        L = sc.lights[i]
        L.corner[:], L.v1[:], L.v2[:], L.normal[:], L.color[:], L.falloff = r[0:3], r[3:6], r[6:9], r[9:12], r[12:15], r[15]
    cam12 = f32(cam12)
    sc.eye[:], sc.U[:], sc.V[:], sc.W[:] = cam12[0:3].tolist(), cam12[3:6].tolist(), cam12[6:9].tolist(), cam12[9:12].tolist()
    sc.bg[:] = list(bg)
    return sc


def light_from_matrix(M, color=(1.0, 1.0, 1.0), falloff=0.0):
    """SurfaceLight record (16 floats) of a unit rectangle under M (light.cpp:9-28)"""
    L = Light()
    lib().oracle_light_from_matrix(fptr(f32(M).reshape(16).copy()), fptr(f32(color)), float(falloff), C.byref(L))
    return np.array(list(L.corner) + list(L.v1) + list(L.v2) + list(L.normal) + list(L.color) + [L.falloff], dtype=np.float32)


def tex2d(texture, u, v):
    """oracle_tex2d on a uint8 [h, w, 4] array"""
    a = np.ascontiguousarray(texture, dtype=np.uint8)
    out = np.zeros(4, dtype=np.float32)
    lib().oracle_tex2d(C.byref(Tex(a.ctypes.data, a.shape[1], a.shape[0])), float(u), float(v), fptr(out))
    return out


def whitted_render(mesh, cam12, width, height, subframes=1, threads=0):
    """the oracle's whitted path (rtgo_oracle_whitted.c) over `subframes` accumulated subframes.
    mesh: dict(positions [nv,3] f32, normals [nv,3] f32 or None, indices [nt,3] u32, tri_material [nt] u32 or None,
    materials [nm,6] f32 (base_color rgba, metallic, roughness), lights [nl,8] (color rgb, intensity, position xyz, falloff as int bits),
    miss (3,)).  Returns (accum [h,w,4] f32, image [h,w,4] u8, {rays_total, rays_occlusion})."""
    pos = np.ascontiguousarray(mesh["positions"], dtype=np.float32)
    nrm = None if mesh.get("normals") is None else np.ascontiguousarray(mesh["normals"], dtype=np.float32)
    idx = np.ascontiguousarray(mesh["indices"], dtype=np.uint32)
    tm = None if mesh.get("tri_material") is None else np.ascontiguousarray(mesh["tri_material"], dtype=np.uint32)
    mats = np.ascontiguousarray(mesh["materials"], dtype=np.float32)
    lights = np.ascontiguousarray(mesh["lights"], dtype=np.float32).reshape(-1, 8)
    s = WhittedScene()
    s.positions, s.normals = pos.ctypes.data, (nrm.ctypes.data if nrm is not None else None)
    s.indices, s.tri_material = idx.ctypes.data, (tm.ctypes.data if tm is not None else None)
    s.materials, s.lights = mats.ctypes.data, (lights.ctypes.data if len(lights) else None)
    s.n_vertices, s.n_triangles, s.n_materials, s.n_lights = len(pos), len(idx), len(mats), len(lights)
    cam = f32(cam12)
    s.eye[:], s.U[:], s.V[:], s.W[:] = cam[0:3].tolist(), cam[3:6].tolist(), cam[6:9].tolist(), cam[9:12].tolist()
    s.miss[:] = f32(mesh["miss"]).tolist()
    # optional: texcoords [nv, 2] and textures = {material index: (base_color, metallic_roughness, normal)}, each uint8 [h, w, 4] or None
    uv = None if mesh.get("texcoords") is None else np.ascontiguousarray(mesh["texcoords"], dtype=np.float32)
    s.texcoords = uv.ctypes.data if uv is not None else None
    keep = []
    mt = _mat_tex(mesh.get("textures"), len(mats), keep)
    if mt is not None:
        s.mat_tex = C.addressof(mt)
    return _whitted_frames(lib().oracle_whitted_render, s, width, height, subframes, threads)


def _threads(threads):
    if threads <= 0:
        threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1
    return threads


def _whitted_frames(fn, s, width, height, subframes, threads):
    acc = np.zeros((height, width, 4), dtype=np.float32)
    img = np.zeros((height, width, 4), dtype=np.uint8)
    rays = (C.c_uint64 * 2)(0, 0)
    for sf in range(subframes):
        rc = fn(C.byref(s), width, height, sf, acc.ctypes.data, img.ctypes.data, rays, _threads(threads))
        assert rc == 0
    return acc, img, {"rays_total": int(rays[0]), "rays_occlusion": int(rays[1])}


def _mat_tex(textures, n_materials, keep):
    """{material index: (base_color, metallic_roughness, normal)}, each uint8 [h, w, 4] or None -> MatTex array (or None)"""
    if not textures:
        return None
    mt = (MatTex * n_materials)()
    for mi, triple in textures.items():
        for name, t in zip(("base_color", "metallic_roughness", "normal"), triple):
            if t is None:
                continue
            a = np.ascontiguousarray(t, dtype=np.uint8)
            keep.append(a)
            setattr(mt[mi], name, Tex(a.ctypes.data, a.shape[1], a.shape[0]))
    keep.append(mt)
    return mt


class InstancedScene:
    """an oracle_whitted_iscene over what Context.whitted_set_scene takes -- meshes (dicts: positions, normals or None, indices,
    tri_material or None, optional texcoords), instances [(3x4 transform, mesh, material_offset)], materials [n, 6] -- plus `extra`
    (lights [nl, 8], miss (3,), optional textures {material: (base_color, metallic_roughness, normal)}) and a camera (eye, U, V, W)"""

    def __init__(self, meshes, instances, materials, extra=None, cam12=None, cull=True):
        keep = self._keep = []

        def arr(a, dt, cols):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt).reshape((-1, cols) if cols else -1)
            keep.append(a)
            return a

        ms = (WhittedMesh * len(meshes))()
        for k, m in enumerate(meshes):
            pos, nrm, uv = arr(m["positions"], np.float32, 3), arr(m.get("normals"), np.float32, 3), arr(m.get("texcoords"), np.float32, 2)
            idx, tm = arr(m["indices"], np.uint32, 3), arr(m.get("tri_material"), np.uint32, 0)
            ms[k] = WhittedMesh(pos.ctypes.data, nrm.ctypes.data if nrm is not None else None, uv.ctypes.data if uv is not None else None,
                                idx.ctypes.data, tm.ctypes.data if tm is not None else None, len(pos), len(idx))
        ins = (WhittedInstance * max(len(instances), 1))()
        for k, (tr, mi, off) in enumerate(instances):
            ins[k].transform[:] = np.asarray(tr, dtype=np.float32).reshape(-1)[:12].tolist()
            ins[k].mesh, ins[k].material_offset = int(mi), int(off)
        mats = arr(materials, np.float32, 6)
        extra = extra or {}
        lights = arr(extra.get("lights", np.zeros((0, 8), np.float32)), np.float32, 8)
        keep += [ms, ins]
        s = self.s = WhittedIScene()
        s.meshes, s.instances, s.materials = C.addressof(ms), C.addressof(ins), mats.ctypes.data
        s.lights = lights.ctypes.data if len(lights) else None
        mt = _mat_tex(extra.get("textures"), len(mats), keep)
        s.mat_tex = C.addressof(mt) if mt is not None else None
        s.n_meshes, s.n_instances, s.n_materials, s.n_lights = len(meshes), len(instances), len(mats), len(lights)
        if cam12 is not None:
            cam = f32(cam12)
            s.eye[:], s.U[:], s.V[:], s.W[:] = cam[0:3].tolist(), cam[3:6].tolist(), cam[6:9].tolist(), cam[9:12].tolist()
        s.miss[:] = f32(extra.get("miss", np.zeros(3, np.float32))).tolist()
        s.cull = 1 if cull else 0

    def render(self, width, height, subframes=1, threads=0):
        return _whitted_frames(lib().oracle_whitted_render_instanced, self.s, width, height, subframes, threads)

    def trace(self, o, d, tmin=0.01, tmax=1e16):
        """oracle_whitted_trace_instanced: (instance, triangle, t, u, v) of the closest hit of the world ray, or None"""
        o, d = f32(o), f32(d)
        ii, tri = C.c_int(-1), C.c_int(-1)
        t, u, v = C.c_float(0), C.c_float(0), C.c_float(0)
        rc = lib().oracle_whitted_trace_instanced(C.byref(self.s), fptr(o), fptr(d), tmin, tmax, C.byref(ii), C.byref(tri), C.byref(t), C.byref(u),
                                                  C.byref(v))
        assert rc >= 0, "invalid instanced scene"
        return (ii.value, tri.value, t.value, u.value, v.value) if rc else None


def whitted_render_instanced(meshes, instances, materials, extra, cam12, width, height, subframes=1, threads=0, cull=True):
    """the oracle's whitted path over an instanced scene (oracle_whitted_render_instanced), `subframes` accumulated: what
    Context.whitted_set_scene takes, `extra` as InstancedScene.  Returns (accum [h,w,4] f32, image [h,w,4] u8, {rays_total, rays_occlusion})."""
    return InstancedScene(meshes, instances, materials, extra, cam12, cull).render(width, height, subframes, threads)


def whitted_shade_point(P, N, corners, corner_uv, UV, rd, material, lights, textures=None, occlusion=False):
    """oracle_whitted_shade_point: the closest-hit program on a stated hit.  P, N, rd (3,), corners (3, 3), corner_uv (3, 2), UV (2,),
    material (6,) (base colour rgba, metallic, roughness), lights [nl, 8], textures (base_color, metallic_roughness, normal) each uint8
    [h, w, 4] or None; occlusion: the triangle of the corners occludes (False: nothing does).  Returns (rgb (3,) f32, gate-passing lights)."""
    a = [f32(np.asarray(x).reshape(-1)) for x in (P, N, corners, corner_uv, UV, rd)]
    mat = f32(np.asarray(material).reshape(6))
    ls = f32(np.asarray(lights).reshape(-1, 8))
    keep = []
    mt = _mat_tex({0: textures} if textures is not None and any(t is not None for t in textures) else None, 1, keep)
    rgb = np.zeros(3, dtype=np.float32)
    n = lib().oracle_whitted_shade_point(*[fptr(x) for x in a], mat.ctypes.data, C.addressof(mt) if mt is not None else None,
                                         ls.ctypes.data if len(ls) else None, len(ls), 0 if occlusion else 1, fptr(rgb))
    assert n >= 0
    return rgb, n
