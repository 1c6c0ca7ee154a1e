"""ctypes binding of the C ABI in include/rtgo.h (librtgo_hip.so).

This is plumbing for the Python drivers (bench.py, tests, the multi-GPU band driver): the product is the shared
library.  There is deliberately no fallback: if the library is missing or no gfx950 GPU is present the calls raise.
"""
import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# RTGO_HIP_LIB: developer override to A/B an experimental build of the same ABI (never a different backend)
LIB_PATH = os.environ.get("RTGO_HIP_LIB") or os.path.join(PKG_DIR, "librtgo_hip.so")

RTGO_MAX_PRIMS = 512
RTGO_MAX_SCENE_PRIMS = 1 << 20   # rtgo_set_large_scene: built and walked in global memory
RTGO_MAX_LIGHTS = 10
CYLINDER, DISK, RECTANGLE, SPHERE = 0, 1, 2, 3

# every symbol include/rtgo.h declares (tests/test_capi_symbols.py checks the header against this list and the .so)
SYMBOLS = [
    "rtgo_create", "rtgo_destroy", "rtgo_last_error", "rtgo_set_stream", "rtgo_set_scene", "rtgo_set_camera",
    "rtgo_set_background", "rtgo_set_lights", "rtgo_resize", "rtgo_bind_output", "rtgo_launch", "rtgo_sync",
    "rtgo_read_image", "rtgo_read_accum", "rtgo_write_accum", "rtgo_get_stats", "rtgo_reset_stats", "rtgo_read_bvh",
    "rtgo_local_rows", "rtgo_abi_version", "rtgo_assemble_bands", "rtgo_set_large_scene",
    "rtgo_whitted_set_mesh", "rtgo_whitted_set_lights", "rtgo_whitted_set_miss_color", "rtgo_whitted_launch",
    "rtgo_whitted_set_texcoords", "rtgo_whitted_set_material_textures", "rtgo_whitted_set_scene", "rtgo_whitted_set_instances",
    "rtgo_whitted_launch_frame", "rtgo_launch_frames", "rtgo_trace_rays", "rtgo_whitted_trace_rays", "rtgo_whitted_update_mesh",
    "rtgo_whitted_update_meshes", "rtgo_whitted_launch_frames", "rtgo_whitted_shade_rays", "rtgo_whitted_rebuild_meshes",
    "rtgo_shade_rays", "rtgo_update_prims", "rtgo_whitted_update_meshes_device",
    "rtgo_set_scene_device", "rtgo_set_large_scene_device", "rtgo_update_prims_device", "rtgo_whitted_set_instances_device",
    "rtgo_whitted_set_scene_device", "rtgo_whitted_set_mesh_device", "rtgo_whitted_set_texcoords_device",
    "rtgo_update_prims_device_async", "rtgo_update_prims_status",
    "rtgo_whitted_refit_instances_device_async", "rtgo_whitted_refit_instances_status",
]
UPDATE_PENDING, UPDATE_APPLIED, UPDATE_REFUSED = 0, 1, 2
UPDATE_REFIT, UPDATE_REBUILD = 0, 1
TRACE_CLOSEST, TRACE_ANY_HIT = 0, 1
HIT_MISS, HIT_INVALID = -1, -2
RTGO_WHITTED_MAX_MESHES = 256
RTGO_WHITTED_MAX_INSTANCES = 8192
RTGO_WHITTED_MAX_MESH_TRIANGLES = 1 << 24     # per mesh of rtgo_whitted_set_scene (beyond RTGO_MAX_TRIANGLES: a clustered mesh)
RTGO_WHITTED_MAX_SCENE_TRIANGLES = 1 << 26    # all meshes of a scene together


class RtgoError(RuntimeError):
    pass


class Prim(C.Structure):
    _fields_ = [("type", C.c_uint32), ("model", C.c_float * 16), ("kd", C.c_float * 3), ("kr", C.c_float * 3),
                ("specularity", C.c_float), ("Le", C.c_float * 3)]


# rtgo_prim as a numpy record (packed, 108 bytes): bulk packing for set_large_scene
PRIM_DTYPE = np.dtype([("type", "<u4"), ("model", "<f4", (16,)), ("kd", "<f4", (3,)), ("kr", "<f4", (3,)), ("specularity", "<f4"),
                       ("Le", "<f4", (3,))])
assert PRIM_DTYPE.itemsize == C.sizeof(Prim)


class Aabb(C.Structure):
    _fields_ = [("minX", C.c_float), ("minY", C.c_float), ("minZ", C.c_float), ("maxX", C.c_float),
                ("maxY", C.c_float), ("maxZ", C.c_float)]


class Light(C.Structure):
    _fields_ = [("corner", C.c_float * 3), ("v1", C.c_float * 3), ("v2", C.c_float * 3), ("normal", C.c_float * 3),
                ("color", C.c_float * 3), ("falloff", C.c_float)]


class Frame(C.Structure):
    _fields_ = [("image_width", C.c_uint32), ("image_height", C.c_uint32), ("sqrt_spp", C.c_int32),
                ("max_trace_depth", C.c_int32), ("frame_count", C.c_uint32), ("path_tracing", C.c_uint32),
                ("use_ambient", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32),
                ("h", C.c_uint32), ("band_h", C.c_uint32), ("n_ranks", C.c_uint32), ("rank", C.c_uint32),
                ("collect_stats", C.c_uint32), ("reserve_cus", C.c_uint32)]


class WhittedFrame(C.Structure):
    _fields_ = [("image_width", C.c_uint32), ("image_height", C.c_uint32), ("subframe_index", C.c_uint32),
                ("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("band_h", C.c_uint32),
                ("n_ranks", C.c_uint32), ("rank", C.c_uint32), ("reserve_cus", C.c_uint32)]


class Texture(C.Structure):
    _fields_ = [("rgba8", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32)]


class WhittedMesh(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("normals", C.c_void_p), ("texcoords", C.c_void_p), ("n_vertices", C.c_uint32),
                ("indices", C.c_void_p), ("material_of_triangle", C.c_void_p), ("n_triangles", C.c_uint32)]


class WhittedInstance(C.Structure):
    _fields_ = [("transform", C.c_float * 12), ("mesh", C.c_uint32), ("material_offset", C.c_uint32)]


class WhittedMeshUpdate(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("positions", C.c_void_p), ("normals", C.c_void_p), ("n_vertices", C.c_uint32)]


class UpdateStatus(C.Structure):
    _fields_ = [("state", C.c_uint32), ("fault", C.c_uint32), ("entry", C.c_uint32), ("reserved", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("rays_total", C.c_uint64), ("rays_occlusion", C.c_uint64), ("node_visits", C.c_uint64),
                ("prim_tests", C.c_uint64), ("hits", C.c_uint64), ("last_launch_ms", C.c_float),
                ("total_launch_ms", C.c_float), ("launches", C.c_uint32), ("lbvh_depth", C.c_uint32),
                ("dbg_fast_boxes", C.c_uint64), ("dbg_fast_tests", C.c_uint64), ("rays_culled", C.c_uint64),
                ("launches_canonical", C.c_uint32), ("cuboid_groups", C.c_uint32),
                ("guard_reach", C.c_float), ("guard_quadric", C.c_float),
                ("last_variant", C.c_uint32), ("launches_trial", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Ray(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("tmin", C.c_float), ("dir", C.c_float * 3), ("tmax", C.c_float)]


class ShadeOptions(C.Structure):
    _fields_ = [("max_trace_depth", C.c_int32), ("path_tracing", C.c_uint32), ("use_ambient", C.c_uint32), ("sample_index", C.c_uint32)]


class Hit(C.Structure):
    _fields_ = [("t", C.c_float), ("prim", C.c_int32), ("instance", C.c_int32), ("u", C.c_float), ("v", C.c_float), ("n", C.c_float * 3)]


# rtgo_ray / rtgo_hit as numpy records (32 bytes each): what Context.trace_rays takes and returns
RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("tmin", "<f4"), ("dir", "<f4", (3,)), ("tmax", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<i4"), ("instance", "<i4"), ("u", "<f4"), ("v", "<f4"), ("n", "<f4", (3,))])
assert RAY_DTYPE.itemsize == C.sizeof(Ray) == 32 and HIT_DTYPE.itemsize == C.sizeof(Hit) == 32


def make_rays(origins, dirs, tmin=1e-3, tmax=1e16):
    """a RAY_DTYPE array from origins [n, 3] and directions [n, 3] (broadcast against each other) and scalar or per-ray tmin / tmax"""
    o, d = np.broadcast_arrays(np.asarray(origins, dtype=np.float32).reshape(-1, 3), np.asarray(dirs, dtype=np.float32).reshape(-1, 3))
    r = np.zeros(len(o), dtype=RAY_DTYPE)
    r["origin"], r["dir"], r["tmin"], r["tmax"] = o, d, tmin, tmax
    return r


_lib = None


def load():
    """dlopen librtgo_hip.so and declare the prototypes. Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RtgoError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                        "There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    fp = C.POINTER(C.c_float)
    L.rtgo_abi_version.restype = C.c_uint32
    L.rtgo_last_error.restype = C.c_char_p
    L.rtgo_last_error.argtypes = [vp]
    L.rtgo_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.rtgo_destroy.argtypes = [vp]
    L.rtgo_set_stream.argtypes = [vp, vp]
    L.rtgo_set_scene.argtypes = [vp, C.POINTER(Prim), C.POINTER(Aabb), C.c_uint32]
    L.rtgo_set_large_scene.argtypes = [vp, C.POINTER(Prim), C.POINTER(Aabb), C.c_uint32]
    L.rtgo_update_prims.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(Prim), C.POINTER(Aabb), C.c_uint32, C.c_uint32]
    L.rtgo_set_scene_device.argtypes = [vp, vp, vp, C.c_uint32]
    L.rtgo_set_large_scene_device.argtypes = [vp, vp, vp, C.c_uint32]
    L.rtgo_update_prims_device.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32]
    L.rtgo_update_prims_device_async.argtypes = [vp, vp, vp, vp, C.c_uint32, C.POINTER(Aabb), C.POINTER(C.c_uint64)]
    L.rtgo_update_prims_status.argtypes = [vp, C.c_uint64, C.POINTER(UpdateStatus)]
    L.rtgo_set_camera.argtypes = [vp, fp, fp, fp, fp]
    L.rtgo_set_background.argtypes = [vp, fp]
    L.rtgo_set_lights.argtypes = [vp, C.POINTER(Light), C.c_int]
    L.rtgo_resize.argtypes = [vp, C.c_size_t]
    L.rtgo_bind_output.argtypes = [vp, vp, vp, C.c_size_t]
    L.rtgo_launch.argtypes = [vp, C.POINTER(Frame)]
    L.rtgo_launch_frames.argtypes = [vp, C.POINTER(Frame), C.c_uint32]
    L.rtgo_sync.argtypes = [vp]
    L.rtgo_read_image.argtypes = [vp, vp, C.c_size_t]
    L.rtgo_read_accum.argtypes = [vp, vp, C.c_size_t]
    L.rtgo_write_accum.argtypes = [vp, vp, C.c_size_t]
    L.rtgo_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.rtgo_reset_stats.argtypes = [vp]
    L.rtgo_read_bvh.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t]
    L.rtgo_local_rows.restype = C.c_uint32
    L.rtgo_local_rows.argtypes = [C.c_uint32] * 4
    L.rtgo_assemble_bands.argtypes = [vp, vp, vp, vp] + [C.c_uint32] * 6
    L.rtgo_whitted_set_mesh.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, C.c_uint32]
    L.rtgo_whitted_set_lights.argtypes = [vp, vp, C.c_uint32]
    L.rtgo_whitted_set_miss_color.argtypes = [vp, fp]
    L.rtgo_whitted_launch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32]
    L.rtgo_whitted_set_texcoords.argtypes = [vp, vp, C.c_uint32]
    L.rtgo_whitted_set_material_textures.argtypes = [vp, C.c_uint32, C.POINTER(Texture), C.POINTER(Texture), C.POINTER(Texture)]
    L.rtgo_whitted_set_scene.argtypes = [vp, C.POINTER(WhittedMesh), C.c_uint32, C.POINTER(WhittedInstance), C.c_uint32, vp, C.c_uint32]
    L.rtgo_whitted_set_instances.argtypes = [vp, C.POINTER(WhittedInstance), C.c_uint32]
    L.rtgo_whitted_update_mesh.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint32]
    L.rtgo_whitted_update_meshes.argtypes = [vp, C.POINTER(WhittedMeshUpdate), C.c_uint32]
    L.rtgo_whitted_rebuild_meshes.argtypes = [vp, C.POINTER(WhittedMeshUpdate), C.c_uint32]
    L.rtgo_whitted_update_meshes_device.argtypes = [vp, C.POINTER(WhittedMeshUpdate), C.c_uint32, C.c_uint32]
    L.rtgo_whitted_set_instances_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    L.rtgo_whitted_refit_instances_device_async.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint64)]
    L.rtgo_whitted_refit_instances_status.argtypes = [vp, C.c_uint64, C.POINTER(UpdateStatus)]
    L.rtgo_whitted_set_scene_device.argtypes = [vp, C.POINTER(WhittedMesh), C.c_uint32, C.POINTER(WhittedInstance), C.c_uint32, vp, C.c_uint32]
    L.rtgo_whitted_set_mesh_device.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, C.c_uint32]
    L.rtgo_whitted_set_texcoords_device.argtypes = [vp, vp, C.c_uint32]
    L.rtgo_whitted_launch_frame.argtypes = [vp, C.POINTER(WhittedFrame)]
    L.rtgo_whitted_launch_frames.argtypes = [vp, C.POINTER(WhittedFrame), C.c_uint32]
    L.rtgo_trace_rays.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32]
    L.rtgo_whitted_trace_rays.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32]
    L.rtgo_whitted_shade_rays.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32]
    L.rtgo_shade_rays.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.POINTER(ShadeOptions)]
    for name in SYMBOLS:
        fn = getattr(L, name)
        if fn.restype is C.c_int and name not in ("rtgo_last_error", "rtgo_local_rows", "rtgo_abi_version"):
            fn.restype = C.c_int
    _lib = L
    return L


_hip = None


def hip_runtime():
    """the HIP runtime librtgo_hip.so runs on (the copy this process has mapped), for the few device buffers the binding itself needs"""
    global _hip
    if _hip is None:
        load()
        with open("/proc/self/maps") as f:
            path = next((line.split()[-1] for line in f if "libamdhip64.so" in line), "libamdhip64.so")
        H = C.CDLL(path)
        H.hipSetDevice.argtypes = [C.c_int]
        H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        H.hipFree.argtypes = [C.c_void_p]
        H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]   # kind: 1 host to device, 2 device to host
        _hip = H
    return _hip


def local_rows(h, band_h, n_ranks, rank):
    return int(load().rtgo_local_rows(h, band_h, n_ranks, rank))


def _f3(v):
    a = np.ascontiguousarray(v, dtype=np.float32).reshape(3)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


class Context:
    """One rtgo_ctx (one GPU). Thin: every method is one C-ABI call plus error translation."""

    def __init__(self, device=0):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.rtgo_create(int(device), C.byref(h))
        if rc != 0:
            raise RtgoError("rtgo_create(%d) failed (%d): %s" % (device, rc, self._lib.rtgo_last_error(None).decode()))
        self._h = h
        self.device = int(device)
        self.pixels = 0

    def _check(self, rc, what):
        if rc != 0:
            raise RtgoError("%s failed (%d): %s" % (what, rc, self._lib.rtgo_last_error(self._h).decode()))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rtgo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream_ptr):
        self._check(self._lib.rtgo_set_stream(self._h, C.c_void_p(hip_stream_ptr or 0)), "rtgo_set_stream")

    def set_scene(self, types, models, materials, aabbs=None):
        """types[n] int, models[n,16] float32 row-major, materials[n,10] = kd(3) kr(3) specularity Le(3)."""
        types = np.asarray(types)
        models = np.ascontiguousarray(models, dtype=np.float32).reshape(-1, 16)
        materials = np.ascontiguousarray(materials, dtype=np.float32).reshape(-1, 10)
        n = len(types)
        arr = (Prim * max(n, 1))()
        for i in range(n):
            p = arr[i]
            p.type = int(types[i])
            p.model[:] = models[i].tolist()
            p.kd[:] = materials[i, 0:3].tolist()
            p.kr[:] = materials[i, 3:6].tolist()
            p.specularity = float(materials[i, 6])
            p.Le[:] = materials[i, 7:10].tolist()
        bb = None
        if aabbs is not None:
            aabbs = np.ascontiguousarray(aabbs, dtype=np.float32).reshape(-1, 6)
            bb = (Aabb * n)()
            for i in range(n):
                (bb[i].minX, bb[i].minY, bb[i].minZ, bb[i].maxX, bb[i].maxY, bb[i].maxZ) = aabbs[i].tolist()
        self._check(self._lib.rtgo_set_scene(self._h, arr, bb, n), "rtgo_set_scene")
        self.n_prims = n

    def set_large_scene(self, types, models, materials, aabbs=None):
        """rtgo_set_large_scene: set_scene's arguments, up to RTGO_MAX_SCENE_PRIMS primitives.  The records are packed with numpy
        (a million primitives upload in seconds)."""
        types = np.asarray(types)
        n = len(types)
        rec = np.zeros(n, dtype=PRIM_DTYPE)
        rec["type"] = types.astype(np.uint32)
        rec["model"] = np.asarray(models, dtype=np.float32).reshape(-1, 16)
        mat = np.asarray(materials, dtype=np.float32).reshape(-1, 10)
        rec["kd"], rec["kr"], rec["specularity"], rec["Le"] = mat[:, 0:3], mat[:, 3:6], mat[:, 6], mat[:, 7:10]
        bb = None
        if aabbs is not None:
            bb = np.ascontiguousarray(aabbs, dtype=np.float32).reshape(-1, 6)
            if len(bb) != n:
                raise ValueError("aabbs: %d boxes for %d primitives" % (len(bb), n))
        self._check(self._lib.rtgo_set_large_scene(self._h, rec.ctypes.data_as(C.POINTER(Prim)) if n else (Prim * 1)(),
                                                   bb.ctypes.data_as(C.POINTER(Aabb)) if bb is not None else None, n),
                    "rtgo_set_large_scene")
        self.n_prims = n

    def update_prims(self, indices, types, models, materials, aabbs=None, rebuild=False):
        """rtgo_update_prims: primitive indices[j] becomes (types[j], models[j], materials[j]) with the box aabbs[j]; the arguments as
        set_scene takes them.  aabbs: given exactly when the scene was set with boxes.  rebuild: RTGO_UPDATE_REBUILD, else a refit."""
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        k = len(idx)
        rec = np.zeros(k, dtype=PRIM_DTYPE)
        rec["type"] = np.asarray(types).astype(np.uint32).reshape(-1)
        rec["model"] = np.asarray(models, dtype=np.float32).reshape(-1, 16)
        mat = np.asarray(materials, dtype=np.float32).reshape(-1, 10)
        rec["kd"], rec["kr"], rec["specularity"], rec["Le"] = mat[:, 0:3], mat[:, 3:6], mat[:, 6], mat[:, 7:10]
        bb = None
        if aabbs is not None:
            bb = np.ascontiguousarray(aabbs, dtype=np.float32).reshape(-1, 6)
            if len(bb) != k:
                raise ValueError("aabbs: %d boxes for %d updates" % (len(bb), k))
        self._check(self._lib.rtgo_update_prims(self._h, idx.ctypes.data_as(C.POINTER(C.c_uint32)), rec.ctypes.data_as(C.POINTER(Prim)),
                                                bb.ctypes.data_as(C.POINTER(Aabb)) if bb is not None else None, k,
                                                UPDATE_REBUILD if rebuild else UPDATE_REFIT),
                    "rtgo_update_prims")

    # ---- the same three calls for records a device already holds (torch tensors; see device_prims_args and prims_tensor) ----
    def _device_args(self, who, indices, prims, aabbs):
        k, ptrs = device_prims_args(who, self.device, indices, prims, aabbs)
        hip_runtime().hipDeviceSynchronize()   # (whatever stream filled the tensors: the calls run on the context's)
        return k, [C.c_void_p(p) for p in ptrs]

    def set_scene_device(self, prims, aabbs=None):
        """rtgo_set_scene_device: prims a tensor of n rtgo_prim records (prims_tensor's layout), aabbs float32 [n, 6] or None, both on the
        context's device.  Synchronous."""
        n, (_, p, b) = self._device_args("set_scene_device", None, prims, aabbs)
        self._check(self._lib.rtgo_set_scene_device(self._h, p, b, n), "rtgo_set_scene_device")
        self.n_prims = n

    def set_large_scene_device(self, prims, aabbs=None):
        """rtgo_set_large_scene_device: set_scene_device's arguments, up to RTGO_MAX_SCENE_PRIMS records, read where they lie."""
        n, (_, p, b) = self._device_args("set_large_scene_device", None, prims, aabbs)
        self._check(self._lib.rtgo_set_large_scene_device(self._h, p, b, n), "rtgo_set_large_scene_device")
        self.n_prims = n

    def update_prims_device(self, indices, prims, aabbs=None, rebuild=False):
        """rtgo_update_prims_device: primitive indices[j] becomes record prims[j] with the box aabbs[j].  indices: a contiguous int32
        tensor [k] (its bits are read as uint32); prims, aabbs: as set_scene_device takes them, k of each; all on the context's device.
        aabbs: given exactly when the scene was set with boxes.  rebuild: RTGO_UPDATE_REBUILD, else a refit.  Synchronous."""
        k, (i, p, b) = self._device_args("update_prims_device", indices, prims, aabbs)
        self._check(self._lib.rtgo_update_prims_device(self._h, i, p, b, k, UPDATE_REBUILD if rebuild else UPDATE_REFIT), "rtgo_update_prims_device")

    def update_prims_device_async(self, indices, prims, aabbs=None, reach=None):
        """rtgo_update_prims_device_async: update_prims_device's refit of a scene of set_large_scene[_device], enqueued on the context's
        stream with no wait on the host -- none here either: the tensors' writes must be complete or ordered on that stream.  reach: six
        floats (min xyz, max xyz), a box every updated primitive's box stays inside; None: the bounds the context holds.  Returns the
        ticket update_prims_status takes."""
        k, (i, p, b) = device_prims_args("update_prims_device_async", self.device, indices, prims, aabbs)
        box = None if reach is None else Aabb(*[float(x) for x in np.asarray(reach, dtype=np.float32).reshape(6)])
        ticket = C.c_uint64(0)
        self._check(self._lib.rtgo_update_prims_device_async(self._h, i, p, b, k, None if box is None else C.byref(box), C.byref(ticket)),
                    "rtgo_update_prims_device_async")
        return ticket.value

    def update_prims_status(self, ticket):
        """rtgo_update_prims_status: {"state": UPDATE_PENDING / UPDATE_APPLIED / UPDATE_REFUSED, "fault": 0 or the kind 1 .. 7, "entry": the
        offending entry of a refused update}; never blocks"""
        st = UpdateStatus()
        self._check(self._lib.rtgo_update_prims_status(self._h, int(ticket), C.byref(st)), "rtgo_update_prims_status")
        return {"state": st.state, "fault": st.fault, "entry": st.entry}

    def set_camera(self, eye, U, V, W):
        a = [_f3(x) for x in (eye, U, V, W)]
        self._check(self._lib.rtgo_set_camera(self._h, a[0][1], a[1][1], a[2][1], a[3][1]), "rtgo_set_camera")

    def set_background(self, rgb):
        a = _f3(rgb)
        self._check(self._lib.rtgo_set_background(self._h, a[1]), "rtgo_set_background")

    def set_lights(self, lights16):
        """lights16[n,16] = corner v1 v2 normal color falloff"""
        lights16 = np.ascontiguousarray(lights16, dtype=np.float32).reshape(-1, 16)
        n = lights16.shape[0]
        arr = (Light * max(n, 1))()
        for i in range(n):
            L = arr[i]
            r = lights16[i].tolist()
            L.corner[:], L.v1[:], L.v2[:], L.normal[:], L.color[:], L.falloff = r[0:3], r[3:6], r[6:9], r[9:12], r[12:15], r[15]
        self._check(self._lib.rtgo_set_lights(self._h, arr, n), "rtgo_set_lights")

    def resize(self, pixels):
        self._check(self._lib.rtgo_resize(self._h, int(pixels)), "rtgo_resize")
        self.pixels = int(pixels)

    def bind_output(self, d_accum_ptr, d_image_ptr, pixels):
        self._check(self._lib.rtgo_bind_output(self._h, C.c_void_p(d_accum_ptr), C.c_void_p(d_image_ptr), int(pixels)),
                    "rtgo_bind_output")
        self.pixels = int(pixels)

    def launch(self, frame):
        self._check(self._lib.rtgo_launch(self._h, C.byref(frame)), "rtgo_launch")

    def launch_frames(self, frame, n_frames):
        """n_frames progressive frames from frame.frame_count on (rtgo_launch_frames: one kernel launch where the batched kernels apply)"""
        self._check(self._lib.rtgo_launch_frames(self._h, C.byref(frame), int(n_frames)), "rtgo_launch_frames")

    def sync(self):
        self._check(self._lib.rtgo_sync(self._h), "rtgo_sync")

    def read_accum(self, rows, w):
        out = np.empty((rows, w, 4), dtype=np.float32)
        self._check(self._lib.rtgo_read_accum(self._h, out.ctypes.data, out.nbytes), "rtgo_read_accum")
        return out

    def read_image(self, rows, w):
        out = np.empty((rows, w, 4), dtype=np.uint8)
        self._check(self._lib.rtgo_read_image(self._h, out.ctypes.data, out.nbytes), "rtgo_read_image")
        return out

    def write_accum(self, accum):
        a = np.ascontiguousarray(accum, dtype=np.float32)
        self._check(self._lib.rtgo_write_accum(self._h, a.ctypes.data, a.nbytes), "rtgo_write_accum")

    # ---- the whitted triangle path (cuda/whitted.cu), one call per C-ABI entry ----
    def whitted_set_mesh(self, positions, normals, indices, tri_material, materials):
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        tm = None if tri_material is None else np.ascontiguousarray(tri_material, dtype=np.uint32)
        mats = np.ascontiguousarray(materials, dtype=np.float32).reshape(-1, 6)
        self._check(self._lib.rtgo_whitted_set_mesh(self._h, pos.ctypes.data, nrm.ctypes.data if nrm is not None else None, len(pos),
                                                    idx.ctypes.data, tm.ctypes.data if tm is not None else None, len(idx),
                                                    mats.ctypes.data, len(mats)), "rtgo_whitted_set_mesh")

    def whitted_set_scene(self, meshes, instances, materials):
        """meshes: list of dicts shaped like tests/whitted_scene.build()'s output (positions, normals or None, indices, tri_material or None)
        plus an optional texcoords [nv, 2]; instances: see whitted_instances(); materials [n, 6] (base colour rgba, metallic, roughness)"""
        keep = []

        def arr(a, dt, cols):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt).reshape((-1, cols) if cols else -1)
            keep.append(a)
            return a

        ms = (WhittedMesh * max(len(meshes), 1))()
        for k, m in enumerate(meshes):
            pos, nrm, uv = arr(m["positions"], np.float32, 3), arr(m.get("normals"), np.float32, 3), arr(m.get("texcoords"), np.float32, 2)
            idx, tm = arr(m["indices"], np.uint32, 3), arr(m.get("tri_material"), np.uint32, 0)
            ms[k] = WhittedMesh(pos.ctypes.data, nrm.ctypes.data if nrm is not None else None, uv.ctypes.data if uv is not None else None,
                                len(pos), idx.ctypes.data, tm.ctypes.data if tm is not None else None, len(idx))
        inst = whitted_instances(instances)
        mats = np.ascontiguousarray(materials, dtype=np.float32).reshape(-1, 6)
        self._check(self._lib.rtgo_whitted_set_scene(self._h, ms, len(meshes), inst, len(instances), mats.ctypes.data, len(mats)),
                    "rtgo_whitted_set_scene")

    def whitted_set_instances(self, instances):
        inst = whitted_instances(instances)
        self._check(self._lib.rtgo_whitted_set_instances(self._h, inst, len(instances)), "rtgo_whitted_set_instances")

    def whitted_update_mesh(self, mesh, positions, normals=None):
        """rtgo_whitted_update_mesh: new positions [nv, 3] (and normals, None keeps them) for mesh `mesh` of the scene, refitted in place"""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if nrm is not None and len(nrm) != len(pos):
            raise ValueError("whitted_update_mesh: one normal per position")
        self._check(self._lib.rtgo_whitted_update_mesh(self._h, int(mesh), pos.ctypes.data, nrm.ctypes.data if nrm is not None else None, len(pos)),
                    "rtgo_whitted_update_mesh")

    def _mesh_updates(self, updates, who):
        arr = (WhittedMeshUpdate * max(len(updates), 1))()
        keep = []   # the arrays the entries point into, alive until the call returns
        for k, (mesh, positions, normals) in enumerate(updates):
            pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
            nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
            if nrm is not None and len(nrm) != len(pos):
                raise ValueError(who + ": one normal per position")
            keep += [pos, nrm]
            arr[k] = WhittedMeshUpdate(int(mesh), pos.ctypes.data, nrm.ctypes.data if nrm is not None else None, len(pos))
        return arr, keep

    def whitted_update_meshes(self, updates):
        """rtgo_whitted_update_meshes: [(mesh, positions [nv, 3], normals or None), ...] refitted as one transaction (clustered meshes too)"""
        arr, keep = self._mesh_updates(updates, "whitted_update_meshes")
        self._check(self._lib.rtgo_whitted_update_meshes(self._h, arr, len(updates)), "rtgo_whitted_update_meshes")

    def whitted_rebuild_meshes(self, updates):
        """rtgo_whitted_rebuild_meshes: [(mesh, positions [nv, 3], normals or None), ...] built again in place as one transaction; the
        rest of the scene (other meshes, instances, materials, textures) stays"""
        arr, keep = self._mesh_updates(updates, "whitted_rebuild_meshes")
        self._check(self._lib.rtgo_whitted_rebuild_meshes(self._h, arr, len(updates)), "rtgo_whitted_rebuild_meshes")

    def whitted_update_meshes_device(self, updates, rebuild=False):
        """rtgo_whitted_update_meshes_device: [(mesh, positions, normals or None), ...] with positions / normals contiguous float32
        torch tensors [nv, 3] on the context's device, refitted (rebuild=False: whitted_update_meshes) or built again (rebuild=True:
        whitted_rebuild_meshes) from where they lie.  The tensors' writes must be complete (torch.cuda.synchronize()) or ordered on the
        context's stream.  Synchronous."""
        who = "whitted_update_meshes_device"
        arr = (WhittedMeshUpdate * max(len(updates), 1))()
        keep = []   # the tensors the entries point into, alive until the call returns
        for k, (mesh, positions, normals) in enumerate(updates):
            for t in (positions,) if normals is None else (positions, normals):
                if not hasattr(t, "data_ptr") or not t.is_cuda or t.device.index != self.device:
                    raise ValueError("%s: positions and normals must be torch tensors on device %d" % (who, self.device))
                if str(t.dtype) != "torch.float32" or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous():
                    raise ValueError(who + ": positions and normals must be contiguous float32 tensors of shape [nv, 3]")
            if normals is not None and normals.shape[0] != positions.shape[0]:
                raise ValueError(who + ": one normal per position")
            keep += [positions, normals]
            arr[k] = WhittedMeshUpdate(int(mesh), positions.data_ptr(), normals.data_ptr() if normals is not None else None, positions.shape[0])
        self._check(self._lib.rtgo_whitted_update_meshes_device(self._h, arr, len(updates), UPDATE_REBUILD if rebuild else UPDATE_REFIT),
                    "rtgo_whitted_update_meshes_device")

    def whitted_set_instances_device(self, instances, refit=False):
        """rtgo_whitted_set_instances_device: instances a contiguous tensor of n rtgo_whitted_instance records (instances_tensor's
        layout: uint8 [n, 56], or float32 / int32 [n, 14]) on the context's device.  refit=False: the top level built again, as
        whitted_set_instances builds it; refit=True: RTGO_UPDATE_REFIT, the same count and mesh choices as the scene holds, the top
        level refitted in place.  The tensor's writes must be complete (torch.cuda.synchronize()) or ordered on the context's stream.
        Synchronous."""
        n, ptr = device_instances_args("whitted_set_instances_device", self.device, instances)
        self._check(self._lib.rtgo_whitted_set_instances_device(self._h, C.c_void_p(ptr), n, UPDATE_REFIT if refit else UPDATE_REBUILD),
                    "rtgo_whitted_set_instances_device")

    def whitted_refit_instances_device_async(self, instances):
        """rtgo_whitted_refit_instances_device_async: whitted_set_instances_device's refit (refit=True: the same tensor, count and mesh
        choices), enqueued on the context's stream with no wait on the host -- none here either: the tensor's writes must be complete
        or ordered on that stream, and it must stay as it is until the update has run.  Returns the ticket
        whitted_refit_instances_status takes."""
        n, ptr = device_instances_args("whitted_refit_instances_device_async", self.device, instances)
        ticket = C.c_uint64(0)
        self._check(self._lib.rtgo_whitted_refit_instances_device_async(self._h, C.c_void_p(ptr), n, C.byref(ticket)),
                    "rtgo_whitted_refit_instances_device_async")
        return ticket.value

    def whitted_refit_instances_status(self, ticket):
        """rtgo_whitted_refit_instances_status: {"state": UPDATE_PENDING / UPDATE_APPLIED / UPDATE_REFUSED, "fault": 0 or the kind 1 .. 5,
        "entry": the offending instance of a refused update}; never blocks"""
        st = UpdateStatus()
        self._check(self._lib.rtgo_whitted_refit_instances_status(self._h, int(ticket), C.byref(st)), "rtgo_whitted_refit_instances_status")
        return {"state": st.state, "fault": st.fault, "entry": st.entry}

    def whitted_set_scene_device(self, meshes, instances, materials):
        """rtgo_whitted_set_scene_device: whitted_set_scene's arguments with contiguous torch tensors on the context's device in place
        of the meshes' arrays (positions / normals float32 [nv, 3], texcoords float32 [nv, 2], indices int32 or uint32 [nt, 3],
        tri_material int32 or uint32 [nt]; normals, texcoords and tri_material optional); instances and materials stay host data.  The
        tensors' writes must be complete (torch.cuda.synchronize()) or ordered on the context's stream.  Synchronous."""
        who = "whitted_set_scene_device"
        ms = (WhittedMesh * max(len(meshes), 1))()
        for k, m in enumerate(meshes):
            nv, nt, p = device_mesh_args("%s: mesh %d" % (who, k), self.device, m["positions"], m.get("normals"), m.get("texcoords"), m["indices"],
                                         m.get("tri_material"))
            ms[k] = WhittedMesh(p[0], p[1], p[2], nv, p[3], p[4], nt)
        inst = whitted_instances(instances)
        mats = np.ascontiguousarray(materials, dtype=np.float32).reshape(-1, 6)
        self._check(self._lib.rtgo_whitted_set_scene_device(self._h, ms, len(meshes), inst, len(instances), mats.ctypes.data, len(mats)),
                    "rtgo_whitted_set_scene_device")

    def whitted_set_mesh_device(self, positions, normals, indices, tri_material, materials):
        """rtgo_whitted_set_mesh_device: whitted_set_mesh's arguments with torch tensors on the context's device (see
        whitted_set_scene_device) for positions, normals (or None), indices and tri_material (or None)"""
        nv, nt, p = device_mesh_args("whitted_set_mesh_device", self.device, positions, normals, None, indices, tri_material)
        mats = np.ascontiguousarray(materials, dtype=np.float32).reshape(-1, 6)
        self._check(self._lib.rtgo_whitted_set_mesh_device(self._h, p[0], p[1], nv, p[3], p[4], nt, mats.ctypes.data, len(mats)),
                    "rtgo_whitted_set_mesh_device")

    def whitted_set_texcoords_device(self, uv):
        """rtgo_whitted_set_texcoords_device: uv a contiguous float32 torch tensor [nv, 2] on the context's device, or None (removes them)"""
        if uv is None:
            self._check(self._lib.rtgo_whitted_set_texcoords_device(self._h, None, 0), "rtgo_whitted_set_texcoords_device")
            return
        device_mesh_tensor("whitted_set_texcoords_device", self.device, "uv", uv, ("torch.float32",), 2)
        self._check(self._lib.rtgo_whitted_set_texcoords_device(self._h, C.c_void_p(uv.data_ptr()), uv.shape[0]), "rtgo_whitted_set_texcoords_device")

    def whitted_set_texcoords(self, uv):
        if uv is None:
            self._check(self._lib.rtgo_whitted_set_texcoords(self._h, None, 0), "rtgo_whitted_set_texcoords")
            return
        a = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        self._check(self._lib.rtgo_whitted_set_texcoords(self._h, a.ctypes.data, len(a)), "rtgo_whitted_set_texcoords")

    def whitted_set_material_textures(self, material, base_color=None, metallic_roughness=None, normal=None):
        """each texture: uint8 array [h, w, 4] (row 0 first) or None"""
        keep, ptrs = [], []
        for t in (base_color, metallic_roughness, normal):
            if t is None:
                ptrs.append(None)
                continue
            a = np.ascontiguousarray(t, dtype=np.uint8)
            assert a.ndim == 3 and a.shape[2] == 4
            keep.append(a)
            ptrs.append(C.pointer(Texture(a.ctypes.data, a.shape[1], a.shape[0])))
        self._check(self._lib.rtgo_whitted_set_material_textures(self._h, int(material), ptrs[0], ptrs[1], ptrs[2]), "rtgo_whitted_set_material_textures")

    def whitted_set_lights(self, lights8):
        l = np.ascontiguousarray(lights8, dtype=np.float32).reshape(-1, 8)
        self._check(self._lib.rtgo_whitted_set_lights(self._h, l.ctypes.data if len(l) else None, len(l)), "rtgo_whitted_set_lights")

    def whitted_set_miss_color(self, rgb):
        a, p = _f3(rgb)
        self._check(self._lib.rtgo_whitted_set_miss_color(self._h, p), "rtgo_whitted_set_miss_color")

    def whitted_launch(self, width, height, subframe):
        self._check(self._lib.rtgo_whitted_launch(self._h, width, height, subframe), "rtgo_whitted_launch")

    def whitted_launch_frame(self, frame):
        """one subframe of a window / row band of the image (make_whitted_frame): the output holds the share's compact rows"""
        self._check(self._lib.rtgo_whitted_launch_frame(self._h, C.byref(frame)), "rtgo_whitted_launch_frame")

    def whitted_launch_frames(self, frame, n):
        """n subframes of the frame's share from frame.subframe_index on, in one kernel launch (rtgo_whitted_launch_frames)"""
        self._check(self._lib.rtgo_whitted_launch_frames(self._h, C.byref(frame), int(n)), "rtgo_whitted_launch_frames")

    # ---- ray queries: the caller's own rays against the context's scene ----
    def _trace(self, fn, what, rays, flags):
        H = hip_runtime()
        if hasattr(rays, "data_ptr"):   # a torch device tensor: traced where it is
            if not rays.is_cuda or not rays.is_contiguous() or rays.numel() * rays.element_size() % 32:
                raise ValueError("%s: rays must be a contiguous device tensor of 32-byte rtgo_ray records" % what)
            n, host = rays.numel() * rays.element_size() // 32, None
        else:
            host = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
            n = len(host)
        hits = np.empty(n, dtype=HIT_DTYPE)
        if n == 0:
            return hits
        if H.hipSetDevice(self.device) != 0:
            raise RtgoError("%s: hipSetDevice(%d) failed" % (what, self.device))
        buf = C.c_void_p()
        if H.hipMalloc(C.byref(buf), 32 * n * (1 if host is None else 2)) != 0:
            raise RtgoError("%s: hipMalloc of %d bytes failed" % (what, 64 * n))
        try:
            d_hits = buf.value
            if host is None:
                d_rays = rays.data_ptr()
                H.hipDeviceSynchronize()   # (whatever stream filled the tensor: the trace runs on the context's)
            else:
                d_rays = buf.value + 32 * n
                if H.hipMemcpy(d_rays, host.ctypes.data, 32 * n, 1) != 0:
                    raise RtgoError("%s: upload failed" % what)
            self._check(fn(self._h, C.c_void_p(d_rays), C.c_void_p(d_hits), n, int(flags)), what)
            self.sync()
            if H.hipMemcpy(hits.ctypes.data, d_hits, 32 * n, 2) != 0:
                raise RtgoError("%s: download failed" % what)
        finally:
            H.hipFree(buf)
        return hits

    def trace_rays(self, rays, flags=0):
        """rtgo_trace_rays over the scene of set_scene / set_large_scene.  rays: a RAY_DTYPE array (uploaded) or a contiguous torch
        device tensor of rtgo_ray records; returns the hits as a HIT_DTYPE array.  Synchronous."""
        return self._trace(self._lib.rtgo_trace_rays, "rtgo_trace_rays", rays, flags)

    def whitted_trace_rays(self, rays, flags=0):
        """rtgo_whitted_trace_rays over the scene of whitted_set_mesh / whitted_set_scene; as trace_rays"""
        return self._trace(self._lib.rtgo_whitted_trace_rays, "rtgo_whitted_trace_rays", rays, flags)

    def trace_rays_raw(self, d_rays_ptr, d_hits_ptr, n, flags=0, whitted=False):
        """the bare C call on two device pointers (asynchronous); returns the library's code instead of raising"""
        fn = self._lib.rtgo_whitted_trace_rays if whitted else self._lib.rtgo_trace_rays
        return int(fn(self._h, C.c_void_p(d_rays_ptr), C.c_void_p(d_hits_ptr), int(n), int(flags)))

    def whitted_shade_rays(self, rays, sample_index=0, accum=None, image=True):
        """rtgo_whitted_shade_rays over the scene of whitted_set_mesh / whitted_set_scene.  rays: as trace_rays takes them.  accum: the mean
        of the samples before this one, [n, 4] float32, uploaded when sample_index > 0 (None: zeros).  Returns (accum [n, 4] float32,
        image [n, 4] uint8, or None with image=False).  Synchronous."""
        what = "rtgo_whitted_shade_rays"
        H = hip_runtime()
        if hasattr(rays, "data_ptr"):   # a torch device tensor: shaded where it is
            if not rays.is_cuda or not rays.is_contiguous() or rays.numel() * rays.element_size() % 32:
                raise ValueError("%s: rays must be a contiguous device tensor of 32-byte rtgo_ray records" % what)
            n, host = rays.numel() * rays.element_size() // 32, None
        else:
            host = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
            n = len(host)
        out = np.zeros((n, 4), dtype=np.float32)
        if sample_index > 0 and accum is not None:
            out[:] = np.asarray(accum, dtype=np.float32).reshape(n, 4)
        img = np.zeros((n, 4), dtype=np.uint8) if image else None
        if n == 0:
            return out, img
        if H.hipSetDevice(self.device) != 0:
            raise RtgoError("%s: hipSetDevice(%d) failed" % (what, self.device))
        buf = C.c_void_p()   # [accum 16 n][rays 32 n, when uploaded][image 4 n]
        ray_bytes = 0 if host is None else 32 * n
        if H.hipMalloc(C.byref(buf), 16 * n + ray_bytes + 4 * n) != 0:
            raise RtgoError("%s: hipMalloc of %d bytes failed" % (what, 20 * n + ray_bytes))
        try:
            d_accum, d_image = buf.value, buf.value + 16 * n + ray_bytes
            if host is None:
                d_rays = rays.data_ptr()
                H.hipDeviceSynchronize()   # (whatever stream filled the tensor: the call runs on the context's)
            else:
                d_rays = buf.value + 16 * n
                if H.hipMemcpy(d_rays, host.ctypes.data, 32 * n, 1) != 0:
                    raise RtgoError("%s: upload failed" % what)
            if sample_index > 0 and H.hipMemcpy(d_accum, out.ctypes.data, 16 * n, 1) != 0:
                raise RtgoError("%s: upload failed" % what)
            self._check(self._lib.rtgo_whitted_shade_rays(self._h, C.c_void_p(d_rays), C.c_void_p(d_accum), C.c_void_p(d_image if image else 0), n,
                                                          int(sample_index)), what)
            self.sync()
            if H.hipMemcpy(out.ctypes.data, d_accum, 16 * n, 2) != 0 or (image and H.hipMemcpy(img.ctypes.data, d_image, 4 * n, 2) != 0):
                raise RtgoError("%s: download failed" % what)
        finally:
            H.hipFree(buf)
        return out, img

    def whitted_shade_rays_raw(self, d_rays_ptr, d_accum_ptr, d_image_ptr, n, sample_index=0):
        """the bare C call on three device pointers (asynchronous); returns the library's code instead of raising"""
        return int(self._lib.rtgo_whitted_shade_rays(self._h, C.c_void_p(d_rays_ptr), C.c_void_p(d_accum_ptr), C.c_void_p(d_image_ptr or 0), int(n),
                                                     int(sample_index)))

    def shade_rays(self, rays, seeds=None, path=True, ambient=False, max_depth=5, sample_index=0, accum=None, image=True):
        """rtgo_shade_rays over the scene of set_scene / set_large_scene.  rays: as trace_rays takes them.  seeds: one uint32 per ray (a
        numpy array, uploaded, or a contiguous torch device tensor), or None: tea<16>(i, sample_index).  accum: the mean of the samples
        before this one, [n, 4] float32, uploaded when sample_index > 0 (None: zeros).  Returns (accum [n, 4] float32, image [n, 4]
        uint8, or None with image=False).  Synchronous."""
        what = "rtgo_shade_rays"
        H = hip_runtime()
        if hasattr(rays, "data_ptr"):   # a torch device tensor: shaded where it is
            if not rays.is_cuda or not rays.is_contiguous() or rays.numel() * rays.element_size() % 32:
                raise ValueError("%s: rays must be a contiguous device tensor of 32-byte rtgo_ray records" % what)
            n, host = rays.numel() * rays.element_size() // 32, None
        else:
            host = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
            n = len(host)
        host_seeds = None
        if seeds is not None:
            if hasattr(seeds, "data_ptr"):
                if not seeds.is_cuda or not seeds.is_contiguous() or seeds.numel() * seeds.element_size() != 4 * n:
                    raise ValueError("%s: seeds must be a contiguous device tensor of one 32-bit word per ray" % what)
            else:
                host_seeds = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
                if len(host_seeds) != n:
                    raise ValueError("%s: %d seeds for %d rays" % (what, len(host_seeds), n))
        out = np.zeros((n, 4), dtype=np.float32)
        if sample_index > 0 and accum is not None:
            out[:] = np.asarray(accum, dtype=np.float32).reshape(n, 4)
        img = np.zeros((n, 4), dtype=np.uint8) if image else None
        if n == 0:
            return out, img
        if H.hipSetDevice(self.device) != 0:
            raise RtgoError("%s: hipSetDevice(%d) failed" % (what, self.device))
        buf = C.c_void_p()   # [accum 16 n][rays 32 n, when uploaded][image 4 n][seeds 4 n, when uploaded]
        ray_bytes = 0 if host is None else 32 * n
        total = 16 * n + ray_bytes + 4 * n + (0 if host_seeds is None else 4 * n)
        if H.hipMalloc(C.byref(buf), total) != 0:
            raise RtgoError("%s: hipMalloc of %d bytes failed" % (what, total))
        try:
            d_accum, d_image = buf.value, buf.value + 16 * n + ray_bytes
            if host is None:
                d_rays = rays.data_ptr()
            else:
                d_rays = buf.value + 16 * n
                if H.hipMemcpy(d_rays, host.ctypes.data, 32 * n, 1) != 0:
                    raise RtgoError("%s: upload failed" % what)
            d_seeds = 0
            if host_seeds is not None:
                d_seeds = d_image + 4 * n
                if H.hipMemcpy(d_seeds, host_seeds.ctypes.data, 4 * n, 1) != 0:
                    raise RtgoError("%s: upload failed" % what)
            elif seeds is not None:
                d_seeds = seeds.data_ptr()
            if host is None or (seeds is not None and host_seeds is None):
                H.hipDeviceSynchronize()   # (whatever stream filled the tensors: the call runs on the context's)
            if sample_index > 0 and H.hipMemcpy(d_accum, out.ctypes.data, 16 * n, 1) != 0:
                raise RtgoError("%s: upload failed" % what)
            opt = ShadeOptions(int(max_depth), 1 if path else 0, 1 if ambient else 0, int(sample_index))
            self._check(self._lib.rtgo_shade_rays(self._h, C.c_void_p(d_rays), C.c_void_p(d_seeds), C.c_void_p(d_accum),
                                                  C.c_void_p(d_image if image else 0), n, C.byref(opt)), what)
            self.sync()
            if H.hipMemcpy(out.ctypes.data, d_accum, 16 * n, 2) != 0 or (image and H.hipMemcpy(img.ctypes.data, d_image, 4 * n, 2) != 0):
                raise RtgoError("%s: download failed" % what)
        finally:
            H.hipFree(buf)
        return out, img

    def shade_rays_raw(self, d_rays_ptr, d_seeds_ptr, d_accum_ptr, d_image_ptr, n, opt):
        """the bare C call on four device pointers and a ShadeOptions (or None) (asynchronous); returns the library's code instead of raising"""
        return int(self._lib.rtgo_shade_rays(self._h, C.c_void_p(d_rays_ptr or 0), C.c_void_p(d_seeds_ptr or 0), C.c_void_p(d_accum_ptr or 0),
                                             C.c_void_p(d_image_ptr or 0), int(n), C.byref(opt) if opt is not None else None))

    def stats(self):
        s = Stats()
        self._check(self._lib.rtgo_get_stats(self._h, C.byref(s)), "rtgo_get_stats")
        return s.as_dict()

    def reset_stats(self):
        self._check(self._lib.rtgo_reset_stats(self._h), "rtgo_reset_stats")

    def read_bvh(self):
        n = self.n_prims
        nodes = np.empty((2 * n - 1, 8), dtype=np.float32)
        inv = np.empty((n, 12), dtype=np.float32)
        aabb = np.empty((n, 6), dtype=np.float32)
        self._check(self._lib.rtgo_read_bvh(self._h, nodes.ctypes.data, nodes.nbytes, inv.ctypes.data, inv.nbytes,
                                            aabb.ctypes.data, aabb.nbytes), "rtgo_read_bvh")
        links = nodes.view(np.int32)[:, [3, 7]].copy()
        boxes = nodes[:, [0, 1, 2, 4, 5, 6]].copy()
        return boxes, links, inv, aabb

    # ---- diagnostics outside include/rtgo.h (resolved when first used, not declared in load(): SYMBOLS is the header's list) ----
    def build_digest(self, whitted):
        """rtgo_debug_build_digest: one FNV-1a digest per span of what the builds wrote, as a list of ints"""
        fn = self._lib.rtgo_debug_build_digest
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32)]
        out, n = (C.c_uint64 * 4096)(), C.c_uint32(0)
        self._check(fn(self._h, 1 if whitted else 0, out, 4096, C.byref(n)), "rtgo_debug_build_digest")
        return [int(out[k]) for k in range(min(n.value, 4096))]

    def read_build(self, whitted):
        """rtgo_debug_read_build: every span of what the builds wrote for the current scene, as a dict name -> numpy array, in the
        library's order.  float4 arrays come as float32 [n, 4], box lists as float32 [n, 6], qrecs / tidx / clusters / top.inst as 32-bit
        words per row, grid.image as bytes, everything else (meta words, infos) as int32 words (view them as float32 where they are)."""
        fn = self._lib.rtgo_debug_read_build_named
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]
        n_spans = len(self.build_digest(whitted))
        shapes = {"nodes": (np.float32, 4), "prims": (np.float32, 4), "frames": (np.float32, 4), "fnodes": (np.float32, 4), "fprims": (np.float32, 4),
                  "recs": (np.float32, 4), "tris": (np.float32, 4), "tight": (np.float32, 6), "aabb": (np.float32, 6), "qrecs": (np.uint32, 4),
                  "tidx": (np.uint32, 2), "clusters": (np.int32, 4), "inst": (np.uint32, 16), "image": (np.uint8, 0)}
        out = {}
        for k in range(n_spans):
            size, name = C.c_size_t(0), C.create_string_buffer(64)
            self._check(fn(self._h, 1 if whitted else 0, k, None, 0, C.byref(size), name, 64), "rtgo_debug_read_build")
            raw = np.zeros(size.value, np.uint8)
            self._check(fn(self._h, 1 if whitted else 0, k, raw.ctypes.data if size.value else None, raw.nbytes, C.byref(size), None, 0), "rtgo_debug_read_build")
            dt, cols = shapes.get(name.value.decode().split(".")[-1], (np.int32, 0))
            a = raw.view(dt)
            out[name.value.decode()] = a.reshape(-1, cols) if cols else a
        return out


def whitted_instances(instances):
    """instances: a list of (transform, mesh, material_offset) -- transform a row-major 3 x 4 (or 4 x 4, last row ignored) object-to-world
    matrix -- or a structured array with those fields.  Returns a ctypes array of WhittedInstance."""
    n = len(instances)
    arr = (WhittedInstance * max(n, 1))()
    for i in range(n):
        tr, mesh, off = instances[i][0], instances[i][1], instances[i][2]
        arr[i].transform[:] = np.asarray(tr, dtype=np.float32).reshape(-1)[:12].tolist()
        arr[i].mesh = int(mesh)
        arr[i].material_offset = int(off)
    return arr


def device_instances_args(who, device, t):
    """The checks of Context.whitted_set_instances_device on its tensor (needs no context): contiguous, n * 56 bytes, uint8 [n, 56] or
    int32 / float32 [n, 14], on device `device`.  Returns (n, pointer); ValueError otherwise."""
    if not hasattr(t, "data_ptr"):
        raise ValueError("%s: instances must be a torch tensor" % who)
    if not t.is_contiguous():
        raise ValueError("%s: instances must be contiguous" % who)
    cols = {"torch.uint8": 56, "torch.int32": 14, "torch.float32": 14}.get(str(t.dtype))
    if cols is None or t.dim() != 2 or t.shape[1] != cols:
        raise ValueError("%s: instances must be uint8 [n, 56] or int32 / float32 [n, 14] (56 bytes per record), not %s %s"
                         % (who, t.dtype, tuple(t.shape)))
    if not t.is_cuda or t.device.index != device:
        raise ValueError("%s: instances must lie on device %d, not on %s" % (who, device, t.device))
    return t.shape[0], t.data_ptr()


def device_mesh_tensor(who, device, name, t, dtypes, cols):
    """One tensor of Context.whitted_set_scene_device / whitted_set_mesh_device / whitted_set_texcoords_device (needs no context): a
    contiguous torch tensor of one of `dtypes`, [n, cols] (cols = 0: [n]), on device `device`.  Layout first, then where it lies, as
    device_prims_args.  ValueError otherwise."""
    if not hasattr(t, "data_ptr"):
        raise ValueError("%s: %s must be a torch tensor" % (who, name))
    if not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous" % (who, name))
    if str(t.dtype) not in dtypes or t.dim() != (2 if cols else 1) or (cols and t.shape[1] != cols):
        raise ValueError("%s: %s must be %s %s, not %s %s" % (who, name, " or ".join(d[6:] for d in dtypes), "[n, %d]" % cols if cols else "[n]",
                                                              t.dtype, tuple(t.shape)))
    if not t.is_cuda or t.device.index != device:
        raise ValueError("%s: %s must lie on device %d, not on %s" % (who, name, device, t.device))


def device_mesh_args(who, device, positions, normals, texcoords, indices, tri_material):
    """The checks of Context.whitted_set_scene_device (one mesh of it) and whitted_set_mesh_device on their tensors (needs no context):
    positions / normals float32 [nv, 3], texcoords float32 [nv, 2], indices int32 or uint32 [nt, 3], tri_material int32 or uint32 [nt];
    normals, texcoords and tri_material may be None.  Returns (nv, nt, the five pointers or None, in rtgo_whitted_mesh's order);
    ValueError for anything that is not a contiguous tensor of that dtype and shape on device `device`, or whose count disagrees."""
    f32, u32 = ("torch.float32",), ("torch.int32", "torch.uint32")
    spec = (("positions", positions, f32, 3), ("normals", normals, f32, 3), ("texcoords", texcoords, f32, 2), ("indices", indices, u32, 3),
            ("tri_material", tri_material, u32, 0))
    for name, t, dtypes, cols in spec:
        if t is None and name in ("positions", "indices"):
            raise ValueError("%s: %s must be a torch tensor" % (who, name))
        if t is not None:
            device_mesh_tensor(who, device, name, t, dtypes, cols)
    nv, nt = positions.shape[0], indices.shape[0]
    for name, t, want in (("normals", normals, nv), ("texcoords", texcoords, nv), ("tri_material", tri_material, nt)):
        if t is not None and t.shape[0] != want:
            raise ValueError("%s: %s has %d rows, the mesh has %d" % (who, name, t.shape[0], want))
    return nv, nt, [None if t is None else t.data_ptr() for _, t, _, _ in spec]


def instances_tensor(transforms, meshes, material_offsets):
    """rtgo_whitted_instance records packed with torch ops on whatever device the inputs live on: transforms [n, 12] or [n, 3, 4]
    (row-major object-to-world), meshes [n] and material_offsets [n] (integers up to 2^32 - 1: their low 32 bits are stored).  Returns
    float32 [n, 14] with the two integers' bits in columns 12 and 13: byte for byte whitted_instances()'s array, and what
    Context.whitted_set_instances_device takes."""
    import torch
    transforms = transforms.reshape(-1, 12).to(torch.float32)
    n = transforms.shape[0]
    out = torch.empty((n, 14), dtype=torch.float32, device=transforms.device)
    out[:, :12] = transforms
    words = out.view(torch.int32)
    for col, v in ((12, meshes), (13, material_offsets)):
        v = v.reshape(n).to(device=transforms.device, dtype=torch.int64)
        words[:, col] = torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)
    return out


def device_prims_args(who, device, indices, prims, aabbs):
    """The checks of Context.set_scene_device / set_large_scene_device / update_prims_device[_async] on their tensors (needs no context).
    prims: contiguous, k * 108 bytes, uint8 [k, 108] or int32 / float32 [k, 27]; aabbs: contiguous float32 [k, 6] or None; indices:
    contiguous int32 [k] or None (the set calls); all on device `device`.  Returns (k, [indices pointer or None, prims pointer, aabbs
    pointer or None]); ValueError for a tensor that is not on that device, is not contiguous, or has another dtype, shape or byte count."""
    given = [(name, t) for name, t in (("indices", indices), ("prims", prims), ("aabbs", aabbs)) if t is not None or name == "prims"]
    for name, t in given:   # layout first, then where it lies: a tensor of the wrong shape is named as that on any device
        if not hasattr(t, "data_ptr"):
            raise ValueError("%s: %s must be a torch tensor" % (who, name))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (who, name))
    rows = {"torch.uint8": 108, "torch.int32": 27, "torch.float32": 27}.get(str(prims.dtype))
    nbytes = prims.numel() * prims.element_size()
    if rows is None or prims.dim() != 2 or prims.shape[1] != rows:
        raise ValueError("%s: prims must be uint8 [k, 108] or int32 / float32 [k, 27] (108 bytes per record), not %s %s (%d bytes)"
                         % (who, prims.dtype, tuple(prims.shape), nbytes))
    k = nbytes // 108
    if indices is not None:
        if str(indices.dtype) != "torch.int32" or indices.dim() != 1:
            raise ValueError("%s: indices must be an int32 tensor [k]" % who)
        if indices.numel() != k:
            raise ValueError("%s: %d records (%d bytes) for %d indices" % (who, k, nbytes, indices.numel()))
    if aabbs is not None:
        if str(aabbs.dtype) != "torch.float32" or aabbs.dim() != 2 or aabbs.shape[1] != 6:
            raise ValueError("%s: aabbs must be a float32 tensor [k, 6]" % who)
        if aabbs.shape[0] != k:
            raise ValueError("%s: %d boxes (%d bytes) for %d records" % (who, aabbs.shape[0], 24 * aabbs.shape[0], k))
    for name, t in given:
        if not t.is_cuda or t.device.index != device:
            raise ValueError("%s: %s must lie on device %d, not on %s" % (who, name, device, t.device))
    return k, [None if indices is None else indices.data_ptr(), prims.data_ptr(), None if aabbs is None else aabbs.data_ptr()]


def prims_tensor(types, models, materials):
    """rtgo_prim records packed with torch ops on whatever device the inputs live on: types [k] (integers), models [k, 16] (row-major),
    materials [k, 10] = kd(3) kr(3) specularity Le(3).  Returns float32 [k, 27] whose column 0 holds the type's bits: byte for byte the
    PRIM_DTYPE records of Context.set_large_scene, and what the *_device calls take."""
    import torch
    models = models.reshape(-1, 16).to(torch.float32)
    k = models.shape[0]
    out = torch.empty((k, 27), dtype=torch.float32, device=models.device)
    out.view(torch.int32)[:, 0] = types.reshape(k).to(device=models.device, dtype=torch.int32)
    out[:, 1:17] = models
    out[:, 17:27] = materials.reshape(k, 10).to(device=models.device, dtype=torch.float32)
    return out


def make_frame(width, height, sqrt_spp=1, frame_count=0, path=True, ambient=False, window=None, bands=(4, 1, 0),
               max_depth=5, stats=False, reserve_cus=0):
    x0, y0, w, h = window if window is not None else (0, 0, width, height)
    band_h, n_ranks, rank = bands
    return Frame(width, height, sqrt_spp, max_depth, frame_count, int(path), int(ambient), x0, y0, w, h, band_h,
                 n_ranks, rank, int(stats), int(reserve_cus))


def make_whitted_frame(width, height, subframe, window=None, bands=(4, 1, 0), reserve_cus=0):
    """rtgo_whitted_frame: subframe `subframe` of the window (x0, y0, w, h) of a width x height image (None: all of it), the rows of
    band interleave (band_h, n_ranks, rank)"""
    x0, y0, w, h = window if window is not None else (0, 0, width, height)
    band_h, n_ranks, rank = bands
    return WhittedFrame(width, height, subframe, x0, y0, w, h, band_h, n_ranks, rank, int(reserve_cus))
