// rtgo_whitted_inst_update.h -- the kernels of rtgo_whitted_set_instances_device: the instances of an instanced whitted scene taken from
// a device buffer (under OptiX the OptixInstance array of an IAS build input is a device pointer, sutil/Scene.cpp:985-1010).
//
//   inst_prepare_kernel   per instance: what whitted_prepare_instances (rtgo_whitted_host.h) decides and lays out on the host -- the
//                         checks into a verdict of a few words, the InstShade record and the world box into buffers of the call
//   inst_gather_kernel    per leaf position of the top level: the InstWalk record of the instance that sits there
//
// Between the two the host runs whitted_build (RTGO_UPDATE_REBUILD) or refit_kernel (RTGO_UPDATE_REFIT) over the boxes, both unchanged:
// the top level is a structure over boxes like a clustered mesh's mid level.  Included after rtgo_ctx.h: mat3_det_inverse is the host's.
#pragma once

#include "rtgo_ctx.h"

namespace rtgo {
namespace whitted {

constexpr int kInstDwords = 14;   // rtgo_whitted_instance: transform[12], mesh, material_offset
constexpr int kInstStride = 15;   // ... and its stride in LDS: odd, see inst_prepare_kernel
static_assert(sizeof(rtgo_whitted_instance) == kInstDwords * sizeof(unsigned int), "rtgo_whitted_instance is 14 dwords");

// What the two kernels read of a mesh: WhittedMeshInfo without its host-only members, 12 dwords
struct InstMesh {
    float lo[3], hi[3];
    int rec_base, tri_base, vert_base, root, flags;
    unsigned int max_material;
};
constexpr int kInstMeshDwords = 12;
static_assert(sizeof(InstMesh) == kInstMeshDwords * sizeof(unsigned int), "twelve words");

// The verdict: one word per kind of fault, the lowest offending instance (kNoFault: none), as prims_check_kernel's.  A lane reports the
// first check it fails, in whitted_prepare_instances's order, so the lowest entry over all kinds is the instance the host would refuse
// and its kind the reason.  kInstChangedMesh: RTGO_UPDATE_REFIT only (the instance names another mesh than it names in the scene).
enum { kInstBadMesh = 0, kInstChangedMesh = 1, kInstBadMaterial = 2, kInstBadTransform = 3, kInstBadBox = 4, kInstVerdictKinds = 5 };
static_assert(kInstVerdictKinds <= kVerdictWords, "the context's verdict words hold it");

__device__ __forceinline__ bool inst_finite_bits(unsigned int b) { return (b & 0x7F800000u) != 0x7F800000u; }

// Instance i < n: record inst[i] (14 dwords, the host struct's layout).  Writes shade[i], box i (lo xyz, hi xyz) and the index triple
// (2i, 2i + 1, 2i) under which build_kernel and refit_kernel take that box as the degenerate triangle (lo, hi, lo) -- all three are
// buffers of the call, nothing of the scene is written.  old_shade / old_walk: NULL, or (RTGO_UPDATE_REFIT) the scene's InstShade and
// InstWalk arrays: an instance must then name the mesh it names there (a mesh is known by its tri_base: every mesh has triangles), and
// seed[3 pos].w gets the instance at leaf position pos, which is where refit_kernel reads a structure's leaf order from.
//
// A lane that read its own record from global memory would read at a stride of 14 dwords; the workgroup loads its 256 records with
// coalesced dword loads into LDS instead, as prims_check_kernel does, and the mesh table beside them.  In LDS a record takes 15 dwords:
// at the record's own even stride lanes l and l + 16 of a ds_read_b32 would share a bank (14 x 16 = 0 mod 32), at 15 no two lanes of a
// 32-lane group do.  The last workgroup loads the dwords of its own entries only: nothing beyond the caller's n entries is read.
// The arithmetic is whitted_prepare_instances's, operation for operation, in double, one rounding each.
__global__ __launch_bounds__(256) void inst_prepare_kernel(const unsigned int* __restrict__ inst, unsigned int n, const unsigned int* __restrict__ meshes,
                                                           unsigned int n_meshes, unsigned int n_materials, const InstShade* __restrict__ old_shade,
                                                           const InstWalk* __restrict__ old_walk, InstShade* __restrict__ shade, float* __restrict__ boxes,
                                                           unsigned int* __restrict__ idx, float4* __restrict__ seed, unsigned int* __restrict__ verdict)
{
#pragma clang fp contract(off)
    __shared__ unsigned int s_inst[256 * kInstStride];
    __shared__ unsigned int s_mesh[kMaxMeshes * kInstMeshDwords];
    const unsigned int tid = threadIdx.x, base = blockIdx.x * 256u;
    if (base >= n) return;
    const unsigned int here = n - base < 256u ? n - base : 256u;   // this workgroup's entries
    const unsigned int* src = inst + (size_t)base * kInstDwords;
    for (unsigned int d = tid; d < here * kInstDwords; d += 256u) s_inst[(d / kInstDwords) * kInstStride + d % kInstDwords] = src[d];
    for (unsigned int d = tid; d < n_meshes * kInstMeshDwords; d += 256u) s_mesh[d] = meshes[d];
    __syncthreads();
    const unsigned int i = base + tid;
    int kind = -1;
    if (tid < here) {
        const unsigned int* r = s_inst + tid * kInstStride;
        const unsigned int mesh = r[12], material_offset = r[13];
        if (old_walk) seed[3 * (size_t)i] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(old_walk[i].instance));
        idx[3 * (size_t)i + 0] = 2u * i;
        idx[3 * (size_t)i + 1] = 2u * i + 1u;
        idx[3 * (size_t)i + 2] = 2u * i;
        if (mesh >= n_meshes) {
            kind = kInstBadMesh;
        } else {
            const unsigned int* m = s_mesh + mesh * kInstMeshDwords;
            const int tri_base = (int)m[7], vert_base = (int)m[8], flags = (int)m[10];
            if (old_shade && old_shade[i].tri_base != tri_base) kind = kInstChangedMesh;
            else if ((unsigned long long)material_offset + m[11] >= n_materials) kind = kInstBadMaterial;
            if (kind < 0) {
                bool finite = true;
                for (int k = 0; k < 12; ++k) finite = finite && inst_finite_bits(r[k]);
                double A[3][4], B[3][4];   // B: the inverse, adj(A) / det, then -A^-1 t
                for (int q = 0; q < 3; ++q)
                    for (int k = 0; k < 4; ++k) A[q][k] = __uint_as_float(r[4 * q + k]);
                const double det = mat3_det_inverse(A, B);
                if (!finite || !isfinite(det) || fabs(det) < 1e-30) kind = kInstBadTransform;
                for (int q = 0; q < 3; ++q) B[q][3] = -(B[q][0] * A[0][3] + B[q][1] * A[1][3] + B[q][2] * A[2][3]);
                float w2o[12];
                for (int k = 0; k < 12; ++k) {
                    w2o[k] = (float)B[k / 4][k % 4];
                    if (kind < 0 && !inst_finite_bits(__float_as_uint(w2o[k]))) kind = kInstBadTransform;
                }
                float box[6];
                if (kind < 0) {
                    const double mlo[3] = {__uint_as_float(m[0]), __uint_as_float(m[1]), __uint_as_float(m[2])};
                    const double mhi[3] = {__uint_as_float(m[3]), __uint_as_float(m[4]), __uint_as_float(m[5])};
                    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
                    for (int corner = 0; corner < 8; ++corner) {
                        const double x = (corner & 1) ? mhi[0] : mlo[0], y = (corner & 2) ? mhi[1] : mlo[1], z = (corner & 4) ? mhi[2] : mlo[2];
                        for (int q = 0; q < 3; ++q) {
                            const double v = A[q][0] * x + A[q][1] * y + A[q][2] * z + A[q][3];
                            lo[q] = fmin(lo[q], v);
                            hi[q] = fmax(hi[q], v);
                        }
                    }
                    for (int q = 0; q < 3; ++q) {
                        float l = (float)lo[q], h = (float)hi[q];
                        if ((double)l > lo[q]) l = nextafterf(l, -INFINITY);
                        if ((double)h < hi[q]) h = nextafterf(h, INFINITY);
                        if (!inst_finite_bits(__float_as_uint(l)) || !inst_finite_bits(__float_as_uint(h))) kind = kInstBadBox;
                        box[q] = l;
                        box[3 + q] = h;
                    }
                }
                if (kind < 0) {
                    float4* out = reinterpret_cast<float4*>(shade + i);
                    for (int q = 0; q < 3; ++q) {
                        out[q] = make_float4(__uint_as_float(r[4 * q]), __uint_as_float(r[4 * q + 1]), __uint_as_float(r[4 * q + 2]), __uint_as_float(r[4 * q + 3]));
                        out[3 + q] = make_float4(w2o[4 * q], w2o[4 * q + 1], w2o[4 * q + 2], w2o[4 * q + 3]);
                    }
                    out[6] = make_float4(__int_as_float((int)material_offset), __int_as_float(vert_base), __int_as_float(tri_base), __int_as_float(flags));
                    for (int q = 0; q < 6; ++q) boxes[6 * (size_t)i + q] = box[q];
                }
            }
        }
    }
    // the lowest offending entry of the wave, one atomic per wave and kind
    if (!__any(kind >= 0)) return;
    const unsigned int lane = tid & 63u;
    for (int q = 0; q < kInstVerdictKinds; ++q) {
        const unsigned long long b = __ballot(kind == q);
        if (b != 0 && lane == (unsigned int)(__ffsll((long long)b) - 1)) atomicMin(&verdict[q], i);
    }
}

// Leaf position pos < n of the top level: walk[pos] = {shade[i].w2o, the mesh's rec_base, tri_base, root, i} for the instance i that sits
// there.  order: the triangles whitted_build wrote for the boxes, whose first corners carry i in .w (RTGO_UPDATE_REBUILD: read where they
// lie), or NULL: walk[pos].instance as it is (RTGO_UPDATE_REFIT: the leaf order stays).  inst: the caller's records, for i's mesh (checked
// by inst_prepare_kernel before this runs).
__global__ __launch_bounds__(256) void inst_gather_kernel(const float4* __restrict__ order, const InstShade* __restrict__ shade,
                                                          const unsigned int* __restrict__ inst, const InstMesh* __restrict__ meshes, unsigned int n,
                                                          InstWalk* walk)
{
    const unsigned int pos = blockIdx.x * 256u + threadIdx.x;
    if (pos >= n) return;
    const int i = order ? __float_as_int(order[3 * (size_t)pos].w) : walk[pos].instance;
    if ((unsigned int)i >= n) return;   // (a leaf order is a permutation of [0, n): never taken)
    const InstMesh m = meshes[inst[(size_t)i * kInstDwords + 12]];
    const InstShade& sh = shade[i];
    float4* out = reinterpret_cast<float4*>(walk + pos);
    out[0] = sh.w2o[0];
    out[1] = sh.w2o[1];
    out[2] = sh.w2o[2];
    out[3] = make_float4(__int_as_float(m.rec_base), __int_as_float(m.tri_base), __int_as_float(m.root), __int_as_float(i));
}

// ---- the refit of rtgo_whitted_refit_instances_device_async: inst_prepare_kernel into buffers the scene owns, its verdict
// in a slot of the context's ring and never read by the host in between; the two kernels below do every write to the scene, and each reads
// that verdict first.  The kernel boundary after inst_prepare_kernel is what makes the verdict complete and visible to them
// (rtgo_large.h's argument for large_update_staged_kernel).

// the gate: the same address in every lane, so five scalar loads per wave
__device__ __forceinline__ bool inst_verdict_clean(const unsigned int* __restrict__ verdict)
{
    unsigned int all = kNoFault;
    for (int q = 0; q < kInstVerdictKinds; ++q) all &= verdict[q];
    return all == kNoFault;
}

constexpr int kInstShadeQuads = 7;   // InstShade: seven float4
static_assert(sizeof(InstShade) == kInstShadeQuads * sizeof(float4), "InstShade is seven float4");

// What a clean verdict lets into the scene, everything but the top level's records: shade[0, n) = staged[0, n) (inst_prepare_kernel's
// records); walk[pos] as inst_gather_kernel writes it under RTGO_UPDATE_REFIT (the leaf order stays: walk[pos].instance as it is, read by
// the lane that rewrites it); kept[0, 14 n) = the caller's records, the copy the host adopts when it next needs the instances; and
// *applied, which counts the updates that got this far, bumped once.  The two copies are flat streams -- the 112-byte records as float4,
// the 56-byte ones as dwords (the caller's buffer is 4-byte aligned, no more) -- lane after lane over the arrays, not a lane per record
// at a stride of 28 or 14 dwords; so nothing is staged in LDS.  The grid is inst_prepare_kernel's: one lane per instance.
__global__ __launch_bounds__(256) void inst_commit_kernel(const unsigned int* __restrict__ verdict, const unsigned int* __restrict__ inst,
                                                          const InstShade* __restrict__ staged, const InstMesh* __restrict__ meshes, unsigned int n,
                                                          InstShade* __restrict__ shade, InstWalk* walk, unsigned int* __restrict__ kept,
                                                          unsigned int* __restrict__ applied)
{
    if (!inst_verdict_clean(verdict)) return;
    const unsigned int g = blockIdx.x * 256u + threadIdx.x, lanes = gridDim.x * 256u;
    const float4* __restrict__ src = reinterpret_cast<const float4*>(staged);
    float4* __restrict__ dst = reinterpret_cast<float4*>(shade);
    for (unsigned int k = g; k < n * kInstShadeQuads; k += lanes) dst[k] = src[k];
    for (unsigned int k = g; k < n * kInstDwords; k += lanes) kept[k] = inst[k];
    if (g == 0) atomicAdd(applied, 1u);
    if (g >= n) return;
    const int i = walk[g].instance;
    if ((unsigned int)i >= n) return;   // (a leaf order is a permutation of [0, n): never taken)
    const InstMesh m = meshes[inst[(size_t)i * kInstDwords + 12]];
    const InstShade& sh = staged[i];
    float4* out = reinterpret_cast<float4*>(walk + g);
    out[0] = sh.w2o[0];
    out[1] = sh.w2o[1];
    out[2] = sh.w2o[2];
    out[3] = make_float4(__int_as_float(m.rec_base), __int_as_float(m.tri_base), __int_as_float(m.root), __int_as_float(i));
}

// refit_kernel behind the gate, over the staged boxes and index triples and the scene's top-level records: one workgroup of
// kBuildThreads, launched only for a top level that has records.  refit_structure clears done[0, n_recs) itself before its first pass,
// and writes out_meta (a block the scene owns) like everything else only once the verdict has been read clean.
__global__ __launch_bounds__(kBuildThreads) void inst_refit_gated_kernel(const unsigned int* __restrict__ verdict, const float* __restrict__ boxes,
                                                                         const unsigned int* __restrict__ idx, int n, int n_recs, int walk_depth,
                                                                         float4* recs, float4* tris, uint4* qrecs, int* done,
                                                                         WhittedBuildMeta* __restrict__ out_meta)
{
    __shared__ float s_red[6][kBuildThreads];
    if (!inst_verdict_clean(verdict)) return;
    refit_structure<false>({boxes, idx, n, n_recs, walk_depth, recs, tris, qrecs, done, out_meta}, s_red);
}

}  // namespace whitted
}  // namespace rtgo
