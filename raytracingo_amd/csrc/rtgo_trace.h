// rtgo_trace.h -- ray queries: the kernels behind rtgo_trace_rays and rtgo_whitted_trace_rays (include/rtgo.h).  The rays come from
// device memory instead of from a camera (under OptiX: the caller's own raygen program calling optixTrace); the walks are the render
// kernels' own -- closest_hit<false> over the canonical LBVH, whitted::trace over one mesh, whitted::trace_inst over an instanced or
// clustered scene -- so acceptance (tmin < t < tmax) and the tie rules are theirs, bit for bit.
//
// One lane holds one ray.  Lane i reads ray i as two float4 (origin, tmin) (dir, tmax) and writes hit i as two float4
// (t, prim, instance, u) (v, n.xyz): both coalesced, 32 bytes a lane.  A grid-stride loop takes a workgroup through the batch.
// A ray that is not valid (rtgo_ray's rules) gets RTGO_HIT_INVALID without entering a walk: the walks' loops are finite whatever they
// compare, but their reciprocals and quotients are only meaningful for finite rays.
#pragma once

#include "rtgo_device.h"
#include "rtgo_whitted_inst.h"

namespace rtgo {

constexpr int kTraceHitMiss = -1, kTraceHitInvalid = -2;   // RTGO_HIT_MISS, RTGO_HIT_INVALID

struct TraceParams {
    const float4* nodes;    // canonical LBVH and primitive records (LaunchParams::nodes / prims)
    const float4* prims;
    const float4* rays;     // 2 float4 per ray
    float4* hits;           // 2 float4 per ray
    unsigned int n;
    int n_nodes, n_prims;
    int stack_depth;        // per-lane LDS stack entries (float2 each)
};

// rtgo_ray's validity rule: every component finite, dir != 0, tmin >= 0, tmax > tmin (a NaN fails the first test)
__device__ __forceinline__ bool trace_ray_valid(const float4 a, const float4 b)
{
    const bool finite = isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(a.w) && isfinite(b.x) && isfinite(b.y) && isfinite(b.z) && isfinite(b.w);
    return finite && (b.x != 0.0f || b.y != 0.0f || b.z != 0.0f) && a.w >= 0.0f && b.w > a.w;
}

__device__ __forceinline__ void trace_store(float4* __restrict__ hits, unsigned int i, float t, int prim, int instance, float u, float v, v3 n)
{
    hits[2 * (size_t)i + 0] = make_float4(t, __int_as_float(prim), __int_as_float(instance), u);
    hits[2 * (size_t)i + 1] = make_float4(v, n.x, n.y, n.z);
}

// The analytic path (scenes of rtgo_set_scene / rtgo_set_large_scene).
// SCENE_IN_LDS: the workgroup stages nodes and primitive records in LDS, as render_kernel's canonical instantiation does, and walks
// them there: [nodes, 2 float4 each][records, 6 float4 each][stacks].  Otherwise the walk reads both from global memory (render_kernel's
// GLOBAL way) and LDS holds the stacks alone.  Same walk, same records: the same bits.
template <bool SCENE_IN_LDS>
__global__ __launch_bounds__(kMaxBlock) void trace_rays_kernel(const TraceParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char tr_smem[];
    const int tid = (int)threadIdx.x, block = (int)blockDim.x;
    float4* s_scene = reinterpret_cast<float4*>(tr_smem);
    const float4* nodes = SCENE_IN_LDS ? static_cast<const float4*>(s_scene) : p.nodes;
    const float4* prims = SCENE_IN_LDS ? static_cast<const float4*>(s_scene + 2 * p.n_nodes) : p.prims;
    float2* s_stack = reinterpret_cast<float2*>(SCENE_IN_LDS ? s_scene + 2 * p.n_nodes + 6 * p.n_prims : s_scene) + tid;
    const int bshift = 31 - __clz(block);   // per-lane stack entry e lives at [e << bshift] (the workgroup is a power of two)
    if (SCENE_IN_LDS) {
        for (int i = tid; i < 2 * p.n_nodes; i += block) s_scene[i] = p.nodes[i];
        for (int i = tid; i < 6 * p.n_prims; i += block) s_scene[2 * p.n_nodes + i] = p.prims[i];
        __syncthreads();
    }
    const unsigned int step = gridDim.x * (unsigned int)block;   // (n <= 2^30 and the grid is a few workgroups per CU: i + step stays below 2^32)
    for (unsigned int i = blockIdx.x * (unsigned int)block + (unsigned int)tid; i < p.n; i += step) {
        const float4 a = p.rays[2 * (size_t)i + 0], b = p.rays[2 * (size_t)i + 1];
        if (!trace_ray_valid(a, b)) {
            trace_store(p.hits, i, 0.0f, kTraceHitInvalid, 0, 0.0f, 0.0f, mk(0.0f, 0.0f, 0.0f));
            continue;
        }
        Hit h;
        unsigned int c_nodes = 0, c_tests = 0;
        if (closest_hit<false>(nodes, prims, s_stack, bshift, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), a.w, b.w, h, c_nodes, c_tests))
            trace_store(p.hits, i, h.t, h.prim, -1, 0.0f, 0.0f, h.n);
        else
            trace_store(p.hits, i, b.w, kTraceHitMiss, 0, 0.0f, 0.0f, mk(0.0f, 0.0f, 0.0f));
    }
}

namespace whitted {

// what the walk of a whitted_trace_kernel is: one mesh in world space (whitted::trace, records through L2), or an instanced scene
// (trace_inst) without / with clustered meshes, its top level read through L2 or staged in LDS
constexpr int kTraceMesh = 0, kTraceInst = 1, kTraceInstLds = 2, kTraceClustered = 3, kTraceClusteredLds = 4;

struct TraceRaysParams {
    Params mesh;            // kTraceMesh: recs, tris, n_recs, n_triangles (the frame and the shading arrays stay zero)
    InstParams inst;        // the others: top_recs, inst, n_top_recs, n_instances, recs, tris, clusters
    const float4* rays;
    float4* hits;
    unsigned int n;
};

// The triangle path (rtgo_whitted_set_mesh / rtgo_whitted_set_scene).  LDS: [top records][InstWalk] (the *Lds kinds) then the lanes'
// 2-byte stacks, entry e of a lane at [e * workgroup size] as in the render kernels.
// ANY: terminate on the first accepted hit (the occlusion rays' instantiations of the walks).
template <int KIND, bool ANY>
__global__ __launch_bounds__(kRenderBlock) void whitted_trace_kernel(const TraceRaysParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char wt_smem[];
    constexpr bool kTopInLds = KIND == kTraceInstLds || KIND == kTraceClusteredLds;
    constexpr bool kClustered = KIND == kTraceClustered || KIND == kTraceClusteredLds;
    const int stride = (int)blockDim.x;
    float4* s_top = reinterpret_cast<float4*>(wt_smem);
    InstWalk* s_inst = reinterpret_cast<InstWalk*>(s_top + 4 * p.inst.n_top_recs);
    unsigned short* s_stack = (kTopInLds ? reinterpret_cast<unsigned short*>(s_inst + p.inst.n_instances) : reinterpret_cast<unsigned short*>(wt_smem)) + threadIdx.x;
    if (kTopInLds) {
        for (int i = (int)threadIdx.x; i < 4 * p.inst.n_top_recs; i += stride) s_top[i] = p.inst.top_recs[i];
        for (int i = (int)threadIdx.x; i < p.inst.n_instances; i += stride) s_inst[i] = p.inst.inst[i];
        __syncthreads();
    }
    const float4* top = kTopInLds ? static_cast<const float4*>(s_top) : p.inst.top_recs;
    const InstWalk* inst = kTopInLds ? static_cast<const InstWalk*>(s_inst) : p.inst.inst;
    const unsigned int step = gridDim.x * (unsigned int)stride;
    for (unsigned int i = blockIdx.x * (unsigned int)stride + threadIdx.x; i < p.n; i += step) {
        const float4 a = p.rays[2 * (size_t)i + 0], b = p.rays[2 * (size_t)i + 1];
        const v3 zero = mk(0.0f, 0.0f, 0.0f);
        if (!trace_ray_valid(a, b)) {
            trace_store(p.hits, i, 0.0f, kTraceHitInvalid, 0, 0.0f, 0.0f, zero);
            continue;
        }
        const v3 o = mk(a.x, a.y, a.z), d = mk(b.x, b.y, b.z);
        int tri = 0, instance = 0, pos;
        float t, u, v;
        bool hit;
        if constexpr (KIND == kTraceMesh) {
            hit = trace<ANY>(p.mesh, p.mesh.recs, s_stack, stride, o, d, a.w, b.w, tri, pos, t, u, v);
        } else {
            InstKey<kClustered> key;
            hit = trace_inst<ANY, kClustered>(p.inst, top, inst, s_stack, stride, o, d, a.w, b.w, key, pos, t, u, v);
            if constexpr (kClustered) {
                instance = (int)(key >> 32);
                tri = (int)(key & 0xFFFFFFFF);
            } else {
                instance = key >> kInstShift;
                tri = key & ((1 << kInstShift) - 1);
            }
        }
        if (hit) trace_store(p.hits, i, t, tri, instance, u, v, zero);
        else trace_store(p.hits, i, b.w, kTraceHitMiss, 0, 0.0f, 0.0f, zero);
    }
}

}  // namespace whitted
}  // namespace rtgo
