// rtgo_whitted_shade.h -- the kernel behind rtgo_whitted_shade_rays (include/rtgo.h): __closesthit__radiance and
// __miss__constant_radiance (rtgo_whitted.h) for rays from device memory instead of from __raygen__pinhole.  Under OptiX: the caller's own
// raygen program over the scene's closest-hit program.  Nothing here is new arithmetic: the closest walk and the occlusion walk are the
// render kernels' (whitted::trace / trace_inst), hit geometry and shading are theirs (mesh_shade_hit / inst_shade_hit), running_mean() and
// make_color() are the ones every launch goes through -- so a batch of subframe s's pinhole rays with sample_index s leaves the bits of
// rtgo_whitted_launch in the caller's two buffers.
//
// One lane holds one ray, as in whitted_trace_kernel (rtgo_trace.h), whose kinds, LDS image and grid-stride loop these are.  Lane i reads
// ray i as two float4, walks, shades, and writes accum[i] (float4) and image[i] (uchar4, when asked for): all coalesced, bounded by i < n.
// An invalid ray (rtgo_ray's rule) enters no walk.
#pragma once

#include "rtgo_trace.h"

namespace rtgo {
namespace whitted {

struct ShadeRaysParams {
    Params mesh;            // kTraceMesh: the scene and the frame (of the frame: mat_tex, materials, lights, n_lights, miss, counters)
    InstParams inst;        // the others: the same
    const float4* rays;     // 2 float4 per ray
    float4* accum;          // one per ray
    uchar4* image;          // one per ray, or null
    unsigned int n;
    unsigned int sample_index;   // 0: accum = result; k > 0: accum = running_mean(accum, result, k)
};

template <int KIND>
__global__ __launch_bounds__(kRenderBlock) void whitted_shade_kernel(const ShadeRaysParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ws_smem[];
    constexpr bool kTopInLds = KIND == kTraceInstLds || KIND == kTraceClusteredLds;
    constexpr bool kClustered = KIND == kTraceClustered || KIND == kTraceClusteredLds;
    const int stride = (int)blockDim.x;
    float4* s_top = reinterpret_cast<float4*>(ws_smem);
    InstWalk* s_inst = reinterpret_cast<InstWalk*>(s_top + 4 * p.inst.n_top_recs);
    unsigned short* s_stack = (kTopInLds ? reinterpret_cast<unsigned short*>(s_inst + p.inst.n_instances) : reinterpret_cast<unsigned short*>(ws_smem)) + threadIdx.x;
    if (kTopInLds) {
        for (int i = (int)threadIdx.x; i < 4 * p.inst.n_top_recs; i += stride) s_top[i] = p.inst.top_recs[i];
        for (int i = (int)threadIdx.x; i < p.inst.n_instances; i += stride) s_inst[i] = p.inst.inst[i];
        __syncthreads();
    }
    const float4* top = kTopInLds ? static_cast<const float4*>(s_top) : p.inst.top_recs;
    const InstWalk* inst = kTopInLds ? static_cast<const InstWalk*>(s_inst) : p.inst.inst;
    const Frame& f = KIND == kTraceMesh ? p.mesh.frame : p.inst.frame;
    auto occluded = [&](v3 o, v3 d, float t0, float t1) -> bool {
        int pos;
        float t, u, v;
        if constexpr (KIND == kTraceMesh) {
            int tri;
            return trace<true>(p.mesh, p.mesh.recs, s_stack, stride, o, d, t0, t1, tri, pos, t, u, v);
        } else {
            InstKey<kClustered> key;
            return trace_inst<true, kClustered>(p.inst, top, inst, s_stack, stride, o, d, t0, t1, key, pos, t, u, v);
        }
    };
    Rays rays;   // the occlusion rays shade() sends (the batch's own n rays are the host's arithmetic, as for the trace calls)
    const unsigned int step = gridDim.x * (unsigned int)stride;   // (n <= 2^30: i + step stays below 2^32)
    for (unsigned int i = blockIdx.x * (unsigned int)stride + threadIdx.x; i < p.n; i += step) {
        const float4 a = p.rays[2 * (size_t)i + 0], b = p.rays[2 * (size_t)i + 1];
        if (!trace_ray_valid(a, b)) {
            if (p.sample_index == 0u) {
                p.accum[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p.image) p.image[i] = make_uchar4(0u, 0u, 0u, 0u);
            }
            continue;
        }
        const v3 o = mk(a.x, a.y, a.z), d = mk(b.x, b.y, b.z);
        v3 result = f.miss;   // __miss__constant_radiance (read ahead of the walk, as the render kernels do)
        int tpos;
        float t, bu, bv;
        if constexpr (KIND == kTraceMesh) {
            int tri;
            if (trace<false>(p.mesh, p.mesh.recs, s_stack, stride, o, d, a.w, b.w, tri, tpos, t, bu, bv))
                result = mesh_shade_hit<kAllInL2>(p.mesh, nullptr, nullptr, tri, tpos, bu, bv, d, occluded, rays);
        } else {
            InstKey<kClustered> key;
            if (trace_inst<false, kClustered>(p.inst, top, inst, s_stack, stride, o, d, a.w, b.w, key, tpos, t, bu, bv))
                result = inst_shade_hit<kClustered>(p.inst, key, tpos, bu, bv, d, occluded, rays);
        }
        // accumulate()'s fold and stores, over the caller's buffers
        v3 acc = result;
        if (p.sample_index > 0u) {
            const float4 prev = p.accum[i];
            acc = running_mean(mk(prev.x, prev.y, prev.z), acc, p.sample_index);
        }
        p.accum[i] = make_float4(acc.x, acc.y, acc.z, 1.0f);
        if (p.image) p.image[i] = make_color(acc);
    }
    const unsigned int total = wave_sum(rays.total), occlusion = wave_sum(rays.occlusion);
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(&f.counters[0], (unsigned long long)total);
        atomicAdd(&f.counters[1], (unsigned long long)occlusion);
    }
}

}  // namespace whitted
}  // namespace rtgo
