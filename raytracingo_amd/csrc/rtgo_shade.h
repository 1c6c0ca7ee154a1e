// rtgo_shade.h -- the kernel behind rtgo_shade_rays (include/rtgo.h): __closesthit__ch, __closesthit__full_occlusion and __miss__ms
// (kernel.cu:419-549) for rays from device memory instead of from __raygen__rg.  Under OptiX: the caller's own raygen program over the
// scene's hit and miss programs.  Nothing here is new arithmetic: the walk is closest_hit<false> over the canonical LBVH, as in
// trace_rays_kernel (rtgo_trace.h), whose frame this is; the shading is rtgo_ray_shade.inc, the text the render kernels run, under
// MS = 6 (the canonical records); the fold and make_color are write_pixel's and store_pixel's operations -- so a batch of frame f's
// pinhole rays of sqrt_spp 1, with the seeds as they stand after the two jitter draws and sample_index f, leaves the bits of rtgo_launch
// in the caller's two buffers.
//
// One lane holds one ray and runs its whole path: trace, shade, trace the occlusion or the bounce ray, ... until the path ends, the
// lock-step loop of rtgo_render_body.inc without its raygen, units and work queue.  Lane i reads ray i as two float4 (and seed i, when
// seeds are given), and writes accum[i] (float4) and image[i] (uchar4, when asked for): all coalesced, all bounded by i < n.  An
// invalid ray enters no walk.
#pragma once

#include "rtgo_trace.h"

namespace rtgo {

struct ShadeParams {
    const float4* nodes;        // canonical LBVH and primitive records (LaunchParams::nodes / prims)
    const float4* prims;
    const LightRec* lights;     // the context's surface lights (kMaxLights records)
    const float4* rays;         // 2 float4 per ray
    const unsigned int* seeds;  // one per ray, or null: tea<16>(i, sample_index)
    float4* accum;              // one per ray
    uchar4* image;              // one per ray, or null
    unsigned long long* counters;   // [0] rays_total [1] rays_occlusion
    unsigned int n;
    unsigned int sample_index;  // 0: accum = result; f > 0: write_pixel's step for frame f
    int n_nodes, n_prims, n_lights;
    int stack_depth;            // per-lane LDS stack entries (float2 each)
    int max_depth, ambient;     // Params::maxTraceDepth, Params::useAmbientLight
    v3 bg;
};

// rtgo_ray's rule and a unit direction: the shader places a hit at o + t d in path mode and at o + t normalize(d) in distributed mode
__device__ __forceinline__ bool shade_ray_valid(const float4 a, const float4 b)
{
    return trace_ray_valid(a, b) && fabsf((b.x * b.x + b.y * b.y + b.z * b.z) - 1.0f) <= 1e-5f;
}

// LDS: [nodes, 2 float4 each][records, 6 float4 each] (SCENE_IN_LDS: the render kernel's canonical image; otherwise both are read from
// global memory, render_kernel's GLOBAL way) [stacks, entry e of a lane at [e << bshift]] [lights].  The per-level path records stay in
// registers in both modes (LVLDS off): distributed mode fits 111 VGPRs with them, and the stacks' 192 bytes a lane already hold a CU
// to 13 waves -- with the records in LDS as well (80 bytes a lane more) balls in distributed mode ran at 4 waves a CU and twice the time.
template <bool PATH, bool SCENE_IN_LDS>
__global__ __launch_bounds__(kMaxBlock) void shade_rays_kernel(const ShadeParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sh_smem[];
    constexpr int MS = 6;
    constexpr bool FRAMES = false;      // (the per-hit frame: the same bits as the precomputed one, and no frame table to stage)
    constexpr bool LVLDS = false;
    constexpr bool FOLDLATE = false;    // (a path folds its level records where it ends)
    constexpr bool UNIT16 = false;      // (... and there are no LDS records to address)
    constexpr int LVW = PATH ? 3 : 4;
    const int tid = (int)threadIdx.x, block = (int)blockDim.x;
    float4* s_scene = reinterpret_cast<float4*>(sh_smem);
    const float4* nodes = SCENE_IN_LDS ? static_cast<const float4*>(s_scene) : p.nodes;
    const float4* prims = SCENE_IN_LDS ? static_cast<const float4*>(s_scene + 2 * p.n_nodes) : p.prims;
    const float4* s_mat = prims + 3;    // material rows of a canonical record: (kd|spec, kr|type, Le)
    const float4* s_frame = nullptr;
    float2* s_stack_base = reinterpret_cast<float2*>(SCENE_IN_LDS ? s_scene + 2 * p.n_nodes + 6 * p.n_prims : s_scene);
    float2* s_stack = s_stack_base + tid;
    const int bshift = 31 - __clz(block);   // (the workgroup is a power of two)
    LightRec* s_lights = reinterpret_cast<LightRec*>(s_stack_base + (size_t)p.stack_depth * block);
    float* s_lv = nullptr;              // (LVLDS off: the fragment's LDS form of the level records is not instantiated)
    if (SCENE_IN_LDS) {
        for (int i = tid; i < 2 * p.n_nodes; i += block) s_scene[i] = p.nodes[i];
        for (int i = tid; i < 6 * p.n_prims; i += block) s_scene[2 * p.n_nodes + i] = p.prims[i];
    }
    {
        const float* src = reinterpret_cast<const float*>(p.lights);
        float* dst = reinterpret_cast<float*>(s_lights);
        for (int i = tid; i < p.n_lights * 16; i += block) dst[i] = src[i];
    }
    __syncthreads();

    unsigned int c_rays = 0, c_occl = 0;   // the rays the paths sent beyond the batch's own (the host's arithmetic): bounces and occlusion
    const unsigned int step = gridDim.x * (unsigned int)block;   // (n <= 2^30 and the grid is a few workgroups per CU: i + step stays below 2^32)
    for (unsigned int i = blockIdx.x * (unsigned int)block + (unsigned int)tid; i < p.n; i += step) {
        const float4 a = p.rays[2 * (size_t)i + 0], b = p.rays[2 * (size_t)i + 1];
        if (!shade_ray_valid(a, b)) {
            if (p.sample_index == 0u) {
                p.accum[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p.image) p.image[i] = make_uchar4(0u, 0u, 0u, 0u);
            }
            continue;
        }
        // trace(...) of __raygen__rg at depth 0 (kernel.cu:46-79): the seed goes in by value, after whatever the caller's raygen drew
        bool active = true;
        int depth = 0;
        int phase = 0;                 // distributed mode: 0 = radiance ray in flight, 1 = shadow ray in flight
        unsigned int seed = p.seeds ? p.seeds[i] : tea16(i, p.sample_index);
        v3 ro = mk(a.x, a.y, a.z), rd = mk(b.x, b.y, b.z);
        float tmin = a.w, tmax = b.w;
        v3 result = mk(0.0f, 0.0f, 0.0f);
        v3 lvA[kMaxLevels];
        int lvPrim[kMaxLevels];
        int ended_in = kEndsInZero;    // (FOLDLATE alone reads it)
#pragma unroll
        for (int q = 0; q < kMaxLevels; ++q) {
            lvA[q] = mk(0, 0, 0);
            lvPrim[q] = 0;
        }
        v3 sN = mk(0, 0, 0), sRr = mk(0, 0, 0);
        float sDist = 0.0f;
        int sPrim = 0, sLight = 0;
        c_rays -= 1;   // (the path's first ray is one of the batch's n)
        while (__ballot(active) != 0ull) {
            if (active) {
                Hit h;
                unsigned int c_nodes = 0, c_tests = 0;
                c_rays += 1;
                const bool hit = closest_hit<false>(nodes, prims, s_stack, bshift, ro, rd, tmin, tmax, h, c_nodes, c_tests);
#include "rtgo_ray_shade.inc"
            }
        }
        // __raygen__rg's one sample (kernel.cu:232-237): color = 0 + payload, times 1 / (1 * 1); then write_pixel's step and store_pixel
        v3 acc = vscale(vadd(mk(0.0f, 0.0f, 0.0f), result), 1.0f / 1.0f);
        if (p.sample_index > 0u) {
            const float4 prev4 = p.accum[i];
            const v3 prev = mk(prev4.x, prev4.y, prev4.z);
            acc = vadd(prev, vscale(vsub(acc, prev), 1.0f / (float)(p.sample_index + 1u)));
        }
        p.accum[i] = make_float4(acc.x, acc.y, acc.z, 1.0f);
        if (p.image)
            p.image[i] = make_uchar4((unsigned char)(clampf(acc.x, 0.0f, 1.0f) * 255.0f), (unsigned char)(clampf(acc.y, 0.0f, 1.0f) * 255.0f),
                                     (unsigned char)(clampf(acc.z, 0.0f, 1.0f) * 255.0f), 255u);
    }
    // one atomic per wave per counter, as the render kernels sum theirs
    c_rays = wave_sum(c_rays);
    c_occl = wave_sum(c_occl);
    if ((tid & 63) == 0) {
        atomicAdd(&p.counters[0], (unsigned long long)c_rays);
        if (!PATH) atomicAdd(&p.counters[1], (unsigned long long)c_occl);
    }
}

}  // namespace rtgo
