// rtgo_large.h -- the device-wide build of a scene of rtgo_set_large_scene (beyond build_kernel's one workgroup of kMaxPrims threads).
// It builds the canonical LBVH of build_kernel / oracle_lbvh_build bit for bit, in global memory, with the same __device__ functions:
//   large_prep_kernel     per primitive: the 6-float4 record (inverse_rows012, store_prim_record) and, without caller boxes, the CubeBox
//                         box (cube_aabb)
//   whitted::big_bounds_final_kernel over the boxes: the scene bounds (exact min / max)
//   large_keys_kernel     the 30-bit Morton code of each box centre (morton_cell, morton3), key = code << 32 | index; then the four stable
//                         radix passes of rtgo_whitted_big.h over the code's bytes: the (code, index) order
//   large_karras_kernel   one thread per internal node (karras_node): links and parents; leaves are nodes n-1+j, node 0 the root
//   large_depth_kernel    every node's depth (its parent chain), the leaves' boxes and links, and the largest leaf depth
//   large_fit_kernel      one launch per tree level, deepest first: node box = fminf / fmaxf of its two children's, in build_kernel's
//                         operand order.  The kernel boundary between two levels is what makes a child box written by another
//                         workgroup (on another XCD's L2) visible to its parent's: no inter-workgroup hand-off inside a launch.
#pragma once

#include "rtgo_device.h"
#include "rtgo_whitted_big.h"

namespace rtgo {

constexpr int kLargeMaxDepth = 64;   // per-lane LDS stack entries of the global-memory walk: deeper trees are refused

__global__ __launch_bounds__(256) void large_prep_kernel(const PrimIn* __restrict__ prims, float* __restrict__ aabb_io, int have_aabb, int n,
                                                         float4* __restrict__ out_prims)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const PrimIn P = prims[i];
    float inv[12];
    inverse_rows012(P.M, inv);
    store_prim_record(out_prims + 6 * (size_t)i, P, inv);
    if (!have_aabb) {
        float bb[6];
        cube_aabb(P.M, bb);
        for (int a = 0; a < 6; ++a) aabb_io[6 * (size_t)i + a] = bb[a];
    }
}

__global__ __launch_bounds__(256) void large_keys_kernel(const float* __restrict__ aabb, int n, const float* __restrict__ bounds,
                                                         unsigned long long* __restrict__ keys)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned int q[3];
    for (int a = 0; a < 3; ++a) {
        const float c = (aabb[6 * (size_t)i + a] + aabb[6 * (size_t)i + 3 + a]) * 0.5f;
        q[a] = morton_cell(c, bounds[a], bounds[3 + a] - bounds[a]);
    }
    keys[i] = ((unsigned long long)morton3(q) << 32) | (unsigned int)i;
}

// parent[0] = -1 (the root); every other node gets its parent from the one internal node that links it
__global__ __launch_bounds__(256) void large_karras_kernel(const unsigned long long* __restrict__ keys, int n, int* __restrict__ left,
                                                           int* __restrict__ right, int* __restrict__ parent)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) parent[0] = -1;
    if (i >= n - 1) return;
    int l, r, lo, hi;
    karras_node(keys, n, i, l, r, lo, hi);
    left[i] = l;
    right[i] = r;
    parent[l] = i;
    parent[r] = i;
}

// node k of the 2n-1: its depth (internal nodes -> depth[k]); a leaf also writes its node record and raises *max_depth.  A chain longer
// than kLargeMaxDepth stops counting there (the host refuses such a tree; the walk up cannot run away either).
__global__ __launch_bounds__(256) void large_depth_kernel(const unsigned long long* __restrict__ keys, int n, const float* __restrict__ aabb,
                                                          const int* __restrict__ parent, int* __restrict__ depth, float4* __restrict__ nodes,
                                                          int* __restrict__ max_depth)
{
    __shared__ int s_max;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    if (k < 2 * n - 1) {
        int d = 0;
        for (int q = parent[k]; q >= 0 && q < n - 1 && d <= kLargeMaxDepth; q = parent[q]) ++d;
        if (k < n - 1) {
            depth[k] = d;
        } else {
            const int prim = (int)(keys[k - (n - 1)] & 0xFFFFFFFFull);
            const float* b = aabb + 6 * (size_t)prim;
            nodes[2 * (size_t)k + 0] = make_float4(b[0], b[1], b[2], __int_as_float(prim));
            nodes[2 * (size_t)k + 1] = make_float4(b[3], b[4], b[5], __int_as_float(-1));
            atomicMax(&s_max, d);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(max_depth, s_max);
}

// the internal nodes at depth `level`: their children (deeper) were written by earlier launches
__global__ __launch_bounds__(256) void large_fit_kernel(const int* __restrict__ left, const int* __restrict__ right, const int* __restrict__ depth,
                                                        int n_internal, int level, float4* __restrict__ nodes)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_internal || depth[i] != level) return;
    const int L = left[i], R = right[i];
    const float4 l0 = nodes[2 * (size_t)L], l1 = nodes[2 * (size_t)L + 1], r0 = nodes[2 * (size_t)R], r1 = nodes[2 * (size_t)R + 1];
    nodes[2 * (size_t)i + 0] = make_float4(fminf(l0.x, r0.x), fminf(l0.y, r0.y), fminf(l0.z, r0.z), __int_as_float(L));
    nodes[2 * (size_t)i + 1] = make_float4(fmaxf(l1.x, r1.x), fmaxf(l1.y, r1.y), fmaxf(l1.z, r1.z), __int_as_float(R));
}

}  // namespace rtgo
