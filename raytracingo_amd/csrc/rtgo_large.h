// rtgo_large.h -- the device-wide build of a scene of rtgo_set_large_scene (beyond build_kernel's one workgroup of kMaxPrims threads).
// It builds the canonical LBVH of build_kernel / oracle_lbvh_build bit for bit, in global memory, with the same __device__ functions:
//   large_prep_kernel     per primitive: the 6-float4 record and, without caller boxes, the CubeBox box (prim_record_and_box, below)
//   whitted::big_bounds_final_kernel over the boxes: the scene bounds (exact min / max)
//   large_keys_kernel     the 30-bit Morton code of each box centre (morton_cell, morton3), key = code << 32 | index; then the four stable
//                         radix passes of rtgo_whitted_big.h over the code's bytes: the (code, index) order
//   large_karras_kernel   one thread per internal node (karras_node): links and parents; leaves are nodes n-1+j, node 0 the root
//   large_depth_kernel    every node's depth (its parent chain), the leaves' boxes and links, and the largest leaf depth
//   large_fit_kernel      one launch per tree level, deepest first: node box = fminf / fmaxf of its two children's, in build_kernel's
//                         operand order.  The kernel boundary between two levels is what makes a child box written by another
//                         workgroup (on another XCD's L2) visible to its parent's: no inter-workgroup hand-off inside a launch.
// and the edit of such a scene in place (rtgo_update_prims), over what the build keeps on the device -- every node's
// parent, the internal nodes' depths, each primitive's leaf node and a mark word per internal node.  What an edit does to one primitive
// is written once, in __device__ functions every kernel below calls:
//   prim_record_and_box   the 6-float4 record (inverse_rows012, store_prim_record) and the box: the caller's, or the CubeBox rule's (cube_aabb)
//   write_box_and_leaf    the box into the scene's array and into the primitive's leaf node; whether it changed bitwise (`moved`)
//   mark_ancestors        the walk from a moved leaf to the root, every node on it stamped with the refit's epoch
//   refit_marked_node     large_fit_kernel's box (fit_node) for a marked node of one level, the links read from the node itself
//   large_update_kernel   per update, the record read from global memory: the first three; a rebuild also keeps what it overwrites
//   large_refit_kernel    refit_marked_node: one launch per level again, for large_fit_kernel's reason
//   large_restore_kernel  puts back the records and boxes large_update_kernel saved (a rebuild that is refused)
//   prims_patch_kernel    a scene of rtgo_set_scene: the updates scattered into build_kernel's inputs
// and the checks of the calls that take records, boxes and indices from device memory:
//   prims_check_kernel    per entry: the host's check_prims rules and the index rules of rtgo_update_prims, into a verdict of a few words
// and the refit that waits for nothing on the host (rtgo_update_prims_device_async):
//   prims_check_reach_kernel    prims_check_kernel plus the test of each entry's box against the caller's `reach`
//   large_update_staged_kernel  the three functions behind the verdict's gate, the record taken from the workgroup's staged copy in LDS
//   large_refit_gated_kernel    refit_marked_node behind the gate and the ticket's `changed` word
#pragma once

#include "rtgo_device.h"
#include "rtgo_whitted_big.h"

namespace rtgo {

constexpr int kLargeMaxDepth = 64;   // per-lane LDS stack entries of the global-memory walk: deeper trees are refused

// Primitive P's 6-float4 record into out_prims at i, and its box: bb = entry e of the caller's boxes `given` (global memory or LDS), or,
// given == nullptr, the CubeBox rule's.  The build, the synchronous and the asynchronous edit write the same bits because all call this.
__device__ __forceinline__ void prim_record_and_box(const PrimIn& P, const float* given, size_t e, float4* out_prims, size_t i, float bb[6])
{
    float inv[12];
    inverse_rows012(P.M, inv);
    store_prim_record(out_prims + 6 * i, P, inv);
    if (given) {
        for (int a = 0; a < 6; ++a) bb[a] = given[6 * e + a];
    } else {
        cube_aabb(P.M, bb);
    }
}

__global__ __launch_bounds__(256) void large_prep_kernel(const PrimIn* __restrict__ prims, float* __restrict__ aabb_io, int have_aabb, int n,
                                                         float4* __restrict__ out_prims)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const PrimIn P = prims[i];
    float bb[6];   // (the caller's boxes are in place already: only the rule's box is of use here)
    prim_record_and_box(P, nullptr, 0, out_prims, i, bb);
    if (!have_aabb)
        for (int a = 0; a < 6; ++a) aabb_io[6 * (size_t)i + a] = bb[a];
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

// node k of the 2n-1: its depth (internal nodes -> depth[k]); a leaf also writes its node record, its primitive's leaf_of and raises *max_depth.  A chain longer
// than kLargeMaxDepth stops counting there (the host refuses such a tree; the walk up cannot run away either).
__global__ __launch_bounds__(256) void large_depth_kernel(const unsigned long long* __restrict__ keys, int n, const float* __restrict__ aabb,
                                                          const int* __restrict__ parent, int* __restrict__ depth, float4* __restrict__ nodes,
                                                          int* __restrict__ max_depth, int* __restrict__ leaf_of)
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
            leaf_of[prim] = k;
            atomicMax(&s_max, d);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(max_depth, s_max);
}

// internal node i over its children L and R: the box of their boxes, and the links
__device__ __forceinline__ void fit_node(int i, int L, int R, float4* __restrict__ nodes)
{
    const float4 l0 = nodes[2 * (size_t)L], l1 = nodes[2 * (size_t)L + 1], r0 = nodes[2 * (size_t)R], r1 = nodes[2 * (size_t)R + 1];
    nodes[2 * (size_t)i + 0] = make_float4(fminf(l0.x, r0.x), fminf(l0.y, r0.y), fminf(l0.z, r0.z), __int_as_float(L));
    nodes[2 * (size_t)i + 1] = make_float4(fmaxf(l1.x, r1.x), fmaxf(l1.y, r1.y), fmaxf(l1.z, r1.z), __int_as_float(R));
}

// the internal nodes at depth `level`: their children (deeper) were written by earlier launches
__global__ __launch_bounds__(256) void large_fit_kernel(const int* __restrict__ left, const int* __restrict__ right, const int* __restrict__ depth,
                                                        int n_internal, int level, float4* __restrict__ nodes)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_internal || depth[i] != level) return;
    fit_node(i, left[i], right[i], nodes);
}

// Primitive i's box becomes bb: into the scene's array and into its leaf node, `leaf`.  Returns `moved`: the box changed bitwise, so the
// leaf's ancestors have to be fitted again.
__device__ __forceinline__ bool write_box_and_leaf(const float bb[6], size_t i, float* __restrict__ aabb, const int* __restrict__ leaf_of, float4* __restrict__ nodes, int& leaf)
{
    bool moved = false;
    for (int a = 0; a < 6; ++a) {
        moved = moved || __float_as_uint(bb[a]) != __float_as_uint(aabb[6 * i + a]);
        aabb[6 * i + a] = bb[a];
    }
    leaf = leaf_of[i];
    nodes[2 * (size_t)leaf + 0] = make_float4(bb[0], bb[1], bb[2], __int_as_float((int)i));
    nodes[2 * (size_t)leaf + 1] = make_float4(bb[3], bb[4], bb[5], __int_as_float(-1));
    return moved;
}

// Every ancestor of `leaf` is marked with `epoch`; a thread that finds one marked stops: whoever marked it first goes on to the root
__device__ __forceinline__ void mark_ancestors(int leaf, const int* parent, unsigned int epoch, unsigned int* mark)
{
    int q = parent[leaf];
    for (int d = 0; q >= 0 && d <= kLargeMaxDepth; ++d) {   // (a chain is at most kLargeMaxDepth long: the build refused deeper trees)
        if (atomicExch(&mark[q], epoch) == epoch) break;
        q = parent[q];
    }
}

// Update j: primitive idx[j] becomes upd[j], its box upd_aabb[j] (nullable).  old_prims / old_aabb (nullable): what they replace, kept
// at j.  nodes (nullable): a rebuild, which stops after the box.  Where a box moved *changed is set.  The indices are distinct and below n (the host checked): no two threads write the same record.
__global__ __launch_bounds__(256) void large_update_kernel(const unsigned int* __restrict__ idx, const PrimIn* __restrict__ upd,
                                                           const float* __restrict__ upd_aabb, int k, const int* __restrict__ leaf_of,
                                                           const int* __restrict__ parent, unsigned int epoch, unsigned int* __restrict__ mark,
                                                           float4* __restrict__ out_prims, float* __restrict__ aabb, float4* __restrict__ nodes,
                                                           float4* __restrict__ old_prims, float* __restrict__ old_aabb, int* __restrict__ changed)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    const size_t i = idx[j];
    const PrimIn P = upd[j];
    if (old_prims) {
        for (int q = 0; q < 6; ++q) old_prims[6 * (size_t)j + q] = out_prims[6 * i + q];
        for (int a = 0; a < 6; ++a) old_aabb[6 * (size_t)j + a] = aabb[6 * i + a];
    }
    float bb[6];
    prim_record_and_box(P, upd_aabb, j, out_prims, i, bb);
    if (!nodes) {   // (a rebuild writes its leaves itself, from the boxes)
        for (int a = 0; a < 6; ++a) aabb[6 * i + a] = bb[a];
        return;
    }
    int leaf;
    if (!write_box_and_leaf(bb, i, aabb, leaf_of, nodes, leaf)) return;
    *changed = 1;
    mark_ancestors(leaf, parent, epoch, mark);
}

// node i, if it is a marked internal node at depth `level`: fit_node again, the links read from the node itself, over children an earlier launch wrote
__device__ __forceinline__ void refit_marked_node(int i, const int* __restrict__ depth, const unsigned int* __restrict__ mark, unsigned int epoch, int n_internal, int level,
                                                  float4* __restrict__ nodes)
{
    if (i >= n_internal || mark[i] != epoch || depth[i] != level) return;
    fit_node(i, __float_as_int(nodes[2 * (size_t)i].w), __float_as_int(nodes[2 * (size_t)i + 1].w), nodes);
}

__global__ __launch_bounds__(256) void large_refit_kernel(const int* __restrict__ depth, const unsigned int* __restrict__ mark, unsigned int epoch,
                                                          int n_internal, int level, float4* __restrict__ nodes)
{
    refit_marked_node(blockIdx.x * 256 + threadIdx.x, depth, mark, epoch, n_internal, level, nodes);
}

__global__ __launch_bounds__(256) void large_restore_kernel(const unsigned int* __restrict__ idx, const float4* __restrict__ old_prims,
                                                            const float* __restrict__ old_aabb, int k, float4* __restrict__ out_prims,
                                                            float* __restrict__ aabb)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    const size_t i = idx[j];
    for (int q = 0; q < 6; ++q) out_prims[6 * i + q] = old_prims[6 * (size_t)j + q];
    for (int a = 0; a < 6; ++a) aabb[6 * i + a] = old_aabb[6 * (size_t)j + a];
}

// a scene of rtgo_set_scene: update j goes into build_kernel's inputs at idx[j] (upd_aabb == nullptr: the build derives the boxes)
__global__ __launch_bounds__(256) void prims_patch_kernel(const unsigned int* __restrict__ idx, const PrimIn* __restrict__ upd,
                                                          const float* __restrict__ upd_aabb, int k, PrimIn* __restrict__ prims, float* __restrict__ aabb)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    const size_t i = idx[j];
    prims[i] = upd[j];
    for (int a = 0; upd_aabb && a < 6; ++a) aabb[6 * i + a] = upd_aabb[6 * (size_t)j + a];
}

// ---- the checks of the device-pointer calls (rtgo_set_scene_device, rtgo_set_large_scene_device, rtgo_update_prims_device):
// what check_prims and rtgo_update_prims decide on the host, decided where the caller's arrays lie.  The verdict is one word per kind of
// fault, the lowest offending entry (kNoFault: none); the host fills it with kNoFault before the launch and reads it back once.
constexpr int kPrimDwords = 27;
static_assert(sizeof(PrimIn) == kPrimDwords * sizeof(unsigned int), "rtgo_prim is 27 dwords");
enum { kBadType = 0, kBadFloat = 1, kBadMatrix = 2, kBadBox = 3, kBadIndex = 4, kBadTwice = 5, kVerdictKinds = 6, kVerdictWords = 8 };
enum { kBadReach = 6, kAsyncVerdictKinds = 7 };   // the seventh kind, of rtgo_update_prims_device_async's check alone
constexpr unsigned int kNoFault = 0xFFFFFFFFu;

// Entry j < k: record prims[j] (27 dwords), box aabbs[j] (aabbs nullable), index idx[j] (idx nullable: the set calls).
// A thread that read its own record from global memory would read at a stride of 27 dwords, a wave's load touching 64 scattered lines; the
// workgroup loads its 256 records (and boxes) with coalesced dword loads into LDS instead and each thread checks its record there -- at
// stride 27, odd, so free of bank conflicts.  The last workgroup loads the dwords of its own entries only: nothing beyond the caller's
// k entries is read.  An index is compared with n before anything else is done with it; one in range is claimed by writing `epoch` into
// claim[index] (n words of the scene's, stamped per call like LargeKeep::mark): whoever finds `epoch` there already is the second to name it.

// The staging: the workgroup's entries [base, base + here) of prims (and of aabbs, nullable) into s_prim [256 * kPrimDwords] and s_box
// [256 * 6]; every thread of the workgroup calls it.  Returns `here`, at most 256; 0 for a workgroup beyond the k entries (nothing is
// loaded and no barrier passed: the whole workgroup leaves).
__device__ __forceinline__ unsigned int stage_entries(const unsigned int* __restrict__ prims, const float* __restrict__ aabbs, unsigned int k,
                                                      unsigned int* s_prim, float* s_box)
{
    const unsigned int tid = threadIdx.x, base = blockIdx.x * 256u;
    if (base >= k) return 0;
    const unsigned int here = k - base < 256u ? k - base : 256u;   // this workgroup's entries
    const unsigned int* src = prims + (size_t)base * kPrimDwords;
    for (unsigned int d = tid; d < here * kPrimDwords; d += 256u) s_prim[d] = src[d];
    if (aabbs) {
        const float* bsrc = aabbs + (size_t)base * 6;
        for (unsigned int d = tid; d < here * 6u; d += 256u) s_box[d] = bsrc[d];
    }
    __syncthreads();
    return here;
}

// what rtgo_update_prims_device_async's caller vouches for: every updated primitive's box lies inside
struct ReachBox {
    float lo[3], hi[3];
};

// The checks of the staged entries.  REACH: also kBadReach, for an entry whose box -- the given one, or without boxes the cube_aabb of its
// matrix, the box the update would write -- does not lie inside `reach` (a box that is not finite lies inside nothing).
template <bool REACH>
__device__ __forceinline__ void check_entries(unsigned int here, const unsigned int* s_prim, const float* s_box, bool have_boxes,
                                              const unsigned int* __restrict__ idx, unsigned int n, unsigned int epoch,
                                              unsigned int* __restrict__ claim, unsigned int* __restrict__ verdict, const ReachBox& reach)
{
#pragma clang fp contract(off)
    const unsigned int tid = threadIdx.x, j = blockIdx.x * 256u + tid;
    unsigned int bad = 0;
    if (tid < here) {
        const unsigned int* r = s_prim + tid * kPrimDwords;
        if (r[0] > 3u) bad |= 1u << kBadType;
        bool finite = true;
        for (int q = 1; q < kPrimDwords; ++q) finite = finite && (r[q] & 0x7F800000u) != 0x7F800000u;
        if (!finite) bad |= 1u << kBadFloat;
        // check_prims' determinant: the model matrix' 3x3 in double, mat3_det_inverse's expression, one rounding per operation
        const double a00 = __uint_as_float(r[1]), a01 = __uint_as_float(r[2]), a02 = __uint_as_float(r[3]);
        const double a10 = __uint_as_float(r[5]), a11 = __uint_as_float(r[6]), a12 = __uint_as_float(r[7]);
        const double a20 = __uint_as_float(r[9]), a21 = __uint_as_float(r[10]), a22 = __uint_as_float(r[11]);
        const double det = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
        if (!isfinite(det) || fabs(det) < 1e-30) bad |= 1u << kBadMatrix;
        if (have_boxes) {
            const float* b = s_box + tid * 6;
            if (!(b[0] <= b[3] && b[1] <= b[4] && b[2] <= b[5]) || !isfinite(b[0] + b[1] + b[2] + b[3] + b[4] + b[5])) bad |= 1u << kBadBox;
        }
        if (REACH) {
            float bb[6];
            if (have_boxes) {
                for (int a = 0; a < 6; ++a) bb[a] = s_box[tid * 6 + a];
            } else {
                float M[16];
                for (int q = 0; q < 16; ++q) M[q] = __uint_as_float(r[1 + q]);
                cube_aabb(M, bb);
            }
            bool inside = true;
            for (int a = 0; a < 3; ++a) inside = inside && bb[a] >= reach.lo[a] && bb[3 + a] <= reach.hi[a];
            if (!inside) bad |= 1u << kBadReach;
        }
        if (idx) {
            const unsigned int i = idx[j];
            if (i >= n) bad |= 1u << kBadIndex;
            else if (atomicExch(&claim[i], epoch) == epoch) bad |= 1u << kBadTwice;
        }
    }
    // the lowest offending entry of the wave, one atomic per wave and kind
    if (!__any(bad != 0)) return;
    const unsigned int lane = tid & 63u;
    for (int kind = 0; kind < (REACH ? kAsyncVerdictKinds : kVerdictKinds); ++kind) {
        const unsigned long long m = __ballot((bad >> kind) & 1u);
        if (m != 0 && lane == (unsigned int)(__ffsll((long long)m) - 1)) atomicMin(&verdict[kind], j);
    }
}

__global__ __launch_bounds__(256) void prims_check_kernel(const unsigned int* __restrict__ prims, const float* __restrict__ aabbs,
                                                          const unsigned int* __restrict__ idx, unsigned int k, unsigned int n, unsigned int epoch,
                                                          unsigned int* __restrict__ claim, unsigned int* __restrict__ verdict)
{
    __shared__ unsigned int s_prim[256 * kPrimDwords];
    __shared__ float s_box[256 * 6];
    const unsigned int here = stage_entries(prims, aabbs, k, s_prim, s_box);
    if (here == 0) return;
    check_entries<false>(here, s_prim, s_box, aabbs != nullptr, idx, n, epoch, claim, verdict, ReachBox{});
}

// ---- the refit of rtgo_update_prims_device_async: the check, the update and the refit enqueued back to back, no verdict
// read by the host in between.  The verdict is a slot of the context's ring (kVerdictWords words, filled with kNoFault ahead of the check);
// the kernels that write the scene read it first and leave at once unless it is clean.  The kernel boundary after the check is what makes
// the verdict complete and visible to them, large_fit_kernel's argument for one launch per level.

// prims_check_kernel with the reach test, for the updates of a scene of rtgo_set_large_scene (idx is not nullable here)
__global__ __launch_bounds__(256) void prims_check_reach_kernel(const unsigned int* __restrict__ prims, const float* __restrict__ aabbs,
                                                                const unsigned int* __restrict__ idx, unsigned int k, unsigned int n,
                                                                unsigned int epoch, unsigned int* __restrict__ claim,
                                                                unsigned int* __restrict__ verdict, ReachBox reach)
{
    __shared__ unsigned int s_prim[256 * kPrimDwords];
    __shared__ float s_box[256 * 6];
    const unsigned int here = stage_entries(prims, aabbs, k, s_prim, s_box);
    if (here == 0) return;
    check_entries<true>(here, s_prim, s_box, aabbs != nullptr, idx, n, epoch, claim, verdict, reach);
}

// the gate: the same address in every lane, so eight scalar loads per wave
__device__ __forceinline__ bool verdict_clean(const unsigned int* __restrict__ verdict)
{
    unsigned int all = kNoFault;
    for (int q = 0; q < kVerdictWords; ++q) all &= verdict[q];
    return all == kNoFault;
}

// large_update_kernel's refit for checked updates that lie in device memory, behind the gate.  large_update_kernel reads its 108-byte
// records at a stride of 27 dwords (a wave's load touches 64 lines, 27 times); here the workgroup stages its 256 records and boxes in LDS
// as the check does and each thread takes its record from there.  From there on the two call the same functions: what they write is
// equal bit for bit.  *changed: the ticket's word.
__global__ __launch_bounds__(256) void large_update_staged_kernel(const unsigned int* __restrict__ verdict, const unsigned int* __restrict__ idx,
                                                                  const unsigned int* __restrict__ upd, const float* __restrict__ upd_aabb,
                                                                  unsigned int k, const int* __restrict__ leaf_of, const int* __restrict__ parent,
                                                                  unsigned int epoch, unsigned int* __restrict__ mark,
                                                                  float4* __restrict__ out_prims, float* __restrict__ aabb,
                                                                  float4* __restrict__ nodes, unsigned int* __restrict__ changed)
{
    __shared__ unsigned int s_prim[256 * kPrimDwords];
    __shared__ float s_box[256 * 6];
    if (!verdict_clean(verdict)) return;
    const unsigned int tid = threadIdx.x;
    const unsigned int here = stage_entries(upd, upd_aabb, k, s_prim, s_box);
    if (tid >= here) return;
    const size_t i = idx[blockIdx.x * 256u + tid];
    PrimIn P;
    __builtin_memcpy(&P, s_prim + tid * kPrimDwords, sizeof P);
    float bb[6];
    prim_record_and_box(P, upd_aabb ? s_box : nullptr, tid, out_prims, i, bb);
    int leaf;
    if (!write_box_and_leaf(bb, i, aabb, leaf_of, nodes, leaf)) return;
    *changed = 1u;
    mark_ancestors(leaf, parent, epoch, mark);
}

// large_refit_kernel behind the gate: the host cannot skip these launches (it no longer knows *changed), so each leaves at once for a
// refused update and for one that moved no box -- the node array then stays bitwise as it was
__global__ __launch_bounds__(256) void large_refit_gated_kernel(const unsigned int* __restrict__ verdict, const unsigned int* __restrict__ changed,
                                                                const int* __restrict__ depth, const unsigned int* __restrict__ mark,
                                                                unsigned int epoch, int n_internal, int level, float4* __restrict__ nodes)
{
    if (!verdict_clean(verdict) || *changed == 0u) return;
    refit_marked_node(blockIdx.x * 256 + threadIdx.x, depth, mark, epoch, n_internal, level, nodes);
}

}  // namespace rtgo
