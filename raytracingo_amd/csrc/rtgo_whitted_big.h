// rtgo_whitted_big.h -- the device-wide build steps of a clustered mesh (a mesh of an instanced whitted scene beyond kMaxTriangles
// triangles, rtgo_whitted_set_scene).  build_kernel sorts one mesh in one workgroup's LDS; a bigger mesh is first put in Morton order
// here, over the whole device, and then cut into clusters of at most kClusterTris consecutive triangles, each built by the single-mesh
// pair (build_kernel + sah_kernel) and joined by a mid level over the clusters' boxes (rtgo_whitted_inst.h walks the three levels).
//
// Steps, one launch each (kernel boundaries are the only grid-wide synchronisation: nothing waits on another workgroup):
//   big_bounds_kernel (grid-stride partial boxes) -> big_bounds_final_kernel (one workgroup) -> big_keys_kernel (Morton code of the
//   centroid on build_kernel's 10-bit grid, key = code << 32 | triangle) -> four LSD radix passes over the code's bytes
//   (radix_count_kernel, radix_scan_kernel, radix_scatter_kernel; stable, and the keys start in triangle order, so the order is
//   (code, triangle): unique keys, one deterministic order) -> big_gather_kernel (each sorted triangle's index triple) -> the batched
//   builds, whitted_build over every structure of the call with one workgroup each (big_build_batch_kernel, big_sah_batch_kernel,
//   big_build_batch_kernel for the surface-area trees that came out too deep, big_batch_offsets_kernel, big_pack_records_kernel: below)
//   -> big_remap_kernel (cluster-local triangle numbers in tris[].w back to the mesh's own).
// A refit to moved vertices (rtgo_whitted_update_meshes) keeps all of that and runs big_bounds_kernel, big_bounds_final_kernel (the
// mesh's box), big_refit_clusters_kernel (every cluster, one workgroup each), big_cluster_boxes_kernel and refit_kernel (the mid level).
// The small meshes a call names are refitted by one launch, big_refit_meshes_kernel (one workgroup each).  Vertices that are on the
// device already (rtgo_whitted_update_meshes_device) are checked and bounded where they lie by big_update_check_kernel and
// big_update_check_final_kernel, one pair of launches over a table of the call's entries.
#pragma once

#include "rtgo_whitted.h"

namespace rtgo {
namespace whitted {

#ifndef RTGO_CLUSTER_TRIS
#define RTGO_CLUSTER_TRIS 4096
#endif
constexpr int kClusterTris = RTGO_CLUSTER_TRIS;   // sah_kernel's LDS (33 B per triangle, <= 150 KiB) holds a cluster: surface-area records
static_assert(kClusterTris > 4 * kLeafTris && kClusterTris <= kMaxTriangles, "cluster size");
constexpr int kBigMaxMeshTriangles = 1 << 24;      // per mesh: at most kBigMaxMeshTriangles / (kClusterTris / 2) clusters, a mid level
constexpr int kBigMaxSceneTriangles = 1 << 26;     //   that build_kernel can sort; over a scene: int indices into the arrays stay far from 2^31
static_assert(kBigMaxMeshTriangles / (kClusterTris / 2) <= kMaxTriangles, "mid level");
constexpr int kRadixThreads = 1024;
constexpr int kRadixTile = 8 * kRadixThreads;      // keys per workgroup of the count and scatter passes

// the clusters of a mesh of n triangles in sorted order: ncl = ceil(n / kClusterTris) runs as even as they come, the first n % ncl one
// triangle longer (so none is shorter than kClusterTris / 2, and every one has records)
__host__ __device__ __forceinline__ int cluster_start(long long n, int ncl, int c)
{
    const long long q = n / ncl, r = n % ncl;
    return (int)(c * q + (c < r ? c : r));
}

__global__ __launch_bounds__(1024) void big_bounds_kernel(const float* __restrict__ positions, const unsigned int* __restrict__ indices, int n,
                                                          float* __restrict__ partial)
{
    __shared__ float s_red[6][1024];
    const int tid = threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = (long long)blockIdx.x * 1024 + tid; i < n; i += (long long)gridDim.x * 1024)
        for (int k = 0; k < 3; ++k) {
            const unsigned int vi = indices[3 * i + k];
            for (int a = 0; a < 3; ++a) {
                const float c = positions[3 * (size_t)vi + a];
                lo[a] = fminf(lo[a], c);
                hi[a] = fmaxf(hi[a], c);
            }
        }
    reduce_bounds<1024>(s_red, tid, lo, hi);
    if (tid < 6) partial[6 * blockIdx.x + tid] = s_red[tid][0];
}

// one workgroup: the partial boxes of big_bounds_kernel's n_parts workgroups -> bounds[6] = lo xyz, hi xyz
__global__ __launch_bounds__(1024) void big_bounds_final_kernel(const float* __restrict__ partial, int n_parts, float* __restrict__ bounds)
{
    __shared__ float s_red[6][1024];
    const int tid = threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < n_parts; i += 1024)
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], partial[6 * i + a]);
            hi[a] = fmaxf(hi[a], partial[6 * i + 3 + a]);
        }
    reduce_bounds<1024>(s_red, tid, lo, hi);
    if (tid < 6) bounds[tid] = s_red[tid][0];
}

// build_kernel's Morton key of every triangle, over the whole mesh's bounds
__global__ __launch_bounds__(256) void big_keys_kernel(const float* __restrict__ positions, const unsigned int* __restrict__ indices, int n,
                                                       const float* __restrict__ bounds, unsigned long long* __restrict__ keys)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float lo[3] = {bounds[0], bounds[1], bounds[2]}, ext[3] = {bounds[3] - bounds[0], bounds[4] - bounds[1], bounds[5] - bounds[2]};
    keys[i] = triangle_key(positions, indices, i, lo, ext);
}

// radix pass, step 1: how many keys of workgroup b's tile have digit d at `shift` -> hist[d * n_blocks + b]
__global__ __launch_bounds__(kRadixThreads) void radix_count_kernel(const unsigned long long* __restrict__ keys, int n, int shift,
                                                                    unsigned int* __restrict__ hist)
{
    __shared__ unsigned int s_h[256];
    const int tid = threadIdx.x;
    if (tid < 256) s_h[tid] = 0u;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kRadixTile;
    for (int k = tid; k < kRadixTile; k += kRadixThreads) {
        const long long i = base + k;
        if (i < n) atomicAdd(&s_h[(unsigned int)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 256) hist[(size_t)tid * gridDim.x + blockIdx.x] = s_h[tid];
}

// step 2, one workgroup: exclusive prefix sum of the m counts in place (digit-major: every key of digit d goes after all of d - 1)
__global__ __launch_bounds__(1024) void radix_scan_kernel(unsigned int* __restrict__ hist, int m)
{
    __shared__ unsigned int s_sum[1024];
    const int tid = threadIdx.x;
    const int per = (m + 1023) / 1024;
    const long long a = (long long)tid * per, b = a + per < m ? a + per : m;
    unsigned int s = 0u;
    for (long long i = a; i < b; ++i) s += hist[i];
    s_sum[tid] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned int run = 0u;
        for (int k = 0; k < 1024; ++k) {
            const unsigned int v = s_sum[k];
            s_sum[k] = run;
            run += v;
        }
    }
    __syncthreads();
    unsigned int run = s_sum[tid];
    for (long long i = a; i < b; ++i) {
        const unsigned int v = hist[i];
        hist[i] = run;
        run += v;
    }
}

// step 3: every key to its place, stably: the tile goes 1024 keys at a time in order; within a wave a key's rank among the lanes
// below it with the same digit comes from eight ballots, and the waves of the workgroup follow each other through LDS
__global__ __launch_bounds__(kRadixThreads) void radix_scatter_kernel(const unsigned long long* __restrict__ keys, int n, int shift,
                                                                      const unsigned int* __restrict__ offs, unsigned long long* __restrict__ out)
{
    constexpr int kWaves = kRadixThreads / 64;
    __shared__ unsigned int s_base[256], s_total[256];
    __shared__ unsigned int s_wave[kWaves][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 256) s_base[tid] = offs[(size_t)tid * gridDim.x + blockIdx.x];
    const long long base = (long long)blockIdx.x * kRadixTile;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int chunk = 0; chunk < kRadixTile; chunk += kRadixThreads) {
        for (int k = tid; k < kWaves * 256; k += kRadixThreads) (&s_wave[0][0])[k] = 0u;
        __syncthreads();
        const long long i = base + chunk + tid;
        const bool valid = i < n;
        const unsigned long long key = valid ? keys[i] : 0ull;
        const unsigned int dig = (unsigned int)(key >> shift) & 255u;
        unsigned long long same = __builtin_amdgcn_ballot_w64(valid);
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long ones = __builtin_amdgcn_ballot_w64(valid && ((dig >> bit) & 1u));
            same &= ((dig >> bit) & 1u) ? ones : ~ones;
        }
        const unsigned int rank = (unsigned int)__popcll(same & below);
        if (valid && rank == 0u) s_wave[wave][dig] = (unsigned int)__popcll(same);   // the lowest lane of each digit speaks for it
        __syncthreads();
        if (tid < 256) {
            unsigned int run = 0u;
            for (int w = 0; w < kWaves; ++w) {
                const unsigned int v = s_wave[w][tid];
                s_wave[w][tid] = run;
                run += v;
            }
            s_total[tid] = run;
        }
        __syncthreads();
        if (valid) out[s_base[dig] + s_wave[wave][dig] + rank] = key;
        __syncthreads();
        if (tid < 256) s_base[tid] += s_total[tid];
        // (the next chunk's first barrier orders this update before any read of s_base)
    }
}

// each sorted triangle's index triple (relative to the mesh's vertices, as the caller gave it)
__global__ __launch_bounds__(256) void big_gather_kernel(const unsigned long long* __restrict__ sorted, int n, const unsigned int* __restrict__ indices,
                                                         unsigned int* __restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const size_t t = (size_t)(sorted[j] & 0xFFFFFFFFull);
    out[3 * (size_t)j + 0] = indices[3 * t + 0];
    out[3 * (size_t)j + 1] = indices[3 * t + 1];
    out[3 * (size_t)j + 2] = indices[3 * t + 2];
}

// tris[].w of every cluster: build_kernel wrote the triangle's number within its cluster (its place in the cluster's slice of the
// gathered triples); the mesh's own index is the sorted key at the cluster's start + that number
__global__ __launch_bounds__(256) void big_remap_kernel(float4* __restrict__ tris, const unsigned long long* __restrict__ sorted, int n, int ncl)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int q = n / ncl, r = n % ncl;
    const int c = p < r * (q + 1) ? p / (q + 1) : r + (p - r * (q + 1)) / q;
    const int local = __float_as_int(tris[3 * (size_t)p].w);
    tris[3 * (size_t)p].w = __int_as_float((int)(sorted[cluster_start(n, ncl, c) + local] & 0xFFFFFFFFull));
}

// the mid level's input: cluster c's box (the union of its root record's two child boxes) as the degenerate triangle (lo, hi, lo)
// of the top level's recipe -> pos[6 c .. 6 c + 5]
__global__ __launch_bounds__(256) void big_cluster_boxes_kernel(const float4* __restrict__ recs, const int* __restrict__ rec_base, int ncl,
                                                                float* __restrict__ pos)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncl) return;
    const float4* r = recs + 4 * (size_t)rec_base[c];
    const float4 a0 = r[0], a1 = r[1], b0 = r[2], b1 = r[3];
    pos[6 * c + 0] = fminf(a0.x, b0.x);
    pos[6 * c + 1] = fminf(a0.y, b0.y);
    pos[6 * c + 2] = fminf(a0.z, b0.z);
    pos[6 * c + 3] = fmaxf(a1.x, b1.x);
    pos[6 * c + 4] = fmaxf(a1.y, b1.y);
    pos[6 * c + 5] = fmaxf(a1.z, b1.z);
}

// ---- refit (rtgo_whitted_update_meshes) ---------------------------------------------------------------------------------------------
// One cluster of a clustered mesh as its build left it: its records start at recs[4 rec0] of the scene, its sorted triangles at
// position tri0 of the mesh's (tris, qrecs and done are the mesh's own slices), n of them; n_recs and walk_depth as that build reported
struct ClusterRefit { int rec0, tri0, n, n_recs, walk_depth; };

// refit_kernel's body over every cluster of one mesh, one workgroup per cluster.  positions / indices are the mesh's own: since
// big_remap_kernel a cluster's tris[].w holds the mesh's triangle index, and that triple is the one the cluster's build read from its
// slice of the gathered triples; bounds, pad and grid are taken over the cluster's triangles alone, as that build took them.  A
// workgroup reads and writes its own cluster's records, triangles and flags only, so nothing orders the workgroups: the mid level is
// refitted by a later launch (big_cluster_boxes_kernel, then refit_kernel over the clusters' boxes).  out_meta[c] gets cluster c's grid.
__global__ __launch_bounds__(kBuildThreads) void big_refit_clusters_kernel(const float* __restrict__ positions, const unsigned int* __restrict__ indices,
                                                                           const ClusterRefit* __restrict__ table, float4* recs, float4* tris, uint4* qrecs,
                                                                           int* done, WhittedBuildMeta* __restrict__ out_meta)
{
    __shared__ float s_red[6][kBuildThreads];
    const ClusterRefit c = table[blockIdx.x];
    refit_structure<true>({positions, indices, c.n, c.n_recs, c.walk_depth, recs + 4 * (size_t)c.rec0, tris + 3 * (size_t)c.tri0, qrecs + 2 * (size_t)c.tri0,
                           done + c.tri0, out_meta + blockIdx.x},
                          s_red);
}

// One small mesh of a call's refits as its build left it, by absolute offsets into the scene's arrays: its vertices start at vertex
// vert0, its index triples and sorted triangles at triangle tri0, its records at rec0; its flags at done0 of the call's scratch
struct MeshRefit { int vert0, tri0, rec0, n, n_recs, walk_depth, done0, pad; };
static_assert(sizeof(MeshRefit) == 8 * sizeof(int), "eight words");

// refit_kernel's body over every small mesh a call names, one workgroup per mesh: the records are refit_kernel's bit for bit.  A
// workgroup reads and writes its own mesh's slices only.  out_meta[m] gets mesh m's grid.
__global__ __launch_bounds__(kBuildThreads) void big_refit_meshes_kernel(const float* __restrict__ positions, const unsigned int* __restrict__ indices,
                                                                         const MeshRefit* __restrict__ table, float4* recs, float4* tris, uint4* qrecs, int* done,
                                                                         WhittedBuildMeta* __restrict__ out_meta)
{
    __shared__ float s_red[6][kBuildThreads];
    const MeshRefit m = table[blockIdx.x];
    refit_structure<false>({positions + 3 * (size_t)m.vert0, indices + 3 * (size_t)m.tri0, m.n, m.n_recs, m.walk_depth, recs + 4 * (size_t)m.rec0,
                            tris + 3 * (size_t)m.tri0, qrecs + 2 * (size_t)m.tri0, done + m.done0, out_meta + blockIdx.x},
                           s_red);
}

// ---- vertices that are on the device already (rtgo_whitted_update_meshes_device) ------------------------------------------------------
// One entry of the call as its checks see it.  positions / normals: the caller's buffers, 3 n_verts floats each (normals NULL: the mesh
// keeps its own).  indices: the mesh's n_tris index triples in the scene's arrays when the call needs the bounds of the vertices they
// name (a small mesh of an instanced scene), else NULL.  Workgroups first_block .. first_block + n_blocks - 1 of big_update_check_kernel
// are the entry's.
struct UpdateCheck {
    const float* positions;
    const float* normals;
    const unsigned int* indices;
    unsigned int n_verts;
    int n_tris, first_block, n_blocks;
};
static_assert(sizeof(UpdateCheck) == 40, "three pointers, four words");

// ... and what comes back of it: the exact min / max over the vertices its triangles name (indices given), and whether any float of its
// buffers, named by a triangle or not, is an infinity or a NaN
struct UpdateReport { float lo[3], hi[3]; unsigned int bad, pad; };

__device__ __forceinline__ unsigned int non_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

// whitted_check_updates' loop over the floats and big_bounds_kernel, for every entry of a table in one launch: each workgroup takes a
// grid-stride share of its entry's floats and triangles -> its partial box at partial[6 b ..] and its flag at part_bad[b] (fminf / fmaxf
// drop NaNs and the box sees named vertices only, so the flag is taken over the floats themselves).  Reads the caller's buffers, writes
// nothing of the scene.
__global__ __launch_bounds__(1024) void big_update_check_kernel(const UpdateCheck* __restrict__ table, int n_entries, float* __restrict__ partial,
                                                                unsigned int* __restrict__ part_bad)
{
    __shared__ float s_red[6][1024];
    const int tid = threadIdx.x, b = blockIdx.x;
    int e = 0, last = n_entries - 1;   // the entry whose run of workgroups holds b (uniform)
    while (e < last) {
        const int mid = (e + last + 1) / 2;
        if (table[mid].first_block <= b) e = mid;
        else last = mid - 1;
    }
    const UpdateCheck u = table[e];
    const size_t first = (size_t)(b - u.first_block) * 1024 + tid, stride = (size_t)u.n_blocks * 1024, n_floats = 3 * (size_t)u.n_verts;
    unsigned int bad = 0;
    for (size_t i = first; i < n_floats; i += stride) {
        bad |= non_finite(u.positions[i]);
        if (u.normals) bad |= non_finite(u.normals[i]);
    }
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (u.indices)
        for (size_t i = first; i < (size_t)u.n_tris; i += stride)
            for (int k = 0; k < 3; ++k) {
                const unsigned int vi = u.indices[3 * i + k];
                for (int a = 0; a < 3; ++a) {
                    const float c = u.positions[3 * (size_t)vi + a];
                    lo[a] = fminf(lo[a], c);
                    hi[a] = fmaxf(hi[a], c);
                }
            }
    reduce_bounds<1024>(s_red, tid, lo, hi);
    if (tid < 6) partial[6 * (size_t)b + tid] = s_red[tid][0];
    const int any = __syncthreads_or((int)bad);
    if (tid == 0) part_bad[b] = any ? 1u : 0u;
}

// one workgroup per entry: its workgroups' partial boxes and flags -> report[entry]
__global__ __launch_bounds__(1024) void big_update_check_final_kernel(const UpdateCheck* __restrict__ table, const float* __restrict__ partial,
                                                                      const unsigned int* __restrict__ part_bad, UpdateReport* __restrict__ report)
{
    __shared__ float s_red[6][1024];
    const int tid = threadIdx.x;
    const UpdateCheck u = table[blockIdx.x];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned int bad = 0;
    for (int i = tid; i < u.n_blocks; i += 1024) {
        const size_t p = (size_t)u.first_block + i;
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], partial[6 * p + a]);
            hi[a] = fmaxf(hi[a], partial[6 * p + 3 + a]);
        }
        bad |= part_bad[p];
    }
    reduce_bounds<1024>(s_red, tid, lo, hi);
    const int any = __syncthreads_or((int)bad);
    UpdateReport& r = report[blockIdx.x];
    if (tid < 3) r.lo[tid] = s_red[tid][0];
    else if (tid < 6) r.hi[tid - 3] = s_red[tid][0];
    else if (tid == 6) r.bad = any ? 1u : 0u;
    else if (tid == 7) r.pad = 0u;
}

// ---- batched builds (rtgo_whitted_set_scene, rtgo_whitted_rebuild_meshes) -----------------------------------------------------------
// One structure of a call's build table: a cluster of a clustered mesh (indices: its slice of the gathered triples) or a whole small
// mesh, n <= kMaxTriangles triangles.  tris, qrecs and tidx are its final slices (addressed by triangle slot); its records go to the
// staging of its workgroup's slot first, since where they start in the scene's arrays is known only once the structures before it
// have reported how many they have.  rec_start >= 0: the first structure of its mesh, whose records start there; the others' follow.
struct BuildEntry {
    const float* positions;
    const unsigned int* indices;
    float4* tris;
    uint4* qrecs;
    uint2* tidx;
    int n, sah, rec_start, pad;   // sah: the surface-area pass applies (its LDS need fits, RTGO_WHITTED_NO_SAH unset)
};
static_assert(sizeof(BuildEntry) == 56, "five pointers, four words");

// The scratch of a round of at most kBatchRound structures, each of at most max_n triangles: slot b (workgroup b of the round's
// launches) has nodes [2 (2 max_n - 1)] float4, BuildScratch's ints [build_scratch_ints(max_n)] and record staging [4 max_n] float4
constexpr int kBatchRound = 256;   // of the order of the CU count: one build workgroup fills a CU's LDS
struct BatchSlots {
    float4* nodes;
    int* ints;
    float4* stage;
    int max_n;
    __host__ __device__ float4* nodes_of(int b) const { return nodes + (size_t)b * 2 * (2 * (size_t)max_n - 1); }
    __host__ __device__ int* ints_of(int b) const { return ints + (size_t)b * build_scratch_ints((size_t)max_n); }
    __host__ __device__ float4* stage_of(int b) const { return stage + (size_t)b * 4 * (size_t)max_n; }
};

// build_kernel's body over entries first .. first + gridDim.x - 1 of the table, one workgroup per entry; metas[e] gets entry e's meta.
// redo = 0: every entry.  redo = 1, launched after big_sah_batch_kernel: only the entries whose surface-area tree came out deeper than
// the walk's stack get their Morton records back (whitted_build's fallback); the other workgroups leave at once.  A workgroup touches
// its own entry's slices and its own slot only.
__global__ __launch_bounds__(kBuildThreads) void big_build_batch_kernel(const BuildEntry* __restrict__ table, int first, BatchSlots slots,
                                                                        WhittedBuildMeta* metas, int redo)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char build_batch_keys_dyn[];   // kMaxTriangles x 8 B
    const int e = first + blockIdx.x;
    const BuildEntry en = table[e];
    if (redo && !(en.sah && metas[e].walk_depth > kMaxWalkDepth)) return;   // (uniform over the workgroup)
    const BuildScratch w(slots.ints_of(blockIdx.x), en.n);
    build_structure({en.positions, en.indices, en.n, slots.nodes_of(blockIdx.x), w.parent, w.visit, w.first_of, w.count_of, w.rec_of,
                     slots.stage_of(blockIdx.x), en.tris, en.qrecs, en.tidx, metas + e},
                    reinterpret_cast<unsigned long long*>(build_batch_keys_dyn));
}

// sah_kernel's body over the same entries and slots (the entries without the pass leave at once)
__global__ __launch_bounds__(kBuildThreads) void big_sah_batch_kernel(const BuildEntry* __restrict__ table, int first, BatchSlots slots, WhittedBuildMeta* metas)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sah_batch_dyn[];   // 33 B per triangle of the round's largest entry
    const int e = first + blockIdx.x;
    const BuildEntry en = table[e];
    if (!en.sah) return;
    const BuildScratch w(slots.ints_of(blockIdx.x), en.n);
    sah_structure({en.n, slots.nodes_of(blockIdx.x), w.parent, w.first_of, w.count_of, w.sah, slots.stage_of(blockIdx.x), en.qrecs, metas + e}, sah_batch_dyn);
}

// One workgroup: where the records of entries first .. first + count - 1 (count <= kBatchRound) start in the scene's arrays -> rec0[e]:
// rec_start for the first structure of a mesh, else where the structure before it ends.  *carry holds that end across rounds.
__global__ __launch_bounds__(kBatchRound) void big_batch_offsets_kernel(const BuildEntry* __restrict__ table, int first, int count,
                                                                        const WhittedBuildMeta* __restrict__ metas, int* __restrict__ rec0, int* carry)
{
    __shared__ int s_n[kBatchRound], s_start[kBatchRound];
    const int tid = threadIdx.x;
    if (tid < count) {
        s_n[tid] = metas[first + tid].n_recs;
        s_start[tid] = table[first + tid].rec_start;
    }
    __syncthreads();
    if (tid == 0) {
        int run = *carry;
        for (int k = 0; k < count; ++k) {
            if (s_start[k] >= 0) run = s_start[k];
            rec0[first + k] = run;
            run += s_n[k];
        }
        *carry = run;
    }
}

// The staged records of entry first + blockIdx.x to their place, recs[4 rec0 ..] of the scene (links inside a structure are relative to
// its first record: a plain copy)
__global__ __launch_bounds__(256) void big_pack_records_kernel(int first, BatchSlots slots, const WhittedBuildMeta* __restrict__ metas,
                                                               const int* __restrict__ rec0, float4* __restrict__ recs)
{
    const int e = first + blockIdx.x;
    const int n4 = 4 * metas[e].n_recs;
    const float4* __restrict__ src = slots.stage_of(blockIdx.x);
    float4* __restrict__ dst = recs + 4 * (size_t)rec0[e];
    for (int k = threadIdx.x; k < n4; k += 256) dst[k] = src[k];
}

}  // namespace whitted
}  // namespace rtgo
