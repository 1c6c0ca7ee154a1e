// rtgo_whitted_mesh_device.h -- the kernels of rtgo_whitted_set_scene_device, rtgo_whitted_set_mesh_device and
// rtgo_whitted_set_texcoords_device: a first build from meshes that are already on the device (under OptiX the vertex and index buffers
// of a build input are device pointers).  What whitted_layout_meshes (rtgo_whitted_host.h) does in host loops, done where the data lies:
//
//   mesh_check_kernel        over a host-built table of all meshes of the call: per workgroup which kinds of fault its share of its mesh
//                            holds (whitted_check_mesh's four checks), the largest material index, the exact min / max over the vertices
//                            the triangles name (whitted_mesh_box's, before the pad)
//   mesh_check_final_kernel  one workgroup per mesh: its workgroups' partial results -> report[mesh], 32 bytes
//   mesh_pack_kernel         after the verdict: every mesh's slice of the five packed arrays (positions, normals, texcoords, indices,
//                            tri_material), zeros where a mesh has none -- the image whitted_layout_meshes packs and whitted_upload_meshes
//                            uploads
//
// The pattern is big_update_check_kernel's (rtgo_whitted_big.h): runs of workgroups per entry, grid-stride shares, a binary search for
// the entry.  Everything after the pack is the host twin's own code on the same arrays.
#pragma once

#include "rtgo_whitted_big.h"

namespace rtgo {
namespace whitted {

constexpr int kMeshCheckThreads = 1024;

// One mesh of the call.  The five pointers are the caller's device buffers (rtgo_whitted_mesh's, 4-byte aligned), any of them NULL: that
// array is neither checked nor copied (rtgo_whitted_set_texcoords_device's table has texcoords alone).  Workgroups first_block ..
// first_block + n_blocks - 1 of both kernels are the mesh's; vert_base / tri_base: where its slices start in the packed arrays.
struct MeshSource {
    const float* positions;
    const float* normals;
    const float* texcoords;
    const unsigned int* indices;
    const unsigned int* material_of_triangle;
    unsigned int n_verts, n_tris;
    int first_block, n_blocks;
    unsigned int vert_base, tri_base;
};
static_assert(sizeof(MeshSource) == 64, "five pointers, six words");

// whitted_check_mesh's four refusals, in its order: bit k of MeshReport::faults
enum { kMeshBadIndex = 0, kMeshBadVertex = 1, kMeshBadTexcoord = 2, kMeshBadMaterial = 3, kMeshFaultKinds = 4 };

// What comes back of a mesh: the exact min / max over the vertices its triangles name (in-range indices only), which kinds of fault any
// element of its arrays holds, named by a triangle or not, and its largest material index (0 without a material array)
struct MeshReport { float lo[3], hi[3]; unsigned int faults, max_material; };
static_assert(sizeof(MeshReport) == 32, "eight words");

// the entry whose run of workgroups holds b (uniform over the workgroup)
__device__ __forceinline__ int mesh_entry_of(const MeshSource* __restrict__ table, int n_entries, int b)
{
    int e = 0, last = n_entries - 1;
    while (e < last) {
        const int mid = (e + last + 1) / 2;
        if (table[mid].first_block <= b) e = mid;
        else last = mid - 1;
    }
    return e;
}

// Each workgroup takes a grid-stride share of every array of its mesh, all by coalesced dword loads (4-byte alignment is all the
// contract gives): the floats of positions, normals and texcoords for infinities and NaNs, the material words against n_materials, the
// index words against n_verts.  -> its partial box at partial[6 b ..], its fault bits at part_words[2 b], its largest material index at
// part_words[2 b + 1].  Reads the caller's buffers, writes nothing of the context's scene.
//
// THE RULE OF THIS KERNEL: it never reads through an index it has not compared with n_verts in the same thread.  The host twin can check
// every index first and gather afterwards; here an unchecked gather is a fault of the card.  The comparison and the load are the two
// lines at (*) below and nowhere else: an out-of-range index sets its flag and is skipped by the bounds gather.  (fminf / fmaxf drop
// NaNs and the box sees named vertices only, so the vertex flag is taken over the floats themselves.)
__global__ __launch_bounds__(kMeshCheckThreads) void mesh_check_kernel(const MeshSource* __restrict__ table, int n_entries, unsigned int n_materials,
                                                                       float* __restrict__ partial, unsigned int* __restrict__ part_words)
{
    __shared__ float s_red[6][kMeshCheckThreads];
    __shared__ unsigned int s_words[2];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (tid < 2) s_words[tid] = 0u;
    const MeshSource m = table[mesh_entry_of(table, n_entries, b)];
    const size_t first = (size_t)(b - m.first_block) * kMeshCheckThreads + tid, stride = (size_t)m.n_blocks * kMeshCheckThreads;
    const size_t n_pos = 3 * (size_t)m.n_verts, n_uv = 2 * (size_t)m.n_verts, n_idx = 3 * (size_t)m.n_tris;
    unsigned int faults = 0, max_material = 0;
    if (m.positions)
        for (size_t i = first; i < n_pos; i += stride) faults |= non_finite(m.positions[i]) << kMeshBadVertex;
    if (m.normals)
        for (size_t i = first; i < n_pos; i += stride) faults |= non_finite(m.normals[i]) << kMeshBadVertex;
    if (m.texcoords)
        for (size_t i = first; i < n_uv; i += stride) faults |= non_finite(m.texcoords[i]) << kMeshBadTexcoord;
    if (m.material_of_triangle)
        for (size_t i = first; i < (size_t)m.n_tris; i += stride) {
            const unsigned int mat = m.material_of_triangle[i];
            faults |= (mat >= n_materials ? 1u : 0u) << kMeshBadMaterial;
            max_material = max(max_material, mat);
        }
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (m.indices && m.positions)
        for (size_t i = first; i < n_idx; i += stride) {
            const unsigned int vi = m.indices[i];
            if (vi >= m.n_verts) {   // (*) the comparison ...
                faults |= 1u << kMeshBadIndex;
                continue;
            }
            const float* v = m.positions + 3 * (size_t)vi;   // (*) ... and the load it guards: vi < n_verts here
            for (int a = 0; a < 3; ++a) {
                const float c = v[a];
                lo[a] = fminf(lo[a], c);
                hi[a] = fmaxf(hi[a], c);
            }
        }
    reduce_bounds<kMeshCheckThreads>(s_red, tid, lo, hi);   // (its first barrier orders s_words' zeros before the atomics)
    if (faults) atomicOr(&s_words[0], faults);
    if (max_material) atomicMax(&s_words[1], max_material);
    __syncthreads();
    if (tid < 6) partial[6 * (size_t)b + tid] = s_red[tid][0];
    else if (tid < 8) part_words[2 * (size_t)b + (tid - 6)] = s_words[tid - 6];
}

// one workgroup per mesh: its workgroups' partial boxes, fault bits and material indices -> report[mesh]
__global__ __launch_bounds__(kMeshCheckThreads) void mesh_check_final_kernel(const MeshSource* __restrict__ table, const float* __restrict__ partial,
                                                                             const unsigned int* __restrict__ part_words, MeshReport* __restrict__ report)
{
    __shared__ float s_red[6][kMeshCheckThreads];
    __shared__ unsigned int s_words[2];
    const int tid = threadIdx.x;
    if (tid < 2) s_words[tid] = 0u;
    const MeshSource m = table[blockIdx.x];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned int faults = 0, max_material = 0;
    for (int i = tid; i < m.n_blocks; i += kMeshCheckThreads) {
        const size_t p = (size_t)m.first_block + i;
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], partial[6 * p + a]);
            hi[a] = fmaxf(hi[a], partial[6 * p + 3 + a]);
        }
        faults |= part_words[2 * p];
        max_material = max(max_material, part_words[2 * p + 1]);
    }
    reduce_bounds<kMeshCheckThreads>(s_red, tid, lo, hi);
    if (faults) atomicOr(&s_words[0], faults);
    if (max_material) atomicMax(&s_words[1], max_material);
    __syncthreads();
    MeshReport& r = report[blockIdx.x];
    if (tid < 3) r.lo[tid] = s_red[tid][0];
    else if (tid < 6) r.hi[tid - 3] = s_red[tid][0];
    else if (tid == 6) r.faults = s_words[0];
    else if (tid == 7) r.max_material = s_words[1];
}

// The meshes of the table back to back in the five packed arrays (freshly allocated: 3 / 3 / 2 words per vertex, 3 / 1 per triangle of
// the scene), indices relative to their own mesh as given; zeros where a mesh has no normals, texture coordinates or materials.  The
// same runs of workgroups as mesh_check_kernel's, the same grid-stride shares, dword for dword.  (Every mesh of a scene has positions and
// indices: the host refused the call otherwise.)
__global__ __launch_bounds__(kMeshCheckThreads) void mesh_pack_kernel(const MeshSource* __restrict__ table, int n_entries, float* __restrict__ positions,
                                                                      float* __restrict__ normals, float* __restrict__ texcoords,
                                                                      unsigned int* __restrict__ indices, unsigned int* __restrict__ tri_material)
{
    const int tid = threadIdx.x, b = blockIdx.x;
    const MeshSource m = table[mesh_entry_of(table, n_entries, b)];
    const size_t first = (size_t)(b - m.first_block) * kMeshCheckThreads + tid, stride = (size_t)m.n_blocks * kMeshCheckThreads;
    const size_t n_pos = 3 * (size_t)m.n_verts, n_uv = 2 * (size_t)m.n_verts, n_idx = 3 * (size_t)m.n_tris;
    float* pos = positions + 3 * (size_t)m.vert_base;
    unsigned int* idx = indices + 3 * (size_t)m.tri_base;
    for (size_t i = first; i < n_pos; i += stride) pos[i] = m.positions[i];
    for (size_t i = first; i < n_idx; i += stride) idx[i] = m.indices[i];
    float* nrm = normals + 3 * (size_t)m.vert_base;
    float* uv = texcoords + 2 * (size_t)m.vert_base;
    unsigned int* mat = tri_material + m.tri_base;
    for (size_t i = first; i < n_pos; i += stride) nrm[i] = m.normals ? m.normals[i] : 0.0f;
    for (size_t i = first; i < n_uv; i += stride) uv[i] = m.texcoords ? m.texcoords[i] : 0.0f;
    for (size_t i = first; i < (size_t)m.n_tris; i += stride) mat[i] = m.material_of_triangle ? m.material_of_triangle[i] : 0u;
}

}  // namespace whitted
}  // namespace rtgo
