// rtgo_whitted_inst.h -- the whitted path over instanced meshes: sutil::Scene's two-level structure (one GAS per MeshGroup,
// buildMeshAccels; one OptixInstance per group in an IAS, buildInstanceAccel, sutil/Scene.cpp:985-1010) and getLocalGeometry's
// object-to-world mapping (cuda/LocalGeometry.h:84, 103, 112).
//
// Bottom level: every mesh gets the single-mesh path's structure (build_kernel + sah_kernel, unchanged), in OBJECT space; the meshes'
// records and Morton-ordered triangles sit back to back in one array each.  Top level: the same two 64-byte-record build run over the
// instances' world boxes (one box per instance, handed to build_kernel as the degenerate triangle (lo, hi, lo), whose bounds are the
// box); its leaves are runs of at most kLeafTris instances in Morton order, and the per-instance walk records (InstWalk) are stored
// in that order, so a leaf code indexes them directly.  At an instance the ray is taken to object space -- o' = W2O (o, 1),
// d' = W2O (d, 0), not renormalised, so t means the same in both spaces (OptiX's semantics) -- that mesh's records are walked with the
// current closest t, and the world ray is used again above.  Closest hit: smallest t, then lowest (instance, triangle).
#pragma once

#include "rtgo_whitted.h"

#include <type_traits>

namespace rtgo {
namespace whitted {

constexpr int kMaxMeshes = 256;
constexpr int kMaxInstances = 8192;     // the top level is built by build_kernel: at most kMaxTriangles boxes
constexpr int kMaxInstWalkDepth = 72;   // per-lane stack entries of both levels together: 1024 lanes x 72 x 2 B = 144 KiB of LDS
constexpr int kInstShift = 13;          // hit key = instance << kInstShift | triangle (triangles of a mesh < 2^13)
static_assert(kMaxInstances <= kMaxTriangles && kMaxTriangles <= (1 << kInstShift), "instance limits");

struct InstWalk {      // what the walk reads of an instance, 64 B, in the top level's leaf order
    float4 w2o[3];     // rows of the world-to-object 3x4 matrix (the inverse of the instance transform, computed in double on the host)
    int rec_base;      // the mesh's first record in InstParams::recs
    int tri_base;      // its first triangle in InstParams::tris (Morton order), indices and tri_material
    int root;          // 0: record 0 of the mesh; < 0: the leaf code of a mesh of at most kLeafTris triangles (no records);
                       // > 0: a clustered mesh (rec_base: its mid level's records), 1 + (cluster table base << 3 | mid_root_bits)
    int instance;      // the instance's index in the caller's array
};
struct InstShade {     // what shading reads of an instance, 112 B, in the caller's order
    float4 o2w[3];     // rows of the object-to-world 3x4 matrix (the instance transform as given)
    float4 w2o[3];     // InstWalk::w2o again
    int material_offset, vert_base, tri_base, flags;   // flags: kHasNormals | kHasTexcoords
};
constexpr int kHasNormals = 1, kHasTexcoords = 2;

struct InstParams {
    Frame frame;
    const float4* top_recs;     // the top level's records (layout of Params::recs; leaf codes index InstWalk)
    const InstWalk* inst;
    const InstShade* shade;
    int n_top_recs, n_instances;   // n_top_recs 0: every instance in one leaf
    const float4* recs;         // the meshes' records and Morton-ordered triangles (layout of Params::recs / tris), in object space
    const float4* tris;
    const int4* clusters;       // clustered meshes: (record base, triangle base, root, 0) per cluster, each mesh's in its mid level's leaf order
    const float* positions;     // all meshes' vertices back to back (InstShade::vert_base)
    const float* normals;       // (zero where a mesh has none: then N = Ng)
    const float* texcoords;     // (zero where a mesh has none: then UV = the barycentrics)
    const unsigned int* indices;       // per mesh, relative to its vertex base
    const unsigned int* tri_material;  // per mesh (0 where the mesh has none), before InstShade::material_offset
};

// M (p, 1) and M (d, 0) for a row-major 3x4 M; one rounding per operation in row order
__device__ __forceinline__ v3 xform_point(const float4 m0, const float4 m1, const float4 m2, v3 p)
{
    return mk(m0.x * p.x + m0.y * p.y + m0.z * p.z + m0.w, m1.x * p.x + m1.y * p.y + m1.z * p.z + m1.w, m2.x * p.x + m2.y * p.y + m2.z * p.z + m2.w);
}
__device__ __forceinline__ v3 xform_vector(const float4 m0, const float4 m1, const float4 m2, v3 d)
{
    return mk(m0.x * d.x + m0.y * d.y + m0.z * d.z, m1.x * d.x + m1.y * d.y + m1.z * d.z, m2.x * d.x + m2.y * d.y + m2.z * d.z);
}
// optixTransformNormalFromObjectToWorldSpace: W2O^T n
__device__ __forceinline__ v3 xform_normal(const float4 m0, const float4 m1, const float4 m2, v3 n)
{
    return mk(m0.x * n.x + m1.x * n.y + m2.x * n.z, m0.y * n.x + m1.y * n.y + m2.y * n.z, m0.z * n.x + m1.z * n.y + m2.z * n.z);
}

// the triangles of one leaf of one instance's mesh (leaf_tris with the two-level key).  The closest-hit walk asks for the whole leaf
// before testing it, as leaf_tris does; the occlusion walk, which runs with the shading state live beside it, one triangle at a time
// (the 48 VGPRs of a whole leaf would not fit next to that state without scratch).
// Key: int (instance << kInstShift | triangle) or, in a scene with clustered meshes, long long (instance << 32 | triangle).
template <bool ANY, typename Key>
__device__ __forceinline__ bool leaf_tris_inst(const float4* __restrict__ tris, int first, int cnt, v3 o, v3 d, float tmin, float tmax, Key kbase,
                                               int pos_base, Key& best, int& best_pos, float& bt, float& bu, float& bv)
{
    if constexpr (ANY) {
        for (int k = 0; k < cnt; ++k) {
            const float4 a = tris[3 * (first + k) + 0], b = tris[3 * (first + k) + 1], c = tris[3 * (first + k) + 2];
            float t, u, v;
            if (tri_intersect(mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(c.x, c.y, c.z), o, d, tmin, tmax, t, u, v)) {
                bt = t;
                bu = u;
                bv = v;
                best = kbase | (Key)__float_as_int(a.w);
                best_pos = pos_base + first + k;
                return true;
            }
        }
        return false;
    }
    float4 a[kLeafTris], b[kLeafTris], c[kLeafTris];
#pragma unroll
    for (int k = 0; k < kLeafTris; ++k) {
        a[k] = b[k] = c[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (k < cnt) {
            a[k] = tris[3 * (first + k) + 0];
            b[k] = tris[3 * (first + k) + 1];
            c[k] = tris[3 * (first + k) + 2];
        }
    }
#pragma unroll
    for (int k = 0; k < kLeafTris; ++k) {
        if (k < cnt) {
            const Key key = kbase | (Key)__float_as_int(a[k].w);
            float t, u, v;
            if (tri_intersect(mk(a[k].x, a[k].y, a[k].z), mk(b[k].x, b[k].y, b[k].z), mk(c[k].x, c[k].y, c[k].z), o, d, tmin, tmax, t, u, v) &&
                (t < bt || (t == bt && best >= 0 && key < best))) {
                bt = t;
                bu = u;
                bv = v;
                best = key;
                best_pos = pos_base + first + k;
                if (ANY) return true;
            }
        }
    }
    return false;
}

// One mesh's structure below an instance (ray in object space): its records from `root` (0: record 0; < 0: the leaf code of a mesh
// without records), its triangles at `tris`, which sit at pos_base of InstParams::tris.  Its stack entries go above the caller's, from
// sp on.  True only when ANY and a hit was found (the walk is over; sp is left where it was).
template <bool ANY, typename Key>
__device__ __forceinline__ bool walk_mesh(const float4* __restrict__ recs, const float4* __restrict__ tris, int root, int pos_base, Key kbase,
                                          unsigned short* __restrict__ s_stack, int stride, int& sp, v3 o, v3 d, v3 id, float tmin, float tmax, Key& best,
                                          int& best_pos, float& bt, float& bu, float& bv)
{
    const int floor = sp;
    int m = root;
    for (;;) {
        bool pop = true;
        if (m >= 0) {
            pop = !record_step(recs, m, s_stack, stride, sp, o, id, tmin, bt);
        } else {
            const int code = -1 - m;
            if (leaf_tris_inst<ANY>(tris, code & ((1 << kLeafShift) - 1), (code >> kLeafShift) + 1, o, d, tmin, tmax, kbase, pos_base, best, best_pos, bt, bu, bv))
                return true;
        }
        if (pop && !pop_entry(s_stack, stride, sp, floor, m)) return false;
    }
}

// Closest hit (ANY = false) or any hit (ANY = true) over the top level and the meshes below it.  pos_out = the hit triangle's position
// in InstParams::tris.  Each level keeps its stack entries above the one it came from, on the same lane stack, with its own floor;
// record indices and leaf codes stay local to their level.
//
// CLUSTERED: the scene holds clustered meshes (render_inst_kernel<*, true>): a mesh beyond kMaxTriangles triangles is a mid level over
// clusters of at most kClusterTris triangles, each with the single-mesh structure (rtgo_whitted_big.h).  At an instance the ray is
// taken to object space once; a clustered mesh's mid records are walked, and at a mid leaf each of its clusters' records with that
// cluster's bases.  A mesh of today's structure is walked as a mid level of one leaf holding one cluster (the instance's own bases).
// Key: instance << kInstShift | triangle, or with CLUSTERED (instance << 32 | the mesh's own triangle index), 64 bits: the same order,
// so a clustered mesh renders like the same triangles cut into contiguous identity instances.
constexpr int kMidHasRecords = 4;   // mid_root_bits: the mid level has records (root record 0); else the count - 1 of its one leaf's clusters
template <bool CLUSTERED>
using InstKey = std::conditional_t<CLUSTERED, long long, int>;
template <bool ANY, bool CLUSTERED>
__device__ __forceinline__ bool trace_inst(const InstParams& p, const float4* top, const InstWalk* inst, unsigned short* __restrict__ s_stack, int stride, v3 o,
                                           v3 d, float tmin, float tmax, InstKey<CLUSTERED>& key_out, int& pos_out, float& t_out, float& u_out, float& v_out)
{
    using Key = InstKey<CLUSTERED>;
    const v3 id = safe_inv(d);
    Key best = -1;
    int best_pos = 0;
    float bt = tmax, bu = 0.0f, bv = 0.0f;
    int sp = 0;
    int cur = p.n_top_recs > 0 ? 0 : -1 - ((p.n_instances - 1) << kLeafShift);
    bool done = false;
    for (;;) {
        bool pop = true;
        if (cur >= 0) {
            pop = !record_step(top, cur, s_stack, stride, sp, o, id, tmin, bt);
        } else {
            const int code = -1 - cur, first = code & ((1 << kLeafShift) - 1), cnt = (code >> kLeafShift) + 1;
            for (int k = 0; k < cnt && !done; ++k) {
                const InstWalk w = inst[first + k];
                const v3 oo = xform_point(w.w2o[0], w.w2o[1], w.w2o[2], o), od = xform_vector(w.w2o[0], w.w2o[1], w.w2o[2], d);
                const v3 oid = safe_inv(od);
                if constexpr (!CLUSTERED) {
                    done = walk_mesh<ANY>(p.recs + 4 * w.rec_base, p.tris + 3 * w.tri_base, w.root, w.tri_base, w.instance << kInstShift, s_stack, stride, sp, oo,
                                          od, oid, tmin, tmax, best, best_pos, bt, bu, bv);
                } else {
                    // the mid level
                    const Key kbase = (long long)w.instance << 32;
                    const bool big = w.root > 0;
                    const int bits = w.root - 1, tbase = bits >> 3;
                    const float4* __restrict__ mrecs = p.recs + 4 * w.rec_base;
                    const int gfloor = sp;
                    int g = (big && (bits & kMidHasRecords)) ? 0 : -1 - ((big ? (bits & 3) : 0) << kLeafShift);
                    for (;;) {
                        bool gpop = true;
                        if (g >= 0) {
                            gpop = !record_step(mrecs, g, s_stack, stride, sp, oo, oid, tmin, bt);
                        } else {
                            const int gc = -1 - g, gfirst = gc & ((1 << kLeafShift) - 1), gcnt = (gc >> kLeafShift) + 1;
                            for (int q = 0; q < gcnt && !done; ++q) {
                                const int4 cl = big ? p.clusters[tbase + gfirst + q] : make_int4(w.rec_base, w.tri_base, w.root, 0);
                                done = walk_mesh<ANY>(p.recs + 4 * cl.x, p.tris + 3 * cl.y, cl.z, cl.y, kbase, s_stack, stride, sp, oo, od, oid, tmin, tmax, best,
                                                      best_pos, bt, bu, bv);
                            }
                            if (done) break;
                        }
                        if (gpop && !pop_entry(s_stack, stride, sp, gfloor, g)) break;
                    }
                }
            }
            if (done) break;
        }
        if (pop && !pop_entry(s_stack, stride, sp, 0, cur)) break;
    }
    key_out = best;
    pos_out = best_pos;
    t_out = bt;
    u_out = bu;
    v_out = bv;
    return best >= 0;
}

// __closesthit__radiance at a hit of an instanced mesh, from the walk's answer: the hit key (trace_inst's), the triangle's position tpos in
// InstParams::tris, barycentrics (bu, bv) -- the hit geometry, then shade().  render_inst_kernel and whitted_shade_kernel
// (rtgo_whitted_shade.h) both call it.
template <bool CLUSTERED, typename Occluded>
__device__ __forceinline__ v3 inst_shade_hit(const InstParams& p, InstKey<CLUSTERED> key, int tpos, float bu, float bv, v3 rd, Occluded&& occluded, Rays& rays)
{
    // the corners in object space, o2w for P (LocalGeometry.h:84), W2O^T for the normals (:103, :112)
    const int ii = CLUSTERED ? (int)(key >> 32) : (int)(key >> kInstShift), tri = CLUSTERED ? (int)(key & 0xFFFFFFFF) : (int)(key & ((1 << kInstShift) - 1));
    const InstShade sh = p.shade[ii];
    const float4 c0 = p.tris[3 * tpos + 0], c1 = p.tris[3 * tpos + 1], c2 = p.tris[3 * tpos + 2];
    HitGeom h;
    h.i0 = h.i1 = h.i2 = 0;
    if (sh.flags) {
        h.i0 = (unsigned int)sh.vert_base + p.indices[3 * (sh.tri_base + tri) + 0];
        h.i1 = (unsigned int)sh.vert_base + p.indices[3 * (sh.tri_base + tri) + 1];
        h.i2 = (unsigned int)sh.vert_base + p.indices[3 * (sh.tri_base + tri) + 2];
    }
    h.P0 = mk(c0.x, c0.y, c0.z);
    h.P1 = mk(c1.x, c1.y, c1.z);
    h.P2 = mk(c2.x, c2.y, c2.z);
    h.w0 = 1.0f - bu - bv;
    h.bu = bu;
    h.bv = bv;
    h.P = xform_point(sh.o2w[0], sh.o2w[1], sh.o2w[2], vadd(vadd(vscale(h.P0, h.w0), vscale(h.P1, bu)), vscale(h.P2, bv)));
    const float4 m0 = sh.w2o[0], m1 = sh.w2o[1], m2 = sh.w2o[2];
    h.N = xform_normal(m0, m1, m2, vnormalize(vcross(vsub(h.P1, h.P0), vsub(h.P2, h.P0))));   // Ng: not unit length under a transform that is not rigid (:103, 116)
    if (sh.flags & kHasNormals) {
        const v3 N0 = ld3(p.normals, h.i0), N1 = ld3(p.normals, h.i1), N2 = ld3(p.normals, h.i2);
        h.N = vnormalize(xform_normal(m0, m1, m2, vadd(vadd(vscale(N0, h.w0), vscale(N1, bu)), vscale(N2, bv))));
    }
    h.texcoords = (sh.flags & kHasTexcoords) ? p.texcoords : nullptr;
    h.material = (unsigned int)sh.material_offset + p.tri_material[sh.tri_base + tri];
    return shade(p.frame, h, rd, occluded, rays);
}

// Instanced meshes: render_tiles' pipeline over the two-level walk.
// TOP_IN_LDS: the top level's records and the InstWalk array are copied into LDS ahead of the lanes' stacks; otherwise they are read
// through L2 like the meshes' records.  CLUSTERED: the scene holds a clustered mesh (trace_inst's mid level and 64-bit hit key).
// FRAMES: render_tiles'.
template <bool TOP_IN_LDS, bool CLUSTERED = false, bool FRAMES = false>
__global__ __launch_bounds__(kRenderBlock) void render_inst_kernel(const InstParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char wi_smem[];
    // LDS image.  TOP_IN_LDS: [top records, 64 B each][InstWalk, 64 B each][stacks];  otherwise: [stacks]
    float4* s_top = reinterpret_cast<float4*>(wi_smem);
    InstWalk* s_inst = reinterpret_cast<InstWalk*>(s_top + 4 * p.n_top_recs);
    const int stride = (int)blockDim.x;
    unsigned short* s_stack = (TOP_IN_LDS ? reinterpret_cast<unsigned short*>(s_inst + p.n_instances) : reinterpret_cast<unsigned short*>(wi_smem)) + threadIdx.x;
    auto preload = [&]() {
        if (TOP_IN_LDS) {
            for (int i = (int)threadIdx.x; i < 4 * p.n_top_recs; i += stride) s_top[i] = p.top_recs[i];
            for (int i = (int)threadIdx.x; i < p.n_instances; i += stride) s_inst[i] = p.inst[i];
            __syncthreads();
        }
    };
    const float4* top = TOP_IN_LDS ? static_cast<const float4*>(s_top) : p.top_recs;
    const InstWalk* inst = TOP_IN_LDS ? static_cast<const InstWalk*>(s_inst) : p.inst;
    auto occluded = [&](v3 o, v3 d, float t0, float t1) -> bool {
        InstKey<CLUSTERED> key;
        int pos;
        float t, u, v;
        return trace_inst<true, CLUSTERED>(p, top, inst, s_stack, stride, o, d, t0, t1, key, pos, t, u, v);
    };
    render_tiles<FRAMES>(p.frame, preload, [&](unsigned int x, unsigned int y, unsigned int subframe, Rays& rays) -> v3 {
        const v3 rd = raygen(p.frame, x, y, subframe);
        const v3 miss = p.frame.miss;   // (read ahead of the walk, as render_kernel does)
        InstKey<CLUSTERED> key;
        int tpos;
        float t, bu, bv;
        rays.total += 1;
        if (!trace_inst<false, CLUSTERED>(p, top, inst, s_stack, stride, p.frame.eye, rd, 0.01f, 1e16f, key, tpos, t, bu, bv)) return miss;
        return inst_shade_hit<CLUSTERED>(p, key, tpos, bu, bv, rd, occluded, rays);
    });
}

}  // namespace whitted
}  // namespace rtgo
