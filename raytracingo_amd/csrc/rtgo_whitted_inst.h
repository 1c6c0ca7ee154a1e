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
    const float4* top_recs;     // the top level's records (layout of Params::recs; leaf codes index InstWalk)
    const InstWalk* inst;
    const InstShade* shade;
    int n_top_recs, n_instances;   // n_top_recs 0: every instance in one leaf
    const float4* recs;         // the meshes' records and Morton-ordered triangles (layout of Params::recs / tris), in object space
    const float4* tris;
    const float* positions;     // all meshes' vertices back to back (InstShade::vert_base)
    const float* normals;       // (zero where a mesh has none: then N = Ng)
    const float* texcoords;     // (zero where a mesh has none: then UV = the barycentrics)
    const unsigned int* indices;       // per mesh, relative to its vertex base
    const unsigned int* tri_material;  // per mesh (0 where the mesh has none), before InstShade::material_offset
    int stack_depth;
    unsigned int* tile_counter;
    unsigned int* tile_counter_next;
    unsigned int tiles_x, tiles_y;
    unsigned int tile_stride;
    const MatTex* mat_tex;
    const Pbr* materials;
    const PointLight* lights;
    int n_lights;
    float4* accum;
    uchar4* image;
    unsigned int width, height, subframe;
    Share share;
    v3 eye, U, V, W, miss;
    unsigned long long* counters;
    const int4* clusters;       // clustered meshes: (record base, triangle base, root, 0) per cluster, each mesh's in its mid level's leaf order
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

// one step of either level: read one record (both children's boxes), descend into the nearer child that is hit, park the other
__device__ __forceinline__ bool record_step(const float4* __restrict__ recs, int& cur, unsigned short* __restrict__ s_stack, int stride, int& sp, v3 o,
                                            v3 id, float tmin, float bt)
{
    const float4 a0 = recs[4 * cur + 0], a1 = recs[4 * cur + 1], b0 = recs[4 * cur + 2], b1 = recs[4 * cur + 3];
    float tl, tr;
    const bool hl = node_hit(a0, a1, o, id, tmin, bt, tl);
    const bool hr = node_hit(b0, b1, o, id, tmin, bt, tr);
    const int ll = __float_as_int(a0.w), lr = __float_as_int(b0.w);
    const bool go_r = hr && (!hl || tr < tl);
    if (hl && hr) {
        const int far = go_r ? ll : lr;
        s_stack[sp * stride] = (unsigned short)(far >= 0 ? far : (0x8000 | (-1 - far)));
        ++sp;
    }
    if (hl || hr) {
        cur = go_r ? lr : ll;
        return true;
    }
    return false;
}
__device__ __forceinline__ bool pop_entry(const unsigned short* __restrict__ s_stack, int stride, int& sp, int sp_floor, int& cur)
{
    if (sp == sp_floor) return false;
    --sp;
    const int e = (int)s_stack[sp * stride];
    cur = (e & 0x8000) ? -1 - (e & 0x7FFF) : e;
    return true;
}

// closest hit (ANY = false) or any hit (ANY = true) over both levels.  key_out = instance << kInstShift | triangle; pos_out = the hit
// triangle's position in InstParams::tris.  The mesh walk keeps its stack entries above the top level's on the same lane stack.
template <bool ANY, typename Top, typename Inst>
__device__ __forceinline__ bool trace_inst(const InstParams& p, Top top, Inst inst, unsigned short* __restrict__ s_stack, int stride, v3 o, v3 d, float tmin,
                                           float tmax, int& key_out, int& pos_out, float& t_out, float& u_out, float& v_out)
{
    auto safe_inv = [](float x) { return fabsf(x) < 1e-30f ? copysignf(1e30f, x) : 1.0f / x; };
    const v3 id = mk(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
    int best = -1, best_pos = 0;
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
                const v3 oid = mk(safe_inv(od.x), safe_inv(od.y), safe_inv(od.z));
                const float4* __restrict__ recs = p.recs + 4 * w.rec_base;
                const float4* __restrict__ tris = p.tris + 3 * w.tri_base;
                const int kbase = w.instance << kInstShift;
                const int floor = sp;
                int m = w.root;
                for (;;) {
                    bool mpop = true;
                    if (m >= 0) {
                        mpop = !record_step(recs, m, s_stack, stride, sp, oo, oid, tmin, bt);
                    } else {
                        const int mc = -1 - m;
                        if (leaf_tris_inst<ANY>(tris, mc & ((1 << kLeafShift) - 1), (mc >> kLeafShift) + 1, oo, od, tmin, tmax, kbase, w.tri_base, best, best_pos, bt, bu,
                                                bv)) {   // (true only when ANY)
                            done = true;
                            break;
                        }
                    }
                    if (mpop && !pop_entry(s_stack, stride, sp, floor, m)) break;
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

// trace_inst over scenes that hold clustered meshes (render_inst_kernel<*, true>): a mesh beyond kMaxTriangles triangles is a mid level
// over clusters of at most kClusterTris triangles, each with the single-mesh structure (rtgo_whitted_big.h).  At an instance the ray is
// taken to object space once; a clustered mesh's mid records are walked, and at a mid leaf each of its clusters' records with that
// cluster's bases.  A mesh of today's structure is walked as a mid level of one leaf holding one cluster (the instance's own bases).
// Each level keeps its stack entries above the one it came from, on the same lane stack, with its own floor; record indices and leaf
// codes stay local to their level.  The hit key is (instance << 32 | the mesh's own triangle index), 64 bits: the same order as
// trace_inst's key, so a clustered mesh renders like the same triangles cut into contiguous identity instances.
constexpr int kMidHasRecords = 4;   // mid_root_bits: the mid level has records (root record 0); else the count - 1 of its one leaf's clusters
template <bool ANY, typename Top, typename Inst>
__device__ __forceinline__ bool trace_inst_big(const InstParams& p, Top top, Inst inst, unsigned short* __restrict__ s_stack, int stride, v3 o, v3 d,
                                               float tmin, float tmax, long long& key_out, int& pos_out, float& t_out, float& u_out, float& v_out)
{
    auto safe_inv = [](float x) { return fabsf(x) < 1e-30f ? copysignf(1e30f, x) : 1.0f / x; };
    const v3 id = mk(safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
    long long best = -1;
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
                const v3 oid = mk(safe_inv(od.x), safe_inv(od.y), safe_inv(od.z));
                const long long kbase = (long long)w.instance << 32;
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
                            const float4* __restrict__ recs = p.recs + 4 * cl.x;
                            const float4* __restrict__ tris = p.tris + 3 * cl.y;
                            const int floor = sp;
                            int m = cl.z;
                            for (;;) {
                                bool mpop = true;
                                if (m >= 0) {
                                    mpop = !record_step(recs, m, s_stack, stride, sp, oo, oid, tmin, bt);
                                } else {
                                    const int mc = -1 - m;
                                    if (leaf_tris_inst<ANY>(tris, mc & ((1 << kLeafShift) - 1), (mc >> kLeafShift) + 1, oo, od, tmin, tmax, kbase, cl.y, best,
                                                            best_pos, bt, bu, bv)) {   // (true only when ANY)
                                        done = true;
                                        break;
                                    }
                                }
                                if (mpop && !pop_entry(s_stack, stride, sp, floor, m)) break;
                            }
                        }
                        if (done) break;
                    }
                    if (gpop && !pop_entry(s_stack, stride, sp, gfloor, g)) break;
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

// render_kernel's pipeline (same tile queue, __raygen__pinhole, accumulation and make_color) over the two-level structure.
// TOP_IN_LDS: the top level's records and the InstWalk array are copied into LDS ahead of the lanes' stacks; otherwise they are read
// through L2 like the meshes' records.  CLUSTERED: the scene holds a clustered mesh (trace_inst_big and its 64-bit hit key).
template <bool TOP_IN_LDS, bool CLUSTERED = false>
__global__ __launch_bounds__(kRenderBlock) void render_inst_kernel(const InstParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char wi_smem[];
    // LDS image.  TOP_IN_LDS: [top records, 64 B each][InstWalk, 64 B each][stacks];  otherwise: [stacks]
    float4* s_top = reinterpret_cast<float4*>(wi_smem);
    InstWalk* s_inst = reinterpret_cast<InstWalk*>(s_top + 4 * p.n_top_recs);
    const int stride = (int)blockDim.x;
    unsigned short* s_stack = (TOP_IN_LDS ? reinterpret_cast<unsigned short*>(s_inst + p.n_instances) : reinterpret_cast<unsigned short*>(wi_smem)) + threadIdx.x;
    if (TOP_IN_LDS) {
        for (int i = (int)threadIdx.x; i < 4 * p.n_top_recs; i += stride) s_top[i] = p.top_recs[i];
        for (int i = (int)threadIdx.x; i < p.n_instances; i += stride) s_inst[i] = p.inst[i];
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x < (unsigned int)kTileHeads) p.tile_counter_next[kTileHeadStride * threadIdx.x] = 0u;
    auto pick_top = [&]() {
        if constexpr (TOP_IN_LDS) return static_cast<const float4*>(s_top);
        else return p.top_recs;
    };
    auto pick_inst = [&]() {
        if constexpr (TOP_IN_LDS) return static_cast<const InstWalk*>(s_inst);
        else return p.inst;
    };
    const auto top = pick_top();
    const auto inst = pick_inst();
    const unsigned int lane = threadIdx.x & 63u;
    const unsigned int n_tiles = p.tiles_x * p.tiles_y;
    unsigned int rays = 0, occl = 0;
    // the tile queue of render_kernel
    auto tiles_of = [&](unsigned int h) { return (n_tiles + (unsigned int)kTileHeads - 1u - h) / (unsigned int)kTileHeads; };
    unsigned int head = blockIdx.x % (unsigned int)kTileHeads;
    unsigned int pending = 0u;
    if (lane == 0u) pending = atomicAdd(p.tile_counter + kTileHeadStride * head, 1u);
    for (;;) {
        unsigned int pos = (unsigned int)__builtin_amdgcn_readfirstlane((int)pending);
        if (pos >= tiles_of(head)) {
            unsigned int v = 0xFFFFFFFFu;
            if (lane < (unsigned int)kTileHeads) v = __hip_atomic_load(p.tile_counter + kTileHeadStride * lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long open = __builtin_amdgcn_ballot_w64(lane < (unsigned int)kTileHeads && v < tiles_of(lane));
            if (open == 0ull) break;
            const unsigned long long above = open & ~((2ull << head) - 1ull);
            head = (unsigned int)(__ffsll((long long)(above ? above : open)) - 1);
            if (lane == 0u) pending = atomicAdd(p.tile_counter + kTileHeadStride * head, 1u);
            continue;
        }
        const unsigned int tile = (unsigned int)(((unsigned long long)(pos * (unsigned int)kTileHeads + head) * p.tile_stride) % n_tiles);
        if (lane == 0u) pending = atomicAdd(p.tile_counter + kTileHeadStride * head, 1u);
        const unsigned int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
        const unsigned int lx = tx * 8u + (lane & 7u), ly = ty * 8u + (lane >> 3);   // render_kernel's share mapping
        if (lx < p.share.lw && ly < p.share.lh) {
            const unsigned int idx = ly * p.share.lw + lx;
            const unsigned int x = p.share.x0 + lx, y = share_row(p.share, ly);
            // __raygen__pinhole, whitted.cu:183-240
            unsigned int seed = tea4(y * p.width + x, p.subframe);
            float jx = 0.0f, jy = 0.0f;
            if (p.subframe != 0) {
                jx = rnd(seed) - 0.5f;
                jy = rnd(seed) - 0.5f;
            }
            const float dx = 2.0f * div_cr((float)x + jx, (float)p.width) - 1.0f;
            const float dy = 2.0f * div_cr((float)y + jy, (float)p.height) - 1.0f;
            const v3 rd = vnormalize(vadd(vadd(vscale(p.U, dx), vscale(p.V, dy)), p.W));
            const v3 ro = p.eye;
            v3 result = p.miss;
            std::conditional_t<CLUSTERED, long long, int> key;
            int tpos;
            float t, bu, bv;
            rays += 1;
            bool hit;
            if constexpr (CLUSTERED) hit = trace_inst_big<false>(p, top, inst, s_stack, stride, ro, rd, 0.01f, 1e16f, key, tpos, t, bu, bv);
            else hit = trace_inst<false>(p, top, inst, s_stack, stride, ro, rd, 0.01f, 1e16f, key, tpos, t, bu, bv);
            if (hit) {
                // __closesthit__radiance, :255-337, with getLocalGeometry (LocalGeometry.h:55-141) of an instanced mesh
                const int ii = CLUSTERED ? (int)(key >> 32) : (int)(key >> kInstShift), tri = CLUSTERED ? (int)(key & 0xFFFFFFFF) : (int)(key & ((1 << kInstShift) - 1));
                const InstShade sh = p.shade[ii];
                const float4 c0 = p.tris[3 * tpos + 0], c1 = p.tris[3 * tpos + 1], c2 = p.tris[3 * tpos + 2];   // object space
                unsigned int i0 = 0, i1 = 0, i2 = 0;
                if (sh.flags) {
                    i0 = (unsigned int)sh.vert_base + p.indices[3 * (sh.tri_base + tri) + 0];
                    i1 = (unsigned int)sh.vert_base + p.indices[3 * (sh.tri_base + tri) + 1];
                    i2 = (unsigned int)sh.vert_base + p.indices[3 * (sh.tri_base + tri) + 2];
                }
                // the instance's two matrices: o2w for P (:84), W2O^T for the normals (:103, :112)
                const v3 P0 = mk(c0.x, c0.y, c0.z), P1 = mk(c1.x, c1.y, c1.z), P2 = mk(c2.x, c2.y, c2.z);
                const float w0 = 1.0f - bu - bv;
                const v3 P = xform_point(sh.o2w[0], sh.o2w[1], sh.o2w[2], vadd(vadd(vscale(P0, w0), vscale(P1, bu)), vscale(P2, bv)));
                const float4 m0 = sh.w2o[0], m1 = sh.w2o[1], m2 = sh.w2o[2];
                const v3 Ng = xform_normal(m0, m1, m2, vnormalize(vcross(vsub(P1, P0), vsub(P2, P0))));
                v3 N = Ng;   // (not unit length under a transform that is not rigid: LocalGeometry.h:103, 116)
                if (sh.flags & kHasNormals) {
                    const v3 N0 = ld3(p.normals, i0), N1 = ld3(p.normals, i1), N2 = ld3(p.normals, i2);
                    N = vnormalize(xform_normal(m0, m1, m2, vadd(vadd(vscale(N0, w0), vscale(N1, bu)), vscale(N2, bv))));
                }
                const unsigned int mi = (unsigned int)sh.material_offset + p.tri_material[sh.tri_base + tri];
                const Pbr m = p.materials[mi];
                v3 base = mk(m.base_color[0], m.base_color[1], m.base_color[2]);
                float mr_y = 1.0f, mr_z = 1.0f;
                if (p.mat_tex) {
                    const MatTex mt = p.mat_tex[mi];
                    if (mt.base_color.px || mt.metallic_roughness.px || mt.normal.px) {
                        float2 UV0 = make_float2(0.0f, 0.0f), UV1 = make_float2(0.0f, 1.0f), UV2 = make_float2(1.0f, 0.0f), UV = make_float2(bu, bv);
                        if (sh.flags & kHasTexcoords) {
                            UV0 = make_float2(p.texcoords[2 * i0], p.texcoords[2 * i0 + 1]);
                            UV1 = make_float2(p.texcoords[2 * i1], p.texcoords[2 * i1 + 1]);
                            UV2 = make_float2(p.texcoords[2 * i2], p.texcoords[2 * i2 + 1]);
                            UV = make_float2(w0 * UV0.x + bu * UV1.x + bv * UV2.x, w0 * UV0.y + bu * UV1.y + bv * UV2.y);
                        }
                        if (mt.base_color.px) {
                            const float4 tc = tex2d(mt.base_color, UV.x, UV.y);
                            base = vmul(base, mk(powf(tc.x, 2.2f), powf(tc.y, 2.2f), powf(tc.z, 2.2f)));
                        }
                        if (mt.metallic_roughness.px) {
                            const float4 tc = tex2d(mt.metallic_roughness, UV.x, UV.y);
                            mr_y = tc.y;
                            mr_z = tc.z;
                        }
                        if (mt.normal.px) {
                            // whitted.cu:288-292: dp/du, dp/dv stay in OBJECT space (LocalGeometry.h:118-134) beside the world N
                            const float du1 = UV0.x - UV2.x, du2 = UV1.x - UV2.x, dv1 = UV0.y - UV2.y, dv2 = UV1.y - UV2.y;
                            const v3 dp1 = vsub(P0, P2), dp2 = vsub(P1, P2);
                            const float det = du1 * dv2 - dv1 * du2;
                            const float invdet = 1.0f / det;
                            const v3 dpdu = vscale(vsub(vscale(dp1, dv2), vscale(dp2, dv1)), invdet);
                            const v3 dpdv = vscale(vadd(vscale(dp1, -du2), vscale(dp2, du1)), invdet);
                            const float4 tc = tex2d(mt.normal, UV.x, UV.y);
                            const float nx = 2.0f * tc.x - 1.0f, ny = 2.0f * tc.y - 1.0f, nz = 2.0f * tc.z - 1.0f;
                            N = vnormalize(vadd(vadd(vscale(vnormalize(dpdu), nx), vscale(vnormalize(dpdv), ny)), vscale(N, nz)));
                        }
                    }
                }
                const float metallic = m.metallic * mr_z, roughness = m.roughness * mr_y;
                const float F0 = 0.04f;
                const v3 diff_color = vscale(vscale(base, 1.0f - F0), 1.0f - metallic);
                const v3 spec_color = vadd(mk(F0, F0, F0), vscale(vsub(base, mk(F0, F0, F0)), metallic));
                const float alpha = roughness * roughness;
                result = mk(0.0f, 0.0f, 0.0f);
                for (int l = 0; l < p.n_lights; ++l) {
                    const PointLight L = p.lights[l];
                    const v3 toL = vsub(mk(L.position[0], L.position[1], L.position[2]), P);
                    const float Ldist = vlength(toL);
                    const v3 Lv = vscale(toL, 1.0f / Ldist);
                    const v3 Vv = vneg(vnormalize(rd));   // the WORLD ray direction (whitted.cu:307)
                    const v3 H = vnormalize(vadd(Lv, Vv));
                    const float NdotL = vdot(N, Lv), NdotV = vdot(N, Vv), NdotH = vdot(N, H), VdotH = vdot(Vv, H);
                    if (NdotL > 0.0f && NdotV > 0.0f) {
                        rays += 1;
                        occl += 1;
                        std::conditional_t<CLUSTERED, long long, int> ok;
                        int opos;
                        float ot, ou, ov;
                        bool occluded;
                        if constexpr (CLUSTERED) occluded = trace_inst_big<true>(p, top, inst, s_stack, stride, P, Lv, 0.001f, Ldist - 0.001f, ok, opos, ot, ou, ov);
                        else occluded = trace_inst<true>(p, top, inst, s_stack, stride, P, Lv, 0.001f, Ldist - 0.001f, ok, ok, ot, ou, ov);
                        if (!occluded) {
                            const v3 F = schlick(spec_color, VdotH);
                            const float G = vis(NdotL, NdotV, alpha);
                            const float D = ggx_normal(NdotH, alpha);
                            const v3 one_minus_F = vsub(mk(1.0f, 1.0f, 1.0f), F);
                            const v3 dd = vmul(one_minus_F, diff_color);
                            const float ip = 1.0f / kPi;
                            const v3 diff = vscale(dd, ip);
                            const v3 spec = vscale(vscale(F, G), D);
                            const v3 lc = vscale(mk(L.color[0], L.color[1], L.color[2]), L.intensity);
                            result = vadd(result, vmul(vscale(lc, NdotL), vadd(diff, spec)));
                        }
                    }
                }
            }
            // whitted.cu:226-239
            v3 acc = result;
            if (p.subframe > 0) {
                const float a = 1.0f / (float)(p.subframe + 1);
                const float4 prev = p.accum[idx];
                acc = vadd(mk(prev.x, prev.y, prev.z), vscale(vsub(acc, mk(prev.x, prev.y, prev.z)), a));
            }
            p.accum[idx] = make_float4(acc.x, acc.y, acc.z, 1.0f);
            const float g = (float)(1.0 / 2.2f);
            p.image[idx] = make_uchar4((unsigned char)(powf(clampf(acc.x, 0.0f, 1.0f), g) * 255.0f), (unsigned char)(powf(clampf(acc.y, 0.0f, 1.0f), g) * 255.0f),
                                       (unsigned char)(powf(clampf(acc.z, 0.0f, 1.0f), g) * 255.0f), 255u);
        }
    }
    rays = wave_sum(rays);
    occl = wave_sum(occl);
    if (lane == 0u) {
        atomicAdd(&p.counters[0], (unsigned long long)rays);
        atomicAdd(&p.counters[1], (unsigned long long)occl);
    }
}

}  // namespace whitted
}  // namespace rtgo
