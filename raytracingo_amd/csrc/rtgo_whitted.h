// rtgo_whitted.h -- gfx950 device code of the "whitted" triangle path: the programs of the reference's cuda/whitted.cu
// (__raygen__pinhole :183-240, __miss__constant_radiance :243-246, __closesthit__occlusion :249-252, __closesthit__radiance
// :255-337 with cuda/LocalGeometry.h:55-141) over triangle meshes, without textures.  The reference hands triangle
// intersection and the acceleration structure to OptiX (built-in triangles, optixAccelBuild in sutil/Scene.cpp); here both are
// written out: a Moeller-Trumbore test with a fixed operation order (shared with the oracle, so the two agree bit for bit) and
// an LBVH over the triangles built on the device by one workgroup (Morton codes -> bitonic sort in LDS -> Karras hierarchy ->
// bottom-up fit -> subtrees of at most four triangles collapsed into leaves, one 64-byte record per remaining node holding
// BOTH children's boxes).  The render kernel is persistent like the analytic path's: one workgroup of 1024 threads per CU keeps
// the records in LDS (when they fit: always below ~2000 triangles, usually up to the limit), its waves pull 8 x 8-pixel tiles
// from a counter; one lane = one pixel, one launch per subframe: a primary ray plus one shadow ray per point light, no
// recursion (whitted.cu traces none either).  rtgo_whitted_launch_frames renders n subframes in one launch: the FRAMES instantiations,
// S lanes per pixel (render_tiles).
//
// Compiled with -ffp-contract=off like the rest of the library: one IEEE rounding per operation.
#pragma once

#include "rtgo_device.h"

namespace rtgo {
namespace whitted {

constexpr int kMaxTriangles = 8192;   // one workgroup sorts the Morton keys in (dynamic) LDS, 8 B per key; leaf codes and 2-byte stack entries hold 13 bits of triangle position
constexpr int kLeafShift = 13;        // leaf code = first sorted triangle | (count - 1) << kLeafShift   (count <= 4: 15 bits, what a stack entry holds beside its flag)
constexpr int kBuildThreads = 1024;
constexpr int kStack = 32;            // the bottom-up fit runs 2 * kStack + 2 = 66 passes: enough for any Karras hierarchy over 30-bit codes of <= 8192 triangles (depth <= 43)
constexpr int kRenderBlock = 1024;    // one workgroup per CU shares one LDS copy of the records
constexpr size_t kRenderLds = 160 * 1024;   // the most LDS a render workgroup takes: its stacks and what of the structure fits beside them
#ifndef RTGO_LEAF_TRIS
#define RTGO_LEAF_TRIS 4
#endif
constexpr int kLeafTris = RTGO_LEAF_TRIS;          // a subtree of at most this many triangles is one leaf of the walk
constexpr int kMaxWalkDepth = 40;
// where the walk reads from: records and triangles in L2 / fp32 records in LDS, triangles in L2 / quantised records, vertices and
// triangle indices all in LDS
constexpr int kAllInL2 = 0, kRecordsInLds = 1, kAllInLds = 2;
constexpr int kTileHeads = 32;        // tile-queue heads (<= 64), kTileHeadStride words apart
constexpr unsigned int kTileHeadStride = 16;     // words between two heads: one 64-byte line each

struct PointLight {   // Light::Point, cuda/Light.h:47-53
    float color[3];
    float intensity;
    float position[3];
    int falloff;      // never read by whitted.cu
};

struct Pbr {          // MaterialData::Pbr without its texture handles, cuda/MaterialData.h:43-52
    float base_color[4];
    float metallic, roughness;
};

// one texture of a material (cudaTextureObject_t of sutil::Scene::addSampler, sutil/Scene.cpp:505-538: RGBA8 read as normalised floats,
// normalised coordinates, and -- because addSampler compares its CUDA enums with GL constants -- always wrap addressing and linear filtering)
struct Tex {
    const uchar4* px;           // row 0 first; null: the material has no such texture
    unsigned int w, h;
};
struct MatTex {                 // MaterialData::Pbr's three handles, cuda/MaterialData.h:43-52
    Tex base_color, metallic_roughness, normal;
};

// The window and row band one launch renders (rtgo_whitted_frame): its k-th owned window row is row k of a compact lw-wide buffer, as on
// the analytic path.  The full frame is x0 = y0 = 0, lw x lh = width x height, one rank.
struct Share {
    unsigned int x0, y0, lw, lh;   // lh: rows this rank owns (rtgo_local_rows)
    unsigned int band_h, n_ranks, rank;
};

// local row -> global row under the band interleave (the analytic kernel's, rtgo_device.h)
__device__ __forceinline__ unsigned int share_row(const Share& s, unsigned int ly)
{
    const unsigned int band = ly / s.band_h;
    return s.y0 + (band * s.n_ranks + s.rank) * s.band_h + (ly - band * s.band_h);
}

// What a launch renders, whatever structure it walks (rtgo_whitted_launch_frame fills it once; Params and InstParams embed it)
struct Frame {
    unsigned int* tile_counter; // this launch's tile queue heads (kTileHeads of them, zero at launch) and the set it zeroes for the next launch
    unsigned int* tile_counter_next;
    unsigned int tiles_x, tiles_y;  // 8 x 8 tiles over the compact local image, lw x lh
    unsigned int tile_stride;   // coprime to tiles_x * tiles_y
    unsigned int lanes_log2;    // the FRAMES kernels alone (rtgo_whitted_launch_frames): 1 << lanes_log2 lanes per pixel, so tiles of
                                //   64 >> lanes_log2 pixels (tiles_x, tiles_y and tile_stride count those); n_subframes goes with it.
                                //   (The two sit in the words the pointers' alignment left empty: the layout is the single launch's.)
    const MatTex* mat_tex;      // per material, or null when no material has a texture
    const Pbr* materials;
    const PointLight* lights;
    int n_lights;
    unsigned int n_subframes;   // FRAMES: the launch renders subframes subframe .. subframe + n_subframes - 1
    float4* accum;              // lw x lh, local row k = the k-th window row this launch owns
    uchar4* image;
    unsigned int width, height, subframe;   // the FULL image: seeds and ray directions
    Share share;
    v3 eye, U, V, W, miss;
    unsigned long long* counters;   // [0] rays_total [1] rays_occlusion
};
static_assert(sizeof(Frame) == 192 && alignof(Frame) == 8, "Frame: lanes_log2 and n_subframes fill the two padding words");

struct Params {       // whitted::LaunchParams, cuda/whitted.h:59-74, over one mesh in world space
    Frame frame;
    const float4* recs;         // the walk's records, 4 float4 each: (left min, left link) (left max, -) (right min, right link) (right max, -);
                                //   link >= 0: a record; link < 0: a leaf, -1 - (first sorted triangle | (count - 1) << kLeafShift)
    const float4* tris;         // 3 float4 per triangle in Morton order: (P0, original index) (P1, -) (P2, -)
    // the compact form of the same structure, for meshes that fit a CU's LDS whole (kAllInLds):
    const uint4* qrecs;         // 2 uint4 per record: (x, y, z planes of the left box as lo | hi << 16 on a 16-bit grid, left link), same for the right box
    const uint2* tidx;          // per triangle in Morton order: (v0 | v1 << 16, v2 | original index << 16)
    int n_vertices;
    v3 grid_lo, grid_step;      // world = grid_lo + cell * grid_step
    int n_recs;                 // 0: the whole mesh is one leaf (at most kLeafTris triangles)
    int n_triangles;
    const float* positions;     // 3 floats per vertex
    const float* normals;       // 3 floats per vertex, or null (then N = Ng, LocalGeometry.h:113-116)
    const unsigned int* indices;    // 3 per triangle
    const unsigned int* tri_material;
    const float* texcoords;     // 2 floats per vertex, or null (then UV = the barycentrics, LocalGeometry.h:97-102)
};

// tea<4>, cuda/random.h:30-45 with N = 4
__device__ __forceinline__ unsigned int tea4(unsigned int v0, unsigned int v1)
{
    unsigned int s0 = 0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        s0 += 0x9e3779b9u;
        v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
        v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    return v0;
}

__device__ __forceinline__ v3 ld3(const float* p, unsigned int i) { return mk(p[3 * i + 0], p[3 * i + 1], p[3 * i + 2]); }

// Moeller-Trumbore, two-sided (OptiX built-in triangles cull nothing unless asked to); the operation order is the contract
// between this kernel and the oracle (oracle_tri_intersect).  Accepts tmin < t < tmax like the analytic path.
__device__ __forceinline__ bool tri_intersect(v3 p0, v3 p1, v3 p2, v3 o, v3 d, float tmin, float tmax, float& t_out, float& u_out, float& v_out)
{
    const v3 e1 = vsub(p1, p0), e2 = vsub(p2, p0);
    const v3 pv = vcross(d, e2);
    const float det = vdot(e1, pv);
    if (det == 0.0f) return false;
    const float inv = div_cr(1.0f, det);   // (rtgo_device.h: the compiler's own correctly rounded steps; |det| is 0 or far above 2^-96 for triangles of any sane size)
    const v3 tv = vsub(o, p0);
    const float u = vdot(tv, pv) * inv;
    if (u < 0.0f || u > 1.0f) return false;
    const v3 qv = vcross(tv, e1);
    const float v = vdot(d, qv) * inv;
    if (v < 0.0f || u + v > 1.0f) return false;
    const float t = vdot(e2, qv) * inv;
    if (!(t > tmin && t < tmax)) return false;
    t_out = t;
    u_out = u;
    v_out = v;
    return true;
}

// slab test of a node box (exact reciprocal: the boxes carry a small pad, see build)
__device__ __forceinline__ bool node_hit(const float4 q0, const float4 q1, v3 o, v3 id, float tmin, float tmax, float& tn)
{
    float t0 = (q0.x - o.x) * id.x, t1 = (q1.x - o.x) * id.x;
    float a = fminf(t0, t1), b = fmaxf(t0, t1);
    t0 = (q0.y - o.y) * id.y;
    t1 = (q1.y - o.y) * id.y;
    a = fmaxf(a, fminf(t0, t1));
    b = fminf(b, fmaxf(t0, t1));
    t0 = (q0.z - o.z) * id.z;
    t1 = (q1.z - o.z) * id.z;
    a = fmaxf(a, fminf(t0, t1));
    b = fminf(b, fmaxf(t0, t1));
    a = fmaxf(a, tmin);
    b = fminf(b, tmax);
    tn = a;
    return a <= b * 1.000002f + 1e-7f;
}

// the triangles [first, first + cnt) of one leaf, in Morton order (contiguous 48-byte records).  All of them are asked for before
// the first one is tested: one round trip to L2 per leaf instead of one per triangle.
template <bool ANY>
__device__ __forceinline__ bool leaf_tris(const float4* __restrict__ tris, int first, int cnt, v3 o, v3 d, float tmin, float tmax, int& best, int& best_pos,
                                          float& bt, float& bu, float& bv)
{
    float4 a[kLeafTris], b[kLeafTris], c[kLeafTris];
#pragma unroll
    for (int k = 0; k < kLeafTris; ++k) {
        a[k] = b[k] = c[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (k < cnt) {   // (lanes whose leaf is shorter ask for nothing: the memory pipeline is paced by addresses, not by instructions)
            a[k] = tris[3 * (first + k) + 0];
            b[k] = tris[3 * (first + k) + 1];
            c[k] = tris[3 * (first + k) + 2];
        }
    }
#pragma unroll
    for (int k = 0; k < kLeafTris; ++k) {
        if (k < cnt) {
            const int tri = __float_as_int(a[k].w);
            float t, u, v;
            if (tri_intersect(mk(a[k].x, a[k].y, a[k].z), mk(b[k].x, b[k].y, b[k].z), mk(c[k].x, c[k].y, c[k].z), o, d, tmin, tmax, t, u, v) &&
                (t < bt || (t == bt && best >= 0 && tri < best))) {
                bt = t;
                bu = u;
                bv = v;
                best = tri;
                best_pos = first + k;
                if (ANY) return true;
            }
        }
    }
    return false;
}

// the reciprocal direction of the slab tests (exact, with a finite stand-in for division by zero)
__device__ __forceinline__ v3 safe_inv(v3 d)
{
    auto inv = [](float x) { return fabsf(x) < 1e-30f ? copysignf(1e30f, x) : 1.0f / x; };
    return mk(inv(d.x), inv(d.y), inv(d.z));
}

// One step of a walk over 64-byte records (every level of every walk but trace_lds): read ONE record -- both children's boxes, 64
// contiguous bytes -- descend into the nearer child that is hit and park the other one on the lane's stack (2-byte entries: a record
// index, or 0x8000 | leaf code).  False: neither child is hit.
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
// the next parked entry above sp_floor (a level's own part of the lane stack); false: that part is empty
__device__ __forceinline__ bool pop_entry(const unsigned short* __restrict__ s_stack, int stride, int& sp, int sp_floor, int& cur)
{
    if (sp == sp_floor) return false;
    --sp;
    const int e = (int)s_stack[sp * stride];
    cur = (e & 0x8000) ? -1 - (e & 0x7FFF) : e;
    return true;
}

// closest hit (ANY = false: smallest t, lowest triangle index on ties) or any hit (ANY = true: the occlusion ray's
// OPTIX_RAY_FLAG_TERMINATE_ON_FIRST_HIT, whitted.cu:140-151) over the triangle LBVH, one record_step at a time.
template <bool ANY>
__device__ __forceinline__ bool trace(const Params& p, const float4* recs, unsigned short* __restrict__ s_stack, int stride, v3 o, v3 d, float tmin, float tmax,
                                      int& tri_out, int& pos_out, float& t_out, float& u_out, float& v_out)
{
    const v3 id = safe_inv(d);
    int best = -1, best_pos = 0;
    float bt = tmax, bu = 0.0f, bv = 0.0f;
    if (p.n_recs == 0) {
        leaf_tris<ANY>(p.tris, 0, p.n_triangles, o, d, tmin, tmax, best, best_pos, bt, bu, bv);
    } else {
        int sp = 0;
        int cur = 0;   // >= 0: a record; < 0: a leaf code
        for (;;) {
            bool pop = true;
            if (cur >= 0) {
                pop = !record_step(recs, cur, s_stack, stride, sp, o, id, tmin, bt);
            } else {
                const int code = -1 - cur;
                if (leaf_tris<ANY>(p.tris, code & ((1 << kLeafShift) - 1), (code >> kLeafShift) + 1, o, d, tmin, tmax, best, best_pos, bt, bu, bv)) break;   // (true only when ANY)
            }
            if (pop && !pop_entry(s_stack, stride, sp, 0, cur)) break;
        }
    }
    tri_out = best;
    pos_out = best_pos;
    t_out = bt;
    u_out = bu;
    v_out = bv;
    return best >= 0;
}

// whitted.cu:49-80 (powf / sqrtf are the device libm's)
__device__ __forceinline__ v3 schlick(v3 spec, float VdotH)
{
    const float k = powf(1.0f - VdotH, 5.0f);
    return vadd(spec, vscale(vsub(mk(1.0f, 1.0f, 1.0f), spec), k));
}
__device__ __forceinline__ float vis(float NdotL, float NdotV, float alpha)
{
    const float a2 = alpha * alpha;
    const float g0 = NdotL * sqrt_cr(NdotV * NdotV * (1.0f - a2) + a2);
    const float g1 = NdotV * sqrt_cr(NdotL * NdotL * (1.0f - a2) + a2);
    return 2.0f * NdotL * NdotV / (g0 + g1);
}
__device__ __forceinline__ float ggx_normal(float NdotH, float alpha)
{
    const float a2 = alpha * alpha;
    const float n2 = NdotH * NdotH;
    const float x = n2 * (a2 - 1.0f) + 1.0f;
    return a2 / (kPi * x * x);
}

// tex2D<float4>( tex, u, v ) of a cudaReadModeNormalizedFloat / normalizedCoords / cudaAddressModeWrap / cudaFilterModeLinear texture, as
// the CUDA programming guide states it (appendix "Texture Fetching", linear filtering): x = u N, xB = x - 0.5, i = floor(xB),
// alpha = frac(xB) kept in 1.8 fixed point (8 fractional bits; rounded to nearest here -- the hardware's rounding is not published:
// parity unpinned), tex = (1-a)(1-b) T[i,j] + a (1-b) T[i+1,j] + (1-a) b T[i,j+1] + a b T[i+1,j+1] with indices wrapped.
// The operation order is the contract between this kernel and the oracle (oracle_tex2d).
__device__ __forceinline__ float4 tex2d(const Tex t, float u, float v)
{
    const float xb = u * (float)t.w - 0.5f, yb = v * (float)t.h - 0.5f;
    const float fx = floorf(xb), fy = floorf(yb);
    const float a = floorf((xb - fx) * 256.0f + 0.5f) * (1.0f / 256.0f), b = floorf((yb - fy) * 256.0f + 0.5f) * (1.0f / 256.0f);
    // wrap: floored modulo of the integer texel index (|u|, |v| stay far below 2^24 / N)
    const int w = (int)t.w, h = (int)t.h;
    int i0 = (int)fx % w, j0 = (int)fy % h;
    i0 += i0 < 0 ? w : 0;
    j0 += j0 < 0 ? h : 0;
    const int i1 = i0 + 1 == w ? 0 : i0 + 1, j1 = j0 + 1 == h ? 0 : j0 + 1;
    const uchar4 t00 = t.px[(size_t)j0 * t.w + i0], t10 = t.px[(size_t)j0 * t.w + i1], t01 = t.px[(size_t)j1 * t.w + i0], t11 = t.px[(size_t)j1 * t.w + i1];
    const float k = 1.0f / 255.0f;
    const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    auto mix = [&](unsigned char c00, unsigned char c10, unsigned char c01, unsigned char c11) {
        return w00 * ((float)c00 * k) + w10 * ((float)c10 * k) + w01 * ((float)c01 * k) + w11 * ((float)c11 * k);
    };
    return make_float4(mix(t00.x, t10.x, t01.x, t11.x), mix(t00.y, t10.y, t01.y, t11.y), mix(t00.z, t10.z, t01.z, t11.z), mix(t00.w, t10.w, t01.w, t11.w));
}

// ---- the walk over the LDS-resident compact form (kAllInLds) -------------------------------------------------------------
// slab test of a quantised box: world plane = grid_lo + cell * step, so t = fma(cell, step / d, (grid_lo - o) / d) -- one FMA per
// plane on two per-ray constants.  The build rounds lower planes down and upper planes up by one extra cell (3e-5 of the scene), which
// swallows the rounding of these products: the boxes only grow.
__device__ __forceinline__ bool qbox_hit(const uint4 q, v3 sid, v3 snoid, float tmin, float tmax, float& tn)
{
    float t0 = fmaf((float)(q.x & 0xFFFFu), sid.x, snoid.x), t1 = fmaf((float)(q.x >> 16), sid.x, snoid.x);
    float a = fminf(t0, t1), b = fmaxf(t0, t1);
    t0 = fmaf((float)(q.y & 0xFFFFu), sid.y, snoid.y);
    t1 = fmaf((float)(q.y >> 16), sid.y, snoid.y);
    a = fmaxf(a, fminf(t0, t1));
    b = fminf(b, fmaxf(t0, t1));
    t0 = fmaf((float)(q.z & 0xFFFFu), sid.z, snoid.z);
    t1 = fmaf((float)(q.z >> 16), sid.z, snoid.z);
    a = fmaxf(a, fminf(t0, t1));
    b = fminf(b, fmaxf(t0, t1));
    a = fmaxf(a, tmin);
    b = fminf(b, tmax);
    tn = a;
    return a <= b * 1.000002f + 1e-7f;
}

template <bool ANY>
__device__ __forceinline__ bool leaf_tris_lds(const float4* __restrict__ s_verts, const uint2* __restrict__ s_tidx, int first, int cnt, v3 o, v3 d, float tmin,
                                              float tmax, int& best, int& best_pos, float& bt, float& bu, float& bv)
{
    uint2 ti[kLeafTris];
#pragma unroll
    for (int k = 0; k < kLeafTris; ++k) ti[k] = s_tidx[first + (k < cnt ? k : 0)];
    float4 a[kLeafTris], b[kLeafTris], c[kLeafTris];
#pragma unroll
    for (int k = 0; k < kLeafTris; ++k) {
        a[k] = s_verts[ti[k].x & 0xFFFFu];
        b[k] = s_verts[ti[k].x >> 16];
        c[k] = s_verts[ti[k].y & 0xFFFFu];
    }
#pragma unroll
    for (int k = 0; k < kLeafTris; ++k) {
        if (k < cnt) {
            const int tri = (int)(ti[k].y >> 16);
            float t, u, v;
            if (tri_intersect(mk(a[k].x, a[k].y, a[k].z), mk(b[k].x, b[k].y, b[k].z), mk(c[k].x, c[k].y, c[k].z), o, d, tmin, tmax, t, u, v) &&
                (t < bt || (t == bt && best >= 0 && tri < best))) {
                bt = t;
                bu = u;
                bv = v;
                best = tri;
                best_pos = first + k;
                if (ANY) return true;
            }
        }
    }
    return false;
}

template <bool ANY>
__device__ __forceinline__ bool trace_lds(const Params& p, const uint4* __restrict__ s_q, const float4* __restrict__ s_verts, const uint2* __restrict__ s_tidx,
                                          unsigned short* __restrict__ s_stack, int stride, v3 o, v3 d, float tmin, float tmax, int& tri_out, int& pos_out,
                                          float& t_out, float& u_out, float& v_out)
{
    const v3 id = safe_inv(d);
    const v3 sid = mk(p.grid_step.x * id.x, p.grid_step.y * id.y, p.grid_step.z * id.z);
    const v3 snoid = mk((p.grid_lo.x - o.x) * id.x, (p.grid_lo.y - o.y) * id.y, (p.grid_lo.z - o.z) * id.z);
    int best = -1, best_pos = 0;
    float bt = tmax, bu = 0.0f, bv = 0.0f;
    if (p.n_recs == 0) {
        leaf_tris_lds<ANY>(s_verts, s_tidx, 0, p.n_triangles, o, d, tmin, tmax, best, best_pos, bt, bu, bv);
    } else {
        // while-while: every lane first descends to its next leaf (or runs out of work), then the lanes that hold a leaf test it
        int sp = 0;
        int cur = 0;
        bool have = true;
        auto pop = [&]() {
            have = sp > 0;
            if (have) {
                --sp;
                const int e = (int)s_stack[sp * stride];
                cur = (e & 0x8000) ? -1 - (e & 0x7FFF) : e;
            }
        };
        while (have) {
            while (have && cur >= 0) {
                const uint4 L = s_q[2 * cur + 0], R = s_q[2 * cur + 1];
                float tl, tr;
                const bool hl = qbox_hit(L, sid, snoid, tmin, bt, tl);
                const bool hr = qbox_hit(R, sid, snoid, tmin, bt, tr);
                const int ll = (int)L.w, lr = (int)R.w;
                const bool go_r = hr && (!hl || tr < tl);
                if (hl && hr) {
                    const int far = go_r ? ll : lr;
                    s_stack[sp * stride] = (unsigned short)(far >= 0 ? far : (0x8000 | (-1 - far)));
                    ++sp;
                }
                if (hl || hr) cur = go_r ? lr : ll;
                else pop();
            }
            if (have) {
                const int code = -1 - cur;
                if (leaf_tris_lds<ANY>(s_verts, s_tidx, code & ((1 << kLeafShift) - 1), (code >> kLeafShift) + 1, o, d, tmin, tmax, best, best_pos, bt, bu, bv)) break;   // (true only when ANY)
                pop();
            }
        }
    }
    tri_out = best;
    pos_out = best_pos;
    t_out = bt;
    u_out = bu;
    v_out = bv;
    return best >= 0;
}

// ---- the pixel pipeline every render kernel runs: whitted.cu's programs around the kernel's own walk and hit geometry -------------

// __raygen__pinhole, whitted.cu:183-240: the primary ray's direction through pixel (x, y) of the full image (its origin is the eye)
__device__ __forceinline__ v3 raygen(const Frame& f, unsigned int x, unsigned int y, unsigned int subframe)
{
    unsigned int seed = tea4(y * f.width + x, subframe);
    float jx = 0.0f, jy = 0.0f;
    if (subframe != 0) {
        jx = rnd(seed) - 0.5f;   // x first (source order)
        jy = rnd(seed) - 0.5f;
    }
    const float dx = 2.0f * div_cr((float)x + jx, (float)f.width) - 1.0f;
    const float dy = 2.0f * div_cr((float)y + jy, (float)f.height) - 1.0f;
    return vnormalize(vadd(vadd(vscale(f.U, dx), vscale(f.V, dy)), f.W));
}

struct Rays {   // a lane's share of the counters
    unsigned int total = 0, occlusion = 0;
};

// What a kernel's hit step hands to shading: getLocalGeometry (LocalGeometry.h:55-141) up to the shading normal, which is N here
// before the normal map
struct HitGeom {
    v3 P, N;                // world space
    v3 P0, P1, P2;          // the corners in the space dp/du, dp/dv are taken in (world for one mesh, object for an instance: :118-134)
    float w0, bu, bv;       // barycentrics
    unsigned int i0, i1, i2;    // vertex indices (into texcoords)
    const float* texcoords; // 2 floats per vertex, or null (then UV = the barycentrics, :97-102)
    unsigned int material;
};

// __closesthit__radiance, whitted.cu:255-337, from the hit geometry on: material, textures, and the GGX light loop with one occlusion
// ray per light that faces the surface (occluded(o, d, tmin, tmax): the kernel's any-hit walk).  rd: the WORLD ray direction (:307).
template <typename Occluded>
__device__ __forceinline__ v3 shade(const Frame& f, const HitGeom& h, v3 rd, Occluded&& occluded, Rays& rays)
{
    v3 N = h.N;
    const Pbr m = f.materials[h.material];
    v3 base = mk(m.base_color[0], m.base_color[1], m.base_color[2]);
    float mr_y = 1.0f, mr_z = 1.0f;   // the (1,1,1,1) of an absent metallic-roughness texture, whitted.cu:271
    if (f.mat_tex) {
        const MatTex mt = f.mat_tex[h.material];
        if (mt.base_color.px || mt.metallic_roughness.px || mt.normal.px) {
            // getLocalGeometry's UV and dp/du, dp/dv (LocalGeometry.h:88-135); the texcoords are read here only, so that nothing of
            // them stays live across the light loop
            const float w0 = h.w0, bu = h.bu, bv = h.bv;
            float2 UV0 = make_float2(0.0f, 0.0f), UV1 = make_float2(0.0f, 1.0f), UV2 = make_float2(1.0f, 0.0f), UV = make_float2(bu, bv);
            if (h.texcoords) {
                const float* tc = h.texcoords;
                UV0 = make_float2(tc[2 * h.i0], tc[2 * h.i0 + 1]);
                UV1 = make_float2(tc[2 * h.i1], tc[2 * h.i1 + 1]);
                UV2 = make_float2(tc[2 * h.i2], tc[2 * h.i2 + 1]);
                UV = make_float2(w0 * UV0.x + bu * UV1.x + bv * UV2.x, w0 * UV0.y + bu * UV1.y + bv * UV2.y);
            }
            if (mt.base_color.px) {
                // base_color *= linearize( tex2D ), whitted.cu:78-85, 264-267
                const float4 tc = tex2d(mt.base_color, UV.x, UV.y);
                base = vmul(base, mk(powf(tc.x, 2.2f), powf(tc.y, 2.2f), powf(tc.z, 2.2f)));
            }
            if (mt.metallic_roughness.px) {
                const float4 tc = tex2d(mt.metallic_roughness, UV.x, UV.y);   // (occlusion, roughness, metallic), :272-276
                mr_y = tc.y;
                mr_z = tc.z;
            }
            if (mt.normal.px) {
                // whitted.cu:288-292 over LocalGeometry.h:118-134
                const float du1 = UV0.x - UV2.x, du2 = UV1.x - UV2.x, dv1 = UV0.y - UV2.y, dv2 = UV1.y - UV2.y;
                const v3 dp1 = vsub(h.P0, h.P2), dp2 = vsub(h.P1, h.P2);
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
    const float metallic = m.metallic * mr_z, roughness = m.roughness * mr_y;   // :269-276
    const float F0 = 0.04f;
    const v3 diff_color = vscale(vscale(base, 1.0f - F0), 1.0f - metallic);
    // lerp(a, b, t) = a + t * (b - a), vec_math.h:496-499
    const v3 spec_color = vadd(mk(F0, F0, F0), vscale(vsub(base, mk(F0, F0, F0)), metallic));
    const float alpha = roughness * roughness;
    v3 result = mk(0.0f, 0.0f, 0.0f);
    for (int l = 0; l < f.n_lights; ++l) {
        const PointLight L = f.lights[l];
        const v3 toL = vsub(mk(L.position[0], L.position[1], L.position[2]), h.P);
        const float Ldist = vlength(toL);
        const v3 Lv = vscale(toL, 1.0f / Ldist);   // float3 / float multiplies by the reciprocal (vec_math.h:479-483)
        const v3 Vv = vneg(vnormalize(rd));
        const v3 H = vnormalize(vadd(Lv, Vv));
        const float NdotL = vdot(N, Lv), NdotV = vdot(N, Vv), NdotH = vdot(N, H), VdotH = vdot(Vv, H);
        if (NdotL > 0.0f && NdotV > 0.0f) {
            rays.total += 1;
            rays.occlusion += 1;
            if (!occluded(h.P, Lv, 0.001f, Ldist - 0.001f)) {
                const v3 F = schlick(spec_color, VdotH);
                const float G = vis(NdotL, NdotV, alpha);
                const float D = ggx_normal(NdotH, alpha);
                const v3 one_minus_F = vsub(mk(1.0f, 1.0f, 1.0f), F);
                const v3 dd = vmul(one_minus_F, diff_color);
                const float ip = 1.0f / kPi;
                const v3 diff = vscale(dd, ip);   // float3 / float
                const v3 spec = vscale(vscale(F, G), D);
                const v3 lc = vscale(mk(L.color[0], L.color[1], L.color[2]), L.intensity);
                result = vadd(result, vmul(vscale(lc, NdotL), vadd(diff, spec)));
            }
        }
    }
    return result;
}

// whitted.cu:226-239: the running mean over subframes (one step of it: subframe > 0 folds `result` into the mean of the subframes
// before it), and make_color (:164-173, gamma 2.2) of it.  Both launch forms fold through running_mean, one subframe at a time in
// subframe order, so they round alike.
__device__ __forceinline__ v3 running_mean(v3 prev, v3 result, unsigned int subframe)
{
    const float a = 1.0f / (float)(subframe + 1);
    return vadd(prev, vscale(vsub(result, prev), a));
}
__device__ __forceinline__ uchar4 make_color(v3 acc)
{
    const float g = (float)(1.0 / 2.2f);
    return make_uchar4((unsigned char)(powf(clampf(acc.x, 0.0f, 1.0f), g) * 255.0f), (unsigned char)(powf(clampf(acc.y, 0.0f, 1.0f), g) * 255.0f),
                       (unsigned char)(powf(clampf(acc.z, 0.0f, 1.0f), g) * 255.0f), 255u);
}
__device__ __forceinline__ void accumulate(const Frame& f, unsigned int idx, v3 result)
{
    v3 acc = result;
    if (f.subframe > 0) {
        const float4 prev = f.accum[idx];
        acc = running_mean(mk(prev.x, prev.y, prev.z), acc, f.subframe);
    }
    f.accum[idx] = make_float4(acc.x, acc.y, acc.z, 1.0f);
    f.image[idx] = make_color(acc);
}

// One tile of a FRAMES launch (rtgo_whitted_launch_frames): S = 1 << lanes_log2 lanes per pixel, so the wave's tile is 64 / S pixels
// (8 x 8, 8 x 4, 4 x 4, 4 x 2 for S = 1, 2, 4, 8).  Lane p S + j renders subframe first + j of pixel p with the pixel() body of the single
// launch; lane p S then reads the S radiances from its neighbours and folds them in subframe order through running_mean: the operations
// of S launches on that pixel, in their order.  More subframes than S are further chunks of the tile; between chunks the mean rests in the
// accumulation buffer, which the folding lane alone writes and reads back (nothing of it is held across pixel(): the walks leave no
// register for that).  Lanes of subframes past the last one trace nothing and count no ray.  The 8-bit image is written once.
template <typename Pixel>
__device__ __forceinline__ void render_tile_subframes(const Frame& f, unsigned int tile, Pixel&& pixel, Rays& rays)
{
    const unsigned int ls = f.lanes_log2, S = 1u << ls;
    // the lane's pixel in the compact local image.  Derived again from the tile and the lane on either side of pixel() (opaque_lane,
    // rtgo_device.h): held across it, these would be the registers the walks do not have
    auto place = [&](unsigned int lane, unsigned int& lx, unsigned int& ly) -> bool {
        unsigned int t = tile;
        asm volatile("" : "+s"(t));
        const unsigned int tw = 3u - (ls >> 1), th = 3u - ((ls + 1u) >> 1);   // log2 of the tile's width and height
        const unsigned int ty = t / f.tiles_x, tx = t - ty * f.tiles_x;
        const unsigned int pix = lane >> ls;
        lx = (tx << tw) + (pix & ((1u << tw) - 1u));
        ly = (ty << th) + (pix >> tw);
        return lx < f.share.lw && ly < f.share.lh;
    };
    for (unsigned int c = 0;; c += S) {
        const unsigned int left = f.n_subframes - c;   // subframes from this chunk on (>= 1)
        v3 r = mk(0.0f, 0.0f, 0.0f);
        {
            const unsigned int lane = opaque_lane(), j = lane & (S - 1u);
            unsigned int lx, ly;
            if (place(lane, lx, ly) && j < left) r = pixel(f.share.x0 + lx, share_row(f.share, ly), f.subframe + c + j, rays);
        }
        const unsigned int lane = opaque_lane();
        unsigned int lx, ly;
        const bool fold = place(lane, lx, ly) && (lane & (S - 1u)) == 0u;
        const unsigned int idx = ly * f.share.lw + lx;
        const unsigned int first = f.subframe + c;   // the chunk's first subframe
        v3 acc = mk(0.0f, 0.0f, 0.0f);
        if (fold && first > 0u) {
            const float4 prev = f.accum[idx];
            acc = mk(prev.x, prev.y, prev.z);
        }
        for (unsigned int q = 0; q < S; ++q) {   // (every lane takes part in the cross-lane reads)
            const int src = (int)((lane & ~(S - 1u)) + q);
            const v3 rq = mk(__shfl(r.x, src), __shfl(r.y, src), __shfl(r.z, src));
            if (q < left) acc = first + q == 0u ? rq : running_mean(acc, rq, first + q);
        }
        if (fold) {
            f.accum[idx] = make_float4(acc.x, acc.y, acc.z, 1.0f);
            if (left <= S) f.image[idx] = make_color(acc);
        }
        if (left <= S) break;
    }
}

// The body of every render kernel: preload() (the kernel's LDS image of its structure, ending in a barrier), then the wave's tiles
// from the queue, pixel(x, y, subframe, rays) -> radiance for each pixel of the launch's share (x, y: in the full image), accumulated,
// and the wave's ray counts added to the counters.  FRAMES: the launch renders Frame::n_subframes subframes of every pixel
// (render_tile_subframes); queue, stacks and counters are the single launch's.
//
// Tile queue: kTileHeads counters 64 bytes apart, head h serves the tiles h, h + kTileHeads, ...  (one counter hands out ~88 entries per
// microsecond chip-wide: a 1080p subframe is 32 k tiles).  A wave starts on head blockIdx % kTileHeads; when that is dry it looks at all
// heads with one load and moves to an open one.  The pull for the next tile is in flight while the current one is rendered.
template <bool FRAMES, typename Preload, typename Pixel>
__device__ __forceinline__ void render_tiles(const Frame& f, Preload&& preload, Pixel&& pixel)
{
    WhittedTiming timing;   // (diagnostic build's probe, rtgo_probes.h: an empty type in the product build)
    timing.wave_start();
    preload();
    if (blockIdx.x == 0 && threadIdx.x < (unsigned int)kTileHeads) f.tile_counter_next[kTileHeadStride * threadIdx.x] = 0u;
    const unsigned int lane = threadIdx.x & 63u;
    const unsigned int n_tiles = f.tiles_x * f.tiles_y;
    Rays rays;
    auto tiles_of = [&](unsigned int h) { return (n_tiles + (unsigned int)kTileHeads - 1u - h) / (unsigned int)kTileHeads; };
    unsigned int head = blockIdx.x % (unsigned int)kTileHeads;
    unsigned int pending = 0u;
    if (lane == 0u) pending = atomicAdd(f.tile_counter + kTileHeadStride * head, 1u);
    for (;;) {
        unsigned int pos = (unsigned int)__builtin_amdgcn_readfirstlane((int)pending);
        if (pos >= tiles_of(head)) {
            // this head is dry: any other one still open?
            unsigned int v = 0xFFFFFFFFu;
            if (lane < (unsigned int)kTileHeads) v = __hip_atomic_load(f.tile_counter + kTileHeadStride * lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long open = __builtin_amdgcn_ballot_w64(lane < (unsigned int)kTileHeads && v < tiles_of(lane));
            if (open == 0ull) break;
            // the first open head after this one (waves spread over the open heads instead of all falling on the lowest)
            const unsigned long long above = open & ~((2ull << head) - 1ull);
            head = (unsigned int)(__ffsll((long long)(above ? above : open)) - 1);
            if (lane == 0u) pending = atomicAdd(f.tile_counter + kTileHeadStride * head, 1u);
            continue;
        }
        // queue entry -> tile through a fixed permutation (multiplication by a number coprime to the tile count, near the golden
        // section of it): in row-major order every wave of the chip reaches the dense part of the mesh at the same time and they all
        // queue at the vector memory pipeline for its triangles; scattered, tiles that wait for triangles overlap tiles that do not
        const unsigned int tile = (unsigned int)(((unsigned long long)(pos * (unsigned int)kTileHeads + head) * f.tile_stride) % n_tiles);
        if (lane == 0u) pending = atomicAdd(f.tile_counter + kTileHeadStride * head, 1u);
        if constexpr (FRAMES) {
            render_tile_subframes(f, tile, pixel, rays);   // (the timing probe stays on the single launch)
        } else {
            timing.tile_begin();
            const unsigned int ty = tile / f.tiles_x, tx = tile - ty * f.tiles_x;
            const unsigned int lx = tx * 8u + (lane & 7u), ly = ty * 8u + (lane >> 3);   // in the compact local image
            if (lx < f.share.lw && ly < f.share.lh) accumulate(f, ly * f.share.lw + lx, pixel(f.share.x0 + lx, share_row(f.share, ly), f.subframe, rays));
            timing.tile_end(f, lx < f.share.lw && ly < f.share.lh, ly * f.share.lw + lx, rays.total);
        }
    }
    const unsigned int total = wave_sum(rays.total), occlusion = wave_sum(rays.occlusion);
    if (lane == 0u) {
        atomicAdd(&f.counters[0], (unsigned long long)total);
        atomicAdd(&f.counters[1], (unsigned long long)occlusion);
        timing.flush(f);
    }
}

// __closesthit__radiance at a hit of a mesh in world space, from the walk's answer: triangle `tri` at position tpos of the Morton order,
// barycentrics (bu, bv) -- the hit geometry, then shade().  MODE: where the render kernel keeps the structure (kAllInLds: corners and indices
// from its LDS image, s_verts / s_tidx; otherwise through L2, and the LDS pointers are not read).  render_kernel and whitted_shade_kernel
// (rtgo_whitted_shade.h) both call it, so the arithmetic cannot drift.  (Geometry and shading are ONE function on purpose: with the
// geometry alone behind a call the compiler forms the normal loads' offsets right after the index load and waits for it there.)
template <int MODE, typename Occluded>
__device__ __forceinline__ v3 mesh_shade_hit(const Params& p, const float4* s_verts, const uint2* s_tidx, int tri, int tpos, float bu, float bv, v3 rd,
                                             Occluded&& occluded, Rays& rays)
{
    // (The corners come from the Morton-ordered copy the walk read them from: same values, no trip through the index array.)
    float4 c0, c1, c2;
    HitGeom h;
    h.i0 = h.i1 = h.i2 = 0;
    if constexpr (MODE == kAllInLds) {
        const uint2 ti = s_tidx[tpos];
        h.i0 = ti.x & 0xFFFFu;
        h.i1 = ti.x >> 16;
        h.i2 = ti.y & 0xFFFFu;
        c0 = s_verts[h.i0];
        c1 = s_verts[h.i1];
        c2 = s_verts[h.i2];
    } else {
        c0 = p.tris[3 * tpos + 0];
        c1 = p.tris[3 * tpos + 1];
        c2 = p.tris[3 * tpos + 2];
        if (p.normals || p.texcoords) {
            h.i0 = p.indices[3 * tri + 0];
            h.i1 = p.indices[3 * tri + 1];
            h.i2 = p.indices[3 * tri + 2];
        }
    }
    h.P0 = mk(c0.x, c0.y, c0.z);
    h.P1 = mk(c1.x, c1.y, c1.z);
    h.P2 = mk(c2.x, c2.y, c2.z);
    h.w0 = 1.0f - bu - bv;
    h.bu = bu;
    h.bv = bv;
    h.P = vadd(vadd(vscale(h.P0, h.w0), vscale(h.P1, bu)), vscale(h.P2, bv));
    h.N = vnormalize(vcross(vsub(h.P1, h.P0), vsub(h.P2, h.P0)));   // Ng
    if (p.normals) {
        const v3 N0 = ld3(p.normals, h.i0), N1 = ld3(p.normals, h.i1), N2 = ld3(p.normals, h.i2);
        h.N = vnormalize(vadd(vadd(vscale(N0, h.w0), vscale(N1, bu)), vscale(N2, bv)));
    }
    h.texcoords = p.texcoords;
    h.material = p.tri_material ? p.tri_material[tri] : 0u;
    return shade(p.frame, h, rd, occluded, rays);
}

// One mesh in world space.  MODE: where the walk reads its structure from (kAllInL2 / kRecordsInLds / kAllInLds);  FRAMES: render_tiles'
template <int MODE, bool FRAMES = false>
__global__ __launch_bounds__(kRenderBlock) void render_kernel(const Params p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char w_smem[];
    // LDS image.  kRecordsInLds: [fp32 records, 64 B each][stacks];  kAllInLds: [quantised records, 32 B][vertices, 16 B][triangle
    // indices, 8 B][stacks];  kAllInL2: [stacks]
    float4* s_recs = reinterpret_cast<float4*>(w_smem);
    uint4* s_q = reinterpret_cast<uint4*>(w_smem);
    float4* s_verts = reinterpret_cast<float4*>(s_q + 2 * p.n_recs);
    uint2* s_tidx = reinterpret_cast<uint2*>(s_verts + p.n_vertices);
    const int stride = (int)blockDim.x;
    unsigned short* s_stack = (MODE == kAllInLds ? reinterpret_cast<unsigned short*>(s_tidx + p.n_triangles)
                                                 : reinterpret_cast<unsigned short*>(s_recs + (MODE == kRecordsInLds ? 4 * p.n_recs : 0))) + threadIdx.x;   // entry e at [e * stride]
    auto preload = [&]() {
        if (MODE == kRecordsInLds) {
            for (int i = (int)threadIdx.x; i < 4 * p.n_recs; i += stride) s_recs[i] = p.recs[i];
            __syncthreads();
        }
        if (MODE == kAllInLds) {
            for (int i = (int)threadIdx.x; i < 2 * p.n_recs; i += stride) s_q[i] = p.qrecs[i];
            for (int i = (int)threadIdx.x; i < p.n_vertices; i += stride) s_verts[i] = make_float4(p.positions[3 * i + 0], p.positions[3 * i + 1], p.positions[3 * i + 2], 0.0f);
            for (int i = (int)threadIdx.x; i < p.n_triangles; i += stride) s_tidx[i] = p.tidx[i];
            __syncthreads();
        }
    };
    const float4* recs = MODE == kRecordsInLds ? static_cast<const float4*>(s_recs) : p.recs;
    auto occluded = [&](v3 o, v3 d, float t0, float t1) -> bool {
        int tri, pos;
        float t, u, v;
        if constexpr (MODE == kAllInLds) return trace_lds<true>(p, s_q, s_verts, s_tidx, s_stack, stride, o, d, t0, t1, tri, pos, t, u, v);
        else return trace<true>(p, recs, s_stack, stride, o, d, t0, t1, tri, pos, t, u, v);
    };
    render_tiles<FRAMES>(p.frame, preload, [&](unsigned int x, unsigned int y, unsigned int subframe, Rays& rays) -> v3 {
        const v3 rd = raygen(p.frame, x, y, subframe);
        const v3 miss = p.frame.miss;   // __miss__constant_radiance, :243-246 (read ahead of the walk: after it, kAllInLds spills)
        int tri, tpos;
        float t, bu, bv;
        rays.total += 1;
        bool hit;
        if constexpr (MODE == kAllInLds) hit = trace_lds<false>(p, s_q, s_verts, s_tidx, s_stack, stride, p.frame.eye, rd, 0.01f, 1e16f, tri, tpos, t, bu, bv);
        else hit = trace<false>(p, recs, s_stack, stride, p.frame.eye, rd, 0.01f, 1e16f, tri, tpos, t, bu, bv);
        if (!hit) return miss;
        return mesh_shade_hit<MODE>(p, s_verts, s_tidx, tri, tpos, bu, bv, rd, occluded, rays);
    });
}

// What the two build kernels report (build_kernel writes all of it, sah_kernel rewrites n_recs and walk_depth)
struct WhittedBuildMeta {
    int depth;              // of the Morton hierarchy
    int n_recs;             // records of the walk; 0: the structure is one leaf
    int walk_depth;         // stack entries the walk needs
    v3 grid_lo, grid_step;  // the grid of the compact records
};
static_assert(sizeof(WhittedBuildMeta) == 9 * sizeof(int), "nine words");

// One record of the walk, r: BOTH children's boxes (a* / b*: lower and upper corner, .w unused) and links, so that a step of the walk reads
// 64 contiguous bytes -> recs[4 r ..]; and the same record on the 16-bit grid over the padded scene box (lower planes one cell below
// their floor, upper planes one above their ceiling) -> qrecs[2 r ..]
__device__ __forceinline__ void write_walk_record(float4* __restrict__ recs, uint4* __restrict__ qrecs, int r, const float4 a0, const float4 a1, int link_a,
                                                  const float4 b0, const float4 b1, int link_b, const float glo[3], const float gstep[3])
{
    recs[4 * r + 0] = make_float4(a0.x, a0.y, a0.z, __int_as_float(link_a));
    recs[4 * r + 1] = make_float4(a1.x, a1.y, a1.z, 0.0f);
    recs[4 * r + 2] = make_float4(b0.x, b0.y, b0.z, __int_as_float(link_b));
    recs[4 * r + 3] = make_float4(b1.x, b1.y, b1.z, 0.0f);
    auto cell = [&](float v, int a, bool up) -> unsigned int {
        const float c = (v - glo[a]) / gstep[a];
        const float q = up ? ceilf(c) + 1.0f : floorf(c) - 1.0f;
        return (unsigned int)fminf(fmaxf(q, 0.0f), 65535.0f);
    };
    qrecs[2 * r + 0] = make_uint4(cell(a0.x, 0, false) | (cell(a1.x, 0, true) << 16), cell(a0.y, 1, false) | (cell(a1.y, 1, true) << 16),
                                  cell(a0.z, 2, false) | (cell(a1.z, 2, true) << 16), (unsigned int)link_a);
    qrecs[2 * r + 1] = make_uint4(cell(b0.x, 0, false) | (cell(b1.x, 0, true) << 16), cell(b0.y, 1, false) | (cell(b1.y, 1, true) << 16),
                                  cell(b0.z, 2, false) | (cell(b1.z, 2, true) << 16), (unsigned int)link_b);
}

// ---------------------------------------------------------------------------------------------------------------------
// The pad of every box the builds write: 1e-4 of the scene's extent + 1e-6, and at least two floats at the bounds' largest coordinate
// (`reach`).  Far from the origin -- vertex data at 1e4, where one float is 1e-3 -- the first alone rounds away, lo - pad == lo, and a
// box face lies ON the vertices it bounds: a ray in that face plane (a zero direction component, an origin coordinate equal to the
// plane's) then has a slab interval that ends at -0 or starts at +0 and is cut off from a triangle it meets.  With 2^-22 reach every
// coordinate c of the scene has c - pad < c and c + pad > c.  Wherever reach is below ~420 extents this is the first term, bit for bit.
__host__ __device__ inline float box_pad(float maxext, float reach) { return fmaxf(maxext * 1e-4f + 1e-6f, reach * 2.3841858e-7f); }

// LBVH over the triangles, one workgroup: replaces optixAccelBuild over OPTIX_BUILD_INPUT_TYPE_TRIANGLES (sutil/Scene.cpp,
// buildMeshAccels).  Same recipe as the analytic path's canonical tree, with rtgo_build.h's functions: 30-bit Morton code of the
// centroid normalised to the scene bounds, stable order by (code, triangle index), Karras 2012, one triangle per leaf, bottom-up fit.
// Boxes are padded by box_pad (1e-4 of the scene's extent + 1e-6, or two floats at its largest coordinate): the slab test rounds, the
// triangle test must never be cut off.
// ---------------------------------------------------------------------------------------------------------------------
// The work arrays of one build of n triangles (host side: whitted_build), carved out of build_scratch_ints(n) ints: parent [2n - 1], visit,
// first, count, record [n each], 16 words for the meta, sah_kernel's 32 n
constexpr size_t build_scratch_ints(size_t n) { return 38 * n + 16; }
struct BuildScratch {
    int *parent, *visit, *first_of, *count_of, *rec_of, *sah;
    WhittedBuildMeta* meta;
    __host__ __device__ BuildScratch(int* ints, int n)
        : parent(ints), visit(parent + (2 * n - 1)), first_of(visit + n), count_of(first_of + n), rec_of(count_of + n), sah(rec_of + n + 16),
          meta(reinterpret_cast<WhittedBuildMeta*>(rec_of + n))
    {
    }
};

// What one build works on: the vertices and the n index triples of its triangles, its work arrays (BuildScratch's, and the Morton
// hierarchy's nodes [(2n - 1) x 2]), and where its structure goes.  The body is build_structure, one workgroup over one BuildJob:
// build_kernel runs it over one structure, big_build_batch_kernel (rtgo_whitted_big.h) with one workgroup per structure of a table.
struct BuildJob {
    const float* positions;
    const unsigned int* indices;
    int n;
    float4* nodes;
    int *parent, *visit, *first_of, *count_of, *rec_of;
    float4 *recs, *tris;
    uint4* qrecs;
    uint2* tidx;
    WhittedBuildMeta* out_meta;
};

// One workgroup of kBuildThreads threads; s_keys: its kMaxTriangles x 8 B of (dynamic) LDS.  (The job's arrays do not overlap: the body
// takes them as __restrict__ parameters, as build_kernel always declared them.)
__device__ __forceinline__ void build_structure_body(const float* __restrict__ positions, const unsigned int* __restrict__ indices, int n,
                                                     float4* __restrict__ nodes, int* __restrict__ parent, int* __restrict__ visit, int* __restrict__ first_of,
                                                     int* __restrict__ count_of, int* __restrict__ rec_of, float4* __restrict__ recs, float4* __restrict__ tris,
                                                     uint4* __restrict__ qrecs, uint2* __restrict__ tidx, WhittedBuildMeta* __restrict__ out_meta,
                                                     unsigned long long* s_keys)
{
    __shared__ float s_red[6][kBuildThreads];
    __shared__ int s_depth, s_nrec, s_wdepth;
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_depth = 0;
        s_nrec = 0;
        s_wdepth = 0;
    }
    // scene bounds
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < n; i += kBuildThreads)
        for (int k = 0; k < 3; ++k) {
            const unsigned int vi = indices[3 * i + k];
            for (int a = 0; a < 3; ++a) {
                const float c = positions[3 * vi + a];
                lo[a] = fminf(lo[a], c);
                hi[a] = fmaxf(hi[a], c);
            }
        }
    reduce_bounds<kBuildThreads>(s_red, tid, lo, hi);
    float blo[3], ext[3], maxext = 0.0f, reach = 0.0f;
    for (int a = 0; a < 3; ++a) {
        blo[a] = s_red[a][0];
        ext[a] = s_red[3 + a][0] - s_red[a][0];
        maxext = fmaxf(maxext, ext[a]);
        reach = fmaxf(reach, fmaxf(fabsf(s_red[a][0]), fabsf(s_red[3 + a][0])));
    }
    const float pad = box_pad(maxext, reach);
    // Morton keys, sorted (unique: the index is part of the key)
    for (int i = tid; i < kMaxTriangles; i += kBuildThreads) s_keys[i] = i < n ? triangle_key(positions, indices, i, blo, ext) : ~0ull;
    bitonic_sort<kMaxTriangles, kBuildThreads>(s_keys, tid);
    const int leaf0 = n - 1;
    // leaves
    for (int i = tid; i < n; i += kBuildThreads) {
        const int tri = (int)(s_keys[i] & 0xFFFFFFFFu);
        float l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) {
                const float c = positions[3 * indices[3 * tri + k] + a];
                l[a] = fminf(l[a], c);
                h[a] = fmaxf(h[a], c);
            }
        nodes[2 * (leaf0 + i) + 0] = make_float4(l[0] - pad, l[1] - pad, l[2] - pad, __int_as_float(tri));
        nodes[2 * (leaf0 + i) + 1] = make_float4(h[0] + pad, h[1] + pad, h[2] + pad, __int_as_float(-1));
    }
    for (int i = tid; i < 2 * n - 1; i += kBuildThreads) parent[i] = -1;
    __syncthreads();
    // Karras 2012
    for (int i = tid; i < n - 1; i += kBuildThreads) {
        int left, right, lo_i, hi_i;
        karras_node(s_keys, n, i, left, right, lo_i, hi_i);
        nodes[2 * i + 0].w = __int_as_float(left);
        nodes[2 * i + 1].w = __int_as_float(right);
        parent[left] = i;
        parent[right] = i;
        first_of[i] = lo_i;               // the node's triangles: sorted positions [lo_i, hi_i]
        count_of[i] = hi_i - lo_i + 1;
    }
    __syncthreads();
    // bottom-up fit, level by level: a node is fitted in the pass after both of its children (visit[] = 1 once a node is done;
    // leaves are done from the start).  A workgroup barrier orders the passes, global memory included.
    for (int i = tid; i < n; i += kBuildThreads) visit[i] = 0;   // (per internal node)
    __syncthreads();
    for (int pass = 0; pass < 2 * kStack + 2; ++pass) {
        int fitted[kMaxTriangles / kBuildThreads], nf = 0;   // nodes this thread fits in this pass
        for (int i = tid; i < n - 1; i += kBuildThreads) {
            if (visit[i]) continue;
            const int L = __float_as_int(nodes[2 * i + 0].w), R = __float_as_int(nodes[2 * i + 1].w);
            const bool ldone = L >= leaf0 || visit[L] == 1, rdone = R >= leaf0 || visit[R] == 1;
            if (ldone && rdone) {
                const float4 a0 = nodes[2 * L], a1 = nodes[2 * L + 1], b0 = nodes[2 * R], b1 = nodes[2 * R + 1];
                nodes[2 * i + 0] = make_float4(fminf(a0.x, b0.x), fminf(a0.y, b0.y), fminf(a0.z, b0.z), __int_as_float(L));
                nodes[2 * i + 1] = make_float4(fmaxf(a1.x, b1.x), fmaxf(a1.y, b1.y), fmaxf(a1.z, b1.z), __int_as_float(R));
                fitted[nf++] = i;   // marked after the barrier: a node fitted in THIS pass must not feed its parent before it
            }
        }
        __syncthreads();
        for (int k = 0; k < nf; ++k) visit[fitted[k]] = 1;
        __syncthreads();
        if (n < 2 || visit[0] == 1) break;   // the root is done (uniform: every thread reads the same word after the barrier)
    }
    for (int i = tid; i < n; i += kBuildThreads) {
        int dd = 0;
        for (int q = n > 1 ? parent[leaf0 + i] : -1; q >= 0; q = parent[q]) ++dd;
        atomicMax(&s_depth, dd);
    }
    __syncthreads();
    // ---- the structure the render kernel walks --------------------------------------------------------------------
    // Subtrees of at most kLeafTris triangles become leaves (their triangles are neighbours in Morton order); every node above
    // them gets one record with BOTH children's boxes, so that a step of the walk reads 64 contiguous bytes.
    // Records are numbered in node order, by a prefix sum over the nodes that get one (the root's is record 0): the same numbers whichever
    // kernel runs this body and however its waves are scheduled -- a counter handed out by atomicAdd numbers them in arrival order, and
    // then two builds of the same mesh need not write the same arrays.
    {
        constexpr int kPer = kMaxTriangles / kBuildThreads;    // a thread numbers kPer consecutive nodes
        int* s_cnt = reinterpret_cast<int*>(&s_red[0][0]);     // [kBuildThreads] (the bounds were read out of s_red long ago)
        int mine = 0;
        for (int k = 0; k < kPer; ++k) {
            const int i = tid * kPer + k;
            if (i < n - 1 && count_of[i] > kLeafTris) ++mine;
        }
        s_cnt[tid] = mine;
        __syncthreads();
        for (int d = 1; d < kBuildThreads; d <<= 1) {
            const int below = tid >= d ? s_cnt[tid - d] : 0;
            __syncthreads();
            s_cnt[tid] += below;
            __syncthreads();
        }
        int r = s_cnt[tid] - mine;
        for (int k = 0; k < kPer; ++k) {
            const int i = tid * kPer + k;
            if (i < n - 1) rec_of[i] = count_of[i] > kLeafTris ? r++ : -1;
        }
        if (tid == kBuildThreads - 1) s_nrec = s_cnt[tid];
    }
    __syncthreads();
    // grid of the compact form: cells 1 .. 65534 span the padded scene box
    float glo[3], gstep[3];
    for (int a = 0; a < 3; ++a) {
        glo[a] = blo[a] - pad;
        gstep[a] = (ext[a] + 2.0f * pad) * (1.0f / 65533.0f);
    }
    auto link_of = [&](int child) -> int {
        if (child >= leaf0) return -1 - (child - leaf0);                                         // one triangle
        if (count_of[child] <= kLeafTris) return -1 - (first_of[child] | ((count_of[child] - 1) << kLeafShift));
        return rec_of[child];
    };
    for (int i = tid; i < n - 1; i += kBuildThreads) {
        const int r = rec_of[i];
        if (r < 0) continue;
        const int L = __float_as_int(nodes[2 * i + 0].w), R = __float_as_int(nodes[2 * i + 1].w);
        const float4 a0 = nodes[2 * L], a1 = nodes[2 * L + 1], b0 = nodes[2 * R], b1 = nodes[2 * R + 1];
        write_walk_record(recs, qrecs, r, a0, a1, link_of(L), b0, b1, link_of(R), glo, gstep);
        int dd = 1;   // stack entries a walk can hold below this record: one per record on the way down, its own included
        for (int q = parent[i]; q >= 0; q = parent[q]) ++dd;
        atomicMax(&s_wdepth, dd);
    }
    for (int i = tid; i < n; i += kBuildThreads) {
        const unsigned int tri = (unsigned int)(s_keys[i] & 0xFFFFFFFFu);
        const unsigned int i0 = indices[3 * tri + 0], i1 = indices[3 * tri + 1], i2 = indices[3 * tri + 2];
        tris[3 * i + 0] = make_float4(positions[3 * i0 + 0], positions[3 * i0 + 1], positions[3 * i0 + 2], __int_as_float((int)tri));
        tris[3 * i + 1] = make_float4(positions[3 * i1 + 0], positions[3 * i1 + 1], positions[3 * i1 + 2], 0.0f);
        tris[3 * i + 2] = make_float4(positions[3 * i2 + 0], positions[3 * i2 + 1], positions[3 * i2 + 2], 0.0f);
        tidx[i] = make_uint2((i0 & 0xFFFFu) | (i1 << 16), (i2 & 0xFFFFu) | (tri << 16));   // (used only when every vertex index fits 16 bits)
    }
    __syncthreads();
    if (tid == 0) {
        out_meta->depth = s_depth;
        out_meta->n_recs = n > kLeafTris ? s_nrec : 0;   // 0: the mesh is one leaf, no records
        out_meta->walk_depth = s_wdepth;
        out_meta->grid_lo = mk(glo[0], glo[1], glo[2]);
        out_meta->grid_step = mk(gstep[0], gstep[1], gstep[2]);
    }
}

__device__ __forceinline__ void build_structure(const BuildJob& j, unsigned long long* s_keys)
{
    build_structure_body(j.positions, j.indices, j.n, j.nodes, j.parent, j.visit, j.first_of, j.count_of, j.rec_of, j.recs, j.tris, j.qrecs, j.tidx, j.out_meta, s_keys);
}

__global__ __launch_bounds__(kBuildThreads) void build_kernel(const float* __restrict__ positions, const unsigned int* __restrict__ indices, int n,
                                                              float4* __restrict__ nodes, int* __restrict__ parent, int* __restrict__ visit,
                                                              int* __restrict__ first_of, int* __restrict__ count_of, int* __restrict__ rec_of,
                                                              float4* __restrict__ recs, float4* __restrict__ tris, uint4* __restrict__ qrecs,
                                                              uint2* __restrict__ tidx, WhittedBuildMeta* __restrict__ out_meta)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char build_keys_dyn[];   // kMaxTriangles x 8 B: the launch passes the size
    build_structure({positions, indices, n, nodes, parent, visit, first_of, count_of, rec_of, recs, tris, qrecs, tidx, out_meta},
                    reinterpret_cast<unsigned long long*>(build_keys_dyn));
}

// ---------------------------------------------------------------------------------------------------------------------
// The walk's records rebuilt over the same leaves with the surface-area heuristic (second session of round 2).  build_kernel's
// Morton hierarchy forms the leaves (subtrees of at most kLeafTris triangles: neighbours in Morton order, contiguous in `tris`);
// above them bit prefixes know nothing of box areas, and any tree over the same leaves returns the same hits, so the topology is
// rebuilt top-down by the analytic path's sah_build (rtgo_build.h) with T = triangles as the weights, ties to the median.
// What sets the whitted launch is one wave's serial walk over the finely tessellated part: fewer steps there.
// Overwrites recs / qrecs and out_meta's n_recs and walk_depth; scratch: 32 n ints.
// ---------------------------------------------------------------------------------------------------------------------
// What one surface-area pass works on: build_structure's hierarchy over n triangles (read), its 32 n ints of scratch, and the records and
// meta it rewrites.  The body is sah_structure, one workgroup over one SahJob: sah_kernel runs it over one structure,
// big_sah_batch_kernel (rtgo_whitted_big.h) with one workgroup per structure of a table.
struct SahJob {
    int n;
    const float4* nodes;
    const int *parent, *first_of, *count_of;
    int* scratch;
    float4* recs;
    uint4* qrecs;
    WhittedBuildMeta* out_meta;
};

// One workgroup of kBuildThreads threads; sah_dyn: its 33 n + 16 bytes of (dynamic) LDS
__device__ __forceinline__ void sah_structure_body(int n, const float4* __restrict__ nodes, const int* __restrict__ parent, const int* __restrict__ first_of,
                                                   const int* __restrict__ count_of, int* __restrict__ scratch, float4* __restrict__ recs,
                                                   uint4* __restrict__ qrecs, WhittedBuildMeta* __restrict__ out_meta, unsigned char* sah_dyn)
{
    if (n <= kLeafTris) return;   // the mesh is one leaf: no records
    float (*u_box)[6] = reinterpret_cast<float (*)[6]>(sah_dyn);      // [n] leaf boxes
    int* u_link = reinterpret_cast<int*>(u_box + n);                  // [n] the leaf's link in the walk's records
    short* perm = reinterpret_cast<short*>(u_link + n);               // [n] leaves in the current task order
    short* tmp = perm + n;                                            // [n]
    unsigned char* u_w = reinterpret_cast<unsigned char*>(tmp + n);   // [n] triangles of the leaf
    __shared__ int s_U, s_wdepth, s_nrec;
    __shared__ SahShared s_sah;
    // global scratch (one thread group, barriers order it)
    // tree: left [2n] first child / the leaf's link, right [2n] second child, -1: a leaf, parent [2n]; the task queue [2n] x 3; box [2n][6]
    const SahTree t = {reinterpret_cast<float*>(scratch + 12 * n), scratch, scratch + 2 * n, scratch + 4 * n};
    const SahQueue<int> tq = {scratch + 6 * n, scratch + 8 * n, scratch + 10 * n};
    int* start = reinterpret_cast<int*>(t.box + 12 * n);      // [n] node of the leaf that starts at a Morton position, -1: none
    int* rec_of = start + n;                                  // [2n]
    float* sfx = reinterpret_cast<float*>(rec_of + 2 * n);    // [n][2] suffix area and triangles of the sweep
    const int tid = threadIdx.x, leaf0 = n - 1;
    for (int pos = tid; pos < n; pos += kBuildThreads) start[pos] = -1;
    __syncthreads();
    for (int k = tid; k < 2 * n - 1; k += kBuildThreads) {
        const int cnt = k >= leaf0 ? 1 : count_of[k];
        const bool is_leaf = cnt <= kLeafTris && k != 0 && count_of[parent[k]] > kLeafTris;
        if (is_leaf) start[k >= leaf0 ? k - leaf0 : first_of[k]] = k;
    }
    __syncthreads();
    if (tid == 0) {
        int U = 0;
        for (int pos = 0; pos < n; ++pos)
            if (start[pos] >= 0) rec_of[U++] = start[pos];   // (rec_of borrowed: leaf u's node)
        s_U = U;
        s_wdepth = 0;
    }
    __syncthreads();
    const int U = s_U;
    for (int u = tid; u < U; u += kBuildThreads) {
        const int k = rec_of[u];
        const float4 b0 = nodes[2 * k], b1 = nodes[2 * k + 1];
        u_box[u][0] = b0.x; u_box[u][1] = b0.y; u_box[u][2] = b0.z;
        u_box[u][3] = b1.x; u_box[u][4] = b1.y; u_box[u][5] = b1.z;
        const int first = k >= leaf0 ? k - leaf0 : first_of[k], cnt = k >= leaf0 ? 1 : count_of[k];
        u_link[u] = -1 - (first | ((cnt - 1) << kLeafShift));
        u_w[u] = (unsigned char)cnt;
        perm[u] = (short)u;
    }
    const int n_nodes = sah_build<kBuildThreads, true>(
        tid, U, 2 * n, [&](int u, int c) { return u_box[u][c]; }, [&](int u) { return (int)u_w[u]; }, perm, tmp, sfx, tq, t, s_sah, [&](int node, int u) {
            t.left[node] = u_link[u];
            t.right[node] = -1;
        });
    if (tid == 0) {
        int r = 0;
        for (int k = 0; k < n_nodes; ++k) rec_of[k] = t.right[k] >= 0 ? r++ : -1;   // (the root is node 0 and record 0)
        s_nrec = r;
    }
    __syncthreads();
    const float glo[3] = {out_meta->grid_lo.x, out_meta->grid_lo.y, out_meta->grid_lo.z};
    const float gstep[3] = {out_meta->grid_step.x, out_meta->grid_step.y, out_meta->grid_step.z};
    for (int k = tid; k < n_nodes; k += kBuildThreads) {
        const int r = rec_of[k];
        if (r < 0) continue;
        const int L = t.left[k], R = t.right[k];
        const int linkL = t.right[L] >= 0 ? rec_of[L] : t.left[L], linkR = t.right[R] >= 0 ? rec_of[R] : t.left[R];
        const float* a = t.box + 6 * L;
        const float* b = t.box + 6 * R;
        write_walk_record(recs, qrecs, r, make_float4(a[0], a[1], a[2], 0.0f), make_float4(a[3], a[4], a[5], 0.0f), linkL, make_float4(b[0], b[1], b[2], 0.0f),
                          make_float4(b[3], b[4], b[5], 0.0f), linkR, glo, gstep);
        int dd = 1;   // stack entries a walk can hold below this record: one per record on the way down, its own included
        for (int q = t.parent[k]; q >= 0; q = t.parent[q]) ++dd;
        atomicMax(&s_wdepth, dd);
    }
    __syncthreads();
    if (tid == 0) {
        out_meta->n_recs = s_nrec;
        out_meta->walk_depth = s_wdepth;
    }
}

__device__ __forceinline__ void sah_structure(const SahJob& j, unsigned char* sah_dyn)
{
    sah_structure_body(j.n, j.nodes, j.parent, j.first_of, j.count_of, j.scratch, j.recs, j.qrecs, j.out_meta, sah_dyn);
}

__global__ __launch_bounds__(kBuildThreads) void sah_kernel(int n, const float4* __restrict__ nodes, const int* __restrict__ parent, const int* __restrict__ first_of,
                                                            const int* __restrict__ count_of, int* __restrict__ scratch, float4* __restrict__ recs,
                                                            uint4* __restrict__ qrecs, WhittedBuildMeta* __restrict__ out_meta)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sah_dyn[];
    sah_structure({n, nodes, parent, first_of, count_of, scratch, recs, qrecs, out_meta}, sah_dyn);
}

// ---------------------------------------------------------------------------------------------------------------------
// Refit (optixAccelBuild with OPTIX_BUILD_OPERATION_UPDATE): the structure of one build over MOVED vertices, topology kept.  One
// workgroup, n <= kMaxTriangles.  Keeps the Morton order (tris[3 i].w), tidx and every link; from the new positions it writes what
// build_kernel + sah_kernel would write over this topology: the bounds and from them the pad and the grid (build_kernel's formulas,
// word for word), the corners of `tris`, and every record's two boxes -- a leaf link's box from its triangles' corners -/+ pad, a
// record link's box as the union of that record's two boxes (what both builds' fits compute: fminf / fmaxf are exact, so over unchanged
// vertices the arrays come out bit for bit as built).  The records are fitted bottom-up in passes like build_kernel's fit: a record is
// fitted in the pass after the records it links to.  done[r] = the pass that fitted record r (0: not yet); a stamp of the running pass
// reads as "not yet", so one barrier per pass orders them.  The topology is read from `recs` alone, whichever build left it.
// Writes out_meta's grid_lo / grid_step only (depth, n_recs and walk_depth stay).  Scratch: done[n_recs].
// The body is refit_structure, one workgroup over one RefitTarget: refit_kernel runs it over a mesh (and over a clustered mesh's mid
// level), big_refit_clusters_kernel (rtgo_whitted_big.h) with one workgroup per cluster.
// ---------------------------------------------------------------------------------------------------------------------
// What one refit works on: the vertices and index triples its triangles name, the structure of one build (n triangles, n_recs records
// at recs / qrecs, the sorted triangles at tris), done[n_recs], and where the grid goes
struct RefitTarget {
    const float* positions;
    const unsigned int* indices;
    int n, n_recs, walk_depth;
    float4* recs;
    float4* tris;
    uint4* qrecs;
    int* done;
    WhittedBuildMeta* out_meta;
};

// One workgroup of kBuildThreads threads, s_red: its 6 x kBuildThreads floats of LDS.  kSubset: the structure's triangles are the n that
// tris[3 i].w names among the triples of `indices` (a cluster of a clustered mesh: the bounds are taken over them, as the cluster's build
// took them over its slice of the gathered triples); otherwise they are triples 0 .. n - 1.
template <bool kSubset>
__device__ __forceinline__ void refit_structure(const RefitTarget& t, float (*s_red)[kBuildThreads])
{
    const float* __restrict__ positions = t.positions;
    const unsigned int* __restrict__ indices = t.indices;
    const int n = t.n, n_recs = t.n_recs, walk_depth = t.walk_depth;
    float4* recs = t.recs;
    float4* tris = t.tris;
    uint4* qrecs = t.qrecs;
    int* done = t.done;
    WhittedBuildMeta* __restrict__ out_meta = t.out_meta;
    const int tid = threadIdx.x;
    // scene bounds, pad and grid: build_kernel's
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < n; i += kBuildThreads) {
        const int tri = kSubset ? __float_as_int(tris[3 * i + 0].w) : i;
        for (int k = 0; k < 3; ++k) {
            const unsigned int vi = indices[3 * tri + k];
            for (int a = 0; a < 3; ++a) {
                const float c = positions[3 * vi + a];
                lo[a] = fminf(lo[a], c);
                hi[a] = fmaxf(hi[a], c);
            }
        }
    }
    reduce_bounds<kBuildThreads>(s_red, tid, lo, hi);
    float blo[3], ext[3], maxext = 0.0f, reach = 0.0f;
    for (int a = 0; a < 3; ++a) {
        blo[a] = s_red[a][0];
        ext[a] = s_red[3 + a][0] - s_red[a][0];
        maxext = fmaxf(maxext, ext[a]);
        reach = fmaxf(reach, fmaxf(fabsf(s_red[a][0]), fabsf(s_red[3 + a][0])));
    }
    const float pad = box_pad(maxext, reach);
    float glo[3], gstep[3];
    for (int a = 0; a < 3; ++a) {
        glo[a] = blo[a] - pad;
        gstep[a] = (ext[a] + 2.0f * pad) * (1.0f / 65533.0f);
    }
    if (tid == 0) {
        out_meta->grid_lo = mk(glo[0], glo[1], glo[2]);
        out_meta->grid_step = mk(gstep[0], gstep[1], gstep[2]);
    }
    // the triangles' corners, in the order they have
    for (int i = tid; i < n; i += kBuildThreads) {
        const unsigned int tri = (unsigned int)__float_as_int(tris[3 * i + 0].w);
        const unsigned int i0 = indices[3 * tri + 0], i1 = indices[3 * tri + 1], i2 = indices[3 * tri + 2];
        tris[3 * i + 0] = make_float4(positions[3 * i0 + 0], positions[3 * i0 + 1], positions[3 * i0 + 2], __int_as_float((int)tri));
        tris[3 * i + 1] = make_float4(positions[3 * i1 + 0], positions[3 * i1 + 1], positions[3 * i1 + 2], 0.0f);
        tris[3 * i + 2] = make_float4(positions[3 * i2 + 0], positions[3 * i2 + 1], positions[3 * i2 + 2], 0.0f);
    }
    for (int r = tid; r < n_recs; r += kBuildThreads) done[r] = 0;
    __syncthreads();
    // the box behind a link: a leaf's from its triangles, a record's from its two boxes (fitted in an earlier pass)
    auto link_box = [&](int link, float4& b0, float4& b1) {
        if (link < 0) {
            const int code = -1 - link, first = code & ((1 << kLeafShift) - 1), cnt = (code >> kLeafShift) + 1;
            float l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int k = 3 * first; k < 3 * (first + cnt); ++k) {
                const float4 c = tris[k];
                l[0] = fminf(l[0], c.x); l[1] = fminf(l[1], c.y); l[2] = fminf(l[2], c.z);
                h[0] = fmaxf(h[0], c.x); h[1] = fmaxf(h[1], c.y); h[2] = fmaxf(h[2], c.z);
            }
            b0 = make_float4(l[0] - pad, l[1] - pad, l[2] - pad, 0.0f);
            b1 = make_float4(h[0] + pad, h[1] + pad, h[2] + pad, 0.0f);
        } else {
            const float4 q0 = recs[4 * link + 0], q1 = recs[4 * link + 1], q2 = recs[4 * link + 2], q3 = recs[4 * link + 3];
            b0 = make_float4(fminf(q0.x, q2.x), fminf(q0.y, q2.y), fminf(q0.z, q2.z), 0.0f);
            b1 = make_float4(fmaxf(q1.x, q3.x), fmaxf(q1.y, q3.y), fmaxf(q1.z, q3.z), 0.0f);
        }
    };
    // leaves lie within the triangles and records within the records; anything else is never ready, and the passes run out
    auto ready = [&](int link, int pass) {
        if (link < 0) return ((-1 - link) & ((1 << kLeafShift) - 1)) + ((-1 - link) >> kLeafShift) < n;
        const int stamp = link < n_recs ? done[link] : 0;
        return stamp != 0 && stamp < pass;
    };
    if (n_recs == 0) return;   // the mesh is one leaf: the triangles and the grid are all of it
    for (int pass = 1; pass <= walk_depth; ++pass) {   // (a record's height in the tree is at most walk_depth)
        for (int r = tid; r < n_recs; r += kBuildThreads) {
            if (done[r] != 0) continue;
            const int la = __float_as_int(recs[4 * r + 0].w), lb = __float_as_int(recs[4 * r + 2].w);
            if (!ready(la, pass) || !ready(lb, pass)) continue;
            float4 a0, a1, b0, b1;
            link_box(la, a0, a1);
            link_box(lb, b0, b1);
            write_walk_record(recs, qrecs, r, a0, a1, la, b0, b1, lb, glo, gstep);
            done[r] = pass;
        }
        __syncthreads();
        // the root is done (uniform: a thread already in the next pass can only turn a 0 into pass + 1, and both read as "not done")
        const int root = done[0];
        if (root != 0 && root <= pass) break;
    }
}


__global__ __launch_bounds__(kBuildThreads) void refit_kernel(const float* __restrict__ positions, const unsigned int* __restrict__ indices, int n, int n_recs,
                                                              int walk_depth, float4* recs, float4* tris, uint4* qrecs, int* done,
                                                              WhittedBuildMeta* __restrict__ out_meta)
{
    __shared__ float s_red[6][kBuildThreads];
    refit_structure<false>({positions, indices, n, n_recs, walk_depth, recs, tris, qrecs, done, out_meta}, s_red);
}

}  // namespace whitted
}  // namespace rtgo
