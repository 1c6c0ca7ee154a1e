// rtgo_device.h -- gfx950 device code of the RayTracinGO hot path: the render megakernel that replaces the OptiX pipeline of engine/kernel.cu (raygen + traversal + 4 intersection
// programs + 2 closest-hit programs + miss + accumulation), all in one launch.  What builds the structures it walks (scene
// preparation, the LBVH build kernel) is rtgo_build.h, included below.
//
// Written for CDNA4 only (wave64, LDS-resident scene, per-lane LDS traversal stack).  No MFMA: there is no dense
// contraction on this path.  Arithmetic follows the reference's IEEE-float32 statement operation by operation (this
// translation unit is compiled with -ffp-contract=off); the few places where the hoisted form differs from the
// literal one only in the sign of a zero are noted.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtgo {

constexpr int kMaxBlock = 1024;      // workgroup = 256, 512 or 1024 threads: chosen per scene so that 16 waves fit a CU's LDS
constexpr int kStackDepth = 24;      // per-lane traversal stack entries of the canonical walk (LBVH depth is checked against it at build)
constexpr int kDefaultLeafBudget = 6;   // fast walk: LBVH subtrees whose leaf-test cost is <= this many rectangle tests become one leaf (6 = one cube)
constexpr int kMaxPrims = 512;
constexpr int kMaxLights = 10;
constexpr int kSamplesPerPass = 16;   // samples of one pixel that run side by side (the in-order sum costs this many lane exchanges)
constexpr int kQueues = 32;          // work-queue heads (power of two <= 64; 8 / 16 / 32 heads: a 1/8 frame share takes 0.261 / 0.248 / 0.244 ms)
constexpr unsigned int kQueueStride = 16;   // words between two heads: one 64-byte line each
constexpr int kUnitsPerGrab = 4;     // most units (64 paths each) in one strip = one queue entry (longer strips: seeds cheaper, balance worse)
constexpr int kSampleTab = 256;     // samples per pixel whose start (LCG skip, jitter cell) comes from a table in LDS (16 B each); beyond: computed
constexpr int kCamWords = 16;        // raygen constants in LDS (render_kernel's s_cam) ...
constexpr int kCamWordsLean = 20;    // ... + the launch's two reciprocals in the 6-waves variant (a multiple of 4: s_tab follows)
constexpr int kMaxLevels = 5;        // bounce records kept per path (maxTraceDepth <= 5)
// path mode, the deferred fold (FOLDLATE, rtgo_render_body.inc): what an ended path's payload is, where it is no emitter's primitive index
constexpr int kEndsInBackground = -1, kEndsInZero = -2;
constexpr int kMaxEmitters = 4;      // emitters of the last-ray certificate (LaunchParams::emit_n); scenes with more go without it
// the pair kernels' scene (fast_pair: a root over two cuboid leaves of six records each), which their launches vouch for: the tree's
// nodes and its records.  Compile-time values there, so that the up-front list -- the records from kPairSmall on, in LDS and in global
// memory -- sits at constant offsets instead of at offsets every ray derives from LaunchParams::n_fnodes and n_small
constexpr int kPairNodes = 3, kPairSmall = 12;
constexpr float kPi = 3.14159265358979323846f;  // M_PIf, sutil/vec_math.h:43

struct v3 {
    float x, y, z;
};

// ---- LDS/global scene layout ----------------------------------------------------------------------------------
// node record, 32 B = 2 x float4:  q0 = (bmin.xyz, bits(left)), q1 = (bmax.xyz, bits(right))
//   internal nodes [0, n-2], leaves [n-1, 2n-2]; leaf: left = primitive (SBT) index, right = -1
// primitive record, 96 B = 6 x float4:
//   q0..q2 = rows 0..2 of M^-1 (row 3 is never needed: TransformRay/TransformNormal drop w, kernel.cu:125-142)
//   q3 = (kd.xyz, specularity)   q4 = (kr.xyz, bits(type))   q5 = (Le.xyz, 0)
struct LightRec {
    float corner[3], v1[3], v2[3], normal[3], color[3], falloff;  // device::SurfaceLight, params.h:73-87
};

// The fast walk's third structure (GRID instantiations): a uniform grid over the small primitives, walked cell by cell (fast_grid).
// It travels in the buffer and the LDS region of the tree it replaces: n_cells words (first item | count << 16), then the items (16-bit
// positions into fprims).
struct GridParams {
    float min_x, min_y, min_z, cs_x, cs_y, cs_z, ics_x, ics_y, ics_z;   // lower corner, cell size, 1 / cell size
    int nx, ny, nz;                 // cells per axis (<= 32 each)
    int n_cells;                    // words of the table: (nx + 2) (ny + 2) (nz + 2), a border of empty cells around the grid
    int rec_off4, items_off4;       // where the cell records and the item lists start, in float4 units from the table's start
    float margin;                   // fast_grid stops once the closest hit lies this far (in t) before the exit of the cell it is in
};

// ---- the packed fields of the fast walk's structure: build_kernel (rtgo_build.h) encodes, the walk and the host decode
// A group the walk scans linearly (the up-front list, a multi-record leaf): pairs of opposite rectangles at its start (pair_test) and
// its cuboid certificate (0: none, 1: a box seen from outside, 2: a room seen from inside; cuboid_range)
__host__ __device__ constexpr int encode_group(int pairs, int cert) { return pairs | (cert << 8); }
__host__ __device__ constexpr int group_pairs(int group) { return group & 0xFF; }
__host__ __device__ constexpr int group_cert(int group) { return group >> 8; }
// A leaf of the fast walk's tree: left = its first record, right = -(count | group << 12), i.e. -(count | pairs << 12 | cuboid << 20)
__host__ __device__ constexpr int encode_leaf_link(int count, int group) { return -(count | (group << 12)); }
__host__ __device__ constexpr int leaf_count(int link) { return (-link) & 0xFFF; }
__host__ __device__ constexpr int leaf_pairs(int link) { return ((-link) >> 12) & 0xFF; }
__host__ __device__ constexpr int leaf_cuboid(int link) { return (-link) >> 20; }

// The pair kernels' launches (render_pair_kernel, render_pair7_kernel): the three words each of their rays reads before its walk, side by
// side, so that they arrive as a two-word and a one-word scalar load under one wait.  cub_mu and n_prims are LaunchParams' fields of
// those names.  last_depth is the last-ray certificate as the one value the ray loop compares: the depth at which a ray is its path's
// last (max_depth) when the launch has the certificate (emit_n != 0), -1 (no depth) when it has not -- the host decides once what every
// ray would otherwise decide from two fields.  The other kernels read LaunchParams' own fields, as they did; the words lie where a GRID
// launch has its grid, so that no field of LaunchParams moves and every other kernel compiles to the instructions it had.
// The words from room_map on are read by render_roomw_kernel alone (room_world): the room's slab certificate in WORLD axes
// (rtgo_room_world.h), filled when the walked tree holds it at this launch's reach.  room_lo / room_hi: the room's planes per world axis;
// room_mu: the margin in world units; room_thr: |d_j| at or below it counts as parallel to the walls of axis j; room_map: three bits per
// plane, the face's offset in the group, plane = 2 * world axis + (0: low, 1: high).
struct PairWords {
    float cub_mu;
    int last_depth;
    int n_prims;
    int room_map;
    float room_lo[3], room_hi[3];
    float room_mu, room_thr;
};

struct LaunchParams {
    const float4* nodes;            // canonical LBVH, 2 float4 per node
    const float4* prims;            // 6 float4 per primitive, SBT order
    const float4* fnodes;           // the fast walk's tree: 2 float4 per node, root 0; leaf: left = first record, right = -(count | pairs << 12)
    int n_fnodes;
    const float4* fprims;           // 4 float4 per primitive in Morton order: rows 0..2 of M^-1, (bits(type), bits(SBT index), 0, 0)
    const float4* frames;           // 2 float4 per primitive, SBT order: the shading frame of a flat primitive (see build_kernel), w of the first = 1 when it has one
    int stack_depth;                // per-lane LDS stack entries this launch needs
    int n_small;                    // fast walk: fprims [0, n_small) are in the tree, [n_small, n_prims) are tested up front
    int n_big_pairs;                // ... of which the first 2*n_big_pairs records are pairs of opposite rectangles (pair_test)
    int list_cub;                   // 1 / 2: the up-front list starts with three pairs certified as one box / one room (cuboid_range), 0: it does not
    float cub_mu;                   // cuboid_range's margin for this launch (object-space units of a face's y axis)
    int tree_spheres;              // 1: every primitive of the fast walk's tree is a sphere (balls): leaves go straight to the sphere test
    union {
        GridParams grid;            // GRID instantiations: fnodes holds the grid instead of a tree
        PairWords pair;             // the pair kernels' launches (they walk no grid): see PairWords
    };
    const LightRec* lights;
    float4* accum;
    uchar4* image;
    unsigned int* queue;            // kQueues work-queue heads, kQueueStride words apart, all zero when the launch starts
    unsigned int* queue_next;       // the other set of heads: zeroed by this launch for the next one (no memset between frames)
    // Pixel seeds of a progressive job: tea<16>(pixel, frame) for every pixel of the hot strips, grab * 64 / nn_eff words per strip
    // (word strip * strip_px + i: pixel i of strip `strip`).  `seeds`: this frame's, written by the previous launch on this context
    // (null: hash them inline).  `seeds_next`: where this launch writes frame + 1's (null: it does not), 64 pixels per chunk, by
    // the waves whose queue has run dry.
    const unsigned int* seeds;
    unsigned int* seeds_next;
    unsigned long long* counters;   // [0] rays_total [1] rays_occlusion [2] node_visits [3] prim_tests [4] hits
    int n_prims, n_nodes, n_lights;
    unsigned int W, H;              // full image
    int sqrt_spp, max_depth;
    unsigned int frame;
    int ambient;
    int count_stats;                // canonical walk only: flush the V/T/h counters (0 when the walk is a fallback, not a request)
    unsigned int x0, y0, w, h;      // window
    unsigned int band_h, n_ranks, rank, local_rows;
    unsigned int n_tiles;            // work-queue entries of this launch = n_hot strips, then n_cold chunks
    // The strips that can contain geometry form a rectangle of hot_w x hot_h strips at (strip column hot_x0, local row hot_y0):
    // the screen bounds of the scene, computed by the host.  Queue entries [0, n_hot) are those strips, row-major.
    unsigned int hot_x0, hot_y0, hot_w, hot_h, n_hot;
    // Every pixel outside it is background whatever its samples' jitter (no primary ray can reach the scene's bounds), so the
    // timed kernel writes those without tracing (the instrumented kernel, which defines V/T/h, traces everything: the host
    // then makes the rectangle the whole window).  They are cut into 64-pixel row segments, enumerated region by region
    // (rows below the rectangle, rows above, left of it, right of it); queue entry n_hot + c is cold chunk c = segments
    // [c*cold_cs, (c+1)*cold_cs).  They sit at the END of the queue: cheap filler for the waves that run out of strips first.
    unsigned int cold_x0, cold_x1;   // window columns [cold_x0, cold_x1) belong to the rectangle's strips
    unsigned int rows_above;         // local rows over the rectangle (those below it: hot_y0)
    unsigned int segs_full, segs_l, segs_r;   // 64-pixel segments per full row, per row left / right of the rectangle
    unsigned int n_cold_segs, cold_cs;
    unsigned int grab;               // units per strip (1..kUnitsPerGrab, strip <= 64 pixels)
    // One bit per strip of the rectangle (bit = strip index, row-major): 0 = no primitive's screen rectangle reaches the strip, so
    // its pixels are background like those outside the rectangle and are written without tracing.  Null when every strip is hot
    // (scenes that fill their rectangle: nothing to look up then).
    const unsigned int* hot_mask;
#ifdef RTGO_TIMELINE
    unsigned long long* timeline;    // diagnostic build: 8 words per wave, see tools/timeline.py
#endif
#ifdef RTGO_CMPWALK
    float* cmp;                      // diagnostic build: [0] = number of rays on which the two walks disagree, then 16-float records
#endif
    v3 eye, U, V, Wv, bg;
    v3 bg_pixel;                     // ((0 + bg) + bg + ... N*N times) * (1/(N*N)) in float: the value of a pixel whose samples all miss
    // Last-ray certificate (path mode; rtgo_capi.hip, emitter_cert and last_ray_params): the up-front list is a room followed by the
    // scene's emitters and nothing else, each emitter inside every wall by more than a margin, and a miss pays the same +0 as a
    // non-emitter hit.  A path's last ray then skips the room, and only the lanes that hit an emitter walk the tree (closest_hit_fast).
    // emit_n: the emitters (fprims [n_small + 6, n_prims)); 0: off.
    int emit_n;
    // render_frames_kernel: this launch renders frames frame .. frame + n_frames - 1 (the other kernels render `frame` and do not read it)
    unsigned int n_frames;
};
// (PairWords lies inside the grid's space: no field after it moves, so every kernel but the pair kernels compiles as it did without it)
static_assert(sizeof(PairWords) <= sizeof(GridParams) && alignof(PairWords) <= alignof(GridParams), "PairWords must fit the space of LaunchParams::grid");
static_assert(offsetof(LaunchParams, pair) == offsetof(LaunchParams, grid) && offsetof(LaunchParams, lights) == offsetof(LaunchParams, grid) + sizeof(GridParams),
              "LaunchParams: the pair words overlay the grid and the fields after it stay where they are");

// ---- float3 helpers, same operation order as sutil/vec_math.h ----------------------------------------------------
__device__ __forceinline__ v3 mk(float x, float y, float z) { return v3{x, y, z}; }
__device__ __forceinline__ v3 vadd(v3 a, v3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ v3 vsub(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ v3 vmul(v3 a, v3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ v3 vscale(v3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ v3 vneg(v3 a) { return mk(-a.x, -a.y, -a.z); }
__device__ __forceinline__ float vdot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }  // vec_math.h:523-526
__device__ __forceinline__ v3 vcross(v3 a, v3 b)                                                   // vec_math.h:529-532
{
    return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
// Correctly rounded a / b and sqrt(x) as the compiler's own expansions compute them, without the range plumbing around them.
// hipcc expands an IEEE f32 division into v_div_scale x 2, v_rcp, six v_fma / v_mul, v_div_fmas, v_div_fixup (12 instructions): the
// scale / fmas / fixup steps only act when an operand is zero, infinite, NaN or subnormal, when |a / b| leaves [2^-126, 2^96) or when
// |a| < 2^-103 (V_DIV_SCALE_F32's rules); otherwise they pass their operands through and the quotient is the value of the eight steps
// below, bit for bit.  Likewise sqrtf: v_sqrt_f32 and two residual tests against the neighbouring floats are the correctly rounded
// root for normal x in [2^-96, inf); the other nine instructions rescale subnormal inputs and pass 0 / inf / NaN through.
// Where these run (ray parameters t = -o.y / d.y of front-facing planes with o.y > 0, sphere roots, lengths of directions and
// normals) a quotient outside those ranges is rejected by the comparisons that follow whatever its value (|t| >= 2^95 or < 2^-126
// against 1e-4 < t < tmax <= 1e16), and operands are float combinations of scene coordinates (|.| <= 500, granularity ~1e-7 of
// them): zero, or nowhere near 2^-103.  The canonical walk keeps the plain operators, so every fast == canonical test -- the suite,
// tools/cmp_walks.py ray by ray, the fuzzers -- holds the lean forms to IEEE on every ray traced.  -DRTGO_IEEE_OPS: plain operators.
__device__ __forceinline__ float div_cr(float a, float b)
{
#ifdef RTGO_IEEE_OPS
    return a / b;
#else
    const float y0 = __builtin_amdgcn_rcpf(b);
    const float e = fmaf(-b, y0, 1.0f);
    const float y1 = fmaf(e, y0, y0);
    const float q0 = a * y1;
    const float r0 = fmaf(-b, q0, a);
    const float q1 = fmaf(r0, y1, q0);
    const float r1 = fmaf(-b, q1, a);
    return fmaf(r1, y1, q1);
#endif
}
__device__ __forceinline__ float sqrt_cr(float x)
{
#ifdef RTGO_IEEE_OPS
    return sqrtf(x);
#else
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sdn = __uint_as_float(__float_as_uint(s) - 1u), sup = __uint_as_float(__float_as_uint(s) + 1u);
    const float vdn = fmaf(-sdn, s, x), vup = fmaf(-sup, s, x);
    float r = vdn <= 0.0f ? sdn : s;
    r = vup > 0.0f ? sup : r;
    return r;
#endif
}

// sincosf(x) for 0 <= x < 131072, finite: the device library's own small-argument path (three-constant Cody-Waite reduction by pi/2, its
// two minimax polynomials, the quadrant logic) without what it wraps around it -- the test for the Payne-Hanek path, the sign of x, the
// inf / NaN class test on both results.  GetRayOnHemisphere's angles are acos(..) in [0, pi/2] and 2 pi r in [0, 2 pi).
// tools/lean_ops_probe.hip runs it against sincosf on EVERY float of [0, 8): identical bits.  -DRTGO_IEEE_OPS: the library call.
__device__ __forceinline__ void sincos_cr(float x, float* s_out, float* c_out)
{
#ifdef RTGO_IEEE_OPS
    sincosf(x, s_out, c_out);
#else
    const float n = rintf(x * __uint_as_float(0x3f22f983u));                  // x * 2/pi, to nearest even
    const int ni = (int)n;
    float r = fmaf(n, __uint_as_float(0xbfc90fdau), x);
    r = fmaf(n, __uint_as_float(0xb3a22168u), r);
    r = fmaf(n, __uint_as_float(0xa7c234c4u), r);
    const float r2 = r * r;
    float t = fmaf(__uint_as_float(0xb94c1982u), r2, __uint_as_float(0x3c0881c4u));
    t = fmaf(r2, t, __uint_as_float(0xbe2aaa9du));
    t = r2 * t;
    const float sr = fmaf(r, t, r);
    float u = fmaf(__uint_as_float(0x37d75334u), r2, __uint_as_float(0xbab64f3bu));
    u = fmaf(r2, u, __uint_as_float(0x3d2aabf7u));
    u = fmaf(r2, u, __uint_as_float(0xbf000004u));
    const float cr = fmaf(r2, u, 1.0f);
    const bool even = (ni & 1) == 0;
    const unsigned int flip = ((unsigned int)ni << 30) & 0x80000000u;          // quadrants 2 and 3
    *s_out = __uint_as_float(__float_as_uint(even ? sr : cr) ^ flip);
    *c_out = __uint_as_float(__float_as_uint(even ? cr : -sr) ^ flip);
#endif
}

__device__ __forceinline__ float vlength(v3 v) { return sqrt_cr(vdot(v, v)); }  // vec_math.h:535-538
__device__ __forceinline__ v3 vnormalize(v3 v)                               // vec_math.h:541-545
{
    float invLen = div_cr(1.0f, sqrt_cr(vdot(v, v)));
    return vscale(v, invLen);
}

// ---- RNG: cuda/random.h:30-66 -------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int tea16(unsigned int v0, unsigned int v1)
{
    unsigned int s0 = 0;
#pragma unroll
    for (int n = 0; n < 16; ++n) {
        s0 += 0x9e3779b9u;
        v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
        v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    return v0;
}
// the LCG advanced by m draws in O(log m): f(s) = a*s + c, f^m(s) = A*s + C by repeated squaring of the affine map
__device__ __forceinline__ unsigned int lcg_skip(unsigned int s, unsigned int m)
{
    unsigned int A = 1u, C = 0u, a = 1664525u, c = 1013904223u;
    while (m) {
        if (m & 1u) {
            A = A * a;
            C = C * a + c;
        }
        c = (a + 1u) * c;
        a = a * a;
        m >>= 1;
    }
    return A * s + C;
}
__device__ __forceinline__ float rnd(unsigned int& prev)
{
    prev = 1664525u * prev + 1013904223u;
    return (float)(prev & 0x00FFFFFFu) / (float)0x01000000;
}

// ---- intersection programs (kernel.cu:250-416) with M^-1 hoisted to scene upload -------------------------------------
// TransformRay (kernel.cu:125-135).  The w = 0 / w = 1 products of the 4-term operator* (Matrix.h:472-493) are
// dropped / folded: x*1 is exact and +(m*0) can only change the sign of a zero.
__device__ __forceinline__ v3 xf_dir(const float4 r0, const float4 r1, const float4 r2, v3 d)
{
    return mk(r0.x * d.x + r0.y * d.y + r0.z * d.z, r1.x * d.x + r1.y * d.y + r1.z * d.z,
              r2.x * d.x + r2.y * d.y + r2.z * d.z);
}
__device__ __forceinline__ v3 xf_point(const float4 r0, const float4 r1, const float4 r2, v3 o)
{
    return mk(r0.x * o.x + r0.y * o.y + r0.z * o.z + r0.w, r1.x * o.x + r1.y * o.y + r1.z * o.z + r1.w,
              r2.x * o.x + r2.y * o.y + r2.z * o.z + r2.w);
}
// TransformNormal (kernel.cu:138-142): transpose(M^-1) * (n, 0)
__device__ __forceinline__ v3 xf_normal(const float4 r0, const float4 r1, const float4 r2, v3 n)
{
    return mk(r0.x * n.x + r1.x * n.y + r2.x * n.z, r0.y * n.x + r1.y * n.y + r2.y * n.z,
              r0.z * n.x + r1.z * n.y + r2.z * n.z);
}

// returns true when the program would call optixReportIntersection(t, n)
__device__ __forceinline__ bool intersect_prim(int type, const float4 r0, const float4 r1, const float4 r2, v3 wo, v3 wd,
                                               float& t_out, v3& n_out)
{
    const v3 d = xf_dir(r0, r1, r2, wd);
    const v3 o = xf_point(r0, r1, r2, wo);
    if (type == 2) {  // __intersection__rectangle, kernel.cu:372-416 (one-sided: only rays going down in object space)
        const float divisor = d.y;
        if (divisor != 0.0f) {
            const float t = (0.0f - o.y) / divisor;
            if (t > 0.0001f) {
                const float px = o.x + t * d.x, pz = o.z + t * d.z;
                const float u = px + 0.5f;      // dot(p - p0, a), a = (1,0,0), p0 = (-1/2, 0, 1/2)
                const float v = -(pz - 0.5f);   // dot(p - p0, b), b = (0,0,-1)
                if (0.0f < u && u < 1.0f && 0.0f < v && v < 1.0f && d.y < 0.0f) {
                    t_out = t;
                    n_out = xf_normal(r0, r1, r2, mk(0.0f, 1.0f, 0.0f));
                    return true;
                }
            }
        }
        return false;
    }
    if (type == 3) {  // __intersection__sphere, kernel.cu:250-287 (near root only)
        const float a = vdot(d, d);
        const float b = 2.0f * vdot(d, o);
        const float c = vdot(o, o) - 1.0f;
        const float discr = b * b - 4.0f * a * c;
        if (discr > 0.0f) {
            const float sdiscr = sqrtf(discr);
            const float t = (-b - sdiscr) / (2.0f * a);
            if (t > 0.0001f) {
                const v3 n = vnormalize(vadd(o, vscale(d, t)));
                t_out = t;
                n_out = xf_normal(r0, r1, r2, n);
                return true;
            }
        }
        return false;
    }
    if (type == 0) {  // __intersection__cylinder + GetTMinCylinder, kernel.cu:290-331, 152-181
        const float a = d.x * d.x + d.z * d.z;
        const float b = 2.0f * (o.x * d.x + o.z * d.z);
        const float c = o.x * o.x + o.z * o.z - 1.0f;
        const float discr = b * b - 4.0f * a * c;
        if (discr > 0.001f) {
            const float sdiscr = sqrtf(discr);
            const float t0 = (-b + sdiscr) / (2.0f * a);
            const float t1 = (-b - sdiscr) / (2.0f * a);
            float t = 1e16f;
            bool valid = false;
            if (t0 > 0.001f) {
                const float py = o.y + t0 * d.y;
                if (py > -1.0f && py < 1.0f) {
                    t = t0;
                    valid = true;
                }
            }
            if (t1 > 0.001f && t1 < t) {
                const float py = o.y + t1 * d.y;
                if (py > -1.0f && py < 1.0f) {
                    t = t1;
                    valid = true;
                }
            }
            if (valid) {
                const float px = o.x + t * d.x, pz = o.z + t * d.z;
                t_out = t;
                n_out = xf_normal(r0, r1, r2, mk(px, 0.0f, pz));
                return true;
            }
        }
        return false;
    }
    {  // __intersection__disk, kernel.cu:334-369 (two-sided, |d.y| >= 0.01)
        const float divisor = d.y;
        if (!(divisor > 0.0f - 0.01f && divisor < 0.0f + 0.01f)) {
            const float t = (-o.y) / divisor;
            if (t > 0.0001f) {
                const v3 p = vadd(o, vscale(d, t));
                if (vdot(p, p) < 1.0f) {
                    t_out = t;
                    n_out = xf_normal(r0, r1, r2, mk(0.0f, 1.0f, 0.0f));
                    return true;
                }
            }
        }
        return false;
    }
}

// slab test of one node box against [tmin, tmax]; identical, operation for operation, to oracle box_test()
__device__ __forceinline__ bool box_test(const float4 q0, const float4 q1, v3 o, v3 id, float tmin, float tmax, float& tn_out)
{
    float t0 = (q0.x - o.x) * id.x, t1 = (q1.x - o.x) * id.x;
    float tn = fminf(t0, t1), tf = fmaxf(t0, t1);
    t0 = (q0.y - o.y) * id.y;
    t1 = (q1.y - o.y) * id.y;
    tn = fmaxf(tn, fminf(t0, t1));
    tf = fminf(tf, fmaxf(t0, t1));
    t0 = (q0.z - o.z) * id.z;
    t1 = (q1.z - o.z) * id.z;
    tn = fmaxf(tn, fminf(t0, t1));
    tf = fminf(tf, fmaxf(t0, t1));
    tn = fmaxf(tn, tmin);
    tf = fminf(tf, tmax);
    tn_out = tn;
    return tn <= tf;
}

struct Hit {
    float t;
    v3 n;      // world-space normal, not normalised (TransformNormal); not filled in for flat winners of the fast walk: their frame is in LDS
    int prim;
};

// optixTrace's traversal over the LDS-resident canonical LBVH: nearest child first, far child pushed on the per-lane LDS
// stack with its entry distance and culled against the current closest hit when popped.  A hit is accepted iff
// tmin < t < current tmax; ties keep the lower SBT index.
template <bool STATS>
__device__ __forceinline__ bool closest_hit(const float4* __restrict__ s_nodes, const float4* __restrict__ s_prims,
                                            float2* __restrict__ s_stack, int bshift, v3 o, v3 d, float tmin, float tmax, Hit& best,
                                            unsigned int& c_nodes, unsigned int& c_tests)
{
    best.prim = -1;
    best.t = tmax;
    best.n = mk(0.0f, 0.0f, 0.0f);
    const v3 id = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    float tn;
    float4 q0 = s_nodes[0], q1 = s_nodes[1];
    if (STATS) c_nodes += 1;
    if (!box_test(q0, q1, o, id, tmin, best.t, tn)) return false;
    int sp = 0;
    int left = __float_as_int(q0.w), right = __float_as_int(q1.w);
    for (;;) {
        bool pop = false;
        if (right < 0) {
            const int i = left;
            const float4 r0 = s_prims[6 * i + 0], r1 = s_prims[6 * i + 1], r2 = s_prims[6 * i + 2];
            const int type = __float_as_int(s_prims[6 * i + 4].w);
            float t;
            v3 n;
            if (STATS) c_tests += 1;
            if (intersect_prim(type, r0, r1, r2, o, d, t, n) && t > tmin &&
                (t < best.t || (t == best.t && best.prim >= 0 && i < best.prim))) {
                best.t = t;
                best.n = n;
                best.prim = i;
            }
            pop = true;
        } else {
            const float4 l0 = s_nodes[2 * left], l1 = s_nodes[2 * left + 1];
            const float4 h0 = s_nodes[2 * right], h1 = s_nodes[2 * right + 1];
            float tl, tr;
            if (STATS) c_nodes += 2;
            const bool hl = box_test(l0, l1, o, id, tmin, best.t, tl);
            const bool hr = box_test(h0, h1, o, id, tmin, best.t, tr);
            if (hl && hr) {
                const bool swap = tr < tl;
                // push the far child
                const int far_idx = swap ? left : right;
                const float far_t = swap ? tl : tr;
                s_stack[sp << bshift] = make_float2(far_t, __int_as_float(far_idx));
                ++sp;
                if (swap) {
                    left = __float_as_int(h0.w);
                    right = __float_as_int(h1.w);
                } else {
                    left = __float_as_int(l0.w);
                    right = __float_as_int(l1.w);
                }
            } else if (hl) {
                left = __float_as_int(l0.w);
                right = __float_as_int(l1.w);
            } else if (hr) {
                left = __float_as_int(h0.w);
                right = __float_as_int(h1.w);
            } else {
                pop = true;
            }
        }
        if (pop) {
            bool found = false;
            while (sp > 0) {
                --sp;
                const float2 e = s_stack[sp << bshift];
                if (e.x <= best.t) {
                    const int idx = __float_as_int(e.y);
                    const float4 n0 = s_nodes[2 * idx], n1 = s_nodes[2 * idx + 1];
                    left = __float_as_int(n0.w);
                    right = __float_as_int(n1.w);
                    found = true;
                    break;
                }
            }
            if (!found) break;
        }
    }
    return best.prim >= 0;
}

// =====================================================================================================================
// Fast walk (the kernel that is timed).  Same closest hit, bit for bit, as the canonical walk above -- every accepted
// candidate goes through the same intersection arithmetic and the same acceptance rule -- but organised for the SIMDs:
//   * LBVH subtrees whose leaf-test cost fits a budget are collapsed into one leaf whose primitives sit contiguously (Morton order), so
//     a wave spends its time in short uniform primitive loops instead of divergent one-primitive leaves;
//   * while-while structure: all lanes first descend to their next leaf, then all lanes with a leaf test it;
//   * the slab test is 6 FMAs on a reciprocal direction (v_rcp_f32): it only steers culling, which stays conservative
//     because every reference AABB is padded by 1e-3 (primitive.cpp:16,62-67), three orders above the rounding at stake;
//   * rejections that need no division come first (rectangle: d.y >= 0 or o.y <= 0 in object space can never pass
//     kernel.cu:394-400), and the normal is transformed once, for the winner only.
// =====================================================================================================================
struct FastHit {
    float t;
    int pos;   // Morton position of the winner | kFlat when it is a rectangle or a disk (object-space normal (0,1,0): kernel.cu:345,388)
    int orig;  // its SBT index (tie-break + material lookup)
};
constexpr int kFlat = 0x10000;
constexpr float kCuboidTol = 1e-4f;   // cuboid certificate: how far (in a face's object-space y) another face's corner may be on the wrong side of its plane

__device__ __forceinline__ unsigned int wave_sum(unsigned int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// A predicate of the fast walk's leaf tests, in one of two carriers (Pred<MASK>::T).  Pred<false>: a lane's bool; votes go through
// __ballot, which is what every kernel had.  Pred<true>: the whole wave's lane mask, 64 bits in an SGPR pair.  A compare builtin makes it
// (the v_cmp's own result: the bits of the lanes live at that point, zero elsewhere), it is combined on the scalar unit, a vote is
// `!= 0`, and inverse_ballot hands it back to selects and branches as the per-lane condition.  hipcc lowers __ballot of a COMBINATION of
// compares by turning the mask into a 0/1 vector register and comparing that back (v_cndmask, v_cmp_ne, s_cmp, s_cselect, s_and ahead of
// the branch), and keeps bools that live across a loop as 0/1 integers in VGPRs; the mask form compiles to s_and / s_cmp / branch alone.
// The pair kernels' ray loop takes it (MASKS, rtgo_render_body.inc); everything else keeps the bool.
// Both carriers combine with the language's own `&`, `|` and `^`; what differs is a static function here.  The compares keep their IEEE
// meaning: lt / gt / le / eq are the ordered ones (false on NaN), not_lt is the complement of ordered-less (true on NaN).  A mask has no
// bits outside the lanes live where it was made, so `a & b`, `a | b`, `a ^ b` and andnot(a, b) of such masks have none either; inv(a)
// is the complement WITHIN the lanes live where it is taken (~a alone would set the bits of the lanes that are off, which a vote would
// count).  A mask made in a region is used in that region or in one nested in it, where `&` with a mask made there, or lane(), cuts it
// down to the region's lanes.  (Plain types and static functions, no objects: a struct around the bool went through scratch.)
enum : int {   // the compare builtins' condition codes (LLVM's CmpInst::Predicate)
    kCmpFOeq = 1, kCmpFOgt = 2, kCmpFOlt = 4, kCmpFOle = 5, kCmpFUge = 11, kCmpIEq = 32, kCmpIUlt = 36, kCmpISge = 39, kCmpISlt = 40
};
template <bool MASK>
struct Pred;
template <>
struct Pred<false> {
    typedef bool T;
    static __device__ __forceinline__ T off() { return false; }
    static __device__ __forceinline__ T lt(float a, float b) { return a < b; }
    static __device__ __forceinline__ T gt(float a, float b) { return a > b; }
    static __device__ __forceinline__ T le(float a, float b) { return a <= b; }
    static __device__ __forceinline__ T eq(float a, float b) { return a == b; }
    static __device__ __forceinline__ T not_lt(float a, float b) { return !(a < b); }
    static __device__ __forceinline__ T ieq(int a, int b) { return a == b; }
    static __device__ __forceinline__ T ige(int a, int b) { return a >= b; }
    static __device__ __forceinline__ T ilt(int a, int b) { return a < b; }
    static __device__ __forceinline__ T ult(unsigned int a, unsigned int b) { return a < b; }
    static __device__ __forceinline__ T of(bool b) { return b; }
    static __device__ __forceinline__ T inv(T a) { return !a; }
    static __device__ __forceinline__ T andnot(T a, T b) { return a & !b; }
    static __device__ __forceinline__ T either(T a, T b) { return a || b; }
    static __device__ __forceinline__ T differ(T a, T b) { return a != b; }
    static __device__ __forceinline__ bool lane(T a) { return a; }
    static __device__ __forceinline__ bool any(T a) { return __ballot(a) != 0ull; }
    static __device__ __forceinline__ bool none(T a) { return __ballot(a) == 0ull; }
};
template <>
struct Pred<true> {
    typedef unsigned long long T;
    static __device__ __forceinline__ T off() { return 0ull; }
    static __device__ __forceinline__ T lt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kCmpFOlt); }
    static __device__ __forceinline__ T gt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kCmpFOgt); }
    static __device__ __forceinline__ T le(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kCmpFOle); }
    static __device__ __forceinline__ T eq(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kCmpFOeq); }
    static __device__ __forceinline__ T not_lt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kCmpFUge); }
    static __device__ __forceinline__ T ieq(int a, int b) { return __builtin_amdgcn_sicmp(a, b, kCmpIEq); }
    static __device__ __forceinline__ T ige(int a, int b) { return __builtin_amdgcn_sicmp(a, b, kCmpISge); }
    static __device__ __forceinline__ T ilt(int a, int b) { return __builtin_amdgcn_sicmp(a, b, kCmpISlt); }
    static __device__ __forceinline__ T ult(unsigned int a, unsigned int b) { return __builtin_amdgcn_uicmp(a, b, kCmpIUlt); }
    static __device__ __forceinline__ T of(bool b) { return __builtin_amdgcn_ballot_w64(b); }
    static __device__ __forceinline__ T inv(T a) { return ~a & __builtin_amdgcn_ballot_w64(true); }
    static __device__ __forceinline__ T andnot(T a, T b) { return a & ~b; }
    static __device__ __forceinline__ T either(T a, T b) { return a | b; }
    static __device__ __forceinline__ T differ(T a, T b) { return a ^ b; }
    static __device__ __forceinline__ bool lane(T a) { return __builtin_amdgcn_inverse_ballot_w64(a); }
    static __device__ __forceinline__ bool any(T a) { return a != 0ull; }
    static __device__ __forceinline__ bool none(T a) { return a == 0ull; }
};
#include "rtgo_probes.h"   // the diagnostic builds' instruments: Timeline, StreamStats, FastCounters, CmpWalk, WhittedTiming

// the acceptance rule of SURVEY a14 (tmin < t < current closest; ties keep the lower SBT index), without branches
template <bool MASK = false>
__device__ __forceinline__ typename Pred<MASK>::T closer(float t, int orig, float tmin, const FastHit& best)
{
    typedef Pred<MASK> P;
    return P::gt(t, tmin) & (P::lt(t, best.t) | (P::eq(t, best.t) & P::ige(best.orig, 0) & P::ilt(orig, best.orig)));
}

// __intersection__rectangle (kernel.cu:372-416) on M^-1 rows, as straight-line code: every lane evaluates the whole test and the
// result is committed through selects.  The lanes of a wave carry unrelated rays once paths have bounced, so some lane needs every
// stage of the test anyway; nesting the stages in branches then only adds exec-mask bookkeeping and idle lanes.  `facing` (d.y < 0 in
// object space, evaluated by the caller) and the other conditions of the reference enter as predicates.
// second half of the rectangle test for the lanes in `c` (everything up to t > 0.0001 and the closest-hit rule has passed): the hit
// point against the unit square, and the commit through selects
template <bool MASK = false, typename Ptr>
__device__ __forceinline__ void rect_finish(Ptr rec, float t, typename Pred<MASK>::T c, int pos, int orig, v3 wo, v3 wd, FastHit& best)
{
    typedef Pred<MASK> P;
    if (P::none(c)) return;   // (coherent waves -- primary rays -- often leave here together)
    const float4 r0 = rec[0], r2 = rec[2];
    const float dx = r0.x * wd.x + r0.y * wd.y + r0.z * wd.z, dz = r2.x * wd.x + r2.y * wd.y + r2.z * wd.z;
    const float ox = r0.x * wo.x + r0.y * wo.y + r0.z * wo.z + r0.w, oz = r2.x * wo.x + r2.y * wo.y + r2.z * wo.z + r2.w;
    const float px = ox + t * dx, pz = oz + t * dz;
    const float u = px + 0.5f, v = -(pz - 0.5f);
    c = c & P::lt(0.0f, u) & P::lt(u, 1.0f) & P::lt(0.0f, v) & P::lt(v, 1.0f);
    const bool cl = P::lane(c);
    best.t = cl ? t : best.t;
    best.pos = cl ? (pos | kFlat) : best.pos;
    best.orig = cl ? orig : best.orig;
}

template <bool MASK = false, typename Ptr>
__device__ __forceinline__ void rect_commit(Ptr rec, const float4 r1, float dy, typename Pred<MASK>::T facing, int pos, int orig, v3 wo, v3 wd, float tmin, FastHit& best)
{
    typedef Pred<MASK> P;
    const float oy = r1.x * wo.x + r1.y * wo.y + r1.z * wo.z + r1.w;
    // oy > 0 with d.y < 0 is the only way to t > 0 (so d.y != 0 and t > 1e-4 can hold); lanes that fail carry garbage in t
    const float t = div_cr(0.0f - oy, dy);
    const typename P::T c = facing & P::gt(oy, 0.0f) & P::gt(t, 0.0001f) & closer<MASK>(t, orig, tmin, best);
    rect_finish<MASK>(rec, t, c, pos, orig, wo, wd, best);
}

// MASK: the carrier of the rectangle branch's predicates (Pred); the quadrics' branches are per-lane code either way
template <bool MASK = false, typename Ptr>
__device__ __forceinline__ void leaf_test(Ptr s_fprims, int pos, v3 wo, v3 wd, float tmin, FastHit& best)
{
    const float4 r1 = s_fprims[4 * pos + 1];
    const float4 meta = s_fprims[4 * pos + 3];
    const int type = __float_as_int(meta.x), orig = __float_as_int(meta.y);
    if (type == 2) {  // rectangle
        const float dy = r1.x * wd.x + r1.y * wd.y + r1.z * wd.z;
        rect_commit<MASK>(s_fprims + 4 * pos, r1, dy, Pred<MASK>::lt(dy, 0.0f), pos, orig, wo, wd, tmin, best);
        return;
    }
    const float4 r0 = s_fprims[4 * pos + 0], r2 = s_fprims[4 * pos + 2];
    const v3 d = xf_dir(r0, r1, r2, wd);
    const v3 o = xf_point(r0, r1, r2, wo);
    if (type == 3) {  // sphere
        const float a = vdot(d, d);
        const float b = 2.0f * vdot(d, o);
        const float c = vdot(o, o) - 1.0f;
        const float discr = b * b - 4.0f * a * c;
        if (discr > 0.0f) {
            const float sdiscr = sqrt_cr(discr);
            const float t = div_cr(-b - sdiscr, 2.0f * a);
            if (t > 0.0001f && closer(t, orig, tmin, best)) {
                best.t = t;
                best.pos = pos;
                best.orig = orig;
            }
        }
    } else if (type == 0) {  // cylinder
        const float a = d.x * d.x + d.z * d.z;
        const float b = 2.0f * (o.x * d.x + o.z * d.z);
        const float c = o.x * o.x + o.z * o.z - 1.0f;
        const float discr = b * b - 4.0f * a * c;
        if (discr > 0.001f) {
            const float sdiscr = sqrt_cr(discr);
            const float t0 = div_cr(-b + sdiscr, 2.0f * a);
            const float t1 = div_cr(-b - sdiscr, 2.0f * a);
            float t = 1e16f;
            bool valid = false;
            if (t0 > 0.001f) {
                const float py = o.y + t0 * d.y;
                if (py > -1.0f && py < 1.0f) {
                    t = t0;
                    valid = true;
                }
            }
            if (t1 > 0.001f && t1 < t) {
                const float py = o.y + t1 * d.y;
                if (py > -1.0f && py < 1.0f) {
                    t = t1;
                    valid = true;
                }
            }
            if (valid && closer(t, orig, tmin, best)) {
                best.t = t;
                best.pos = pos;
                best.orig = orig;
            }
        }
    } else {  // disk
        const float divisor = d.y;
        if (!(divisor > 0.0f - 0.01f && divisor < 0.0f + 0.01f)) {
            const float t = div_cr(-o.y, divisor);
            if (t > 0.0001f && closer(t, orig, tmin, best)) {
                const v3 p = vadd(o, vscale(d, t));
                if (vdot(p, p) < 1.0f) {
                    best.t = t;
                    best.pos = pos | kFlat;
                    best.orig = orig;
                }
            }
        }
    }
}

// Two rectangles that the build has put side by side because their normals are opposite (the two faces of a box, floor and
// ceiling, left and right wall).  A rectangle is one-sided: its test starts with d.y < 0 in object space (kernel.cu:394-400),
// and d.y is the ray direction against the world normal, so at most one of the two can get past that first test -- the
// rest of the test then runs once, on whichever it is, instead of twice.  Exactly the tests leaf_test() would make, on the same
// values: when rounding lets BOTH through (a wave-level vote; rare), those lanes run both.
template <bool LIST, typename Ptr>
__device__ __forceinline__ void pair_test(Ptr fp, const float4* __restrict__ lds, int pos, v3 wo, v3 wd, float tmin, FastHit& best)
{
    // fp: where the two normals come from (the up-front list reads them through scalar loads); lds: the LDS copy of the same
    // records, from which each lane then reads the ONE rectangle it goes on with (a per-lane address costs one ds_read; choosing
    // between two rows held in SGPRs costs three VALU instructions per float)
    const float4 r1a = fp[4 * pos + 1], r1b = fp[4 * pos + 5];
    const float dya = r1a.x * wd.x + r1a.y * wd.y + r1a.z * wd.z;
    const float dyb = r1b.x * wd.x + r1b.y * wd.y + r1b.z * wd.z;
    const bool fa = dya < 0.0f, fb = dyb < 0.0f;
    if (__ballot(fa & fb) != 0ull) {
        if (fa & fb) {
            leaf_test(lds, pos, wo, wd, tmin, best);
            leaf_test(lds, pos + 1, wo, wd, tmin, best);
        }
    }
    const int sel = fa ? pos : pos + 1;
    const float4 r1 = LIST ? lds[4 * sel + 1] : make_float4(fa ? r1a.x : r1b.x, fa ? r1a.y : r1b.y, fa ? r1a.z : r1b.z, fa ? r1a.w : r1b.w);
    const int orig = __float_as_int(lds[4 * sel + 3].y);
    rect_commit(lds + 4 * sel, r1, fa ? dya : dyb, fa != fb, sel, orig, wo, wd, tmin, best);
}

// the records [first, first + cnt) of one leaf (or of the up-front list): npairs pairs first, then single primitives
template <bool LIST, bool MASK = false, typename Ptr>
__device__ __forceinline__ void leaf_range(Ptr fp, const float4* __restrict__ lds, int first, int cnt, int npairs, v3 wo, v3 wd, float tmin, FastHit& best)
{
#pragma unroll 1
    for (int k = 0; k < npairs; ++k) pair_test<LIST>(fp, lds, first + 2 * k, wo, wd, tmin, best);
    if (LIST) {
#pragma unroll 2
        for (int k = 2 * npairs; k < cnt; ++k) leaf_test<MASK>(fp, first + k, wo, wd, tmin, best);
    } else {
        for (int k = 2 * npairs; k < cnt; ++k) leaf_test<MASK>(fp, first + k, wo, wd, tmin, best);
    }
}

// Three rectangle pairs that the build has certified as the faces of ONE cuboid -- a box seen from outside (rectangles facing away
// from it: every point of face f lies at or below the plane of every face g of the other two pairs, y_g <= tol in g's object space) or a
// room seen from inside (facing into it: y_g >= -tol).  pair_test's argument says at most one face of a pair is front-facing; this one
// says at most one of the three front-facing faces can be HIT: the point where the ray meets face f's plane has to lie on the inner
// side of the other front-facing planes, or it is outside f's square.  So the first halves of the three tests run as in
// kernel.cu:372-400 (same operations: d.y, o.y, t = -o.y / d.y for the front-facing face of each pair), then a face is dropped when
// that point, o + t_f d, is beyond another front-facing plane by more than `mu` -- y_g(t_f) = o.y_g + t_f d.y_g from the values
// already at hand -- and the second half (the other two rows of M^-1, the unit-square test, kernel.cu:401-414) runs ONCE, on the face
// that is left, instead of three times.  Near an edge two faces can be left: a wave-level vote runs the second half again for those.
// mu covers the certificate's tolerance and the rounding of the reference's u, v and of y_g (rtgo_capi.hip, cub_mu): a face the
// reference accepts is never dropped, and a face that is not dropped gets the reference's whole test, so the closest hit is the same.
// mu_out / mu_in: drop when y > mu_out or y < mu_in (box: (mu, -inf); room: (+inf, -mu)).
// KIND: what the certificate says the cuboid is, where the kernel knows it when it is compiled -- kCubBox (every leaf) compares against
// mu_out alone, kCubRoom (the list of the pair kernels, whose launches vouch for a room) against mu_in alone: one comparison per pair of
// faces, and the margins need not be built per ray.  kCubEither: the list of a kernel that serves both kinds of launch; the kind is in
// the margins, one of which is infinite and never fires -- the same faces dropped, at two comparisons each.
enum CubKind { kCubEither = 0, kCubBox = 1, kCubRoom = 2 };   // (= LaunchParams::list_cub's values)
// MASK: the carrier of the predicates (Pred): a lane's bool, or the wave's lane mask (the pair kernels' ray loop).
template <bool LIST, CubKind KIND, bool MASK = false, typename Ptr>
__device__ __forceinline__ void cuboid_range(Ptr fp, const float4* __restrict__ lds, int first, float mu_out, float mu_in, v3 wo, v3 wd, float tmin, FastHit& best)
{
    typedef Pred<MASK> P;
    float t[3], dy[3];
    typedef typename P::T B;
    B front[3], ok[3], second[3];   // second: the pair's front-facing face is its second record
    int face[3];                    // MASK: ... as the record's position, a lane's word in place of three masks held through the finish loop
    B both = P::off();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int pos = first + 2 * k;
        const float4 r1a = fp[4 * pos + 1], r1b = fp[4 * pos + 5];
        const float dya = r1a.x * wd.x + r1a.y * wd.y + r1a.z * wd.z;
        const float dyb = r1b.x * wd.x + r1b.y * wd.y + r1b.z * wd.z;
        const B fa = P::lt(dya, 0.0f), fb = P::lt(dyb, 0.0f);
        both = both | (fa & fb);
        const int pos_f = P::lane(fa) ? pos : pos + 1;
        if constexpr (MASK) face[k] = pos_f;
        else second[k] = P::inv(fa);
        const float4 r1 = lds[4 * pos_f + 1];   // (a per-lane read of the one row: cheaper than holding both for selects)
        dy[k] = P::lane(fa) ? dya : dyb;
        const float oyk = r1.x * wo.x + r1.y * wo.y + r1.z * wo.z + r1.w;
        t[k] = div_cr(0.0f - oyk, dy[k]);
        front[k] = P::differ(fa, fb);
        ok[k] = front[k] & P::gt(oyk, 0.0f);
        both = both | (front[k] & P::not_lt(fabsf(t[k]), 1e30f));   // (t overflowed: y_g below needs it finite; never seen, handled like `both`)
    }
    // rounding can let both faces of a pair through the sign test (the ray all but parallel to them): those lanes take the six
    // single tests and nothing else
    if (P::any(both)) {
        if (P::lane(both)) {
#pragma unroll 1
            for (int k = 0; k < 6; ++k) leaf_test<MASK>(lds, first + k, wo, wd, tmin, best);
        }
    }
    auto beyond = [&](int f, int g) {
        // y_g at the point where the ray meets f's plane: o.y_g + t_f d.y_g = d.y_g (t_f - t_g) up to 2^-24 of o.y_g (t_g = -o.y_g / d.y_g
        // correctly rounded), which the margin covers -- and three registers fewer than keeping the o.y
        const float y = dy[g] * (t[f] - t[g]);
        if constexpr (KIND == kCubBox) return front[g] & P::gt(y, mu_out);
        else if constexpr (KIND == kCubRoom) return front[g] & P::lt(y, mu_in);
        else return front[g] & (P::gt(y, mu_out) | P::lt(y, mu_in));
    };
    B s0, s1, s2;
    if constexpr (MASK) {   // (`!` is the bool's complement; the mask's is andnot)
        s0 = P::andnot(P::andnot(P::andnot(ok[0], both), beyond(0, 1)), beyond(0, 2));
        s1 = P::andnot(P::andnot(P::andnot(ok[1], both), beyond(1, 0)), beyond(1, 2));
        s2 = P::andnot(P::andnot(P::andnot(ok[2], both), beyond(2, 0)), beyond(2, 1));
    } else {
        s0 = ok[0] & !both & !beyond(0, 1) & !beyond(0, 2);
        s1 = ok[1] & !both & !beyond(1, 0) & !beyond(1, 2);
        s2 = ok[2] & !both & !beyond(2, 0) & !beyond(2, 1);
    }
#pragma unroll 1
    for (;;) {
        const B any = s0 | s1 | s2;
        if (P::none(any)) break;
        const float tt = P::lane(s0) ? t[0] : (P::lane(s1) ? t[1] : t[2]);
        int ps;
        if constexpr (MASK) ps = P::lane(s0) ? face[0] : (P::lane(s1) ? face[1] : face[2]);
        else ps = first + (P::lane(s0) ? (P::lane(second[0]) ? 1 : 0) : (P::lane(s1) ? (P::lane(second[1]) ? 3 : 2) : (P::lane(second[2]) ? 5 : 4)));
        s2 = s2 & (s0 | s1);
        s1 = s1 & s0;
        s0 = P::off();
        const int orig = __float_as_int(lds[4 * ps + 3].y);
        const B c = any & P::gt(tt, 0.0001f) & closer<MASK>(tt, orig, tmin, best);
        rect_finish<MASK>(lds + 4 * ps, tt, c, ps, orig, wo, wd, best);
    }
}

// cuboid_range's successor for a cuboid that also holds the SLAB certificate (rtgo_build.h, slab_certify): in the object frame of the
// group's first face -- rows 0..2 of its record -- the six faces are the planes of one axis-aligned box [lo, hi].  One transform of the
// ray into that frame and a slab test say which face the ray can meet at all -- a box seen from outside: the face of the axis entered
// LAST, on the side the ray comes from; a room seen from inside: the face of the axis left FIRST, on the side the ray goes to -- and
// only that face gets the reference's test (kernel.cu:372-416, through rect_commit: the same operations on the same values as a single
// test, so an accepted hit is bit for bit the reference's).  The frame arithmetic only steers (fused multiply-adds, the hardware
// reciprocal): what it must never do is leave out a face the reference accepts, and the margins see to that.  With mu = the launch's
// cuboid margin (rtgo_capi.hip, cub_mu: the certificate's tolerance plus the rounding of coordinates within the launch's reach) carried
// into frame units by the certificate's rho: the slabs are widened by mu; the plane of axis a is met somewhere in [m - w, m + w], m the
// plane's parameter as computed and w = mu |1 / d_a|; the face is a candidate iff that interval meets the other two widened slabs'
// [entry, exit].  A grazing ray (|1 / d_a| large) makes more candidates, never fewer, and so does a NaN (the compares are the
// complements of "certainly not"); two candidates (near an edge) are tested one after the other.  A ray all but parallel to a pair of
// faces (|d_a| <= the certificate's threshold, 2e-5 of the longest axis row: below that a face's own d.y, from its own matrix, could
// have the other sign) takes the six single tests instead, like cuboid_range's `both` lanes.
// The certificate's numbers ride in the words z, w of row 3 of the group's records: record a (a = 0, 1, 2) the bounds (lo, hi) of frame
// axis a, record 3 (map, rho), record 4 (the parallel threshold, 0).  map: three bits per plane, the face's offset in the group, low
// plane of axis 0 first.
// KIND: kCubBox or kCubRoom (the kernel knows which when it is compiled).  MASK: the predicates' carrier (Pred).
template <bool LIST, CubKind KIND, bool MASK = false, typename Ptr>
__device__ __forceinline__ void cuboid_slab(Ptr fp, const float4* __restrict__ lds, int first, float mu_launch, v3 wo, v3 wd, float tmin, FastHit& best)
{
    static_assert(KIND != kCubEither, "the slab test is compiled for a box or for a room");
    constexpr bool ROOM = KIND == kCubRoom;
    typedef Pred<MASK> P;
    typedef typename P::T B;
    // (the certificate's words: the upper half of a record's row 3)
    auto cert = [&](int rec) { return reinterpret_cast<const float2*>(fp + 4 * rec + 3)[1]; };
    const float2 m3 = cert(first + 3);
    const int map = __float_as_int(m3.x);
    const float mu = mu_launch * m3.y, thr = cert(first + 4).x;
    // per axis two numbers stay: the plane's parameter as computed (box: the entry, room: the exit) and w with the sign of d_a; E, X: the
    // latest entry and the earliest exit over the three widened slabs.  An axis's own entry is never past its own interval and its own
    // exit never before it, so "meets the OTHER slabs" is a compare against E and X themselves.
    float tp[3], ws[3], E = -INFINITY, X = INFINITY;
    B flat = P::off();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float4 r = fp[4 * first + a];
        const float2 m = cert(first + a);
        const float da = fmaf(r.x, wd.x, fmaf(r.y, wd.y, r.z * wd.z));
        const float oa = fmaf(r.x, wo.x, fmaf(r.y, wo.y, fmaf(r.z, wo.z, r.w)));
        flat = flat | P::le(fabsf(da), thr);
        const float ia = __builtin_amdgcn_rcpf(da);
        const float noia = -(oa * ia);
        const float tl = fmaf(m.x, ia, noia), th = fmaf(m.y, ia, noia);
        ws[a] = mu * ia;
        const float tn = fminf(tl, th), tf = fmaxf(tl, th);
        E = fmaxf(E, tn - fabsf(ws[a]));
        X = fminf(X, tf + fabsf(ws[a]));
        tp[a] = ROOM ? tf : tn;
    }
    B s0, s1, s2;
    s0 = P::andnot(P::not_lt(tp[0] + fabsf(ws[0]), E) & P::not_lt(X, tp[0] - fabsf(ws[0])), flat);
    s1 = P::andnot(P::not_lt(tp[1] + fabsf(ws[1]), E) & P::not_lt(X, tp[1] - fabsf(ws[1])), flat);
    s2 = P::andnot(P::not_lt(tp[2] + fabsf(ws[2]), E) & P::not_lt(X, tp[2] - fabsf(ws[2])), flat);
#pragma unroll 1
    for (;;) {
        const B any = s0 | s1 | s2;
        if (P::none(any)) break;
        // the lowest candidate axis, and its plane on the side the ray's sign gives: a box is entered through the side the ray comes from
        // (d_a > 0: the low plane), a room is left through the side it goes to (d_a > 0: the high plane)
        const int sg = __float_as_int(P::lane(s0) ? ws[0] : (P::lane(s1) ? ws[1] : ws[2])) >> 31;   // (-1: d_a < 0)
        const int sh = (P::lane(s0) ? 0 : (P::lane(s1) ? 6 : 12)) + ((ROOM ? ~sg : sg) & 3);
        const int ps = first + ((map >> sh) & 7);
        s2 = s2 & (s0 | s1);
        s1 = s1 & s0;
        s0 = P::off();
        const float4 r1 = lds[4 * ps + 1];
        const int orig = __float_as_int(lds[4 * ps + 3].y);
        const float dy = r1.x * wd.x + r1.y * wd.y + r1.z * wd.z;
        rect_commit<MASK>(lds + 4 * ps, r1, dy, any & P::lt(dy, 0.0f), ps, orig, wo, wd, tmin, best);
    }
    // (last, so that nothing but the mask lives across it: the closest hit does not depend on the order of the tests, closer())
    // (the six records are rectangles, or the group held no cuboid certificate: leaf_test's rectangle branch on each)
    if (P::any(flat)) {
#pragma unroll 1
        for (int k = 0; k < 6; ++k) {
            const int ps = first + k;
            const float4 r1 = lds[4 * ps + 1];
            const int orig = __float_as_int(lds[4 * ps + 3].y);
            const float dy = r1.x * wd.x + r1.y * wd.y + r1.z * wd.z;
            rect_commit<MASK>(lds + 4 * ps, r1, dy, flat & P::lt(dy, 0.0f), ps, orig, wo, wd, tmin, best);
        }
    }
}

// What a ROOMW walk hands from closest_hit_fast to the list and to fast_pair: the launch's words and the ray's reciprocals.
struct RoomRay {
    const PairWords* words;
    v3 id, noid;
};
// cuboid_slab<true, kCubRoom> for a room whose slab certificate also holds in WORLD axes (rtgo_room_world.h: the frame rows of the room's
// first face are s e_j plus a residue the margin covers), so that the steering needs no transform and no reciprocal of its own: id and
// noid are the walk's (closest_hit_fast), the planes and the margin arrive in world units through PairWords.  A room needs no entry side:
// the candidate is the face of the axis left first, and leaving the compare against the latest entry out can only add candidates.  Per
// axis: the parallel threshold, the exit as two fma and a max, w = mu id, the earliest exit X, and "not certainly past X".  The side is
// the sign of id (w carries it); the candidate loop, the flat lanes and the compare sense (a NaN makes candidates) are cuboid_slab's,
// and the chosen face gets the reference's whole test through rect_commit: the bits are made there, this only steers.
template <bool MASK>
__device__ __forceinline__ void room_world(const RoomRay& rr, const float4* __restrict__ lds, int first, v3 wo, v3 wd, float tmin, FastHit& best)
{
    typedef Pred<MASK> P;
    typedef typename P::T B;
    const PairWords& rw = *rr.words;
    const v3 id = rr.id, noid = rr.noid;
    const int map = rw.room_map;
    const float mu = rw.room_mu, thr = rw.room_thr;
    const float dd[3] = {wd.x, wd.y, wd.z}, ii[3] = {id.x, id.y, id.z}, nn[3] = {noid.x, noid.y, noid.z};
    float tp[3], ws[3], X = INFINITY;
    B flat = P::off();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        flat = flat | P::le(fabsf(dd[a]), thr);
        tp[a] = fmaxf(fmaf(rw.room_lo[a], ii[a], nn[a]), fmaf(rw.room_hi[a], ii[a], nn[a]));
        ws[a] = mu * ii[a];
        X = fminf(X, tp[a] + fabsf(ws[a]));
    }
    B s0, s1, s2;
    s0 = P::andnot(P::not_lt(X, tp[0] - fabsf(ws[0])), flat);
    s1 = P::andnot(P::not_lt(X, tp[1] - fabsf(ws[1])), flat);
    s2 = P::andnot(P::not_lt(X, tp[2] - fabsf(ws[2])), flat);
#pragma unroll 1
    for (;;) {
        const B any = s0 | s1 | s2;
        if (P::none(any)) break;
        // the lowest candidate axis; a room is left through the side the ray goes to (d_j > 0: the high plane)
        const int sg = __float_as_int(P::lane(s0) ? ws[0] : (P::lane(s1) ? ws[1] : ws[2])) >> 31;   // (-1: d_j < 0)
        const int sh = (P::lane(s0) ? 0 : (P::lane(s1) ? 6 : 12)) + (~sg & 3);
        const int ps = first + ((map >> sh) & 7);
        s2 = s2 & (s0 | s1);
        s1 = s1 & s0;
        s0 = P::off();
        const float4 r1 = lds[4 * ps + 1];
        const int orig = __float_as_int(lds[4 * ps + 3].y);
        const float dy = r1.x * wd.x + r1.y * wd.y + r1.z * wd.z;
        rect_commit<MASK>(lds + 4 * ps, r1, dy, any & P::lt(dy, 0.0f), ps, orig, wo, wd, tmin, best);
    }
    if (P::any(flat)) {
#pragma unroll 1
        for (int k = 0; k < 6; ++k) {
            const int ps = first + k;
            const float4 r1 = lds[4 * ps + 1];
            const int orig = __float_as_int(lds[4 * ps + 3].y);
            const float dy = r1.x * wd.x + r1.y * wd.y + r1.z * wd.z;
            rect_commit<MASK>(lds + 4 * ps, r1, dy, flat & P::lt(dy, 0.0f), ps, orig, wo, wd, tmin, best);
        }
    }
}

// conservative slab test: t = fma(b, 1/d, -o/d) with the hardware reciprocal
template <bool MASK = false>
__device__ __forceinline__ typename Pred<MASK>::T box_fast(const float4 q0, const float4 q1, v3 id, v3 noid, float tmin, float tmax, float& tn_out)
{
    float t0 = fmaf(q0.x, id.x, noid.x), t1 = fmaf(q1.x, id.x, noid.x);
    float tn = fminf(t0, t1), tf = fmaxf(t0, t1);
    t0 = fmaf(q0.y, id.y, noid.y);
    t1 = fmaf(q1.y, id.y, noid.y);
    tn = fmaxf(tn, fminf(t0, t1));
    tf = fminf(tf, fmaxf(t0, t1));
    t0 = fmaf(q0.z, id.z, noid.z);
    t1 = fmaf(q1.z, id.z, noid.z);
    tn = fmaxf(tn, fminf(t0, t1));
    tf = fminf(tf, fmaxf(t0, t1));
    tn = fmaxf(tn, tmin);
    tf = fminf(tf, tmax);
    tn_out = tn;
#ifdef RTGO_NO_WIDEN
    return Pred<MASK>::le(tn, tf);
#else
    // widen by a few ulps so that the reciprocal's rounding can never drop a box the exact test keeps
    return Pred<MASK>::le(tn, tf * 1.000002f + 1e-7f);
#endif
}


// The fast walk in three parts (closest_hit_fast below runs them back to back; an experiment of round 2 ran the middle one in another
// lane than the other two: profiles/r02f/README.md).  fast_list: the up-front list, which also gives the ray its first closest-hit bound.
// LAST, `last`: the lane's ray is the last of its path under the last-ray certificate (closest_hit_fast): it skips the room.
// KIND: kCubRoom when the launch vouches for a list that starts with a certified room (the pair kernels), else kCubEither (list_cub says).
// ROOMW: the room's steering is the world-axis form (room_world) on the walk's id and noid, which `rr` holds with the launch's words.
template <bool LAST = false, CubKind KIND = kCubEither, bool MASK = false, bool SLAB = false, bool ROOMW = false>
__device__ __forceinline__ void fast_list(const float4* __restrict__ s_fprims, const float4* __restrict__ g_fprims, int n_small, int n_prims, int n_big_pairs,
                                          int list_cub, float cub_mu, v3 o, v3 d, float tmin, FastHit& best, typename Pred<MASK>::T last = Pred<MASK>::off(),
                                          const RoomRay* rr = nullptr)
{
    static_assert(!ROOMW || (SLAB && KIND == kCubRoom), "the world form replaces the slab test of a room");
    // the few "big" primitives (walls, floors; the whole scene when it is tiny) first.  The loop index is wave-uniform and
    // g_fprims is a read-only kernel argument, so the records arrive by scalar loads (s_load_dwordx4) into SGPRs: no LDS
    // traffic, no VGPRs for the matrices, and the loads of the next primitives overlap the tests of the current ones.
    // It also gives every ray a closest-hit bound before it enters the tree.
    if (KIND != kCubEither || list_cub != 0) {
        // the room's six walls (or one big box) as a cuboid, the rest of the list after them
        if (!LAST || Pred<MASK>::any(Pred<MASK>::inv(last))) {
            const bool box = KIND == kCubEither && list_cub == 1;
            if constexpr (ROOMW) {
                if (!LAST || Pred<MASK>::lane(Pred<MASK>::inv(last))) room_world<MASK>(*rr, s_fprims, n_small, o, d, tmin, best);
            } else if constexpr (SLAB) {
                if (!LAST || Pred<MASK>::lane(Pred<MASK>::inv(last))) cuboid_slab<true, KIND, MASK>(g_fprims, s_fprims, n_small, cub_mu, o, d, tmin, best);
            } else if (!LAST || Pred<MASK>::lane(Pred<MASK>::inv(last))) cuboid_range<true, KIND, MASK>(g_fprims, s_fprims, n_small, box ? cub_mu : INFINITY, box ? -INFINITY : -cub_mu, o, d, tmin, best);
        }
        leaf_range<true, MASK>(g_fprims, s_fprims, n_small + 6, n_prims - n_small - 6, 0, o, d, tmin, best);
    } else {
        leaf_range<true>(g_fprims, s_fprims, n_small, n_prims - n_small, n_big_pairs, o, d, tmin, best);
    }
}

// A leaf of a tree that holds nothing but spheres (a scene-wide fact the build reports): __intersection__sphere (kernel.cu:250-287)
// without the per-lane dispatch on the primitive's type that leaf_test opens with -- three exec-masked regions per leaf phase that
// a wave of sphere leaves walks through for nothing
__device__ __forceinline__ void sphere_leaf(const float4* __restrict__ s_fprims, int first, int cnt, v3 wo, v3 wd, float tmin, FastHit& best)
{
    for (int k = 0; k < cnt; ++k) {
        const int pos = first + k;
        const float4 r0 = s_fprims[4 * pos + 0], r1 = s_fprims[4 * pos + 1], r2 = s_fprims[4 * pos + 2];
        const int orig = __float_as_int(s_fprims[4 * pos + 3].y);
        const v3 d = xf_dir(r0, r1, r2, wd);
        const v3 o = xf_point(r0, r1, r2, wo);
        const float a = vdot(d, d);
        const float b = 2.0f * vdot(d, o);
        const float c = vdot(o, o) - 1.0f;
        const float discr = b * b - 4.0f * a * c;
        if (discr > 0.0f) {
            const float sdiscr = sqrt_cr(discr);
            const float t = div_cr(-b - sdiscr, 2.0f * a);
            if (t > 0.0001f && closer(t, orig, tmin, best)) {
                best.t = t;
                best.pos = pos;
                best.orig = orig;
            }
        }
    }
}

// fast_tree: the walk proper -- everything in the tree that can beat `best`
__device__ __forceinline__ void fast_tree(const float4* __restrict__ s_fnodes, const float4* __restrict__ s_fprims, unsigned int* __restrict__ s_stack, int bshift,
                                          int n_small, float cub_mu, v3 o, v3 d, float tmin, FastHit& best, unsigned int& dbg_boxes, unsigned int& dbg_tests, bool tree_spheres)
{
    // 1/d for the slab tests.  A direction component that is exactly zero is not rare: the hemisphere sample has sin(phi) = 0
    // whenever its random number is 0 (one ray in 2^24 per bounce, a few per 1080p frame), and cameras can be axis-aligned.
    // rcp(0) = inf would turn fma(b, 1/d, -o/d) into inf - inf = NaN on one side of the origin and -inf on the other, and a
    // box straddling zero would be dropped; a huge FINITE reciprocal keeps both products finite and the slab's sign logic
    // intact (inside: (-huge, +huge); outside: both ends on one side).
    auto safe_rcp = [](float x) { return __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(x), -1e30f, 1e30f); };   // (rcp(+-0) = +-inf and anything beyond 1e30 end up at +-1e30)
    const v3 id = mk(safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z));
    const v3 noid = mk(-(o.x * id.x), -(o.y * id.y), -(o.z * id.z));
    float tn;
    float4 q0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q1 = q0;
    bool have = n_small > 0;
    if (have) {
        q0 = s_fnodes[0];
        q1 = s_fnodes[1];
        have = box_fast(q0, q1, id, noid, tmin, best.t, tn);
    }
    int left = __float_as_int(q0.w), right = __float_as_int(q1.w);
    int sp = 0;
    // A stack entry is ONE word: the far child's entry distance cut to its upper 16 bits (toward zero: a lower bound of a
    // positive number, so culling at pop time stays conservative) | its node index (< 2 * kMaxPrims).
    auto pop = [&]() -> bool {
        while (sp > 0) {
            --sp;
            const unsigned int e = s_stack[sp << bshift];
            if (__uint_as_float(e & 0xFFFF0000u) <= best.t) {
                const int idx = (int)(e & 0xFFFFu);
                left = __float_as_int(s_fnodes[2 * idx].w);
                right = __float_as_int(s_fnodes[2 * idx + 1].w);
                return true;
            }
        }
        return false;
    };
    while (have) {
        while (have && right >= 0) {
            const float4 l0 = s_fnodes[2 * left], l1 = s_fnodes[2 * left + 1];
            const float4 h0 = s_fnodes[2 * right], h1 = s_fnodes[2 * right + 1];
            float tl, tr;
            FastCounters::step(dbg_boxes, 2u);
            const bool hl = box_fast(l0, l1, id, noid, tmin, best.t, tl);
            const bool hr = box_fast(h0, h1, id, noid, tmin, best.t, tr);
            // the step as selects: go to the right child when only it is hit, or when both are and it is nearer; the other one
            // of two hit children waits on the stack
            const bool go_r = hr & (!hl | (tr < tl));
            // (the entry is written whether or not it is needed -- the slot past the top is scratch: the launch allots one entry more -- and
            // only the stack pointer depends on the vote: one exec-masked region less per step; balls -1.7 %, checkered -1.3 %)
            s_stack[sp << bshift] = (__float_as_uint(go_r ? tl : tr) & 0xFFFF0000u) | (unsigned int)(go_r ? left : right);
            sp += (hl & hr) ? 1 : 0;
            if (hl | hr) {
                left = __float_as_int(go_r ? h0.w : l0.w);
                right = __float_as_int(go_r ? h1.w : l1.w);
            } else {
                have = pop();
            }
        }
        if (have) {
            const int first = left, cnt = leaf_count(right), npairs = leaf_pairs(right);
            FastCounters::step(dbg_tests, (unsigned int)cnt);
            if (tree_spheres) sphere_leaf(s_fprims, first, cnt, o, d, tmin, best);
            else if (leaf_cuboid(right) != 0 && cub_mu > 0.0f) cuboid_range<false, kCubBox>(s_fprims, s_fprims, first, cub_mu, -INFINITY, o, d, tmin, best);
            else leaf_range<false>(s_fprims, s_fprims, first, cnt, npairs, o, d, tmin, best);
            have = pop();
        }
    }
}

// fast_pair: fast_tree over a tree that is a root (node 0) over two leaves (nodes 1 and 2), both certified cuboids -- cornell's two boxes;
// the launch vouches for that shape (rtgo_capi.hip, FastTree::pair) -- as straight-line code.  The same leaf tests on the same values for
// every lane: both child boxes against the list's closest hit, the nearer hit child's leaf (go_r, as fast_tree steps), then the other
// one's for the lanes that hit both boxes and whose far entry distance, cut to its upper 16 bits like fast_tree's stack word, is still
// <= the closest hit.  What is gone is the machinery of a deep tree: the root's own box test (the root box is the union of the two, and
// fma(q, id, noid) is monotone in q: a lane that passes a child's slab test passes the root's), the while-while loop, the stack word
// in LDS, the pop loop with its dependent reads of a node's links, and the leaf's dispatch on tree_spheres / leaf_cuboid / cub_mu.
// HAVEID: the caller made id and noid, by these same operations, for the list's room test and hands them over in `rr` (ROOMW, closest_hit_fast).
template <bool MASK, bool SLAB = false, bool HAVEID = false>
__device__ __forceinline__ void fast_pair(const float4* __restrict__ s_fnodes, const float4* __restrict__ s_fprims, float cub_mu, v3 o, v3 d, float tmin, FastHit& best,
                                          unsigned int& dbg_boxes, unsigned int& dbg_tests, const RoomRay* rr = nullptr)
{
    typedef Pred<MASK> P;
    auto safe_rcp = [](float x) { return __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(x), -1e30f, 1e30f); };   // (see fast_tree on 1 / 0)
    const v3 id = HAVEID ? rr->id : mk(safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z));
    const v3 noid = HAVEID ? rr->noid : mk(-(o.x * id.x), -(o.y * id.y), -(o.z * id.z));
    // (wave-uniform addresses: four reads under one wait; a leaf's first record comes with its box)
    const float4 l0 = s_fnodes[2], l1 = s_fnodes[3], h0 = s_fnodes[4], h1 = s_fnodes[5];
    float tl, tr;
    FastCounters::step(dbg_boxes, 2u);
    typedef typename P::T B;
    const B hl = box_fast<MASK>(l0, l1, id, noid, tmin, best.t, tl);
    const B hr = box_fast<MASK>(h0, h1, id, noid, tmin, best.t, tr);
    const B go_r = hr & (P::inv(hl) | P::lt(tr, tl));
    // (what the far leaf needs is picked per lane before the near leaf runs: two words and one mask live across it, not three masks and the boxes)
    const bool right = P::lane(go_r);
    const B two = hl & hr;
    const float t_far = __uint_as_float(__float_as_uint(right ? tl : tr) & 0xFFFF0000u);
    const int first_far = __float_as_int(right ? l0.w : h0.w);
    const unsigned int count_far = (unsigned int)leaf_count(__float_as_int(right ? l1.w : h1.w));
    if (P::lane(hl | hr)) {
        FastCounters::step(dbg_tests, (unsigned int)leaf_count(__float_as_int(right ? h1.w : l1.w)));
        // (the near leaf keeps the bool carrier: as masks its predicates cost render_pair7_kernel ten more SGPR spills than its budget has)
        // (cuboid_slab's predicates fit the seven-waves budget as masks here too: 3 SGPR spills in render_slab7_kernel, none in the ray loop)
        if constexpr (SLAB) cuboid_slab<false, kCubBox, MASK>(s_fprims, s_fprims, __float_as_int(right ? h0.w : l0.w), cub_mu, o, d, tmin, best);
        else cuboid_range<false, kCubBox, false>(s_fprims, s_fprims, __float_as_int(right ? h0.w : l0.w), cub_mu, -INFINITY, o, d, tmin, best);
    }
    const B far = two & P::le(t_far, best.t);
    if (P::any(far)) {
        if (P::lane(far)) {
            FastCounters::step(dbg_tests, count_far);
            if constexpr (SLAB) cuboid_slab<false, kCubBox, MASK>(s_fprims, s_fprims, first_far, cub_mu, o, d, tmin, best);
            else cuboid_range<false, kCubBox, MASK>(s_fprims, s_fprims, first_far, cub_mu, -INFINITY, o, d, tmin, best);
        }
    }
}

// fast_grid: the same job as fast_tree over a uniform grid (Amanatides & Woo's walk, one lane = one ray).  The host bins every small
// primitive into the cells its box -- grown by a pad that is far above the rounding of the walk -- overlaps; a lane steps from cell to
// cell along its ray, tests what the cell lists through the same leaf tests as the tree (so an accepted hit is the tree's and the
// canonical walk's, bit for bit; a primitive met again in the next cell changes nothing: closer() is strict), and stops once its closest
// hit lies before the exit of the cell it is in (everything that could beat it is listed in a cell already visited).  No stack, no box
// tests: ~20 vector instructions per cell where the tree pays ~50 per node pair; scenes of many small, evenly spread primitives (balls).
__device__ __forceinline__ void fast_grid(const float4* __restrict__ s_grid, const float4* __restrict__ s_fprims, const GridParams g, bool spheres,
                                          v3 o, v3 d, float tmin, FastHit& best, unsigned int& dbg_boxes, unsigned int& dbg_tests)
{
    // (everything of `g` into scalars first: it is wave-uniform, and a struct member read inside the loop through a reference went to scratch)
    const float gx = g.min_x, gy = g.min_y, gz = g.min_z, csx = g.cs_x, csy = g.cs_y, csz = g.cs_z, margin = g.margin;
    const int nx = g.nx, ny = g.ny, nz = g.nz, n_cells = g.n_cells;
    // the table: one word per cell, 0 = lists nothing, else 1 + the index of the cell's record = two float4: the box around everything the
    // cell lists (min.xyz | first item + count << 16, max.xyz | 0); then the items, 16-bit positions into fprims
    const unsigned int* __restrict__ cells = reinterpret_cast<const unsigned int*>(s_grid);
    const float4* __restrict__ recs = s_grid + g.rec_off4;
    const unsigned short* __restrict__ items = reinterpret_cast<const unsigned short*>(s_grid + g.items_off4);
    const float idx = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(d.x), -1e30f, 1e30f);   // (see fast_tree on 1 / 0)
    const float idy = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(d.y), -1e30f, 1e30f);
    const float idz = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(d.z), -1e30f, 1e30f);
    // the ray's stretch inside the grid's bounds
    float t0 = tmin, t1 = best.t;
    {
        const float ax = (gx - o.x) * idx, bx = (gx + csx * (float)nx - o.x) * idx;
        const float ay = (gy - o.y) * idy, by = (gy + csy * (float)ny - o.y) * idy;
        const float az = (gz - o.z) * idz, bz = (gz + csz * (float)nz - o.z) * idz;
        t0 = fmaxf(fmaxf(t0, fminf(ax, bx)), fmaxf(fminf(ay, by), fminf(az, bz)));
        t1 = fminf(fminf(t1, fmaxf(ax, bx)), fminf(fmaxf(ay, by), fmaxf(az, bz)));
    }
    bool live = (n_cells > 0) & (t0 <= t1 * 1.000002f + margin);
    // the cell of the entry point (clamped: the point may sit a rounding outside), the parameter at which the ray leaves it on each
    // axis and the parameter per cell.  The table has a border of empty cells around the nx x ny x nz that list something: the step
    // out of the grid lands there and the walk ends on the parameter test alone, without a count of cells per axis (a ray leaves through
    // a face, an edge or a corner: at most one step per axis beyond t1, all inside the border).
    const int cx = min(max((int)floorf((o.x + d.x * t0 - gx) * g.ics_x), 0), nx - 1);
    const int cy = min(max((int)floorf((o.y + d.y * t0 - gy) * g.ics_y), 0), ny - 1);
    const int cz = min(max((int)floorf((o.z + d.z * t0 - gz) * g.ics_z), 0), nz - 1);
    const bool fx = idx >= 0.0f, fy = idy >= 0.0f, fz = idz >= 0.0f;
    float tmx = (gx + csx * (float)(cx + (fx ? 1 : 0)) - o.x) * idx;
    float tmy = (gy + csy * (float)(cy + (fy ? 1 : 0)) - o.y) * idy;
    float tmz = (gz + csz * (float)(cz + (fz ? 1 : 0)) - o.z) * idz;
    const float tdx = csx * fabsf(idx), tdy = csy * fabsf(idy), tdz = csz * fabsf(idz);
    const int NX = nx + 2, NXY = NX * (ny + 2);
    const int sx = fx ? 1 : -1, sy = fy ? NX : -NX, sz = fz ? NXY : -NXY;
    int cell = (cz + 1) * NXY + (cy + 1) * NX + cx + 1;
    // A ray this walk cannot take -- an infinite or NaN component (its reciprocal, and with it the parameter per cell, is zero or no number:
    // te would never grow), or a direction so long that a cell is crossed in less than the margin (the border argument above needs
    // td > margin) -- is dropped here, once (1.4 % of balls' frame; a range test per step cost 4 %): every step then adds a positive td to the
    // parameter it compares, so the loop ends, and it ends inside the table.  Such rays only exist where the arithmetic has broken down
    // (far beyond the far-field guard, where the launch walks the canonical tree anyway).
    live = live & (tdx > 2.0f * margin) & (tdy > 2.0f * margin) & (tdz > 2.0f * margin) & (fabsf(tmx + tmy + tmz) < 3e38f);
    float tstop = fminf(best.t, t1) + margin;   // the walk goes on while the current cell's exit lies before this
    int last = -1;                              // the record tested last: a shape that straddles two cells along the ray is listed in both
    // A lane stops at a cell only when its ray meets the box around what the cell lists (the conservative slab test of the tree walk):
    // a sphere fills a tenth of its cell, and every stop is a test phase in which the lanes that did not stop wait.
    const v3 id = mk(idx, idy, idz);
    const v3 noid = mk(-(o.x * idx), -(o.y * idy), -(o.z * idz));
    unsigned int fc = 0u;                       // first item | count << 16 of the cell this lane has stopped at, 0 = it has not
    auto look = [&]() {
        const unsigned int c = cells[cell];
        if (c != 0u) {
            const float4 q0 = recs[2u * c - 2u], q1 = recs[2u * c - 1u];
            float tn;
            fc = box_fast(q0, q1, id, noid, tmin, best.t, tn) ? __float_as_uint(q0.w) : 0u;
        }
    };
    if (live) look();
    while (live) {
        // to the next cell that lists something in the ray's way: out of the current one through the nearest of its three far planes
        while (live && fc == 0u) {
            FastCounters::step(dbg_boxes, 1u);
            const bool ux = (tmx <= tmy) & (tmx <= tmz), uy = !ux & (tmy <= tmz);
            const float te = ux ? tmx : (uy ? tmy : tmz);
            live = te <= tstop;
            tmx += ux ? tdx : 0.0f;
            tmy += uy ? tdy : 0.0f;
            tmz += (ux | uy) ? 0.0f : tdz;
            cell += ux ? sx : (uy ? sy : sz);
            if (live) look();
        }
        if (live) {
            const int first = (int)(fc & 0xFFFFu), cnt = (int)(fc >> 16);
            for (int k = 0; k < cnt; ++k) {
                const int pos = (int)items[first + k];
                FastCounters::wave_only(dbg_tests);
                if (pos != last) {
                    FastCounters::lane_only(dbg_tests, 1u);
                    if (spheres) sphere_leaf(s_fprims, pos, 1, o, d, tmin, best);
                    else leaf_test(s_fprims, pos, o, d, tmin, best);
                }
                last = pos;
            }
            tstop = fminf(best.t, t1) + margin;
            fc = 0u;   // (back into the stepping loop)
        }
    }
}

// fast_winner: the closest hit's record for the closest-hit program (t, SBT index, world normal)
__device__ __forceinline__ bool fast_winner(const float4* __restrict__ s_fprims, v3 o, v3 d, float tmax, const FastHit& best, Hit& out)
{
    out.prim = -1;
    out.t = tmax;
    out.n = mk(0.0f, 0.0f, 0.0f);
    if (best.pos < 0) return false;
    const int wpos = best.pos & (kFlat - 1);
    const bool flat = (best.pos & kFlat) != 0;
    const float4 r0 = s_fprims[4 * wpos + 0], r1 = s_fprims[4 * wpos + 1], r2 = s_fprims[4 * wpos + 2];
    out.t = best.t;
    // the object-space normal of the winner only (kernel.cu:270 sphere, :315 cylinder, :345/:388 disk and rectangle), from the same
    // object-space ray and the same t as its test: candidates that were overtaken never needed one
    v3 nobj = mk(0.0f, 1.0f, 0.0f);
    if (!flat) {
        const v3 od = xf_dir(r0, r1, r2, d);
        const v3 oo = xf_point(r0, r1, r2, o);
        const bool sphere = __float_as_int(s_fprims[4 * wpos + 3].x) == 3;
        const v3 at = sphere ? vadd(oo, vscale(od, best.t)) : mk(oo.x + best.t * od.x, 0.0f, oo.z + best.t * od.z);
        nobj = sphere ? vnormalize(at) : at;
    }
    out.n = xf_normal(r0, r1, r2, nobj);   // (flat winners: the closest-hit code takes the primitive's precomputed frame instead and this is dead code there)
    out.prim = best.orig;
    return true;
}

// `last`: this lane traces the last ray of its path under the last-ray certificate (LaunchParams::emit_n).  Only an emitter can make
// that ray's payload nonzero, and the certificate shows that no wall of the room can be met before an emitter.  So the lane skips the
// room (fast_list), tests the emitters as the list always does, and, when it hits none, is done: no hit, payload = the background (+0,
// like the term of a non-emitter hit).  When it hits one, the tree walks from `best` = that hit: the closest hit does not depend on the
// order in which candidates are met (closer()).  LAST: the instantiation has this path at all (else `last` is ignored).
// PAIR (render_pair_kernel): the tree is a root over two cuboid leaves, walked by fast_pair.
// MASK: the carrier of `last` and of the walk's predicates from here down (Pred); the pair kernels' ray loop alone sets it.
// ROOMW (render_roomw_kernel): the list's room takes the world-axis form on id and noid, made here once for it and for fast_pair; `rw`: its words.
template <bool GRID, bool LAST = false, bool PAIR = false, bool MASK = false, bool SLAB = false, bool ROOMW = false>
__device__ __forceinline__ bool closest_hit_fast(const float4* __restrict__ s_fnodes, const float4* __restrict__ s_fprims,
                                                 const float4* __restrict__ g_fprims, const GridParams grid,
 unsigned int* __restrict__ s_stack, int bshift,
                                                 int n_small, int n_prims, int n_big_pairs, int list_cub, float cub_mu, bool tree_spheres, v3 o, v3 d, float tmin, float tmax, Hit& out,
                                                 unsigned int& dbg_boxes, unsigned int& dbg_tests, typename Pred<MASK>::T last, Timeline& tl, const PairWords* rw)
{
    static_assert(!MASK || PAIR, "the lane-mask predicates are the pair kernels'");
    static_assert(!ROOMW || (PAIR && SLAB), "the world-axis room serves the slab launches of the pair kernels");
    static_assert(!SLAB || PAIR, "the slab test serves the pair kernels' launches");
    tl.walk_begin();
    FastHit best;
    best.t = tmax;
    best.pos = -1;
    best.orig = -1;
    if constexpr (ROOMW) {
        // (1 / d and -o / d as fast_pair makes them, see fast_tree on 1 / 0: made once, before the list, for the room and for the two boxes)
        auto safe_rcp = [](float x) { return __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(x), -1e30f, 1e30f); };
        RoomRay rr;
        rr.words = rw;
        rr.id = mk(safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z));
        rr.noid = mk(-(o.x * rr.id.x), -(o.y * rr.id.y), -(o.z * rr.id.z));
        fast_list<LAST, kCubRoom, MASK, SLAB, true>(s_fprims, g_fprims, n_small, n_prims, n_big_pairs, list_cub, cub_mu, o, d, tmin, best, last, &rr);
        const bool walk = Pred<MASK>::lane(Pred<MASK>::either(Pred<MASK>::inv(last), Pred<MASK>::ige(best.pos, 0)));
        FastCounters::lane_only(dbg_tests, (unsigned int)(n_prims - n_small - (Pred<MASK>::lane(last) ? 6 : 0)));
        tl.list_done(best.pos);
        if (!LAST || walk) fast_pair<MASK, SLAB, true>(s_fnodes, s_fprims, cub_mu, o, d, tmin, best, dbg_boxes, dbg_tests, &rr);
        tl.walk_done(best.pos);
        return fast_winner(s_fprims, o, d, tmax, best, out);
    }
    fast_list<LAST, PAIR ? kCubRoom : kCubEither, MASK, SLAB>(s_fprims, g_fprims, n_small, n_prims, n_big_pairs, list_cub, cub_mu, o, d, tmin, best, last);
    const bool walk = Pred<MASK>::lane(Pred<MASK>::either(Pred<MASK>::inv(last), Pred<MASK>::ige(best.pos, 0)));
    FastCounters::lane_only(dbg_tests, (unsigned int)(n_prims - n_small - (Pred<MASK>::lane(last) ? 6 : 0)));
    tl.list_done(best.pos);
    if constexpr (GRID) fast_grid(s_fnodes, s_fprims, grid, tree_spheres, o, d, tmin, best, dbg_boxes, dbg_tests);
    else if constexpr (PAIR) {
        if (!LAST || walk) fast_pair<MASK, SLAB>(s_fnodes, s_fprims, cub_mu, o, d, tmin, best, dbg_boxes, dbg_tests);
    } else if (!LAST || walk) fast_tree(s_fnodes, s_fprims, s_stack, bshift, n_small, cub_mu, o, d, tmin, best, dbg_boxes, dbg_tests, tree_spheres);
    tl.walk_done(best.pos);
    return fast_winner(s_fprims, o, d, tmax, best, out);
}

// acos(pow(base, expo)) with both steps in f64, each rounded to float like the reference's float calls.  Kept out of line:
// the f64 libm bodies need ~80 VGPRs that would otherwise be charged to every wave of the megakernel.
__device__ __attribute__((noinline)) float glossy_theta(float base, float expo)
{
    // x^e as exp(e * log x): each f64 call is good to ~1e-16 relative, |e log x| < 20, so the product carries ~1e-14 -- far
    // inside the 3e-8 half-ulp of the float it is rounded to, at about half the cost of the extended-precision f64 pow
    const float c = (float)exp((double)expo * log((double)base));
    return (float)acos((double)c);
}

// GetRayOnHemisphere, kernel.cu:101-122
// UNIT_DIR: the caller's `direction` is a unit vector already (a normalised normal): kernel.cu:103 normalises it again, which moves it by
// an ulp at most; the default build takes it as it is.
// Diffuse lobe (coefficient 0: every path-mode bounce, kernel.cu:467): theta = acos(1 - r2) and then cos(theta), sin(theta) -- i.e.
// cos = 1 - r2 (exact in float: r2 = k / 2^24) and sin = sqrt(r2 (2 - r2)), each within an ulp or two of what acosf / sinf / cosf
// return, for a fifth of the instructions.  Both are inside the tolerance the contract states (1e-4 on >= 99 % of the pixels;
// the reference's own build is --use_fast_math, CMakeLists.txt:165-170); the oracle keeps the libm calls.  Both walks share this code,
// so fast == canonical stays bit for bit.  -DRTGO_LITERAL_SHADING: the literal forms (acosf, the second normalisation), as in round 2.
// LEAN is set by path mode only: a diffuse bounce forgets the incoming direction, so an ulp in the hit point stays an ulp.  Distributed
// mode keeps the literal forms: its mirror and glossy bounces off small spheres multiply a direction's last bit by ~2 d / r per bounce
// (balls: 3.5 % of the pixels of a 96 x 64 frame left the tolerance when it ran lean, profiles/r03c).
// have_x / Xpre: the tangent X of this direction is known already (a flat primitive's frame from build_kernel, bit for bit the value
// computed here): lanes that have it skip the normalisation (a wave vote skips it altogether when every lane has).
constexpr int kHemisphereMaxTries = 1024;   // (= ORACLE_HEMISPHERE_MAX_TRIES)
template <bool LEAN_IN>
__device__ __forceinline__ v3 hemisphere(v3 normal, v3 direction, float coefficient, unsigned int& seed, bool have_x = false, v3 Xpre = v3{0.0f, 0.0f, 0.0f})
{
    v3 ray;
#ifdef RTGO_LITERAL_SHADING
    constexpr bool LEAN = false;
#else
    constexpr bool LEAN = LEAN_IN;
#endif
    const v3 Y = LEAN ? direction : vnormalize(direction);   // (lean callers pass a unit vector: a normalised normal)
    v3 X;
    if (have_x) X = Xpre;   // (wave-uniform: LaunchParams::all_flat)
    else X = vnormalize(mk(Y.y - Y.z, -Y.x, Y.x));
    const v3 Z = vcross(Y, X);
    const float expo = div_cr(1.f, coefficient + 1.f);
    // The reference's rejection loop (kernel.cu:109-120) is unbounded, and it never ends when the lobe lies wholly below the horizon of
    // `normal`: kernel.cu:443-447 flips N by V = normalize(origin - x), which is rounding noise when t is tiny against the coordinates, and
    // Rr = reflect about a wrongly flipped N (:508-510) points into the surface -- a mirror's lobe around it never passes the test and the
    // launch hangs the GPU (tools/fuzz_farfield.py, random scene 45 seen 270 units off the origin).  kHemisphereMaxTries draws, then the
    // last one stands; the oracle does the same, and wherever the reference's loop ends within that many draws nothing changes.
    int tries = 0;
    do {
        const float r1 = rnd(seed);
        const float r2 = rnd(seed);
        const float phi = 2.f * kPi * r1;
        const float base = 1.f - r2;
        float st, ct, sp, cp;
        if (LEAN && expo == 1.0f) {
            ct = base;
            st = sqrt_cr(r2 * (1.0f + base));
        } else {
            float theta;
            if (expo == 1.0f) {
                // diffuse lobe: powf(x, 1) == x exactly in any sound libm
                theta = acosf(base);
            } else if (expo == 0.5f) {
                // specularity 1 (every cornell surface in distributed mode): pow(x, 1/2) is sqrt(x), which IS correctly rounded on
                // the device, and the lobe is as wide as the diffuse one, so float acosf is as benign here as it is there
                theta = acosf(sqrt_cr(base));
            } else {
                // glossy lobe: acos(pow(x, 1/(coef+1))) sits at the ill-conditioned end of acos (argument within 1e-4 of 1),
                // where one ulp of pow moves theta by ~1e-3 relative.  Evaluate both in f64 and round, which reproduces a
                // correctly rounded float libm (tools/libm_probe: <0.02 % differing results vs 12 % / 28 % for the f32 forms).
                theta = glossy_theta(base, expo);
            }
            // sincosf shares the range reduction and returns bit for bit what sinf and cosf return (tools/sincos_probe.hip); sincos_cr is
            // its small-argument path alone
            sincos_cr(theta, &st, &ct);
        }
        sincos_cr(phi, &sp, &cp);
        ray = vsub(vadd(vscale(X, st * cp), vscale(Y, ct)), vscale(Z, st * sp));
    } while (vdot(normal, ray) < 0.f && ++tries < kHemisphereMaxTries);
    return ray;
}

// `dot(N, normalize(w)) < 0` (kernel.cu:437-441: V = normalize(ray.origin - x); if (dot(N, V) < 0) N = -N) without the
// normalisation when the sign is beyond doubt.  V_i = fl(w_i * inv) with inv > 0 carries one rounding, each product and each of
// the two additions one more: the computed dot differs from dot(N, w) * inv by less than 5e-7 of sum |N_i w_i| * inv, so
// beyond 1e-6 of that sum its sign is the sign of dot(N, w).  Closer calls (grazing within a microradian, NaN, w = 0) are
// decided by the reference's own expression.  (Saves a sqrt and a division per hit.)
__device__ __forceinline__ bool faces_away(v3 N, v3 w)
{
    const float ax = N.x * w.x, ay = N.y * w.y, az = N.z * w.z;
    const float s = ax + ay + az;
    const float sa = fabsf(ax) + fabsf(ay) + fabsf(az);
    if (fabsf(s) > 1e-6f * sa) return s < 0.0f;
    return vdot(N, vnormalize(w)) < 0.0f;
}

__device__ __forceinline__ float clampf(float f, float a, float b) { return fmaxf(a, fminf(f, b)); }  // vec_math.h:115-118

// The lane's index within its wave, as a value the compiler cannot hoist out of the loop it is read in.  What render_kernel derives
// from the lane (the pixel and sample of a unit, per-lane queue addresses, the tea<16> input) is cheap to derive again; hoisted to
// the kernel's start, it sat in VGPRs through every ray loop, which the 6-waves-per-SIMD budget (80 VGPRs) cannot afford.
__device__ __forceinline__ unsigned int opaque_lane()
{
    unsigned int l = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(l));
    return l;
}

// x of lane Q of the caller's DPP row (the 16 lanes lane & ~15 .. lane | 15): row_newbcast, which the compiler folds into the
// instruction that consumes it (v_add_f32_dpp).  Every lane of the wave must be enabled where it is called.
template <int Q>
__device__ __forceinline__ float row_bcast(float x)
{
    static_assert(Q >= 0 && Q < 16, "a DPP row is 16 lanes");
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x150 + Q, 0xF, 0xF, false));
}

// color += r of lane 0, 1, ... 15 of the row, in that order (kernel.cu:232 for a pixel whose 16 samples are the row's lanes)
template <int Q = 0>
__device__ __forceinline__ void row_sum16(v3& color, const v3 r)
{
    if constexpr (Q < 16) {
        color = vadd(color, mk(row_bcast<Q>(r.x), row_bcast<Q>(r.y), row_bcast<Q>(r.z)));
        row_sum16<Q + 1>(color, r);
    }
}

// The launch parameters at their place in the kernel-argument segment, through an address the compiler cannot hoist out of the
// scope it is taken in: every field read through it is a scalar load there (SMEM, no vector issue slot).  Read through the kernel
// argument itself, every field is loaded once at the kernel's start and held in an SGPR to the end; the 6-waves variant holds more of
// them than the 102 SGPRs a wave has, and the rest went to VGPR lanes (a v_writelane_b32 per save, a v_readlane_b32 per restore).
// p must be render_kernel's first argument: the only one at the start of the segment, where OPAQUE reads it.
template <bool OPAQUE>
__device__ __forceinline__ const LaunchParams& params_here(const LaunchParams& p)
{
    if constexpr (!OPAQUE) {
        return p;
    } else {
        typedef const __attribute__((address_space(4))) LaunchParams* KernargParams;
        unsigned long long a = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(a));
        return *(const LaunchParams*)(KernargParams)a;
    }
}

// running average + 8-bit image of one pixel: kernel.cu:236-246
// ratio = 1.0f / (float)(p.frame + 1): the 6-waves variant reads it from LDS (s_cam) where it writes, instead of holding the
// VALU division's result in a VGPR for the whole kernel
__device__ __forceinline__ void store_pixel(const LaunchParams& p, size_t idx, v3 cur)
{
    p.accum[idx] = make_float4(cur.x, cur.y, cur.z, 1.0f);
    // make_color, kernel.cu:90-98
    p.image[idx] = make_uchar4((unsigned char)(clampf(cur.x, 0.0f, 1.0f) * 255.0f), (unsigned char)(clampf(cur.y, 0.0f, 1.0f) * 255.0f),
                               (unsigned char)(clampf(cur.z, 0.0f, 1.0f) * 255.0f), 255u);
}

__device__ __forceinline__ void write_pixel(const LaunchParams& p, size_t idx, v3 cur, float ratio)
{
    if (p.frame > 0) {
        const float4 prev4 = p.accum[idx];
        const v3 prev = mk(prev4.x, prev4.y, prev4.z);
        cur = vadd(prev, vscale(vsub(cur, prev), ratio));  // lerp, vec_math.h:496-499
    }
    store_pixel(p, idx, cur);
}

// The batched kernels (render_frames_kernel) hold a pixel's running average in a register from frame to frame: write_pixel's step for
// frame `frame`, on the value the step before left instead of on what it stored.  The same operations in the same order (the build
// contracts nothing: one rounding each), and a float stored and loaded again is the same float, so n steps and one store_pixel leave
// what n launches' write_pixel leave.
__device__ __forceinline__ v3 mean_step(v3 prev, v3 cur, unsigned int frame)
{
    if (frame == 0u) return cur;
    return vadd(prev, vscale(vsub(cur, prev), 1.0f / (float)(frame + 1)));
}

// n frames of a pixel that is `cur` in every one of them (background: cold chunks, masked strips).  The steps are all taken: the
// average of equal values is not the value itself in float once the accumulation buffer held something else.
__device__ __forceinline__ void write_pixel_frames(const LaunchParams& p, size_t idx, v3 cur)
{
    v3 mean = cur;
    if (p.frame > 0) {
        const float4 prev4 = p.accum[idx];
        mean = mk(prev4.x, prev4.y, prev4.z);
    }
    for (unsigned int k = 0; k < p.n_frames; ++k) mean = mean_step(mean, cur, p.frame + k);
    store_pixel(p, idx, mean);
}

// Cold segment s -> (local row, first window column, column limit); see LaunchParams.  Wave-uniform.
__device__ __forceinline__ void cold_segment(const LaunchParams& p, unsigned int s, unsigned int& lr, unsigned int& x, unsigned int& lim)
{
    unsigned int j = s;
    const unsigned int below = p.hot_y0 * p.segs_full;
    if (j < below) {
        lr = j / p.segs_full;
        x = (j - lr * p.segs_full) * 64u;
        lim = p.w;
        return;
    }
    j -= below;
    const unsigned int above = p.rows_above * p.segs_full;
    if (j < above) {
        const unsigned int r = j / p.segs_full;
        lr = p.hot_y0 + p.hot_h + r;
        x = (j - r * p.segs_full) * 64u;
        lim = p.w;
        return;
    }
    j -= above;
    const unsigned int left = p.hot_h * p.segs_l;
    if (j < left) {
        const unsigned int r = j / p.segs_l;
        lr = p.hot_y0 + r;
        x = (j - r * p.segs_l) * 64u;
        lim = p.cold_x0;
        return;
    }
    j -= left;
    const unsigned int r = j / p.segs_r;
    lr = p.hot_y0 + r;
    x = p.cold_x1 + (j - r * p.segs_r) * 64u;
    lim = p.w;
}

// =====================================================================================================================
// The render megakernel.  Persistent workgroups; one lane = one PATH (see the decomposition note inside); each loop iteration
// traces exactly ONE ray per live lane (primary, bounce or shadow), so the 64 lanes of a wave stay at the same bounce and
// share the traversal and shading code.  Replaces __raygen__rg + optixTrace + the closest-hit/miss programs of kernel.cu.
// PATH = Params::enablePathTracing.  STATS = false: the fast walk (timed kernel).  STATS = true: the canonical LBVH walk with
// the V/T/h counters that define the roofline's algorithmic bytes; both produce the same pixels bit for bit.
// =====================================================================================================================
// WPE = waves per SIMD the register allocation targets: 4 (<= 128 VGPRs) for scenes whose LDS image limits a CU to 16 waves
// anyway, 5 (<= 96 VGPRs, per-level path records in LDS) for small scenes, where the fifth wave buys more than the tighter
// budget costs, and 6 (<= 80 VGPRs) for the path-mode FRAMES lock-step kernel, which fits that without scratch (rtgo_capi.hip
// picks per launch; kRenderKernels there lists every instantiation).
#ifndef RTGO_STREAM_WINDOW
#define RTGO_STREAM_WINDOW 4
#endif
constexpr int kStreamWindow = RTGO_STREAM_WINDOW;   // STREAM: passes a lane may run ahead of the oldest pass that is still open (192 floats of LDS per wave each)

// COUNT: the canonical walk's V/T/h counters (collect_stats launches); the same walk without them serves launches beyond the
// far-field guard, where it is the product path.
// FRAMES: the scene holds flat primitives only (cornell, checkered): closest-hit takes N and the sampling tangent from the frames
// build_kernel computed (bit for bit the per-hit values); an instantiation of its own, so that the other scenes' code is untouched.
// A progressive job's next frame redoes this frame's pixels with frame + 1.  A wave whose queue has run dry hashes their seeds for the
// next launch (LaunchParams::seeds_next) in chunks of 64 pixels, one per lane, so that every lane of the 16 rounds is used -- against a
// strip's hash in the ray loop's prologue, of which a 1-unit strip keeps 4 of 64 lanes.  Wave w of the grid takes chunks w, w + waves,
// ... (1080p: ~1.5 per wave): no shared counter, which 6144 waves would queue at (one counter, ~88 atomics / us: +0.39 ms a frame).
// The pixel of word i is the one render_kernel hashes for lane i % strip_px of hot strip i / strip_px.
// Only the 6-waves lock-step variant has the pass (and reads LaunchParams::seeds): the host picks it for launches of >= 8 units per
// wave (kUnitsPerWave4For6), where the strips' hashes saved outweigh a pass at the end of every wave -- a 1/8 band share of the bench
// frame has ~3 strips per wave -- and every other variant compiles as it did without it (their register budgets have no room).
constexpr bool kernel_has_seed_pass(bool stats, int wpe, bool stream) { return !stats && wpe >= 6 && !stream; }

__device__ __forceinline__ void next_frame_seeds(const LaunchParams& p, unsigned int lane, unsigned int P, unsigned int wave, unsigned int waves)
{
    const unsigned int strip_px = p.grab * P;
    const unsigned int n_px = p.n_hot * strip_px;
    for (unsigned int c = wave; c < (n_px + 63u) / 64u; c += waves) {
        const unsigned int i = c * 64u + lane;
        if (i < n_px) {
            const unsigned int strip = i / strip_px, j = i - strip * strip_px;
            const unsigned int lr = p.hot_y0 + strip / p.hot_w;
            const unsigned int sx = p.hot_x0 + (strip - (lr - p.hot_y0) * p.hot_w);
            const unsigned int band = lr / p.band_h;
            const unsigned int gy = p.y0 + (band * p.n_ranks + p.rank) * p.band_h + (lr - band * p.band_h);
            p.seeds_next[i] = tea16(p.W * gy + (p.x0 + sx * strip_px + j), p.frame + 1u);
        }
    }
}

// GLOBAL (with STATS, not FRAMES / GRID / STREAM): a scene of rtgo_set_large_scene.  The canonical walk reads nodes and primitive records
// straight from global memory (p.nodes / p.prims: the same layout and the same arithmetic as the LDS copy), nothing is staged; LDS holds
// the stack (p.stack_depth entries: the scene's depth), the lights, the raygen constants and the sample table.
// BATCH (render_frames_kernel; lock-step, fast walk over a tree): p.n_frames progressive frames of every strip in one launch.  Frame
// f + 1 of a pixel needs frame f of that pixel alone (kernel.cu:236-246), so the wave that holds a strip renders the strip's frames one
// after the other -- new seeds, the same units -- and keeps the running averages in registers, lane j that of the strip's pixel j (a
// strip is at most 64 pixels).  The accumulation buffer is read once (not at all from frame 0) and both outputs are written once, after
// the last frame: no flag, no ordering between waves.
template <bool PATH, bool STATS, int WPE, bool STREAM, bool COUNT = STATS, bool FRAMES = false, bool GRID = false, bool GLOBAL = false>
__global__ __launch_bounds__(kMaxBlock) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void render_kernel(const LaunchParams p_arg, const float4* __restrict__ g_fprims)
{
    constexpr bool BATCH = false, PAIR = false, SLAB = false, UNIT16 = false, ROOMW = false;
#include "rtgo_render_body.inc"
}

// n progressive frames per launch (rtgo_launch_frames): the lock-step loop with the fast walk over a tree, see BATCH above
template <bool PATH, int WPE, bool FRAMES>
__global__ __launch_bounds__(kMaxBlock) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void render_frames_kernel(const LaunchParams p_arg, const float4* __restrict__ g_fprims)
{
    constexpr bool BATCH = true, STATS = false, STREAM = false, COUNT = false, GRID = false, GLOBAL = false, PAIR = false, SLAB = false, UNIT16 = false, ROOMW = false;
#include "rtgo_render_body.inc"
}

// PAIR: path mode over a flat scene whose fast-walk tree is a root over two certified cuboid leaves (cornell: the short and the tall box),
// lock-step, one frame per launch.  render_kernel<true, false, WPE, false, false, true> with fast_pair in fast_tree's place; at 6 waves it
// keeps all that kernel has (LEAN, params_here, the seed pass, LASTRAY).  The host takes it where the launch qualifies (rtgo_capi.hip).
template <int WPE>
__global__ __launch_bounds__(kMaxBlock) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void render_pair_kernel(const LaunchParams p_arg, const float4* __restrict__ g_fprims)
{
    constexpr bool PATH = true, STATS = false, STREAM = false, COUNT = false, FRAMES = true, GRID = false, GLOBAL = false, BATCH = false, PAIR = true, SLAB = false, UNIT16 = false, ROOMW = false;
#include "rtgo_render_body.inc"
}

// ... at 7 waves per SIMD (72 VGPRs): everything render_pair_kernel<6> has -- every WPE >= 6 switch of the body reads 7 as 6 -- under a
// tighter register budget, for launches with enough units per wave to keep 28 waves of a CU busy (pick_block).  A name of its own: the
// template above stays at its two instantiations.
__global__ __launch_bounds__(kMaxBlock) __attribute__((amdgpu_waves_per_eu(7, 7))) void render_pair7_kernel(const LaunchParams p_arg, const float4* __restrict__ g_fprims)
{
    constexpr bool PATH = true, STATS = false, STREAM = false, COUNT = false, FRAMES = true, GRID = false, GLOBAL = false, BATCH = false, PAIR = true, SLAB = false, UNIT16 = false, ROOMW = false;
    constexpr int WPE = 7;
#include "rtgo_render_body.inc"
}

// render_pair7_kernel with the slab test (cuboid_slab) in cuboid_range's place, for the room and for both leaves: launches whose room and
// leaves hold the slab certificate (rtgo_build.h).  The one form of the cuboid test in the kernel is the slab's.
__global__ __launch_bounds__(kMaxBlock) __attribute__((amdgpu_waves_per_eu(7, 7))) void render_slab7_kernel(const LaunchParams p_arg, const float4* __restrict__ g_fprims)
{
    constexpr bool PATH = true, STATS = false, STREAM = false, COUNT = false, FRAMES = true, GRID = false, GLOBAL = false, BATCH = false, PAIR = true, SLAB = true, UNIT16 = false, ROOMW = false;
    constexpr int WPE = 7;
#include "rtgo_render_body.inc"
}

// render_slab7_kernel for launches of 16 samples per pixel in workgroups of 256 threads (the host checks both: rtgo_capi.hip), with what
// such a launch fixes as compile-time values (UNIT16): a unit is 4 pixels x 16 samples in one pass, so a lane's pixel and sample are a
// shift and a mask, a sample's start is the table's, and a pixel's 16 samples are one DPP row -- the in-order sum is 16 row-broadcast
// additions per channel (row_sum16) in place of 16 dependent LDS round trips; a level record's three words lie at fixed offsets from
// one address.  The same float operations on the same values in the same order: the same bits.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 7))) void render_unit16_kernel(const LaunchParams p_arg, const float4* __restrict__ g_fprims)
{
    constexpr bool PATH = true, STATS = false, STREAM = false, COUNT = false, FRAMES = true, GRID = false, GLOBAL = false, BATCH = false, PAIR = true, SLAB = true, UNIT16 = true, ROOMW = false;
    constexpr int WPE = 7;
#include "rtgo_render_body.inc"
}

// render_unit16_kernel with the room's slab test steered in world axes (ROOMW: room_world on the walk's own reciprocals, no transform into
// the first wall's frame): launches whose room also holds the world-axis certificate at their reach (rtgo_room_world.h, rtgo_capi.hip).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 7))) void render_roomw_kernel(const LaunchParams p_arg, const float4* __restrict__ g_fprims)
{
    constexpr bool PATH = true, STATS = false, STREAM = false, COUNT = false, FRAMES = true, GRID = false, GLOBAL = false, BATCH = false, PAIR = true, SLAB = true, UNIT16 = true, ROOMW = true;
    constexpr int WPE = 7;
#include "rtgo_render_body.inc"
}

}  // namespace rtgo

#include "rtgo_build.h"  // scene preparation and the builds: PrimIn .. build_kernel (uses the definitions above)

namespace rtgo {

// =====================================================================================================================
// Presentation step of the multi-GPU driver: the root holds n_ranks compact band buffers back to back (rows_pad rows each) and
// scatters their rows to the rows of the full window they belong to under the band interleave.  T = uint4 (16-byte units) or
// unsigned int (4-byte units); row_units = units per row.  Pure copy: HBM-bound, one unit per thread, coalesced both ways.
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void assemble_bands_kernel(const T* __restrict__ gathered, T* __restrict__ full, unsigned int row_units,
                                                            unsigned int h, unsigned int band_h, unsigned int n_ranks, unsigned int rows_pad)
{
    const unsigned long long total = (unsigned long long)row_units * h;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned int r = (unsigned int)(i / row_units), x = (unsigned int)(i - (unsigned long long)r * row_units);
        const unsigned int band = r / band_h, g = band % n_ranks;
        const unsigned int k = (band / n_ranks) * band_h + (r - band * band_h);   // rank g's local row
        full[i] = gathered[((unsigned long long)g * rows_pad + k) * row_units + x];
    }
}

}  // namespace rtgo
