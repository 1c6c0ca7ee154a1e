// rtgo_build.h -- the code that BUILDS what the render kernels walk.  Included by rtgo_device.h (after v3 and its helpers, xf_normal,
// kMaxPrims, kCuboidTol, which it uses), so every includer of rtgo_device.h has it; not meant to be included on its own.
// Scene preparation (PrimIn, the inverse of Matrix.h, the CubeBox boxes); the pieces every build shares, each once (Morton keys, Karras
// nodes, bounds reduction, bitonic sort, the top-down surface-area build: also used by rtgo_large.h, rtgo_whitted.h, rtgo_whitted_big.h);
// build_kernel: its results as types, its LDS as one struct, its stages as functions in the order they run.
#pragma once

namespace rtgo {

// =====================================================================================================================
// Scene preparation + canonical LBVH build, one workgroup (n <= 512): replaces optixAccelBuild (renderer.cpp:514-611) and
// hoists Matrix4x4::inverse() (Matrix.h:591-635) out of the intersection programs.
// =====================================================================================================================
struct PrimIn {  // = rtgo_prim
    unsigned int type;
    float M[16];
    float kd[3], kr[3], spec, Le[3];
};

__device__ __forceinline__ float det4(const float* m)
{
    // Matrix.h:591-608, term order and product association preserved
    return m[0] * m[5] * m[10] * m[15] - m[0] * m[5] * m[11] * m[14] + m[0] * m[9] * m[14] * m[7] - m[0] * m[9] * m[6] * m[15] +
           m[0] * m[13] * m[6] * m[11] - m[0] * m[13] * m[10] * m[7] - m[4] * m[1] * m[10] * m[15] + m[4] * m[1] * m[11] * m[14] -
           m[4] * m[9] * m[14] * m[3] + m[4] * m[9] * m[2] * m[15] - m[4] * m[13] * m[2] * m[11] + m[4] * m[13] * m[10] * m[3] +
           m[8] * m[1] * m[6] * m[15] - m[8] * m[1] * m[14] * m[7] + m[8] * m[5] * m[14] * m[3] - m[8] * m[5] * m[2] * m[15] +
           m[8] * m[13] * m[2] * m[7] - m[8] * m[13] * m[6] * m[3] - m[12] * m[1] * m[6] * m[11] + m[12] * m[1] * m[10] * m[7] -
           m[12] * m[5] * m[10] * m[3] + m[12] * m[5] * m[2] * m[11] - m[12] * m[9] * m[2] * m[7] + m[12] * m[9] * m[6] * m[3];
}

// one cofactor group of Matrix.h:612-635: a*(b*c - d*e)
#define RTGO_G(a, b, c, d, e) (m[a] * (m[b] * m[c] - m[d] * m[e]))

__device__ __forceinline__ void inverse_rows012(const float* m, float* o)
{
    const float d = 1.0f / det4(m);
    o[0] = d * (RTGO_G(5, 10, 15, 14, 11) + RTGO_G(9, 14, 7, 6, 15) + RTGO_G(13, 6, 11, 10, 7));
    o[4] = d * (RTGO_G(6, 8, 15, 12, 11) + RTGO_G(10, 12, 7, 4, 15) + RTGO_G(14, 4, 11, 8, 7));
    o[8] = d * (RTGO_G(7, 8, 13, 12, 9) + RTGO_G(11, 12, 5, 4, 13) + RTGO_G(15, 4, 9, 8, 5));
    o[1] = d * (RTGO_G(9, 2, 15, 14, 3) + RTGO_G(13, 10, 3, 2, 11) + RTGO_G(1, 14, 11, 10, 15));
    o[5] = d * (RTGO_G(10, 0, 15, 12, 3) + RTGO_G(14, 8, 3, 0, 11) + RTGO_G(2, 12, 11, 8, 15));
    o[9] = d * (RTGO_G(11, 0, 13, 12, 1) + RTGO_G(15, 8, 1, 0, 9) + RTGO_G(3, 12, 9, 8, 13));
    o[2] = d * (RTGO_G(13, 2, 7, 6, 3) + RTGO_G(1, 6, 15, 14, 7) + RTGO_G(5, 14, 3, 2, 15));
    o[6] = d * (RTGO_G(14, 0, 7, 4, 3) + RTGO_G(2, 4, 15, 12, 7) + RTGO_G(6, 12, 3, 0, 15));
    o[10] = d * (RTGO_G(15, 0, 5, 4, 1) + RTGO_G(3, 4, 13, 12, 5) + RTGO_G(7, 12, 1, 0, 13));
    o[3] = d * (RTGO_G(1, 10, 7, 6, 11) + RTGO_G(5, 2, 11, 10, 3) + RTGO_G(9, 6, 3, 2, 7));
    o[7] = d * (RTGO_G(2, 8, 7, 4, 11) + RTGO_G(6, 0, 11, 8, 3) + RTGO_G(10, 4, 3, 0, 7));
    o[11] = d * (RTGO_G(3, 8, 5, 4, 9) + RTGO_G(7, 0, 9, 8, 1) + RTGO_G(11, 4, 1, 0, 5));
}
#undef RTGO_G

// Primitive::GetAabb / CubeBox::TransformAndAlign (primitive.cpp:35-79, 100-115): the 8 corners of [-1,1]^3 through the
// 4-term matrix product (sum seeded with 0.0f, Matrix.h:344-360), min/max seeded with +-50, +-1e-3 pad.
__device__ __forceinline__ void cube_aabb(const float* M, float* bb)
{
    float mn[3] = {50.0f, 50.0f, 50.0f}, mx[3] = {-50.0f, -50.0f, -50.0f};
    // corner order of CubeBox::face0/face1 columns: x = {-1,-1,1,1}, z = {-1,1,-1,1}, y = -1 (face0) / +1 (face1)
    const float cxs[4] = {-1.f, -1.f, 1.f, 1.f}, czs[4] = {-1.f, 1.f, -1.f, 1.f};
    for (int i = 0; i < 4; ++i)
        for (int a = 0; a < 3; ++a) {
            const float* r = M + 4 * a;
            float p0 = 0.0f, p1 = 0.0f;
            p0 += r[0] * cxs[i];
            p0 += r[1] * -1.f;
            p0 += r[2] * czs[i];
            p0 += r[3] * 1.f;
            p1 += r[0] * cxs[i];
            p1 += r[1] * 1.f;
            p1 += r[2] * czs[i];
            p1 += r[3] * 1.f;
            float t = (p0 < mn[a]) ? p0 : mn[a];
            mn[a] = (p1 < t) ? p1 : t;
            t = (mx[a] < p0) ? p0 : mx[a];
            mx[a] = (t < p1) ? p1 : t;
        }
    for (int a = 0; a < 3; ++a) {
        bb[a] = mn[a] - 0.001f;
        bb[3 + a] = mx[a] + 0.001f;
    }
}

__device__ __forceinline__ unsigned int expand_bits(unsigned int v)
{
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

__device__ __forceinline__ int lbvh_delta(const unsigned long long* keys, int n, int i, int j)
{
    if (j < 0 || j >= n) return -1;
    const unsigned int a = (unsigned int)(keys[i] >> 32), b = (unsigned int)(keys[j] >> 32);
    if (a == b) return 32 + __clz((unsigned int)i ^ (unsigned int)j);
    return __clz(a ^ b);
}

// One axis of a box centre c on the 10-bit Morton grid of the scene bounds [lo, lo + ext] (build_kernel and the global-memory build)
__device__ __forceinline__ unsigned int morton_cell(float c, float lo, float ext)
{
    const float u = ext > 0.0f ? (c - lo) / ext : 0.0f;
    return (unsigned int)fminf(fmaxf(u * 1024.0f, 0.0f), 1023.0f);
}
__device__ __forceinline__ unsigned int morton3(const unsigned int q[3])
{
    return (expand_bits(q[0]) << 2) | (expand_bits(q[1]) << 1) | expand_bits(q[2]);
}

// Karras 2012: the children and the sorted key range [lo, hi] of internal node i of the tree over the m sorted unique keys (leaves are
// nodes [m-1, 2m-2]; node 0 is the root)
__device__ __forceinline__ void karras_node(const unsigned long long* keys, int m, int i, int& left, int& right, int& lo, int& hi)
{
    const int leaf0 = m - 1;
    const int d = (lbvh_delta(keys, m, i, i + 1) - lbvh_delta(keys, m, i, i - 1)) >= 0 ? 1 : -1;
    const int dmin = lbvh_delta(keys, m, i, i - d);
    int lmax = 2;
    while (lbvh_delta(keys, m, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (lbvh_delta(keys, m, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = lbvh_delta(keys, m, i, j);
    int s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (lbvh_delta(keys, m, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + (d < 0 ? -1 : 0);
    lo = i < j ? i : j;
    hi = i < j ? j : i;
    left = (lo == gamma) ? leaf0 + gamma : gamma;
    right = (hi == gamma + 1) ? leaf0 + gamma + 1 : gamma + 1;
}

// The 6-float4 record of a primitive (SBT order, layout above) from its PrimIn and rows 0..2 of M^-1
__device__ __forceinline__ void store_prim_record(float4* __restrict__ out, const PrimIn& P, const float* inv)
{
    out[0] = make_float4(inv[0], inv[1], inv[2], inv[3]);
    out[1] = make_float4(inv[4], inv[5], inv[6], inv[7]);
    out[2] = make_float4(inv[8], inv[9], inv[10], inv[11]);
    out[3] = make_float4(P.kd[0], P.kd[1], P.kd[2], P.spec);
    out[4] = make_float4(P.kr[0], P.kr[1], P.kr[2], __int_as_float((int)P.type));
    out[5] = make_float4(P.Le[0], P.Le[1], P.Le[2], 0.0f);
}

// The pieces every build shares (this kernel, rtgo_large.h, rtgo_whitted.h, rtgo_whitted_big.h)

// min / max over the workgroup's THREADS per-thread boxes (lo, hi) -> red[0..5][0] (exact, order-independent).  Every thread calls it.
template <int THREADS>
__device__ __forceinline__ void reduce_bounds(float (*red)[THREADS], int tid, const float lo[3], const float hi[3])
{
    for (int a = 0; a < 3; ++a) {
        red[a][tid] = lo[a];
        red[3 + a][tid] = hi[a];
    }
    __syncthreads();
    for (int stride = THREADS / 2; stride > 0; stride >>= 1) {
        if (tid < stride)
            for (int a = 0; a < 3; ++a) {
                red[a][tid] = fminf(red[a][tid], red[a][tid + stride]);
                red[3 + a][tid] = fmaxf(red[3 + a][tid], red[3 + a][tid + stride]);
            }
        __syncthreads();
    }
}

// bitonic sort of N keys in LDS by the workgroup's THREADS threads; keys are unique, so the result is THE (code, index) order
template <int N, int THREADS>
__device__ __forceinline__ void bitonic_sort(unsigned long long* keys, int tid)
{
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N; i += THREADS) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = keys[i], b = keys[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) {
                        keys[i] = b;
                        keys[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
}

// sort key of triangle i: the 30-bit Morton code of its centroid on the grid of the bounds [lo, lo + ext], then the triangle
__device__ __forceinline__ unsigned long long triangle_key(const float* __restrict__ positions, const unsigned int* __restrict__ indices, int i,
                                                           const float lo[3], const float ext[3])
{
    unsigned int q[3];
    for (int a = 0; a < 3; ++a) {
        const float c = (positions[3 * (size_t)indices[3 * (size_t)i + 0] + a] + positions[3 * (size_t)indices[3 * (size_t)i + 1] + a] +
                         positions[3 * (size_t)indices[3 * (size_t)i + 2] + a]) * (1.0f / 3.0f);
        q[a] = morton_cell(c, lo[a], ext[a]);
    }
    return ((unsigned long long)morton3(q) << 32) | (unsigned int)i;
}

// ---------------------------------------------------------------------------------------------------------------------
// Top-down surface-area build over `n_units` units (boxes with cost weights), one workgroup.  Every node is split where
// A(left) * W(left) + A(right) * W(right) is smallest over the three axes and every position of its units sorted by centroid.  All
// THREADS threads walk one task queue together: a rank sort per axis in parallel, the sweep by one thread.  The callers differ in:
//   box(u, c), weight(u)   unit u's box coordinate c and cost weight
//   perm, tmp [n_units]    the units in the current task order (the caller fills perm with 0 .. n_units - 1) and its double buffer
//   sfx [2 n_units]        suffix area and weight of the sweep
//   q                      the task queue, <= 2 n_units - 1 entries (max_tasks bounds the loop)
//   t                      the tree under construction: node 0 is the root, children are allocated in pairs
//   leaf(node, u)          the links of a node that holds the one unit u (its box is written here)
//   MEDIAN_TIES            equal costs go to the split nearer the median (else the first position wins)
// and in nothing else.  Returns the number of nodes (2 n_units - 1; 0 without units); ends in a barrier.
// ---------------------------------------------------------------------------------------------------------------------
struct SahShared { int qtail, n_nodes, best_axis, best_pos; };   // the workgroup's scalars of sah_build, in LDS
struct SahTree { float* box; int *left, *right, *parent; };   // box: [node][6]
template <class T>
struct SahQueue { T *node, *lo, *hi; };   // task k builds `node` over perm[lo, hi)

template <int THREADS, bool MEDIAN_TIES, class T, class Box, class Weight, class Leaf>
__device__ __forceinline__ int sah_build(int tid, int n_units, int max_tasks, Box box, Weight weight, short* perm, short* tmp, float* sfx,
                                         SahQueue<T> q, SahTree t, SahShared& sh, Leaf leaf)
{
    if (tid == 0) {
        q.node[0] = 0;
        q.lo[0] = 0;
        q.hi[0] = (T)n_units;
        sh.qtail = n_units > 0 ? 1 : 0;
        sh.n_nodes = n_units > 0 ? 1 : 0;
        t.parent[0] = -1;
    }
    __syncthreads();
    for (int qi = 0; qi < max_tasks; ++qi) {
        __syncthreads();
        if (qi >= sh.qtail) break;   // (uniform: every thread reads the same word after the barrier)
        const int lo = q.lo[qi], hi = q.hi[qi], node = q.node[qi], m = hi - lo;
        if (m == 1) {
            if (tid == 0) {
                const int u = perm[lo];
                for (int c = 0; c < 6; ++c) t.box[6 * node + c] = box(u, c);
                leaf(node, u);
            }
            continue;
        }
        if (tid == 0) {
            sh.best_axis = -1;
            sh.best_pos = m / 2;
        }
        float best_cost = INFINITY;   // (thread 0's)
        for (int pass = 0; pass < 4; ++pass) {
            // passes 0..2: try axis `pass`; pass 3: put the range back in the order of the best axis
            __syncthreads();
            const int axis = pass < 3 ? pass : sh.best_axis;
            if (pass == 3 && (axis < 0 || axis == 2)) break;   // (uniform) no finite cost at all, or already in z order
            for (int e = tid; e < m; e += THREADS) {
                const int me = perm[lo + e];
                const float key = box(me, axis) + box(me, 3 + axis);
                int rank = 0;
                for (int j = 0; j < m; ++j) {
                    const int other = perm[lo + j];
                    const float kj = box(other, axis) + box(other, 3 + axis);
                    rank += (kj < key || (kj == key && other < me)) ? 1 : 0;
                }
                tmp[lo + rank] = (short)me;
            }
            __syncthreads();
            for (int e = tid; e < m; e += THREADS) perm[lo + e] = tmp[lo + e];
            __syncthreads();
            if (pass < 3 && tid == 0) {
                // suffix boxes and weights from the right, then the sweep from the left
                float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
                int w = 0;
                for (int j = m - 1; j >= 1; --j) {
                    const int u = perm[lo + j];
                    for (int c = 0; c < 3; ++c) {
                        b[c] = fminf(b[c], box(u, c));
                        b[3 + c] = fmaxf(b[3 + c], box(u, 3 + c));
                    }
                    w += weight(u);
                    const float ex = b[3] - b[0], ey = b[4] - b[1], ez = b[5] - b[2];
                    sfx[2 * j + 0] = ex * ey + ey * ez + ez * ex;
                    sfx[2 * j + 1] = (float)w;
                }
                float a[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
                int wl = 0;
                for (int j = 1; j < m; ++j) {   // left = [0, j), right = [j, m)
                    const int u = perm[lo + j - 1];
                    for (int c = 0; c < 3; ++c) {
                        a[c] = fminf(a[c], box(u, c));
                        a[3 + c] = fmaxf(a[3 + c], box(u, 3 + c));
                    }
                    wl += weight(u);
                    const float ex = a[3] - a[0], ey = a[4] - a[1], ez = a[5] - a[2];
                    const float cost = (ex * ey + ey * ez + ez * ex) * (float)wl + sfx[2 * j] * sfx[2 * j + 1];
                    bool better = cost < best_cost;
                    if (MEDIAN_TIES) {
                        // ties go to the split nearer the median: a range of units with one and the same box (coincident or duplicated
                        // triangles) ties at every position, and "first wins" would peel one unit per level -- a chain as deep as the range
                        const int dj = j > m / 2 ? j - m / 2 : m / 2 - j, db = sh.best_pos > m / 2 ? sh.best_pos - m / 2 : m / 2 - sh.best_pos;
                        better = better || (cost == best_cost && dj < db);
                    }
                    if (better) {
                        best_cost = cost;
                        sh.best_axis = pass;
                        sh.best_pos = j;
                    }
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            // this node: box of its range, two children appended to the queue
            float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
            for (int j = lo; j < hi; ++j) {
                const int u = perm[j];
                for (int c = 0; c < 3; ++c) {
                    b[c] = fminf(b[c], box(u, c));
                    b[3 + c] = fmaxf(b[3 + c], box(u, 3 + c));
                }
            }
            const int cl = sh.n_nodes, cr = sh.n_nodes + 1;
            sh.n_nodes += 2;
            for (int c = 0; c < 6; ++c) t.box[6 * node + c] = b[c];
            t.left[node] = cl;
            t.right[node] = cr;
            t.parent[cl] = node;
            t.parent[cr] = node;
            const int mid = lo + sh.best_pos;
            const int tail = sh.qtail;
            q.node[tail] = (T)cl; q.lo[tail] = (T)lo; q.hi[tail] = (T)mid;
            q.node[tail + 1] = (T)cr; q.lo[tail + 1] = (T)mid; q.hi[tail + 1] = (T)hi;
            sh.qtail = tail + 2;
        }
    }
    __syncthreads();
    return sh.n_nodes;
}

// build_kernel's results: the meta words (the packed fields' codes are rtgo_device.h's encode_group / encode_leaf_link)
struct BuildMeta {
    int canonical_depth;     // of the canonical LBVH
    int walk_depth;          // stack entries the fast walk needs
    int n_small;             // primitives in the fast walk's tree (the rest are tested up front)
    float tight_bounds[6];   // of the tight boxes: min xyz, max xyz
    int list_group;          // encode_group of the up-front list
    int n_fnodes;            // nodes of the fast walk's tree (2 * units - 1)
    float cub_a, cub_b;      // the two coefficients of cuboid_range's margin
    int cuboid_leaves;       // leaves certified as cuboids
    int tree_types;          // primitive types present in the fast walk's tree (bit = type)
};
static_assert(sizeof(BuildMeta) == 15 * sizeof(int), "build_kernel's meta words");

// build_kernel, one workgroup of kMaxPrims threads (thread i = primitive i): its LDS, then its stages in the order they run
// All static LDS of build_kernel (under 64 KiB on purpose).  A union holds the views of storage used twice; the comments name the barrier between them.
struct BuildLds {
    union {
        unsigned long long keys[kMaxPrims];    // canonical_lbvh .. pair_and_certify: the sort keys, code << 32 | primitive
        struct {                               // form_units on (after pair_and_certify's last barrier): the walk's units
            short node[kMaxPrims];             //   Morton-tree node of unit u
            short perm[kMaxPrims], tmp[kMaxPrims];   // sah_build's order arrays
        } unit;
    };
    union {
        float box[kMaxPrims][6];               // prep_primitives .. morton_units: per primitive the reference AABB, later the tight box
        float sfx[2 * kMaxPrims];              // sah_build (after form_units' barriers): suffix area and weight of the sweep
    };
    union {
        float nbox[2 * kMaxPrims][6];          // morton_tree .. sah_build: node boxes (leaves are nodes [m-1, 2m-2])
        float red[6][kMaxPrims];               // the bounds reductions, which run while no tree is in nbox (before canonical_lbvh's tree; between
                                               // its write-out barrier and morton_units' tree)
    };
    union {
        int left[kMaxPrims];                   // morton_tree .. pair_and_certify: first child of an internal node
        int unit_at[kMaxPrims];                // form_units (after its first barrier): node of the unit that starts at a Morton position, -1: none
    };
    union {
        int right[kMaxPrims];                  // morton_tree .. pair_and_certify: second child
        int unit_wt[kMaxPrims];                // form_units on: cost weight of unit u
    };
    union {
        int parent[2 * kMaxPrims];             // morton_tree .. form_units
        struct { short node[2 * kMaxPrims], lo[2 * kMaxPrims]; } tq;   // sah_build (after form_units' last barrier): the task queue
    };
    union {
        int wt[2 * kMaxPrims];                 // morton_units .. form_units: cost weight of each subtree
        short tq_hi[2 * kMaxPrims];            // sah_build (after form_units' last barrier)
    };
    union {
        int visit[kMaxPrims];                  // morton_tree: arrivals at an internal node
        int leaf_group[kMaxPrims];             // pair_and_certify (after morton_units' tree) .. sah_build: encode_group of a collapsed leaf
    };
    union {
        int canonical_depth;                   // canonical_lbvh
        int walk_depth;                        // morton_units on (after canonical_lbvh's last barrier)
    };
    union {
        int n_small;                           // tight_boxes_and_big (every thread keeps its copy)
        int n_unpaired_leaves;                 // pair_and_certify (after morton_units' barriers): leaves that do not pair up completely
        SahShared sah;                         // sah_build (after form_units' barriers)
    };
    int tmask;                                 // primitive types present in the fast walk's tree (bit = type)
    int cub_a, cub_b;                          // cuboid_range's margin coefficients (positive floats as bits: integer max = float max)
    int cuboid_leaves, n_units;
    short lo[kMaxPrims], hi[kMaxPrims];        // Morton range covered by each internal node
    unsigned short order[kMaxPrims];           // primitive at each record position (pairs side by side)
    unsigned char flag[kMaxPrims];             // 1 = "big" primitive kept out of the tree
    unsigned char used[kMaxPrims];             // group_cube_faces: place within a cube (0..5, 0xFF: none); pair_and_certify: already placed
};

// min/max over the boxes of the primitives selected by `take` -> s.red[0..5][0]
__device__ __forceinline__ void reduce_boxes(BuildLds& s, int i, bool take)
{
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = take ? s.box[i][a] : INFINITY;
        hi[a] = take ? s.box[i][3 + a] : -INFINITY;
    }
    reduce_bounds<kMaxPrims>(s.red, i, lo, hi);
}

// 30-bit Morton code of the centre of the union of the boxes [first, first + count), normalised to the bounds in s.red[..][0]
__device__ __forceinline__ unsigned int morton_of(const BuildLds& s, int first, int count = 1, bool cubic = false)
{
    unsigned int q[3];
    // cubic: one scale for the three axes (the longest extent), so that a Morton cell is a cube and not a slab
    const float emax = fmaxf(fmaxf(s.red[3][0] - s.red[0][0], s.red[4][0] - s.red[1][0]), s.red[5][0] - s.red[2][0]);
    for (int a = 0; a < 3; ++a) {
        float lo = s.box[first][a], hi = s.box[first][3 + a];
        for (int k = 1; k < count; ++k) {
            lo = fminf(lo, s.box[first + k][a]);
            hi = fmaxf(hi, s.box[first + k][3 + a]);
        }
        const float c = (lo + hi) * 0.5f;
        const float ext = cubic ? emax : s.red[3 + a][0] - s.red[a][0];
        q[a] = morton_cell(c, s.red[a][0], ext);
    }
    return morton3(q);
}

// Karras 2012 over the first m sorted keys + bottom-up fit of boxes (and cost weights).  Leaves are nodes [m-1, 2m-2].
__device__ __forceinline__ void morton_tree(BuildLds& s, int i, int m, bool with_weights)
{
    const int leaf0 = m - 1;
    if (i < m) {
        const int prim = (int)(s.keys[i] & 0xFFFFFFFFu);
        for (int a = 0; a < 6; ++a) s.nbox[leaf0 + i][a] = s.box[prim][a];
        s.visit[i] = 0;
    }
    if (i < 2 * m - 1) s.parent[i] = -1;
    if (i + kMaxPrims < 2 * m - 1) s.parent[i + kMaxPrims] = -1;
    __syncthreads();
    if (i < m - 1) {
        int left, right, lo, hi;
        karras_node(s.keys, m, i, left, right, lo, hi);
        s.left[i] = left;
        s.right[i] = right;
        s.lo[i] = (short)lo;
        s.hi[i] = (short)hi;
        s.parent[left] = i;
        s.parent[right] = i;
    }
    __syncthreads();
    // the second arrival at a node (LDS atomic) owns it
    if (i < m && m > 1) {
        int pnode = s.parent[leaf0 + i];
        while (pnode >= 0) {
            __threadfence_block();
            if (atomicAdd(&s.visit[pnode], 1) == 0) break;
            __threadfence_block();
            const int L = s.left[pnode], R = s.right[pnode];
            for (int a = 0; a < 3; ++a) {
                s.nbox[pnode][a] = fminf(s.nbox[L][a], s.nbox[R][a]);
                s.nbox[pnode][3 + a] = fmaxf(s.nbox[L][3 + a], s.nbox[R][3 + a]);
            }
            if (with_weights) s.wt[pnode] = s.wt[L] + s.wt[R];
            pnode = s.parent[pnode];
        }
    }
    __syncthreads();
}

// ---- stage: per primitive its inverse, record, shading frame and reference AABB (-> s.box); ends in a barrier
__device__ __forceinline__ void prep_primitives(BuildLds& s, int i, int n, const PrimIn* __restrict__ prims, float* __restrict__ aabb_io, int have_aabb,
                                                float4* __restrict__ out_prims, float4* __restrict__ out_frames, PrimIn& P)
{
    if (i < n) {
        P = prims[i];
        float inv[12];
        inverse_rows012(P.M, inv);
        store_prim_record(out_prims + 6 * i, P, inv);
        // Shading frame of a FLAT primitive (rectangle, disk: object-space normal (0,1,0), kernel.cu:345,388): what the closest-hit
        // program computes from it on every hit -- N = normalize(TransformNormal(0,1,0)) (kernel.cu:428) and the tangent of
        // GetRayOnHemisphere for direction N, X = normalize(N.y - N.z, -N.x, N.x) (kernel.cu:105) -- depends on the primitive alone.
        // Computed here ONCE with the same device functions on the same values, so the bits are those of the per-hit computation;
        // a flipped normal flips both exactly (the expressions are odd in N, negation is exact), and Z = N x X is unchanged.
        const bool flat = P.type == 1u || P.type == 2u;
        v3 fn = mk(0.0f, 0.0f, 0.0f), fx = mk(0.0f, 0.0f, 0.0f);
        if (flat) {
            fn = vnormalize(xf_normal(make_float4(inv[0], inv[1], inv[2], inv[3]), make_float4(inv[4], inv[5], inv[6], inv[7]), make_float4(inv[8], inv[9], inv[10], inv[11]), mk(0.0f, 1.0f, 0.0f)));
            fx = vnormalize(mk(fn.y - fn.z, -fn.x, fn.x));
        }
        out_frames[2 * i + 0] = make_float4(fn.x, fn.y, fn.z, flat ? 1.0f : 0.0f);
        out_frames[2 * i + 1] = make_float4(fx.x, fx.y, fx.z, 0.0f);
        float bb[6];
        if (have_aabb) {
            for (int a = 0; a < 6; ++a) bb[a] = aabb_io[6 * i + a];
        } else {
            cube_aabb(P.M, bb);
            for (int a = 0; a < 6; ++a) aabb_io[6 * i + a] = bb[a];
        }
        for (int a = 0; a < 6; ++a) s.box[i][a] = bb[a];
    }
    __syncthreads();
}

// ---- stage: the canonical LBVH over every primitive and the reference's AABBs -> out_nodes, meta.canonical_depth
__device__ __forceinline__ void canonical_lbvh(BuildLds& s, int i, int n, float4* __restrict__ out_nodes, BuildMeta* __restrict__ out_meta)
{
    reduce_boxes(s, i, i < n);
    s.keys[i] = (i < n) ? (((unsigned long long)morton_of(s, i) << 32) | (unsigned int)i) : ~0ull;
    bitonic_sort<kMaxPrims, kMaxPrims>(s.keys, i);
    morton_tree(s, i, n, false);
    const int leaf0 = n - 1;
    if (i < n) {
        int dep = 0;
        int q = s.parent[leaf0 + i];
        while (q >= 0) {
            ++dep;
            q = s.parent[q];
        }
        atomicMax(&s.canonical_depth, dep);
    }
    for (int k = i; k < 2 * n - 1; k += kMaxPrims) {
        int left, right;
        if (k >= leaf0) {
            left = (int)(s.keys[k - leaf0] & 0xFFFFFFFFu);
            right = -1;
        } else {
            left = s.left[k];
            right = s.right[k];
        }
        out_nodes[2 * k + 0] = make_float4(s.nbox[k][0], s.nbox[k][1], s.nbox[k][2], __int_as_float(left));
        out_nodes[2 * k + 1] = make_float4(s.nbox[k][3], s.nbox[k][4], s.nbox[k][5], __int_as_float(right));
    }
    __syncthreads();   // (the tree in s.nbox is written out: the reductions may use s.red again)
    if (i == 0) out_meta->canonical_depth = s.canonical_depth;
}

// ---- stage: the boxes the fast walk culls with (-> s.box, out_tight, meta.tight_bounds), which primitives are "big" (-> s.flag, the
// return value; n_small = the others), and the bounds of the small ones in s.red for morton_units.
// Any conservative structure returns the same closest hit, so the fast walk's is built for speed:
//  * TIGHT per-shape boxes for rectangles and disks (the reference's CubeBox boxes span a whole cube around a flat shape);
//  * "big" primitives (box spanning >= 36 % of the scene on two axes: room walls, floors) stay out of the tree and are
//    tested first, which also gives every ray an early closest-hit bound for culling the tree;
//  * LBVH over the rest, subtrees collapsed into multi-primitive leaves by a cost budget.
// Spheres and cylinders keep the box the canonical walk uses (the caller's / the CubeBox one): their quadratic loses its
// digits with distance (b*b - 4ac at |o| ~ 2000 radii is good to ~0.1 radius), so from far away the intersection program
// reports hits up to tenths of a unit OFF the surface -- inside the reference's loose box, outside a tight one -- and the
// closest hit must be the reference's arithmetic, not the geometry (tools/fuzz_cameras.py found it: a camera 1200 units
// from the slide scene).  Rectangles and disks divide once (error ~1e-7 of the distance): their tight boxes stand.
__device__ __forceinline__ bool tight_boxes_and_big(BuildLds& s, int i, int n, const PrimIn& P, float big_frac, float* __restrict__ out_tight,
                                                    BuildMeta* __restrict__ out_meta, int& n_small)
{
    if (i < n && (P.type == 2 || P.type == 1)) {
        const float* M = P.M;
        for (int a = 0; a < 3; ++a) {
            const float mx = M[4 * a + 0], mz = M[4 * a + 2], c = M[4 * a + 3];
            float e;  // half extent of the unit shape's image along world axis a
            if (P.type == 2) e = 0.5f * fabsf(mx) + 0.5f * fabsf(mz);   // rectangle |x|,|z| <= 1/2, y = 0
            else e = sqrtf(mx * mx + mz * mz);                          // disk, radius 1 in y = 0
            e = e * 1.00001f + 0.001f;  // rounding headroom + the reference's own pad (AABB_EPSILON)
            s.box[i][a] = c - e;
            s.box[i][3 + a] = c + e;
        }
    }
    __syncthreads();
    if (i < n)   // per primitive: the box the fast walk culls with (the host projects these onto the screen: LaunchParams::hot_mask)
        for (int a = 0; a < 6; ++a) out_tight[6 * i + a] = s.box[i][a];
    reduce_boxes(s, i, i < n);
    if (i < 6) out_meta->tight_bounds[i] = s.red[i][0];  // tight scene bounds: min xyz, max xyz
    bool big = false;
    if (i < n) {
        int wide = 0;
        for (int a = 0; a < 3; ++a)
            if (s.box[i][3 + a] - s.box[i][a] >= big_frac * (s.red[3 + a][0] - s.red[a][0])) ++wide;
        big = wide >= 2;
        s.flag[i] = big ? 1 : 0;
        if (!big) {
            atomicAdd(&s.n_small, 1);
            atomicOr(&s.tmask, 1 << (int)(P.type & 3u));
        }
    }
    __syncthreads();
    n_small = s.n_small;
    reduce_boxes(s, i, i < n && !big);
    return big;
}

// ---- stage: which primitives are the faces of one cube (-> s.used: place within its cube, 0..5, or 0xFF); ends in a barrier.
// Boxes: six consecutive small rectangles that pair up by opposite normals (ShapeFactory::CreateCube emits a cube's faces
// consecutively, shapefactory.cpp) share ONE Morton code, that of the box centre, so that the Karras hierarchy keeps them
// in one subtree and the cost budget (6) turns exactly that subtree into a leaf: whole-box leaves, which pair_test halves.
// Left to the face centroids, Morton order cuts across touching boxes (checkered: leaves of every mix of pairs and singles).
__device__ __forceinline__ void group_cube_faces(BuildLds& s, int i, int n, const PrimIn* __restrict__ prims, const float4* __restrict__ out_prims)
{
    if (i < n) s.used[i] = 0xFF;   // first primitive of the box this one belongs to, relative: 0..5, or 0xFF
    __syncthreads();
    if (i == 0) {
        int a = 0;
        while (a + 6 <= n) {
            bool ok = true;
            for (int k = 0; k < 6 && ok; ++k) ok = prims[a + k].type == 2u && !s.flag[a + k];
            if (ok) {
                unsigned int paired = 0;
                for (int k = 0; k < 6; ++k) {
                    if (paired & (1u << k)) continue;
                    const float4 ra = out_prims[6 * (a + k) + 1];
                    const float la = sqrtf(ra.x * ra.x + ra.y * ra.y + ra.z * ra.z);
                    for (int m = k + 1; m < 6; ++m) {
                        if (paired & (1u << m)) continue;
                        const float4 rb = out_prims[6 * (a + m) + 1];
                        const float lb = sqrtf(rb.x * rb.x + rb.y * rb.y + rb.z * rb.z);
                        if (ra.x * rb.x + ra.y * rb.y + ra.z * rb.z < -0.9999f * la * lb) {
                            paired |= (1u << k) | (1u << m);
                            break;
                        }
                    }
                }
                ok = paired == 0x3Fu;
            }
            if (ok) {
                for (int k = 0; k < 6; ++k) s.used[a + k] = (unsigned char)k;
                a += 6;
            } else {
                a += 1;
            }
        }
    }
    __syncthreads();
}

// ---- stage: the Morton hierarchy that forms the walk's units: small primitives sort by Morton code (big ones after them, in SBT
// order), Karras tree over the n_small with cost weights
__device__ __forceinline__ void morton_units(BuildLds& s, int i, int n, int n_small, bool big, const PrimIn* __restrict__ prims, int leaf_budget)
{
    const bool boxed = i < n && s.used[i] != 0xFF;
    const bool cubic = true;   // (balls -1 %, plateau -1 %, slide -2.5 % against per-axis scaling; nothing lost elsewhere)
    const unsigned int code = (i < n && !big) ? (boxed ? morton_of(s, i - (int)s.used[i], 6, cubic) : morton_of(s, i, 1, cubic)) : 0u;
    s.keys[i] = (i < n) ? ((big ? (0xFFFFFFFEull << 32) : ((unsigned long long)code << 32)) | (unsigned int)i) : ~0ull;
    bitonic_sort<kMaxPrims, kMaxPrims>(s.keys, i);
    if (i < n_small) {
        const int prim = (int)(s.keys[i] & 0xFFFFFFFFu);
        const unsigned int type = prims[prim].type;
        // relative cost of one leaf test vs one box test: rectangles reject on two signs, quadrics need the full transform
        s.wt[n_small - 1 + i] = (type == 2) ? 1 : (type == 1 ? 4 : 32);
    }
    if (i == 0) s.walk_depth = 0;
    __syncthreads();
    if (n_small > 0) morton_tree(s, i, n_small, true);
    const int leaf0 = n_small - 1;
    if (i < n_small) {
        // only ancestors that stay internal (cost above the budget) can push on the fast walk's stack
        int fdep = 0;
        int q = s.parent[leaf0 + i];
        while (q >= 0) {
            if (s.wt[q] > leaf_budget) ++fdep;
            q = s.parent[q];
        }
        atomicMax(&s.walk_depth, fdep);
    }
}

// The slab certificate of one certified cuboid (cuboid_slab, rtgo_device.h), made by the group's thread in pair_and_certify and written
// into the group's records by write_slab.  The frame is the object frame of the group's FIRST face F (rows 0..2 of its record: F is the
// unit square of the plane y = 0 there), not the three pairs' own r1 rows: the walk then transforms the ray with rows it has to read for
// no other reason than this, but they are three rows of ONE record (one address per lane in a leaf).  The frame is affine, not
// orthonormal: a box sheared as a whole (every face's matrix under one affine map) is an axis-aligned box in it and is certified; a
// parallelepiped whose faces carry their own true normals as y axes is not (its first face's rows 0 and 2 are not the other pairs' normals).
struct SlabCert {
    bool ok = false;
    int first = 0;             // the group's first record
    float lo[3], hi[3];        // the box in the frame
    int map = 0;               // three bits per plane: the face's offset in the group; plane = 2 * axis + (0: low, 1: high)
    float rho = 1.0f;          // the largest unit of a face's object-space y, in units of its frame axis: carries cub_mu into the frame
    float thr = 0.0f;          // |d_a| at or below this: the ray counts as parallel to the faces of axis a (2e-5 of the longest axis row, L1)
};
constexpr int kSlabBit = 4;    // in a group's certificate code, beside 1 (box) / 2 (room): the group holds the slab certificate

// Holds iff: the 24 corners of the six faces are corners of one axis-aligned box [lo, hi] in the frame, to kCuboidTol; faces and planes
// are a bijection (each face's centre sits on exactly one plane, mid-box on the other two axes); every face's normal is parallel to its
// axis to 2e-6 (what float products of a rotation leave); everything is finite; and the cuboid's own margin at reach zero, in frame
// units, stays below 2 % of the thinnest slab (a small cuboid far from the origin: its margin is no longer positive for any launch).
// faces: the six primitives in record order; B: the group's own margin coefficient (pair_and_certify).
__device__ __forceinline__ void slab_certify(const int* faces, const PrimIn* __restrict__ prims, const float4* __restrict__ out_prims, float B, SlabCert& sc)
{
    const float4 R[3] = {out_prims[6 * faces[0] + 0], out_prims[6 * faces[0] + 1], out_prims[6 * faces[0] + 2]};
    auto to_frame = [&](float cx, float cy, float cz, float* q) {
        for (int k = 0; k < 3; ++k) q[k] = R[k].x * cx + R[k].y * cy + R[k].z * cz + R[k].w;
    };
    auto corner = [&](const float* M, int c, float* q) {
        const float sx = (c & 1) ? 0.5f : -0.5f, sz = (c & 2) ? 0.5f : -0.5f;
        to_frame(M[0] * sx + M[2] * sz + M[3], M[4] * sx + M[6] * sz + M[7], M[8] * sx + M[10] * sz + M[11], q);
    };
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool ok = true;
    for (int f = 0; f < 6; ++f)
        for (int c = 0; c < 4; ++c) {
            float q[3];
            corner(prims[faces[f]].M, c, q);
            for (int k = 0; k < 3; ++k) {
                lo[k] = fminf(lo[k], q[k]);
                hi[k] = fmaxf(hi[k], q[k]);
                if (!(fabsf(q[k]) < 1e30f)) ok = false;
            }
        }
    float dev = 0.0f, rho = 1.0f, ext = INFINITY;
    for (int k = 0; k < 3; ++k) ext = fminf(ext, hi[k] - lo[k]);
    int map = 0, filled = 0;
    for (int f = 0; f < 6 && ok; ++f) {
        const float* M = prims[faces[f]].M;
        for (int c = 0; c < 4; ++c) {
            float q[3];
            corner(M, c, q);
            for (int k = 0; k < 3; ++k) dev = fmaxf(dev, fminf(fabsf(q[k] - lo[k]), fabsf(hi[k] - q[k])));
        }
        // the face's plane: the axis along which its centre sits on a plane of the box, the other two coordinates mid-box
        float qc[3];
        to_frame(M[3], M[7], M[11], qc);
        int axis = -1, side = 0;
        for (int k = 0; k < 3; ++k) {
            const float e = hi[k] - lo[k];
            const float dl = fabsf(qc[k] - lo[k]), dh = fabsf(hi[k] - qc[k]);
            if (fminf(dl, dh) <= 1e-3f * e) {
                if (axis >= 0) ok = false;   // on two planes at once: not a face of this box
                axis = k;
                side = dl <= dh ? 0 : 1;
            } else if (!(fabsf(qc[k] - 0.5f * (lo[k] + hi[k])) <= 1e-3f * e)) {
                ok = false;
            }
        }
        if (axis < 0) ok = false;
        if (!ok) break;
        const int slot = 2 * axis + side;
        if ((filled >> slot) & 1) ok = false;
        filled |= 1 << slot;
        map |= f << (3 * slot);
        // the face's normal (row 1 of ITS inverse, as a world direction) against the frame axis (row `axis` of F's)
        const float4 nf = out_prims[6 * faces[f] + 1];
        const float4 ax = R[axis];
        const float cxp = nf.y * ax.z - nf.z * ax.y, cyp = nf.z * ax.x - nf.x * ax.z, czp = nf.x * ax.y - nf.y * ax.x;
        const float ln = sqrtf(nf.x * nf.x + nf.y * nf.y + nf.z * nf.z), la = sqrtf(ax.x * ax.x + ax.y * ax.y + ax.z * ax.z);
        if (!(sqrtf(cxp * cxp + cyp * cyp + czp * czp) <= 2e-6f * ln * la)) ok = false;
        // one unit of the face's object-space y, in units of its frame axis: |R_axis . (column 1 of M_f)|
        rho = fmaxf(rho, fabsf(ax.x * M[1] + ax.y * M[5] + ax.z * M[9]));
    }
    float n1max = 0.0f;
    for (int k = 0; k < 3; ++k) n1max = fmaxf(n1max, fabsf(R[k].x) + fabsf(R[k].y) + fabsf(R[k].z));
    const float mu0 = (kCuboidTol + 64.0f * 5.9604645e-8f * B) * rho;   // (rtgo_capi.hip, cub_mu, at reach zero)
    if (ok && filled == 63 && dev <= kCuboidTol && rho < 1e6f && n1max > 0.0f && n1max < 1e30f && ext > 0.0f && mu0 < 0.02f * ext) {
        sc.ok = true;
        for (int k = 0; k < 3; ++k) {
            sc.lo[k] = lo[k];
            sc.hi[k] = hi[k];
        }
        sc.map = map;
        sc.rho = rho;
        sc.thr = 2e-5f * n1max;
    }
}

// ---- stage: record order inside every group the walk scans linearly -- the up-front list and each maximal collapsed leaf (->
// s.order, s.leaf_group, meta.list_group, the margin coefficients, the group's slab certificate); ends in a barrier.
// Rectangles with opposite normals side by side (pair_test), pairs first, the rest after them.  One thread per group.
// Leaves are only paired when EVERY multi-record leaf of the scene pairs up completely (whole boxes): the lanes of a wave
// scan different leaves side by side, and with leaves of both kinds they take turns in the pair loop and the single
// loop (checkered, whose Morton leaves cut across its 64 cubes: +9 %).  The up-front list is scanned by all lanes
// together and is always paired.
__device__ __forceinline__ void pair_and_certify(BuildLds& s, int i, int n, int n_small, const PrimIn* __restrict__ prims, const float4* __restrict__ out_prims,
                                                 int leaf_budget, int cuboids, BuildMeta* __restrict__ out_meta, SlabCert& slab)
{
    const int leaf0 = n_small - 1;
    if (i < n) {
        s.order[i] = (unsigned short)(s.keys[i] & 0xFFFFFFFFu);
        s.used[i] = 0;
        s.leaf_group[i] = 0;   // (morton_tree's arrival counters are no longer needed)
    }
    if (i == 0) {
        out_meta->list_group = 0;
        s.n_unpaired_leaves = 0;
        s.cub_a = 0;
        s.cub_b = 0;
        s.cuboid_leaves = 0;
    }
    __syncthreads();
    int g_lo = 0, g_hi = -1;
    const bool list = (i == kMaxPrims - 1);
    if (list) {
        g_lo = n_small;
        g_hi = n - 1;
    } else if (i < leaf0 && s.wt[i] <= leaf_budget && (s.parent[i] < 0 || s.wt[s.parent[i]] > leaf_budget)) {
        g_lo = s.lo[i];
        g_hi = s.hi[i];
    }
    if (g_hi > g_lo) {
        auto prim_at = [&](int pos) { return (int)(s.keys[pos] & 0xFFFFFFFFu); };
        auto is_rect = [&](int pos) { return prims[prim_at(pos)].type == 2u; };
        auto normal_of = [&](int pos) {   // world normal of a rectangle = row 1 of M^-1 (TransformNormal of (0,1,0))
            const float4 r = out_prims[6 * prim_at(pos) + 1];
            const float l = sqrtf(r.x * r.x + r.y * r.y + r.z * r.z);
            return l > 0.0f ? mk(r.x / l, r.y / l, r.z / l) : mk(0.0f, 0.0f, 0.0f);
        };
        int out = g_lo;
        for (int a = g_lo; a <= g_hi; ++a) {
            if (s.used[a] || !is_rect(a)) continue;
            const v3 na = normal_of(a);
            int bsel = -1;
            float bdot = -0.9999f;
            for (int b = a + 1; b <= g_hi; ++b) {
                if (s.used[b] || !is_rect(b)) continue;
                const float dt = vdot(na, normal_of(b));
                if (dt < bdot) {
                    bdot = dt;
                    bsel = b;
                }
            }
            if (bsel >= 0) {
                s.used[a] = 1;
                s.used[bsel] = 1;
                s.order[out] = (unsigned short)prim_at(a);
                s.order[out + 1] = (unsigned short)prim_at(bsel);
                out += 2;
            }
        }
        const int npairs = (out - g_lo) / 2;
        // Cuboid certificate (cuboid_range): three pairs -- a whole leaf, or the pairs of the up-front list -- are the faces
        // of one box seen from outside when the four corners of every face f lie at or below the plane of every face g of
        // the other two pairs (y_g <= tol in g's object space; y_g is affine, so the whole face does), of one room seen from
        // inside when they lie at or above it.  Checked on the matrices themselves: whatever passes is safe, whatever the
        // shapes were meant to be.  L = how far y_g varies over face f: it carries the rounding of the reference's (u, v) on
        // f into y_g units; A, B: margin = tol + K (A R + B) for rays within R of the origin (rtgo_capi.hip).
        int cert = 0;
        if (cuboids && npairs == 3 && (list || g_hi - g_lo + 1 == 6)) {
            bool outw = true, inw = true;
            float A = 0.0f, B = 0.0f;
            auto n1 = [](const float4 r) { return fabsf(r.x) + fabsf(r.y) + fabsf(r.z); };
            for (int f = 0; f < 6; ++f) {
                const int pf = (int)s.order[g_lo + f];
                const float* M = prims[pf].M;
                const float4 f0 = out_prims[6 * pf + 0], f2 = out_prims[6 * pf + 2];
                const float n1f = fmaxf(n1(f0), n1(f2)), wf = fmaxf(fabsf(f0.w), fabsf(f2.w));
                for (int g = 0; g < 6; ++g) {
                    if ((g >> 1) == (f >> 1)) continue;
                    const float4 r1 = out_prims[6 * (int)s.order[g_lo + g] + 1];
                    float ymax = -INFINITY, ymin = INFINITY;
                    for (int c = 0; c < 4; ++c) {
                        const float sx = (c & 1) ? 0.5f : -0.5f, sz = (c & 2) ? 0.5f : -0.5f;
                        const float cx = M[0] * sx + M[2] * sz + M[3], cy = M[4] * sx + M[6] * sz + M[7], cz = M[8] * sx + M[10] * sz + M[11];
                        const float y = r1.x * cx + r1.y * cy + r1.z * cz + r1.w;
                        ymax = fmaxf(ymax, y);
                        ymin = fminf(ymin, y);
                        if (!(y == y)) outw = inw = false;
                    }
                    outw = outw && ymax <= kCuboidTol;
                    inw = inw && ymin >= -kCuboidTol;
                    const float L = ymax - ymin;
                    A = fmaxf(A, L * n1f + n1(r1));
                    B = fmaxf(B, L * wf + fabsf(r1.w));
                }
            }
            cert = outw ? 1 : ((inw && list) ? 2 : 0);   // (rooms are big: only the list can hold one)
            if (!(A < 1e30f && B < 1e30f)) cert = 0;
            if (cert) {
                atomicMax(&s.cub_a, __float_as_int(A));
                atomicMax(&s.cub_b, __float_as_int(B));
                int faces[6];
                for (int f = 0; f < 6; ++f) faces[f] = (int)s.order[g_lo + f];
                slab_certify(faces, prims, out_prims, B, slab);
                slab.first = g_lo;
                if (slab.ok) cert |= kSlabBit;
            }
        }
        if (list || 2 * npairs == g_hi - g_lo + 1) {
            for (int a = g_lo; a <= g_hi; ++a)
                if (!s.used[a]) s.order[out++] = (unsigned short)prim_at(a);
            if (list) out_meta->list_group = encode_group(npairs, cert);
            else s.leaf_group[i] = encode_group(npairs, cert);
        } else {
            atomicAdd(&s.n_unpaired_leaves, 1);
        }
    }
    __syncthreads();
    if (s.n_unpaired_leaves > 0 && i != kMaxPrims - 1 && g_hi > g_lo) {   // mixed scene: leave every leaf as it was
        for (int a = g_lo; a <= g_hi; ++a) s.order[a] = (unsigned short)(s.keys[a] & 0xFFFFFFFFu);
        s.leaf_group[i] = 0;
        slab.ok = false;
    }
    if (i == 0) {
        out_meta->cub_a = __int_as_float(s.cub_a);
        out_meta->cub_b = __int_as_float(s.cub_b);
    }
    __syncthreads();
}

// ---- stage: the traversal records in the walk's order (inverse rows were written to out_prims by the primitive's own thread in prep_primitives)
__device__ __forceinline__ void write_fprims(const BuildLds& s, int i, int n, const PrimIn* __restrict__ prims, const float4* __restrict__ out_prims,
                                             float4* __restrict__ out_fprims)
{
    if (i < n) {
        const int prim = (int)s.order[i];
        out_fprims[4 * i + 0] = out_prims[6 * prim + 0];
        out_fprims[4 * i + 1] = out_prims[6 * prim + 1];
        out_fprims[4 * i + 2] = out_prims[6 * prim + 2];
        out_fprims[4 * i + 3] = make_float4(__int_as_float((int)prims[prim].type), __int_as_float(prim), 0.0f, 0.0f);
    }
}

// ---- stage: the slab certificates' numbers into the spare words (z, w of row 3) of their groups' records, which write_fprims has just
// written as zeros: record a (a = 0, 1, 2) the bounds of frame axis a, record 3 (map, rho), record 4 (thr, 0); see cuboid_slab
__device__ __forceinline__ void write_slab(int i, const SlabCert& slab, float4* __restrict__ out_fprims)
{
    __syncthreads();   // (write_fprims' rows are another thread's)
    if (slab.ok) {
        const float z[5] = {slab.lo[0], slab.lo[1], slab.lo[2], __int_as_float(slab.map), slab.thr};
        const float w[5] = {slab.hi[0], slab.hi[1], slab.hi[2], slab.rho, 0.0f};
        for (int k = 0; k < 5; ++k) {
            float4 m = out_fprims[4 * (slab.first + k) + 3];
            m.z = z[k];
            m.w = w[k];
            out_fprims[4 * (slab.first + k) + 3] = m;
        }
    }
}

// ---- stage: the walk's UNITS in Morton order (-> s.unit.node, s.unit_wt, s.unit.perm; returns how many).  A unit is a maximal
// collapsed subtree of the Morton hierarchy (cost <= budget: one multi-record leaf whose records are contiguous) or a single primitive;
// the hierarchy only serves to form them.  Ends in the barrier after which s.wt and s.parent are the task queue's.
__device__ __forceinline__ int form_units(BuildLds& s, int i, int n_small, int leaf_budget)
{
    const int leaf0 = n_small - 1;
    auto leafish = [&](int k) { return k >= leaf0 || s.wt[k] <= leaf_budget; };
    __syncthreads();   // (pair_and_certify's readers of s.left and s.keys are done)
    if (i < n_small) s.unit_at[i] = -1;
    __syncthreads();
    for (int k = i; k < 2 * n_small - 1; k += kMaxPrims)
        if (leafish(k) && (s.parent[k] < 0 || s.wt[s.parent[k]] > leaf_budget)) s.unit_at[k >= leaf0 ? k - leaf0 : s.lo[k]] = k;
    __syncthreads();
    if (i == 0) {
        int L = 0;
        for (int pos = 0; pos < n_small; ++pos)
            if (s.unit_at[pos] >= 0) s.unit.node[L++] = (short)s.unit_at[pos];
        s.n_units = L;
    }
    __syncthreads();
    const int L = s.n_units;
    if (i < L) {
        const int k = s.unit.node[i];
        s.unit_wt[i] = s.wt[k] < 1 ? 1 : s.wt[k];
        s.unit.perm[i] = (short)i;
    }
    __syncthreads();
    return L;
}

// the tree the walk uses while it is built and rotated: build_kernel's dynamic LDS, 2 * kMaxPrims nodes of (box 24 B + two links + parent)
__device__ __forceinline__ SahTree carve_tree(unsigned char* dyn)
{
    float* box = reinterpret_cast<float*>(dyn);
    int* left = reinterpret_cast<int*>(box + 6 * 2 * kMaxPrims);
    return SahTree{box, left, left + 2 * kMaxPrims, left + 4 * kMaxPrims};
}

// ---- stage: the tree the walk uses, a top-down surface-area-heuristic build over the units (sah_build; W = leaf-test cost weights).
// Above the units the Morton prefixes are a poor guide for rays (they know nothing of box areas), and any tree over the same leaves
// returns the same closest hit, so the topology is rebuilt.  (Rotations of the Morton tree gave balls -4.5 %; this build ... see DESIGN.)
// Returns the number of nodes.
__device__ __forceinline__ int sah_tree(BuildLds& s, int i, int n_small, int n_units, const SahTree& t)
{
    const int leaf0 = n_small - 1;
    if (i == 0) s.walk_depth = 0;
    return sah_build<kMaxPrims, false>(
        i, n_units, 2 * kMaxPrims, [&](int u, int c) { return s.nbox[s.unit.node[u]][c]; }, [&](int u) { return s.unit_wt[u]; }, s.unit.perm, s.unit.tmp,
        s.sfx, SahQueue<short>{s.tq.node, s.tq.lo, s.tq_hi}, t, s.sah, [&](int node, int u) {
            const int k = s.unit.node[u];
            const int first = k >= leaf0 ? k - leaf0 : (int)s.lo[k];
            const int cnt = k >= leaf0 ? 1 : (int)s.hi[k] - (int)s.lo[k] + 1;
            t.left[node] = first;
            t.right[node] = encode_leaf_link(cnt, k >= leaf0 ? 0 : s.leaf_group[k]);
        });
}

// ---- stage: tree rotations (Kensler 2008) as a second pass: the top-down build is greedy, and a node may still gain from trading one
// child for a grandchild on the other side when that shrinks the grandchild's parent.  One thread; a handful of sweeps.  Ends in a barrier.
__device__ __forceinline__ void rotate_tree(BuildLds& s, int i, int n_nodes, const SahTree& t)
{
    if (i == 0 && n_nodes > 3) {
        auto internal = [&](int k) { return t.right[k] >= 0; };
        auto area2 = [&](int a, int b) {
            float e[3];
            for (int ax = 0; ax < 3; ++ax) e[ax] = fmaxf(t.box[6 * a + 3 + ax], t.box[6 * b + 3 + ax]) - fminf(t.box[6 * a + ax], t.box[6 * b + ax]);
            return e[0] * e[1] + e[1] * e[2] + e[2] * e[0];
        };
        auto refit = [&](int k) {
            const int A = t.left[k], B = t.right[k];
            for (int ax = 0; ax < 3; ++ax) {
                t.box[6 * k + ax] = fminf(t.box[6 * A + ax], t.box[6 * B + ax]);
                t.box[6 * k + 3 + ax] = fmaxf(t.box[6 * A + 3 + ax], t.box[6 * B + 3 + ax]);
            }
        };
        for (int pass = 0; pass < 6; ++pass) {
            int changed = 0;
            for (int N = 0; N < n_nodes; ++N) {
                if (!internal(N)) continue;
                const int A = t.left[N], B = t.right[N];
                float best = 0.0f;
                int which = 0;   // 1: B <-> left(A), 2: B <-> right(A), 3: A <-> left(B), 4: A <-> right(B)
                if (internal(A)) {
                    const float a0 = area2(A, A);
                    const float g1 = a0 - area2(B, t.right[A]), g2 = a0 - area2(t.left[A], B);
                    if (g1 > best) { best = g1; which = 1; }
                    if (g2 > best) { best = g2; which = 2; }
                }
                if (internal(B)) {
                    const float a0 = area2(B, B);
                    const float g3 = a0 - area2(A, t.right[B]), g4 = a0 - area2(t.left[B], A);
                    if (g3 > best) { best = g3; which = 3; }
                    if (g4 > best) { best = g4; which = 4; }
                }
                if (which == 0 || !(best > 1e-6f * area2(N, N))) continue;
                if (which <= 2) {
                    const int g = which == 1 ? t.left[A] : t.right[A];   // the grandchild that moves up
                    if (which == 1) t.left[A] = B; else t.right[A] = B;
                    t.parent[B] = A;
                    t.right[N] = g;
                    t.parent[g] = N;
                    refit(A);
                } else {
                    const int g = which == 3 ? t.left[B] : t.right[B];
                    if (which == 3) t.left[B] = A; else t.right[B] = A;
                    t.parent[A] = B;
                    t.left[N] = g;
                    t.parent[g] = N;
                    refit(B);
                }
                ++changed;
            }
            if (!changed) break;
        }
        s.walk_depth = 0;
    }
    __syncthreads();
}

// ---- stage: the tree -> out_fnodes, and what the host needs to know about it -> the meta words
__device__ __forceinline__ void write_fnodes_and_meta(BuildLds& s, int i, int n_small, int n_nodes, const SahTree& t, float4* __restrict__ out_fnodes,
                                                      BuildMeta* __restrict__ out_meta)
{
    for (int k = i; k < n_nodes; k += kMaxPrims) {
        out_fnodes[2 * k + 0] = make_float4(t.box[6 * k + 0], t.box[6 * k + 1], t.box[6 * k + 2], __int_as_float(t.left[k]));
        out_fnodes[2 * k + 1] = make_float4(t.box[6 * k + 3], t.box[6 * k + 4], t.box[6 * k + 5], __int_as_float(t.right[k]));
        if (t.right[k] < 0) {   // a leaf: internal nodes above it = stack entries the walk can need on the way
            if (leaf_cuboid(t.right[k]) != 0) atomicAdd(&s.cuboid_leaves, 1);
            int d = 0;
            for (int q = t.parent[k]; q >= 0; q = t.parent[q]) ++d;
            atomicMax(&s.walk_depth, d);
        }
    }
    __syncthreads();
    if (i == 0) {
        out_meta->cuboid_leaves = s.cuboid_leaves;
        out_meta->walk_depth = s.walk_depth;
        out_meta->n_small = n_small;
        out_meta->n_fnodes = n_nodes;
        out_meta->tree_types = s.tmask;
    }
}

// Scene preparation + canonical LBVH + the fast walk's structure, one workgroup (n <= kMaxPrims).
// Outputs.  out_nodes: (2n-1) x 2 float4 canonical LBVH; out_prims: n x 6 float4 (SBT order); aabb_io: n x 6 floats (read when
// have_aabb, else written); out_fnodes / out_fprims: the fast walk's tree (2*units-1 nodes) and Morton-ordered records
// (small primitives first, then the "big" ones that are tested up front);
// out_tight: n x 6 floats, the fast walk's box of every primitive (SBT order); out_frames: n x 2 float4 shading frames; out_meta: BuildMeta.
__global__ __launch_bounds__(kMaxPrims) void build_kernel(const PrimIn* __restrict__ prims, float* __restrict__ aabb_io, int have_aabb, int n,
                                                          float4* __restrict__ out_nodes, float4* __restrict__ out_prims, float4* __restrict__ out_fnodes,
                                                          float4* __restrict__ out_fprims, int leaf_budget, float big_frac, BuildMeta* __restrict__ out_meta,
                                                          float* __restrict__ out_tight, int cuboids, float4* __restrict__ out_frames)
{
    __shared__ BuildLds s;
    extern __shared__ __attribute__((aligned(16))) unsigned char build_dyn[];
    const SahTree tree = carve_tree(build_dyn);
    const int i = threadIdx.x;
    if (i == 0) {
        s.canonical_depth = 0;
        s.n_small = 0;
        s.tmask = 0;
    }
    PrimIn P;
    prep_primitives(s, i, n, prims, aabb_io, have_aabb, out_prims, out_frames, P);
    canonical_lbvh(s, i, n, out_nodes, out_meta);
    int n_small;
    const bool big = tight_boxes_and_big(s, i, n, P, big_frac, out_tight, out_meta, n_small);
    group_cube_faces(s, i, n, prims, out_prims);
    morton_units(s, i, n, n_small, big, prims, leaf_budget);
    SlabCert slab;
    pair_and_certify(s, i, n, n_small, prims, out_prims, leaf_budget, cuboids, out_meta, slab);
    write_fprims(s, i, n, prims, out_prims, out_fprims);
    write_slab(i, slab, out_fprims);
    const int n_units = form_units(s, i, n_small, leaf_budget);
    const int n_nodes = sah_tree(s, i, n_small, n_units, tree);
    rotate_tree(s, i, n_nodes, tree);
    write_fnodes_and_meta(s, i, n_small, n_nodes, tree, out_fnodes, out_meta);
}

}  // namespace rtgo
