// rtgo_capi.hip -- the C ABI of include/rtgo.h over the gfx950 kernels of rtgo_device.h.
// Host side of the drop-in boundary: where the reference's Renderer calls the OptiX host API, a port calls these.
// There is no CPU fallback anywhere in this file: every path ends in a HIP launch or an error code.
#include "rtgo_ctx.h"

static_assert(sizeof(rtgo_prim) == sizeof(PrimIn), "rtgo_prim layout");
static_assert(sizeof(rtgo_prim) == 108, "rtgo_prim is type + HitGroupData (104 B, params.h:103-110)");
static_assert(sizeof(rtgo_light) == sizeof(LightRec) && sizeof(rtgo_light) == 64, "SurfaceLight is 64 B");
static_assert(sizeof(rtgo_aabb) == 24, "OptixAabb is 24 B");
static_assert(RTGO_MAX_PRIMS == kMaxPrims && RTGO_MAX_LIGHTS == kMaxLights, "limits");
static_assert(RTGO_MAX_SCENE_PRIMS <= (1 << 29), "2n-1 nodes of 32 bytes and their int indices stay within int range");

// dynamic LDS of build_kernel: the fast walk's tree while it is built and rotated (2 * kMaxPrims nodes x (box 24 B + two links + parent))
static constexpr size_t kBuildDynLds = (size_t)2 * kMaxPrims * (6 * sizeof(float) + 3 * sizeof(int));

// every instantiation of the megakernel, in one place: rtgo_create raises the dynamic-LDS limit of each, rtgo_launch picks one
using RenderKernel = void (*)(const LaunchParams, const float4*);
struct RenderKernelEntry {
    bool path, canon, stream;
    int wpe;
    bool count, frames;
    RenderKernel fn;
    bool grid = false;
    bool global = false;   // the canonical walk over a scene in global memory (rtgo_set_large_scene)
    bool batch = false;    // render_frames_kernel: the frames of rtgo_launch_frames in one launch
    bool pair = false;     // render_pair_kernel: the straight-line walk of a two-leaf tree (fast_pair)
};
#define RTGO_K(P, S, W, T) {P, S, T, W, S, false, render_kernel<P, S, W, T>}
#define RTGO_KF(W, T) {true, false, T, W, false, true, render_kernel<true, false, W, T, false, true>}
#define RTGO_KG(P, W, T) {P, false, T, W, false, false, render_kernel<P, false, W, T, false, false, true>, true}
#define RTGO_KL(P, C) {P, true, false, 4, C, false, render_kernel<P, true, 4, false, C, false, false, true>, false, true}
#define RTGO_KB(P, W, F) {P, false, false, W, false, F, render_frames_kernel<P, W, F>, false, false, true}
#define RTGO_KP(W) {true, false, false, W, false, true, render_pair_kernel<W>, false, false, false, true}
static const RenderKernelEntry kRenderKernels[] = {
    RTGO_K(true, false, 4, false),  RTGO_K(true, false, 5, false),    // path mode, fast walk
    RTGO_K(false, false, 4, false), RTGO_K(false, false, 5, false),   // distributed mode, fast walk
    RTGO_K(true, false, 4, true),   RTGO_K(true, false, 5, true),     // ... more than 16 spp: lanes stream through their samples
    RTGO_K(false, false, 4, true),  RTGO_K(false, false, 5, true),
    RTGO_K(true, true, 4, false),   RTGO_K(false, true, 4, false),    // canonical walk + V/T/h counters (collect_stats launches)
    {true, true, false, 4, false, false, render_kernel<true, true, 4, false, false>},     // canonical walk alone: launches beyond the far-field guard
    {false, true, false, 4, false, false, render_kernel<false, true, 4, false, false>},
    RTGO_KF(4, false), RTGO_KF(5, false), RTGO_KF(4, true), RTGO_KF(5, true),               // path mode, fast walk, scenes of flat primitives only: shading frames from LDS
    RTGO_KF(6, false),                                                                      // ... at 6 waves/SIMD: the only combination that fits 80 VGPRs without scratch
    RTGO_KG(true, 4, false), RTGO_KG(true, 5, false), RTGO_KG(true, 4, true), RTGO_KG(true, 5, true),       // fast walk over the uniform grid instead of the tree (fast_grid)
    RTGO_KG(false, 4, false), RTGO_KG(false, 5, false), RTGO_KG(false, 4, true), RTGO_KG(false, 5, true),
    RTGO_KL(true, false), RTGO_KL(false, false), RTGO_KL(true, true), RTGO_KL(false, true),   // scenes of rtgo_set_large_scene: timed, collect_stats
    RTGO_KB(true, 4, false), RTGO_KB(true, 5, false), RTGO_KB(true, 4, true), RTGO_KB(true, 5, true),   // several frames per launch (rtgo_launch_frames): lock-step, over a tree
    RTGO_KB(false, 4, false), RTGO_KB(false, 5, false),
    RTGO_KP(6), RTGO_KP(5),   // path mode, flat scene, lock-step, a tree of two cuboid leaves (cornell): the bench launch, and a band share of it
    {true, false, false, 7, false, true, render_pair7_kernel, false, false, false, true},   // ... at 7 waves/SIMD (72 VGPRs): launches of many units per wave
};
#undef RTGO_K
#undef RTGO_KF
#undef RTGO_KG
#undef RTGO_KL
#undef RTGO_KB
#undef RTGO_KP
static RenderKernel find_kernel(bool path, bool canon, int wpe, bool stream, bool count, bool frames, bool grid, bool global = false, bool batch = false, bool pair = false)
{
    for (const RenderKernelEntry& e : kRenderKernels)
        if (e.path == path && e.canon == canon && e.wpe == (canon ? 4 : wpe) && e.stream == (canon ? false : stream) && e.count == (canon && count) &&
            e.frames == (frames && path && !canon) && e.grid == (grid && !canon) && e.global == (global && canon) && e.batch == batch && e.pair == pair)
            return e.fn;
    return nullptr;
}

// the pair kernel of `wpe` waves with the slab test in place of cuboid_range (cuboid_slab), where one exists: seven waves only -- six- and
// five-waves forms were not built (profiles/r22a)
static RenderKernel find_slab_kernel(int wpe) { return wpe == 7 ? render_slab7_kernel : nullptr; }

// ... and the form of it that is compiled for 16 samples per pixel in workgroups of 256 threads (UNIT16, rtgo_render_body.inc): the kernel takes
// both for granted, so the launch has to have them
static RenderKernel find_unit16_kernel(int wpe, uint32_t nn, int block) { return (wpe == 7 && nn == 16u && block == 256) ? render_unit16_kernel : nullptr; }

// ... and the form of THAT whose room is steered in world axes (ROOMW, room_world): for launches that would take render_unit16_kernel
static RenderKernel find_roomw_kernel(RenderKernel unit16) { return unit16 == render_unit16_kernel ? render_roomw_kernel : nullptr; }

// window rows below y that this rank owns under the band interleave
static uint32_t owned_rows_below(uint32_t y, uint32_t band_h, uint32_t n_ranks, uint32_t rank)
{
    if (n_ranks <= 1) return y;
    const uint32_t full = y / band_h, part = y % band_h;
    const uint32_t owned_full = full > rank ? (full - rank - 1) / n_ranks + 1 : 0;
    return owned_full * band_h + ((full % n_ranks == rank) ? part : 0);
}

static inline uint32_t passes_of(uint32_t nn) { return (nn + (uint32_t)kSamplesPerPass - 1u) / (uint32_t)kSamplesPerPass; }

// Far-field guard of rtgo_launch: the fast walk serves launches whose rays stay where every traversal returns the same closest hit;
// beyond, the canonical walk ("far field").  Set from tools/fuzz_farfield.py (-DRTGO_CMPWALK build: both walks on
// every ray; profiles/r03a/farfield_*.log: 3.6e9 rays over translated scenes and eye distances of 10 .. 3000 units):
//   kGuardQuadric  max over spheres / cylinders of Q = D^2 smax / smin^2 (D: farthest ray origin -- eye or scene bounds -- to the
//                  primitive; s: its axis scales).  A quadric's reported hit leaves its surface by ~2^-25 Q (b^2 - 4ac cancels), and
//                  the reference's own box (AABB_EPSILON = 1e-3, primitive.cpp:16) no longer holds it from Q ~ 2^25 * 1e-3 = 33554 on.
//                  Measured: no disagreement in 2.1e9 rays with Q < 32000, the first at Q = 33130; EVERY disagreement found, at any
//                  distance, involves a sphere or a cylinder.  8000 = that onset with a safety factor of 4 on the error.
//   kGuardReach    max(|scene bounds|, |eye|), world units, for what is linear in the coordinates (rectangles, disks, the cuboid
//                  margin): 500.  Flat primitives never disagreed up to the largest reach fuzzed (5000): a factor of 10.
static constexpr float kGuardReach = 500.0f;
static constexpr float kGuardQuadric = 8000.0f;

// The environment knobs of a scene set-up or a launch (rtgo_ctx.h has the readers): each rtgo_set_scene and rtgo_launch reads them afresh
struct Knobs {
    bool debug = std::getenv("RTGO_DEBUG") != nullptr;              // a line per scene and launch on stderr
    bool no_frames = std::getenv("RTGO_NO_FRAMES") != nullptr;      // flat scenes compute N and the sampling tangent per hit
    bool no_cuboid = std::getenv("RTGO_NO_CUBOID") != nullptr;      // the build certifies no cuboids
    bool no_last_emitter = std::getenv("RTGO_NO_LAST_EMITTER") != nullptr;   // launches go without the last-ray certificate
    bool no_pair = std::getenv("RTGO_NO_PAIR") != nullptr;          // two-leaf trees are walked by fast_tree like every other (render_pair_kernel is not taken)
    bool no_slab = std::getenv("RTGO_NO_SLAB") != nullptr;          // the pair kernels keep cuboid_range (render_slab7_kernel is not taken)
    bool no_unit16 = std::getenv("RTGO_NO_UNIT16") != nullptr;      // 16 spp launches of the slab kernel keep render_slab7_kernel (render_unit16_kernel is not taken)
    bool no_roomw = std::getenv("RTGO_NO_ROOMW") != nullptr;        // the room keeps its frame's slab test (render_roomw_kernel is not taken: render_unit16_kernel runs)
    bool pin_big = std::getenv("RTGO_BIG_PERCENT") != nullptr;      // one fast-walk structure, of big_percent (else 36 % and 15 %)
    unsigned int big_percent = env_uint("RTGO_BIG_PERCENT", 36);
    unsigned int max_wpe = env_uint("RTGO_MAX_WPE", 0);             // cap of the waves-per-SIMD variant; 0: by the work
    unsigned int grid_min = env_uint("RTGO_GRID_MIN", 64);          // no grid for fewer small primitives ...
    float grid_max_dup = env_float("RTGO_GRID_MAX_DUP", 3.0f);      // ... or more list entries per primitive
    float guard_quadric;                                            // RTGO_GUARD_QUADRIC: the far-field guard's threshold
    int tree = -1, stream = -1;   // RTGO_TREE=0/1/2, RTGO_STREAM=0/1: pin the 36 % / 15 % tree / the grid, the lock-step / streaming loop
    int leaf_budget = -1;         // RTGO_LEAF_BUDGET, -1: unset or out of range
    int grid_dims[3] = {0, 0, 0}; // RTGO_GRID_DIMS=nx,ny,nz instead of the cost model's resolution
    Knobs()
    {
        static const float quadric = env_float("RTGO_GUARD_QUADRIC", kGuardQuadric);   // (read once per process)
        guard_quadric = quadric;
        if (const char* v = std::getenv("RTGO_TREE")) tree = v[0] == '1' ? 1 : (v[0] == '2' ? 2 : 0);
        if (const char* v = std::getenv("RTGO_STREAM")) stream = v[0] != '0' ? 1 : 0;
        if (const char* v = std::getenv("RTGO_LEAF_BUDGET")) leaf_budget = std::atoi(v) >= 0 && std::atoi(v) <= 16 * kMaxPrims ? std::atoi(v) : -1;
        int d[3];
        if (const char* v = std::getenv("RTGO_GRID_DIMS"))
            if (std::sscanf(v, "%d,%d,%d", &d[0], &d[1], &d[2]) == 3)
                for (int a = 0; a < 3; ++a) grid_dims[a] = d[a] < 1 ? 1 : (d[a] > 32 ? 32 : d[a]);
    }
};

// Window rectangle [wx0, wx1) x [wy0, wy1) that can contain geometry: the 8 corners of the scene's tight bounds through the
// pinhole camera of the raygen program (d = dx*U + dy*V + W, kernel.cu:214-220; a sample of pixel (x, y) has dx, dy inside
// that pixel's square).  Conservative: padded by two pixels, and the whole window whenever a corner is not in front of the
// eye.  The kernel traces nothing for pixels outside it (their primary rays cannot reach the bounds: they are misses).
struct Rect { uint32_t x0, x1, y0, y1; };
static Rect box_screen_rect(const float* bounds, const LaunchParams& p)
{
    const Rect whole = {0, p.w, 0, p.h};
    const double uu = (double)p.U.x * p.U.x + (double)p.U.y * p.U.y + (double)p.U.z * p.U.z;
    const double vv = (double)p.V.x * p.V.x + (double)p.V.y * p.V.y + (double)p.V.z * p.V.z;
    const double ww = (double)p.Wv.x * p.Wv.x + (double)p.Wv.y * p.Wv.y + (double)p.Wv.z * p.Wv.z;
    if (!(uu > 0 && vv > 0 && ww > 0)) return whole;
    // the three axes must be orthogonal for the projection below (they are for every Camera: Camera.cpp:55-69); else: no culling
    const double uv = (double)p.U.x * p.V.x + (double)p.U.y * p.V.y + (double)p.U.z * p.V.z;
    const double uw = (double)p.U.x * p.Wv.x + (double)p.U.y * p.Wv.y + (double)p.U.z * p.Wv.z;
    const double vw = (double)p.V.x * p.Wv.x + (double)p.V.y * p.Wv.y + (double)p.V.z * p.Wv.z;
    const double tol = 1e-5;
    if (uv * uv > tol * tol * uu * vv || uw * uw > tol * tol * uu * ww || vw * vw > tol * tol * vv * ww) return whole;
    double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
    for (int k = 0; k < 8; ++k) {
        const double px = bounds[(k & 1) ? 3 : 0] - p.eye.x, py = bounds[(k & 2) ? 4 : 1] - p.eye.y, pz = bounds[(k & 4) ? 5 : 2] - p.eye.z;
        const double a = (px * p.U.x + py * p.U.y + pz * p.U.z) / uu, b = (px * p.V.x + py * p.V.y + pz * p.V.z) / vv;
        const double w = (px * p.Wv.x + py * p.Wv.y + pz * p.Wv.z) / ww;
        if (!(w > 1e-3)) return whole;  // a corner beside or behind the eye: no useful rectangle
        const double sx = (a / w + 1.0) * 0.5 * p.W, sy = (b / w + 1.0) * 0.5 * p.H;
        x0 = sx < x0 ? sx : x0;
        x1 = sx > x1 ? sx : x1;
        y0 = sy < y0 ? sy : y0;
        y1 = sy > y1 ? sy : y1;
    }
    if (!(x0 <= x1 && y0 <= y1)) return whole;   // NaN bounds
    // to window pixels, padded, clamped
    auto clampd = [](double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); };
    Rect r = {(uint32_t)clampd(x0 - 2.0 - p.x0, 0.0, p.w), (uint32_t)clampd(x1 + 3.0 - p.x0, 0.0, p.w),
              (uint32_t)clampd(y0 - 2.0 - p.y0, 0.0, p.h), (uint32_t)clampd(y1 + 3.0 - p.y0, 0.0, p.h)};
    if (r.x1 <= r.x0 || r.y1 <= r.y0) r = Rect{0, 0, 0, 0};   // the scene is off screen
    return r;
}

extern "C" {

// diagnostic (tests, tools; not part of include/rtgo.h): whether the last rtgo_launch read pre-hashed pixel seeds (bit 0) and
// whether it wrote the next frame's (bit 1)
extern "C" int rtgo_debug_seeds(rtgo_ctx* c, uint32_t* out)
{
    if (!c || !out) return fail(c, RTGO_E_INVALID, "rtgo_debug_seeds: NULL argument");
    *out = c->seeds_last;
    return RTGO_OK;
}

// diagnostic (tests, tools; not part of include/rtgo.h): what rtgo_set_scene's grid build came to -- {has one, nx, ny, nz, list entries, bytes}
extern "C" int rtgo_debug_grid(rtgo_ctx* c, int32_t out[6])
{
    if (!c || !out) return RTGO_E_INVALID;
    const AnalyticScene::Grid& g = c->scene.grid;
    out[0] = g.have ? 1 : 0;
    out[1] = g.gp.nx;
    out[2] = g.gp.ny;
    out[3] = g.gp.nz;
    out[4] = g.entries;
    out[5] = g.n_nodes * 32;
    return RTGO_OK;
}

// FNV-1a (64 bit) over `bytes` of device memory, continuing from h
static int digest_device(rtgo_ctx* c, const void* d, size_t bytes, uint64_t& h)
{
    std::vector<unsigned char> host(d ? bytes : 0);
    if (!host.empty()) RTGO_HIP(c, hipMemcpy(host.data(), d, host.size(), hipMemcpyDeviceToHost));
    for (const unsigned char b : host) h = (h ^ b) * 0x100000001B3ull;
    return RTGO_OK;
}
static void digest_host(const void* p, size_t bytes, uint64_t& h)
{
    for (size_t k = 0; k < bytes; ++k) h = (h ^ static_cast<const unsigned char*>(p)[k]) * 0x100000001B3ull;
}

}  // extern "C" (a template follows)

// One thing the builds wrote for the context's current scene, over the range the build defines (not allocation slack): its pieces in
// order, each a range of device memory (dev; a null pointer counts as empty) or bytes the host holds (dev = nullptr, host).
struct BuildSpan {
    std::string name;
    struct Piece {
        const void* dev;
        size_t bytes;
        std::vector<unsigned char> host;
    };
    std::vector<Piece> pieces;
    template <class T>
    BuildSpan& device(const T* p, size_t count)
    {
        pieces.push_back({p, p ? count * sizeof(T) : 0, {}});
        return *this;
    }
    BuildSpan& host(const void* p, size_t bytes)
    {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        pieces.push_back({nullptr, bytes, std::vector<unsigned char>(b, b + bytes)});
        return *this;
    }
    size_t bytes() const
    {
        size_t n = 0;
        for (const Piece& q : pieces) n += q.bytes;
        return n;
    }
};

// The ordered list of spans of rtgo_debug_build_digest and rtgo_debug_read_build.
//   analytic (whitted = 0): nodes, prims, frames, tight, aabb; then for tree[0] and tree[1]: fnodes (2 * n_fnodes float4), fprims, the
//     decoded meta fields {canonical depth, fast_depth, n_small, n_fnodes, n_big_pairs, list_cub, cuboid_groups, tree_spheres, bounds[6],
//     cub_a, cub_b, slab_list, slab_leaves}.  A scene of rtgo_set_large_scene has the first five only (frames and tight boxes empty).  Then, in the clear:
//     scene.info {n_prims, large, have_alt, has a grid}, tree0.meta / tree1.meta (BuildMeta's words), grid.params (GridParams, then
//     {bytes, list entries}), grid.image.
//   whitted (whitted = 1), one mesh: recs (4 * n_recs float4), qrecs (2 * n_recs), tris, tidx, grid {grid_lo, grid_step}, counts {n_recs,
//     walk_depth}; then meta (WhittedBuildMeta's words, then {triangles, vertices}).
//     An instanced scene: per mesh recs, qrecs (each over the ranges its builds wrote, in build order), tris, tidx, {root, depth, n_recs
//     of each build}; then the top level's recs and inst, then clusters.  Then, in the clear: per mesh its info {rec_base, tri_base,
//     vert_base, root, depth, clustered, n_tris, builds, then per build rec0, n_recs, tri0 and WhittedBuildMeta's words}, and top.meta
//     (WhittedBuildMeta's words of the top level, then {n_recs, n_instances, the scene's walk_depth, mesh_depth}).
static int whitted_refresh_host(rtgo_ctx* c);   // (rtgo_whitted_host.h: top.meta's grid may wait on the device for its first reader)

static int build_spans(rtgo_ctx* c, int whitted, std::vector<BuildSpan>& out)
{
    if (whitted)
        if (const int rc = whitted_refresh_host(c)) return rc;
    auto span = [&](const std::string& name) -> BuildSpan& {
        out.push_back(BuildSpan{name, {}});
        return out.back();
    };
    if (!whitted) {
        const AnalyticScene& sc = c->scene;
        const size_t n = sc.n_prims;
        if (n == 0) return fail(c, RTGO_E_STATE, "rtgo_debug_build_digest: no scene");
        span("nodes").device(sc.d_nodes.get(), (2 * n - 1) * 2);
        span("prims").device(sc.d_prims.get(), n * 6);
        span("frames").device(sc.d_frames.get(), sc.large ? 0 : n * 2);
        span("tight").device(sc.d_tight.get(), sc.large ? 0 : n * 6);
        span("aabb").device(sc.d_aabb.get(), n * 6);
        for (int k = 0; k < 2 && !sc.large; ++k) {
            const AnalyticScene::FastTree& t = sc.tree[k];
            const bool have = t.d_fprims.get() != nullptr;
            const std::string pre = "tree" + std::to_string(k) + ".";
            span(pre + "fnodes").device(t.d_fnodes.get(), have ? (size_t)2 * t.n_fnodes : 0);
            span(pre + "fprims").device(t.d_fprims.get(), have ? n * 4 : 0);
            const int ints[] = {sc.lbvh_depth, t.fast_depth, t.n_small, t.n_fnodes, t.n_big_pairs, t.list_cub, t.cuboid_groups, t.tree_spheres};
            const float floats[] = {t.cub_a, t.cub_b};
            const int slab[] = {t.slab_list ? 1 : 0, t.slab_leaves};
            span(pre + "decoded").host(ints, sizeof ints).host(sc.bounds, sizeof sc.bounds).host(floats, sizeof floats).host(slab, sizeof slab);
        }
        const int info[] = {(int)n, sc.large ? 1 : 0, sc.have_alt ? 1 : 0, sc.grid.have ? 1 : 0};
        span("scene.info").host(info, sizeof info);
        for (int k = 0; k < 2 && !sc.large; ++k) {
            const AnalyticScene::FastTree& t = sc.tree[k];
            span("tree" + std::to_string(k) + ".meta").host(&t.meta, t.d_fprims.get() ? sizeof t.meta : 0);
        }
        const AnalyticScene::Grid& g = sc.grid;
        const int gi[] = {g.have ? g.n_nodes * 32 : 0, g.have ? g.entries : 0};
        span("grid.params").host(&g.gp, sizeof g.gp).host(gi, sizeof gi);
        span("grid.image").device(g.have ? g.d.get() : nullptr, (size_t)g.n_nodes * 32);
    } else {
        const WhittedMesh& wm = c->wm;
        if (wm.triangles == 0) return fail(c, RTGO_E_STATE, "rtgo_debug_build_digest: no mesh");
        if (!wm.instanced) {
            span("recs").device(wm.recs.get(), (size_t)4 * wm.meta.n_recs);
            span("qrecs").device(wm.qrecs.get(), (size_t)2 * wm.meta.n_recs);
            span("tris").device(wm.tris.get(), (size_t)3 * wm.triangles);
            span("tidx").device(wm.tidx.get(), (size_t)wm.triangles);
            span("grid").host(&wm.meta.grid_lo, sizeof wm.meta.grid_lo).host(&wm.meta.grid_step, sizeof wm.meta.grid_step);
            const int ints[] = {wm.meta.n_recs, wm.walk_depth};
            span("counts").host(ints, sizeof ints);
            const int sizes[] = {wm.triangles, wm.n_vertices};
            span("meta").host(&wm.meta, sizeof wm.meta).host(sizes, sizeof sizes);
        } else {
            for (size_t k = 0; k < wm.meshes.size(); ++k) {
                const WhittedMeshInfo& mi = wm.meshes[k];
                const std::string pre = "mesh" + std::to_string(k) + ".";
                BuildSpan recs{pre + "recs", {}}, qrecs{pre + "qrecs", {}}, counts{pre + "counts", {}};
                counts.host(&mi.root, sizeof mi.root).host(&mi.depth, sizeof mi.depth);
                for (const WhittedMeshInfo::Built& b : mi.built) {
                    recs.device(wm.recs.get() + 4 * (size_t)b.rec0, (size_t)4 * b.n_recs);
                    if (b.tri0 >= 0) qrecs.device(wm.qrecs.get() + 2 * (size_t)b.tri0, (size_t)2 * b.n_recs);
                    counts.host(&b.n_recs, sizeof b.n_recs);
                }
                out.push_back(recs);
                out.push_back(qrecs);
                span(pre + "tris").device(wm.tris.get() + 3 * (size_t)mi.tri_base, (size_t)3 * mi.n_tris);
                span(pre + "tidx").device(wm.tidx.get() + mi.tri_base, (size_t)mi.n_tris);
                out.push_back(counts);
            }
            span("top.recs").device(wm.top.recs.get(), (size_t)4 * wm.top.n_recs);
            span("top.inst").device(wm.top.inst.get(), (size_t)wm.top.n_instances);
            span("clusters").device(wm.clusters.get(), wm.clusters.size());
            for (size_t k = 0; k < wm.meshes.size(); ++k) {
                const WhittedMeshInfo& mi = wm.meshes[k];
                const int head[] = {mi.rec_base, mi.tri_base, mi.vert_base, mi.root, mi.depth, mi.clustered ? 1 : 0, mi.n_tris, (int)mi.built.size()};
                BuildSpan& s = span("mesh" + std::to_string(k) + ".info").host(head, sizeof head);
                for (const WhittedMeshInfo::Built& b : mi.built) {
                    const int w[] = {b.rec0, b.n_recs, b.tri0};
                    s.host(w, sizeof w).host(&b.meta, sizeof b.meta);
                }
            }
            const int top[] = {wm.top.n_recs, wm.top.n_instances, wm.walk_depth, wm.mesh_depth};
            span("top.meta").host(&wm.top.meta, sizeof wm.top.meta).host(top, sizeof top);
        }
    }
    return RTGO_OK;
}

extern "C" {

// diagnostic (tools/build_digest.py; not part of include/rtgo.h): one FNV-1a digest per span of build_spans; *n_out = how many (at most
// `cap` are stored)
extern "C" int rtgo_debug_build_digest(rtgo_ctx* c, int whitted, uint64_t* out, uint32_t cap, uint32_t* n_out)
{
    if (!c || !out || !n_out) return fail(c, RTGO_E_INVALID, "rtgo_debug_build_digest: NULL argument");
    if (const int rc = rtgo_sync(c)) return rc;
    std::vector<BuildSpan> spans;
    if (const int rc = build_spans(c, whitted, spans)) return rc;
    std::vector<uint64_t> d;
    for (const BuildSpan& s : spans) {
        uint64_t h = 0xCBF29CE484222325ull;
        for (const BuildSpan::Piece& q : s.pieces) {
            if (q.dev) {
                if (const int rc = digest_device(c, q.dev, q.bytes, h)) return rc;
            } else {
                digest_host(q.host.data(), q.host.size(), h);
            }
        }
        d.push_back(h);
    }
    *n_out = (uint32_t)d.size();
    for (size_t k = 0; k < d.size() && k < cap; ++k) out[k] = d[k];
    return RTGO_OK;
}

// diagnostic (tests/accel_check.py, tools/build_digest.py; not part of include/rtgo.h): span `index` of build_spans read back.  *bytes_out
// = its size; its bytes are copied to `host` when they fit cap_bytes (host may be NULL to ask for the size), its name to `name` (up to
// name_cap bytes with the terminator; may be NULL).  An index beyond the list: RTGO_E_INVALID with *bytes_out = 0, which ends an enumeration.
extern "C" int rtgo_debug_read_build_named(rtgo_ctx* c, int whitted, uint32_t index, void* host, size_t cap_bytes, size_t* bytes_out, char* name,
                                           size_t name_cap)
{
    if (!c || !bytes_out) return fail(c, RTGO_E_INVALID, "rtgo_debug_read_build: NULL argument");
    *bytes_out = 0;
    if (const int rc = rtgo_sync(c)) return rc;
    std::vector<BuildSpan> spans;
    if (const int rc = build_spans(c, whitted, spans)) return rc;
    if (index >= spans.size()) return fail(c, RTGO_E_INVALID, "rtgo_debug_read_build: no span " + std::to_string(index));
    const BuildSpan& s = spans[index];
    *bytes_out = s.bytes();
    if (name && name_cap > 0) {
        std::strncpy(name, s.name.c_str(), name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (!host || cap_bytes < s.bytes()) return RTGO_OK;
    unsigned char* at = static_cast<unsigned char*>(host);
    for (const BuildSpan::Piece& q : s.pieces) {
        if (q.dev && q.bytes) RTGO_HIP(c, hipMemcpy(at, q.dev, q.bytes, hipMemcpyDeviceToHost));
        else if (!q.host.empty()) std::memcpy(at, q.host.data(), q.host.size());
        at += q.bytes;
    }
    return RTGO_OK;
}
extern "C" int rtgo_debug_read_build(rtgo_ctx* c, int whitted, uint32_t index, void* host, size_t cap_bytes, size_t* bytes_out)
{
    return rtgo_debug_read_build_named(c, whitted, index, host, cap_bytes, bytes_out, nullptr, 0);
}

#ifdef RTGO_CMPWALK
// diagnostic build only (tools/cmp_walks.py): rays on which the canonical and the fast walk disagreed since the last call
extern "C" int rtgo_debug_cmpwalk(rtgo_ctx* c, void* host, size_t bytes)
{
    if (!c || !c->d_cmp.get()) return -1;
    if (rtgo_sync(c)) return -1;
    const size_t n = 256 * 16 * sizeof(float);
    if (hipMemcpy(host, c->d_cmp.get(), n < bytes ? n : bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemset(c->d_cmp.get(), 0, n) != hipSuccess) return -1;
    if (hipStreamSynchronize(nullptr) != hipSuccess) return -1;
    return 0;
}
#endif

#ifdef RTGO_TIMELINE
// diagnostic build only (tools/timeline.py): per-wave records of the last launch; returns the number of waves
extern "C" int rtgo_debug_timeline(rtgo_ctx* c, void* host, size_t bytes)
{
    if (!c || !c->d_timeline.get()) return -1;
    if (rtgo_sync(c)) return -1;
    const size_t n = (size_t)c->timeline_waves * 128;
    if (hipMemcpy(host, c->d_timeline.get(), n < bytes ? n : bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int)c->timeline_waves;
}
#endif

// Diagnostic builds whose launches do not produce product results (the whitted tile timer overwrites accum.w and reuses the
// V/T/h counters for ticks; the timeline build records per-wave clocks) answer with a tagged version, so that no test suite or
// driver passes on one of them unnoticed (tests/test_capi_symbols.py asserts the plain number).
#if defined(RTGO_WHITTED_TIMING) || defined(RTGO_TIMELINE) || defined(RTGO_STREAM_STATS)
uint32_t rtgo_abi_version(void) { return RTGO_ABI_VERSION | 0x0D1A6000u; }
#else
uint32_t rtgo_abi_version(void) { return RTGO_ABI_VERSION; }
#endif

const char* rtgo_last_error(const rtgo_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

uint32_t rtgo_local_rows(uint32_t h, uint32_t band_h, uint32_t n_ranks, uint32_t rank)
{
    if (n_ranks <= 1) return h;
    if (band_h == 0) band_h = 4;
    const uint32_t bands = (h + band_h - 1) / band_h;
    uint32_t rows = 0;
    for (uint32_t b = rank; b < bands; b += n_ranks) {
        const uint32_t r0 = b * band_h;
        rows += (r0 + band_h <= h) ? band_h : (h - r0);
    }
    return rows;
}

int rtgo_create(int device, rtgo_ctx** out)
{
    if (!out) return fail(nullptr, RTGO_E_INVALID, "rtgo_create: out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, RTGO_E_NO_DEVICE, "rtgo_create: no HIP device (this library has no CPU path)");
    if (device < 0 || device >= count) return fail(nullptr, RTGO_E_INVALID, "rtgo_create: bad device index");
    RTGO_HIP(nullptr, hipSetDevice(device));
    hipDeviceProp_t prop;
    RTGO_HIP(nullptr, hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, RTGO_E_NO_DEVICE,
                    std::string("rtgo_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    rtgo_ctx* c = new rtgo_ctx();
    c->device = device;
    c->num_cus = prop.multiProcessorCount;
    hipError_t err = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    for (int i = 0; i < rtgo_ctx::kEvRing && err == hipSuccess; ++i) {
        err = hipEventCreate(&c->ev_start[i]);
        if (err == hipSuccess) err = hipEventCreate(&c->ev_stop[i]);
    }
    if (err == hipSuccess) err = c->d_queue.alloc(2 * kQueues * kQueueStride);
    if (err == hipSuccess) err = hipMemset(c->d_queue.get(), 0, 2 * kQueues * kQueueStride * sizeof(unsigned int));
    if (err == hipSuccess) err = c->d_counters.alloc(8);
    if (err == hipSuccess) err = hipMemset(c->d_counters.get(), 0, 8 * sizeof(unsigned long long));
    if (err == hipSuccess) err = c->d_lights.alloc(kMaxLights);
    if (err == hipSuccess) err = hipMemset(c->d_lights.get(), 0, kMaxLights * sizeof(LightRec));
    if (err == hipSuccess) err = c->d_meta.alloc(16);
    // the megakernel may use most of the 160 KiB LDS of a CU
    const int max_lds = 160 * 1024;
    for (const RenderKernelEntry& e : kRenderKernels)
        if (err == hipSuccess) err = hipFuncSetAttribute((const void*)e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    // (the build kernel holds ~58 KB of static LDS; its dynamic part is the fast walk's tree under construction)
    if (err == hipSuccess) err = hipFuncSetAttribute((const void*)build_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBuildDynLds);
    if (err == hipSuccess) err = hipFuncSetAttribute((const void*)whitted::sah_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (err == hipSuccess) err = hipFuncSetAttribute((const void*)whitted::build_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(whitted::kMaxTriangles * sizeof(unsigned long long)));
    // (the batched builds of rtgo_whitted_big.h: each keeps the LDS of the kernel whose body it runs)
    if (err == hipSuccess) err = hipFuncSetAttribute((const void*)whitted::big_sah_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (err == hipSuccess) err = hipFuncSetAttribute((const void*)whitted::big_build_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(whitted::kMaxTriangles * sizeof(unsigned long long)));
    for (const void* fn : {(const void*)whitted::render_kernel<whitted::kAllInL2>, (const void*)whitted::render_kernel<whitted::kRecordsInLds>,
                           (const void*)whitted::render_kernel<whitted::kAllInLds>, (const void*)whitted::render_inst_kernel<false>,
                           (const void*)whitted::render_inst_kernel<true>, (const void*)whitted::render_inst_kernel<false, true>,
                           (const void*)whitted::render_inst_kernel<true, true>,
                           // ... and their FRAMES forms (rtgo_whitted_launch_frames)
                           (const void*)whitted::render_kernel<whitted::kAllInL2, true>, (const void*)whitted::render_kernel<whitted::kRecordsInLds, true>,
                           (const void*)whitted::render_kernel<whitted::kAllInLds, true>, (const void*)whitted::render_inst_kernel<false, false, true>,
                           (const void*)whitted::render_inst_kernel<true, false, true>, (const void*)whitted::render_inst_kernel<false, true, true>,
                           (const void*)whitted::render_inst_kernel<true, true, true>})
        if (err == hipSuccess) err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)whitted::kRenderLds);
    for (const void* fn : {(const void*)trace_rays_kernel<false>, (const void*)trace_rays_kernel<true>,
                           (const void*)whitted::whitted_trace_kernel<whitted::kTraceMesh, false>, (const void*)whitted::whitted_trace_kernel<whitted::kTraceMesh, true>,
                           (const void*)whitted::whitted_trace_kernel<whitted::kTraceInst, false>, (const void*)whitted::whitted_trace_kernel<whitted::kTraceInst, true>,
                           (const void*)whitted::whitted_trace_kernel<whitted::kTraceInstLds, false>, (const void*)whitted::whitted_trace_kernel<whitted::kTraceInstLds, true>,
                           (const void*)whitted::whitted_trace_kernel<whitted::kTraceClustered, false>, (const void*)whitted::whitted_trace_kernel<whitted::kTraceClustered, true>,
                           (const void*)whitted::whitted_trace_kernel<whitted::kTraceClusteredLds, false>,
                           (const void*)whitted::whitted_trace_kernel<whitted::kTraceClusteredLds, true>,
                           // ... and the kernels of rtgo_whitted_shade_rays
                           (const void*)whitted::whitted_shade_kernel<whitted::kTraceMesh>, (const void*)whitted::whitted_shade_kernel<whitted::kTraceInst>,
                           (const void*)whitted::whitted_shade_kernel<whitted::kTraceInstLds>, (const void*)whitted::whitted_shade_kernel<whitted::kTraceClustered>,
                           (const void*)whitted::whitted_shade_kernel<whitted::kTraceClusteredLds>,
                           // ... and of rtgo_shade_rays
                           (const void*)shade_rays_kernel<true, false>, (const void*)shade_rays_kernel<true, true>,
                           (const void*)shade_rays_kernel<false, false>, (const void*)shade_rays_kernel<false, true>})
        if (err == hipSuccess) err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    if (err == hipSuccess) err = hipDeviceSynchronize();  // the null-stream memsets above must land before any launch
    if (err != hipSuccess) {
        std::string m = std::string("rtgo_create: ") + hipGetErrorString(err);
        rtgo_destroy(c);
        return fail(nullptr, RTGO_E_HIP_BASE + (int)err, m);
    }
    c->stream = c->own_stream;
    *out = c;
    return RTGO_OK;
}

// (the context's buffers are released by its owners, when `delete c` runs)
int rtgo_destroy(rtgo_ctx* c)
{
    if (!c) return RTGO_OK;
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    // (a caller's stream may still carry a refit of rtgo_whitted_refit_instances_device_async, which writes what `delete c` frees)
    if (c->stream && c->stream != c->own_stream && c->wm.staging.stale) (void)hipStreamSynchronize(c->stream);
    for (int i = 0; i < rtgo_ctx::kEvRing; ++i) {
        if (c->ev_start[i]) (void)hipEventDestroy(c->ev_start[i]);
        if (c->ev_stop[i]) (void)hipEventDestroy(c->ev_stop[i]);
    }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return RTGO_OK;
}

int rtgo_set_stream(rtgo_ctx* c, void* hip_stream)
{
    if (!c) return RTGO_E_INVALID;
    // launches are ordered by the stream they run on (accumulation buffer, the two alternating sets of queue heads): finish the
    // work on the old stream before moving
    const int rc = rtgo_sync(c);
    if (rc) return rc;
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return RTGO_OK;
}

}  // extern "C"

// ---- the analytic scene: what its set and update entry points call is in rtgo_analytic_host.h.  (Included here, above the camera setters:
// the compiler emits the kernel instantiations in the order the host code first names them.)
#include "rtgo_analytic_host.h"

static bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// The argument rules of the four set calls (`what`: the entry point; `device`: its arrays lie in device memory; `limit`: its largest
// scene) and the per-primitive checks: the host's before the stream is drained, the device's after.  RTGO_OK: the stream is idle.
static int check_set_args(rtgo_ctx* c, const std::string& what, const void* prims, const void* aabbs, uint32_t n, uint32_t limit, bool device)
{
    if (!c || !prims) return fail(c, RTGO_E_INVALID, what + ": NULL argument");
    if (device && (!aligned4(prims) || !aligned4(aabbs))) return fail(c, RTGO_E_INVALID, what + ": a pointer is not 4-byte aligned");
    if (n == 0 || n > limit) return fail(c, RTGO_E_UNSUPPORTED, what + ": primitive count must be in [1, " + std::to_string(limit) + "]");
    if (const int rc = device ? RTGO_OK : check_prims(c, static_cast<const rtgo_prim*>(prims), static_cast<const rtgo_aabb*>(aabbs), n, what)) return rc;
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    return device ? check_prims_device(c, nullptr, prims, aabbs, n, 0, what) : RTGO_OK;
}

// The argument rules of the three update calls, in their order of precedence.  The device calls' arrays must be aligned, and more updates than
// primitives are refused here (by pigeonhole an index repeats or lies beyond the scene).  Zero updates pass (ticket 0): the caller's call is over.
enum UpdateCall { kUpdateHost, kUpdateDevice, kUpdateAsync };
static int check_update_args(rtgo_ctx* c, const std::string& what, UpdateCall call, const void* indices, const void* prims, const void* aabbs, uint32_t k,
                             uint32_t flags, uint64_t* ticket)
{
    const bool device = call != kUpdateHost, async = call == kUpdateAsync;
    if (!c) return fail(c, RTGO_E_INVALID, what + ": NULL context");
    if (async && !ticket) return fail(c, RTGO_E_INVALID, what + ": NULL ticket");
    if (flags & ~(uint32_t)RTGO_UPDATE_REBUILD) return fail(c, RTGO_E_INVALID, what + ": unknown flag bits");
    const AnalyticScene& sc = c->scene;
    const uint32_t n = sc.n_prims;
    if (n == 0) return fail(c, RTGO_E_STATE, what + (async ? ": no analytic scene (rtgo_set_large_scene first)" : ": no analytic scene (rtgo_set_scene or rtgo_set_large_scene first)"));
    if (async && !sc.large) return fail(c, RTGO_E_UNSUPPORTED, what + ": a scene of rtgo_set_scene is built again by its update, with host readers (rtgo_update_prims_device)");
    if (k == 0 && async) *ticket = 0;
    if (k == 0) return RTGO_OK;   // (the rules below are about arrays nobody reads)
    if (!indices || !prims) return fail(c, RTGO_E_INVALID, what + ": NULL argument");
    if (device && (!aligned4(indices) || !aligned4(prims) || !aligned4(aabbs))) return fail(c, RTGO_E_INVALID, what + ": a pointer is not 4-byte aligned");
    if ((aabbs != nullptr) != sc.have_aabbs)
        return fail(c, RTGO_E_INVALID, what + (sc.have_aabbs ? ": the scene was set with boxes, the updates need theirs" : ": the scene was set without boxes, the updates cannot bring any"));
    if (device && k > n) return fail(c, RTGO_E_INVALID, what + ": " + std::to_string(k) + " updates for a scene of " + std::to_string(n) + " primitives");
    return RTGO_OK;
}

extern "C" {

int rtgo_set_scene(rtgo_ctx* c, const rtgo_prim* prims, const rtgo_aabb* aabbs, uint32_t n)
{
    if (const int rc = check_set_args(c, "rtgo_set_scene", prims, aabbs, n, RTGO_MAX_PRIMS, false)) return rc;
    return set_resident(c, prims, aabbs, n, false);
}

int rtgo_set_large_scene(rtgo_ctx* c, const rtgo_prim* prims, const rtgo_aabb* aabbs, uint32_t n)
{
    if (const int rc = check_set_args(c, "rtgo_set_large_scene", prims, aabbs, n, RTGO_MAX_SCENE_PRIMS, false)) return rc;
    return set_large(c, prims, aabbs, n, false, "rtgo_set_large_scene");
}

int rtgo_set_scene_device(rtgo_ctx* c, const void* d_prims, const void* d_aabbs, uint32_t n)
{
    if (const int rc = check_set_args(c, "rtgo_set_scene_device", d_prims, d_aabbs, n, RTGO_MAX_PRIMS, true)) return rc;
    return set_resident(c, d_prims, d_aabbs, n, true);
}

int rtgo_set_large_scene_device(rtgo_ctx* c, const void* d_prims, const void* d_aabbs, uint32_t n)
{
    if (const int rc = check_set_args(c, "rtgo_set_large_scene_device", d_prims, d_aabbs, n, RTGO_MAX_SCENE_PRIMS, true)) return rc;
    return set_large(c, d_prims, d_aabbs, n, true, "rtgo_set_large_scene_device");
}

int rtgo_update_prims(rtgo_ctx* c, const uint32_t* indices, const rtgo_prim* prims, const rtgo_aabb* aabbs, uint32_t n_updates, uint32_t flags)
{
    const std::string what = "rtgo_update_prims";
    if (const int rc = check_update_args(c, what, kUpdateHost, indices, prims, aabbs, n_updates, flags, nullptr); rc || n_updates == 0) return rc;
    const uint32_t n = c->scene.n_prims;
    std::vector<uint32_t> sorted(indices, indices + n_updates);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.back() >= n) return fail(c, RTGO_E_INVALID, what + ": index " + std::to_string(sorted.back()) + " in a scene of " + std::to_string(n) + " primitives");
    const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
    if (twice != sorted.end()) return fail(c, RTGO_E_INVALID, what + ": index " + std::to_string(*twice) + " named twice");
    if (const int rc = check_prims(c, prims, aabbs, n_updates, what)) return rc;
    return apply_updates(c, indices, prims, aabbs, n_updates, false, (flags & RTGO_UPDATE_REBUILD) != 0, what);
}

int rtgo_update_prims_device(rtgo_ctx* c, const void* d_indices, const void* d_prims, const void* d_aabbs, uint32_t n_updates, uint32_t flags)
{
    const std::string what = "rtgo_update_prims_device";
    if (const int rc = check_update_args(c, what, kUpdateDevice, d_indices, d_prims, d_aabbs, n_updates, flags, nullptr); rc || n_updates == 0) return rc;
    return apply_updates(c, d_indices, d_prims, d_aabbs, n_updates, true, (flags & RTGO_UPDATE_REBUILD) != 0, what);
}

int rtgo_update_prims_device_async(rtgo_ctx* c, const void* d_indices, const void* d_prims, const void* d_aabbs, uint32_t n_updates,
                                   const rtgo_aabb* reach, uint64_t* ticket)
{
    const std::string what = "rtgo_update_prims_device_async";
    if (const int rc = check_update_args(c, what, kUpdateAsync, d_indices, d_prims, d_aabbs, n_updates, 0, ticket); rc || n_updates == 0) return rc;
    ReachBox rb;
    const float* r = reach ? &reach->minX : c->scene.bounds;
    for (int a = 0; a < 3; ++a) {
        rb.lo[a] = r[a];
        rb.hi[a] = r[3 + a];
        if (!std::isfinite(r[a]) || !std::isfinite(r[3 + a]) || r[a] > r[3 + a]) return fail(c, RTGO_E_INVALID, what + ": reach is empty or not finite");
    }
    return enqueue_update_async(c, d_indices, d_prims, d_aabbs, n_updates, rb, ticket);
}

int rtgo_update_prims_status(rtgo_ctx* c, uint64_t ticket, rtgo_update_status* out)
{
    if (!c || !out) return fail(c, RTGO_E_INVALID, "rtgo_update_prims_status: NULL argument");
    *out = rtgo_update_status{RTGO_UPDATE_APPLIED, 0, 0, 0};
    if (ticket == 0) return RTGO_OK;
    const rtgo_ctx::UpdateRing& ring = c->updates;
    if (!ring.holds(ticket)) return fail(c, RTGO_E_INVALID, "rtgo_update_prims_status: ticket " + std::to_string(ticket) + " was never issued or has left the ring of the last 64");
    const unsigned int slot = rtgo_ctx::UpdateRing::slot(ticket);
    RTGO_HIP(c, hipSetDevice(c->device));
    const hipError_t e = hipEventQuery(ring.done[slot].get());
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();   // (not an error: the next call's hipGetLastError must not find it)
        out->state = RTGO_UPDATE_PENDING;
        return RTGO_OK;
    }
    RTGO_HIP(c, e);
    const unsigned int* v = ring.h.get() + (size_t)slot * kVerdictWords;
    const int kind = lowest_fault(v, kAsyncVerdictKinds);   // (check_prims_device's choice for its message)
    if (kind >= 0) *out = rtgo_update_status{RTGO_UPDATE_REFUSED, (uint32_t)kind + 1u, v[kind], 0};
    return RTGO_OK;
}

int rtgo_set_camera(rtgo_ctx* c, const float eye[3], const float U[3], const float V[3], const float W[3])
{
    if (!c || !eye || !U || !V || !W) return fail(c, RTGO_E_INVALID, "rtgo_set_camera: NULL argument");
    c->eye = v3{eye[0], eye[1], eye[2]};
    c->U = v3{U[0], U[1], U[2]};
    c->V = v3{V[0], V[1], V[2]};
    c->W = v3{W[0], W[1], W[2]};
    c->have_camera = true;
    return RTGO_OK;
}

int rtgo_set_background(rtgo_ctx* c, const float rgb[3])
{
    if (!c || !rgb) return fail(c, RTGO_E_INVALID, "rtgo_set_background: NULL argument");
    c->bg = v3{rgb[0], rgb[1], rgb[2]};
    return RTGO_OK;
}

int rtgo_set_lights(rtgo_ctx* c, const rtgo_light* lights, int n)
{
    if (!c || n < 0 || (n > 0 && !lights)) return fail(c, RTGO_E_INVALID, "rtgo_set_lights: bad argument");
    if (n > RTGO_MAX_LIGHTS) n = RTGO_MAX_LIGHTS;  // Renderer::WriteLights copies at most MAX_LIGHTS (renderer.cpp:661)
    RTGO_HIP(c, hipSetDevice(c->device));
    if (n > 0) RTGO_HIP(c, hipMemcpyAsync(c->d_lights.get(), lights, n * sizeof(rtgo_light), hipMemcpyHostToDevice, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    c->n_lights = n;
    return RTGO_OK;
}

int rtgo_resize(rtgo_ctx* c, size_t pixels)
{
    if (!c || pixels == 0) return fail(c, RTGO_E_INVALID, "rtgo_resize: bad argument");
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    c->out = rtgo_ctx::Output();
    c->seeds = rtgo_ctx::Seeds();
    rtgo_ctx::Output& o = c->out;
    RTGO_HIP(c, o.own_accum.alloc(pixels));
    RTGO_HIP(c, o.own_image.alloc(pixels));
    RTGO_HIP(c, hipMemsetAsync(o.own_accum.get(), 0, pixels * sizeof(float4), c->stream));
    RTGO_HIP(c, hipMemsetAsync(o.own_image.get(), 0, pixels * sizeof(uchar4), c->stream));
    o.accum = o.own_accum.get();
    o.image = o.own_image.get();
    o.pixels = pixels;
    return RTGO_OK;
}

int rtgo_bind_output(rtgo_ctx* c, void* d_accum, void* d_image, size_t pixels)
{
    if (!c || !d_accum || !d_image || pixels == 0) return fail(c, RTGO_E_INVALID, "rtgo_bind_output: bad argument");
    if (((uintptr_t)d_accum & 15u) || ((uintptr_t)d_image & 3u))
        return fail(c, RTGO_E_INVALID, "rtgo_bind_output: accum must be 16-byte aligned, image 4-byte aligned");
    c->out = rtgo_ctx::Output();
    c->out.accum = (float4*)d_accum;
    c->out.image = (uchar4*)d_image;
    c->out.pixels = pixels;
    return RTGO_OK;
}

// The frame's checks, its window and bands, what it binds (outputs, lights, queues) and the value of a pixel whose samples all miss
static int frame_params(rtgo_ctx* c, const rtgo_frame* f, LaunchParams& p)
{
    if (!c || !f) return fail(c, RTGO_E_INVALID, "rtgo_launch: NULL argument");
    if (c->scene.n_prims == 0) return fail(c, RTGO_E_STATE, "rtgo_launch: no scene (call rtgo_set_scene)");
    if (!c->have_camera) return fail(c, RTGO_E_STATE, "rtgo_launch: no camera (call rtgo_set_camera)");
    if (!c->out.accum || !c->out.image) return fail(c, RTGO_E_STATE, "rtgo_launch: no output (call rtgo_resize or rtgo_bind_output)");
    if (f->image_width == 0 || f->image_height == 0 || f->sqrt_spp <= 0)
        return fail(c, RTGO_E_INVALID, "rtgo_launch: image size and sqrt_spp must be positive");
    if (f->max_trace_depth < 0 || f->max_trace_depth > kMaxLevels)
        return fail(c, RTGO_E_UNSUPPORTED, "rtgo_launch: max_trace_depth must be in [0, 5] (reference uses 5, renderer.cpp:616)");
    if (!f->path_tracing && c->n_lights < 1)
        return fail(c, RTGO_E_STATE, "rtgo_launch: distributed mode needs at least one surface light");
    std::memset(&p, 0, sizeof p);
    p.W = f->image_width;
    p.H = f->image_height;
    p.x0 = f->x0;
    p.y0 = f->y0;
    p.w = f->w ? f->w : f->image_width;
    p.h = f->h ? f->h : f->image_height;
    if ((uint64_t)p.x0 + p.w > p.W || (uint64_t)p.y0 + p.h > p.H) return fail(c, RTGO_E_INVALID, "rtgo_launch: window outside the image");
    p.band_h = f->band_h ? f->band_h : 4;
    p.n_ranks = f->n_ranks ? f->n_ranks : 1;
    p.rank = f->rank;
    if (p.rank >= p.n_ranks) return fail(c, RTGO_E_INVALID, "rtgo_launch: rank >= n_ranks");
    p.local_rows = rtgo_local_rows(p.h, p.band_h, p.n_ranks, p.rank);
    if ((size_t)p.local_rows * p.w > c->out.pixels) return fail(c, RTGO_E_INVALID, "rtgo_launch: output buffer too small for this window");
    p.eye = c->eye;
    p.U = c->U;
    p.V = c->V;
    p.Wv = c->W;
    p.bg = c->bg;
    const uint32_t nn = (uint32_t)f->sqrt_spp * (uint32_t)f->sqrt_spp;
    {
        // the same float additions, in the same order, as the kernel's in-order sum over samples that all miss (kernel.cu:232-237)
        volatile float sx = 0.0f, sy = 0.0f, sz = 0.0f;
        for (uint32_t k = 0; k < nn; ++k) {
            sx = sx + c->bg.x;
            sy = sy + c->bg.y;
            sz = sz + c->bg.z;
        }
        const float inv = 1.0f / (float)nn;
        p.bg_pixel = v3{sx * inv, sy * inv, sz * inv};
    }
    p.lights = c->d_lights.get();
    p.accum = c->out.accum;
    p.image = c->out.image;
    p.queue = c->d_queue.get() + (size_t)c->queue_set * kQueues * kQueueStride;
    p.queue_next = c->d_queue.get() + (size_t)(1 - c->queue_set) * kQueues * kQueueStride;
    p.counters = c->d_counters.get();
#ifdef RTGO_CMPWALK
    if (!c->d_cmp.get()) {
        RTGO_HIP(c, c->d_cmp.alloc(256 * 16));
        RTGO_HIP(c, hipMemset(c->d_cmp.get(), 0, 256 * 16 * sizeof(float)));
        RTGO_HIP(c, hipStreamSynchronize(nullptr));   // (null-stream memset: the launch stream does not wait for it)
    }
    p.cmp = c->d_cmp.get();
#endif
#ifdef RTGO_TIMELINE
    if (!c->d_timeline.get()) RTGO_HIP(c, c->d_timeline.alloc(16384 * 128 / sizeof(unsigned long long)));
    p.timeline = c->d_timeline.get();
#endif
    p.n_prims = (int)c->scene.n_prims;
    p.n_nodes = 2 * (int)c->scene.n_prims - 1;
    p.n_lights = c->n_lights;
    p.sqrt_spp = f->sqrt_spp;
    p.max_depth = f->max_trace_depth;
    p.frame = f->frame_count;
    p.ambient = f->use_ambient ? 1 : 0;
    p.count_stats = f->collect_stats ? 1 : 0;
    return RTGO_OK;
}

// The fast walk's tight boxes carry 1e-3 of padding against the rounding of the intersection programs, which grows with
// the coordinates involved (~1e-7 of them for a rectangle's hit point).  Beyond 500 units -- the reference's scenes stay
// within 20, its camera at 14 -- the launch takes the canonical walk instead: slower, and equal to it by definition.
// Returns whether the launch is beyond the guard; records both quantities for rtgo_get_stats.
static bool far_field_guard(rtgo_ctx* c, const LaunchParams& p, const Knobs& kn)
{
    const AnalyticScene& sc = c->scene;
    float reach = 0.0f;
    for (int k = 0; k < 6; ++k) reach = std::fabs(sc.bounds[k]) > reach ? std::fabs(sc.bounds[k]) : reach;
    const float e[3] = {p.eye.x, p.eye.y, p.eye.z};
    for (int k = 0; k < 3; ++k) reach = std::fabs(e[k]) > reach ? std::fabs(e[k]) : reach;
    // ... and a sphere's or cylinder's reported hit leaves its surface as the ray origin recedes: b^2 - 4ac cancels to the last
    // bits of b^2 ~ D^2 / s^4, i.e. the hit lies up to ~2^-25 D^2 smax / smin^2 off the surface (D: origin to the primitive, s: its
    // axis scales) -- outside the reference's own box when that exceeds AABB_EPSILON.  From there on no two traversals agree on
    // grazing rays (the canonical LBVH culls such a hit by the primitive's box, a multi-primitive leaf's box lets it through, and
    // OptiX promises neither), so what is bounded is Q = max over quadrics of D^2 smax / smin^2, D over the eye and the scene's
    // tight bounds (where bounce rays start).  Thresholds: kGuardReach / kGuardQuadric, set from tools/fuzz_farfield.py's table
    // (profiles/r03a) with the safety factors stated at their definition.
    float quad = 0.0f;
    for (const AnalyticScene::Quadric& qd : sc.quadrics) {
        float d2 = 0.0f, e2 = 0.0f;
        for (int k = 0; k < 3; ++k) {
            const float lo = std::fabs(sc.bounds[k] - qd.c[k]), hi = std::fabs(sc.bounds[3 + k] - qd.c[k]);
            const float far_k = lo > hi ? lo : hi;
            d2 += far_k * far_k;
            e2 += (e[k] - qd.c[k]) * (e[k] - qd.c[k]);
        }
        const float q2 = (d2 > e2 ? d2 : e2) * qd.w;
        quad = q2 > quad ? q2 : quad;
    }
    c->guard_reach = reach;
    c->guard_quadric = quad;
    return !(reach <= kGuardReach) || !(quad <= kn.guard_quadric);
}

// What choose_candidate decided.  The trial's part of it (a new key, the choice, the timed launch) is committed by enqueue once the
// kernel is in the stream, so that a launch that fails before that leaves the trial as it was.
struct Pick {
    bool stream = false;
    int structure = 0;              // 0 / 1: the trees of 36 % / 15 %, 2: the grid
    int trial_k = -1, choice = -1;  // the candidate this launch times (-1: none); the trial's winner, once decided
    int n_cand = 1;
    std::vector<uint32_t> new_key;  // non-empty: this launch starts a new trial, for this key
};

// ---- which loop and which structure (rtgo_ctx::Trial).  More than 16 spp = several passes per pixel: the streaming variant
// (render_kernel, STREAM) lets a lane start its next sample when its path has ended instead of waiting for the wave's longest path,
// pass after pass; and where rtgo_set_scene's two builds differ, either structure can be the faster one.  Candidate k = loop (k & 1:
// 0 = streaming when there is a choice) | structure (k >> 1 when both loops are candidates, else k).
// in_trial = false (rtgo_launch_frames): the launch takes no part in the trial -- the settled choice of this very job when there is one,
// else the first candidate; nothing is timed, waited for or recorded.
static int choose_candidate(rtgo_ctx* c, const rtgo_frame* f, const LaunchParams& p, uint32_t nn, const Knobs& kn, bool canon, Pick& pk, bool in_trial = true)
{
    if (canon) {
#ifdef RTGO_CMPWALK
        // (diagnostic build: the instrumented launch also runs the pinned fast structure on every ray, rtgo_ray_trace.inc)
        if (kn.tree == 1 && c->scene.have_alt) pk.structure = 1;
        if (kn.tree == 2 && c->scene.grid.have && c->guard_reach <= c->scene.grid.reach_max) pk.structure = 2;
#endif
        return RTGO_OK;
    }
    const bool path = f->path_tracing != 0, multi_pass = passes_of(nn) > 1;
    // (the grid: where rtgo_set_scene built one, for rays that start within the reach its pad was sized for, and in the instantiations
    // that exist -- not the flat-primitives one)
    const bool flat_only = path && c->scene.quadrics.empty() && !kn.no_frames;
    const bool grid_ok = c->scene.grid.have && c->guard_reach <= c->scene.grid.reach_max && !flat_only;
    int structs[3], n_structs = 0;
    structs[n_structs++] = 0;
    if (c->scene.have_alt) structs[n_structs++] = 1;
    if (grid_ok) structs[n_structs++] = 2;
    if (kn.tree >= 0) {   // (RTGO_TREE, RTGO_STREAM: experiment and test knobs, no trial over that dimension)
        pk.structure = 0;
        for (int k = 0; k < n_structs; ++k)
            if (structs[k] == kn.tree) pk.structure = kn.tree;
        n_structs = 1;
        structs[0] = pk.structure;
    }
    const bool loops = multi_pass && kn.stream < 0;
    if (multi_pass && kn.stream >= 0) pk.stream = kn.stream != 0;
    const int n_loops = loops ? 2 : 1;
    const int n_cand = n_loops * n_structs;
    auto decode = [&](int k) {
        if (loops) pk.stream = (k % n_loops) == 0;
        pk.structure = structs[k / n_loops];
    };
    if (n_cand == 1) {
        decode(0);
        return RTGO_OK;
    }
    rtgo_ctx::Trial& t = c->trial;
    std::vector<uint32_t> key = {p.W, p.H, p.x0, p.y0, p.w, p.h, p.band_h, p.n_ranks, p.rank, nn, (uint32_t)path, (uint32_t)f->max_trace_depth,
                                 (uint32_t)(f->use_ambient != 0), (uint32_t)n_cand, (uint32_t)pk.stream, (uint32_t)pk.structure, (uint32_t)grid_ok};
    const bool fresh = key != t.key;
    if (!in_trial) {
        decode(!fresh && t.choice >= 0 ? t.choice : 0);
        return RTGO_OK;
    }
    const int issued = fresh ? 0 : t.issued;
    int choice = fresh ? -1 : t.choice;
    pk.n_cand = n_cand;
    if (fresh) pk.new_key = std::move(key);
    else if (choice < 0 && issued >= 2 * n_cand) {
        // all are in flight or done: WAIT for them.  A caller that enqueues a whole job without synchronising (bench.py's spin-up,
        // a batch render) would otherwise run it to the end on whatever stands in for an undecided trial -- profiles/r03p caught
        // 90 of 100 launches of C4 on its slowest candidate that way.  One stall of at most 2 * n_cand launches per job.
        while (t.done < 2 * n_cand && c->ev_pending > 0)
            if (const int rc = harvest_events(c, 1)) return rc;
        if (t.done >= 2 * n_cand) {
            choice = 0;
            for (int k = 1; k < n_cand; ++k)
                if (t.best[k] < t.best[choice]) choice = k;
        }
    }
    pk.choice = choice;
    if (choice >= 0) decode(choice);
    else if (issued < 2 * n_cand) {
        pk.trial_k = issued % n_cand;
        decode(pk.trial_k);
    } else decode(0);   // (the trial's events were lost to a key change: start over with the first candidate)
    return RTGO_OK;
}

// what the walk reads: the canonical LBVH, and the chosen fast structure (`ft`, or the grid over ft's small primitives)
static void walk_params(const rtgo_ctx* c, const AnalyticScene::FastTree& ft, bool canon, bool use_grid, LaunchParams& p)
{
    // cuboid_range's margin, in the object-space y units of a face g: the certificate's tolerance plus the rounding of what is
    // compared -- the reference's (u, v) on a face f, carried into y_g units by L_fg, and y_g(t_f) itself.  Each is a handful of
    // float operations on terms no larger than |row| (|o| + t |d|) + |w| <= |row|_1 * 3 reach + |w| (origins within `reach`, hit
    // points within the scene: t |d| <= 2 reach), i.e. <= 12 * 2^-24 of them; K = 64 * 2^-24 leaves five times that, and the
    // build's A, B = max over (f, g) of L_fg |row_f|_1 + |row_g|_1 and of L_fg |w_f| + |w_g|.
    p.cub_mu = kCuboidTol + 64.0f * 5.9604645e-8f * (ft.cub_a * 3.0f * c->guard_reach + ft.cub_b);
    p.list_cub = ft.list_cub;
    p.tree_spheres = ft.tree_spheres;
    if (!(p.cub_mu < 0.02f)) {   // (tiny faces far from the origin: the margin would let two faces through too often to pay)
        p.list_cub = 0;
        p.cub_mu = -1.0f;        // tree leaves: cuboid_range is not taken either (see render_kernel)
    }
    const AnalyticScene& sc = c->scene;
    p.nodes = sc.d_nodes.get();
    p.prims = sc.d_prims.get();
    p.fnodes = use_grid ? (const float4*)sc.grid.d.get() : ft.d_fnodes.get();
    p.n_fnodes = use_grid ? sc.grid.n_nodes : ft.n_fnodes;
    p.grid = use_grid ? sc.grid.gp : rtgo::GridParams();
    p.fprims = ft.d_fprims.get();
    p.frames = sc.d_frames.get();
    p.n_small = ft.n_small;
    p.n_big_pairs = ft.n_big_pairs;
    p.stack_depth = canon ? kStackDepth : ((ft.fast_depth > 0 && !use_grid) ? ft.fast_depth : 1) + 1;   // (+1: fast_tree writes the slot past the top before it knows whether it pushes)
}

// The launch half of the last-ray certificate (see emitter_cert): path mode, the fast walk over a tree, the room still certified at this
// launch's reach (walk_params), a background of +0 in all three channels (a miss then pays what a non-emitter hit pays: compared as
// bits), every emitter inside every wall by more than the margin at this reach, and max_depth >= 1 (the last ray is never a primary
// ray: the pixel's "every primary ray missed" shortcut does not see it).  RTGO_NO_LAST_EMITTER: off.
static void last_ray_params(const rtgo_ctx* c, const AnalyticScene::FastTree& ft, bool path, bool canon, bool use_grid, const Knobs& kn, LaunchParams& p)
{
    p.emit_n = 0;
    const float bg[3] = {p.bg.x, p.bg.y, p.bg.z};
    uint32_t bg_bits[3];
    std::memcpy(bg_bits, bg, sizeof bg_bits);
    if (!path || canon || use_grid || kn.no_last_emitter || p.list_cub != 2 || p.max_depth < 1 || (bg_bits[0] | bg_bits[1] | bg_bits[2]) != 0u)
        return;
    const double K = 64.0 * 5.9604644775390625e-8, R = (double)c->guard_reach;
    for (int k = 0; k < 6 * ft.emit_n; ++k)
        if (!((double)ft.emit_ymin[k] > K * ((double)ft.emit_a[k] * R + (double)ft.emit_b[k]))) return;
    p.emit_n = ft.emit_n;
}

// A launch that takes a pair kernel: the three words a ray of those kernels reads before its walk (PairWords), from the fields walk_params
// and last_ray_params have set.  They lie in the grid's space (a pair launch walks no grid), so this is the last write to that space:
// call it once the kernel is chosen, and write p.grid no more after it.
// rw, room_mu: the room in world axes and this launch's margin for it (room_world_margin), for render_roomw_kernel; null: zeros, read by no kernel.
static void pair_words(LaunchParams& p, const rtgo::RoomWorld* rw, float room_mu)
{
    p.pair = PairWords();
    p.pair.cub_mu = p.cub_mu;
    p.pair.n_prims = p.n_prims;
    p.pair.last_depth = p.emit_n != 0 ? p.max_depth : -1;
    if (rw) {
        p.pair.room_map = rw->map;
        for (int j = 0; j < 3; ++j) {
            p.pair.room_lo[j] = rw->lo[j];
            p.pair.room_hi[j] = rw->hi[j];
        }
        p.pair.room_mu = room_mu;
        p.pair.room_thr = rw->thr;
    }
}

// Scheduling: units of 64 paths = the N*N samples of `unit_px` neighbouring pixels of one row; the queue hands out STRIPS of
// `grab` units side by side (<= 64 pixels) from the rectangle that can contain geometry.  Strips are long when there is
// plenty of work (their pixel seeds are hashed once per strip) and short when units are scarce (small windows, one GPU's
// share of a tiled frame), so that every resident wave still gets >= ~32 turns
// (the last strips in flight set the tail of the launch: cornell 1080p spp 16 runs 6 % faster on 1-unit strips than on 4-unit ones).
// The pixels outside the rectangle `r` are cold: 64-pixel row segments, handed out in chunks.
static int schedule(rtgo_ctx* c, uint32_t nn, const Rect& r, LaunchParams& p, uint32_t& strip_px, uint64_t& units_hot)
{
    const uint32_t unit_px = 64u / (nn < (uint32_t)kSamplesPerPass ? nn : (uint32_t)kSamplesPerPass);
    const uint32_t lr0 = owned_rows_below(r.y0, p.band_h, p.n_ranks, p.rank), lr1 = owned_rows_below(r.y1, p.band_h, p.n_ranks, p.rank);
    units_hot = (uint64_t)((r.x1 - r.x0 + unit_px - 1) / unit_px) * (lr1 - lr0);
    const uint64_t waves_guess = (uint64_t)c->num_cus * 16u;
    const uint32_t grab = (uint32_t)(units_hot / (waves_guess * 32u));
    const uint32_t grab_max = (64u / unit_px) < (uint32_t)kUnitsPerGrab ? (64u / unit_px) : (uint32_t)kUnitsPerGrab;
    p.grab = grab < 1u ? 1u : (grab > grab_max ? grab_max : grab);
    strip_px = unit_px * p.grab;
    p.hot_x0 = r.x0 / strip_px;
    p.hot_w = (r.x1 + strip_px - 1) / strip_px - p.hot_x0;
    p.hot_y0 = lr0;
    p.hot_h = lr1 - lr0;
    if (p.hot_w == 0 || p.hot_h == 0) p.hot_x0 = p.hot_y0 = p.hot_w = p.hot_h = 0;
    if ((uint64_t)p.hot_w * p.hot_h > 0x7FFFFF00ull) return fail(c, RTGO_E_UNSUPPORTED, "rtgo_launch: window too large");
    p.n_hot = p.hot_w * p.hot_h;
    p.cold_x0 = p.hot_x0 * strip_px;
    p.cold_x1 = (p.hot_x0 + p.hot_w) * strip_px < p.w ? (p.hot_x0 + p.hot_w) * strip_px : p.w;
    p.rows_above = p.local_rows - p.hot_y0 - p.hot_h;
    p.segs_full = (p.w + 63u) / 64u;
    p.segs_l = p.n_hot ? (p.cold_x0 + 63u) / 64u : 0u;
    p.segs_r = p.n_hot ? (p.w - p.cold_x1 + 63u) / 64u : 0u;
    const uint64_t cold_segs = (uint64_t)(p.hot_y0 + p.rows_above) * p.segs_full + (uint64_t)p.hot_h * (p.segs_l + p.segs_r);
    if (cold_segs > 0x7FFFFF00ull) return fail(c, RTGO_E_UNSUPPORTED, "rtgo_launch: window too large");
    p.n_cold_segs = (uint32_t)cold_segs;
    // cold chunks: about two per resident wave
    p.cold_cs = (uint32_t)((cold_segs + (uint64_t)c->num_cus * 32u - 1) / ((uint64_t)c->num_cus * 32u));
    if (p.cold_cs == 0) p.cold_cs = 1;
    const uint32_t n_cold = (p.n_cold_segs + p.cold_cs - 1) / p.cold_cs;
    p.n_tiles = p.n_hot + n_cold;
    return RTGO_OK;
}

// Inside the rectangle, strip by strip: does any primitive's own screen rectangle (its box as the fast walk culls with it,
// through the same pinhole projection, padded) reach the strip?  Scenes that do not fill their rectangle -- plateau: a plate and
// a few objects -- have most of it empty.  The mask depends on the launch geometry only; it is rebuilt when that changes.
// Sets p.hot_mask unless every strip is hot; cold_pixels: the pixels of the masked strips.
static int update_hot_mask(rtgo_ctx* c, uint32_t strip_px, LaunchParams& p, unsigned long long& cold_pixels)
{
    std::vector<uint32_t> key = {p.W, p.H, p.x0, p.y0, p.w, p.h, p.band_h, p.n_ranks, p.rank, p.grab, strip_px, p.hot_x0, p.hot_y0, p.hot_w, p.hot_h};
    const float cam[12] = {p.eye.x, p.eye.y, p.eye.z, p.U.x, p.U.y, p.U.z, p.V.x, p.V.y, p.V.z, p.Wv.x, p.Wv.y, p.Wv.z};
    for (float v : cam) {
        uint32_t bits;
        std::memcpy(&bits, &v, 4);
        key.push_back(bits);
    }
    const size_t words = ((size_t)p.n_hot + 31) / 32;
    rtgo_ctx::HotMask& hm = c->mask;
    if (key != hm.key) {
        std::vector<uint32_t> mask(words, 0u);
        bool all_hot = false;
        for (uint32_t i = 0; i < c->scene.n_prims && !all_hot; ++i) {
            const Rect q = box_screen_rect(&c->scene.tight[6 * (size_t)i], p);
            if (q.x0 == 0 && q.x1 == p.w && q.y0 == 0 && q.y1 == p.h) {   // a primitive whose rectangle is the whole window (or unknown)
                all_hot = true;
                break;
            }
            if (q.x1 <= q.x0 || q.y1 <= q.y0) continue;
            const uint32_t sa = q.x0 / strip_px, sb = (q.x1 - 1) / strip_px;   // strip columns the rectangle touches
            const uint32_t ca = sa > p.hot_x0 ? sa : p.hot_x0, cb = sb < p.hot_x0 + p.hot_w - 1 ? sb : p.hot_x0 + p.hot_w - 1;
            if (ca > cb) continue;
            for (uint32_t wrow = q.y0; wrow < q.y1; ++wrow) {
                if (p.n_ranks > 1 && (wrow / p.band_h) % p.n_ranks != p.rank) continue;
                const uint32_t lrow = owned_rows_below(wrow, p.band_h, p.n_ranks, p.rank);
                if (lrow < p.hot_y0 || lrow >= p.hot_y0 + p.hot_h) continue;
                const size_t base = (size_t)(lrow - p.hot_y0) * p.hot_w;
                for (uint32_t sc = ca; sc <= cb; ++sc) {
                    const size_t bit = base + (sc - p.hot_x0);
                    mask[bit >> 5] |= 1u << (bit & 31u);
                }
            }
        }
        unsigned long long cold_px = 0;
        if (!all_hot) {
            size_t hot_bits = 0;
            for (size_t b = 0; b < (size_t)p.n_hot; ++b) {
                if ((mask[b >> 5] >> (b & 31u)) & 1u) {
                    ++hot_bits;
                } else {
                    const uint32_t sc = p.hot_x0 + (uint32_t)(b % p.hot_w);
                    const uint32_t xa = sc * strip_px, xb = xa + strip_px < p.w ? xa + strip_px : p.w;
                    cold_px += xb > xa ? xb - xa : 0;
                }
            }
            all_hot = hot_bits == (size_t)p.n_hot;
        }
        if (!all_hot) {
            if (words > hm.d.size()) {
                // (launches still queued were given the old buffer, and freeing it would wait for the whole device: it is set aside
                // until rtgo_sync has waited for the stream.  Growing to at least twice the size keeps what is set aside below what is held)
                const size_t grown = words > 2 * hm.d.size() ? words : 2 * hm.d.size();
                if (hm.d.get()) hm.retired.push_back(std::move(hm.d));
                RTGO_HIP(c, hm.d.alloc(grown));
            }
            // (the previous launch may still be reading the old mask: stream order takes care of it.)  The copy leaves from pinned
            // memory the context keeps, so nothing here waits for the stream; a slot is reused two rebuilds later, by when its copy
            // has long completed (the event wait is a formality)
            const int slot = hm.slot;
            hm.slot = 1 - slot;
            if (!hm.copied[slot].get()) RTGO_HIP(c, hm.copied[slot].create(hipEventDisableTiming));
            else RTGO_HIP(c, hipEventSynchronize(hm.copied[slot].get()));
            if (words > hm.h[slot].size()) RTGO_HIP(c, hm.h[slot].alloc(words));
            std::memcpy(hm.h[slot].get(), mask.data(), words * sizeof(uint32_t));
            RTGO_HIP(c, hipMemcpyAsync(hm.d.get(), hm.h[slot].get(), words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            RTGO_HIP(c, hipEventRecord(hm.copied[slot].get(), c->stream));
        }
        hm.all_hot = all_hot;
        hm.cold_pixels = all_hot ? 0 : cold_px;
        hm.key = key;
    }
    if (!hm.all_hot) {
        p.hot_mask = hm.d.get();
        cold_pixels = hm.cold_pixels;
    }
    return RTGO_OK;
}

// Pixel seeds of a progressive job (LaunchParams::seeds): a launch of the kernel variant that has the seed pass (the 6-waves lock-step
// one, kernel_has_seed_pass: launches of >= kUnitsPerWave4For6 units per wave) writes frame + 1's seeds of its hot strips into one
// buffer; the next launch reads them when it runs that variant for exactly that frame over exactly that strip layout, and otherwise
// (the first frame, a skipped or repeated frame index, a new window, band share or rectangle, any other variant) hashes them inline.
// Seeds depend on the image width, the pixel and the frame alone, not on camera or scene: the layout is all the key needs.
// Stream order makes the writes of launch f visible to launch f + 1.  `key`: what rtgo_launch records once the launch is on the stream.
static int plan_seeds(rtgo_ctx* c, LaunchParams& p, uint32_t strip_px, bool has_pass, std::vector<uint32_t>& key)
{
    p.seeds = nullptr;
    p.seeds_next = nullptr;
    key.clear();
    const uint64_t words = (uint64_t)p.n_hot * strip_px;
    if (!has_pass || words == 0 || words > (1ull << 27)) return RTGO_OK;
    key = {p.W, p.x0, p.y0, p.w, p.h, p.band_h, p.n_ranks, p.rank, p.grab, strip_px, p.hot_x0, p.hot_y0, p.hot_w, p.hot_h};
    rtgo_ctx::Seeds& sd = c->seeds;
    if (words > sd.d[1].size()) {   // (d[1] is allocated last)
        RTGO_HIP(c, hipStreamSynchronize(c->stream));   // (launches in flight may still use the old buffers)
        sd = rtgo_ctx::Seeds();
        RTGO_HIP(c, sd.d[0].alloc(words));
        RTGO_HIP(c, sd.d[1].alloc(words));
    }
    if (sd.ok && sd.frame == p.frame && sd.key == key) p.seeds = sd.d[sd.read].get();
    p.seeds_next = sd.d[1 - sd.read].get();
    return RTGO_OK;
}

static constexpr uint64_t kUnitsPerWave4For6 = 8;   // launches with fewer units per wave (counted at 4 waves/SIMD) take at most 5 waves (pick_block)
static constexpr uint64_t kUnitsPerWave4For7 = 26;  // ... and with fewer than this at most 6: halfway between the tie at 17 and the win at 35 (pick_block)

struct Block {
    int block = 0, blocks_per_cu = 0, wpe = 4;   // threads per workgroup, workgroups per CU, waves per SIMD of the variant
    size_t lds = 0;
    unsigned int grid = 0;                       // workgroups
};

// LDS image of the chosen kernel (see render_kernel): canonical = nodes + 6/prim; fast = fnodes + 4/prim + 3/prim; global (a scene of
// rtgo_set_large_scene): no scene at all.
// The scene copy is per workgroup and the stack per lane, so bigger scenes want bigger workgroups: pick the size that
// puts the most waves on a CU (4, 5, 6 or 7 per SIMD, what the variant's VGPR budget admits), smallest size on ties.  Without a scene copy
// the stack alone sets the count, and workgroups of one or two waves fit the most of them.
static int pick_block(rtgo_ctx* c, const rtgo_frame* f, const LaunchParams& p, uint32_t nn, bool canon, bool stream, bool frames, bool grid,
                      uint64_t units_hot, const Knobs& kn, Block& b, bool global = false, bool batch = false, bool pair = false)
{
    const bool path = f->path_tracing != 0;
    const int fast_nodes = p.n_fnodes;   // (the tree's nodes, or the grid in their place)
    const size_t scene_lds = (global ? 0 : (size_t)(2 * (canon ? p.n_nodes : fast_nodes) + (canon ? 6 : 7) * p.n_prims + (frames ? 2 * p.n_prims : 0) /* shading frames */) * sizeof(float4)) +
                             (size_t)kMaxLights * sizeof(LightRec) + kCamWords * sizeof(float) +   // + the raygen constants (kCamWordsLean at 6 waves: below)
                             (size_t)(nn < (uint32_t)kSampleTab ? nn : (uint32_t)kSampleTab) * sizeof(uint4);   // + the per-sample start table
    int best_waves = 0;
    // Waves per SIMD the kernel variant is compiled for: 4 (<= 128 VGPRs), 5 (<= 96, level records in LDS) or 6 (<= 80; path mode
    // over flat scenes only, the FRAMES lock-step kernel -- the one combination that fits without scratch).  More resident waves fill
    // more of the vector issue slots (cornell 1080p: 1.32 ms at 4, 1.22 at 5; 0.89 -> 0.86 at 5 -> 6), but every wave then runs
    // slower and the launch ends one unit-duration after the queue runs dry: with few units per wave the shorter tail of fewer
    // waves wins (a 1/16 share: 0.127 / 0.137 ms at 4 / 5).  Round 1's 6-waves kernel spilled 25-32 registers to scratch (472 MB of
    // HBM per launch, profiles/r02d) and was dropped; today's fits because the per-lane values derived from the lane index are
    // derived where they are used (opaque_lane in rtgo_device.h) instead of being held through every ray loop.
    const uint64_t units_per_wave4 = units_hot * (passes_of(nn)) / ((uint64_t)c->num_cus * 16u);
    // `pair`: the launch qualifies for the pair kernels (launch_frame), which exist at 5, 6 and 7 waves -- 7 (<= 72 VGPRs) for them alone --
    // and never touch the traversal stack: at those waves the launch reserves none (launch_frame then sets p.stack_depth to 0).  Seven
    // waves are 7 workgroups of 256 threads per CU; where the LDS image does not fit 7, no block size beats 6 waves' 24 and 6 stays.
    const auto is_pair = [&](int w) { return pair && find_kernel(path, canon, w, stream, false, frames, grid, global, batch, true) != nullptr; };
    const int top_wpe = is_pair(7) ? 7 : (find_kernel(path, canon, 6, stream, false, frames, grid, global, batch) ? 6 : 5);   // the 6-waves variant exists for some combinations only
    // 7 against 6 (profiles/r09a/threshold.log, cornell 1080p and its band shares): the full frame (35 units per wave) 0.6965 -> 0.6854 ms,
    // ranges apart; the 1/2 share (17) ties; the 1/3, 1/4 and 1/8 shares (11, 8, 4) lose 1.5, 2.6 and 10 % to the longer tail.
    const int max_wpe_work = units_per_wave4 >= kUnitsPerWave4For7 ? 7 : (units_per_wave4 >= kUnitsPerWave4For6 ? 6 : (units_per_wave4 >= 3 ? 5 : 4));
    int max_wpe = canon ? 4 : (kn.max_wpe ? (int)kn.max_wpe : max_wpe_work);   // (RTGO_MAX_WPE: experiment knob, clamped to what exists)
    max_wpe = max_wpe < 4 ? 4 : (max_wpe > top_wpe ? top_wpe : max_wpe);
    for (int w = 4; w <= max_wpe; ++w)
        for (int bs = global ? 64 : 256; bs <= kMaxBlock; bs *= 2) {
            const size_t l = scene_lds + (stream ? (size_t)(bs / 64) * 192 * kStreamWindow * sizeof(float) : 0) + (is_pair(w) ? 0 : (size_t)p.stack_depth * bs * (canon ? sizeof(float2) : sizeof(unsigned int))) + ((w >= 5 || (batch && !path)) ? (size_t)bs * (path ? 3 : 4) * kMaxLevels * sizeof(float) : 0) + ((batch && !path && w >= 5) ? (size_t)bs * 9 * sizeof(float) : 0) /* render_frames_kernel, distributed: level records at 4 waves too, the shadow ray's state at 5 */ + ((w >= 6 || (batch && !path && w >= 5)) ? (size_t)(kCamWordsLean - kCamWords) * sizeof(float) : 0);
            int per_cu = (int)((160 * 1024) / l);
            if (per_cu * (bs / 64) > 4 * w) per_cu = (4 * w) / (bs / 64);
            const int waves = per_cu * (bs / 64);
            if (waves > best_waves) {
                best_waves = waves;
                b.block = bs;
                b.blocks_per_cu = per_cu;
                b.lds = l;
                b.wpe = w;
            }
        }
    if (best_waves == 0) return fail(c, RTGO_E_UNSUPPORTED, "rtgo_launch: scene does not fit in LDS");
    int cus = c->num_cus - (int)(f->reserve_cus < (uint32_t)c->num_cus / 2 ? f->reserve_cus : (uint32_t)c->num_cus / 2);
    b.grid = (unsigned int)(cus * b.blocks_per_cu);
    const unsigned int need = (p.n_tiles + (b.block / 64) - 1) / (b.block / 64);
    if (b.grid > need) b.grid = need;
    return RTGO_OK;
}

// The timed launch of the analytic path, then its bookkeeping: only now does the trial (rtgo_ctx::Trial) learn of it
static int enqueue(rtgo_ctx* c, RenderKernel kernel, const LaunchParams& p, const Block& b, Pick& pk, bool canon, uint64_t rays_culled)
{
#ifdef RTGO_TIMELINE
    c->timeline_waves = b.grid * (unsigned int)(b.block / 64);
    if (c->timeline_waves > 16384) return fail(c, RTGO_E_UNSUPPORTED, "timeline buffer too small");
#endif
    RTGO_HIP(c, hipSetDevice(c->device));
    int slot = 0;
    const int rc = timed_launch(c, slot, [&]() -> int {
        hipLaunchKernelGGL(kernel, dim3(b.grid), dim3(b.block), b.lds, c->stream, p, p.fprims);
        RTGO_HIP(c, hipGetLastError());
        return RTGO_OK;
    });
    if (rc) return rc;
    if (pk.n_cand > 1) {
        rtgo_ctx::Trial& t = c->trial;
        if (!pk.new_key.empty()) {
            // (event tags of an unfinished trial of the old key are dropped: nothing reads its minima)
            t = rtgo_ctx::Trial();
            t.key = std::move(pk.new_key);
            for (unsigned char& tag : c->ev_tag) tag = 0;
        }
        t.choice = pk.choice;
        if (pk.trial_k >= 0) {
            c->ev_tag[slot] = (unsigned char)(pk.trial_k + 1);
            t.issued++;
            c->launches_trial++;
        }
    }
    c->queue_set = 1 - c->queue_set;
    c->rays_culled += rays_culled;
    if (canon) c->launches_canonical++;
    c->last_variant = (pk.stream ? 1u : 0u) | (pk.structure == 1 ? 2u : 0u) | (canon ? 4u : 0u) | (pk.trial_k >= 0 ? 8u : 0u) | (pk.structure == 2 ? 16u : 0u) |
                      (p.emit_n > 0 ? 64u : 0u);
    return RTGO_OK;
}

// A launch over a scene of rtgo_set_large_scene: the canonical walk from global memory (render_kernel's GLOBAL instantiations), the
// stack as deep as the scene's tree.  No launch-time trial, fast structure, far-field guard (the canonical walk is what every other
// walk is held to) or seed pass; the screen rectangle comes from the root box, without a per-strip mask.
static int launch_large(rtgo_ctx* c, const rtgo_frame* f, LaunchParams& p, const Knobs& kn)
{
    const uint32_t nn = (uint32_t)f->sqrt_spp * (uint32_t)f->sqrt_spp;
    const bool path = f->path_tracing != 0, stats = f->collect_stats != 0;
    const Rect r = f->collect_stats != 1 ? box_screen_rect(c->scene.bounds, p) : Rect{0, p.w, 0, p.h};
    c->guard_reach = 0.0f;
    c->guard_quadric = 0.0f;
    p.nodes = c->scene.d_nodes.get();
    p.prims = c->scene.d_prims.get();
    p.stack_depth = c->scene.lbvh_depth > 0 ? c->scene.lbvh_depth : 1;
    uint32_t strip_px = 0;
    uint64_t units_hot = 0;
    if (const int rc = schedule(c, nn, r, p, strip_px, units_hot)) return rc;
    if (p.n_tiles == 0) return RTGO_OK;  // this rank owns no rows
    Block b;
    if (const int rc = pick_block(c, f, p, nn, true, false, false, false, units_hot, kn, b, true)) return rc;
    if (kn.debug)
        std::fprintf(stderr, "rtgo_launch: canonical walk from global memory, grid %u x %d threads, %zu B LDS, %d workgroups/CU, %u strips of %u px, stack %d\n",
                     b.grid, b.block, b.lds, b.blocks_per_cu, p.n_hot, strip_px, p.stack_depth);
    const RenderKernel kernel = find_kernel(path, true, 4, false, stats, false, false, true);
    if (!kernel) return fail(c, RTGO_E_UNSUPPORTED, "rtgo_launch: no kernel variant for this configuration");
    const unsigned long long culled = (unsigned long long)p.local_rows * p.w - (unsigned long long)p.hot_h * (p.cold_x1 - p.cold_x0);
    c->seeds.ok = false;
    Pick pk;
    if (const int rc = enqueue(c, kernel, p, b, pk, true, culled * nn)) return rc;
    c->last_variant |= 32u;
    c->seeds_last = 0;
    return RTGO_OK;
}

// One kernel launch: frame f->frame_count (n_frames = 1), or n_frames frames from it on in the batched kernels.  in_trial: see
// choose_candidate.  A launch of several frames that the batched kernels do not cover enqueues nothing and says so in *unbatched.
static int launch_frame(rtgo_ctx* c, const rtgo_frame* f, uint32_t n_frames, bool in_trial, bool* unbatched)
{
    const Knobs kn;
    LaunchParams p;
    if (const int rc = frame_params(c, f, p)) return rc;
    const bool batch = n_frames > 1;
    p.n_frames = n_frames;
    if (batch && (c->scene.large || f->collect_stats != 0 || passes_of((uint32_t)f->sqrt_spp * (uint32_t)f->sqrt_spp) > 1)) {
        *unbatched = true;
        return RTGO_OK;
    }
    if (c->scene.large) return launch_large(c, f, p, kn);
    const uint32_t nn = (uint32_t)f->sqrt_spp * (uint32_t)f->sqrt_spp;
    const bool path = f->path_tracing != 0, stats = f->collect_stats != 0;
    // collect_stats 1: the instrumented kernel traces every pixel (V, T, h over ALL rays); 2: it culls like the timed
    // kernel, so that the counters describe the traversed rays only
    const bool cull = f->collect_stats != 1;
    const Rect r = cull ? box_screen_rect(c->scene.bounds, p) : Rect{0, p.w, 0, p.h};
    const bool canon = far_field_guard(c, p, kn) || stats;
    Pick pk;
    if (const int rc = choose_candidate(c, f, p, nn, kn, canon, pk, in_trial)) return rc;
    const bool use_alt = pk.structure == 1, use_grid = pk.structure == 2;
    if (batch && (canon || use_grid)) {
        *unbatched = true;
        return RTGO_OK;
    }
    walk_params(c, c->scene.tree[use_alt ? 1 : 0], canon, use_grid, p);
    last_ray_params(c, c->scene.tree[use_alt ? 1 : 0], path, canon, use_grid, kn, p);
    uint32_t strip_px = 0;
    uint64_t units_hot = 0;
    if (const int rc = schedule(c, nn, r, p, strip_px, units_hot)) return rc;
    unsigned long long mask_cold_pixels = 0;
    if (cull && p.n_hot > 0)
        if (const int rc = update_hot_mask(c, strip_px, p, mask_cold_pixels)) return rc;
    if (p.n_tiles == 0) return RTGO_OK;  // this rank owns no rows
    const bool frames = path && !canon && c->scene.quadrics.empty() && !kn.no_frames;   // scenes of flat primitives only: N and the sampling tangent from LDS
    // The straight-line walk of a two-leaf tree (render_pair_kernel, fast_pair): path mode over a flat scene with frames, the lock-step loop,
    // one frame per launch, inside the far-field guard, over a tree (not the grid) that is a root over two certified cuboid leaves, the
    // cuboid margin still positive at this launch's reach, an up-front list that starts with a certified room (the kind of cuboid the pair
    // kernels' list test is compiled for: fast_list's KIND) -- and a variant at the waves per SIMD pick_block chose (5, 6 and, as
    // render_pair7_kernel, 7).  RTGO_NO_PAIR: off.
    const bool pair_ok = path && !canon && !pk.stream && frames && !use_grid && !batch && !kn.no_pair && c->scene.tree[use_alt ? 1 : 0].pair && p.cub_mu > 0.0f &&
                         p.list_cub == 2;
    Block b;
    if (const int rc = pick_block(c, f, p, nn, canon, pk.stream, frames, use_grid, units_hot, kn, b, false, batch, pair_ok)) return rc;
    const RenderKernel pair_kernel = pair_ok ? find_kernel(path, canon, b.wpe, pk.stream, stats, frames, use_grid, false, batch, true) : nullptr;
    // ... and with cuboid_slab where the room and both leaves also hold the slab certificate and the waves have such a kernel.  RTGO_NO_SLAB: off.
    const AnalyticScene::FastTree& walked = c->scene.tree[use_alt ? 1 : 0];
    const RenderKernel slab_kernel = (pair_kernel && !kn.no_slab && walked.slab_list && walked.slab_leaves == 3) ? find_slab_kernel(b.wpe) : nullptr;
    // ... and, at 16 samples per pixel in workgroups of 256 threads, its form with both compiled in.  RTGO_NO_UNIT16: off.
    const RenderKernel unit16_kernel = (slab_kernel && !kn.no_unit16) ? find_unit16_kernel(b.wpe, nn, b.block) : nullptr;
    // ... and, where the room also holds the world-axis certificate with a margin below 2 % of its thinnest slab at this launch's reach
    // (rtgo_room_world.h), the form of that kernel that steers the room in world axes.  RTGO_NO_ROOMW: off.
    const float room_mu = (unit16_kernel && !kn.no_roomw) ? room_world_margin(walked.room_world, p.cub_mu, c->guard_reach) : -1.0f;
    const RenderKernel roomw_kernel = room_mu > 0.0f ? find_roomw_kernel(unit16_kernel) : nullptr;
    const RenderKernel kernel = roomw_kernel ? roomw_kernel : unit16_kernel ? unit16_kernel : (slab_kernel ? slab_kernel : (pair_kernel ? pair_kernel : find_kernel(path, canon, b.wpe, pk.stream, stats, frames, use_grid, false, batch)));
    if (pair_kernel) p.stack_depth = 0;   // (fast_pair has no stack: pick_block reserved none, and the lights follow the scene directly)
    if (pair_kernel) pair_words(p, roomw_kernel ? &walked.room_world : nullptr, room_mu);
    const bool pair7 = pair_kernel && b.wpe == 7;
    if (kn.debug) {
        char kname[256];   // (the 7-waves pair kernel is no template instantiation: its name carries its waves)
        // (the slab kernel is named with the pair kernel whose body it is and which RTGO_NO_SLAB=1 would run: readers of this line that
        // ask which walk a launch took -- the pair walk at these waves -- find it where they found it)
        // (likewise the 16 spp form, named with the slab kernel whose body it is and which RTGO_NO_UNIT16=1 would run)
        // (and the world-room form, named with the 16 spp kernel whose body it is and which RTGO_NO_ROOMW=1 would run)
        if (roomw_kernel) std::snprintf(kname, sizeof kname, "render_roomw_kernel, the world-room form of kernel render_unit16_kernel, the 16 spp form of kernel render_slab%d_kernel, the slab form of kernel render_pair%d_kernel", b.wpe, b.wpe);
        else if (unit16_kernel) std::snprintf(kname, sizeof kname, "render_unit16_kernel, the 16 spp form of kernel render_slab%d_kernel, the slab form of kernel render_pair%d_kernel", b.wpe, b.wpe);
        else if (slab_kernel) std::snprintf(kname, sizeof kname, "render_slab%d_kernel, the slab form of kernel render_pair%d_kernel", b.wpe, b.wpe);
        else if (pair7) std::snprintf(kname, sizeof kname, "render_pair7_kernel");
        else std::snprintf(kname, sizeof kname, "%s<%d>", pair_kernel ? "render_pair_kernel" : (batch ? "render_frames_kernel" : "render_kernel"), b.wpe);
        std::fprintf(stderr, "rtgo_launch: %u frame(s), %s walk%s, grid %u x %d threads, %zu B LDS, %d waves/SIMD variant, %d workgroups/CU, %u strips of %u px (%u x %u at %u,%u), %u cold segments in chunks of %u, stack %d, cuboid margin %g, guard reach %g quadric %g, kernel %s\n",
                     n_frames, canon ? "canonical" : "fast", (canon && !stats) ? " (beyond the far-field guard)" : "", b.grid, b.block, b.lds, b.wpe, b.blocks_per_cu, p.n_hot, strip_px, p.hot_w, p.hot_h, p.hot_x0, p.hot_y0, p.n_cold_segs, p.cold_cs, p.stack_depth, p.cub_mu, c->guard_reach, c->guard_quadric, kname);
    }
    if (!kernel) return fail(c, RTGO_E_UNSUPPORTED, "rtgo_launch: no kernel variant for this configuration");
    const unsigned long long culled = (unsigned long long)p.local_rows * p.w - (unsigned long long)p.hot_h * (p.cold_x1 - p.cold_x0) + mask_cold_pixels;
    std::vector<uint32_t> seeds_key;
    // (the batched kernels have no seed pass: they neither read pre-hashed seeds nor leave any, and the next launch hashes inline)
    if (const int rc = plan_seeds(c, p, strip_px, !batch && kernel_has_seed_pass(canon, b.wpe, pk.stream), seeds_key)) return rc;
    c->seeds.ok = false;   // (until this launch is on the stream)
    if (const int rc = enqueue(c, kernel, p, b, pk, canon, culled * nn * n_frames)) return rc;
    if (batch) c->last_variant |= 128u;
    if (pair_kernel) c->last_variant |= 256u;
    if (pair7) c->last_variant |= 512u;
    if (slab_kernel) c->last_variant |= 1024u;
    if (unit16_kernel) c->last_variant |= 2048u;
    if (roomw_kernel) c->last_variant |= 4096u;
    c->seeds_last = (p.seeds ? 1u : 0u) | (p.seeds_next ? 2u : 0u);
    if (p.seeds_next) {
        c->seeds.read = 1 - c->seeds.read;
        c->seeds.frame = p.frame + 1u;
        c->seeds.key = std::move(seeds_key);
        c->seeds.ok = true;
    }
    return RTGO_OK;
}

int rtgo_launch(rtgo_ctx* c, const rtgo_frame* f) { return launch_frame(c, f, 1, true, nullptr); }

int rtgo_launch_frames(rtgo_ctx* c, const rtgo_frame* f, uint32_t n_frames)
{
    if (!c || !f) return fail(c, RTGO_E_INVALID, "rtgo_launch_frames: NULL argument");
    if (n_frames == 0 || (uint64_t)f->frame_count + n_frames > (1ull << 32))
        return fail(c, RTGO_E_INVALID, "rtgo_launch_frames: n_frames must be positive and frame_count + n_frames must not pass 2^32");
    if (n_frames == 1) return rtgo_launch(c, f);
    bool unbatched = false;
    if (const int rc = launch_frame(c, f, n_frames, false, &unbatched)) return rc;
    if (!unbatched) return RTGO_OK;
    // what the batched kernels do not cover (more than 16 spp, the grid, the canonical walk, large scenes): a launch per frame
    rtgo_frame g = *f;
    for (uint32_t k = 0; k < n_frames; ++k) {
        g.frame_count = f->frame_count + k;
        if (const int rc = launch_frame(c, &g, 1, false, nullptr)) return rc;
    }
    return RTGO_OK;
}

int rtgo_assemble_bands(rtgo_ctx* c, void* hip_stream, const void* d_gathered, void* d_full, uint32_t w, uint32_t h, uint32_t band_h,
                        uint32_t n_ranks, uint32_t rows_pad, uint32_t elem_bytes)
{
    if (!c || !d_gathered || !d_full) return fail(c, RTGO_E_INVALID, "rtgo_assemble_bands: NULL argument");
    if (w == 0 || h == 0 || n_ranks == 0 || (elem_bytes != 4 && elem_bytes != 16))
        return fail(c, RTGO_E_INVALID, "rtgo_assemble_bands: empty window, no ranks, or element size not 4 / 16");
    if (band_h == 0) band_h = 4;
    for (uint32_t g = 0; g < n_ranks; ++g)
        if (rtgo_local_rows(h, band_h, n_ranks, g) > rows_pad) return fail(c, RTGO_E_INVALID, "rtgo_assemble_bands: rows_pad smaller than a rank's share");
    RTGO_HIP(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const uint64_t row_bytes = (uint64_t)w * elem_bytes;
    const bool wide = (row_bytes % 16 == 0) && (((uintptr_t)d_gathered | (uintptr_t)d_full) % 16 == 0);
    const uint64_t units = (wide ? row_bytes / 16 : row_bytes / 4) * h;
    uint64_t blocks = (units + 255) / 256;
    const uint64_t cap = (uint64_t)c->num_cus * 16;
    if (blocks > cap) blocks = cap;
    if (wide)
        hipLaunchKernelGGL(assemble_bands_kernel<uint4>, dim3((unsigned int)blocks), dim3(256), 0, st, (const uint4*)d_gathered, (uint4*)d_full,
                           (unsigned int)(row_bytes / 16), h, band_h, n_ranks, rows_pad);
    else
        hipLaunchKernelGGL(assemble_bands_kernel<unsigned int>, dim3((unsigned int)blocks), dim3(256), 0, st, (const unsigned int*)d_gathered,
                           (unsigned int*)d_full, (unsigned int)(row_bytes / 4), h, band_h, n_ranks, rows_pad);
    RTGO_HIP(c, hipGetLastError());
    return RTGO_OK;
}

}  // extern "C"

// ---- the whitted triangle path: what its entry points call is in rtgo_whitted_host.h.  (Included here, below rtgo_create: the compiler
// emits the kernel instantiations in the order the host code first names them, and rtgo_create's lists set that order.)
#include "rtgo_whitted_host.h"

extern "C" {

int rtgo_whitted_set_mesh(rtgo_ctx* c, const float* positions, const float* normals, uint32_t n_vertices, const uint32_t* indices,
                          const uint32_t* material_of_triangle, uint32_t n_triangles, const rtgo_pbr* materials, uint32_t n_materials)
{
    if (!c || !positions || !indices || !materials) return fail(c, RTGO_E_INVALID, "rtgo_whitted_set_mesh: NULL argument");
    if (n_triangles == 0 || n_triangles > RTGO_MAX_TRIANGLES || n_vertices == 0 || n_materials == 0)
        return fail(c, RTGO_E_UNSUPPORTED, "rtgo_whitted_set_mesh: triangle count must be in [1, " + std::to_string(RTGO_MAX_TRIANGLES) + "], vertices and materials non-empty");
    const rtgo_whitted_mesh mesh = {positions, normals, nullptr, n_vertices, indices, material_of_triangle, n_triangles};
    return whitted_set_mesh(c, "rtgo_whitted_set_mesh", mesh, materials, n_materials, false);
}

int rtgo_whitted_set_mesh_device(rtgo_ctx* c, const void* d_positions, const void* d_normals, uint32_t n_vertices, const void* d_indices,
                                 const void* d_material_of_triangle, uint32_t n_triangles, const rtgo_pbr* materials, uint32_t n_materials)
{
    const std::string w = "rtgo_whitted_set_mesh_device";
    if (!c || !d_positions || !d_indices || !materials) return fail(c, RTGO_E_INVALID, w + ": NULL argument");
    if (!aligned4(d_positions) || !aligned4(d_normals) || !aligned4(d_indices) || !aligned4(d_material_of_triangle))
        return fail(c, RTGO_E_INVALID, w + ": a pointer is not 4-byte aligned");
    if (n_triangles == 0 || n_triangles > RTGO_MAX_TRIANGLES || n_vertices == 0 || n_materials == 0)
        return fail(c, RTGO_E_UNSUPPORTED, w + ": triangle count must be in [1, " + std::to_string(RTGO_MAX_TRIANGLES) + "], vertices and materials non-empty");
    const rtgo_whitted_mesh mesh = {static_cast<const float*>(d_positions), static_cast<const float*>(d_normals), nullptr, n_vertices,
                                    static_cast<const uint32_t*>(d_indices), static_cast<const uint32_t*>(d_material_of_triangle), n_triangles};
    return whitted_set_mesh(c, w.c_str(), mesh, materials, n_materials, true);
}

// (rtgo_whitted_host.h's stages over a scene built aside: a refusal by the checks leaves the old scene; once that is dropped, a failure leaves none)
int rtgo_whitted_set_scene(rtgo_ctx* c, const rtgo_whitted_mesh* meshes, uint32_t n_meshes, const rtgo_whitted_instance* instances, uint32_t n_instances,
                           const rtgo_pbr* materials, uint32_t n_materials)
{
    if (!c || !meshes || !instances || !materials) return fail(c, RTGO_E_INVALID, "rtgo_whitted_set_scene: NULL argument");
    if (n_meshes == 0 || n_meshes > RTGO_WHITTED_MAX_MESHES || n_materials == 0)
        return fail(c, RTGO_E_UNSUPPORTED, "rtgo_whitted_set_scene: mesh count must be in [1, " + std::to_string(RTGO_WHITTED_MAX_MESHES) + "], materials non-empty");
    return whitted_set_scene(c, "rtgo_whitted_set_scene", meshes, n_meshes, instances, n_instances, materials, n_materials, false);
}

int rtgo_whitted_set_scene_device(rtgo_ctx* c, const rtgo_whitted_mesh* meshes, uint32_t n_meshes, const rtgo_whitted_instance* instances, uint32_t n_instances,
                                  const rtgo_pbr* materials, uint32_t n_materials)
{
    const std::string w = "rtgo_whitted_set_scene_device";
    if (!c || !meshes || !instances || !materials) return fail(c, RTGO_E_INVALID, w + ": NULL argument");
    if (n_meshes == 0 || n_meshes > RTGO_WHITTED_MAX_MESHES || n_materials == 0)
        return fail(c, RTGO_E_UNSUPPORTED, w + ": mesh count must be in [1, " + std::to_string(RTGO_WHITTED_MAX_MESHES) + "], materials non-empty");
    return whitted_set_scene(c, w.c_str(), meshes, n_meshes, instances, n_instances, materials, n_materials, true);
}

int rtgo_whitted_set_instances(rtgo_ctx* c, const rtgo_whitted_instance* instances, uint32_t n_instances)
{
    if (!c) return RTGO_E_INVALID;
    if (!c->wm.instanced) return fail(c, RTGO_E_STATE, "rtgo_whitted_set_instances: no instanced scene (call rtgo_whitted_set_scene first)");
    std::vector<whitted::InstShade> shade;
    std::vector<float> box_pos;
    if (const int rc = whitted_prepare_instances(c, c->wm.meshes, (uint32_t)c->wm.n_materials, instances, n_instances, shade, box_pos, "rtgo_whitted_set_instances")) return rc;
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    return whitted_build_top(c, c->wm, shade, box_pos, instances, "rtgo_whitted_set_instances");
}

int rtgo_whitted_update_mesh(rtgo_ctx* c, uint32_t mesh, const float* positions, const float* normals, uint32_t n_vertices)
{
    if (!c) return RTGO_E_INVALID;
    if (c->wm.triangles == 0) return fail(c, RTGO_E_STATE, "rtgo_whitted_update_mesh: no mesh (call rtgo_whitted_set_mesh or rtgo_whitted_set_scene first)");
    return whitted_update_mesh(c, mesh, positions, normals, n_vertices);
}

int rtgo_whitted_update_meshes(rtgo_ctx* c, const rtgo_whitted_mesh_update* updates, uint32_t n_updates)
{
    if (!c) return RTGO_E_INVALID;
    if (c->wm.triangles == 0) return fail(c, RTGO_E_STATE, "rtgo_whitted_update_meshes: no mesh (call rtgo_whitted_set_mesh or rtgo_whitted_set_scene first)");
    return whitted_update_meshes(c, updates, n_updates);
}

int rtgo_whitted_rebuild_meshes(rtgo_ctx* c, const rtgo_whitted_mesh_update* updates, uint32_t n_updates)
{
    if (!c) return RTGO_E_INVALID;
    if (c->wm.triangles == 0) return fail(c, RTGO_E_STATE, "rtgo_whitted_rebuild_meshes: no mesh (call rtgo_whitted_set_mesh or rtgo_whitted_set_scene first)");
    return whitted_rebuild_meshes(c, updates, n_updates);
}

int rtgo_whitted_update_meshes_device(rtgo_ctx* c, const rtgo_whitted_mesh_update* updates, uint32_t n_updates, uint32_t flags)
{
    if (!c) return RTGO_E_INVALID;
    if (flags & ~(uint32_t)RTGO_UPDATE_REBUILD) return fail(c, RTGO_E_INVALID, "rtgo_whitted_update_meshes_device: unknown flag bits");
    if (c->wm.triangles == 0) return fail(c, RTGO_E_STATE, "rtgo_whitted_update_meshes_device: no mesh (call rtgo_whitted_set_mesh or rtgo_whitted_set_scene first)");
    return whitted_update_meshes_device(c, updates, n_updates, (flags & RTGO_UPDATE_REBUILD) != 0);
}

int rtgo_whitted_set_instances_device(rtgo_ctx* c, const void* d_instances, uint32_t n_instances, uint32_t flags)
{
    const std::string w = "rtgo_whitted_set_instances_device";
    if (!c) return RTGO_E_INVALID;
    if (flags & ~(uint32_t)RTGO_UPDATE_REBUILD) return fail(c, RTGO_E_INVALID, w + ": unknown flag bits");
    const bool rebuild = (flags & RTGO_UPDATE_REBUILD) != 0;
    if (const int rc = whitted_check_instances_args(c, w, d_instances, n_instances, !rebuild)) return rc;
    return whitted_set_instances_device(c, d_instances, n_instances, rebuild);
}

int rtgo_whitted_refit_instances_device_async(rtgo_ctx* c, const void* d_instances, uint32_t n_instances, uint64_t* ticket)
{
    const std::string w = "rtgo_whitted_refit_instances_device_async";
    if (!c) return RTGO_E_INVALID;
    if (!ticket) return fail(c, RTGO_E_INVALID, w + ": NULL ticket");
    if (const int rc = whitted_check_instances_args(c, w, d_instances, n_instances, true)) return rc;
    return whitted_refit_instances_async(c, d_instances, n_instances, ticket);
}

int rtgo_whitted_refit_instances_status(rtgo_ctx* c, uint64_t ticket, rtgo_update_status* out)
{
    const std::string w = "rtgo_whitted_refit_instances_status";
    if (!c || !out) return fail(c, RTGO_E_INVALID, w + ": NULL argument");
    *out = rtgo_update_status{RTGO_UPDATE_APPLIED, 0, 0, 0};
    const rtgo_ctx::UpdateRing& ring = c->w_updates;
    if (!ring.holds(ticket)) return fail(c, RTGO_E_INVALID, w + ": ticket " + std::to_string(ticket) + " was never issued or has left the ring of the last 64");
    const unsigned int slot = rtgo_ctx::UpdateRing::slot(ticket);
    RTGO_HIP(c, hipSetDevice(c->device));
    const hipError_t e = hipEventQuery(ring.done[slot].get());
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();   // (not an error: the next call's hipGetLastError must not find it)
        out->state = RTGO_UPDATE_PENDING;
        return RTGO_OK;
    }
    RTGO_HIP(c, e);
    const unsigned int* v = ring.h.get() + (size_t)slot * kVerdictWords;
    const int kind = lowest_fault(v, whitted::kInstVerdictKinds);   // (rtgo_whitted_set_instances_device's choice for its message)
    if (kind >= 0) *out = rtgo_update_status{RTGO_UPDATE_REFUSED, (uint32_t)kind + 1u, v[kind], 0};
    return RTGO_OK;
}

int rtgo_whitted_set_texcoords(rtgo_ctx* c, const float* uv, uint32_t n_vertices)
{
    if (!c) return RTGO_E_INVALID;
    if (c->wm.triangles == 0) return fail(c, RTGO_E_STATE, "rtgo_whitted_set_texcoords: no mesh (call rtgo_whitted_set_mesh first)");
    if (c->wm.instanced) return fail(c, RTGO_E_STATE, "rtgo_whitted_set_texcoords: an instanced scene takes its texture coordinates per mesh (rtgo_whitted_set_scene)");
    if (uv && n_vertices != (uint32_t)c->wm.n_vertices) return fail(c, RTGO_E_INVALID, "rtgo_whitted_set_texcoords: one (u, v) per vertex of the mesh");
    return whitted_set_texcoords(c, "rtgo_whitted_set_texcoords", uv, n_vertices, false);
}

int rtgo_whitted_set_texcoords_device(rtgo_ctx* c, const void* d_uv, uint32_t n_vertices)
{
    const std::string w = "rtgo_whitted_set_texcoords_device";
    if (!c) return RTGO_E_INVALID;
    if (!aligned4(d_uv)) return fail(c, RTGO_E_INVALID, w + ": the pointer is not 4-byte aligned");
    if (c->wm.triangles == 0) return fail(c, RTGO_E_STATE, w + ": no mesh (call rtgo_whitted_set_mesh first)");
    if (c->wm.instanced) return fail(c, RTGO_E_STATE, w + ": an instanced scene takes its texture coordinates per mesh (rtgo_whitted_set_scene)");
    if (d_uv && n_vertices != (uint32_t)c->wm.n_vertices) return fail(c, RTGO_E_INVALID, w + ": one (u, v) per vertex of the mesh");
    return whitted_set_texcoords(c, w.c_str(), static_cast<const float*>(d_uv), n_vertices, true);
}

int rtgo_whitted_set_material_textures(rtgo_ctx* c, uint32_t material, const rtgo_texture* base_color, const rtgo_texture* metallic_roughness,
                                       const rtgo_texture* normal)
{
    if (!c) return RTGO_E_INVALID;
    if (c->wm.triangles == 0) return fail(c, RTGO_E_STATE, "rtgo_whitted_set_material_textures: no mesh (call rtgo_whitted_set_mesh first)");
    if (material >= (uint32_t)c->wm.n_materials) return fail(c, RTGO_E_INVALID, "rtgo_whitted_set_material_textures: material index beyond the table");
    const rtgo_texture* in[3] = {base_color, metallic_roughness, normal};
    for (const rtgo_texture* t : in)
        if (t && (!t->rgba8 || t->width == 0 || t->height == 0 || t->width > 16384 || t->height > 16384))
            return fail(c, RTGO_E_INVALID, "rtgo_whitted_set_material_textures: a texture needs texels and a size in [1, 16384]^2");
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    WhittedMesh& wm = c->wm;
    std::array<DeviceArray<uchar4>, 3> texels;
    whitted::Tex out[3] = {};
    for (int k = 0; k < 3; ++k) {
        if (!in[k]) continue;
        RTGO_HIP(c, texels[k].upload((const uchar4*)in[k]->rgba8, (size_t)in[k]->width * in[k]->height, c->stream));
        out[k] = whitted::Tex{texels[k].get(), in[k]->width, in[k]->height};
    }
    if (!wm.mat_tex.get()) RTGO_HIP(c, wm.mat_tex.alloc((size_t)wm.n_materials));
    if (wm.mat_tex_host.empty()) {
        wm.mat_tex_host.assign((size_t)wm.n_materials, whitted::MatTex{{nullptr, 0, 0}, {nullptr, 0, 0}, {nullptr, 0, 0}});
        wm.texels.resize((size_t)wm.n_materials);
    }
    wm.mat_tex_host[material] = whitted::MatTex{out[0], out[1], out[2]};
    wm.texels[material] = std::move(texels);   // (frees the texel arrays these replace: no launch is in flight)
    RTGO_HIP(c, hipMemcpyAsync(wm.mat_tex.get(), wm.mat_tex_host.data(), (size_t)wm.n_materials * sizeof(whitted::MatTex), hipMemcpyHostToDevice, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    return RTGO_OK;
}

int rtgo_whitted_set_lights(rtgo_ctx* c, const rtgo_point_light* lights, uint32_t n)
{
    if (!c || (n > 0 && !lights)) return fail(c, RTGO_E_INVALID, "rtgo_whitted_set_lights: bad argument");
    if (n > RTGO_MAX_LIGHTS) return fail(c, RTGO_E_UNSUPPORTED, "rtgo_whitted_set_lights: at most " + std::to_string(RTGO_MAX_LIGHTS) + " lights");
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    if (!c->w_lights.get()) RTGO_HIP(c, c->w_lights.alloc(RTGO_MAX_LIGHTS));
    if (n > 0) RTGO_HIP(c, hipMemcpyAsync(c->w_lights.get(), lights, n * sizeof(whitted::PointLight), hipMemcpyHostToDevice, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    c->w_n_lights = (int)n;
    return RTGO_OK;
}

int rtgo_whitted_set_miss_color(rtgo_ctx* c, const float rgb[3])
{
    if (!c || !rgb) return fail(c, RTGO_E_INVALID, "rtgo_whitted_set_miss_color: NULL argument");
    c->w_miss = v3{rgb[0], rgb[1], rgb[2]};
    return RTGO_OK;
}

int rtgo_whitted_launch(rtgo_ctx* c, uint32_t width, uint32_t height, uint32_t subframe_index)
{
    rtgo_whitted_frame f;
    std::memset(&f, 0, sizeof f);
    f.image_width = width;
    f.image_height = height;
    f.subframe_index = subframe_index;
    return rtgo_whitted_launch_frame(c, &f);
}

// Lanes per pixel of a launch of n subframes (log2; whitted::render_tile_subframes): of 8, 4 and 2 the one that leaves the fewest lanes
// idle in the last chunk, the larger on a tie (2 -> 2, 3 -> 4, 5 -> 2, 7 -> 8, 11 -> 4, 16 -> 8).  RTGO_WHITTED_SUBFRAME_LANES (experiment
// knob; no result depends on it): 1, 2, 4 or 8 instead -- 1 is one lane looping over its pixel's subframes.
static unsigned int whitted_lanes_log2(uint32_t n)
{
    const unsigned int forced = env_uint("RTGO_WHITTED_SUBFRAME_LANES", 0);
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8) return forced == 1 ? 0u : (forced == 2 ? 1u : (forced == 4 ? 2u : 3u));
    unsigned int best = 3;
    for (unsigned int ls = 3; ls >= 1; --ls) {
        auto slots = [&](unsigned int l) { return (((uint64_t)n + (1u << l) - 1) >> l) << l; };
        if (slots(ls) < slots(best)) best = ls;
    }
    return best;
}

// rtgo_whitted_launch_frame (n_subframes 1: the single-subframe kernels) and rtgo_whitted_launch_frames (n_subframes > 1: their FRAMES forms)
static int whitted_launch(rtgo_ctx* c, const rtgo_whitted_frame* f, uint32_t n_subframes)
{
    if (!c) return RTGO_E_INVALID;
    if (!f) return fail(c, RTGO_E_INVALID, "rtgo_whitted_launch: NULL frame");
    if (c->wm.triangles == 0) return fail(c, RTGO_E_STATE, "rtgo_whitted_launch: no mesh (call rtgo_whitted_set_mesh or rtgo_whitted_set_scene)");
    if (!c->have_camera) return fail(c, RTGO_E_STATE, "rtgo_whitted_launch: no camera (call rtgo_set_camera)");
    if (!c->out.accum || !c->out.image) return fail(c, RTGO_E_STATE, "rtgo_whitted_launch: no output (call rtgo_resize or rtgo_bind_output)");
    const uint32_t width = f->image_width, height = f->image_height;
    if (width == 0 || height == 0) return fail(c, RTGO_E_INVALID, "rtgo_whitted_launch: image empty");
    // the window and band of rtgo_launch's frame (rtgo_frame's fields, the same defaults)
    whitted::Share s;
    s.x0 = f->x0;
    s.y0 = f->y0;
    const uint32_t win_w = f->w ? f->w : width, win_h = f->h ? f->h : height;
    if ((uint64_t)s.x0 + win_w > width || (uint64_t)s.y0 + win_h > height) return fail(c, RTGO_E_INVALID, "rtgo_whitted_launch: window outside the image");
    s.band_h = f->band_h ? f->band_h : 4;
    s.n_ranks = f->n_ranks ? f->n_ranks : 1;
    s.rank = f->rank;
    if (s.rank >= s.n_ranks) return fail(c, RTGO_E_INVALID, "rtgo_whitted_launch: rank >= n_ranks");
    s.lw = win_w;
    s.lh = rtgo_local_rows(win_h, s.band_h, s.n_ranks, s.rank);
    if ((uint64_t)s.lh * s.lw > c->out.pixels) return fail(c, RTGO_E_INVALID, "rtgo_whitted_launch: image larger than the output buffers");
    if (f->reserve_cus >= (uint32_t)c->num_cus) return fail(c, RTGO_E_INVALID, "rtgo_whitted_launch: reserve_cus leaves no CU");
    if (s.lh == 0) return RTGO_OK;   // a rank that owns no row of the window: nothing to enqueue
    RTGO_HIP(c, hipSetDevice(c->device));
    if (!c->w_lights.get()) RTGO_HIP(c, c->w_lights.alloc(RTGO_MAX_LIGHTS));
    whitted::Frame fr;
    std::memset(&fr, 0, sizeof fr);
    fr.tile_counter = c->w_tile_counters.get() + (size_t)c->w_launch_parity * whitted::kTileHeads * whitted::kTileHeadStride;
    fr.tile_counter_next = c->w_tile_counters.get() + (size_t)(1 - c->w_launch_parity) * whitted::kTileHeads * whitted::kTileHeadStride;
    // the wave's tile: 8 x 8 pixels, or with 1 << lanes_log2 lanes per pixel 8 x 4, 4 x 4, 4 x 2
    const bool frames = n_subframes > 1;
    fr.n_subframes = n_subframes;
    fr.lanes_log2 = frames ? whitted_lanes_log2(n_subframes) : 0u;
    const unsigned int tile_w = 8u >> (fr.lanes_log2 >> 1), tile_h = 8u >> ((fr.lanes_log2 + 1u) >> 1);
    fr.tiles_x = (s.lw + tile_w - 1) / tile_w;
    fr.tiles_y = (s.lh + tile_h - 1) / tile_h;
    {
        const uint64_t nt = (uint64_t)fr.tiles_x * fr.tiles_y;
        auto gcd = [](uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a; };
        uint64_t stride = (uint64_t)((double)nt * 0.6180339887498949);
        if (stride < 1) stride = 1;
        while (gcd(stride, nt) != 1) ++stride;   // (terminates: nt - 1 and 1 are coprime to nt)
        fr.tile_stride = (unsigned int)(stride % (nt > 1 ? nt : 2));
        if (fr.tile_stride == 0) fr.tile_stride = 1;
    }
    fr.mat_tex = c->wm.mat_tex.get();
    fr.materials = c->wm.materials.get();
    fr.lights = c->w_lights.get();
    fr.n_lights = c->w_n_lights;
    fr.accum = c->out.accum;
    fr.image = c->out.image;
    fr.width = width;
    fr.height = height;
    fr.subframe = f->subframe_index;
    fr.share = s;
    fr.eye = c->eye;
    fr.U = c->U;
    fr.V = c->V;
    fr.W = c->W;
    fr.miss = c->w_miss;
    fr.counters = c->d_counters.get();
    // one persistent workgroup per CU; its LDS holds the lanes' stacks and, beside them, as much of the structure as fits
    const size_t stack_bytes = (size_t)whitted::kRenderBlock * (size_t)c->wm.walk_depth * sizeof(unsigned short);
    const unsigned int n_tiles = fr.tiles_x * fr.tiles_y;
    unsigned int blocks = (n_tiles + (whitted::kRenderBlock / 64) - 1) / (whitted::kRenderBlock / 64);
    // reserve_cus as rtgo_launch takes it: at most half the CUs are left to other streams
    const unsigned int cus = (unsigned int)c->num_cus - (f->reserve_cus < (uint32_t)c->num_cus / 2 ? f->reserve_cus : (uint32_t)c->num_cus / 2);
    if (blocks > cus) blocks = cus;
    int slot = 0;
    return timed_launch(c, slot, [&]() -> int {
        const int rc = whitted_enqueue(c, fr, stack_bytes, env_whitted_mode(), blocks, frames);
        if (rc == RTGO_OK) c->w_launch_parity = 1 - c->w_launch_parity;   // (only once the launch that zeroes the other head is in the stream)
        return rc;
    });
}

int rtgo_whitted_launch_frame(rtgo_ctx* c, const rtgo_whitted_frame* f) { return whitted_launch(c, f, 1); }

int rtgo_whitted_launch_frames(rtgo_ctx* c, const rtgo_whitted_frame* f, uint32_t n_subframes)
{
    if (!c) return RTGO_E_INVALID;
    if (!f) return fail(c, RTGO_E_INVALID, "rtgo_whitted_launch_frames: NULL frame");
    if (n_subframes == 0 || (uint64_t)f->subframe_index + n_subframes > (1ull << 32))
        return fail(c, RTGO_E_INVALID, "rtgo_whitted_launch_frames: n_subframes must be positive and subframe_index + n_subframes must not pass 2^32");
    return whitted_launch(c, f, n_subframes);
}

// ---- ray queries (rtgo_trace.h) ----


// Fewer rays than this walk the analytic scene from global memory: every workgroup of the LDS form copies the whole scene first (61 KB
// for checkered).  From the smallest batch measured on, the copy repays itself (the measurement).
static constexpr uint32_t kTraceLdsMinRays = 64;
static constexpr uint32_t kTraceMaxRays = 1u << 30;
static constexpr size_t kTraceLds = 160 * 1024;

// the checks both entry points share; RTGO_OK with n == 0 means "nothing to do"
static int trace_check(rtgo_ctx* c, const void* d_rays, void* d_hits, uint32_t n, uint32_t flags, const char* what)
{
    if (!c) return RTGO_E_INVALID;
    if (!d_rays || !d_hits) return fail(c, RTGO_E_INVALID, std::string(what) + ": NULL ray or hit buffer");
    if (((uintptr_t)d_rays | (uintptr_t)d_hits) & 15u) return fail(c, RTGO_E_INVALID, std::string(what) + ": ray and hit buffers must be 16-byte aligned");
    if (flags & ~(uint32_t)RTGO_TRACE_ANY_HIT) return fail(c, RTGO_E_INVALID, std::string(what) + ": unknown flag bits");
    if (n > kTraceMaxRays) return fail(c, RTGO_E_INVALID, std::string(what) + ": more than 2^30 rays");
    return RTGO_OK;
}

// The grid of a grid-stride launch: enough workgroups for the batch, at most per_cu on every CU, at most RTGO_TRACE_BLOCKS
static unsigned int trace_grid(const rtgo_ctx* c, uint32_t n, int block, int per_cu)
{
    const uint64_t need = ((uint64_t)n + (uint64_t)block - 1) / (uint64_t)block;
    uint64_t grid = (uint64_t)c->num_cus * (uint64_t)(per_cu > 0 ? per_cu : 1);
    if (grid > need) grid = need;
    const unsigned int cap = env_uint("RTGO_TRACE_BLOCKS", 0);
    if (cap && grid > cap) grid = cap;
    return (unsigned int)grid;
}

// What the two ray-batch calls of the analytic path share (rtgo_trace_rays, rtgo_shade_rays): whether the workgroups stage the scene in
// LDS, the stacks' depth, the workgroup and its LDS.  A workgroup's LDS is the scene copy (when staged), `group_bytes` of its own, and a
// stack per lane.  max_waves: waves a CU can hold of the kernel (its registers).
struct AnalyticRaysPlan {
    bool in_lds;
    int stack_depth, block, per_cu;
    size_t lds;
};
static bool analytic_rays_plan(const AnalyticScene& sc, uint32_t n, size_t group_bytes, int max_waves, AnalyticRaysPlan& plan)
{
    const int n_prims = (int)sc.n_prims, n_nodes = 2 * n_prims - 1;
    // the stacks as deep as the canonical instantiations have them: kStackDepth over a scene of rtgo_set_scene (its build checks the
    // tree against it), the tree's own depth over a scene of rtgo_set_large_scene
    plan.stack_depth = sc.large ? (sc.lbvh_depth > 0 ? sc.lbvh_depth : 1) : kStackDepth;
    const size_t scene_lds = (size_t)(2 * n_nodes + 6 * n_prims) * sizeof(float4);
    // the workgroup that puts the most waves on a CU (pick_block's rule: the scene copy is per workgroup, the stacks per lane), at
    // most max_waves, the smallest on ties
    auto pick = [&](bool in_lds, int& block, int& per_cu, size_t& lds) {
        int best_waves = 0;
        for (int bs = 64; bs <= kMaxBlock; bs *= 2) {
            const size_t l = (in_lds ? scene_lds : 0) + group_bytes + (size_t)plan.stack_depth * bs * sizeof(float2);
            int k = (int)(kTraceLds / l);
            if (k * (bs / 64) > max_waves) k = max_waves / (bs / 64);
            if (k * (bs / 64) > best_waves) {
                best_waves = k * (bs / 64);
                block = bs;
                per_cu = k;
                lds = l;
            }
        }
        return best_waves > 0;
    };
    const int mode = env_trace_mode();
    plan.block = plan.per_cu = 0;
    plan.lds = 0;
    plan.in_lds = !sc.large && sc.n_prims <= (uint32_t)kMaxPrims && (mode == 1 || (mode < 0 && n >= kTraceLdsMinRays));
    if (plan.in_lds && !pick(true, plan.block, plan.per_cu, plan.lds)) plan.in_lds = false;
    return plan.in_lds || pick(false, plan.block, plan.per_cu, plan.lds);
}

int rtgo_trace_rays(rtgo_ctx* c, const void* d_rays, void* d_hits, uint32_t n, uint32_t flags)
{
    if (const int rc = trace_check(c, d_rays, d_hits, n, flags, "rtgo_trace_rays")) return rc;
    const AnalyticScene& sc = c->scene;
    if (sc.n_prims == 0) return fail(c, RTGO_E_STATE, "rtgo_trace_rays: no scene (call rtgo_set_scene or rtgo_set_large_scene)");
    if (n == 0) return RTGO_OK;
    TraceParams p;
    std::memset(&p, 0, sizeof p);
    p.nodes = sc.d_nodes.get();
    p.prims = sc.d_prims.get();
    p.rays = (const float4*)d_rays;
    p.hits = (float4*)d_hits;
    p.n = n;
    p.n_prims = (int)sc.n_prims;
    p.n_nodes = 2 * (int)sc.n_prims - 1;
    AnalyticRaysPlan plan;
    if (!analytic_rays_plan(sc, n, 0, 32, plan)) return fail(c, RTGO_E_UNSUPPORTED, "rtgo_trace_rays: the walk's stacks do not fit in LDS");
    p.stack_depth = plan.stack_depth;
    const unsigned int grid = trace_grid(c, n, plan.block, plan.per_cu);
    RTGO_HIP(c, hipSetDevice(c->device));
    if (plan.in_lds) hipLaunchKernelGGL(trace_rays_kernel<true>, dim3(grid), dim3(plan.block), plan.lds, c->stream, p);
    else hipLaunchKernelGGL(trace_rays_kernel<false>, dim3(grid), dim3(plan.block), plan.lds, c->stream, p);
    RTGO_HIP(c, hipGetLastError());
    c->trace_rays += n;
    if (flags & RTGO_TRACE_ANY_HIT) c->trace_rays_any += n;   // (the analytic path has no any-hit walk: the closest walk answers)
    return RTGO_OK;
}

// The render launches' queues, trial and counters of launches are not touched: the kernel has no work queue.
int rtgo_shade_rays(rtgo_ctx* c, const void* d_rays, const void* d_seeds, void* d_accum, void* d_image, uint32_t n, const rtgo_shade_options* opt)
{
    if (!c) return RTGO_E_INVALID;
    if (!d_rays || !d_accum || !opt) return fail(c, RTGO_E_INVALID, "rtgo_shade_rays: NULL ray buffer, accumulation buffer or options");
    if ((((uintptr_t)d_rays | (uintptr_t)d_accum) & 15u) || (((uintptr_t)d_seeds | (uintptr_t)d_image) & 3u))
        return fail(c, RTGO_E_INVALID, "rtgo_shade_rays: ray and accumulation buffers must be 16-byte aligned, seeds and image 4-byte aligned");
    if (n > kTraceMaxRays) return fail(c, RTGO_E_INVALID, "rtgo_shade_rays: more than 2^30 rays");
    if (opt->path_tracing > 1u || opt->use_ambient > 1u) return fail(c, RTGO_E_INVALID, "rtgo_shade_rays: path_tracing and use_ambient must be 0 or 1");
    if (opt->max_trace_depth < 0 || opt->max_trace_depth > kMaxLevels)
        return fail(c, RTGO_E_UNSUPPORTED, "rtgo_shade_rays: max_trace_depth must be in [0, 5] (reference uses 5, renderer.cpp:616)");
    const AnalyticScene& sc = c->scene;
    if (sc.n_prims == 0) return fail(c, RTGO_E_STATE, "rtgo_shade_rays: no scene (call rtgo_set_scene or rtgo_set_large_scene)");
    if (!opt->path_tracing && c->n_lights < 1) return fail(c, RTGO_E_STATE, "rtgo_shade_rays: distributed mode needs at least one surface light");
    if (n == 0) return RTGO_OK;
    const bool path = opt->path_tracing != 0;
    ShadeParams p;
    std::memset(&p, 0, sizeof p);
    p.nodes = sc.d_nodes.get();
    p.prims = sc.d_prims.get();
    p.lights = c->d_lights.get();
    p.rays = (const float4*)d_rays;
    p.seeds = (const unsigned int*)d_seeds;
    p.accum = (float4*)d_accum;
    p.image = (uchar4*)d_image;
    p.counters = c->d_counters.get();
    p.n = n;
    p.sample_index = opt->sample_index;
    p.n_prims = (int)sc.n_prims;
    p.n_nodes = 2 * (int)sc.n_prims - 1;
    p.n_lights = c->n_lights;
    p.max_depth = opt->max_trace_depth;
    p.ambient = (int)opt->use_ambient;
    p.bg = c->bg;
    // behind the stacks: the light records.  The kernels' registers allow five waves a SIMD in path mode (86 / 93 VGPRs) and four in
    // distributed mode (108 / 111): 20 and 16 a CU
    AnalyticRaysPlan plan;
    if (!analytic_rays_plan(sc, n, kMaxLights * sizeof(LightRec), path ? 20 : 16, plan))
        return fail(c, RTGO_E_UNSUPPORTED, "rtgo_shade_rays: the walk's stacks do not fit in LDS");
    p.stack_depth = plan.stack_depth;
    const dim3 grid(trace_grid(c, n, plan.block, plan.per_cu)), bdim(plan.block);
    RTGO_HIP(c, hipSetDevice(c->device));
    if (path) {
        if (plan.in_lds) hipLaunchKernelGGL((shade_rays_kernel<true, true>), grid, bdim, plan.lds, c->stream, p);
        else hipLaunchKernelGGL((shade_rays_kernel<true, false>), grid, bdim, plan.lds, c->stream, p);
    } else {
        if (plan.in_lds) hipLaunchKernelGGL((shade_rays_kernel<false, true>), grid, bdim, plan.lds, c->stream, p);
        else hipLaunchKernelGGL((shade_rays_kernel<false, false>), grid, bdim, plan.lds, c->stream, p);
    }
    RTGO_HIP(c, hipGetLastError());
    c->trace_rays += n;   // the batch; the bounce and occlusion rays are counted by the kernel
    return RTGO_OK;
}

// What the two ray-batch calls of the triangle path share (rtgo_whitted_trace_rays, rtgo_whitted_shade_rays): the walk's kind, the scene
// half of its parameters, LDS and grid.  Workgroups of 256 lanes: nothing is shared between the lanes but the top level's copy, and the
// tail of a batch is shorter.  max_per_cu: workgroups a CU can hold of the kernel (its registers).
static constexpr int kWhittedRaysBlock = 256;
struct WhittedRaysPlan {
    int kind;
    size_t lds;
    unsigned int grid;
};
static WhittedRaysPlan whitted_rays_plan(const rtgo_ctx* c, const WhittedMesh& wm, uint32_t n, whitted::Params& mesh, whitted::InstParams& inst, int max_per_cu)
{
    const size_t stack_bytes = (size_t)kWhittedRaysBlock * (size_t)(wm.walk_depth > 0 ? wm.walk_depth : 1) * sizeof(unsigned short);
    WhittedRaysPlan plan{whitted::kTraceMesh, stack_bytes, 0};
    if (!wm.instanced) {
        mesh = mesh_params(wm);
    } else {
        inst = inst_params(wm);
        // the top level in LDS where four workgroups a CU still fit with it (RTGO_TRACE_MODE: never / wherever one fits)
        const size_t top_bytes = (size_t)inst.n_top_recs * 4 * sizeof(float4) + (size_t)inst.n_instances * sizeof(whitted::InstWalk);
        const int mode = env_trace_mode();
        const bool in_lds = mode != 0 && top_bytes + stack_bytes <= (mode == 1 ? kTraceLds : kTraceLds / 4);
        if (in_lds) plan.lds += top_bytes;
        plan.kind = inst.clusters ? (in_lds ? whitted::kTraceClusteredLds : whitted::kTraceClustered) : (in_lds ? whitted::kTraceInstLds : whitted::kTraceInst);
    }
    int per_cu = (int)(kTraceLds / plan.lds);
    if (per_cu > max_per_cu) per_cu = max_per_cu;
    plan.grid = trace_grid(c, n, kWhittedRaysBlock, per_cu);
    return plan;
}

int rtgo_whitted_trace_rays(rtgo_ctx* c, const void* d_rays, void* d_hits, uint32_t n, uint32_t flags)
{
    if (const int rc = trace_check(c, d_rays, d_hits, n, flags, "rtgo_whitted_trace_rays")) return rc;
    const WhittedMesh& wm = c->wm;
    if (wm.triangles == 0) return fail(c, RTGO_E_STATE, "rtgo_whitted_trace_rays: no mesh (call rtgo_whitted_set_mesh or rtgo_whitted_set_scene)");
    if (n == 0) return RTGO_OK;
    whitted::TraceRaysParams p;
    std::memset(&p, 0, sizeof p);
    p.rays = (const float4*)d_rays;
    p.hits = (float4*)d_hits;
    p.n = n;
    const bool any = (flags & RTGO_TRACE_ANY_HIT) != 0;
    const WhittedRaysPlan plan = whitted_rays_plan(c, wm, n, p.mesh, p.inst, 8);
    const int kind = plan.kind;
    const size_t lds = plan.lds;
    const dim3 grid(plan.grid), bdim(kWhittedRaysBlock);
    RTGO_HIP(c, hipSetDevice(c->device));
    using namespace whitted;
#define RTGO_WT(K)                                                                                             \
    case K:                                                                                                    \
        if (any) hipLaunchKernelGGL((whitted_trace_kernel<K, true>), grid, bdim, lds, c->stream, p);           \
        else hipLaunchKernelGGL((whitted_trace_kernel<K, false>), grid, bdim, lds, c->stream, p);              \
        break;
    switch (kind) {
        RTGO_WT(kTraceMesh)
        RTGO_WT(kTraceInst)
        RTGO_WT(kTraceInstLds)
        RTGO_WT(kTraceClustered)
        RTGO_WT(kTraceClusteredLds)
    }
#undef RTGO_WT
    RTGO_HIP(c, hipGetLastError());
    c->trace_rays += n;
    if (any) c->trace_rays_any += n;
    return RTGO_OK;
}

// Lights never set: none (the launches allocate the array on first use; this call reads none of it then).  The render launches' tile
// counters and parity are not touched: the kernel has no tile queue.
int rtgo_whitted_shade_rays(rtgo_ctx* c, const void* d_rays, void* d_accum, void* d_image, uint32_t n, uint32_t sample_index)
{
    if (!c) return RTGO_E_INVALID;
    if (!d_rays || !d_accum) return fail(c, RTGO_E_INVALID, "rtgo_whitted_shade_rays: NULL ray or accumulation buffer");
    if ((((uintptr_t)d_rays | (uintptr_t)d_accum) & 15u) || ((uintptr_t)d_image & 3u))
        return fail(c, RTGO_E_INVALID, "rtgo_whitted_shade_rays: ray and accumulation buffers must be 16-byte aligned, the image 4-byte aligned");
    if (n > kTraceMaxRays) return fail(c, RTGO_E_INVALID, "rtgo_whitted_shade_rays: more than 2^30 rays");
    const WhittedMesh& wm = c->wm;
    if (wm.triangles == 0) return fail(c, RTGO_E_STATE, "rtgo_whitted_shade_rays: no mesh (call rtgo_whitted_set_mesh or rtgo_whitted_set_scene)");
    if (n == 0) return RTGO_OK;
    whitted::ShadeRaysParams p;
    std::memset(&p, 0, sizeof p);
    p.rays = (const float4*)d_rays;
    p.accum = (float4*)d_accum;
    p.image = (uchar4*)d_image;
    p.n = n;
    p.sample_index = sample_index;
    // at 128 VGPRs a CU holds four of the kernel's 256-lane workgroups
    const WhittedRaysPlan plan = whitted_rays_plan(c, wm, n, p.mesh, p.inst, 4);
    whitted::Frame& fr = wm.instanced ? p.inst.frame : p.mesh.frame;   // what shade() reads of a frame
    fr.mat_tex = wm.mat_tex.get();
    fr.materials = wm.materials.get();
    fr.lights = c->w_lights.get();
    fr.n_lights = c->w_lights.get() ? c->w_n_lights : 0;
    fr.miss = c->w_miss;
    fr.counters = c->d_counters.get();
    const dim3 grid(plan.grid), bdim(kWhittedRaysBlock);
    RTGO_HIP(c, hipSetDevice(c->device));
    using namespace whitted;
#define RTGO_WS(K)                                                                                 \
    case K:                                                                                        \
        hipLaunchKernelGGL((whitted_shade_kernel<K>), grid, bdim, plan.lds, c->stream, p);         \
        break;
    switch (plan.kind) {
        RTGO_WS(kTraceMesh)
        RTGO_WS(kTraceInst)
        RTGO_WS(kTraceInstLds)
        RTGO_WS(kTraceClustered)
        RTGO_WS(kTraceClusteredLds)
    }
#undef RTGO_WS
    RTGO_HIP(c, hipGetLastError());
    c->trace_rays += n;   // the batch; the occlusion rays are counted by the kernel, in both counters
    return RTGO_OK;
}

int rtgo_sync(rtgo_ctx* c)
{
    if (!c) return RTGO_E_INVALID;
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    c->mask.retired.clear();   // (no launch reads an outgrown hot mask any more)
    return harvest_events(c, c->ev_pending);
}

static int copy_out(rtgo_ctx* c, void* host, const void* dev, size_t bytes, size_t elem)
{
    if (!c || !host) return fail(c, RTGO_E_INVALID, "rtgo_read: NULL argument");
    if (!dev) return fail(c, RTGO_E_STATE, "rtgo_read: no output buffer");
    if (bytes > c->out.pixels * elem) return fail(c, RTGO_E_INVALID, "rtgo_read: more bytes than the output holds");
    int rc = rtgo_sync(c);
    if (rc) return rc;
    RTGO_HIP(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    return RTGO_OK;
}

int rtgo_read_image(rtgo_ctx* c, void* host, size_t bytes) { return copy_out(c, host, c ? c->out.image : nullptr, bytes, sizeof(uchar4)); }
int rtgo_read_accum(rtgo_ctx* c, void* host, size_t bytes) { return copy_out(c, host, c ? c->out.accum : nullptr, bytes, sizeof(float4)); }

int rtgo_write_accum(rtgo_ctx* c, const void* host, size_t bytes)
{
    if (!c || !host) return fail(c, RTGO_E_INVALID, "rtgo_write_accum: NULL argument");
    if (!c->out.accum) return fail(c, RTGO_E_STATE, "rtgo_write_accum: no output buffer");
    if (bytes > c->out.pixels * sizeof(float4)) return fail(c, RTGO_E_INVALID, "rtgo_write_accum: too many bytes");
    int rc = rtgo_sync(c);
    if (rc) return rc;
    RTGO_HIP(c, hipMemcpyAsync(c->out.accum, host, bytes, hipMemcpyHostToDevice, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    return RTGO_OK;
}

int rtgo_get_stats(rtgo_ctx* c, rtgo_stats* out)
{
    if (!c || !out) return fail(c, RTGO_E_INVALID, "rtgo_get_stats: NULL argument");
    int rc = rtgo_sync(c);
    if (rc) return rc;
    unsigned long long h[8];
    RTGO_HIP(c, hipMemcpyAsync(h, c->d_counters.get(), sizeof h, hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    out->rays_total = h[0] + c->trace_rays;
    out->rays_occlusion = h[1] + c->trace_rays_any;
    out->node_visits = h[2];
    out->prim_tests = h[3];
    out->hits = h[4];
    out->last_launch_ms = c->last_ms;
    out->total_launch_ms = c->total_ms;
    out->launches = c->launches;
    out->lbvh_depth = (uint32_t)c->scene.lbvh_depth;
    out->dbg_fast_boxes = h[5];
    out->dbg_fast_tests = h[6];
    out->rays_culled = c->rays_culled;
    out->launches_canonical = c->launches_canonical;
    out->cuboid_groups = (uint32_t)c->scene.tree[0].cuboid_groups;
    out->guard_reach = c->guard_reach;
    out->guard_quadric = c->guard_quadric;
    out->last_variant = c->last_variant;
    out->launches_trial = c->launches_trial;
    return RTGO_OK;
}

int rtgo_reset_stats(rtgo_ctx* c)
{
    if (!c) return RTGO_E_INVALID;
    int rc = rtgo_sync(c);
    if (rc) return rc;
    // on the launch stream: a memset on the null stream is not ordered against a non-blocking stream's kernels
    RTGO_HIP(c, hipMemsetAsync(c->d_counters.get(), 0, 8 * sizeof(unsigned long long), c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    c->total_ms = 0.0f;
    c->last_ms = 0.0f;
    c->launches = 0;
    c->launches_canonical = 0;
    c->launches_trial = 0;
    c->rays_culled = 0;
    c->trace_rays = 0;
    c->trace_rays_any = 0;
    return RTGO_OK;
}

int rtgo_read_bvh(rtgo_ctx* c, void* host_nodes, size_t node_bytes, void* host_inv, size_t inv_bytes, void* host_aabbs, size_t aabb_bytes)
{
    if (!c) return RTGO_E_INVALID;
    const AnalyticScene& sc = c->scene;
    if (sc.n_prims == 0) return fail(c, RTGO_E_STATE, "rtgo_read_bvh: no scene");
    const size_t n = sc.n_prims;
    if ((host_nodes && node_bytes != (2 * n - 1) * 32) || (host_inv && inv_bytes != n * 48) || (host_aabbs && aabb_bytes != n * 24))
        return fail(c, RTGO_E_INVALID, "rtgo_read_bvh: buffer sizes must be (2n-1)*32, n*48, n*24");
    int rc = rtgo_sync(c);
    if (rc) return rc;
    if (host_nodes) RTGO_HIP(c, hipMemcpy(host_nodes, sc.d_nodes.get(), node_bytes, hipMemcpyDeviceToHost));
    if (host_inv) {
        std::vector<float4> tmp(6 * n);
        RTGO_HIP(c, hipMemcpy(tmp.data(), sc.d_prims.get(), 6 * n * sizeof(float4), hipMemcpyDeviceToHost));
        float* o = (float*)host_inv;
        for (size_t i = 0; i < n; ++i) std::memcpy(o + 12 * i, &tmp[6 * i], 48);
    }
    if (host_aabbs) RTGO_HIP(c, hipMemcpy(host_aabbs, sc.d_aabb.get(), aabb_bytes, hipMemcpyDeviceToHost));
    return RTGO_OK;
}

}  // extern "C"
