// rtgo_ctx.h -- what the host side (rtgo_capi.hip and the host headers it includes) shares: the scene structs and the context, error
// reporting, the timed-launch ring, the environment readers, and the few helpers more than one set-up path uses.
#pragma once

#include "../../include/rtgo.h"
#include "rtgo_device.h"
#include "rtgo_large.h"
#include "rtgo_owners.h"
#include "rtgo_room_world.h"
#include "rtgo_shade.h"
#include "rtgo_ticket_ring.h"
#include "rtgo_trace.h"
#include "rtgo_whitted_big.h"
#include "rtgo_whitted_inst.h"
#include "rtgo_whitted_shade.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace rtgo;

// one mesh of an instanced whitted scene (rtgo_whitted_set_scene), host side
struct WhittedMeshInfo {
    float lo[3], hi[3];        // a box around the mesh's root record (the padded triangle bounds, padded once more)
    int rec_base, tri_base, vert_base;   // where its records / triangles / vertices start in the context's arrays
    int root;                  // InstWalk::root
    int flags;                 // whitted::kHasNormals | kHasTexcoords
    int depth;                 // stack entries its walk needs (a clustered mesh: its mid level's + its deepest cluster's)
    uint32_t max_material;     // its largest material_of_triangle
    bool clustered;            // beyond kMaxTriangles triangles: a mid level over clusters (rtgo_whitted_big.h)
    int n_tris, n_verts;
    // what each whitted_build of this mesh wrote into the context's arrays (rtgo_debug_build_digest): records [rec0, rec0 + n_recs) and
    // their quantised forms at qrecs[2 tri0 ..] (tri0 < 0: none kept, a mid level's)
    struct Built { int rec0, n_recs, tri0; whitted::WhittedBuildMeta meta; };   // (meta: what that build reported)
    std::vector<Built> built;
    std::vector<int> mid_order;   // a clustered mesh: the cluster at each leaf position of its mid level (a refit lays the mid level's input out again)
};

// The analytic scene (rtgo_set_scene, rtgo_set_large_scene): replaced as a whole, by assigning a fresh one
struct AnalyticScene {
    // The third structure of the trial (rtgo_ctx::Trial): a uniform grid over structure 0's small primitives (rtgo::fast_grid), built by
    // the host from the boxes build_kernel reports.  Scenes of many small primitives spread evenly (balls: 256 spheres in a room) walk it
    // in a third of the tree's instructions; where it is slower the trial drops it after two launches.
    struct Grid {
        DeviceArray<unsigned char> d;      // [table: n_cells words, 0 = empty cell, else 1 + its record][records: 32 B per listing cell, its box
                                           // and (first item | count << 16)][items: 16-bit positions into d_fprims] (GridParams' offsets)
        int n_nodes = 0;                   // its size in 32-byte units (what LaunchParams::n_fnodes counts)
        int entries = 0;                   // list entries (rtgo_debug_grid)
        rtgo::GridParams gp = {};
        float reach_max = 0.0f;            // the pad of the binning covers the walk's rounding for rays that start within this reach
        bool have = false;
    } grid;
    struct FastTree {                      // what build_kernel makes for one big_frac
        DeviceArray<float4> d_fnodes;      // collapsed LBVH of the fast walk
        DeviceArray<float4> d_fprims;      // Morton-ordered traversal records of the fast walk
        int fast_depth = 0, n_small = 0, n_fnodes = 0;   // its depth, primitives (the rest are tested up front) and nodes
        int cuboid_groups = 0;             // certified groups in the scene (leaves + the list's)
        int tree_spheres = 0;              // every primitive of the tree is a sphere
        bool pair = false;                 // the tree is node 0 over the leaves 1 and 2, both certified cuboids: what render_pair_kernel walks
        int list_cub = 0, n_big_pairs = 0; // the up-front list starts with a certified box (1) / room (2): cuboid_range
        bool slab_list = false;            // the list's cuboid also holds the slab certificate (cuboid_slab)
        int slab_leaves = 0;               // ... and so do the pair kernels' leaves: bit 0 node 1, bit 1 node 2 (0 when `pair` is false)
        rtgo::RoomWorld room_world;        // the list's room in world axes (rtgo_room_world.h; ok = false: it does not hold); a launch adds its reach
        float cub_a = 0.0f, cub_b = 0.0f;  // its margin = kCuboidTol + K (cub_a R + cub_b), R = reach of the launch's rays
        // the last-ray certificate's scene half (emitter_cert): the emitters, the list's records after the room (emit_n = 0: no certificate), and
        // for each (emitter, wall) pair k = 6 e + g the least y_g over the emitter's corners and the coefficients of the margin it
        // has to exceed, K (emit_a R + emit_b) (last_ray_params)
        int emit_n = 0;
        float emit_ymin[6 * kMaxEmitters] = {}, emit_a[6 * kMaxEmitters] = {}, emit_b[6 * kMaxEmitters] = {};
        BuildMeta meta = {};               // build_kernel's meta words as it wrote them (rtgo_debug_read_build)
        bool sane(uint32_t n) const { return n_fnodes >= 0 && n_fnodes <= 2 * (int)n - 1 && !(n_small > 0 && n_fnodes < 1); }
    } tree[2];                             // the structures of 36 % and 15 %
    bool have_alt = false;                 // tree[1] is a candidate: false when the two builds came out the same, or RTGO_BIG_PERCENT pins one
    uint32_t n_prims = 0;                  // 0: no scene (set last, once the build succeeded)
    DeviceArray<PrimIn> d_prims_in;
    DeviceArray<float> d_aabb;
    DeviceArray<float4> d_nodes, d_prims;
    DeviceArray<float4> d_frames;          // shading frames of the flat primitives (2 float4 per primitive, SBT order)
    bool large = false;                    // the scene came from rtgo_set_large_scene: d_nodes / d_prims / d_aabb only, walked from global memory
    int lbvh_depth = 0;
    float bounds[6] = {0, 0, 0, 0, 0, 0};  // tight world bounds of the scene (min xyz, max xyz)
    // far-field guard (rtgo_launch): per sphere / cylinder its centre and smax / smin^2 of its model matrix' axis scales -- the
    // reported hit of a quadric seen from distance D lies up to ~2^-25 D^2 smax / smin^2 off its surface (b^2 - 4ac cancels)
    struct Quadric { float c[3], w; };
    std::vector<Quadric> quadrics;
    DeviceArray<float> d_tight;            // the fast walk's box of every primitive (device), and its host copy
    std::vector<float> tight;
    // ---- what rtgo_update_prims needs of the set call
    bool have_aabbs = false;               // the caller gave boxes (else d_aabb holds the CubeBox rule's)
    std::vector<rtgo_prim> host_prims;     // a scene of rtgo_set_scene: the primitives as last given (emitter_cert and the quadric list read them)
    // a scene of rtgo_set_large_scene: the tree's shape, 20 bytes per primitive (the links are in the nodes themselves)
    struct LargeKeep {
        DeviceArray<int> parent;           // of each of the 2n-1 nodes; -1: the root
        DeviceArray<int> depth;            // of each internal node
        DeviceArray<int> leaf_of;          // each primitive's leaf node
        DeviceArray<unsigned int> mark;    // per internal node: the refit that last changed a box below it (`epoch` then; 0: none)
        unsigned int epoch = 0;
    } keep;
    // rtgo_update_prims_device: one word per primitive, the call that last named it (`epoch` then; 0: none) -- how prims_check_kernel
    // finds an index named twice.  Allocated by the scene's first such call, 4 bytes per primitive; outlives a rebuild.
    struct Claim {
        DeviceArray<unsigned int> d;
        unsigned int epoch = 0;
    } claim;
};

// An instanced scene's top level (rtgo_whitted_set_instances replaces it alone)
struct WhittedTop {
    DeviceArray<float4> recs;
    DeviceArray<whitted::InstWalk> inst;       // in the top level's leaf order
    DeviceArray<whitted::InstShade> shade;     // in the caller's order
    int n_recs = 0, n_instances = 0;
    whitted::WhittedBuildMeta meta = {};       // what its build reported (rtgo_debug_read_build)
};

// What rtgo_whitted_refit_instances_device_async keeps with an instanced scene ("The refit that waits for nothing"):
// allocated by the scene's first such call, reused by every later one (they are ordered on one stream), dropped with the top level or
// the scene.  n: the scene's instances.
struct WhittedInstStaging {
    DeviceArray<whitted::InstShade> shade;     // inst_prepare_kernel's records [n], copied into top.shade behind the gate
    DeviceArray<float> boxes;                  // ... its boxes [6 n]
    DeviceArray<unsigned int> idx;             // ... and index triples [3 n]
    DeviceArray<float4> tris;                  // the leaf order refit_structure reads, and the corners it writes [3 n]
    DeviceArray<uint4> qrecs;                  // the refit's compact records [2 n] (no launch reads a top level's)
    DeviceArray<int> done;                     // the refit's stamps [n_recs]
    // kMetaWords words for the refit's WhittedBuildMeta, then the count of applied updates; read back by whitted_refresh_host
    static constexpr int kMetaWords = 12, kWords = 16;
    DeviceArray<unsigned int> words;
    DeviceArray<unsigned int> kept;            // the instances of the last applied update [14 n]: wm.instances, not yet read back
    // the mesh table inst_prepare_kernel reads (InstMesh, 12 words per mesh) and its pinned image: uploaded when the image differs from
    // wm.meshes, which change only in calls that have drained the stream
    DeviceArray<unsigned int> table;
    PinnedArray<unsigned int> h_table;
    size_t table_words = 0;                    // words uploaded (0: nothing yet)
    // wm.instances and wm.top.meta's grid are behind the device by the updates applied since `adopted`, the count at the last refresh
    unsigned int adopted = 0;
    bool stale = false;                        // an update was enqueued since the last refresh
};

// The whitted triangle path's scene (rtgo_whitted.h; rtgo_whitted_set_mesh, rtgo_whitted_set_scene): replaced as a whole
struct WhittedMesh {
    DeviceArray<float> positions, normals;
    DeviceArray<float> texcoords;              // 2 floats per vertex, or empty
    DeviceArray<unsigned int> indices, tri_material;
    DeviceArray<whitted::Pbr> materials;
    // textures: per material its three texel arrays, the table that points into them, and its device copy (empty while no material
    // has a texture)
    std::vector<std::array<DeviceArray<uchar4>, 3>> texels;
    std::vector<whitted::MatTex> mat_tex_host;
    DeviceArray<whitted::MatTex> mat_tex;
    DeviceArray<float4> recs, tris;            // the walk's records (4 float4 each) and the triangles in Morton order (3 float4 each)
    DeviceArray<uint4> qrecs;                  // the compact form: quantised records, (vertex indices | triangle index) per triangle
    DeviceArray<uint2> tidx;
    int n_vertices = 0, walk_depth = 0;
    whitted::WhittedBuildMeta meta = {};       // what the build reported (one mesh: its n_recs and grid are what the launches read)
    int triangles = 0, n_materials = 0;        // triangles = 0: no mesh
    // an instanced scene (rtgo_whitted_set_scene): the mesh buffers above hold every mesh back to back in object space, plus the top level
    bool instanced = false;
    std::vector<WhittedMeshInfo> meshes;
    int mesh_depth = 0;                        // the deepest mesh walk
    WhittedTop top;
    WhittedInstStaging staging;                // (while staging.stale, `instances` and top.meta's grid wait for whitted_refresh_host)
    std::vector<rtgo_whitted_instance> instances;   // the caller's instances as last given (rtgo_whitted_update_mesh lays them out again)
    DeviceArray<int4> clusters;                // the clustered meshes' cluster tables (InstParams::clusters), or empty when there are none
};

struct rtgo_ctx {
    int device = 0;
    int num_cus = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // ring of HIP-event pairs bracketing each megakernel launch on the launch stream (launches are asynchronous, so the
    // elapsed times are harvested later: at rtgo_sync, or when the ring wraps)
    static constexpr int kEvRing = 64;
    hipEvent_t ev_start[kEvRing] = {}, ev_stop[kEvRing] = {};
    int ev_head = 0, ev_pending = 0;
    unsigned char ev_tag[kEvRing] = {};    // a trial launch of candidate k carries k + 1, any other launch 0 (see `trial` below)
    DeviceArray<unsigned int> d_queue;     // two sets of work-queue heads: a launch counts on one and zeroes the other for the next
    int queue_set = 0;
    DeviceArray<unsigned long long> d_counters;   // 8 x u64
    DeviceArray<LightRec> d_lights;
    int n_lights = 0;
    DeviceArray<int> d_meta;               // build_kernel's meta words (one build at a time)
    DeviceArray<unsigned int> d_verdict;   // prims_check_kernel's or inst_prepare_kernel's verdict (kVerdictWords; allocated by the first device-pointer call)
    // rtgo_update_prims_device_async: the tickets (rtgo_ticket_ring.h) and what each slot holds.  Allocated by the
    // context's first such call, then reused: no call after it allocates or frees.
    struct UpdateRing : TicketRing {
        DeviceArray<unsigned int> d;       // kSlots verdicts of kVerdictWords words, then kSlots `changed` words
        PinnedArray<unsigned int> h;       // the verdicts as copied back behind each check
        LazyEvent done[kSlots];            // recorded behind that copy: what rtgo_update_prims_status queries
    } updates;
    // rtgo_whitted_refit_instances_device_async: a ring of its own, of the same shape (d: kSlots verdicts alone).  The two rings count
    // their tickets separately: a number means one update here and another there.
    UpdateRing w_updates;
    int leaf_budget = kDefaultLeafBudget;
    bool have_camera = false;
    v3 eye{0, 0, 0}, U{0, 0, 0}, V{0, 0, 0}, W{0, 0, 0}, bg{0, 0, 0};
    // stats (rtgo_get_stats)
    float guard_reach = 0.0f, guard_quadric = 0.0f;   // of the last launch
    unsigned long long rays_culled = 0;       // since rtgo_reset_stats (host arithmetic: the cold pixels of each launch x N*N)
    uint32_t launches_canonical = 0;          // since rtgo_reset_stats
    uint32_t launches_trial = 0, last_variant = 0;
    float total_ms = 0.0f, last_ms = 0.0f;
    uint32_t launches = 0;
    uint32_t seeds_last = 0;                  // rtgo_debug_seeds: 1 = the last launch read pre-hashed seeds, 2 = it wrote the next frame's
    unsigned long long trace_rays = 0, trace_rays_any = 0;   // rays of rtgo_trace_rays / rtgo_whitted_trace_rays / rtgo_whitted_shade_rays (its batch; its occlusion rays are the kernel's count) since rtgo_reset_stats (host arithmetic)
#ifdef RTGO_CMPWALK
    DeviceArray<float> d_cmp;                 // diagnostic build: disagreements between the two walks
#endif
#ifdef RTGO_TIMELINE
    DeviceArray<unsigned long long> d_timeline;   // diagnostic build: 8 x u64 per wave
    unsigned int timeline_waves = 0;
#endif

    AnalyticScene scene;
    // ---- launch caches of the analytic path
    // Frames of several passes per pixel (> 16 spp) have two kernels with bitwise the same output: lanes streaming through their
    // samples (open scenes, where path lengths differ: plateau 3840x2160 spp 256 18.8 ms against 20.5) or the wave running pass by
    // pass in lock-step (closed scenes, where nearly every path runs to the depth limit and regeneration only costs: cornell spp 64
    // 4.42 ms against 4.9).  Which one is faster is a property of scene and frame that the host cannot see, but the launch times
    // it takes anyway tell: the first four launches of a (scene, frame geometry, spp, mode) alternate between the two, the faster
    // minimum keeps the job.
    // Round 3: the same trial also decides WHICH fast-walk structure a launch walks.  How big a primitive has to be to be tested up
    // front by every ray instead of sitting in the tree (build_kernel's big_frac) is worth 20 % on plateau (nearly everything up front:
    // a dozen tests at full lanes beat a walk at a third of them) and costs 20 % on cornell (its two boxes lose their cuboid leaves), and
    // no rule read off the scene predicts it (profiles/r03n/big_sweep.log); so rtgo_set_scene builds the structure twice -- 36 % and 15 % --
    // and the candidates of a trial are (loop, structure) pairs: every candidate gets two timed launches, the best minimum keeps the job.
    // All candidates return the same pixels bit for bit (any tree over the same primitives returns the same closest hit).
    struct Trial {
        std::vector<uint32_t> key;
        int issued = 0, done = 0;
        float best[8] = {1e30f, 1e30f, 1e30f, 1e30f, 1e30f, 1e30f, 1e30f, 1e30f};
        int choice = -1;                   // index of the winning candidate, -1 = undecided
    } trial;
    // per-strip mask of the scene's screen rectangle (LaunchParams::hot_mask), kept until the launch geometry changes; its buffers
    // outlive a scene
    struct HotMask {
        DeviceArray<unsigned int> d;
        std::vector<DeviceArray<unsigned int>> retired;   // masks outgrown while launches that read them may be queued; freed by rtgo_sync
        // pinned staging for its upload, two slots used in turn with an event each: a camera change (every frame of an interactive
        // drag) rebuilds the mask, and the upload must not make the host wait for the stream
        PinnedArray<unsigned int> h[2];
        LazyEvent copied[2];
        int slot = 0;
        std::vector<uint32_t> key;         // what the cached mask was built for
        bool all_hot = true;
        unsigned long long cold_pixels = 0;
    } mask;
    // next frame's pixel seeds (LaunchParams::seeds): two buffers, a launch reads one and writes the other.  ok: the buffer `read`
    // holds frame `frame`'s seeds for the strip layout `key` (written by the last launch on this context)
    struct Seeds {
        DeviceArray<unsigned int> d[2];
        int read = 0;
        bool ok = false;
        uint32_t frame = 0;
        std::vector<uint32_t> key;
    } seeds;
    // ---- output: the context's own buffers (rtgo_resize) or the caller's (rtgo_bind_output)
    struct Output {
        DeviceArray<float4> own_accum;
        DeviceArray<uchar4> own_image;
        float4* accum = nullptr;           // what launches write
        uchar4* image = nullptr;
        size_t pixels = 0;
    } out;
    // ---- the whitted triangle path: the scene, and what outlives it (lights, tile-queue heads, miss colour)
    WhittedMesh wm;
    DeviceArray<whitted::PointLight> w_lights;
    int w_n_lights = 0;
    DeviceArray<unsigned int> w_tile_counters;   // two sets of tile-queue heads: a launch counts on one and zeroes the other
    int w_launch_parity = 0;
    v3 w_miss{0, 0, 0};
    std::string err;
};

static_assert(sizeof(rtgo_pbr) == sizeof(whitted::Pbr) && sizeof(rtgo_point_light) == sizeof(whitted::PointLight) && sizeof(rtgo_point_light) == 32,
              "whitted records");
static_assert(RTGO_MAX_TRIANGLES == whitted::kMaxTriangles, "limits");
static_assert(RTGO_WHITTED_MAX_MESHES == whitted::kMaxMeshes && RTGO_WHITTED_MAX_INSTANCES == whitted::kMaxInstances, "instance limits");
static_assert(RTGO_WHITTED_MAX_MESH_TRIANGLES == whitted::kBigMaxMeshTriangles && RTGO_WHITTED_MAX_SCENE_TRIANGLES == whitted::kBigMaxSceneTriangles,
              "clustered mesh limits");
static_assert(sizeof(rtgo_whitted_instance) == 56 && sizeof(whitted::InstWalk) == 64 && sizeof(whitted::InstShade) == 112, "instance records");
static_assert(sizeof(rtgo_whitted_mesh_update) == 32, "rtgo_whitted_update_meshes's entry");

static std::string g_create_error;

static int fail(rtgo_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

#define RTGO_HIP(ctx, call)                                                                                       \
    do {                                                                                                          \
        hipError_t e_ = (call);                                                                                   \
        if (e_ != hipSuccess)                                                                                     \
            return fail(ctx, RTGO_E_HIP_BASE + (int)e_,                                                           \
                        std::string(#call) + " failed: " + hipGetErrorString(e_) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
    } while (0)

// read back the oldest `count` pending event pairs (blocks until their stop events have completed)
static int harvest_events(rtgo_ctx* c, int count)
{
    while (count-- > 0 && c->ev_pending > 0) {
        const int slot = (c->ev_head - c->ev_pending + 2 * rtgo_ctx::kEvRing) % rtgo_ctx::kEvRing;
        RTGO_HIP(c, hipEventSynchronize(c->ev_stop[slot]));
        float ms = 0.0f;
        RTGO_HIP(c, hipEventElapsedTime(&ms, c->ev_start[slot], c->ev_stop[slot]));
        c->last_ms = ms;
        c->total_ms += ms;
        c->ev_pending--;
        if (c->ev_tag[slot] != 0) {
            float& best = c->trial.best[(c->ev_tag[slot] - 1) & 7];
            best = ms < best ? ms : best;
            c->trial.done++;
            c->ev_tag[slot] = 0;
        }
    }
    return RTGO_OK;
}

// One launch of either path between the two events of the ring's next slot on the context's stream (the oldest pair read back
// first when the ring is full), counted.  `launch` enqueues the kernel and returns an RTGO code; `slot`: the ring slot it took.
template <class Launch>
static int timed_launch(rtgo_ctx* c, int& slot, Launch&& launch)
{
    if (c->ev_pending == rtgo_ctx::kEvRing)
        if (const int rc = harvest_events(c, 1)) return rc;
    slot = c->ev_head;
    RTGO_HIP(c, hipEventRecord(c->ev_start[slot], c->stream));
    if (const int rc = launch()) return rc;
    RTGO_HIP(c, hipEventRecord(c->ev_stop[slot], c->stream));
    c->ev_head = (c->ev_head + 1) % rtgo_ctx::kEvRing;
    c->ev_pending++;
    c->launches++;
    return RTGO_OK;
}

// Environment knobs for tests and experiments (no result depends on them; DESIGN.md, "Knobs"): read afresh by every call that uses them
static float env_float(const char* name, float dflt)
{
    const char* v = std::getenv(name);
    return v ? (float)std::atof(v) : dflt;
}
static unsigned int env_uint(const char* name, unsigned int dflt)
{
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    const long k = std::strtol(v, nullptr, 10);
    return k > 0 ? (unsigned int)k : dflt;
}
// RTGO_WHITTED_MODE (test and experiment knob): 0 / 1 / 2 = at most that much of the whitted structure in LDS (kAllInL2 / kRecordsInLds /
// kAllInLds); unset, empty or negative: kAllInLds, above 2: 2.  (env_uint cannot carry it: 0 is a value here.)
static int env_whitted_mode()
{
    const char* v = std::getenv("RTGO_WHITTED_MODE");
    if (!v || !*v) return whitted::kAllInLds;
    const long k = std::strtol(v, nullptr, 10);
    return k < 0 ? whitted::kAllInLds : (int)std::min<long>(k, whitted::kAllInLds);
}
// RTGO_TRACE_MODE (test and experiment knob, RTGO_WHITTED_MODE's way): 0 = scene / top level read from global memory, 1 = staged in LDS
// (where it fits); unset, empty or anything else: the host's own choice (-1).  No result depends on it.
static int env_trace_mode()
{
    const char* v = std::getenv("RTGO_TRACE_MODE");
    if (!v || !*v) return -1;
    return v[0] == '0' ? 0 : (v[0] == '1' ? 1 : -1);
}

// Sorts n keys by their upper 32 bits: four stable passes (radix_count_kernel, radix_scan_kernel, radix_scatter_kernel) over those bytes,
// from `keys` to `keys_alt` and back.  hist: 256 words per tile of kRadixTile keys.  Returns the buffer that holds the sorted keys.
static const unsigned long long* radix_sort_keys(rtgo_ctx* c, unsigned long long* keys, unsigned long long* keys_alt, unsigned int* hist, int n)
{
    using namespace whitted;
    const int nb = (n + kRadixTile - 1) / kRadixTile;
    unsigned long long *src = keys, *dst = keys_alt;
    for (int shift = 32; shift < 64; shift += 8) {
        hipLaunchKernelGGL(radix_count_kernel, dim3(nb), dim3(kRadixThreads), 0, c->stream, (const unsigned long long*)src, n, shift, hist);
        hipLaunchKernelGGL(radix_scan_kernel, dim3(1), dim3(1024), 0, c->stream, hist, 256 * nb);
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(nb), dim3(kRadixThreads), 0, c->stream, (const unsigned long long*)src, n, shift, (const unsigned int*)hist, dst);
        std::swap(src, dst);
    }
    return src;
}

// The determinant of the 3x3 in the first three columns of a, expanded along its first row; with `inv`, also the inverse (adj(a) / det).
// One text for the host and for inst_prepare_kernel (rtgo_whitted_inst_update.h): both compiles round once per operation.
template <int S>
__host__ __device__ static double mat3_det_inverse(const double (&a)[3][S], double (*inv)[S] = nullptr)
{
    const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                       a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    for (int i = 0; inv && i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (j + 1) % 3, i2 = (j + 2) % 3, j1 = (i + 1) % 3, j2 = (i + 2) % 3;
            inv[i][j] = (a[i1][j1] * a[i2][j2] - a[i1][j2] * a[i2][j1]) / det;
        }
    return det;
}
