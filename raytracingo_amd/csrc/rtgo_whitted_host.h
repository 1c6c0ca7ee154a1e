// rtgo_whitted_host.h -- host side of the whitted (triangle) path: what the rtgo_whitted_* entry points of rtgo_capi.hip call once they
// have checked their arguments (no exported symbol lives here).  Scene set-up first, then the launches' parameter blocks.  Every build
// works on the WhittedMesh it is handed -- a scene built aside, or the context's -- and frees its temporaries on return.
#pragma once

#include "rtgo_ctx.h"
#include "rtgo_whitted_inst_update.h"
#include "rtgo_whitted_mesh_device.h"

using whitted::WhittedBuildMeta;

// the two sets of tile-queue heads of the whitted launches (allocated once, zero)
static int whitted_tile_heads(rtgo_ctx* c)
{
    if (!c->w_tile_counters.get()) {
        const size_t heads = 2 * (size_t)whitted::kTileHeads * whitted::kTileHeadStride;
        RTGO_HIP(c, c->w_tile_counters.alloc(heads));
        RTGO_HIP(c, hipMemsetAsync(c->w_tile_counters.get(), 0, heads * sizeof(unsigned int), c->stream));
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
    }
    return RTGO_OK;
}

// What one whitted_build of n triangles writes (recs n x 4 float4, tris n x 3 float4, qrecs n x 2 uint4, tidx n uint2), and the slice of a
// scene's arrays that starts at record `rec` and (sorted) triangle `tri`
struct WhittedBuildTarget { float4 *recs, *tris; uint4* qrecs; uint2* tidx; };
static WhittedBuildTarget whitted_target(const WhittedMesh& wm, size_t rec, size_t tri)
{
    return {wm.recs.get() + 4 * rec, wm.tris.get() + 3 * tri, wm.qrecs.get() + 2 * tri, wm.tidx.get() + tri};
}

// What a whitted_build of up to n triangles needs while it runs: the Morton hierarchy's nodes and the kernels' work arrays
struct WhittedBuildScratch {
    DeviceArray<float4> nodes;
    DeviceArray<int> ints;
    hipError_t alloc(size_t n)
    {
        const hipError_t e = nodes.alloc((2 * n - 1) * 2);
        return e != hipSuccess ? e : ints.alloc(whitted::build_scratch_ints(n));
    }
};

// The records over a build's leaves are rebuilt top-down with the surface-area heuristic when sah_kernel's LDS holds them (leaf boxes,
// links, order arrays: 33 B per triangle, so structures beyond ~4650 triangles keep the Morton records) and RTGO_WHITTED_NO_SAH is unset.
// RTGO_WHITTED_SEQ_BUILD (set): rtgo_whitted_set_scene builds its structures one after another (whitted_build) instead of by the batched
// launches (whitted_run_batch) -- the same arrays; for A/B timing and tests/test_whitted_rebuild_meshes.py.
static size_t whitted_sah_lds(int n) { return (size_t)n * (6 * sizeof(float) + sizeof(int) + 2 * sizeof(short) + 1) + 16; }
static bool whitted_sah_applies(int n) { return !std::getenv("RTGO_WHITTED_NO_SAH") && whitted_sah_lds(n) <= 150 * 1024; }
static bool whitted_sequential_builds() { return std::getenv("RTGO_WHITTED_SEQ_BUILD") != nullptr; }

// One structure of the whitted path, built on the device over n triangles (positions, indices: device memory) into `t`: build_kernel's
// Morton hierarchy, its records rebuilt top-down with the surface-area heuristic (sah_kernel) when the leaves fit its LDS, and the Morton
// records again when the surface-area tree comes out deeper than the walk's stack.  Synchronous.
static int whitted_build(rtgo_ctx* c, const float* positions, const unsigned int* indices, int n, const WhittedBuildTarget& t, const WhittedBuildScratch& s,
                         WhittedBuildMeta& m, const char* what)
{
    const whitted::BuildScratch w(s.ints.get(), n);
    const size_t keys_lds = (size_t)whitted::kMaxTriangles * sizeof(unsigned long long);
    hipLaunchKernelGGL(whitted::build_kernel, dim3(1), dim3(whitted::kBuildThreads), keys_lds, c->stream, positions, indices, n, s.nodes.get(),
                       w.parent, w.visit, w.first_of, w.count_of, w.rec_of, t.recs, t.tris, t.qrecs, t.tidx, w.meta);
    RTGO_HIP(c, hipGetLastError());
    const size_t sah_lds = whitted_sah_lds(n);
    const bool sah = whitted_sah_applies(n);
    if (sah) {
        hipLaunchKernelGGL(whitted::sah_kernel, dim3(1), dim3(whitted::kBuildThreads), sah_lds, c->stream, n, (const float4*)s.nodes.get(), (const int*)w.parent,
                           (const int*)w.first_of, (const int*)w.count_of, w.sah, t.recs, t.qrecs, w.meta);
        RTGO_HIP(c, hipGetLastError());
    }
    std::memset(&m, 0, sizeof m);
    RTGO_HIP(c, hipMemcpyAsync(&m, w.meta, sizeof m, hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    if (m.walk_depth > whitted::kMaxWalkDepth && sah) {
        // the surface-area tree came out deeper than the walk's stack (it has no depth bound of its own): back to the Morton records,
        // whose depth is bounded by the code length
        hipLaunchKernelGGL(whitted::build_kernel, dim3(1), dim3(whitted::kBuildThreads), keys_lds, c->stream, positions, indices, n, s.nodes.get(),
                           w.parent, w.visit, w.first_of, w.count_of, w.rec_of, t.recs, t.tris, t.qrecs, t.tidx, w.meta);
        RTGO_HIP(c, hipGetLastError());
        RTGO_HIP(c, hipMemcpyAsync(&m, w.meta, sizeof m, hipMemcpyDeviceToHost, c->stream));
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (m.depth > 2 * whitted::kStack)
        return fail(c, RTGO_E_UNSUPPORTED, std::string(what) + ": triangle LBVH depth " + std::to_string(m.depth) + " exceeds what the build handles (" +
                                               std::to_string(2 * whitted::kStack) + ")");
    if (m.walk_depth > whitted::kMaxWalkDepth)
        return fail(c, RTGO_E_UNSUPPORTED, std::string(what) + ": the walk needs " + std::to_string(m.walk_depth) + " stack entries (limit " +
                                               std::to_string(whitted::kMaxWalkDepth) + ")");
    return RTGO_OK;
}

// One structure over n boxes (d_boxes: lo xyz, hi xyz each, device memory): the top level over the instances' boxes, a mid level over the
// clusters'.  whitted_build takes box k as the degenerate triangle (lo, hi, lo) of "vertices" 2k and 2k + 1, whose bounds are the box; its
// Morton-ordered "triangles" carry k in .w of their first corner: the leaf order returned.  Records to recs (n x 4 float4).  Synchronous.
static int whitted_build_boxes(rtgo_ctx* c, const float* d_boxes, int n, float4* recs, std::vector<int>& order, WhittedBuildMeta& m, const char* what)
{
    std::vector<unsigned int> idx((size_t)3 * n);
    for (int k = 0; k < 3 * n; ++k) idx[k] = 2 * (k / 3) + (k % 3 == 1 ? 1 : 0);
    DeviceArray<unsigned int> d_idx;
    DeviceArray<float4> d_tris;   // (what the build writes beside the records: only the order is read)
    DeviceArray<uint4> d_qrecs;
    DeviceArray<uint2> d_tidx;
    WhittedBuildScratch scratch;
    RTGO_HIP(c, d_idx.upload(idx.data(), idx.size(), c->stream));
    RTGO_HIP(c, d_tris.alloc((size_t)n * 3));
    RTGO_HIP(c, d_qrecs.alloc((size_t)n * 2));
    RTGO_HIP(c, d_tidx.alloc(n));
    RTGO_HIP(c, scratch.alloc(n));
    if (const int rc = whitted_build(c, d_boxes, d_idx.get(), n, {recs, d_tris.get(), d_qrecs.get(), d_tidx.get()}, scratch, m, what)) return rc;
    std::vector<float4> tris((size_t)3 * n);
    RTGO_HIP(c, hipMemcpyAsync(tris.data(), d_tris.get(), tris.size() * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    order.resize(n);
    for (int pos = 0; pos < n; ++pos) std::memcpy(&order[pos], &tris[3 * pos].w, sizeof(int));
    return RTGO_OK;
}

// The checks every mesh of the whitted path passes (rtgo_whitted_set_mesh, rtgo_whitted_set_scene; `at` names it in the messages): vertex
// indices inside the vertex array, finite vertex data, material indices inside the table.  Also finds the mesh's largest material index.
// (kMeshFault: its refusals, in its order -- the kinds mesh_check_kernel reports of a mesh on the device)
static const char* const kMeshFault[whitted::kMeshFaultKinds] = {": index beyond the vertex array", ": non-finite vertex data", ": non-finite texture coordinate",
                                                                 ": material index beyond the material array"};
static int whitted_check_mesh(rtgo_ctx* c, const rtgo_whitted_mesh& q, uint32_t n_materials, const std::string& at, uint32_t& max_material)
{
    using namespace whitted;
    for (uint32_t i = 0; i < 3 * q.n_triangles; ++i)
        if (q.indices[i] >= q.n_vertices) return fail(c, RTGO_E_INVALID, at + kMeshFault[kMeshBadIndex]);
    for (uint32_t i = 0; i < 3 * q.n_vertices; ++i)
        if (!std::isfinite(q.positions[i]) || (q.normals && !std::isfinite(q.normals[i]))) return fail(c, RTGO_E_INVALID, at + kMeshFault[kMeshBadVertex]);
    if (q.texcoords)
        for (uint32_t i = 0; i < 2 * q.n_vertices; ++i)
            if (!std::isfinite(q.texcoords[i])) return fail(c, RTGO_E_INVALID, at + kMeshFault[kMeshBadTexcoord]);
    max_material = 0;
    if (q.material_of_triangle)
        for (uint32_t i = 0; i < q.n_triangles; ++i) {
            if (q.material_of_triangle[i] >= n_materials) return fail(c, RTGO_E_INVALID, at + kMeshFault[kMeshBadMaterial]);
            max_material = std::max(max_material, q.material_of_triangle[i]);
        }
    return RTGO_OK;
}

// The one mesh of rtgo_whitted_set_mesh into `wm` (empty): uploads, the build, and what the launches read of its meta.  kind: where q's
// arrays lie (rtgo_whitted_set_mesh_device: the device, and they move device to device)
static int whitted_build_single(rtgo_ctx* c, WhittedMesh& wm, const rtgo_whitted_mesh& q, const rtgo_pbr* materials, uint32_t n_materials, const char* what,
                                hipMemcpyKind kind = hipMemcpyHostToDevice)
{
    const size_t n = q.n_triangles;
    WhittedBuildScratch scratch;
    auto put = [&](auto& keep, const auto* src, size_t count) -> hipError_t {
        const hipError_t e = keep.alloc(count);
        return e != hipSuccess ? e : hipMemcpyAsync(keep.get(), src, count * sizeof *src, kind, c->stream);
    };
    RTGO_HIP(c, put(wm.positions, q.positions, (size_t)q.n_vertices * 3));
    if (q.normals) RTGO_HIP(c, put(wm.normals, q.normals, (size_t)q.n_vertices * 3));
    RTGO_HIP(c, put(wm.indices, q.indices, n * 3));
    if (q.material_of_triangle) RTGO_HIP(c, put(wm.tri_material, q.material_of_triangle, n));
    RTGO_HIP(c, wm.materials.upload((const whitted::Pbr*)materials, n_materials, c->stream));
    RTGO_HIP(c, wm.recs.alloc(n * 4));
    RTGO_HIP(c, wm.tris.alloc(n * 3));
    RTGO_HIP(c, wm.qrecs.alloc(n * 2));
    RTGO_HIP(c, wm.tidx.alloc(n));
    RTGO_HIP(c, scratch.alloc(n));
    if (const int rc = whitted_build(c, wm.positions.get(), wm.indices.get(), (int)n, whitted_target(wm, 0, 0), scratch, wm.meta, what)) return rc;
    wm.n_vertices = (int)q.n_vertices;
    wm.walk_depth = wm.meta.walk_depth < 1 ? 1 : wm.meta.walk_depth;
    wm.n_materials = (int)n_materials;
    return RTGO_OK;
}

// ---- instanced scenes ----------------------------------------------------------------------------------------------------
// The instances' side, checked and laid out on the host before anything on the device changes: per instance its InstShade record
// (o2w as given, W2O = its inverse in double, rounded once) and its world box (the 8 corners of its mesh's box through o2w in double,
// rounded outwards), which the top-level build takes as the degenerate triangle (lo, hi, lo).
static int whitted_prepare_instances(rtgo_ctx* c, const std::vector<WhittedMeshInfo>& meshes, uint32_t n_materials, const rtgo_whitted_instance* inst,
                                     uint32_t n, std::vector<whitted::InstShade>& shade, std::vector<float>& box_pos, const char* what)
{
    const std::string w(what);
    if (!inst) return fail(c, RTGO_E_INVALID, w + ": NULL instance array");
    if (n == 0 || n > RTGO_WHITTED_MAX_INSTANCES)
        return fail(c, RTGO_E_UNSUPPORTED, w + ": instance count must be in [1, " + std::to_string(RTGO_WHITTED_MAX_INSTANCES) + "]");
    shade.assign(n, whitted::InstShade{});
    box_pos.assign((size_t)6 * n, 0.0f);
    for (uint32_t i = 0; i < n; ++i) {
        const rtgo_whitted_instance& q = inst[i];
        const std::string at = w + ": instance " + std::to_string(i);
        if (q.mesh >= meshes.size()) return fail(c, RTGO_E_INVALID, at + " names a mesh beyond the meshes array");
        const WhittedMeshInfo& mi = meshes[q.mesh];
        if ((uint64_t)q.material_offset + mi.max_material >= n_materials) return fail(c, RTGO_E_INVALID, at + ": material offset + material index beyond the material array");
        bool finite = true;
        for (int k = 0; k < 12; ++k) finite = finite && std::isfinite(q.transform[k]);
        // the walk takes rays to object space through the inverse: the transform must be finite and invertible (the analytic path's
        // test of a model matrix, rtgo_set_scene)
        double A[3][4], B[3][4];   // B: the inverse, adj(A) / det, then -A^-1 t
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 4; ++k) A[r][k] = q.transform[4 * r + k];
        const double det = mat3_det_inverse(A, B);
        if (!finite || !std::isfinite(det) || std::fabs(det) < 1e-30) return fail(c, RTGO_E_INVALID, at + " has a non-finite or singular transform");
        for (int r = 0; r < 3; ++r) B[r][3] = -(B[r][0] * A[0][3] + B[r][1] * A[1][3] + B[r][2] * A[2][3]);
        whitted::InstShade& sh = shade[i];
        float* o2w = &sh.o2w[0].x;
        float* w2o = &sh.w2o[0].x;
        for (int k = 0; k < 12; ++k) {
            o2w[k] = q.transform[k];
            w2o[k] = (float)B[k / 4][k % 4];
            if (!std::isfinite(w2o[k])) return fail(c, RTGO_E_INVALID, at + " has a non-finite or singular transform");
        }
        sh.material_offset = (int)q.material_offset;
        sh.vert_base = mi.vert_base;
        sh.tri_base = mi.tri_base;
        sh.flags = mi.flags;
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int corner = 0; corner < 8; ++corner) {
            const double x = (corner & 1) ? mi.hi[0] : mi.lo[0], y = (corner & 2) ? mi.hi[1] : mi.lo[1], z = (corner & 4) ? mi.hi[2] : mi.lo[2];
            for (int r = 0; r < 3; ++r) {
                const double v = A[r][0] * x + A[r][1] * y + A[r][2] * z + A[r][3];
                lo[r] = std::fmin(lo[r], v);
                hi[r] = std::fmax(hi[r], v);
            }
        }
        for (int r = 0; r < 3; ++r) {
            float l = (float)lo[r], h = (float)hi[r];
            if ((double)l > lo[r]) l = std::nextafter(l, -INFINITY);
            if ((double)h < hi[r]) h = std::nextafter(h, INFINITY);
            if (!std::isfinite(l) || !std::isfinite(h)) return fail(c, RTGO_E_INVALID, at + " places its mesh beyond the float range");
            box_pos[6 * i + r] = l;
            box_pos[6 * i + 3 + r] = h;
        }
    }
    return RTGO_OK;
}

// The top level of `wm` (its meshes built) over prepared instances, into `top`: the structure over the instance boxes, the InstWalk records
// in leaf order, and the stack both levels need (depth).  Nothing of wm changes.  whitted_make_top_over: the same over meshes that are not
// wm's yet (rtgo_whitted_rebuild_meshes: a rebuilt mesh's root link and depth can differ).
static int whitted_make_top_over(rtgo_ctx* c, const std::vector<WhittedMeshInfo>& meshes, int mesh_depth, const std::vector<whitted::InstShade>& shade,
                                 const std::vector<float>& box_pos, const rtgo_whitted_instance* inst, const char* what, WhittedTop& top, int& depth)
{
    const int n = (int)shade.size();
    DeviceArray<float> d_boxes;
    std::vector<int> order;
    RTGO_HIP(c, d_boxes.upload(box_pos.data(), box_pos.size(), c->stream));
    RTGO_HIP(c, top.recs.alloc((size_t)n * 4));
    if (const int rc = whitted_build_boxes(c, d_boxes.get(), n, top.recs.get(), order, top.meta, what)) return rc;
    depth = (top.meta.n_recs > 0 ? top.meta.walk_depth : 0) + mesh_depth;
    if (depth > whitted::kMaxInstWalkDepth)
        return fail(c, RTGO_E_UNSUPPORTED, std::string(what) + ": the two-level walk needs " + std::to_string(depth) + " stack entries (limit " +
                                               std::to_string(whitted::kMaxInstWalkDepth) + ")");
    std::vector<whitted::InstWalk> walk((size_t)n);
    for (int pos = 0; pos < n; ++pos) {
        const int i = order[pos];
        const WhittedMeshInfo& mi = meshes[inst[i].mesh];
        walk[pos] = whitted::InstWalk{{shade[i].w2o[0], shade[i].w2o[1], shade[i].w2o[2]}, mi.rec_base, mi.tri_base, mi.root, i};
    }
    RTGO_HIP(c, top.inst.upload(walk.data(), walk.size(), c->stream));
    RTGO_HIP(c, top.shade.upload(shade.data(), shade.size(), c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    top.n_recs = top.meta.n_recs;
    top.n_instances = n;
    return RTGO_OK;
}

static int whitted_make_top(rtgo_ctx* c, const WhittedMesh& wm, const std::vector<whitted::InstShade>& shade, const std::vector<float>& box_pos,
                            const rtgo_whitted_instance* inst, const char* what, WhittedTop& top, int& depth)
{
    return whitted_make_top_over(c, wm.meshes, wm.mesh_depth, shade, box_pos, inst, what, top, depth);
}

// What rtgo_whitted_refit_instances_device_async leaves for later: wm.instances and wm.top.meta's grid as the device holds them.  Every
// synchronous reader or writer of either calls this first.  It waits for the stream, then adopts what the applied updates since the last
// refresh wrote: if their count has not moved, every update in between was refused, the host's fields are current as they stand, and the
// kept instances and the meta block (which nothing may have filled yet) are not read.
static int whitted_refresh_host(rtgo_ctx* c)
{
    WhittedMesh& wm = c->wm;
    WhittedInstStaging& st = wm.staging;
    if (!st.stale) return RTGO_OK;
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    unsigned int w[WhittedInstStaging::kWords];
    RTGO_HIP(c, hipMemcpyAsync(w, st.words.get(), sizeof w, hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    st.stale = false;
    const unsigned int applied = w[WhittedInstStaging::kMetaWords];
    if (applied == st.adopted) return RTGO_OK;
    std::vector<rtgo_whitted_instance> instances((size_t)wm.top.n_instances);
    RTGO_HIP(c, hipMemcpyAsync(instances.data(), st.kept.get(), instances.size() * sizeof(rtgo_whitted_instance), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    wm.instances = std::move(instances);
    if (wm.top.n_recs > 0) {   // (a top level of one leaf has no refit: its grid stays, as under the synchronous call)
        whitted::WhittedBuildMeta m;
        std::memcpy(&m, w, sizeof m);
        wm.top.meta.grid_lo = m.grid_lo;
        wm.top.meta.grid_step = m.grid_step;
    }
    st.adopted = applied;
    return RTGO_OK;
}

// ... and that top level in wm's place (the refit staging went with the old one's size; the stream has drained)
static void whitted_install_top(WhittedMesh& wm, WhittedTop&& top, int depth)
{
    wm.staging = WhittedInstStaging();
    wm.top = std::move(top);
    wm.walk_depth = depth < 1 ? 1 : depth;
}

// Both, for instances the caller hands in: built aside, wm's top level replaced only once all of it succeeded; wm keeps a copy of the
// instances (rtgo_whitted_update_mesh lays them out again over a mesh's new box)
static int whitted_build_top(rtgo_ctx* c, WhittedMesh& wm, const std::vector<whitted::InstShade>& shade, const std::vector<float>& box_pos,
                             const rtgo_whitted_instance* inst, const char* what)
{
    WhittedTop top;
    int depth = 0;
    if (const int rc = whitted_make_top(c, wm, shade, box_pos, inst, what, top, depth)) return rc;
    wm.instances.assign(inst, inst + shade.size());
    whitted_install_top(wm, std::move(top), depth);
    return RTGO_OK;
}

// Device scratch of one clustered mesh's build, alive from its sort to its mid level (28 B per triangle: the sorted keys and the
// gathered index triples are what its clusters' builds and big_remap_kernel read)
struct WhittedBigScratch {
    DeviceArray<unsigned long long> keys, keys_alt;
    DeviceArray<unsigned int> hist, cidx;
    DeviceArray<float> partial, bounds, boxes;
    DeviceArray<int> crec;
    const unsigned long long* sorted = nullptr;   // keys or keys_alt, whichever the last radix pass wrote
};

// What the builds of a clustered mesh's clusters reported: where each cluster's records start, its root link, the deepest cluster walk
struct WhittedClusterBuilds {
    std::vector<int> crec, croot;
    int cdepth = 0;
    void add(int rec, int nc, const WhittedBuildMeta& m)
    {
        crec.push_back(rec);
        croot.push_back(m.n_recs > 0 ? 0 : -1 - ((nc - 1) << whitted::kLeafShift));   // (nc >= kClusterTris / 2: always records)
        cdepth = std::max(cdepth, m.n_recs > 0 ? m.walk_depth : 0);
    }
};

// ---- batched builds -------------------------------------------------------------------------------------------------------------------
// The structures of one call (rtgo_whitted_set_scene: every mesh; rtgo_whitted_rebuild_meshes: the named ones) as one table: all
// clusters of its clustered meshes and its small meshes, built by whitted_run_batch; then what each build reported, entry for entry
struct WhittedBatch {
    std::vector<whitted::BuildEntry> entries;
    std::vector<WhittedBuildMeta> metas;
    std::vector<int> rec0;   // where each entry's records start in the scene's arrays
    int max_n = 0;
    // rec_start >= 0: the first structure of its mesh, its records start there; < 0: they follow the entry before
    void add(const float* positions, const unsigned int* indices, int n, const WhittedBuildTarget& t, int rec_start)
    {
        entries.push_back({positions, indices, t.tris, t.qrecs, t.tidx, n, whitted_sah_applies(n) ? 1 : 0, rec_start, 0});
        max_n = std::max(max_n, n);
    }
};

// whitted_build over every entry of the table, in rounds of at most kBatchRound structures (one workgroup each): the Morton builds, the
// surface-area passes, the Morton builds again where that tree came out too deep, the records' places, the records packed into
// `recs` (the scene's) -- five launches a round, whatever the table holds, and one wait at the end.  Scratch: 280 B per triangle of a
// round (nodes, work arrays, record staging) = min(entries, kBatchRound) x the largest entry, at most 587 MB (256 x 8192 triangles).
static int whitted_run_batch(rtgo_ctx* c, WhittedBatch& b, float4* recs, const char* what)
{
    using namespace whitted;
    const int ne = (int)b.entries.size();
    if (ne == 0) return RTGO_OK;
    const int round = std::min(ne, kBatchRound);
    const size_t max_n = (size_t)b.max_n;
    DeviceArray<BuildEntry> d_table;
    DeviceArray<WhittedBuildMeta> d_metas;
    DeviceArray<int> d_rec0;   // [ne], then big_batch_offsets_kernel's carry
    DeviceArray<float4> d_nodes, d_stage;
    DeviceArray<int> d_ints;
    RTGO_HIP(c, d_table.upload(b.entries.data(), b.entries.size(), c->stream));
    RTGO_HIP(c, d_metas.alloc(ne));
    RTGO_HIP(c, d_rec0.alloc((size_t)ne + 1));
    RTGO_HIP(c, d_nodes.alloc((size_t)round * 2 * (2 * max_n - 1)));
    RTGO_HIP(c, d_ints.alloc((size_t)round * build_scratch_ints(max_n)));
    RTGO_HIP(c, d_stage.alloc((size_t)round * 4 * max_n));
    RTGO_HIP(c, hipMemsetAsync(d_rec0.get() + ne, 0, sizeof(int), c->stream));
    const BatchSlots slots = {d_nodes.get(), d_ints.get(), d_stage.get(), b.max_n};
    const size_t keys_lds = (size_t)kMaxTriangles * sizeof(unsigned long long);
    for (int first = 0; first < ne; first += round) {
        const int count = std::min(round, ne - first);
        size_t sah_lds = 0;   // of the round's largest entry that takes the pass
        for (int k = first; k < first + count; ++k)
            if (b.entries[k].sah) sah_lds = std::max(sah_lds, whitted_sah_lds(b.entries[k].n));
        hipLaunchKernelGGL(big_build_batch_kernel, dim3(count), dim3(kBuildThreads), keys_lds, c->stream, (const BuildEntry*)d_table.get(), first, slots,
                           d_metas.get(), 0);
        if (sah_lds > 0) {
            hipLaunchKernelGGL(big_sah_batch_kernel, dim3(count), dim3(kBuildThreads), sah_lds, c->stream, (const BuildEntry*)d_table.get(), first, slots,
                               d_metas.get());
            hipLaunchKernelGGL(big_build_batch_kernel, dim3(count), dim3(kBuildThreads), keys_lds, c->stream, (const BuildEntry*)d_table.get(), first, slots,
                               d_metas.get(), 1);
        }
        hipLaunchKernelGGL(big_batch_offsets_kernel, dim3(1), dim3(kBatchRound), 0, c->stream, (const BuildEntry*)d_table.get(), first, count,
                           (const WhittedBuildMeta*)d_metas.get(), d_rec0.get(), d_rec0.get() + ne);
        hipLaunchKernelGGL(big_pack_records_kernel, dim3(count), dim3(256), 0, c->stream, first, slots, (const WhittedBuildMeta*)d_metas.get(),
                           (const int*)d_rec0.get(), recs);
        RTGO_HIP(c, hipGetLastError());
    }
    b.metas.assign(ne, WhittedBuildMeta{});
    b.rec0.assign(ne, 0);
    RTGO_HIP(c, hipMemcpyAsync(b.metas.data(), d_metas.get(), ne * sizeof(WhittedBuildMeta), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipMemcpyAsync(b.rec0.data(), d_rec0.get(), ne * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    for (const WhittedBuildMeta& m : b.metas) {   // (whitted_build's refusals)
        if (m.depth > 2 * kStack)
            return fail(c, RTGO_E_UNSUPPORTED, std::string(what) + ": triangle LBVH depth " + std::to_string(m.depth) + " exceeds what the build handles (" +
                                                   std::to_string(2 * kStack) + ")");
        if (m.walk_depth > kMaxWalkDepth)
            return fail(c, RTGO_E_UNSUPPORTED, std::string(what) + ": the walk needs " + std::to_string(m.walk_depth) + " stack entries (limit " +
                                                   std::to_string(kMaxWalkDepth) + ")");
    }
    return RTGO_OK;
}

// One clustered mesh (n > kMaxTriangles triangles; rtgo_whitted_big.h), in its slices of wm's arrays: Morton order over the
// whole mesh on the device, clusters of consecutive sorted triangles each built by whitted_build (tris[].w then remapped to the mesh's
// own indices), and a mid level over the clusters' boxes whose records take the first ncl - 1 record slots of the mesh (the clusters
// follow: a mesh of n triangles has at most n slots, and a cluster of m triangles fewer than m records).  Appends the mesh's clusters,
// in the mid level's leaf order, to `table`; sets mi.root, mi.depth, and widens mi.lo / hi over every box the walk can reach from the
// mesh's root, so the instance boxes built from it contain them by construction.  Three steps: the sort (whitted_sort_clustered,
// enqueued), the clusters' builds (whitted_add_clusters + whitted_run_batch with the call's other structures, or
// whitted_build_clusters_sequential), the rest (whitted_finish_clustered, synchronous).
static int whitted_sort_clustered(rtgo_ctx* c, const WhittedMesh& wm, const WhittedMeshInfo& mi, WhittedBigScratch& bs)
{
    using namespace whitted;
    const int n = mi.n_tris, ncl = (n + kClusterTris - 1) / kClusterTris, nb = (n + kRadixTile - 1) / kRadixTile;
    const float* positions = wm.positions.get() + 3 * (size_t)mi.vert_base;
    const unsigned int* indices = wm.indices.get() + 3 * (size_t)mi.tri_base;
    RTGO_HIP(c, bs.keys.alloc(n));
    RTGO_HIP(c, bs.keys_alt.alloc(n));
    RTGO_HIP(c, bs.hist.alloc((size_t)256 * nb));
    RTGO_HIP(c, bs.cidx.alloc((size_t)3 * n));
    RTGO_HIP(c, bs.partial.alloc((size_t)6 * 1024));
    RTGO_HIP(c, bs.bounds.alloc(6));
    RTGO_HIP(c, bs.crec.alloc(ncl));
    RTGO_HIP(c, bs.boxes.alloc((size_t)6 * ncl));
    // Morton keys over the mesh's bounds, sorted by four stable passes over the code's bytes
    const int nbb = std::min(1024, (n + 1023) / 1024);
    hipLaunchKernelGGL(big_bounds_kernel, dim3(nbb), dim3(1024), 0, c->stream, positions, indices, n, bs.partial.get());
    hipLaunchKernelGGL(big_bounds_final_kernel, dim3(1), dim3(1024), 0, c->stream, (const float*)bs.partial.get(), nbb, bs.bounds.get());
    hipLaunchKernelGGL(big_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, positions, indices, n, (const float*)bs.bounds.get(), bs.keys.get());
    bs.sorted = radix_sort_keys(c, bs.keys.get(), bs.keys_alt.get(), bs.hist.get(), n);
    hipLaunchKernelGGL(big_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, bs.sorted, n, indices, bs.cidx.get());
    RTGO_HIP(c, hipGetLastError());
    return RTGO_OK;
}

// the clusters of a sorted mesh as entries of a call's table ...
static void whitted_add_clusters(const WhittedMesh& wm, const WhittedMeshInfo& mi, const WhittedBigScratch& bs, WhittedBatch& batch)
{
    using namespace whitted;
    const int n = mi.n_tris, ncl = (n + kClusterTris - 1) / kClusterTris;
    for (int k = 0; k < ncl; ++k) {
        const int s = cluster_start(n, ncl, k), nc = cluster_start(n, ncl, k + 1) - s;
        batch.add(wm.positions.get() + 3 * (size_t)mi.vert_base, bs.cidx.get() + 3 * (size_t)s, nc, whitted_target(wm, 0, mi.tri_base + s),
                  k == 0 ? mi.rec_base + ncl - 1 : -1);
    }
}

// ... and what the table's entries first .. first + ncl - 1 report of them
static void whitted_take_clusters(WhittedMeshInfo& mi, const WhittedBatch& batch, int first, WhittedClusterBuilds& cb)
{
    using namespace whitted;
    const int n = mi.n_tris, ncl = (n + kClusterTris - 1) / kClusterTris;
    for (int k = 0; k < ncl; ++k) {
        const int s = cluster_start(n, ncl, k), nc = cluster_start(n, ncl, k + 1) - s;
        const WhittedBuildMeta& m = batch.metas[first + k];
        mi.built.push_back({batch.rec0[first + k], m.n_recs, mi.tri_base + s, m});
        cb.add(batch.rec0[first + k], nc, m);
    }
}

// The clusters one after another, a host wait after each (RTGO_WHITTED_SEQ_BUILD)
static int whitted_build_clusters_sequential(rtgo_ctx* c, const WhittedMesh& wm, WhittedMeshInfo& mi, const WhittedBigScratch& bs, const WhittedBuildScratch& scratch,
                                             WhittedClusterBuilds& cb, const char* what)
{
    using namespace whitted;
    const int n = mi.n_tris, ncl = (n + kClusterTris - 1) / kClusterTris;
    const float* positions = wm.positions.get() + 3 * (size_t)mi.vert_base;
    int rec = mi.rec_base + ncl - 1;
    for (int k = 0; k < ncl; ++k) {
        const int s = cluster_start(n, ncl, k), nc = cluster_start(n, ncl, k + 1) - s;
        WhittedBuildMeta m;
        if (const int rc = whitted_build(c, positions, bs.cidx.get() + 3 * (size_t)s, nc, whitted_target(wm, rec, mi.tri_base + s), scratch, m, what)) return rc;
        mi.built.push_back({rec, m.n_recs, mi.tri_base + s, m});
        cb.add(rec, nc, m);
        rec += m.n_recs;
    }
    return RTGO_OK;
}

// The clusters built: the mesh's own triangle numbers, the mid level, the mesh's clusters at table[tbase ..], root, depth and box
static int whitted_finish_clustered(rtgo_ctx* c, const WhittedMesh& wm, WhittedMeshInfo& mi, WhittedBigScratch& bs, const WhittedClusterBuilds& cb,
                                    std::vector<int4>& table, int tbase, const char* what)
{
    using namespace whitted;
    const int n = mi.n_tris, ncl = (n + kClusterTris - 1) / kClusterTris;
    const WhittedBuildTarget mesh = whitted_target(wm, mi.rec_base, mi.tri_base);
    const unsigned long long* sorted = bs.sorted;
    const std::vector<int>&crec = cb.crec, &croot = cb.croot;
    const int cdepth = cb.cdepth;
    hipLaunchKernelGGL(big_remap_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, mesh.tris, sorted, n, ncl);
    RTGO_HIP(c, hipGetLastError());
    // the mid level over the clusters' boxes
    RTGO_HIP(c, hipMemcpyAsync(bs.crec.get(), crec.data(), ncl * sizeof(int), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(big_cluster_boxes_kernel, dim3((ncl + 255) / 256), dim3(256), 0, c->stream, (const float4*)wm.recs.get(), (const int*)bs.crec.get(), ncl,
                       bs.boxes.get());
    RTGO_HIP(c, hipGetLastError());
    WhittedBuildMeta m;
    std::vector<int> order;
    if (const int rc = whitted_build_boxes(c, bs.boxes.get(), ncl, mesh.recs, order, m, what)) return rc;
    mi.built.push_back({mi.rec_base, m.n_recs, -1, m});
    mi.mid_order = order;
    std::vector<float4> root_rec(4);
    std::vector<float> boxes((size_t)6 * ncl);
    RTGO_HIP(c, hipMemcpyAsync(boxes.data(), bs.boxes.get(), boxes.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (m.n_recs > 0) RTGO_HIP(c, hipMemcpyAsync(root_rec.data(), mesh.recs, 4 * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    if (table.size() < (size_t)tbase + ncl) table.resize((size_t)tbase + ncl);
    for (int pos = 0; pos < ncl; ++pos) {
        const int k = order[pos];
        table[(size_t)tbase + pos] = make_int4(crec[k], mi.tri_base + cluster_start(n, ncl, k), croot[k], 0);
    }
    // what the walk can reach first below an instance: the mid root's two child boxes, or (a mid level of one leaf) the clusters' root
    // records, whose boxes are the ones big_cluster_boxes_kernel took
    auto widen = [&](const float* l, const float* h) {
        for (int a = 0; a < 3; ++a) {
            mi.lo[a] = std::fmin(mi.lo[a], l[a]);
            mi.hi[a] = std::fmax(mi.hi[a], h[a]);
        }
    };
    if (m.n_recs > 0) {
        widen(&root_rec[0].x, &root_rec[1].x);
        widen(&root_rec[2].x, &root_rec[3].x);
    }
    for (int k = 0; k < ncl; ++k) widen(&boxes[6 * k], &boxes[6 * k + 3]);
    mi.root = 1 + ((tbase << 3) | (m.n_recs > 0 ? kMidHasRecords : ncl - 1));
    mi.depth = (m.n_recs > 0 ? m.walk_depth : 0) + cdepth;
    return RTGO_OK;
}

// where the meshes of an instanced scene sit in its arrays, and the sizes its builds need
struct WhittedLayout {
    std::vector<WhittedMeshInfo> info;
    size_t n_vert = 0, n_tri = 0;
    int max_tri = 0, max_big = 0;   // the largest single build, the largest clustered mesh
    // the meshes back to back (indices stay relative to their mesh's vertices: each build reads its own slice)
    std::vector<float> pos, nrm, uv;
    std::vector<unsigned int> idx, tmat;
    // ... or (rtgo_whitted_set_scene_device) the vectors stay empty and the meshes lie on the device: the table mesh_pack_kernel packs them from
    std::vector<whitted::MeshSource> source;
    int source_blocks = 0;
    bool on_device() const { return !source.empty(); }
};

// The box an instanced mesh's instances are laid out from (WhittedMeshInfo::lo / hi), from the bounds of the vertices its triangles name:
// the root record's boxes lie within those bounds padded by build_kernel's pad, twice that pad covers them and their rounding
static void whitted_pad_mesh_box(const float lo[3], const float hi[3], float out_lo[3], float out_hi[3])
{
    float maxext = 0.0f, reach = 0.0f;
    for (int a = 0; a < 3; ++a) {
        maxext = std::fmax(maxext, hi[a] - lo[a]);
        reach = std::fmax(reach, std::fmax(std::fabs(lo[a]), std::fabs(hi[a])));
    }
    const float pad = 2.0f * whitted::box_pad(maxext, reach);
    for (int a = 0; a < 3; ++a) {
        out_lo[a] = lo[a] - pad;
        out_hi[a] = hi[a] + pad;
    }
}

// ... with the bounds taken on the host
static void whitted_mesh_box(const float* positions, const uint32_t* indices, uint32_t n_triangles, float out_lo[3], float out_hi[3])
{
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = 0; i < 3 * n_triangles; ++i)
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::fmin(lo[a], positions[3 * indices[i] + a]);
            hi[a] = std::fmax(hi[a], positions[3 * indices[i] + a]);
        }
    whitted_pad_mesh_box(lo, hi, out_lo, out_hi);
}

// What the host decides of mesh q of a scene from its pointers and counts alone (`at` names it in the messages; on_device: its arrays
// are device memory, rtgo_whitted_set_scene_device -- a NULL or misaligned pointer never reaches a launch), lay.n_tri triangles before it
static int whitted_admit_mesh(rtgo_ctx* c, const rtgo_whitted_mesh& q, const std::string& at, const WhittedLayout& lay, bool on_device)
{
    if (!q.positions || !q.indices) return fail(c, RTGO_E_INVALID, at + ": NULL positions or indices");
    if (on_device && !(aligned4(q.positions) && aligned4(q.normals) && aligned4(q.texcoords) && aligned4(q.indices) && aligned4(q.material_of_triangle)))
        return fail(c, RTGO_E_INVALID, at + ": a pointer is not 4-byte aligned");
    if (q.n_triangles == 0 || q.n_triangles > RTGO_WHITTED_MAX_MESH_TRIANGLES || q.n_vertices == 0)
        return fail(c, RTGO_E_UNSUPPORTED, at + ": triangle count must be in [1, " + std::to_string(RTGO_WHITTED_MAX_MESH_TRIANGLES) + "], vertices non-empty");
    if (lay.n_tri + q.n_triangles > RTGO_WHITTED_MAX_SCENE_TRIANGLES)
        return fail(c, RTGO_E_UNSUPPORTED, at + ": the meshes hold more than " + std::to_string(RTGO_WHITTED_MAX_SCENE_TRIANGLES) + " triangles together");
    return RTGO_OK;
}

// ... and, once it has passed its checks, where it will sit in the arrays (mi: box and max_material are set already)
static void whitted_place_mesh(const rtgo_whitted_mesh& q, WhittedLayout& lay, WhittedMeshInfo& mi)
{
    mi.rec_base = (int)lay.n_tri;   // (a mesh of n triangles has fewer than n records)
    mi.tri_base = (int)lay.n_tri;
    mi.vert_base = (int)lay.n_vert;
    mi.flags = (q.normals ? whitted::kHasNormals : 0) | (q.texcoords ? whitted::kHasTexcoords : 0);
    mi.clustered = q.n_triangles > (uint32_t)whitted::kMaxTriangles;
    mi.n_tris = (int)q.n_triangles;
    mi.n_verts = (int)q.n_vertices;
    lay.n_vert += q.n_vertices;
    lay.n_tri += q.n_triangles;
    if (mi.clustered) {
        // one workgroup's builds: clusters of at most kClusterTris triangles and a mid level of ncl boxes
        const int ncl = ((int)q.n_triangles + whitted::kClusterTris - 1) / whitted::kClusterTris;
        lay.max_tri = std::max(lay.max_tri, std::max(whitted::kClusterTris, ncl));
        lay.max_big = std::max(lay.max_big, (int)q.n_triangles);
    } else {
        lay.max_tri = std::max(lay.max_tri, (int)q.n_triangles);
    }
}

// The stages of rtgo_whitted_set_scene.  Stage 1 (host only): every mesh as rtgo_whitted_set_mesh checks it, its padded box, where it will sit in the arrays, and packed there
static int whitted_layout_meshes(rtgo_ctx* c, const rtgo_whitted_mesh* meshes, uint32_t n_meshes, uint32_t n_materials, WhittedLayout& lay, const char* what)
{
    lay.info.assign(n_meshes, WhittedMeshInfo());
    for (uint32_t k = 0; k < n_meshes; ++k) {
        const rtgo_whitted_mesh& q = meshes[k];
        const std::string at = std::string(what) + ": mesh " + std::to_string(k);
        if (const int rc = whitted_admit_mesh(c, q, at, lay, false)) return rc;
        WhittedMeshInfo& mi = lay.info[k];
        if (const int rc = whitted_check_mesh(c, q, n_materials, at, mi.max_material)) return rc;
        whitted_mesh_box(q.positions, q.indices, q.n_triangles, mi.lo, mi.hi);
        whitted_place_mesh(q, lay, mi);
    }
    // the meshes' arrays back to back, zero where a mesh has no normals, texture coordinates or materials
    lay.pos.assign(3 * lay.n_vert, 0.0f);
    lay.nrm.assign(3 * lay.n_vert, 0.0f);
    lay.uv.assign(2 * lay.n_vert, 0.0f);
    lay.idx.assign(3 * lay.n_tri, 0u);
    lay.tmat.assign(lay.n_tri, 0u);
    for (size_t k = 0; k < lay.info.size(); ++k) {
        const rtgo_whitted_mesh& q = meshes[k];
        const WhittedMeshInfo& mi = lay.info[k];
        std::memcpy(&lay.pos[3 * (size_t)mi.vert_base], q.positions, (size_t)q.n_vertices * 3 * sizeof(float));
        if (q.normals) std::memcpy(&lay.nrm[3 * (size_t)mi.vert_base], q.normals, (size_t)q.n_vertices * 3 * sizeof(float));
        if (q.texcoords) std::memcpy(&lay.uv[2 * (size_t)mi.vert_base], q.texcoords, (size_t)q.n_vertices * 2 * sizeof(float));
        std::memcpy(&lay.idx[3 * (size_t)mi.tri_base], q.indices, (size_t)q.n_triangles * 3 * sizeof(unsigned int));
        if (q.material_of_triangle) std::memcpy(&lay.tmat[mi.tri_base], q.material_of_triangle, (size_t)q.n_triangles * sizeof(unsigned int));
    }
    return RTGO_OK;
}

// ---- meshes on the device (rtgo_whitted_set_scene_device, rtgo_whitted_set_mesh_device, rtgo_whitted_set_texcoords_device) ------------
// mesh_check_kernel and mesh_check_final_kernel over a table of the call's meshes (first_block / n_blocks are set here: a workgroup per
// kMeshCheckThreads vertices or triangles, whichever are more, at most 1024 per mesh): what whitted_check_mesh and whitted_mesh_box
// find of each in host loops, as report[k].  Up: 64 B per mesh; back: 32 B per mesh, one wait.  Nothing of the context is written.
// n_blocks: the workgroups of the table (mesh_pack_kernel's grid too).
static int whitted_check_meshes_on_device(rtgo_ctx* c, std::vector<whitted::MeshSource>& table, uint32_t n_materials, std::vector<whitted::MeshReport>& report,
                                          int& n_blocks)
{
    using namespace whitted;
    n_blocks = 0;
    for (MeshSource& m : table) {
        const size_t work = std::max<size_t>(std::max(m.n_verts, m.n_tris), 1);
        m.first_block = n_blocks;
        m.n_blocks = (int)std::min<size_t>(1024, (work + kMeshCheckThreads - 1) / kMeshCheckThreads);
        n_blocks += m.n_blocks;
    }
    DeviceArray<MeshSource> d_table;
    DeviceArray<float> partial;
    DeviceArray<unsigned int> part_words;
    DeviceArray<MeshReport> d_report;
    RTGO_HIP(c, d_table.upload(table.data(), table.size(), c->stream));
    RTGO_HIP(c, partial.alloc((size_t)6 * n_blocks));
    RTGO_HIP(c, part_words.alloc((size_t)2 * n_blocks));
    RTGO_HIP(c, d_report.alloc(table.size()));
    hipLaunchKernelGGL(mesh_check_kernel, dim3(n_blocks), dim3(kMeshCheckThreads), 0, c->stream, (const MeshSource*)d_table.get(), (int)table.size(), n_materials,
                       partial.get(), part_words.get());
    hipLaunchKernelGGL(mesh_check_final_kernel, dim3((unsigned int)table.size()), dim3(kMeshCheckThreads), 0, c->stream, (const MeshSource*)d_table.get(),
                       (const float*)partial.get(), (const unsigned int*)part_words.get(), d_report.get());
    RTGO_HIP(c, hipGetLastError());
    report.assign(table.size(), MeshReport{});
    RTGO_HIP(c, hipMemcpyAsync(report.data(), d_report.get(), table.size() * sizeof(MeshReport), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    return RTGO_OK;
}

// the refusal whitted_check_mesh gives a mesh with these kinds of fault: the first in its order
static int whitted_mesh_verdict(rtgo_ctx* c, const whitted::MeshReport& r, const std::string& at)
{
    for (int kind = 0; kind < whitted::kMeshFaultKinds; ++kind)
        if (r.faults >> kind & 1u) return fail(c, RTGO_E_INVALID, at + kMeshFault[kind]);
    return RTGO_OK;
}

// Stage 1 of rtgo_whitted_set_scene_device: whitted_layout_meshes for meshes whose arrays are device memory.  The host walks the meshes
// in the twin's order and decides what pointers and counts decide; the data of every mesh before the first it refuses (of all, when it
// refuses none) is checked where it lies, and the refusal is the twin's: the first mesh with a fault, and of its faults the first in
// whitted_check_mesh's order.  The boxes and largest material indices come back with the verdict; nothing is packed yet
// (lay.source: whitted_upload_meshes packs on the device, once the old scene is gone).  The stream has drained.
static int whitted_layout_meshes_device(rtgo_ctx* c, const rtgo_whitted_mesh* meshes, uint32_t n_meshes, uint32_t n_materials, WhittedLayout& lay, const char* what)
{
    using namespace whitted;
    lay.info.assign(n_meshes, WhittedMeshInfo());
    std::vector<MeshSource> table;
    int refused = RTGO_OK;   // what the host refuses of mesh table.size(), kept until the meshes before it are known to be sound
    std::string refusal;
    for (uint32_t k = 0; k < n_meshes && !refused; ++k) {
        const rtgo_whitted_mesh& q = meshes[k];
        refused = whitted_admit_mesh(c, q, std::string(what) + ": mesh " + std::to_string(k), lay, true);
        if (refused) {
            refusal = c->err;
            break;
        }
        table.push_back({q.positions, q.normals, q.texcoords, q.indices, q.material_of_triangle, q.n_vertices, q.n_triangles, 0, 0, (unsigned int)lay.n_vert,
                         (unsigned int)lay.n_tri});
        whitted_place_mesh(q, lay, lay.info[k]);
    }
    std::vector<MeshReport> report;
    if (!table.empty())
        if (const int rc = whitted_check_meshes_on_device(c, table, n_materials, report, lay.source_blocks)) return rc;
    for (size_t k = 0; k < table.size(); ++k) {
        if (const int rc = whitted_mesh_verdict(c, report[k], std::string(what) + ": mesh " + std::to_string(k))) return rc;
        WhittedMeshInfo& mi = lay.info[k];
        mi.max_material = report[k].max_material;
        whitted_pad_mesh_box(report[k].lo, report[k].hi, mi.lo, mi.hi);
    }
    if (refused) return fail(c, refused, refusal);
    lay.source = std::move(table);
    return RTGO_OK;
}

// Stage 2: the packed meshes and the materials to the device, and the arrays the builds write.  Meshes on the device: one launch packs
// them all (mesh_pack_kernel), whatever their number
static int whitted_upload_meshes(rtgo_ctx* c, WhittedMesh& wm, const WhittedLayout& lay, const rtgo_pbr* materials, uint32_t n_materials)
{
    if (lay.on_device()) {
        using namespace whitted;
        DeviceArray<MeshSource> d_table;
        RTGO_HIP(c, d_table.upload(lay.source.data(), lay.source.size(), c->stream));
        RTGO_HIP(c, wm.positions.alloc(3 * lay.n_vert));
        RTGO_HIP(c, wm.normals.alloc(3 * lay.n_vert));
        RTGO_HIP(c, wm.texcoords.alloc(2 * lay.n_vert));
        RTGO_HIP(c, wm.indices.alloc(3 * lay.n_tri));
        RTGO_HIP(c, wm.tri_material.alloc(lay.n_tri));
        hipLaunchKernelGGL(mesh_pack_kernel, dim3(lay.source_blocks), dim3(kMeshCheckThreads), 0, c->stream, (const MeshSource*)d_table.get(),
                           (int)lay.source.size(), wm.positions.get(), wm.normals.get(), wm.texcoords.get(), wm.indices.get(), wm.tri_material.get());
        RTGO_HIP(c, hipGetLastError());
        RTGO_HIP(c, hipStreamSynchronize(c->stream));   // (the table goes with this scope)
    } else {
        RTGO_HIP(c, wm.positions.upload(lay.pos.data(), lay.pos.size(), c->stream));
        RTGO_HIP(c, wm.normals.upload(lay.nrm.data(), lay.nrm.size(), c->stream));
        RTGO_HIP(c, wm.texcoords.upload(lay.uv.data(), lay.uv.size(), c->stream));
        RTGO_HIP(c, wm.indices.upload(lay.idx.data(), lay.idx.size(), c->stream));
        RTGO_HIP(c, wm.tri_material.upload(lay.tmat.data(), lay.tmat.size(), c->stream));
    }
    RTGO_HIP(c, wm.materials.upload((const whitted::Pbr*)materials, n_materials, c->stream));
    RTGO_HIP(c, wm.recs.alloc(lay.n_tri * 4));
    RTGO_HIP(c, wm.tris.alloc(lay.n_tri * 3));
    RTGO_HIP(c, wm.qrecs.alloc(lay.n_tri * 2));
    RTGO_HIP(c, wm.tidx.alloc(lay.n_tri));
    wm.n_vertices = (int)lay.n_vert;
    wm.n_materials = (int)n_materials;
    return RTGO_OK;
}

// The structures of the meshes `which` of info (laid out in wm's arrays, their vertices and indices on the device), each in its slice: a
// small mesh's one build, a clustered mesh's clusters and mid level.  Every build of the call goes through one table (whitted_run_batch),
// or with RTGO_WHITTED_SEQ_BUILD one after another -- the same arrays either way.  A mesh that was built before (built not empty: a
// rebuild) keeps its place in `table`, a new one is appended; built, mid_order, root and depth are set, a clustered mesh's box is widened
// (box_from_device: first taken from the triangle bounds its sort found, for a caller that has no indices on the host).  Synchronous.
static int whitted_build_structures(rtgo_ctx* c, const WhittedMesh& wm, std::vector<WhittedMeshInfo>& info, const std::vector<int>& which,
                                    std::vector<int4>& table, bool box_from_device, const char* what)
{
    using namespace whitted;
    const bool sequential = whitted_sequential_builds();
    const size_t nw = which.size();
    std::vector<WhittedBigScratch> big(nw);
    std::vector<float> bounds(6 * nw, 0.0f);
    std::vector<int> tbase(nw, -1), first(nw, 0);
    WhittedBatch batch;
    int next_tbase = (int)table.size(), max_tri = 1;
    for (size_t i = 0; i < nw; ++i) {
        WhittedMeshInfo& mi = info[which[i]];
        const int ncl = (mi.n_tris + kClusterTris - 1) / kClusterTris;
        if (mi.clustered) {
            tbase[i] = mi.built.empty() ? next_tbase : (mi.root - 1) >> 3;
            if (mi.built.empty()) next_tbase += ncl;
        }
        mi.built.clear();
        mi.mid_order.clear();
        first[i] = (int)batch.entries.size();
        max_tri = std::max(max_tri, mi.clustered ? std::max(kClusterTris, ncl) : mi.n_tris);
        if (mi.clustered) {
            if (const int rc = whitted_sort_clustered(c, wm, mi, big[i])) return rc;
            if (box_from_device) RTGO_HIP(c, hipMemcpyAsync(&bounds[6 * i], big[i].bounds.get(), 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            if (!sequential) whitted_add_clusters(wm, mi, big[i], batch);
        } else if (!sequential) {
            batch.add(wm.positions.get() + 3 * (size_t)mi.vert_base, wm.indices.get() + 3 * (size_t)mi.tri_base, mi.n_tris, whitted_target(wm, 0, mi.tri_base),
                      mi.rec_base);
        }
    }
    WhittedBuildScratch scratch;
    if (sequential) {
        RTGO_HIP(c, scratch.alloc(max_tri));
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
    } else if (const int rc = whitted_run_batch(c, batch, wm.recs.get(), what)) {
        return rc;
    }
    for (size_t i = 0; i < nw; ++i) {
        WhittedMeshInfo& mi = info[which[i]];
        if (mi.clustered) {
            WhittedClusterBuilds cb;
            if (sequential) {
                if (const int rc = whitted_build_clusters_sequential(c, wm, mi, big[i], scratch, cb, what)) return rc;
            } else {
                whitted_take_clusters(mi, batch, first[i], cb);
            }
            if (box_from_device) whitted_pad_mesh_box(&bounds[6 * i], &bounds[6 * i + 3], mi.lo, mi.hi);
            if (const int rc = whitted_finish_clustered(c, wm, mi, big[i], cb, table, tbase[i], what)) return rc;
        } else {
            WhittedBuildMeta m;
            if (sequential) {
                if (const int rc = whitted_build(c, wm.positions.get() + 3 * (size_t)mi.vert_base, wm.indices.get() + 3 * (size_t)mi.tri_base, mi.n_tris,
                                                 whitted_target(wm, mi.rec_base, mi.tri_base), scratch, m, what))
                    return rc;
            } else {
                m = batch.metas[first[i]];
            }
            mi.built.push_back({mi.rec_base, m.n_recs, mi.tri_base, m});
            mi.root = m.n_recs > 0 ? 0 : -1 - ((mi.n_tris - 1) << kLeafShift);
            mi.depth = m.n_recs > 0 ? m.walk_depth : 0;
        }
    }
    return RTGO_OK;
}

// Stage 3, the bottom level: each mesh's own structure in its slice of the arrays (a clustered mesh: its clusters and mid level), then the table
static int whitted_build_meshes(rtgo_ctx* c, WhittedMesh& wm, WhittedLayout& lay, const char* what)
{
    std::vector<int> all(lay.info.size());
    for (size_t k = 0; k < all.size(); ++k) all[k] = (int)k;
    std::vector<int4> table;
    if (const int rc = whitted_build_structures(c, wm, lay.info, all, table, false, what)) return rc;
    for (const WhittedMeshInfo& mi : lay.info) wm.mesh_depth = std::max(wm.mesh_depth, mi.depth);
    if (!table.empty()) RTGO_HIP(c, wm.clusters.upload(table.data(), table.size(), c->stream));
    wm.meshes = lay.info;
    return RTGO_OK;
}

// rtgo_whitted_set_scene and rtgo_whitted_set_scene_device (`what`, for the messages; on_device: the meshes' arrays are device memory)
// once the arguments themselves are known to be there: the stages above over a scene built aside.  A refusal by the checks, on the host or
// on the device, leaves the old scene; once that is dropped, a failure leaves none.
static int whitted_set_scene(rtgo_ctx* c, const char* what, const rtgo_whitted_mesh* meshes, uint32_t n_meshes, const rtgo_whitted_instance* instances,
                             uint32_t n_instances, const rtgo_pbr* materials, uint32_t n_materials, bool on_device)
{
    WhittedLayout lay;
    std::vector<whitted::InstShade> shade;
    std::vector<float> box_pos;
    if (on_device) {   // (the checks launch: the device current and the stream drained before them)
        RTGO_HIP(c, hipSetDevice(c->device));
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
        if (const int rc = whitted_layout_meshes_device(c, meshes, n_meshes, n_materials, lay, what)) return rc;
    } else if (const int rc = whitted_layout_meshes(c, meshes, n_meshes, n_materials, lay, what)) {
        return rc;
    }
    if (const int rc = whitted_prepare_instances(c, lay.info, n_materials, instances, n_instances, shade, box_pos, what)) return rc;
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    c->wm = WhittedMesh();
    WhittedMesh next;
    if (const int rc = whitted_upload_meshes(c, next, lay, materials, n_materials)) return rc;
    if (const int rc = whitted_build_meshes(c, next, lay, what)) return rc;
    // the clustered meshes' boxes took in their mid levels' boxes: the instance boxes again from them (the checks passed above)
    if (next.clusters.get())
        if (const int rc = whitted_prepare_instances(c, next.meshes, n_materials, instances, n_instances, shade, box_pos, what)) return rc;
    if (const int rc = whitted_build_top(c, next, shade, box_pos, instances, what)) return rc;
    if (const int rc = whitted_tile_heads(c)) return rc;
    next.instanced = true;
    next.triangles = (int)std::min(lay.n_tri, (size_t)0x7FFFFFFF);
    c->wm = std::move(next);
    return RTGO_OK;
}

// rtgo_whitted_set_mesh and rtgo_whitted_set_mesh_device (`what`; on_device: the mesh's arrays are device memory, checked where they
// lie by the scene call's kernels over a table of this one mesh) once pointers and counts have passed
static int whitted_set_mesh(rtgo_ctx* c, const char* what, const rtgo_whitted_mesh& mesh, const rtgo_pbr* materials, uint32_t n_materials, bool on_device)
{
    if (on_device) {
        RTGO_HIP(c, hipSetDevice(c->device));
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
        std::vector<whitted::MeshSource> table = {{mesh.positions, mesh.normals, nullptr, mesh.indices, mesh.material_of_triangle, mesh.n_vertices, mesh.n_triangles, 0, 0, 0, 0}};
        std::vector<whitted::MeshReport> report;
        int n_blocks = 0;
        if (const int rc = whitted_check_meshes_on_device(c, table, n_materials, report, n_blocks)) return rc;
        if (const int rc = whitted_mesh_verdict(c, report[0], what)) return rc;
    } else {
        uint32_t max_material;
        if (const int rc = whitted_check_mesh(c, mesh, n_materials, what, max_material)) return rc;
    }
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    c->wm = WhittedMesh();   // (the old scene goes before the new one is allocated; a failure from here on leaves none)
    WhittedMesh next;
    if (const int rc = whitted_build_single(c, next, mesh, materials, n_materials, what, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)) return rc;
    if (const int rc = whitted_tile_heads(c)) return rc;
    next.triangles = (int)mesh.n_triangles;
    c->wm = std::move(next);
    return RTGO_OK;
}

// rtgo_whitted_set_texcoords and rtgo_whitted_set_texcoords_device (`what`; on_device: uv is device memory) once state and count have
// passed: the finite check (on the device: mesh_check_kernel over a table that has texture coordinates alone), then the copy
static int whitted_set_texcoords(rtgo_ctx* c, const char* what, const float* uv, uint32_t n_vertices, bool on_device)
{
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    bool bad = false;
    if (uv && on_device) {
        std::vector<whitted::MeshSource> table = {{nullptr, nullptr, uv, nullptr, nullptr, n_vertices, 0, 0, 0, 0, 0}};
        std::vector<whitted::MeshReport> report;
        int n_blocks = 0;
        if (const int rc = whitted_check_meshes_on_device(c, table, 1, report, n_blocks)) return rc;
        bad = report[0].faults != 0;
    } else if (uv) {
        for (size_t k = 0; k < (size_t)n_vertices * 2 && !bad; ++k) bad = !std::isfinite(uv[k]);
    }
    if (bad) return fail(c, RTGO_E_INVALID, std::string(what) + ": non-finite coordinate");
    c->wm.texcoords.reset();
    if (uv) {
        RTGO_HIP(c, c->wm.texcoords.alloc((size_t)n_vertices * 2));
        RTGO_HIP(c, hipMemcpyAsync(c->wm.texcoords.get(), uv, (size_t)n_vertices * 2 * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
    }
    return RTGO_OK;
}

// ---- refit (rtgo_whitted_update_mesh) -------------------------------------------------------------------------------------------
// What rtgo_whitted_update_mesh needs to know of the mesh it moves: where it sits in wm's arrays and what its build reported
struct WhittedRefitMesh { int vert_base, tri_base, rec_base, n_verts, n_tris; bool has_normals; WhittedBuildMeta meta; };

// New vertices into the mesh's slice of wm's arrays and refit_kernel over its structure; `m.meta` gets the new grid.  Synchronous.
static int whitted_refit(rtgo_ctx* c, WhittedMesh& wm, WhittedRefitMesh& m, const float* positions, const float* normals)
{
    float* d_pos = wm.positions.get() + 3 * (size_t)m.vert_base;
    const size_t bytes = (size_t)m.n_verts * 3 * sizeof(float);
    DeviceArray<int> done;                          // refit_kernel's flags, one per record
    DeviceArray<WhittedBuildMeta> d_meta;
    RTGO_HIP(c, done.alloc((size_t)std::max(m.meta.n_recs, 1)));
    RTGO_HIP(c, d_meta.alloc(1));
    RTGO_HIP(c, hipMemcpyAsync(d_pos, positions, bytes, hipMemcpyHostToDevice, c->stream));
    if (normals) RTGO_HIP(c, hipMemcpyAsync(wm.normals.get() + 3 * (size_t)m.vert_base, normals, bytes, hipMemcpyHostToDevice, c->stream));
    const WhittedBuildTarget t = whitted_target(wm, m.rec_base, m.tri_base);
    hipLaunchKernelGGL(whitted::refit_kernel, dim3(1), dim3(whitted::kBuildThreads), 0, c->stream, (const float*)d_pos,
                       (const unsigned int*)(wm.indices.get() + 3 * (size_t)m.tri_base), m.n_tris, m.meta.n_recs, m.meta.walk_depth, t.recs, t.tris, t.qrecs,
                       done.get(), d_meta.get());
    RTGO_HIP(c, hipGetLastError());
    v3 grid[2];
    RTGO_HIP(c, hipMemcpyAsync(grid, &d_meta.get()->grid_lo, sizeof grid, hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    m.meta.grid_lo = grid[0];
    m.meta.grid_step = grid[1];
    return RTGO_OK;
}

// rtgo_whitted_update_mesh once the scene is known to exist: every check on the host first, and for an instanced scene the new top level
// built aside (it needs only the mesh's new box) -- a refused call leaves the scene as it was; then the refit, then what the host keeps.
static int whitted_update_mesh(rtgo_ctx* c, uint32_t mesh, const float* positions, const float* normals, uint32_t n_vertices)
{
    const char* what = "rtgo_whitted_update_mesh";
    const std::string w(what);
    WhittedMesh& wm = c->wm;
    if (mesh >= (wm.instanced ? wm.meshes.size() : (size_t)1)) return fail(c, RTGO_E_INVALID, w + ": mesh index beyond the scene's meshes");
    if (!positions) return fail(c, RTGO_E_INVALID, w + ": NULL positions");
    WhittedRefitMesh m = {0, 0, 0, wm.n_vertices, wm.triangles, wm.normals.get() != nullptr, wm.meta};
    if (wm.instanced) {
        const WhittedMeshInfo& mi = wm.meshes[mesh];
        if (mi.clustered)
            return fail(c, RTGO_E_UNSUPPORTED, w + ": a mesh beyond " + std::to_string(RTGO_MAX_TRIANGLES) + " triangles (clustered) takes new vertices through rtgo_whitted_set_scene");
        m = {mi.vert_base, mi.tri_base, mi.rec_base, mi.n_verts, mi.n_tris, (mi.flags & whitted::kHasNormals) != 0, mi.built[0].meta};
    }
    if (n_vertices != (uint32_t)m.n_verts) return fail(c, RTGO_E_INVALID, w + ": the mesh has " + std::to_string(m.n_verts) + " vertices");
    if (normals && !m.has_normals) return fail(c, RTGO_E_INVALID, w + ": normals for a mesh that was set without");
    for (size_t i = 0; i < (size_t)3 * n_vertices; ++i)
        if (!std::isfinite(positions[i]) || (normals && !std::isfinite(normals[i]))) return fail(c, RTGO_E_INVALID, w + ": non-finite vertex data");
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    if (const int rc = whitted_refresh_host(c)) return rc;
    if (!wm.instanced) {
        if (const int rc = whitted_refit(c, wm, m, positions, normals)) return rc;
        wm.meta = m.meta;
        return RTGO_OK;
    }
    // the mesh's new box (its indices are on the device only), every instance laid out again, the top level over them
    std::vector<uint32_t> idx((size_t)3 * m.n_tris);
    RTGO_HIP(c, hipMemcpyAsync(idx.data(), wm.indices.get() + 3 * (size_t)m.tri_base, idx.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<WhittedMeshInfo> meshes = wm.meshes;
    whitted_mesh_box(positions, idx.data(), (uint32_t)m.n_tris, meshes[mesh].lo, meshes[mesh].hi);
    std::vector<whitted::InstShade> shade;
    std::vector<float> box_pos;
    if (const int rc = whitted_prepare_instances(c, meshes, (uint32_t)wm.n_materials, wm.instances.data(), (uint32_t)wm.instances.size(), shade, box_pos, what)) return rc;
    WhittedTop top;
    int depth = 0;
    if (const int rc = whitted_make_top(c, wm, shade, box_pos, wm.instances.data(), what, top, depth)) return rc;
    if (const int rc = whitted_refit(c, wm, m, positions, normals)) return rc;
    meshes[mesh].built[0].meta = m.meta;
    wm.meshes = std::move(meshes);
    whitted_install_top(wm, std::move(top), depth);
    return RTGO_OK;
}

// ---- refit of a clustered mesh (rtgo_whitted_update_meshes) -------------------------------------------------------------------------
// One clustered mesh's refit in flight: what it replaces of wm's arrays, kept until the call is known to succeed (the box its instances
// are laid out from is known only after the refit, so a refusal can follow it: whitted_restore_clustered puts these back), the device
// scratch of its launches, and what they report.  All of it is proportional to the mesh and freed with this.
struct WhittedClusteredRefit {
    int mesh = 0, ncl = 0;
    const float *positions = nullptr, *normals = nullptr;   // the caller's, and where they lie
    hipMemcpyKind kind = hipMemcpyHostToDevice;
    DeviceArray<float> old_positions, old_normals;
    DeviceArray<float4> old_recs, old_tris;
    DeviceArray<uint4> old_qrecs;
    DeviceArray<int> ints;          // ClusterRefit[ncl], the clusters' record bases [ncl], the mid level's index triples [3 ncl]; then done[n] and the mid level's done[ncl]
    DeviceArray<float4> mid_tris;   // the mid level's "triangles": .w of each first corner is the cluster at that leaf position
    DeviceArray<uint4> mid_qrecs;
    DeviceArray<float> partial;     // big_bounds_kernel's
    DeviceArray<float> report;      // what comes back: bounds [6], the clusters' boxes [6 ncl], WhittedBuildMeta [ncl + 1] (the mid level's last)
    std::vector<float> host;        // ... on the host, then the mid root's record [16]
    std::vector<int> up_ints;       // what `ints` and `mid_tris` are uploaded from: alive until the stream has drained
    std::vector<float4> up_mid_tris;
};

// Stage 2 of whitted_refit_named for a clustered mesh: saves the slices, copies the vertices in and enqueues the refit and its read-back.
// Three launches refit it whatever its size -- every cluster (one workgroup each), the clusters' boxes, the mid level over them -- and
// two find its bounds.  Nothing here waits for the device.
static int whitted_enqueue_clustered_refit(rtgo_ctx* c, WhittedMesh& wm, const WhittedMeshInfo& mi, WhittedClusteredRefit& r)
{
    using namespace whitted;
    const int n = mi.n_tris, ncl = (int)mi.built.size() - 1;
    const size_t nv3 = (size_t)mi.n_verts * 3;
    r.ncl = ncl;
    float* d_pos = wm.positions.get() + 3 * (size_t)mi.vert_base;
    float* d_nrm = wm.normals.get() + 3 * (size_t)mi.vert_base;
    const unsigned int* d_idx = wm.indices.get() + 3 * (size_t)mi.tri_base;
    const WhittedBuildTarget t = whitted_target(wm, mi.rec_base, mi.tri_base);   // (a mesh of n triangles owns n record slots)
    auto save = [&](auto& keep, const auto* src, size_t count) -> hipError_t {
        const hipError_t e = keep.alloc(count);
        return e != hipSuccess ? e : hipMemcpyAsync(keep.get(), src, count * sizeof *src, hipMemcpyDeviceToDevice, c->stream);
    };
    RTGO_HIP(c, save(r.old_positions, d_pos, nv3));
    if (r.normals) RTGO_HIP(c, save(r.old_normals, d_nrm, nv3));
    RTGO_HIP(c, save(r.old_recs, t.recs, (size_t)4 * n));
    RTGO_HIP(c, save(r.old_tris, t.tris, (size_t)3 * n));
    RTGO_HIP(c, save(r.old_qrecs, t.qrecs, (size_t)2 * n));
    RTGO_HIP(c, hipMemcpyAsync(d_pos, r.positions, nv3 * sizeof(float), r.kind, c->stream));
    if (r.normals) RTGO_HIP(c, hipMemcpyAsync(d_nrm, r.normals, nv3 * sizeof(float), r.kind, c->stream));
    // the launches' tables, one upload
    static_assert(sizeof(ClusterRefit) == 5 * sizeof(int), "five words");
    const size_t o_crec = (size_t)5 * ncl, o_idx = o_crec + ncl, o_done = o_idx + (size_t)3 * ncl, o_mid_done = o_done + n;
    std::vector<int>& ints = r.up_ints;
    std::vector<float4>& mid_tris = r.up_mid_tris;
    ints.assign(o_done, 0);
    mid_tris.assign((size_t)3 * ncl, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (int k = 0; k < ncl; ++k) {
        const WhittedMeshInfo::Built& b = mi.built[k];
        const ClusterRefit cr = {b.rec0, b.tri0 - mi.tri_base, cluster_start(n, ncl, k + 1) - cluster_start(n, ncl, k), b.n_recs, b.meta.walk_depth};
        std::memcpy(&ints[(size_t)5 * k], &cr, sizeof cr);
        ints[o_crec + k] = b.rec0;
        for (int j = 0; j < 3; ++j) ints[o_idx + 3 * (size_t)k + j] = 2 * k + (j == 1 ? 1 : 0);   // whitted_build_boxes's degenerate triangle (lo, hi, lo)
        std::memcpy(&mid_tris[3 * (size_t)k].w, &mi.mid_order[k], sizeof(int));
    }
    RTGO_HIP(c, r.ints.alloc(o_mid_done + ncl));
    RTGO_HIP(c, hipMemcpyAsync(r.ints.get(), ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    RTGO_HIP(c, r.mid_tris.upload(mid_tris.data(), mid_tris.size(), c->stream));
    RTGO_HIP(c, r.mid_qrecs.alloc((size_t)2 * ncl));
    RTGO_HIP(c, r.partial.alloc((size_t)6 * 1024));
    const size_t o_boxes = 6, o_meta = o_boxes + (size_t)6 * ncl, n_report = o_meta + (size_t)9 * (ncl + 1);
    RTGO_HIP(c, r.report.alloc(n_report));
    float* d_bounds = r.report.get();
    float* d_boxes = r.report.get() + o_boxes;
    WhittedBuildMeta* d_meta = reinterpret_cast<WhittedBuildMeta*>(r.report.get() + o_meta);
    const WhittedBuildMeta& mid = mi.built[ncl].meta;
    // the triangle bounds (exact min / max: whitted_mesh_box's, without the indices leaving the device)
    const int nbb = std::min(1024, (n + 1023) / 1024);
    hipLaunchKernelGGL(big_bounds_kernel, dim3(nbb), dim3(1024), 0, c->stream, (const float*)d_pos, d_idx, n, r.partial.get());
    hipLaunchKernelGGL(big_bounds_final_kernel, dim3(1), dim3(1024), 0, c->stream, (const float*)r.partial.get(), nbb, d_bounds);
    // clusters -> their boxes -> the mid level (kernel boundaries order them)
    hipLaunchKernelGGL(big_refit_clusters_kernel, dim3(ncl), dim3(kBuildThreads), 0, c->stream, (const float*)d_pos, d_idx, (const ClusterRefit*)r.ints.get(),
                       wm.recs.get(), t.tris, t.qrecs, r.ints.get() + o_done, d_meta);
    hipLaunchKernelGGL(big_cluster_boxes_kernel, dim3((ncl + 255) / 256), dim3(256), 0, c->stream, (const float4*)wm.recs.get(), (const int*)(r.ints.get() + o_crec),
                       ncl, d_boxes);
    hipLaunchKernelGGL(refit_kernel, dim3(1), dim3(kBuildThreads), 0, c->stream, (const float*)d_boxes, (const unsigned int*)(r.ints.get() + o_idx), ncl,
                       mi.built[ncl].n_recs, mid.walk_depth, t.recs, r.mid_tris.get(), r.mid_qrecs.get(), r.ints.get() + o_mid_done, d_meta + ncl);
    RTGO_HIP(c, hipGetLastError());
    r.host.assign(n_report + 16, 0.0f);
    RTGO_HIP(c, hipMemcpyAsync(r.host.data(), r.report.get(), n_report * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (mi.built[ncl].n_recs > 0) RTGO_HIP(c, hipMemcpyAsync(&r.host[n_report], t.recs, 16 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return RTGO_OK;
}

// ... and once the stream has drained: the mesh's box as whitted_finish_clustered takes it, and the grids its builds now report
static void whitted_finish_clustered_refit(WhittedMeshInfo& mi, const WhittedClusteredRefit& r)
{
    const int ncl = r.ncl;
    const float* bounds = r.host.data();
    const float* boxes = bounds + 6;
    const float* meta = boxes + (size_t)6 * ncl;
    const float* root = meta + (size_t)9 * (ncl + 1);
    whitted_pad_mesh_box(bounds, bounds + 3, mi.lo, mi.hi);
    auto widen = [&](const float* l, const float* h) {
        for (int a = 0; a < 3; ++a) {
            mi.lo[a] = std::fmin(mi.lo[a], l[a]);
            mi.hi[a] = std::fmax(mi.hi[a], h[a]);
        }
    };
    if (mi.built[ncl].n_recs > 0) {
        widen(root, root + 4);
        widen(root + 8, root + 12);
    }
    for (int k = 0; k < ncl; ++k) widen(boxes + 6 * (size_t)k, boxes + 6 * (size_t)k + 3);
    for (int k = 0; k <= ncl; ++k) {
        WhittedBuildMeta m;
        std::memcpy(&m, meta + (size_t)9 * k, sizeof m);
        mi.built[k].meta.grid_lo = m.grid_lo;
        mi.built[k].meta.grid_step = m.grid_step;
    }
}

// A refused call: the mesh's slices as they were.  Enqueued; the caller waits.
static int whitted_restore_clustered(rtgo_ctx* c, WhittedMesh& wm, const WhittedMeshInfo& mi, const WhittedClusteredRefit& r)
{
    const WhittedBuildTarget t = whitted_target(wm, mi.rec_base, mi.tri_base);
    auto back = [&](auto* dst, const auto& keep) { return hipMemcpyAsync(dst, keep.get(), keep.size() * sizeof *dst, hipMemcpyDeviceToDevice, c->stream); };
    RTGO_HIP(c, back(wm.positions.get() + 3 * (size_t)mi.vert_base, r.old_positions));
    if (r.normals) RTGO_HIP(c, back(wm.normals.get() + 3 * (size_t)mi.vert_base, r.old_normals));
    RTGO_HIP(c, back(t.recs, r.old_recs));
    RTGO_HIP(c, back(t.tris, r.old_tris));
    RTGO_HIP(c, back(t.qrecs, r.old_qrecs));
    return RTGO_OK;
}

// Where the vertices of a call's entries lie: host memory (rtgo_whitted_update_meshes, rtgo_whitted_rebuild_meshes), or the device
// (rtgo_whitted_update_meshes_device), then with what whitted_check_on_device reported of each entry
struct WhittedUpdateSource {
    hipMemcpyKind kind;
    const whitted::UpdateReport* report;   // NULL: host memory
    bool on_device() const { return report != nullptr; }
};

// The checks rtgo_whitted_update_meshes and rtgo_whitted_rebuild_meshes make of their entries on the host (w: the call, for the
// messages).  on_device: the entries point to device memory (rtgo_whitted_update_meshes_device) -- the pointers' alignment is checked
// here, NULL and misaligned ones never reach a launch, and the data itself is left to whitted_check_on_device.
static int whitted_check_updates(rtgo_ctx* c, const WhittedMesh& wm, const std::string& w, const rtgo_whitted_mesh_update* updates, uint32_t n_updates,
                                 bool on_device = false)
{
    const size_t n_meshes = wm.instanced ? wm.meshes.size() : (size_t)1;
    std::vector<char> named(n_meshes, 0);
    for (uint32_t k = 0; k < n_updates; ++k) {
        const rtgo_whitted_mesh_update& u = updates[k];
        const std::string at = w + ": update " + std::to_string(k);
        if (u.mesh >= n_meshes) return fail(c, RTGO_E_INVALID, at + ": mesh index beyond the scene's meshes");
        if (named[u.mesh]) return fail(c, RTGO_E_INVALID, at + ": mesh " + std::to_string(u.mesh) + " is named twice");
        named[u.mesh] = 1;
        if (!u.positions) return fail(c, RTGO_E_INVALID, at + ": NULL positions");
        const int n_verts = wm.instanced ? wm.meshes[u.mesh].n_verts : wm.n_vertices;
        const bool has_normals = wm.instanced ? (wm.meshes[u.mesh].flags & whitted::kHasNormals) != 0 : wm.normals.get() != nullptr;
        if (u.n_vertices != (uint32_t)n_verts) return fail(c, RTGO_E_INVALID, at + ": the mesh has " + std::to_string(n_verts) + " vertices");
        if (u.normals && !has_normals) return fail(c, RTGO_E_INVALID, at + ": normals for a mesh that was set without");
        if (on_device) {
            if ((uintptr_t)u.positions % alignof(float) || (uintptr_t)u.normals % alignof(float))
                return fail(c, RTGO_E_INVALID, at + ": positions and normals must be 4-byte aligned");
            continue;
        }
        for (size_t i = 0; i < (size_t)3 * u.n_vertices; ++i)
            if (!std::isfinite(u.positions[i]) || (u.normals && !std::isfinite(u.normals[i]))) return fail(c, RTGO_E_INVALID, at + ": non-finite vertex data");
    }
    return RTGO_OK;
}

// The rest of those checks for entries in device memory, and the boxes of the call's small meshes, by one pair of launches over a table of
// the entries (big_update_check_kernel, big_update_check_final_kernel): report[k] says whether entry k holds a non-finite float and, for
// a small mesh of an instanced scene, has the bounds of the vertices its triangles name, read from the caller's buffer through the
// scene's indices (whitted_pad_mesh_box then gives whitted_mesh_box's box).  One copy back, 32 B per entry, and one wait; nothing of the
// scene is written.
static int whitted_check_on_device(rtgo_ctx* c, const WhittedMesh& wm, const std::string& w, const rtgo_whitted_mesh_update* updates, uint32_t n_updates,
                                   std::vector<whitted::UpdateReport>& report)
{
    using namespace whitted;
    std::vector<UpdateCheck> table(n_updates);
    int n_blocks = 0;
    for (uint32_t k = 0; k < n_updates; ++k) {
        const rtgo_whitted_mesh_update& u = updates[k];
        const bool box = wm.instanced && !wm.meshes[u.mesh].clustered;   // (a clustered mesh's comes from its refit or build)
        const int n_tris = box ? wm.meshes[u.mesh].n_tris : 0;
        const size_t work = std::max((size_t)3 * u.n_vertices, (size_t)n_tris);
        const int nb = (int)std::min<size_t>(1024, (work + 1023) / 1024);
        table[k] = {u.positions, u.normals, box ? wm.indices.get() + 3 * (size_t)wm.meshes[u.mesh].tri_base : nullptr, u.n_vertices, n_tris, n_blocks, nb};
        n_blocks += nb;
    }
    DeviceArray<UpdateCheck> d_table;
    DeviceArray<float> partial;
    DeviceArray<unsigned int> part_bad;
    DeviceArray<UpdateReport> d_report;
    RTGO_HIP(c, d_table.upload(table.data(), table.size(), c->stream));
    RTGO_HIP(c, partial.alloc((size_t)6 * n_blocks));
    RTGO_HIP(c, part_bad.alloc(n_blocks));
    RTGO_HIP(c, d_report.alloc(n_updates));
    hipLaunchKernelGGL(big_update_check_kernel, dim3(n_blocks), dim3(1024), 0, c->stream, (const UpdateCheck*)d_table.get(), (int)n_updates, partial.get(),
                       part_bad.get());
    hipLaunchKernelGGL(big_update_check_final_kernel, dim3(n_updates), dim3(1024), 0, c->stream, (const UpdateCheck*)d_table.get(), (const float*)partial.get(),
                       (const unsigned int*)part_bad.get(), d_report.get());
    RTGO_HIP(c, hipGetLastError());
    report.assign(n_updates, UpdateReport{});
    RTGO_HIP(c, hipMemcpyAsync(report.data(), d_report.get(), n_updates * sizeof(UpdateReport), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n_updates; ++k)
        if (report[k].bad) return fail(c, RTGO_E_INVALID, w + ": update " + std::to_string(k) + ": non-finite vertex data");
    return RTGO_OK;
}

// An entry's vertices into its mesh's slice of wm's arrays (enqueued)
static int whitted_put_vertices(rtgo_ctx* c, WhittedMesh& wm, int vert_base, int n_verts, const rtgo_whitted_mesh_update& u, hipMemcpyKind kind)
{
    const size_t bytes = (size_t)n_verts * 3 * sizeof(float);
    RTGO_HIP(c, hipMemcpyAsync(wm.positions.get() + 3 * (size_t)vert_base, u.positions, bytes, kind, c->stream));
    if (u.normals) RTGO_HIP(c, hipMemcpyAsync(wm.normals.get() + 3 * (size_t)vert_base, u.normals, bytes, kind, c->stream));
    return RTGO_OK;
}

// whitted_refit's launch for every mesh of `ms` at once (their new vertices are in wm's arrays, or enqueued before this): one workgroup
// per mesh (big_refit_meshes_kernel), one scratch allocation -- the table, the grids that come back, refit_kernel's flags -- and one
// wait, however many meshes; every m.meta gets its new grid.  Synchronous.
static int whitted_refit_small(rtgo_ctx* c, WhittedMesh& wm, std::vector<WhittedRefitMesh>& ms)
{
    using namespace whitted;
    const size_t k = ms.size();
    if (k == 0) return RTGO_OK;
    static_assert(sizeof(MeshRefit) == 8 * sizeof(int) && sizeof(WhittedBuildMeta) == 9 * sizeof(int), "the scratch is laid out in words");
    const size_t o_meta = 8 * k, o_done = o_meta + 9 * k;
    std::vector<MeshRefit> table(k);
    size_t n_done = 0;
    for (size_t i = 0; i < k; ++i) {
        const WhittedRefitMesh& m = ms[i];
        table[i] = {m.vert_base, m.tri_base, m.rec_base, m.n_tris, m.meta.n_recs, m.meta.walk_depth, (int)n_done, 0};
        n_done += (size_t)std::max(m.meta.n_recs, 1);
    }
    DeviceArray<int> scratch;
    RTGO_HIP(c, scratch.alloc(o_done + n_done));
    RTGO_HIP(c, hipMemcpyAsync(scratch.get(), table.data(), k * sizeof(MeshRefit), hipMemcpyHostToDevice, c->stream));
    WhittedBuildMeta* d_meta = reinterpret_cast<WhittedBuildMeta*>(scratch.get() + o_meta);
    hipLaunchKernelGGL(big_refit_meshes_kernel, dim3((unsigned int)k), dim3(kBuildThreads), 0, c->stream, (const float*)wm.positions.get(),
                       (const unsigned int*)wm.indices.get(), reinterpret_cast<const MeshRefit*>(scratch.get()), wm.recs.get(), wm.tris.get(), wm.qrecs.get(),
                       scratch.get() + o_done, d_meta);
    RTGO_HIP(c, hipGetLastError());
    std::vector<WhittedBuildMeta> metas(k);
    RTGO_HIP(c, hipMemcpyAsync(metas.data(), d_meta, k * sizeof(WhittedBuildMeta), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < k; ++i) {   // (the kernel writes the grid alone)
        ms[i].meta.grid_lo = metas[i].grid_lo;
        ms[i].meta.grid_step = metas[i].grid_step;
    }
    return RTGO_OK;
}

// The refits of rtgo_whitted_update_meshes and rtgo_whitted_update_meshes_device (`what`: the call, for the messages) once every entry
// has passed its checks and the stream has drained: rtgo_whitted_update_mesh for every entry as one transaction.  Stages: 2 every mesh's
// new box (a small mesh: from its indices read back, all in one wait -- or, vertices on the device, from what whitted_check_on_device
// reported, and nothing is read back; a clustered mesh: refitted in place with its slices saved, its box from what the device reports);
// 3 the instances laid out and the top level built, once, aside; 4 the small meshes' vertices in and their refits, one launch
// (whitted_refit_small); 5 what the host keeps.  A refusal in stage 3 puts the clustered meshes' slices back: nothing else has changed
// by then.
static int whitted_refit_named(rtgo_ctx* c, const char* what, const rtgo_whitted_mesh_update* updates, uint32_t n_updates, const WhittedUpdateSource& src)
{
    WhittedMesh& wm = c->wm;
    if (!wm.instanced) {
        std::vector<WhittedRefitMesh> one = {{0, 0, 0, wm.n_vertices, wm.triangles, wm.normals.get() != nullptr, wm.meta}};
        if (const int rc = whitted_put_vertices(c, wm, 0, wm.n_vertices, updates[0], src.kind)) return rc;
        if (const int rc = whitted_refit_small(c, wm, one)) return rc;
        wm.meta = one[0].meta;
        return RTGO_OK;
    }
    if (const int rc = whitted_refresh_host(c)) return rc;
    // stage 2
    std::vector<WhittedMeshInfo> meshes = wm.meshes;
    std::vector<std::vector<uint32_t>> idx(n_updates);
    std::vector<WhittedClusteredRefit> big;
    big.reserve(n_updates);
    for (uint32_t k = 0; k < n_updates; ++k) {
        const rtgo_whitted_mesh_update& u = updates[k];
        const WhittedMeshInfo& mi = meshes[u.mesh];
        if (mi.clustered) {
            big.emplace_back();
            big.back().mesh = (int)u.mesh;
            big.back().positions = u.positions;
            big.back().normals = u.normals;
            big.back().kind = src.kind;
            if (const int rc = whitted_enqueue_clustered_refit(c, wm, mi, big.back())) return rc;
        } else if (!src.on_device()) {
            idx[k].resize((size_t)3 * mi.n_tris);
            RTGO_HIP(c, hipMemcpyAsync(idx[k].data(), wm.indices.get() + 3 * (size_t)mi.tri_base, idx[k].size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (!big.empty() || !src.on_device()) RTGO_HIP(c, hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n_updates; ++k) {
        WhittedMeshInfo& mi = meshes[updates[k].mesh];
        if (mi.clustered) continue;
        if (src.on_device()) whitted_pad_mesh_box(src.report[k].lo, src.report[k].hi, mi.lo, mi.hi);
        else whitted_mesh_box(updates[k].positions, idx[k].data(), (uint32_t)mi.n_tris, mi.lo, mi.hi);
    }
    for (const WhittedClusteredRefit& r : big) whitted_finish_clustered_refit(meshes[r.mesh], r);
    // stage 3
    std::vector<whitted::InstShade> shade;
    std::vector<float> box_pos;
    WhittedTop top;
    int depth = 0;
    int rc = whitted_prepare_instances(c, meshes, (uint32_t)wm.n_materials, wm.instances.data(), (uint32_t)wm.instances.size(), shade, box_pos, what);
    if (!rc) rc = whitted_make_top(c, wm, shade, box_pos, wm.instances.data(), what, top, depth);
    if (rc) {
        for (const WhittedClusteredRefit& r : big)
            if (const int rc2 = whitted_restore_clustered(c, wm, wm.meshes[r.mesh], r)) return rc2;
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
        return rc;
    }
    // stage 4
    std::vector<WhittedRefitMesh> small;
    std::vector<uint32_t> small_mesh;
    for (uint32_t k = 0; k < n_updates; ++k) {
        const rtgo_whitted_mesh_update& u = updates[k];
        const WhittedMeshInfo& mi = meshes[u.mesh];
        if (mi.clustered) continue;
        if (const int rc4 = whitted_put_vertices(c, wm, mi.vert_base, mi.n_verts, u, src.kind)) return rc4;
        small.push_back({mi.vert_base, mi.tri_base, mi.rec_base, mi.n_verts, mi.n_tris, (mi.flags & whitted::kHasNormals) != 0, mi.built[0].meta});
        small_mesh.push_back(u.mesh);
    }
    if (const int rc4 = whitted_refit_small(c, wm, small)) return rc4;
    for (size_t i = 0; i < small.size(); ++i) meshes[small_mesh[i]].built[0].meta = small[i].meta;
    // stage 5
    wm.meshes = std::move(meshes);
    whitted_install_top(wm, std::move(top), depth);
    return RTGO_OK;
}

// rtgo_whitted_update_meshes once the scene is known to exist: every check the host can make (stage 1), then the refits
static int whitted_update_meshes(rtgo_ctx* c, const rtgo_whitted_mesh_update* updates, uint32_t n_updates)
{
    const char* what = "rtgo_whitted_update_meshes";
    const std::string w(what);
    if (n_updates == 0) return RTGO_OK;
    if (!updates) return fail(c, RTGO_E_INVALID, w + ": NULL updates");
    if (const int rc = whitted_check_updates(c, c->wm, w, updates, n_updates)) return rc;
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    return whitted_refit_named(c, what, updates, n_updates, {hipMemcpyHostToDevice, nullptr});
}

// ---- rebuild (rtgo_whitted_rebuild_meshes) --------------------------------------------------------------------------------------------
// What a rebuild replaces of one named mesh in wm's arrays, kept on the device until the call is known to succeed: the mesh's depth and
// box are known only after its build, so a refusal can follow it.  (WhittedClusteredRefit's scheme plus tidx: a build writes it too.)
struct WhittedRebuildSave {
    DeviceArray<float> positions, normals;
    DeviceArray<float4> recs, tris;
    DeviceArray<uint4> qrecs;
    DeviceArray<uint2> tidx;
};

// The builds of rtgo_whitted_rebuild_meshes and rtgo_whitted_update_meshes_device (`what`: the call, for the messages) once every entry
// has passed its checks (stage 1) and the stream has drained: the named meshes built again over new vertices, as rtgo_whitted_set_scene
// (rtgo_whitted_set_mesh) builds them, in place; everything else of the scene stays.  Stages: 2 the named meshes' slices saved, the new
// vertices in (a small mesh's box: from its indices read back, or, vertices on the device, from what whitted_check_on_device reported);
// 3 their structures, all through one table (whitted_build_structures), the cluster table aside; 4 the instances laid out over the new
// boxes and the top level built, aside; 5 what the host keeps.  A refusal in stage 3 or 4 puts the slices back: nothing else has changed
// by then.
static int whitted_rebuild_named(rtgo_ctx* c, const char* what, const rtgo_whitted_mesh_update* updates, uint32_t n_updates, const WhittedUpdateSource& src)
{
    WhittedMesh& wm = c->wm;
    if (const int rc = whitted_refresh_host(c)) return rc;
    std::vector<WhittedMeshInfo> meshes = wm.meshes;
    if (!wm.instanced) {   // a scene of rtgo_whitted_set_mesh: its one mesh, at the start of every array
        WhittedMeshInfo mi = WhittedMeshInfo();
        mi.n_tris = wm.triangles;
        mi.n_verts = wm.n_vertices;
        mi.flags = wm.normals.get() ? whitted::kHasNormals : 0;
        meshes.assign(1, mi);
    }
    // stage 2
    std::vector<WhittedRebuildSave> saved(n_updates);
    std::vector<std::vector<uint32_t>> idx(n_updates);
    std::vector<int> which;
    std::vector<int4> table(wm.clusters.size());
    for (uint32_t k = 0; k < n_updates; ++k) {
        const rtgo_whitted_mesh_update& u = updates[k];
        const WhittedMeshInfo& mi = meshes[u.mesh];
        const size_t n = (size_t)mi.n_tris, nv3 = (size_t)mi.n_verts * 3;
        float* d_pos = wm.positions.get() + 3 * (size_t)mi.vert_base;
        float* d_nrm = wm.normals.get() + 3 * (size_t)mi.vert_base;
        const WhittedBuildTarget t = whitted_target(wm, mi.rec_base, mi.tri_base);   // (a mesh of n triangles owns n record slots)
        WhittedRebuildSave& s = saved[k];
        auto save = [&](auto& keep, const auto* src, size_t count) -> hipError_t {
            const hipError_t e = keep.alloc(count);
            return e != hipSuccess ? e : hipMemcpyAsync(keep.get(), src, count * sizeof *src, hipMemcpyDeviceToDevice, c->stream);
        };
        RTGO_HIP(c, save(s.positions, d_pos, nv3));
        if (u.normals) RTGO_HIP(c, save(s.normals, d_nrm, nv3));
        RTGO_HIP(c, save(s.recs, t.recs, 4 * n));
        RTGO_HIP(c, save(s.tris, t.tris, 3 * n));
        RTGO_HIP(c, save(s.qrecs, t.qrecs, 2 * n));
        RTGO_HIP(c, save(s.tidx, t.tidx, n));
        if (const int rc = whitted_put_vertices(c, wm, mi.vert_base, mi.n_verts, u, src.kind)) return rc;
        if (wm.instanced && !mi.clustered && !src.on_device()) {   // its new box needs its indices, which are on the device only
            idx[k].resize(3 * n);
            RTGO_HIP(c, hipMemcpyAsync(idx[k].data(), wm.indices.get() + 3 * (size_t)mi.tri_base, idx[k].size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        }
        which.push_back((int)u.mesh);
    }
    if (!table.empty()) RTGO_HIP(c, hipMemcpyAsync(table.data(), wm.clusters.get(), table.size() * sizeof(int4), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n_updates; ++k) {
        WhittedMeshInfo& mi = meshes[updates[k].mesh];
        if (!wm.instanced || mi.clustered) continue;
        if (src.on_device()) whitted_pad_mesh_box(src.report[k].lo, src.report[k].hi, mi.lo, mi.hi);
        else whitted_mesh_box(updates[k].positions, idx[k].data(), (uint32_t)mi.n_tris, mi.lo, mi.hi);
    }
    auto refused = [&](int rc) -> int {   // the named meshes' slices as they were
        for (uint32_t k = 0; k < n_updates; ++k) {
            const WhittedMeshInfo& mi = wm.instanced ? wm.meshes[updates[k].mesh] : meshes[0];
            const WhittedBuildTarget t = whitted_target(wm, mi.rec_base, mi.tri_base);
            const WhittedRebuildSave& s = saved[k];
            auto back = [&](auto* dst, const auto& keep) { return hipMemcpyAsync(dst, keep.get(), keep.size() * sizeof *dst, hipMemcpyDeviceToDevice, c->stream); };
            RTGO_HIP(c, back(wm.positions.get() + 3 * (size_t)mi.vert_base, s.positions));
            if (s.normals.get()) RTGO_HIP(c, back(wm.normals.get() + 3 * (size_t)mi.vert_base, s.normals));
            RTGO_HIP(c, back(t.recs, s.recs));
            RTGO_HIP(c, back(t.tris, s.tris));
            RTGO_HIP(c, back(t.qrecs, s.qrecs));
            RTGO_HIP(c, back(t.tidx, s.tidx));
        }
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
        return rc;
    };
    // stage 3
    if (const int rc = whitted_build_structures(c, wm, meshes, which, table, true, what)) return refused(rc);
    if (!wm.instanced) {
        wm.meta = meshes[0].built[0].meta;
        wm.walk_depth = wm.meta.walk_depth < 1 ? 1 : wm.meta.walk_depth;
        return RTGO_OK;
    }
    DeviceArray<int4> clusters;
    if (!table.empty()) RTGO_HIP(c, clusters.upload(table.data(), table.size(), c->stream));
    // stage 4
    int mesh_depth = 0;
    for (const WhittedMeshInfo& mi : meshes) mesh_depth = std::max(mesh_depth, mi.depth);
    std::vector<whitted::InstShade> shade;
    std::vector<float> box_pos;
    WhittedTop top;
    int depth = 0;
    int rc = whitted_prepare_instances(c, meshes, (uint32_t)wm.n_materials, wm.instances.data(), (uint32_t)wm.instances.size(), shade, box_pos, what);
    if (!rc) rc = whitted_make_top_over(c, meshes, mesh_depth, shade, box_pos, wm.instances.data(), what, top, depth);
    if (rc) return refused(rc);
    // stage 5
    wm.meshes = std::move(meshes);
    wm.mesh_depth = mesh_depth;
    if (!table.empty()) wm.clusters = std::move(clusters);
    whitted_install_top(wm, std::move(top), depth);
    return RTGO_OK;
}

// rtgo_whitted_rebuild_meshes once the scene is known to exist: every check the host can make (stage 1), then the builds
static int whitted_rebuild_meshes(rtgo_ctx* c, const rtgo_whitted_mesh_update* updates, uint32_t n_updates)
{
    const char* what = "rtgo_whitted_rebuild_meshes";
    const std::string w(what);
    if (n_updates == 0) return RTGO_OK;
    if (!updates) return fail(c, RTGO_E_INVALID, w + ": NULL updates");
    if (const int rc = whitted_check_updates(c, c->wm, w, updates, n_updates)) return rc;
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    return whitted_rebuild_named(c, what, updates, n_updates, {hipMemcpyHostToDevice, nullptr});
}

// ---- vertices on the device (rtgo_whitted_update_meshes_device) -----------------------------------------------------------------------
// Either of the two above for entries whose positions / normals are device memory, once the scene is known to exist and the flags are
// known.  Stage 1 in two halves: what the host can decide without the data (whitted_check_updates: a NULL or misaligned pointer never
// reaches a launch), then the data where it lies (whitted_check_on_device, which also brings the small meshes' boxes: one copy of 32 B
// per entry, one wait) -- both before anything of the scene is written.  The stages after it are the twins', with the vertices copied
// device to device: nothing in proportion to a mesh's vertices or triangles crosses the host, in either direction.
static int whitted_update_meshes_device(rtgo_ctx* c, const rtgo_whitted_mesh_update* updates, uint32_t n_updates, bool rebuild)
{
    const char* what = "rtgo_whitted_update_meshes_device";
    const std::string w(what);
    if (n_updates == 0) return RTGO_OK;
    if (!updates) return fail(c, RTGO_E_INVALID, w + ": NULL updates");
    if (const int rc = whitted_check_updates(c, c->wm, w, updates, n_updates, true)) return rc;
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<whitted::UpdateReport> report;
    if (const int rc = whitted_check_on_device(c, c->wm, w, updates, n_updates, report)) return rc;
    const WhittedUpdateSource src = {hipMemcpyDeviceToDevice, report.data()};
    return rebuild ? whitted_rebuild_named(c, what, updates, n_updates, src) : whitted_refit_named(c, what, updates, n_updates, src);
}

// ---- instances on the device (rtgo_whitted_set_instances_device) ----------------------------------------------------------------------
// rtgo_whitted_set_instances for instances in device memory (rebuild), or the top level refitted to them in place, once the arguments
// have passed the checks the host can make.  Launches: inst_prepare_kernel (checks, InstShade records, boxes and index triples into
// buffers of the call), the verdict read back -- every refusal but a rebuilt top level's depth is known here, before anything of the
// scene is written -- then whitted_build over the boxes into a top level built aside (rebuild) or refit_kernel over the scene's
// records as the mid-level refit launches it (refit: topology, leaf order and depth stay, so nothing needs saving), then
// inst_gather_kernel for the InstWalk records.  The instances themselves are read back beside the verdict (56 B each): the mesh-update
// calls lay the instances out again from wm.instances.  Nothing else in proportion to n crosses the host.
// What the host decides of the arguments of rtgo_whitted_set_instances_device and rtgo_whitted_refit_instances_device_async (`w`: the
// entry point; c is not NULL), in their order of precedence.  refit: RTGO_UPDATE_REFIT, which keeps the scene's count.
static int whitted_check_instances_args(rtgo_ctx* c, const std::string& w, const void* d_instances, uint32_t n, bool refit)
{
    if (!d_instances) return fail(c, RTGO_E_INVALID, w + ": NULL instance array");
    if (!aligned4(d_instances)) return fail(c, RTGO_E_INVALID, w + ": the instance array is not 4-byte aligned");
    if (!c->wm.instanced) return fail(c, RTGO_E_STATE, w + ": no instanced scene (call rtgo_whitted_set_scene first)");
    if (n == 0 || n > RTGO_WHITTED_MAX_INSTANCES)
        return fail(c, RTGO_E_UNSUPPORTED, w + ": instance count must be in [1, " + std::to_string(RTGO_WHITTED_MAX_INSTANCES) + "]");
    if (refit && n != (uint32_t)c->wm.top.n_instances)
        return fail(c, RTGO_E_INVALID, w + ": a refit takes the scene's " + std::to_string(c->wm.top.n_instances) + " instances");
    return RTGO_OK;
}

// the table inst_prepare_kernel and the gather read of wm's meshes, InstMesh for WhittedMeshInfo
static void whitted_mesh_table(const WhittedMesh& wm, whitted::InstMesh* table)
{
    for (size_t k = 0; k < wm.meshes.size(); ++k) {
        const WhittedMeshInfo& mi = wm.meshes[k];
        table[k] = {{mi.lo[0], mi.lo[1], mi.lo[2]}, {mi.hi[0], mi.hi[1], mi.hi[2]}, mi.rec_base, mi.tri_base, mi.vert_base, mi.root, mi.flags, mi.max_material};
    }
}

static int whitted_set_instances_device(rtgo_ctx* c, const void* d_instances, uint32_t n, bool rebuild)
{
    using namespace whitted;
    const char* what = "rtgo_whitted_set_instances_device";
    const std::string w(what);
    WhittedMesh& wm = c->wm;
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    if (const int rc = whitted_refresh_host(c)) return rc;   // (what this call writes of the host's fields must not be overtaken by an older update's)
    std::vector<InstMesh> table(wm.meshes.size());
    whitted_mesh_table(wm, table.data());
    const unsigned int* d_inst = static_cast<const unsigned int*>(d_instances);
    const unsigned int blocks = (n + 255u) / 256u;
    const int n_recs = wm.top.n_recs;   // (refit)
    DeviceArray<InstMesh> d_table;
    DeviceArray<InstShade> shade;
    DeviceArray<float> boxes;
    DeviceArray<unsigned int> idx;
    DeviceArray<float4> tris;       // rebuild: what the build writes beside the records (the leaf order); refit: the leaf order refit_kernel reads
    DeviceArray<uint4> qrecs;
    if (!c->d_verdict.get()) RTGO_HIP(c, c->d_verdict.alloc(kVerdictWords));
    RTGO_HIP(c, d_table.upload(table.data(), table.size(), c->stream));
    RTGO_HIP(c, shade.alloc(n));
    RTGO_HIP(c, boxes.alloc((size_t)6 * n));
    RTGO_HIP(c, idx.alloc((size_t)3 * n));
    RTGO_HIP(c, tris.alloc((size_t)3 * n));
    RTGO_HIP(c, qrecs.alloc((size_t)2 * n));
    RTGO_HIP(c, hipMemsetAsync(c->d_verdict.get(), 0xFF, kVerdictWords * sizeof(unsigned int), c->stream));
    hipLaunchKernelGGL(inst_prepare_kernel, dim3(blocks), dim3(256), 0, c->stream, d_inst, n, reinterpret_cast<const unsigned int*>(d_table.get()),
                       (unsigned int)table.size(), (unsigned int)wm.n_materials, rebuild ? nullptr : (const InstShade*)wm.top.shade.get(),
                       rebuild ? nullptr : (const InstWalk*)wm.top.inst.get(), shade.get(), boxes.get(), idx.get(), tris.get(), c->d_verdict.get());
    RTGO_HIP(c, hipGetLastError());
    unsigned int v[kVerdictWords];
    std::vector<rtgo_whitted_instance> instances(n);
    RTGO_HIP(c, hipMemcpyAsync(v, c->d_verdict.get(), sizeof v, hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipMemcpyAsync(instances.data(), d_instances, (size_t)n * sizeof(rtgo_whitted_instance), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    static const char* const kFault[kInstVerdictKinds] = {" names a mesh beyond the meshes array", " names another mesh than it names in the scene (a refit keeps the mesh choices)",
                                                          ": material offset + material index beyond the material array",
                                                          " has a non-finite or singular transform", " places its mesh beyond the float range"};
    int kind = -1;
    for (int q = 0; q < kInstVerdictKinds; ++q)
        if (v[q] != kNoFault && (kind < 0 || v[q] < v[kind])) kind = q;
    if (kind >= 0) return fail(c, RTGO_E_INVALID, w + ": instance " + std::to_string(v[kind]) + kFault[kind]);
    if (rebuild) {
        WhittedTop top;
        DeviceArray<uint2> tidx;
        WhittedBuildScratch scratch;
        RTGO_HIP(c, top.recs.alloc((size_t)n * 4));
        RTGO_HIP(c, top.inst.alloc(n));
        RTGO_HIP(c, tidx.alloc(n));
        RTGO_HIP(c, scratch.alloc(n));
        if (const int rc = whitted_build(c, boxes.get(), idx.get(), (int)n, {top.recs.get(), tris.get(), qrecs.get(), tidx.get()}, scratch, top.meta, what)) return rc;
        const int depth = (top.meta.n_recs > 0 ? top.meta.walk_depth : 0) + wm.mesh_depth;
        if (depth > kMaxInstWalkDepth)
            return fail(c, RTGO_E_UNSUPPORTED, w + ": the two-level walk needs " + std::to_string(depth) + " stack entries (limit " + std::to_string(kMaxInstWalkDepth) + ")");
        hipLaunchKernelGGL(inst_gather_kernel, dim3(blocks), dim3(256), 0, c->stream, (const float4*)tris.get(), (const InstShade*)shade.get(), d_inst,
                           (const InstMesh*)d_table.get(), n, top.inst.get());
        RTGO_HIP(c, hipGetLastError());
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
        top.shade = std::move(shade);
        top.n_recs = top.meta.n_recs;
        top.n_instances = (int)n;
        wm.instances = std::move(instances);
        whitted_install_top(wm, std::move(top), depth);
        return RTGO_OK;
    }
    // refit: a top level of one leaf has no records, only the two arrays change
    DeviceArray<int> done;
    DeviceArray<WhittedBuildMeta> d_meta;
    v3 grid[2];
    if (n_recs > 0) {
        RTGO_HIP(c, done.alloc((size_t)n_recs));
        RTGO_HIP(c, d_meta.alloc(1));
        hipLaunchKernelGGL(refit_kernel, dim3(1), dim3(kBuildThreads), 0, c->stream, (const float*)boxes.get(), (const unsigned int*)idx.get(), (int)n, n_recs,
                           wm.top.meta.walk_depth, wm.top.recs.get(), tris.get(), qrecs.get(), done.get(), d_meta.get());
        RTGO_HIP(c, hipGetLastError());
        RTGO_HIP(c, hipMemcpyAsync(grid, &d_meta.get()->grid_lo, sizeof grid, hipMemcpyDeviceToHost, c->stream));
    }
    hipLaunchKernelGGL(inst_gather_kernel, dim3(blocks), dim3(256), 0, c->stream, (const float4*)nullptr, (const InstShade*)shade.get(), d_inst,
                       (const InstMesh*)d_table.get(), n, wm.top.inst.get());
    RTGO_HIP(c, hipGetLastError());
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    if (n_recs > 0) {
        wm.top.meta.grid_lo = grid[0];
        wm.top.meta.grid_step = grid[1];
    }
    wm.top.shade = std::move(shade);
    wm.instances = std::move(instances);
    return RTGO_OK;
}

// ---- the refit that waits for nothing on the host (rtgo_whitted_refit_instances_device_async) ---------------------------
// The refit above once the arguments have passed whitted_check_instances_args, enqueued: a slot of the context's ring, then
// inst_prepare_kernel into the scene's staging with its verdict in the slot, the verdict's copy and the slot's event, then the gated
// kernels -- inst_commit_kernel, and for a top level with records inst_refit_gated_kernel -- every time: the verdict is not known here.
// Nothing is read back; wm.instances and wm.top.meta's grid are marked stale instead (whitted_refresh_host).  A context's first call
// allocates the ring, a scene's first call the staging; no other call allocates, frees or waits (but a 65th update in flight, once).
static int whitted_refit_instances_async(rtgo_ctx* c, const void* d_instances, uint32_t n, uint64_t* ticket)
{
    using namespace whitted;
    WhittedMesh& wm = c->wm;
    WhittedInstStaging& st = wm.staging;
    RTGO_HIP(c, hipSetDevice(c->device));
    rtgo_ctx::UpdateRing& ring = c->w_updates;
    const size_t slots = rtgo_ctx::UpdateRing::kSlots;
    if (!ring.d.get()) {
        RTGO_HIP(c, ring.d.alloc(slots * kVerdictWords));
        RTGO_HIP(c, ring.h.alloc(slots * kVerdictWords));
        for (size_t s = 0; s < slots; ++s)
            if (!ring.done[s].get()) RTGO_HIP(c, ring.done[s].create(hipEventDisableTiming));
    }
    const int n_recs = wm.top.n_recs;
    if (!st.shade.get()) {
        st = WhittedInstStaging();
        RTGO_HIP(c, st.boxes.alloc((size_t)6 * n));
        RTGO_HIP(c, st.idx.alloc((size_t)3 * n));
        RTGO_HIP(c, st.tris.alloc((size_t)3 * n));
        RTGO_HIP(c, st.qrecs.alloc((size_t)2 * n));
        RTGO_HIP(c, st.done.alloc((size_t)std::max(n_recs, 1)));
        RTGO_HIP(c, st.words.alloc(WhittedInstStaging::kWords));
        RTGO_HIP(c, st.kept.alloc((size_t)kInstDwords * n));
        RTGO_HIP(c, st.table.alloc((size_t)kMaxMeshes * kInstMeshDwords));
        RTGO_HIP(c, st.h_table.alloc((size_t)kMaxMeshes * kInstMeshDwords));
        RTGO_HIP(c, hipMemsetAsync(st.words.get(), 0, WhittedInstStaging::kWords * sizeof(unsigned int), c->stream));
        RTGO_HIP(c, st.shade.alloc(n));   // (last: what says the staging is there)
    }
    // the mesh table, up again only when the meshes have changed under it (in a call that drained the stream: no copy of the image is in flight)
    InstMesh table[kMaxMeshes];
    const size_t n_meshes = wm.meshes.size(), table_words = n_meshes * kInstMeshDwords;
    whitted_mesh_table(wm, table);
    if (st.table_words != table_words || std::memcmp(st.h_table.get(), table, table_words * sizeof(unsigned int)) != 0) {
        std::memcpy(st.h_table.get(), table, table_words * sizeof(unsigned int));
        RTGO_HIP(c, hipMemcpyAsync(st.table.get(), st.h_table.get(), table_words * sizeof(unsigned int), hipMemcpyHostToDevice, c->stream));
        st.table_words = table_words;
    }
    const uint64_t t = ring.next;
    const unsigned int slot = rtgo_ctx::UpdateRing::slot(t);
    // the slot's last ticket leaves the ring; a ring full of updates in flight waits here for the oldest, as timed_launch's does
    if (ring.next_reuses_a_slot()) RTGO_HIP(c, hipEventSynchronize(ring.done[slot].get()));
    unsigned int* d_verdict = ring.d.get() + (size_t)slot * kVerdictWords;
    const unsigned int* d_inst = static_cast<const unsigned int*>(d_instances);
    const unsigned int blocks = (n + 255u) / 256u;
    unsigned int* d_applied = st.words.get() + WhittedInstStaging::kMetaWords;
    RTGO_HIP(c, hipMemsetAsync(d_verdict, 0xFF, kVerdictWords * sizeof(unsigned int), c->stream));
    hipLaunchKernelGGL(inst_prepare_kernel, dim3(blocks), dim3(256), 0, c->stream, d_inst, n, (const unsigned int*)st.table.get(), (unsigned int)n_meshes,
                       (unsigned int)wm.n_materials, (const InstShade*)wm.top.shade.get(), (const InstWalk*)wm.top.inst.get(), st.shade.get(), st.boxes.get(),
                       st.idx.get(), st.tris.get(), d_verdict);
    RTGO_HIP(c, hipGetLastError());
    RTGO_HIP(c, hipMemcpyAsync(ring.h.get() + (size_t)slot * kVerdictWords, d_verdict, kVerdictWords * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipEventRecord(ring.done[slot].get(), c->stream));
    hipLaunchKernelGGL(inst_commit_kernel, dim3(blocks), dim3(256), 0, c->stream, (const unsigned int*)d_verdict, d_inst, (const InstShade*)st.shade.get(),
                       reinterpret_cast<const InstMesh*>(st.table.get()), n, wm.top.shade.get(), wm.top.inst.get(), st.kept.get(), d_applied);
    if (n_recs > 0)
        hipLaunchKernelGGL(inst_refit_gated_kernel, dim3(1), dim3(kBuildThreads), 0, c->stream, (const unsigned int*)d_verdict, (const float*)st.boxes.get(),
                           (const unsigned int*)st.idx.get(), (int)n, n_recs, wm.top.meta.walk_depth, wm.top.recs.get(), st.tris.get(), st.qrecs.get(), st.done.get(),
                           reinterpret_cast<WhittedBuildMeta*>(st.words.get()));
    RTGO_HIP(c, hipGetLastError());
    st.stale = true;
    ring.next = t + 1;
    *ticket = t;
    return RTGO_OK;
}

// The launches.  What a launch over one mesh (rtgo_whitted_set_mesh) reads of the scene: everything of Params but the frame
static whitted::Params mesh_params(const WhittedMesh& wm)
{
    whitted::Params p;
    std::memset(&p, 0, sizeof p);
    p.recs = wm.recs.get();
    p.tris = wm.tris.get();
    p.qrecs = wm.qrecs.get();
    p.tidx = wm.tidx.get();
    p.n_vertices = wm.n_vertices;
    p.grid_lo = wm.meta.grid_lo;
    p.grid_step = wm.meta.grid_step;
    p.n_recs = wm.meta.n_recs;
    p.n_triangles = wm.triangles;
    p.positions = wm.positions.get();
    p.normals = wm.normals.get();
    p.indices = wm.indices.get();
    p.tri_material = wm.tri_material.get();
    p.texcoords = wm.texcoords.get();
    return p;
}

// ... and over an instanced scene (rtgo_whitted_set_scene): everything of InstParams but the frame
static whitted::InstParams inst_params(const WhittedMesh& wm)
{
    whitted::InstParams q;
    std::memset(&q, 0, sizeof q);
    q.top_recs = wm.top.recs.get();
    q.inst = wm.top.inst.get();
    q.shade = wm.top.shade.get();
    q.n_top_recs = wm.top.n_recs;
    q.n_instances = wm.top.n_instances;
    q.recs = wm.recs.get();
    q.tris = wm.tris.get();
    q.clusters = wm.clusters.get();
    q.positions = wm.positions.get();
    q.normals = wm.normals.get();
    q.texcoords = wm.texcoords.get();
    q.indices = wm.indices.get();
    q.tri_material = wm.tri_material.get();
    return q;
}

// The launch of the context's scene.  One mesh: beside the lanes' stacks (stack_bytes), its LDS holds as much of the structure as fits --
// everything in its compact form (quantised records, vertices, 16-bit vertex indices), or the fp32 records alone, or nothing.  An instanced
// scene: the top level's records and InstWalk array when they fit (and RTGO_WHITTED_MODE allows); the meshes are read through L2.
template <bool FRAMES>
static void whitted_enqueue_kernels(rtgo_ctx* c, const whitted::Frame& fr, size_t stack_bytes, int mode_cap, unsigned int blocks)
{
    const dim3 grid(blocks), block(whitted::kRenderBlock);
    if (!c->wm.instanced) {
        whitted::Params p = mesh_params(c->wm);
        p.frame = fr;
        const size_t rec_bytes = (size_t)p.n_recs * 4 * sizeof(float4);
        const size_t compact_bytes = (size_t)p.n_recs * 2 * sizeof(uint4) + (size_t)p.n_vertices * sizeof(float4) + (size_t)p.n_triangles * sizeof(uint2);
        if (mode_cap >= whitted::kAllInLds && p.n_vertices <= 65535 && compact_bytes + stack_bytes <= whitted::kRenderLds)
            hipLaunchKernelGGL((whitted::render_kernel<whitted::kAllInLds, FRAMES>), grid, block, compact_bytes + stack_bytes, c->stream, p);
        else if (mode_cap >= whitted::kRecordsInLds && rec_bytes + stack_bytes <= whitted::kRenderLds)
            hipLaunchKernelGGL((whitted::render_kernel<whitted::kRecordsInLds, FRAMES>), grid, block, rec_bytes + stack_bytes, c->stream, p);
        else
            hipLaunchKernelGGL((whitted::render_kernel<whitted::kAllInL2, FRAMES>), grid, block, stack_bytes, c->stream, p);
    } else {
        whitted::InstParams q = inst_params(c->wm);
        q.frame = fr;
        const size_t top_bytes = (size_t)q.n_top_recs * 4 * sizeof(float4) + (size_t)q.n_instances * sizeof(whitted::InstWalk);
        const bool in_lds = mode_cap >= whitted::kRecordsInLds && top_bytes + stack_bytes <= whitted::kRenderLds;
        const size_t lds = stack_bytes + (in_lds ? top_bytes : 0);
        if (q.clusters) {   // a clustered mesh in the scene: the three-level walk
            if (in_lds) hipLaunchKernelGGL((whitted::render_inst_kernel<true, true, FRAMES>), grid, block, lds, c->stream, q);
            else hipLaunchKernelGGL((whitted::render_inst_kernel<false, true, FRAMES>), grid, block, lds, c->stream, q);
        } else if (in_lds)
            hipLaunchKernelGGL((whitted::render_inst_kernel<true, false, FRAMES>), grid, block, lds, c->stream, q);
        else
            hipLaunchKernelGGL((whitted::render_inst_kernel<false, false, FRAMES>), grid, block, lds, c->stream, q);
    }
}

// frames: the launch of rtgo_whitted_launch_frames (fr.n_subframes subframes, the FRAMES instantiation of the same kernel)
static int whitted_enqueue(rtgo_ctx* c, const whitted::Frame& fr, size_t stack_bytes, int mode_cap, unsigned int blocks, bool frames)
{
    if (frames) whitted_enqueue_kernels<true>(c, fr, stack_bytes, mode_cap, blocks);
    else whitted_enqueue_kernels<false>(c, fr, stack_bytes, mode_cap, blocks);
    RTGO_HIP(c, hipGetLastError());
    return RTGO_OK;
}
