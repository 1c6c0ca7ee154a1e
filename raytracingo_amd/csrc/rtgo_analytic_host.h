// rtgo_analytic_host.h -- host side of the analytic scene: what the rtgo_set_*scene* and rtgo_update_prims* entry points of rtgo_capi.hip
// call once they have checked their arguments (no exported symbol lives here).  A scene of rtgo_set_scene first, then one of rtgo_set_large_scene,
// the edits in place and what the device-pointer calls add.  Included below Knobs and kBuildDynLds, which the launches read too.
#pragma once

#include "rtgo_ctx.h"

// The uniform grid of rtgo::fast_grid over structure 0's small primitives (fprims [0, n_small)), from the boxes the fast walk culls
// with (scene.tight: build_kernel's, SBT order).  Every box is grown by `pad` before it is binned, and fast_grid stops `pad / 2` (in t)
// late: the walk's own rounding (entry point, 96 accumulated steps: <= ~2e-5 of the rays' reach) stays an order of magnitude inside.
// Cells: <= 32 per axis; table, cell records and lists within 40 KB of LDS; no grid for fewer than 64 small primitives (RTGO_GRID_MIN) or when
// every resolution with at least half as many cells as primitives lists more than 3 entries per primitive (RTGO_GRID_MAX_DUP; a few big shapes among small ones: the tree's job).
static int build_grid(rtgo_ctx* c, uint32_t n, const Knobs& kn)
{
    AnalyticScene& sc = c->scene;
    sc.grid.have = false;
    const int ns = sc.tree[0].n_small;
    if (ns < (int)kn.grid_min) return RTGO_OK;
    std::vector<float4> fp((size_t)n * 4);
    RTGO_HIP(c, hipMemcpyAsync(fp.data(), sc.tree[0].d_fprims.get(), fp.size() * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<const float*> box((size_t)ns);
    float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f}, scene_reach = 0.0f;
    for (int pos = 0; pos < ns; ++pos) {
        int orig;
        std::memcpy(&orig, &fp[4 * (size_t)pos + 3].y, sizeof orig);
        if (orig < 0 || orig >= (int)n) return fail(c, RTGO_E_UNSUPPORTED, "rtgo_set_scene: fast-walk record without a primitive");
        box[pos] = &sc.tight[6 * (size_t)orig];
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::fmin(lo[a], box[pos][a]);
            hi[a] = std::fmax(hi[a], box[pos][3 + a]);
        }
    }
    for (int a = 0; a < 6; ++a) scene_reach = std::fmax(scene_reach, std::fabs(sc.bounds[a]));
    const float reach_max = 4.0f * scene_reach;
    float ext[3], max_ext = 0.0f;
    for (int a = 0; a < 3; ++a) {
        ext[a] = hi[a] - lo[a];
        max_ext = std::fmax(max_ext, ext[a]);
    }
    if (!(max_ext > 0.0f)) return RTGO_OK;
    // Resolution: the (nx, ny, nz) that minimises the classic cost of a grid walk -- a ray meets cells in proportion to their surface
    // area, pays one step per cell and one test per list entry: cost = A_cell (n_cells + kTest entries) -- over every resolution
    // up to 32 per axis, with the entries counted exactly (a primitive's span of cells is separable per axis).  The entries term is what
    // matters: a resolution that cuts through the shapes lists them two to eight times (balls, profiles/r03r: 16 x 4 x 16, one sphere per
    // column, 321 entries, 10.1 ms; 13 x 6 x 13, 754 entries, 13.8 ms; 32 x 1 x 32, 1024 entries, 19.1 ms; the tree 13.5).  kTest: 1.7 fitted there; 1.0 since the walk tests a cell's box before its list (16 x 3 x 16, 9.7 ms).
    constexpr float kTest = 1.0f;
    const float max_dup = kn.grid_max_dup;
    const float pad0 = 2e-3f * (max_ext / 8.0f) + 1e-4f * reach_max;   // (the pad of the binning below depends on the cell size: close enough for counting)
    std::vector<uint8_t> span[3];
    for (int a = 0; a < 3; ++a) {
        span[a].assign((size_t)33 * ns, 1);
        for (int m = 1; m <= 32; ++m) {
            const float g0 = lo[a] - 2.0f * pad0, ics = (float)m / (ext[a] + 4.0f * pad0);
            for (int pos = 0; pos < ns; ++pos) {
                int c0 = (int)std::floor((box[pos][a] - pad0 - g0) * ics), c1 = (int)std::floor((box[pos][3 + a] + pad0 - g0) * ics);
                c0 = c0 < 0 ? 0 : c0;
                c1 = c1 > m - 1 ? m - 1 : c1;
                span[a][(size_t)m * ns + pos] = (uint8_t)(c1 - c0 + 1);
            }
        }
    }
    int dim[3] = {1, 1, 1};
    double best_cost = 1e300;
    std::vector<uint32_t> sxy((size_t)ns);
    for (int mx = 1; mx <= 32; ++mx)
        for (int my = 1; my <= 32; ++my) {
            if ((mx + 2) * (my + 2) * 3 * 4 > 32 * 1024) continue;
            for (int pos = 0; pos < ns; ++pos) sxy[pos] = (uint32_t)span[0][(size_t)mx * ns + pos] * span[1][(size_t)my * ns + pos];
            for (int mz = 1; mz <= 32; ++mz) {
                const size_t words = (size_t)(mx + 2) * (my + 2) * (mz + 2);
                if (words * 4 > 30 * 1024) break;
                size_t entries = 0;
                const uint8_t* sz = &span[2][(size_t)mz * ns];
                for (int pos = 0; pos < ns; ++pos) entries += (size_t)sxy[pos] * sz[pos];
                const size_t listing = entries < (size_t)mx * my * mz ? entries : (size_t)mx * my * mz;   // (at most this many cells carry a record)
                if ((float)entries > max_dup * (float)ns || words * 4 + listing * 32 + entries * 2 > 38 * 1024) continue;
                if (2 * mx * my * mz < ns) continue;   // (fewer cells than half the primitives: lists, not a grid)
                const double cx = (ext[0] + 4.0 * pad0) / mx, cy = (ext[1] + 4.0 * pad0) / my, cz = (ext[2] + 4.0 * pad0) / mz;
                const double cost = 2.0 * (cx * cy + cy * cz + cx * cz) * ((double)mx * my * mz + (double)kTest * (double)entries);
                if (cost < best_cost) {
                    best_cost = cost;
                    dim[0] = mx; dim[1] = my; dim[2] = mz;
                }
            }
        }
    if (best_cost >= 1e300) return RTGO_OK;
    if (kn.grid_dims[0])   // (experiments)
        for (int a = 0; a < 3; ++a) dim[a] = kn.grid_dims[a];
    rtgo::GridParams g = {};
    float max_cs = 0.0f;
    for (int a = 0; a < 3; ++a) max_cs = std::fmax(max_cs, ext[a] / (float)dim[a]);
    const float pad = 2e-3f * max_cs + 1e-4f * reach_max;
    float gmin[3], gcs[3], gics[3];
    for (int a = 0; a < 3; ++a) {
        gmin[a] = lo[a] - 2.0f * pad;
        gcs[a] = (ext[a] + 4.0f * pad) / (float)dim[a];
        gics[a] = 1.0f / gcs[a];
    }
    g.min_x = gmin[0]; g.min_y = gmin[1]; g.min_z = gmin[2];
    g.cs_x = gcs[0]; g.cs_y = gcs[1]; g.cs_z = gcs[2];
    g.ics_x = gics[0]; g.ics_y = gics[1]; g.ics_z = gics[2];
    g.nx = dim[0]; g.ny = dim[1]; g.nz = dim[2];
    // the table carries a border of empty cells (fast_grid steps into it when it leaves the grid)
    const int NX = dim[0] + 2, NY = dim[1] + 2, NZ = dim[2] + 2;
    g.n_cells = NX * NY * NZ;
    g.margin = 0.5f * pad;
    std::vector<std::vector<uint16_t>> lists((size_t)g.n_cells);
    size_t total = 0;
    for (int pos = 0; pos < ns; ++pos) {
        int a0[3], a1[3];
        for (int a = 0; a < 3; ++a) {
            a0[a] = (int)std::floor((box[pos][a] - pad - gmin[a]) * gics[a]);
            a1[a] = (int)std::floor((box[pos][3 + a] + pad - gmin[a]) * gics[a]);
            a0[a] = a0[a] < 0 ? 0 : a0[a];
            a1[a] = a1[a] > dim[a] - 1 ? dim[a] - 1 : a1[a];
        }
        for (int z = a0[2]; z <= a1[2]; ++z)
            for (int y = a0[1]; y <= a1[1]; ++y)
                for (int x = a0[0]; x <= a1[0]; ++x) {
                    lists[((size_t)(z + 1) * NY + (y + 1)) * NX + (x + 1)].push_back((uint16_t)pos);
                    ++total;
                }
    }
    if ((float)total > (max_dup + 0.5f) * (float)ns || total > 60000) return RTGO_OK;   // (the binning's pad is a little larger than the count's)
    // image: [table, one word per cell][records, 2 float4 per listing cell][items, 16 bit each], each part on a 16-byte boundary
    size_t n_rec = 0;
    for (const std::vector<uint16_t>& l : lists) n_rec += l.empty() ? 0 : 1;
    const size_t table_bytes = ((size_t)g.n_cells * 4 + 15) / 16 * 16, rec_bytes = n_rec * 32;
    const size_t bytes = (table_bytes + rec_bytes + total * 2 + 31) / 32 * 32;
    if (bytes > 40 * 1024) return RTGO_OK;
    g.rec_off4 = (int)(table_bytes / 16);
    g.items_off4 = (int)((table_bytes + rec_bytes) / 16);
    std::vector<unsigned char> img(bytes, 0);
    uint32_t* cells = reinterpret_cast<uint32_t*>(img.data());
    float* recs = reinterpret_cast<float*>(img.data() + table_bytes);
    uint16_t* items = reinterpret_cast<uint16_t*>(img.data() + table_bytes + rec_bytes);
    size_t at = 0, rec = 0;
    for (int k = 0; k < g.n_cells; ++k) {
        const std::vector<uint16_t>& l = lists[(size_t)k];
        if (l.empty()) continue;
        cells[k] = (uint32_t)(rec + 1);
        float* q = recs + 8 * rec;
        for (int a = 0; a < 3; ++a) {
            q[a] = 1e30f;
            q[4 + a] = -1e30f;
        }
        for (uint16_t v : l) {
            for (int a = 0; a < 3; ++a) {   // the box around what the cell lists: the shapes' own boxes grown by the pad ...
                q[a] = std::fmin(q[a], box[v][a] - pad);
                q[4 + a] = std::fmax(q[4 + a], box[v][3 + a] + pad);
            }
            items[at++] = v;
        }
        {   // ... cut to the cell, itself grown by the pad: a hit point lies (within the walk's rounding) in a cell the walk visits, that
            // cell lists the shape, and the point is inside this box of it -- so the test happens there at the latest
            const int kx = k % NX - 1, ky = (k / NX) % NY - 1, kz = k / (NX * NY) - 1;
            const int kk[3] = {kx, ky, kz};
            for (int a = 0; a < 3; ++a) {
                q[a] = std::fmax(q[a], gmin[a] + gcs[a] * (float)kk[a] - pad);
                q[4 + a] = std::fmin(q[4 + a], gmin[a] + gcs[a] * (float)(kk[a] + 1) + pad);
            }
        }
        const uint32_t fc = (uint32_t)(at - l.size()) | ((uint32_t)l.size() << 16);
        std::memcpy(&q[3], &fc, 4);
        q[7] = 0.0f;
        ++rec;
    }
    RTGO_HIP(c, sc.grid.d.upload(img.data(), bytes, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    sc.grid.n_nodes = (int)(bytes / 32);
    sc.grid.entries = (int)total;
    sc.grid.gp = g;
    sc.grid.reach_max = reach_max;
    sc.grid.have = true;
    if (kn.debug)
        std::fprintf(stderr, "rtgo_set_scene: grid %d x %d x %d over %d primitives, %zu list entries, %zu bytes, pad %g, for rays within %g\n", dim[0], dim[1], dim[2], ns,
                     total, bytes, pad, reach_max);
    return RTGO_OK;
}

// build_kernel for one big_frac into a structure of its own (the canonical LBVH, boxes and frames it also writes are the same for every
// big_frac), and its meta words decoded
static int build_fast_tree(rtgo_ctx* c, uint32_t n, int have_aabbs, float big_frac, const Knobs& kn, AnalyticScene::FastTree& t, BuildMeta& meta)
{
    AnalyticScene& sc = c->scene;
    RTGO_HIP(c, t.d_fnodes.alloc((2 * n - 1) * 2));
    RTGO_HIP(c, t.d_fprims.alloc(n * 4));
    hipLaunchKernelGGL(build_kernel, dim3(1), dim3(kMaxPrims), kBuildDynLds, c->stream, sc.d_prims_in.get(), sc.d_aabb.get(), have_aabbs, (int)n,
                       sc.d_nodes.get(), sc.d_prims.get(), t.d_fnodes.get(), t.d_fprims.get(), c->leaf_budget, big_frac, reinterpret_cast<BuildMeta*>(c->d_meta.get()), sc.d_tight.get(),
                       kn.no_cuboid ? 0 : 1, sc.d_frames.get());
    RTGO_HIP(c, hipGetLastError());
    RTGO_HIP(c, hipMemcpyAsync(&meta, c->d_meta.get(), sizeof meta, hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    t.meta = meta;
    t.fast_depth = meta.walk_depth;
    t.n_small = meta.n_small;
    t.n_big_pairs = group_pairs(meta.list_group);
    t.list_cub = group_cert(meta.list_group) & 3;
    t.slab_list = (group_cert(meta.list_group) & kSlabBit) != 0;
    t.slab_leaves = 0;
    t.cuboid_groups = meta.cuboid_leaves + (t.list_cub ? 1 : 0);
    t.tree_spheres = (t.n_small > 0 && meta.tree_types == (1 << 3)) ? 1 : 0;   // (type 3 = sphere)
    t.cub_a = meta.cub_a;
    t.cub_b = meta.cub_b;
    t.n_fnodes = meta.n_fnodes;
    // fast_pair's shape: three nodes, the root's links 1 and 2, both of them leaves certified as cuboids, the root's box the union of theirs
    t.pair = false;
    // (the pair kernels take the two counts as compile-time values: kPairNodes, kPairSmall)
    if (meta.n_small == kPairSmall && meta.n_fnodes == kPairNodes && meta.cuboid_leaves == 2) {
        float4 nd[6];
        RTGO_HIP(c, hipMemcpyAsync(nd, t.d_fnodes.get(), sizeof nd, hipMemcpyDeviceToHost, c->stream));
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
        auto link = [&](int k) { int v; std::memcpy(&v, &nd[k].w, sizeof v); return v; };
        auto cuboid = [&](int node) { const int r = link(2 * node + 1); return link(2 * node) >= 0 && r < 0 && leaf_cuboid(r) != 0 && leaf_count(r) == 6; };
        const bool boxed = nd[0].x == std::fmin(nd[2].x, nd[4].x) && nd[0].y == std::fmin(nd[2].y, nd[4].y) && nd[0].z == std::fmin(nd[2].z, nd[4].z) &&
                           nd[1].x == std::fmax(nd[3].x, nd[5].x) && nd[1].y == std::fmax(nd[3].y, nd[5].y) && nd[1].z == std::fmax(nd[3].z, nd[5].z);
        t.pair = link(0) == 1 && link(1) == 2 && cuboid(1) && cuboid(2) && boxed;
        // (which of the pair kernels' two leaves also hold the slab certificate: bit 0 node 1, bit 1 node 2)
        if (t.pair) t.slab_leaves = ((leaf_cuboid(link(3)) & kSlabBit) ? 1 : 0) | ((leaf_cuboid(link(5)) & kSlabBit) ? 2 : 0);
    }
    // the world-axis form of the list's room (render_roomw_kernel): from the group's six records, read back here, once per build
    t.room_world = rtgo::RoomWorld();
    if (t.pair && t.slab_list && t.list_cub == 2 && (uint32_t)meta.n_small + 6u <= n) {
        float rec[6][16];
        RTGO_HIP(c, hipMemcpyAsync(rec, t.d_fprims.get() + 4 * (size_t)meta.n_small, sizeof rec, hipMemcpyDeviceToHost, c->stream));
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
        room_world_certify(rec, true, true, t.room_world);
    }
    return RTGO_OK;
}

// The scene half of the last-ray certificate (render_kernel: a path's last ray tests the emitters first and skips the up-front list; DESIGN.md
// 3.2).  It holds when the up-front list is a certified room followed by nothing but the scene's emitters (material Le.x > 0.01, the
// kernel's test), all of them rectangles, at most kMaxEmitters.  For each (emitter e, wall g) it records how far inside g's plane
// e lies -- the least y_g over e's corners, e taken as the exact rectangle its fprims rows describe (their inverse, in double) -- and
// the margin's coefficients.  Why the margin suffices: a wall is hit only where the ray approaches it (d.y_g < 0) from its inner side
// (o.y_g > 0); y_g falls along the ray, so if y_g > 0 at the emitter's hit point P = o + t_e d the wall's t_w = -o.y_g / d.y_g is
// beyond t_e and the wall cannot be the closest hit.  y_g(P) >= ymin - L * err_e, where err_e is how far the reference's test lets P
// sit outside e (its u, v, and the plane offset o.y_e + t_e d.y_e, in e's object units) and L carries e's object units into y_g's
// (ymax - ymin over the corners: the in-plane part, + |r1_g . e's y axis|).  The kernel's t_w > t_e then needs y_g(P) to exceed the
// rounding of o.y_g, d.y_g and the quotient.  Each is a few float operations on terms <= |row|_1 (|o| + t |d|) + |w| <= |row|_1 3 R
// + |w| (R: the launch's reach, as for cub_mu), <= 12 * 2^-24 of them; K = 64 * 2^-24 leaves five times that.  So the margin is
// K (A R + B) with A = 3 (L max|row_e|_1 + |r1_g|_1), B = L (max|w_e| + 1) + |w_g| (the 1: u = px + 0.5 is rounded at 1's scale).
static int emitter_cert(rtgo_ctx* c, const rtgo_prim* prims, uint32_t n, AnalyticScene::FastTree& t)
{
    t.emit_n = 0;
    if (t.list_cub != 2) return RTGO_OK;
    std::vector<float4> fp((size_t)n * 4);
    RTGO_HIP(c, hipMemcpyAsync(fp.data(), t.d_fprims.get(), fp.size() * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    auto orig_at = [&](int pos) { int o; std::memcpy(&o, &fp[4 * pos + 3].y, 4); return o; };
    auto type_at = [&](int pos) { int o; std::memcpy(&o, &fp[4 * pos + 3].x, 4); return o; };
    uint32_t emitters = 0;
    for (uint32_t i = 0; i < n; ++i) emitters += prims[i].Le[0] > 0.01f ? 1u : 0u;
    const int first = t.n_small + 6;
    if (emitters == 0 || emitters > (uint32_t)kMaxEmitters || (int)n - first != (int)emitters) return RTGO_OK;
    for (int k = 0; k < (int)emitters; ++k) {
        const int o = orig_at(first + k);
        if (o < 0 || o >= (int)n || !(prims[o].Le[0] > 0.01f) || type_at(first + k) != (int)RTGO_RECTANGLE) return RTGO_OK;
    }
    auto n1 = [](const float4& r) { return std::fabs((double)r.x) + std::fabs((double)r.y) + std::fabs((double)r.z); };
    for (int e = 0; e < (int)emitters; ++e) {
        const float4* R = &fp[4 * (first + e)];
        // M = the inverse of the rows' 3x3 part: world = M (obj - w)
        const double a[3][3] = {{R[0].x, R[0].y, R[0].z}, {R[1].x, R[1].y, R[1].z}, {R[2].x, R[2].y, R[2].z}};
        const double w[3] = {R[0].w, R[1].w, R[2].w};
        double M[3][3];
        const double det = mat3_det_inverse(a, M);
        if (!(std::fabs(det) > 1e-300) || !std::isfinite(det)) return RTGO_OK;
        const double n1e = std::max(n1(R[0]), std::max(n1(R[1]), n1(R[2])));
        const double we = std::max(std::fabs(w[0]), std::max(std::fabs(w[1]), std::fabs(w[2]))) + 1.0;
        for (int g = 0; g < 6; ++g) {
            const float4 r1 = fp[4 * (t.n_small + g) + 1];
            const double rg[3] = {r1.x, r1.y, r1.z};
            double ymin = INFINITY, ymax = -INFINITY;
            for (int k = 0; k < 4; ++k) {
                const double ob[3] = {((k & 1) ? 0.5 : -0.5) - w[0], 0.0 - w[1], ((k & 2) ? 0.5 : -0.5) - w[2]};
                double y = r1.w;
                for (int i = 0; i < 3; ++i) y += rg[i] * (M[i][0] * ob[0] + M[i][1] * ob[1] + M[i][2] * ob[2]);
                ymin = std::min(ymin, y);
                ymax = std::max(ymax, y);
            }
            const double L = (ymax - ymin) + std::fabs(rg[0] * M[0][1] + rg[1] * M[1][1] + rg[2] * M[2][1]);
            const double A = 3.0 * (L * n1e + n1(r1)), B = L * we + std::fabs((double)r1.w);
            if (!(std::isfinite(ymin) && A < 1e30 && B < 1e30)) return RTGO_OK;
            t.emit_ymin[6 * e + g] = (float)ymin;
            t.emit_a[6 * e + g] = (float)A;
            t.emit_b[6 * e + g] = (float)B;
        }
    }
    t.emit_n = (int)emitters;
    return RTGO_OK;
}

// the per-primitive checks of rtgo_set_scene and rtgo_set_large_scene (`what`: the entry point, for the message)
static int check_prims(rtgo_ctx* c, const rtgo_prim* prims, const rtgo_aabb* aabbs, uint32_t n, const std::string& what)
{
    for (uint32_t i = 0; i < n; ++i) {
        const rtgo_prim& q = prims[i];
        if (q.type > RTGO_SPHERE) return fail(c, RTGO_E_INVALID, what + ": unknown primitive type");
        // the intersection programs work in object space through M^-1 (kernel.cu:125-135): M must be finite and invertible
        bool finite = std::isfinite(q.specularity);
        for (int k = 0; k < 16; ++k) finite = finite && std::isfinite(q.model[k]);
        for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(q.kd[k]) && std::isfinite(q.kr[k]) && std::isfinite(q.Le[k]);
        const double a[3][3] = {{q.model[0], q.model[1], q.model[2]}, {q.model[4], q.model[5], q.model[6]}, {q.model[8], q.model[9], q.model[10]}};
        const double det = mat3_det_inverse(a);
        if (!finite || !std::isfinite(det) || std::fabs(det) < 1e-30)
            return fail(c, RTGO_E_INVALID, what + ": primitive " + std::to_string(i) + " has a non-finite or singular model matrix / material");
        if (aabbs) {
            const rtgo_aabb& bb = aabbs[i];
            if (!(bb.minX <= bb.maxX && bb.minY <= bb.maxY && bb.minZ <= bb.maxZ) || !std::isfinite(bb.minX + bb.minY + bb.minZ + bb.maxX + bb.maxY + bb.maxZ))
                return fail(c, RTGO_E_INVALID, what + ": box " + std::to_string(i) + " is empty or not finite");
        }
    }
    return RTGO_OK;
}

// What was cached for the scene as it was (a primitive moved outside the old screen rectangle must not be culled); the mask's buffers stay
static void drop_launch_caches(rtgo_ctx* c)
{
    c->seeds = rtgo_ctx::Seeds();
    c->mask.key.clear();
    c->trial = rtgo_ctx::Trial();
}

// Drops the analytic scene and what was cached for it (rtgo_set_scene, rtgo_set_large_scene: after their stream sync)
static void drop_scene(rtgo_ctx* c)
{
    c->scene = AnalyticScene();
    drop_launch_caches(c);
}

// The buffers of a scene of rtgo_set_scene for n primitives, in c->scene
static int alloc_resident(rtgo_ctx* c, uint32_t n)
{
    AnalyticScene& sc = c->scene;
    RTGO_HIP(c, sc.d_prims_in.alloc(n));
    RTGO_HIP(c, sc.d_aabb.alloc(n * 6));
    RTGO_HIP(c, sc.d_nodes.alloc((2 * n - 1) * 2));
    RTGO_HIP(c, sc.d_prims.alloc(n * 6));
    RTGO_HIP(c, sc.d_frames.alloc(n * 2));
    RTGO_HIP(c, sc.d_tight.alloc(n * 6));
    return RTGO_OK;
}

// The build half of rtgo_set_scene, from what is on the device (rtgo_set_scene after its upload, rtgo_update_prims after its patch): both
// fast-walk structures, the emitter certificates, the tight boxes, the grid, the bounds and the quadric list of c->scene, whose
// d_prims_in, d_aabb (with have_aabbs), host_prims and have_aabbs are in place.  Sets n_prims last, once the build succeeded.
static int build_resident(rtgo_ctx* c, uint32_t n)
{
    const Knobs kn;
    AnalyticScene& sc = c->scene;
    const rtgo_prim* prims = sc.host_prims.data();
    if (kn.leaf_budget >= 0) c->leaf_budget = kn.leaf_budget;
    BuildMeta meta;
    if (const int rc = build_fast_tree(c, n, sc.have_aabbs ? 1 : 0, (float)kn.big_percent * 0.01f, kn, sc.tree[0], meta)) return rc;
    if (const int rc = emitter_cert(c, prims, n, sc.tree[0])) return rc;
    sc.tight.assign((size_t)n * 6, 0.0f);
    RTGO_HIP(c, hipMemcpyAsync(sc.tight.data(), sc.d_tight.get(), (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    const AnalyticScene::FastTree& t0 = sc.tree[0];
    const int depth = meta.canonical_depth;
    sc.lbvh_depth = depth;
    if (!t0.sane(n)) return fail(c, RTGO_E_UNSUPPORTED, "rtgo_set_scene: the fast walk's tree has " + std::to_string(t0.n_fnodes) + " nodes");
    std::memcpy(sc.bounds, meta.tight_bounds, sizeof sc.bounds);
    if (!kn.pin_big) {
        // the alternative structure: big_frac 15 % (the canonical outputs, boxes and frames are rewritten with the same values)
        BuildMeta m2;
        if (const int rc = build_fast_tree(c, n, 1, 0.15f, kn, sc.tree[1], m2)) return rc;
        if (const int rc = emitter_cert(c, prims, n, sc.tree[1])) return rc;
        const AnalyticScene::FastTree& t1 = sc.tree[1];
        // (the same split of primitives = the same structure: nothing to try)
        sc.have_alt = m2.canonical_depth == meta.canonical_depth && t1.sane(n) &&
                      !(t1.n_small == t0.n_small && t1.n_fnodes == t0.n_fnodes && t1.n_big_pairs == t0.n_big_pairs && t1.list_cub == t0.list_cub);
    }
    if (const int rc = build_grid(c, n, kn)) return rc;
    if (kn.debug)
        std::fprintf(stderr, "rtgo_set_scene: %d primitives, %d in the fast walk's tree (%d nodes, depth %d), %d up front (%d pairs, cuboid certificate %d, slab certificate %d), %d cuboid leaves (slab certificates of a two-leaf tree: %d %d), margin coefficients %g %g, canonical LBVH depth %d\n",
                     (int)n, t0.n_small, t0.n_fnodes, t0.fast_depth, (int)n - t0.n_small, t0.n_big_pairs, t0.list_cub, t0.slab_list ? 1 : 0, meta.cuboid_leaves, t0.slab_leaves & 1, (t0.slab_leaves >> 1) & 1,
                     t0.cub_a, t0.cub_b, depth);
    if (depth > kStackDepth)
        return fail(c, RTGO_E_UNSUPPORTED, "rtgo_set_scene: LBVH depth " + std::to_string(depth) + " exceeds the per-lane LDS stack (" +
                                               std::to_string(kStackDepth) + ")");
    sc.n_prims = n;
    for (uint32_t i = 0; i < n; ++i) {
        const rtgo_prim& q = prims[i];
        if (q.type != RTGO_SPHERE && q.type != RTGO_CYLINDER) continue;
        // axis scales = column norms of the model matrix' 3x3 (exact for translate * rotate * scale; a cylinder's quadratic lives in x, z)
        double s[3];
        for (int k = 0; k < 3; ++k) s[k] = std::sqrt((double)q.model[k] * q.model[k] + (double)q.model[4 + k] * q.model[4 + k] + (double)q.model[8 + k] * q.model[8 + k]);
        double smin = s[0] < s[2] ? s[0] : s[2], smax = s[0] > s[2] ? s[0] : s[2];
        if (q.type == RTGO_SPHERE) {
            smin = s[1] < smin ? s[1] : smin;
            smax = s[1] > smax ? s[1] : smax;
        }
        AnalyticScene::Quadric e;
        e.c[0] = q.model[3];
        e.c[1] = q.model[7];
        e.c[2] = q.model[11];
        e.w = (float)(smax / (smin * smin));
        sc.quadrics.push_back(e);
    }
    return RTGO_OK;
}

// rtgo_set_scene and rtgo_set_scene_device from drop_scene on: n checked records (and boxes, nullable) in host memory, or (`device`) in
// device memory -- then the host copy that emitter_cert and the quadric list read is taken from the context's own copy of them
static int set_resident(rtgo_ctx* c, const void* prims, const void* aabbs, uint32_t n, bool device)
{
    const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    drop_scene(c);
    AnalyticScene& sc = c->scene;
    if (const int rc = alloc_resident(c, n)) return rc;
    sc.have_aabbs = aabbs != nullptr;
    RTGO_HIP(c, hipMemcpyAsync(sc.d_prims_in.get(), prims, n * sizeof(PrimIn), kind, c->stream));
    if (aabbs) RTGO_HIP(c, hipMemcpyAsync(sc.d_aabb.get(), aabbs, n * sizeof(rtgo_aabb), kind, c->stream));
    if (device) {
        sc.host_prims.resize(n);
        RTGO_HIP(c, hipMemcpyAsync(sc.host_prims.data(), sc.d_prims_in.get(), n * sizeof(PrimIn), hipMemcpyDeviceToHost, c->stream));
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
    } else {
        const rtgo_prim* p = static_cast<const rtgo_prim*>(prims);
        sc.host_prims.assign(p, p + n);
    }
    return build_resident(c, n);
}

// the temporaries of large_build_tree, freed however it ends
struct LargeScratch {
    DeviceArray<unsigned long long> keys, keys_alt;
    DeviceArray<unsigned int> hist;
    DeviceArray<int> left, right;
    DeviceArray<float> small;   // scene bounds (6 floats), then the largest leaf depth (int)
};

// What the build of rtgo_set_large_scene makes over n boxes: the nodes, what AnalyticScene::LargeKeep holds, depth and bounds
struct LargeTree {
    DeviceArray<float4> nodes;
    AnalyticScene::LargeKeep keep;
    int lbvh_depth = 0;
    float bounds[6] = {0, 0, 0, 0, 0, 0};
};

// the box of the root of `nodes` (its two float4, read back with one wait) into bounds
static int read_root_bounds(rtgo_ctx* c, const float4* nodes, float bounds[6])
{
    float4 root[2];
    RTGO_HIP(c, hipMemcpyAsync(root, nodes, sizeof root, hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    const float b[6] = {root[0].x, root[0].y, root[0].z, root[1].x, root[1].y, root[1].z};
    std::memcpy(bounds, b, sizeof b);
    return RTGO_OK;
}

// The canonical LBVH over the n boxes at d_aabb (device), into arrays of its own (rtgo_set_large_scene; rtgo_update_prims' rebuild, which
// swaps them in on success).  A tree deeper than the walk's stack: RTGO_E_UNSUPPORTED.  The stream is idle when it returns.
static int large_build_tree(rtgo_ctx* c, const float* d_aabb, uint32_t n, const std::string& what, LargeTree& t)
{
    const int ni = (int)n, n_int = ni > 1 ? ni - 1 : 1;
    LargeScratch ls;
    RTGO_HIP(c, t.nodes.alloc((2 * (size_t)n - 1) * 2));
    RTGO_HIP(c, t.keep.parent.alloc(2 * (size_t)n - 1));
    RTGO_HIP(c, t.keep.depth.alloc(n_int));
    RTGO_HIP(c, t.keep.leaf_of.alloc(n));
    RTGO_HIP(c, t.keep.mark.alloc(n_int));
    RTGO_HIP(c, ls.keys.alloc(n));
    RTGO_HIP(c, ls.keys_alt.alloc(n));
    RTGO_HIP(c, ls.hist.alloc((size_t)256 * ((ni + whitted::kRadixTile - 1) / whitted::kRadixTile)));
    RTGO_HIP(c, ls.left.alloc(n_int));
    RTGO_HIP(c, ls.right.alloc(n_int));
    RTGO_HIP(c, ls.small.alloc(8));
    RTGO_HIP(c, hipMemsetAsync(ls.small.get(), 0, 8 * sizeof(float), c->stream));
    RTGO_HIP(c, hipMemsetAsync(t.keep.mark.get(), 0, (size_t)n_int * sizeof(unsigned int), c->stream));
    const dim3 g_prims((n + 255) / 256), g_nodes((2 * n - 1 + 255) / 256), g_int((n_int + 255) / 256);
    // bounds; Morton keys in (code, index) order (four stable passes over the code's bytes: back in ls.keys)
    hipLaunchKernelGGL(whitted::big_bounds_final_kernel, dim3(1), dim3(1024), 0, c->stream, d_aabb, ni, ls.small.get());
    hipLaunchKernelGGL(large_keys_kernel, g_prims, dim3(256), 0, c->stream, d_aabb, ni, (const float*)ls.small.get(), ls.keys.get());
    const unsigned long long* src = radix_sort_keys(c, ls.keys.get(), ls.keys_alt.get(), ls.hist.get(), ni);
    // hierarchy, depths and leaves
    int* d_max_depth = reinterpret_cast<int*>(ls.small.get() + 6);
    hipLaunchKernelGGL(large_karras_kernel, g_int, dim3(256), 0, c->stream, src, ni, ls.left.get(), ls.right.get(), t.keep.parent.get());
    hipLaunchKernelGGL(large_depth_kernel, g_nodes, dim3(256), 0, c->stream, src, ni, d_aabb, (const int*)t.keep.parent.get(), t.keep.depth.get(),
                       t.nodes.get(), d_max_depth, t.keep.leaf_of.get());
    RTGO_HIP(c, hipGetLastError());
    int depth = 0;
    RTGO_HIP(c, hipMemcpyAsync(&depth, d_max_depth, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    if (depth > kLargeMaxDepth)
        return fail(c, RTGO_E_UNSUPPORTED, what + ": LBVH depth " + std::to_string(depth) + " exceeds the per-lane LDS stack (" +
                                               std::to_string(kLargeMaxDepth) + ")");
    // boxes, one level per launch from the deepest up (a kernel boundary between a node's children and the node)
    for (int level = depth - 1; level >= 0; --level)
        hipLaunchKernelGGL(large_fit_kernel, g_int, dim3(256), 0, c->stream, (const int*)ls.left.get(), (const int*)ls.right.get(), (const int*)t.keep.depth.get(),
                           ni - 1, level, t.nodes.get());
    RTGO_HIP(c, hipGetLastError());
    t.lbvh_depth = depth;
    return read_root_bounds(c, t.nodes.get(), t.bounds);
}

// a tree large_build_tree made becomes the scene's (its nodes, shape, depth and bounds)
static void adopt_large_tree(AnalyticScene& sc, LargeTree& t)
{
    sc.d_nodes = std::move(t.nodes);
    sc.keep = std::move(t.keep);
    std::memcpy(sc.bounds, t.bounds, sizeof sc.bounds);
    sc.lbvh_depth = t.lbvh_depth;
}

// rtgo_set_large_scene and rtgo_set_large_scene_device from drop_scene on: n checked records (and boxes, nullable) in host memory, or
// (`device`) in device memory -- large_prep_kernel then reads the caller's records where they lie, and no copy of them is made
static int set_large(rtgo_ctx* c, const void* prims, const void* aabbs, uint32_t n, bool device, const std::string& what)
{
    const Knobs kn;
    drop_scene(c);
    AnalyticScene& sc = c->scene;
    const PrimIn* d_in = static_cast<const PrimIn*>(prims);
    if (!device) {
        RTGO_HIP(c, sc.d_prims_in.alloc(n));
        d_in = sc.d_prims_in.get();
    }
    RTGO_HIP(c, sc.d_aabb.alloc((size_t)n * 6));
    RTGO_HIP(c, sc.d_prims.alloc((size_t)n * 6));
    if (!device) RTGO_HIP(c, hipMemcpyAsync(sc.d_prims_in.get(), prims, (size_t)n * sizeof(PrimIn), hipMemcpyHostToDevice, c->stream));
    if (aabbs)
        RTGO_HIP(c, hipMemcpyAsync(sc.d_aabb.get(), aabbs, (size_t)n * sizeof(rtgo_aabb), device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    // records and boxes, then the tree over the boxes
    hipLaunchKernelGGL(large_prep_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, d_in, sc.d_aabb.get(), aabbs ? 1 : 0, (int)n, sc.d_prims.get());
    LargeTree t;
    if (const int rc = large_build_tree(c, sc.d_aabb.get(), n, what, t)) {
        if (rc == RTGO_E_UNSUPPORTED) c->scene = AnalyticScene();
        return rc;
    }
    sc.d_prims_in.reset();   // (the records hold all the walk and the shading read)
    adopt_large_tree(sc, t);
    sc.have_aabbs = aabbs != nullptr;
    sc.n_prims = n;
    sc.large = true;
    if (kn.debug)
        std::fprintf(stderr, "%s: %d primitives, canonical LBVH depth %d in global memory\n", what.c_str(), (int)n, sc.lbvh_depth);
    return RTGO_OK;
}

// ---- rtgo_update_prims ----

// k checked updates where the apply kernels read them: rtgo_update_prims' staging buffers, or the arrays of rtgo_update_prims_device's
// caller.  host_idx / host_prims: the host's copy of the first two (rtgo_update_prims), or nullptr.
struct UpdateRefs {
    const unsigned int* idx;
    const PrimIn* prims;
    const float* aabbs;   // nullptr: the scene was set without boxes
    uint32_t k;
    const uint32_t* host_idx;
    const rtgo_prim* host_prims;
};

// the updates on the device: indices, primitives and (with boxes) boxes, k of each.  stage_updates: u's arrays, which lie in host memory,
// uploaded into st; u then names the copies, and the host's arrays as host_idx / host_prims
struct UpdateStaging {
    DeviceArray<unsigned int> idx;
    DeviceArray<PrimIn> prims;
    DeviceArray<float> aabbs;
};
static int stage_updates(rtgo_ctx* c, UpdateRefs& u, UpdateStaging& st)
{
    static_assert(sizeof(PrimIn) == sizeof(rtgo_prim) && sizeof(rtgo_aabb) == 6 * sizeof(float), "update records");
    RTGO_HIP(c, st.idx.upload(u.idx, u.k, c->stream));
    RTGO_HIP(c, st.prims.upload(u.prims, u.k, c->stream));
    if (u.aabbs) RTGO_HIP(c, st.aabbs.upload(u.aabbs, (size_t)u.k * 6, c->stream));
    u = UpdateRefs{st.idx.get(), st.prims.get(), st.aabbs.get(), u.k, u.idx, reinterpret_cast<const rtgo_prim*>(u.prims)};
    return RTGO_OK;
}

// A scene of rtgo_set_scene: a new scene from the old one's device-resident inputs with the updates patched in, built by build_resident
// into c->scene (the caller has set the old one aside and puts it back when this fails)
static int update_resident(rtgo_ctx* c, const AnalyticScene& old, const UpdateRefs& u)
{
    const uint32_t n = old.n_prims, k = u.k;
    AnalyticScene& sc = c->scene;
    if (const int rc = alloc_resident(c, n)) return rc;
    sc.have_aabbs = old.have_aabbs;
    RTGO_HIP(c, hipMemcpyAsync(sc.d_prims_in.get(), old.d_prims_in.get(), n * sizeof(PrimIn), hipMemcpyDeviceToDevice, c->stream));
    if (sc.have_aabbs) RTGO_HIP(c, hipMemcpyAsync(sc.d_aabb.get(), old.d_aabb.get(), (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(prims_patch_kernel, dim3((k + 255) / 256), dim3(256), 0, c->stream, u.idx, u.prims, u.aabbs, (int)k, sc.d_prims_in.get(), sc.d_aabb.get());
    RTGO_HIP(c, hipGetLastError());
    if (u.host_idx) {
        sc.host_prims = old.host_prims;
        for (uint32_t j = 0; j < k; ++j) sc.host_prims[u.host_idx[j]] = u.host_prims[j];
    } else {   // the updates never were on the host: the patched records, at most RTGO_MAX_PRIMS of them, are read back
        sc.host_prims.resize(n);
        RTGO_HIP(c, hipMemcpyAsync(sc.host_prims.data(), sc.d_prims_in.get(), n * sizeof(PrimIn), hipMemcpyDeviceToHost, c->stream));
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
    }
    const int rc = build_resident(c, n);
    RTGO_HIP(c, hipStreamSynchronize(c->stream));   // (the caller frees its staging buffers on return)
    return rc;
}

// The stamp of one refit over the large scene's mark words
static int next_mark_epoch(rtgo_ctx* c, unsigned int& epoch)
{
    AnalyticScene::LargeKeep& keep = c->scene.keep;
    if (++keep.epoch == 0) {   // (the counter wrapped: start over with clean marks)
        RTGO_HIP(c, hipMemsetAsync(keep.mark.get(), 0, keep.mark.size() * sizeof(unsigned int), c->stream));
        keep.epoch = 1;
    }
    epoch = keep.epoch;
    return RTGO_OK;
}

// k updates of a large scene of n primitives: a thread per update; then per level, deepest first (large_fit_kernel's rule), one per internal node
struct EditGrid {
    int n_internal; dim3 upd, internal;
    EditGrid(uint32_t n, uint32_t k) : n_internal((int)n - 1), upd((k + 255) / 256), internal((std::max(n_internal, 1) + 255) / 256) {}
};

// A scene of rtgo_set_large_scene, refitted or rebuilt in place (`what`: the entry point, for the message)
static int update_large(rtgo_ctx* c, const UpdateRefs& u, bool rebuild, const std::string& what)
{
    AnalyticScene& sc = c->scene;
    const uint32_t n = sc.n_prims, k = u.k;
    const EditGrid g(n, k);
    DeviceArray<int> d_changed;
    RTGO_HIP(c, d_changed.alloc(1));
    RTGO_HIP(c, hipMemsetAsync(d_changed.get(), 0, sizeof(int), c->stream));
    if (!rebuild) {
        unsigned int epoch = 0;
        if (const int rc = next_mark_epoch(c, epoch)) return rc;
        hipLaunchKernelGGL(large_update_kernel, g.upd, dim3(256), 0, c->stream, u.idx, u.prims, u.aabbs, (int)k, (const int*)sc.keep.leaf_of.get(), (const int*)sc.keep.parent.get(),
                           epoch, sc.keep.mark.get(), sc.d_prims.get(), sc.d_aabb.get(), sc.d_nodes.get(), (float4*)nullptr, (float*)nullptr, d_changed.get());
        RTGO_HIP(c, hipGetLastError());
        int changed = 0;
        RTGO_HIP(c, hipMemcpyAsync(&changed, d_changed.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
        if (!changed) return RTGO_OK;
        for (int level = sc.lbvh_depth - 1; level >= 0; --level)
            hipLaunchKernelGGL(large_refit_kernel, g.internal, dim3(256), 0, c->stream, (const int*)sc.keep.depth.get(), (const unsigned int*)sc.keep.mark.get(), epoch,
                               g.n_internal, level, sc.d_nodes.get());
        RTGO_HIP(c, hipGetLastError());
        return read_root_bounds(c, sc.d_nodes.get(), sc.bounds);   // (the bounds from the new root)
    }
    // rebuild: records and boxes patched (the old ones kept), then the set call's pipeline over the boxes into new arrays
    DeviceArray<float4> old_prims;
    DeviceArray<float> old_aabb;
    RTGO_HIP(c, old_prims.alloc((size_t)k * 6));
    RTGO_HIP(c, old_aabb.alloc((size_t)k * 6));
    hipLaunchKernelGGL(large_update_kernel, g.upd, dim3(256), 0, c->stream, u.idx, u.prims, u.aabbs, (int)k, (const int*)nullptr, (const int*)nullptr, 0u,
                       (unsigned int*)nullptr, sc.d_prims.get(), sc.d_aabb.get(), (float4*)nullptr, old_prims.get(), old_aabb.get(), d_changed.get());
    RTGO_HIP(c, hipGetLastError());
    LargeTree t;
    if (const int rc = large_build_tree(c, sc.d_aabb.get(), n, what, t)) {
        const std::string msg = c->err;
        hipLaunchKernelGGL(large_restore_kernel, g.upd, dim3(256), 0, c->stream, u.idx, (const float4*)old_prims.get(),
                           (const float*)old_aabb.get(), (int)k, sc.d_prims.get(), sc.d_aabb.get());
        RTGO_HIP(c, hipStreamSynchronize(c->stream));
        c->err = msg;
        return rc;
    }
    adopt_large_tree(sc, t);
    return RTGO_OK;
}

static int check_prims_device(rtgo_ctx* c, const void* d_idx, const void* d_prims, const void* d_aabbs, uint32_t k, uint32_t n, const std::string& what);

// rtgo_update_prims and (`device`) rtgo_update_prims_device from their argument checks on: the stream drained; the host's updates staged, or
// the caller's arrays checked where they lie; the large / resident split, the old scene put back when the build is refused; the caches dropped
static int apply_updates(rtgo_ctx* c, const void* indices, const void* prims, const void* aabbs, uint32_t k, bool device, bool rebuild, const std::string& what)
{
    RTGO_HIP(c, hipSetDevice(c->device));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    UpdateStaging st;
    UpdateRefs u = {static_cast<const unsigned int*>(indices), static_cast<const PrimIn*>(prims), static_cast<const float*>(aabbs), k, nullptr, nullptr};
    if (const int rc = device ? check_prims_device(c, indices, prims, aabbs, k, c->scene.n_prims, what) : stage_updates(c, u, st)) return rc;
    if (c->scene.large) {
        if (const int rc = update_large(c, u, rebuild, what)) return rc;
    } else {
        // both flags: the set call's build again, into a scene of its own; the old one comes back when the build is refused
        AnalyticScene old = std::move(c->scene);
        c->scene = AnalyticScene();
        c->scene.claim = std::move(old.claim);
        if (const int rc = update_resident(c, old, u)) {
            (void)hipStreamSynchronize(c->stream);
            old.claim = std::move(c->scene.claim);
            c->scene = std::move(old);
            return rc;
        }
    }
    drop_launch_caches(c);
    return RTGO_OK;
}

// ---- the device-pointer twins of the set and update calls ----

// The stamp of one index check over the scene's n claim words (allocated by the scene's first such check), the words cleared on the
// stream when the array is fresh or the counter wrapped
static int next_claim_epoch(rtgo_ctx* c, uint32_t n, unsigned int& epoch)
{
    AnalyticScene::Claim& cl = c->scene.claim;
    if (cl.d.size() != n) {
        RTGO_HIP(c, cl.d.alloc(n));
        cl.epoch = 0;
    }
    if (cl.epoch == 0 || ++cl.epoch == 0) {   // (a fresh array, or the counter wrapped: start over with clean words)
        RTGO_HIP(c, hipMemsetAsync(cl.d.get(), 0, (size_t)n * sizeof(unsigned int), c->stream));
        cl.epoch = 1;
    }
    epoch = cl.epoch;
    return RTGO_OK;
}

// The verdict's choice: the lowest offending entry, of the lowest-numbered kind that names it.  That kind, or -1 for a clean verdict.
static int lowest_fault(const unsigned int* v, int kinds)
{
    int kind = -1;
    for (int q = 0; q < kinds; ++q)
        if (v[q] != kNoFault && (kind < 0 || v[q] < v[kind])) kind = q;
    return kind;
}

// check_prims, and with d_idx rtgo_update_prims' index rules over a scene of n primitives, for k entries in device memory: one launch of
// prims_check_kernel, its verdict read back with one wait.  Nothing of the scene is written; the stream is idle when it returns.
static int check_prims_device(rtgo_ctx* c, const void* d_idx, const void* d_prims, const void* d_aabbs, uint32_t k, uint32_t n, const std::string& what)
{
    if (!c->d_verdict.get()) RTGO_HIP(c, c->d_verdict.alloc(kVerdictWords));
    unsigned int epoch = 0;
    if (d_idx)
        if (const int rc = next_claim_epoch(c, n, epoch)) return rc;
    RTGO_HIP(c, hipMemsetAsync(c->d_verdict.get(), 0xFF, kVerdictWords * sizeof(unsigned int), c->stream));
    hipLaunchKernelGGL(prims_check_kernel, dim3((k + 255) / 256), dim3(256), 0, c->stream, static_cast<const unsigned int*>(d_prims),
                       static_cast<const float*>(d_aabbs), static_cast<const unsigned int*>(d_idx), k, n, epoch, c->scene.claim.d.get(), c->d_verdict.get());
    RTGO_HIP(c, hipGetLastError());
    unsigned int v[kVerdictWords];
    RTGO_HIP(c, hipMemcpyAsync(v, c->d_verdict.get(), sizeof v, hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipStreamSynchronize(c->stream));
    static const char* const kFault[kVerdictKinds] = {"has an unknown primitive type", "holds a value that is not finite", "has a singular model matrix",
                                                      "has a box that is empty or not finite", "names an index beyond the scene's primitives", "names an index another entry names too"};
    const int kind = lowest_fault(v, kVerdictKinds);
    if (kind < 0) return RTGO_OK;
    return fail(c, RTGO_E_INVALID, what + ": entry " + std::to_string(v[kind]) + " " + kFault[kind]);
}

// ---- the refit that waits for nothing on the host ----

// rtgo_update_prims_device_async from its argument checks on: a slot of the ring, then the check, the update and the refit of k entries
// of a large scene enqueued back to back; *ticket = the slot's ticket
static int enqueue_update_async(rtgo_ctx* c, const void* d_indices, const void* d_prims, const void* d_aabbs, uint32_t k, const ReachBox& rb, uint64_t* ticket)
{
    AnalyticScene& sc = c->scene;
    const uint32_t n = sc.n_prims;
    RTGO_HIP(c, hipSetDevice(c->device));
    rtgo_ctx::UpdateRing& ring = c->updates;
    const size_t slots = rtgo_ctx::UpdateRing::kSlots;
    if (!ring.d.get()) {   // the first call: the ring's device words (every call fills its verdict and clears its `changed` word itself), their pinned copy, the events
        RTGO_HIP(c, ring.d.alloc(slots * (kVerdictWords + 1)));
        RTGO_HIP(c, ring.h.alloc(slots * kVerdictWords));
        for (size_t s = 0; s < slots; ++s)
            if (!ring.done[s].get()) RTGO_HIP(c, ring.done[s].create(hipEventDisableTiming));
    }
    const uint64_t t = ring.next;
    const unsigned int slot = rtgo_ctx::UpdateRing::slot(t);
    // the slot's last ticket leaves the ring; a ring full of updates in flight waits here for the oldest, as timed_launch's does
    if (ring.next_reuses_a_slot()) RTGO_HIP(c, hipEventSynchronize(ring.done[slot].get()));
    unsigned int *d_verdict = ring.d.get() + (size_t)slot * kVerdictWords, *d_changed = ring.d.get() + slots * kVerdictWords + slot;
    unsigned int claim_epoch = 0, mark_epoch = 0;
    if (const int rc = next_claim_epoch(c, n, claim_epoch)) return rc;
    if (const int rc = next_mark_epoch(c, mark_epoch)) return rc;
    RTGO_HIP(c, hipMemsetAsync(d_verdict, 0xFF, kVerdictWords * sizeof(unsigned int), c->stream));
    RTGO_HIP(c, hipMemsetAsync(d_changed, 0, sizeof(unsigned int), c->stream));
    const unsigned int *idx = static_cast<const unsigned int*>(d_indices), *prims = static_cast<const unsigned int*>(d_prims);
    const float* boxes = static_cast<const float*>(d_aabbs);
    const EditGrid g(n, k);
    hipLaunchKernelGGL(prims_check_reach_kernel, g.upd, dim3(256), 0, c->stream, prims, boxes, idx, k, n, claim_epoch, sc.claim.d.get(), d_verdict, rb);
    RTGO_HIP(c, hipMemcpyAsync(ring.h.get() + (size_t)slot * kVerdictWords, d_verdict, kVerdictWords * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    RTGO_HIP(c, hipEventRecord(ring.done[slot].get(), c->stream));
    // the gated kernels: all of them, every time -- neither the verdict nor `changed` is known here
    hipLaunchKernelGGL(large_update_staged_kernel, g.upd, dim3(256), 0, c->stream, (const unsigned int*)d_verdict, idx, prims, boxes, k, (const int*)sc.keep.leaf_of.get(),
                       (const int*)sc.keep.parent.get(), mark_epoch, sc.keep.mark.get(), sc.d_prims.get(), sc.d_aabb.get(), sc.d_nodes.get(), d_changed);
    for (int level = sc.lbvh_depth - 1; level >= 0; --level)
        hipLaunchKernelGGL(large_refit_gated_kernel, g.internal, dim3(256), 0, c->stream, (const unsigned int*)d_verdict, (const unsigned int*)d_changed,
                           (const int*)sc.keep.depth.get(), (const unsigned int*)sc.keep.mark.get(), mark_epoch, g.n_internal, level, sc.d_nodes.get());
    RTGO_HIP(c, hipGetLastError());
    // the root box is not read back: from now on the scene lies inside the old bounds or inside `reach`, applied or refused
    for (int a = 0; a < 3; ++a) {
        sc.bounds[a] = std::fmin(sc.bounds[a], rb.lo[a]);
        sc.bounds[3 + a] = std::fmax(sc.bounds[3 + a], rb.hi[a]);
    }
    drop_launch_caches(c);   // (a large scene's launches keep no seed buffers: nothing is freed here)
    ring.next = t + 1;
    *ticket = t;
    return RTGO_OK;
}
