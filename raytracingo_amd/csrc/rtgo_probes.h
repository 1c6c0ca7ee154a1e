// rtgo_probes.h -- the diagnostic builds' instruments, one type per -D flag.  Each type has two definitions, chosen by the one #if at
// the type: the real one carries the clocks and counters and does the work; the empty one has the same methods with empty bodies, so the
// kernels call their probes unconditionally and the product build compiles to the same instructions as if the calls were not there
// (the arguments of a call are plain values: computing them has no side effect, and what an empty method ignores is dead code).
// Included by rtgo_device.h once the types the probes speak of are defined (LaunchParams, GridParams, Hit, wave_sum); inside namespace rtgo.
// Changing what a diagnostic build measures happens here; tests/test_diag_builds.py compiles every flag, which keeps each pair in step.
#pragma once

// A clock read that cannot move ahead of the computation of `v`: the sum depends on it.  (A value that happens to equal the constant costs
// that read one 10 ns tick.)
template <typename T>
__device__ __forceinline__ unsigned long long clock_after(T v) { return wall_clock64() + (v == (T)12345 ? 1 : 0); }

// ---- -DRTGO_TIMELINE: the per-wave timeline of render_kernel, 16 words per wave (tools/timeline.py, tools/timeline_stream.py) ----------
#ifdef RTGO_TIMELINE
struct Timeline {
    unsigned long long t0 = 0, t1 = 0, first = 0, lanes = 0, qwait = 0, cold = 0;
    unsigned int hot = 0;
    unsigned long long a = 0, b = 0, c = 0, d = 0, big = 0, tree = 0, loop = 0;
    unsigned long long s_regen = 0, s_trace = 0, s_shade = 0, s_lanes_trace = 0, s_lanes_regen = 0, s_regens = 0;   // streaming loop
    unsigned int units = 0, iters = 0;
    unsigned int fold_turns = 0, fold_entries = 0, fold_lane_turns = 0;   // the level-record fold of paths that end before their pass's last iteration
    unsigned long long m0 = 0, m1 = 0, m3 = 0, mw = 0;   // the marks an interval is measured from (mw: inside closest_hit_fast)

    __device__ __forceinline__ void kernel_start() { t0 = wall_clock64(); }
    __device__ __forceinline__ void staged() { t1 = wall_clock64(); }
    __device__ __forceinline__ void queue_wait_begin() { m0 = wall_clock64(); }
    __device__ __forceinline__ void queue_wait_end() { qwait += wall_clock64() - m0; }
    __device__ __forceinline__ void first_pull_known() { if (a == 0) a = wall_clock64(); }
    __device__ __forceinline__ void seeds_hashed(unsigned int strip_seed) { if (b == 0) b = clock_after(strip_seed); }
    // (lock-step loop: once per pass of a unit)
    __device__ __forceinline__ void unit_begin(unsigned int ui, bool hot_strip)
    {
        if (units++ == 0) first = wall_clock64();
        if (ui == 0) {
            if (hot_strip) hot += 1;
            else if (cold == 0) cold = wall_clock64();
        }
    }
    __device__ __forceinline__ void iter_begin(bool active)
    {
        if (iters == 1 && c == 0) c = wall_clock64();
        iters += 1;
        m0 = wall_clock64();
        lanes += (unsigned long long)__popcll(__ballot(active));
    }
    // (pinned behind the lane's LCG state, which shading advances, so the interval may end before the iteration's last payload write:
    // a read of the payload there changes the product kernel's instruction order)
    __device__ __forceinline__ void iter_end(unsigned int seed) { loop += clock_after(seed) - m0; }
    // (lock-step loop, after an iteration; `ended`: the lane's path ended in it, after `depth` bounces.)  What a fold inside the loop costs
    // a wave in an iteration that leaves lanes running: a divergent loop of as many turns as the deepest ended path has level records,
    // entered once.  Counted from the paths, so the census reads the same whether the kernel folds there or after the loop.
    __device__ __forceinline__ void iter_ended(bool ended, bool active, int depth)
    {
        if (__ballot(active) == 0ull) return;   // the pass's last iteration: every remaining lane folds
        if (__ballot(ended && depth > 0) != 0ull) fold_entries += 1;
        for (int k = 1; k <= kMaxLevels; ++k) {
            const unsigned long long m = __ballot(ended && depth >= k);
            if (m != 0ull) fold_turns += 1;
            fold_lane_turns += (unsigned int)__popcll(m);
        }
    }
    // closest_hit_fast: the up-front list, then the tree or grid walk
    __device__ __forceinline__ void walk_begin() { mw = wall_clock64(); }
    __device__ __forceinline__ void list_done(int best_pos)
    {
        const unsigned long long t = clock_after(best_pos);
        big += t - mw;
        mw = t;
    }
    __device__ __forceinline__ void walk_done(int best_pos) { tree += clock_after(best_pos) - mw; }
    // streaming loop: regen | trace + shading + ring write | fold of the completed prefix
    __device__ __forceinline__ void stream_iter_begin()
    {
        m0 = wall_clock64();
        iters += 1;
    }
    __device__ __forceinline__ void stream_regen(unsigned int n_take)
    {
        s_lanes_regen += n_take;
        s_regens += 1;
    }
    __device__ __forceinline__ void stream_regen_done(unsigned int seed)
    {
        m1 = clock_after(seed);
        s_regen += m1 - m0;
        m3 = m1;
    }
    __device__ __forceinline__ void stream_trace_begin(bool run) { s_lanes_trace += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(run)); }
    __device__ __forceinline__ void stream_trace_done(float result_x)
    {
        m3 = clock_after(result_x);
        s_trace += m3 - m1;
    }
    __device__ __forceinline__ void stream_fold_done(float color_x) { s_shade += clock_after(color_x) - m3; }
    __device__ __forceinline__ void stream_unit_done() { units += 1; }
    __device__ __forceinline__ void unit_done() { if (d == 0) d = wall_clock64(); }
    template <bool STREAM>
    __device__ __forceinline__ void write(const LaunchParams& p, int lane)
    {
        if (lane != 0) return;
        unsigned long long* r = p.timeline + 16ull * (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
        r[8] = a; r[9] = b; r[10] = c; r[11] = d; r[12] = big; r[13] = tree; r[14] = loop;
        if constexpr (STREAM) {
            r[8] = s_regen; r[9] = s_trace; r[10] = s_shade; r[11] = s_lanes_trace; r[14] = s_regens; r[15] = s_lanes_regen;
        }
        r[0] = t0; r[1] = t1; r[2] = first; r[3] = wall_clock64(); r[4] = units | ((unsigned long long)hot << 32); r[5] = iters; r[6] = lanes;
        r[7] = qwait | ((cold ? cold - t0 : 0ull) << 32);
        if constexpr (!STREAM) r[15] = (unsigned long long)(fold_turns & 0xFFFFu) | ((unsigned long long)(fold_entries & 0xFFFFu) << 16) | ((unsigned long long)fold_lane_turns << 32);
    }
};
#else
struct Timeline {
    __device__ __forceinline__ void kernel_start() {}
    __device__ __forceinline__ void staged() {}
    __device__ __forceinline__ void queue_wait_begin() {}
    __device__ __forceinline__ void queue_wait_end() {}
    __device__ __forceinline__ void first_pull_known() {}
    __device__ __forceinline__ void seeds_hashed(unsigned int) {}
    __device__ __forceinline__ void unit_begin(unsigned int, bool) {}
    __device__ __forceinline__ void iter_begin(bool) {}
    __device__ __forceinline__ void iter_end(unsigned int) {}
    __device__ __forceinline__ void iter_ended(bool, bool, int) {}
    __device__ __forceinline__ void walk_begin() {}
    __device__ __forceinline__ void list_done(int) {}
    __device__ __forceinline__ void walk_done(int) {}
    __device__ __forceinline__ void stream_iter_begin() {}
    __device__ __forceinline__ void stream_regen(unsigned int) {}
    __device__ __forceinline__ void stream_regen_done(unsigned int) {}
    __device__ __forceinline__ void stream_trace_begin(bool) {}
    __device__ __forceinline__ void stream_trace_done(float) {}
    __device__ __forceinline__ void stream_fold_done(float) {}
    __device__ __forceinline__ void stream_unit_done() {}
    __device__ __forceinline__ void unit_done() {}
    template <bool STREAM>
    __device__ __forceinline__ void write(const LaunchParams&, int) {}
};
#endif

// ---- -DRTGO_STREAM_STATS: census of the streaming loop (tools/stream_stats.py reads it from the stats' counter slots) -------------------
#ifdef RTGO_STREAM_STATS
struct StreamStats {
    unsigned long long iter = 0, trace = 0, shade_rounds = 0, shade = 0, stall = 0;

    // an iteration that traces: its live lanes; `stalled`: idle lanes and tasks left, but no room in the ring
    __device__ __forceinline__ void trace_round(bool active, bool stalled)
    {
        iter += 1;
        trace += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(active));
        if (stalled) stall += 1;
    }
    __device__ __forceinline__ void shade_round(bool hit)
    {
        if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {
            shade_rounds += 1;
            shade += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(hit));
        }
    }
    template <bool STATS>
    __device__ __forceinline__ void flush(const LaunchParams& p, int lane)
    {
        if (lane == 0 && !STATS) {
            atomicAdd(&p.counters[2], iter);          // -> node_visits
            atomicAdd(&p.counters[3], trace);         // -> prim_tests
            atomicAdd(&p.counters[4], shade_rounds);  // -> hits
            atomicAdd(&p.counters[5], shade);         // -> dbg_fast_boxes
            atomicAdd(&p.counters[6], stall);         // -> dbg_fast_tests
        }
    }
};
#else
struct StreamStats {
    __device__ __forceinline__ void trace_round(bool, bool) {}
    __device__ __forceinline__ void shade_round(bool) {}
    template <bool STATS>
    __device__ __forceinline__ void flush(const LaunchParams&, int) {}
};
#endif

// ---- -DRTGO_FAST_COUNTERS=1|2: what the FAST walk itself visits (tools/fast_counters.py) ----------------------------------------------
// The counts go into the two counters the canonical walk's COUNT uses (c_nodes: boxes tested, c_tests: leaf tests incl. the up-front list),
// which the fast walk gets by reference and otherwise leaves alone.  1: per lane.  2: wave-level -- one count per executed node step / leaf
// phase / grid iteration, whatever the number of live lanes (the first live lane counts it).
#ifdef RTGO_FAST_COUNTERS
struct FastCounters {
    static __device__ __forceinline__ unsigned int first_live_lane() { return (__ffsll((long long)__ballot(true)) - 1 == (int)(threadIdx.x & 63u)) ? 1u : 0u; }
#if RTGO_FAST_COUNTERS == 2
    static __device__ __forceinline__ void step(unsigned int& c, unsigned int) { c += first_live_lane(); }
    static __device__ __forceinline__ void wave_only(unsigned int& c) { c += first_live_lane(); }
    static __device__ __forceinline__ void lane_only(unsigned int&, unsigned int) {}
#else
    static __device__ __forceinline__ void step(unsigned int& c, unsigned int per_lane) { c += per_lane; }
    static __device__ __forceinline__ void wave_only(unsigned int&) {}
    static __device__ __forceinline__ void lane_only(unsigned int& c, unsigned int per_lane) { c += per_lane; }
#endif
    template <bool STATS>
    static __device__ __forceinline__ void flush(const LaunchParams& p, unsigned int boxes, unsigned int tests, int lane)
    {
        if (!STATS) {
            boxes = wave_sum(boxes);
            tests = wave_sum(tests);
            if (lane == 0) {
                atomicAdd(&p.counters[5], (unsigned long long)boxes);
                atomicAdd(&p.counters[6], (unsigned long long)tests);
            }
        }
    }
};
#else
struct FastCounters {
    static __device__ __forceinline__ void step(unsigned int&, unsigned int) {}       // both modes: per lane `per_lane`, or one per wave
    static __device__ __forceinline__ void wave_only(unsigned int&) {}                // mode 2 alone
    static __device__ __forceinline__ void lane_only(unsigned int&, unsigned int) {}  // mode 1 alone
    template <bool STATS>
    static __device__ __forceinline__ void flush(const LaunchParams&, unsigned int, unsigned int, int) {}
};
#endif

// ---- -DRTGO_CMPWALK: both walks on every ray of a canonical launch (tools/cmp_walks.py, tools/fuzz_farfield.py) -----------------------
#ifdef RTGO_CMPWALK
template <bool GRID, bool LAST, bool PAIR, bool MASK, bool SLAB, bool ROOMW>
__device__ __forceinline__ bool closest_hit_fast(const float4* __restrict__ s_fnodes, const float4* __restrict__ s_fprims, const float4* __restrict__ g_fprims,
                                                 const GridParams grid, unsigned int* __restrict__ s_stack, int bshift, int n_small, int n_prims, int n_big_pairs,
                                                 int list_cub, float cub_mu, bool tree_spheres, v3 o, v3 d, float tmin, float tmax, Hit& out,
                                                 unsigned int& dbg_boxes, unsigned int& dbg_tests, typename Pred<MASK>::T last, Timeline& tl, const PairWords* rw);   // (rtgo_device.h)
struct CmpWalk {
    // the fast walk on the ray the canonical walk has just answered (hit, h), straight from global memory; a disagreement is counted in
    // p.cmp[0] and the first 255 are recorded, 16 floats each
    static __device__ __forceinline__ void check(const LaunchParams& p, float2* s_stack, int bshift, v3 ro, v3 rd, float tmin, float tmax, bool hit, const Hit& h, int depth, int phase)
    {
        Hit hf;
        unsigned int d0 = 0, d1 = 0;
        Timeline tl;
        // (this lane's canonical stack is idle here: its own 8-byte slots serve as the fast walk's one-word entries)
        // (RTGO_TREE=2 hands this launch the grid in p.fnodes: p.grid.n_cells > 0 then)
        const bool hitf = p.grid.n_cells > 0
            ? closest_hit_fast<true, false, false, false, false, false>(p.fnodes, p.fprims, p.fprims, p.grid, reinterpret_cast<unsigned int*>(s_stack), bshift + 1, p.n_small, p.n_prims, p.n_big_pairs, p.list_cub, p.cub_mu, p.tree_spheres != 0, ro, rd, tmin, tmax, hf, d0, d1, false, tl, nullptr)
            : closest_hit_fast<false, false, false, false, false, false>(p.fnodes, p.fprims, p.fprims, p.grid, reinterpret_cast<unsigned int*>(s_stack), bshift + 1, p.n_small, p.n_prims, p.n_big_pairs, p.list_cub, p.cub_mu, p.tree_spheres != 0, ro, rd, tmin, tmax, hf, d0, d1, false, tl, nullptr);
        const bool same = hit == hitf && (!hit || (h.t == hf.t && h.prim == hf.prim && h.n.x == hf.n.x && h.n.y == hf.n.y && h.n.z == hf.n.z));
        if (!same) {
            const unsigned int slot = atomicAdd(reinterpret_cast<unsigned int*>(p.cmp), 1u);
            if (slot < 255u) {
                float* r = p.cmp + 16 * (slot + 1);
                r[0] = ro.x; r[1] = ro.y; r[2] = ro.z; r[3] = rd.x; r[4] = rd.y; r[5] = rd.z; r[6] = tmin; r[7] = tmax;
                r[8] = hit ? h.t : -1.0f; r[9] = hit ? (float)h.prim : -1.0f; r[10] = hitf ? hf.t : -1.0f; r[11] = hitf ? (float)hf.prim : -1.0f;
                r[12] = (float)depth; r[13] = (float)phase; r[14] = 0.0f; r[15] = 0.0f;
            }
        }
    }
};
#else
struct CmpWalk {
    static __device__ __forceinline__ void check(const LaunchParams&, float2*, int, v3, v3, float, float, bool, const Hit&, int, int) {}
};
#endif

// ---- -DRTGO_WHITTED_TIMING: wave and tile times of whitted::render_tiles (tools/whitted_perf.py prints them) ---------------------------
// 10 ns ticks summed over the waves, into the counter slots; each pixel's accum.w holds the ticks of its tile.  Frame: whitted::Frame.
#ifdef RTGO_WHITTED_TIMING
struct WhittedTiming {
    unsigned long long t0 = 0, m = 0, tiles = 0, n = 0, longest = 0;

    __device__ __forceinline__ void wave_start() { t0 = wall_clock64(); }
    __device__ __forceinline__ void tile_begin()
    {
        m = wall_clock64();
        n += 1;
    }
    template <typename Frame>
    __device__ __forceinline__ void tile_end(const Frame& f, bool in_image, unsigned int idx, unsigned int rays_total)
    {
        const unsigned long long t = clock_after(rays_total) - m;
        tiles += t;
        if (in_image) f.accum[idx].w = (float)t;
        longest = t > longest ? t : longest;
    }
    // (lane 0 of the wave)
    template <typename Frame>
    __device__ __forceinline__ void flush(const Frame& f)
    {
        atomicAdd(&f.counters[2], wall_clock64() - t0);   // wave lifetime          -> rtgo_stats.node_visits
        atomicAdd(&f.counters[4], tiles);                 // inside tiles           -> hits
        atomicAdd(&f.counters[5], n);                     // tiles                  -> dbg_fast_boxes
        atomicMax(&f.counters[6], longest);               // the longest tile       -> dbg_fast_tests
    }
};
#else
struct WhittedTiming {
    __device__ __forceinline__ void wave_start() {}
    __device__ __forceinline__ void tile_begin() {}
    template <typename Frame>
    __device__ __forceinline__ void tile_end(const Frame&, bool, unsigned int, unsigned int) {}
    template <typename Frame>
    __device__ __forceinline__ void flush(const Frame&) {}
};
#endif
