// rtgo_render_body.inc -- the body of the render megakernel (rtgo_device.h has the account of it), a textual fragment like the three it
// includes: render_kernel, render_frames_kernel, render_pair_kernel, render_slab7_kernel and render_unit16_kernel are this text under their own template
// parameters.  Expects p_arg, g_fprims and the constants PATH, STATS, WPE, STREAM, COUNT, FRAMES, GRID, GLOBAL, BATCH, PAIR, SLAB, UNIT16 in scope (SLAB:
// the pair kernels' cuboid tests are cuboid_slab's; render_slab7_kernel and render_unit16_kernel set it.  UNIT16: the launch has 16 samples per pixel and
// workgroups of 256 threads, and what follows from the two is compile-time; render_unit16_kernel alone sets it).
    const LaunchParams& p = p_arg;
    static_assert(!BATCH || (!STATS && !STREAM && !GRID && WPE <= 5), "frames are batched by the lock-step kernels over a tree, at 4 and 5 waves");
    static_assert(!GLOBAL || (STATS && !FRAMES && !GRID && !STREAM), "the global-memory scene is walked by the canonical walk alone");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // LDS image.  STATS (canonical, instrumented walk): [nodes 2/node][prims 6/prim, SBT order][frames 2/prim][stack][lights]
    //             fast walk (the timed kernel):          [fnodes 2/node][fprims 4/prim, Morton order][materials 3/prim][frames 2/prim][stack, 4 B/entry][lights]
    //             GLOBAL:                                [stack][lights]
    constexpr int MS = STATS ? 6 : 3;  // float4 stride between two primitives' material rows (kd|spec, kr|type, Le)
    const int n_nodes = STATS ? p.n_nodes : (PAIR ? kPairNodes : p.n_fnodes);
    float4* s_nodes = GLOBAL ? const_cast<float4*>(p.nodes) : reinterpret_cast<float4*>(smem);
    float4* s_prims = GLOBAL ? const_cast<float4*>(p.prims) : s_nodes + 2 * n_nodes;
    float4* s_mat_w = STATS ? s_prims + 3 : s_prims + 4 * p.n_prims;
    float4* s_frame_w = STATS ? s_prims + 6 * p.n_prims : s_mat_w + 3 * p.n_prims;   // shading frames of the flat primitives, 2 float4 per primitive, SBT order
    float4* s_end = GLOBAL ? reinterpret_cast<float4*>(smem) : s_frame_w + (FRAMES ? 2 * p.n_prims : 0);   // (only the instantiation that uses them pays for them)
    const float4* s_frame = s_frame_w;
    float2* s_stack_base = reinterpret_cast<float2*>(s_end);
    const int stack_depth = (STATS && !GLOBAL) ? kStackDepth : p.stack_depth;
    static_assert(!UNIT16 || (PAIR && PATH && !STREAM && !BATCH && !STATS && WPE >= 6), "16 samples in one DPP row: the lean lock-step pair kernels");
    const int kBlock = UNIT16 ? 256 : (int)blockDim.x;           // 256, 512 or 1024
    const int bshift = UNIT16 ? 8 : 31 - __clz(kBlock);          // per-lane stack entry e lives at [e << bshift]
    // (entries x workgroup size x 8 bytes for the canonical walk, x 4 for the fast walk's packed words: a multiple of 1 KiB either way)
    LightRec* s_lights = reinterpret_cast<LightRec*>(reinterpret_cast<unsigned char*>(s_stack_base) + (size_t)stack_depth * kBlock * (STATS ? 8 : 4));
    const float4* s_mat = s_mat_w;
    // small scenes (the 5- and 6-waves-per-SIMD variants): per-level path records live in LDS, [4 words x kMaxLevels][lane], instead of
    // 15-20 VGPRs -- that is what lets the allocation fit 96 registers without spilling to scratch
    // (the batched distributed kernels hold a strip's running averages through the ray loop on top of the shadow ray's state: they keep
    // the level records in LDS at 4 waves too, and at 5 waves the shadow ray's state as well -- SHLDS, 9 words per lane behind the level
    // records -- which is what fits them into 128 / 96 VGPRs without scratch)
    constexpr bool LVLDS = (WPE >= 5) || (BATCH && !PATH);
    constexpr bool SHLDS = BATCH && !PATH && WPE >= 5;
    constexpr int LVW = PATH ? 3 : 4;   // words per level record: the weight (path) / the term and the primitive (distributed)
    // the pair kernels' lock-step loop folds a path's level records once, after the ray loop, for all 64 lanes together -- in the loop
    // the fold is a divergent loop that runs for the lane or two whose path has just ended (a ray that reaches the emitter), at a whole
    // issue slot per instruction.  Until then an ended lane keeps one word, `ended_in`, in place of the payload: in path mode a finished
    // path's payload is the background colour, the Le row of the emitter it hit, or zero (the depth limit), and nothing touches the lane's
    // depth and LDS records while it is inactive.  The same multiplications in the same order: the same bits.
    constexpr bool FOLDLATE = PAIR;
    static_assert(!FOLDLATE || (PATH && LVLDS && !STREAM && !BATCH), "the deferred fold is the path-mode fold over LDS records, in the lock-step loop");
    // the pair kernels' ray loop carries the walk's predicates as the wave's lane masks (Pred<true>, rtgo_device.h): a vote is a scalar
    // compare, with none of the vector instructions hipcc puts around __ballot of a combination of compares
    constexpr bool MASKS = PAIR;
    // raygen constants (eye, U, V, W, image size, sample step): read from LDS where a sample starts, instead of sitting in
    // registers through the ray loop
    float* s_cam = reinterpret_cast<float*>(s_lights + kMaxLights);
    constexpr int CAMW = (WPE >= 6 || SHLDS) ? kCamWordsLean : kCamWords;
    // per sample k of a pixel (the first kSampleTab of them): the LCG's 2k-step map (A, C) -- the sample's jitter starts from A * seed + C,
    // the pixel's tea<16> seed advanced by 2k draws -- and the sample's cell (i, j) = (k / N, k % N) of the N x N jitter grid.  They depend on
    // k alone: a table instead of ~70 instructions of squaring loop and an integer division wherever a sample starts (most of a primary ray's
    // cost where primary rays are most rays: plateau 4K spp 256 17.2 -> 16.4 ms, mirror_spheres 4K spp 64 14.6 -> 14.3, cornell -1 %)
    uint4* s_tab = reinterpret_cast<uint4*>(s_cam + CAMW);
    const unsigned int n_tab = UNIT16 ? 16u : ((unsigned int)(p.sqrt_spp * p.sqrt_spp) < (unsigned int)kSampleTab ? (unsigned int)(p.sqrt_spp * p.sqrt_spp) : (unsigned int)kSampleTab);
    static_assert(kSampleTab >= 16, "UNIT16 starts every sample from the table");
    float* s_lv = s_cam + CAMW + 4 * n_tab + threadIdx.x;
    // STREAM: the payload window of this wave (4 passes x 3 channels x 64 lanes), behind the level records
    float* s_sh = s_cam + CAMW + 4 * n_tab + (int)blockDim.x * LVW * kMaxLevels + 9 * threadIdx.x;
    float* s_win_base = s_cam + CAMW + 4 * n_tab + (LVLDS ? (int)blockDim.x * LVW * kMaxLevels : 0) + 192 * kStreamWindow * (threadIdx.x >> 6);

    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid < kQueues) p.queue_next[kQueueStride * (unsigned int)tid] = 0u;
    Timeline tl;        // (diagnostic builds' probes, rtgo_probes.h: empty types in the product build)
    StreamStats census;
    tl.kernel_start();
    if (STATS) {
        if (!GLOBAL) {
            for (int i = tid; i < 2 * p.n_nodes; i += kBlock) s_nodes[i] = p.nodes[i];
            for (int i = tid; i < 6 * p.n_prims; i += kBlock) s_prims[i] = p.prims[i];
        }
    } else {
        for (int i = tid; i < 2 * n_nodes; i += kBlock) s_nodes[i] = p.fnodes[i];
        for (int i = tid; i < 4 * p.n_prims; i += kBlock) s_prims[i] = p.fprims[i];
        for (int i = tid; i < 3 * p.n_prims; i += kBlock) s_mat_w[i] = p.prims[6 * (i / 3) + 3 + (i % 3)];
    }
    if (FRAMES)
        for (int i = tid; i < 2 * p.n_prims; i += kBlock) s_frame_w[i] = p.frames[i];
    for (unsigned int k = threadIdx.x; k < n_tab; k += blockDim.x) {
        const unsigned int si = k / (unsigned int)p.sqrt_spp;
        s_tab[k] = make_uint4(lcg_skip(1u, 2u * k) - lcg_skip(0u, 2u * k), lcg_skip(0u, 2u * k), si, k - si * (unsigned int)p.sqrt_spp);   // A = map(1) - map(0), C = map(0)
    }
    if (threadIdx.x == 0) {
        s_cam[0] = p.eye.x; s_cam[1] = p.eye.y; s_cam[2] = p.eye.z; s_cam[3] = (float)p.W;
        s_cam[4] = p.U.x; s_cam[5] = p.U.y; s_cam[6] = p.U.z; s_cam[7] = (float)p.H;
        s_cam[8] = p.V.x; s_cam[9] = p.V.y; s_cam[10] = p.V.z; s_cam[11] = 1.0f / (float)p.sqrt_spp;
        s_cam[12] = p.Wv.x; s_cam[13] = p.Wv.y; s_cam[14] = p.Wv.z; s_cam[15] = 0.0f;
        if constexpr (CAMW > 16) {   // (6-waves variant: write_pixel's ratio and 1 / nn)
            s_cam[16] = 1.0f / (float)(p.frame + 1); s_cam[17] = 1.0f / (float)(p.sqrt_spp * p.sqrt_spp); s_cam[18] = 0.0f; s_cam[19] = 0.0f;
        }
    }
    {
        const float* src = reinterpret_cast<const float*>(p.lights);
        float* dst = reinterpret_cast<float*>(s_lights);
        for (int i = tid; i < p.n_lights * 16; i += kBlock) dst[i] = src[i];
    }
    __syncthreads();

    tl.staged();
    float2* s_stack = s_stack_base + tid;                                                 // canonical walk: (distance, node) entries
    unsigned int* s_stack4 = reinterpret_cast<unsigned int*>(s_stack_base) + tid;         // fast walk: one packed word per entry
    const int lane = tid & 63;
    // LEAN (the 6-waves variant): values derived from the lane index, and the two reciprocals write_pixel needs, are derived
    // where they are used (opaque_lane, s_cam) instead of being held in VGPRs through every ray loop -- what fits 80 VGPRs without
    // scratch.  The other variants keep the hoisted values, which their budgets afford and which are cheaper.
    constexpr bool LEAN = (WPE >= 6) || SHLDS;
    // path mode, fast walk over a tree: a path's last ray takes the emitters-first walk when the launch has the certificate (p.emit_n)
    constexpr bool LASTRAY = PATH && !STATS && !GRID;
    constexpr bool SEEDS = kernel_has_seed_pass(STATS, WPE, STREAM);
    auto lane_index = [&]() { return LEAN ? opaque_lane() : (unsigned int)lane; };
    auto frame_ratio = [&]() { return LEAN ? s_cam[16] : 1.0f / (float)(p.frame + 1); };
    const unsigned int nn = UNIT16 ? 16u : (unsigned int)(p.sqrt_spp * p.sqrt_spp);
    auto inv_nn = [&]() { return UNIT16 ? 0.0625f : (LEAN ? s_cam[17] : 1.0f / (float)nn); };   // (1.0f / 16.0f, as s_cam[17] holds it)
    // Work decomposition: ONE LANE = ONE PATH.  A wave takes "units" of 64/nn_eff neighbouring pixels of a row and runs
    // nn_eff = min(nn, 16) samples of each side by side, in ceil(nn / nn_eff) passes.  The samples of a pixel are independent
    // given the LCG state their jitter starts from (trace passes the seed by value, kernel.cu:46-79), which is the pixel's
    // tea<16> seed advanced by 2k draws; their results are then summed IN SAMPLE ORDER (kernel.cu:232), so the pixel is bit
    // for bit what the reference's sequential loop gives.  Against one-lane-per-pixel this keeps the 64 lanes at the same
    // bounce, and makes the unit of scheduling 16x smaller at 16 spp (the frame has only ~2 in-scene 64-pixel tiles per
    // resident wave: whole waves idle behind the last ones, and with the frame split over 8 GPUs most waves never get one).
    // (UNIT16: nn_eff = 16, P = 4 and passes = 1 are constants: the divisions below are shifts and masks, pl < P always holds, the pass loop is gone)
    static_assert(!UNIT16 || kSamplesPerPass == 16, "UNIT16: a pixel's samples of a pass are one DPP row");
    const unsigned int nn_eff = UNIT16 ? 16u : (nn < (unsigned int)kSamplesPerPass ? nn : (unsigned int)kSamplesPerPass);  // samples of one pixel that share a pass
    const unsigned int P = 64u / nn_eff;                        // pixels per unit
    const unsigned int passes = (nn + nn_eff - 1u) / nn_eff;
    const unsigned int pl0 = (unsigned int)lane / nn_eff;        // this lane's pixel within the unit (LEAN: derived where used)
    const unsigned int kl0 = (unsigned int)lane - pl0 * nn_eff;  // this lane's sample within the pass
    const unsigned int group_base0 = (pl0 < P ? pl0 : 0u) * nn_eff;

    unsigned int c_rays = 0, c_occl = 0, c_nodes = 0, c_tests = 0, c_hits = 0;

    // Work queue: kQueues heads, 64 bytes apart; head q serves the entries u with u % kQueues == q.  A wave pulls from the head
    // blockIdx % kQueues and, when that runs dry, from the others.  One head saturates at ~88 dequeues/us chip-wide
    // (MI355X_MICROARCH "dequeue"), which 5120 waves on 64-path units exceed several times over; heads on different lines
    // proceed side by side.  Results do not depend on who takes what.
    unsigned int q = blockIdx.x % (unsigned int)kQueues;
    // The FIRST strip of every wave is assigned statically (its rank among the waves of its queue): 5120 waves pulling at once
    // would queue up behind the heads for 10-30 us.  Head q therefore counts from n_static(q) = the waves on queue q.
    const unsigned int wpb = (unsigned int)kBlock >> 6;
    auto n_static = [&](unsigned int qq) { return ((gridDim.x + (unsigned int)kQueues - 1u - qq) / (unsigned int)kQueues) * wpb; };
    // the pull for the NEXT strip is issued before the current one is processed, so its ~1-2 us round trip hides behind work
    // (the head's offset is added when the value is USED: arithmetic on it here would make the wave wait for the atomic at once)
    // (LEAN: the wave's index in its workgroup as a wave-uniform value: an SGPR to the seed pass at the end instead of a VGPR of tid)
    const unsigned int wave_in_block = LEAN ? __builtin_amdgcn_readfirstlane((unsigned int)tid >> 6) : (unsigned int)tid >> 6;
    unsigned int pending = (blockIdx.x / (unsigned int)kQueues) * wpb + wave_in_block, pending_off = 0u;
    for (;;) {
        const LaunchParams& p = params_here<LEAN>(p_arg);
        const unsigned int lane_q = lane_index();
        const unsigned int q_count = (p.n_tiles + (unsigned int)kQueues - 1u - q) / (unsigned int)kQueues;   // units in queue q
        tl.queue_wait_begin();
        const unsigned int first = __builtin_amdgcn_readfirstlane(pending) + pending_off;
        tl.queue_wait_end();
        tl.first_pull_known();
        if (first >= q_count) {
            // own head is past its end: look at all heads at once (one load, lanes 0..7) and move to one that still has work.
            // Heads only grow, so "none has work" is final: the wave leaves and the grid drains.
            unsigned int head = 0xFFFFFFFFu, cnt_l = 0u;
            if (lane_q < (unsigned int)kQueues) {
                head = __hip_atomic_load(p.queue + kQueueStride * lane_q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + n_static(lane_q);
                cnt_l = (p.n_tiles + (unsigned int)kQueues - 1u - lane_q) / (unsigned int)kQueues;
            }
            const unsigned long long open = __ballot(head < cnt_l);
            if (open == 0ull) break;
            q = (unsigned int)(__ffsll((long long)open) - 1);
            // (rare path: consume the result at once, so that no write to its register is pending where the paths join --
            // the compiler would otherwise wait for the common path's prefetch there as well)
            unsigned int stolen = 0;
            if (lane_index() == 0u) stolen = atomicAdd(p.queue + kQueueStride * q, 1u);
            pending = __builtin_amdgcn_readfirstlane(stolen);
            pending_off = n_static(q);
            continue;
        }
        if (lane_index() == 0u) pending = atomicAdd(p.queue + kQueueStride * q, 1u);
        pending_off = n_static(q);
        // one queue entry = one STRIP: p.grab units side by side on a row (at most 64 pixels).  The strip's tea<16> pixel seeds
        // are computed once, one pixel per lane (the hash is 16 dependent rounds: ~160 instructions whether 4 or 64 lanes need
        // it), and handed to the units by lane exchange.
        const unsigned int strip = first * (unsigned int)kQueues + q;
        if (strip >= p.n_hot) {
            // cold chunk: pixels no primary ray of which can reach the scene's bounds.  Each of their N*N samples is one ray that
            // misses (__miss__ms, kernel.cu:419-423), so the pixel is the in-order sum of N*N background colours / (N*N): p.bg_pixel.
            const unsigned int s0 = (strip - p.n_hot) * p.cold_cs;
            const unsigned int s1 = s0 + p.cold_cs < p.n_cold_segs ? s0 + p.cold_cs : p.n_cold_segs;
            for (unsigned int s = s0; s < s1; ++s) {
                unsigned int clr, cx, clim;
                cold_segment(p, s, clr, cx, clim);
                const unsigned int lx = cx + lane_q;
                if (lx < clim) {
                    if constexpr (BATCH) write_pixel_frames(p, (size_t)clr * p.w + lx, p.bg_pixel);
                    else write_pixel(p, (size_t)clr * p.w + lx, p.bg_pixel, frame_ratio());
                    c_rays += BATCH ? nn * p.n_frames : nn;
                }
            }
            continue;
        }
        const unsigned int lr = p.hot_y0 + strip / p.hot_w;   // local (compact) row
        const unsigned int sx = p.hot_x0 + (strip - (lr - p.hot_y0) * p.hot_w);   // strip column
        if (p.hot_mask != nullptr && ((p.hot_mask[strip >> 5] >> (strip & 31u)) & 1u) == 0u) {
            // a strip of the rectangle that no primitive's own screen rectangle reaches (the word is wave-uniform: a scalar load)
            const unsigned int lx0 = sx * p.grab * P + lane_q;
            if (lane_q < p.grab * P && lx0 < p.w) {
                if constexpr (BATCH) write_pixel_frames(p, (size_t)lr * p.w + lx0, p.bg_pixel);
                else write_pixel(p, (size_t)lr * p.w + lx0, p.bg_pixel, frame_ratio());
                c_rays += BATCH ? nn * p.n_frames : nn;
            }
            continue;
        }
        // local row -> window row under the band interleave
        const unsigned int band = lr / p.band_h;
        const unsigned int wrow = (band * p.n_ranks + p.rank) * p.band_h + (lr - band * p.band_h);
        const unsigned int gy = p.y0 + wrow;
        const float fy = (float)gy;
        const unsigned int strip_x0 = sx * p.grab * P;
        // BATCH: the running average of the strip's pixel `lane`, through the strip's frames (from the accumulation buffer when frames came before)
        v3 mean = mk(0.0f, 0.0f, 0.0f);
        const bool mean_lane = BATCH && lane_q < p.grab * P && strip_x0 + lane_q < p.w;
        if constexpr (BATCH)
            if (mean_lane && p.frame > 0) {
                const float4 prev4 = p.accum[(size_t)lr * p.w + strip_x0 + lane_q];
                mean = mk(prev4.x, prev4.y, prev4.z);
            }
#pragma unroll 1
        for (unsigned int fk = 0; fk < (BATCH ? p.n_frames : 1u); ++fk) {
        // (pre-hashed by the previous launch when the host says they are there: one load instead of the 16 rounds)
        unsigned int strip_seed;
        if (SEEDS && p.seeds != nullptr) strip_seed = lane_q < p.grab * P ? p.seeds[strip * (p.grab * P) + lane_q] : 0u;
        else strip_seed = tea16(p.W * gy + (p.x0 + strip_x0 + lane_q), BATCH ? p.frame + fk : p.frame);
        tl.seeds_hashed(strip_seed);
#pragma unroll 1
        for (unsigned int ui = 0; ui < p.grab; ++ui) {
        const LaunchParams& p = params_here<LEAN>(p_arg);
        const unsigned int lx_u = strip_x0 + ui * P + pl0;
        if (strip_x0 + ui * P >= p.w) break;
        const bool in_range_u = pl0 < P && lx_u < p.w;
        const float fx_u = (float)(p.x0 + lx_u);
        // __raygen__rg (kernel.cu:184-247)
        const unsigned int pix0_u = (unsigned int)__shfl((int)strip_seed, (int)((ui * P + pl0) & 63u), 64);
        v3 color = mk(0.0f, 0.0f, 0.0f);
        if constexpr (!STREAM) {
#pragma unroll 1
        for (unsigned int pass = 0; pass < passes; ++pass) {
        const LaunchParams& p = params_here<LEAN>(p_arg);
        // the lane's pixel and sample, its first jitter input and its LCG seed: held through the unit (the values above), or
        // derived again per pass (LEAN; the *_u values are then dead)
        const unsigned int lane_p = lane_index();
        const unsigned int pl = LEAN ? lane_p / nn_eff : pl0, kl = LEAN ? lane_p - pl * nn_eff : kl0;
        const unsigned int lx = LEAN ? strip_x0 + ui * P + pl : lx_u;
        const bool in_range = LEAN ? ((UNIT16 || pl < P) && lx < p.w) : in_range_u;
        const float fx = LEAN ? (float)(p.x0 + lx) : fx_u;
        const unsigned int pix0 = LEAN ? (unsigned int)__shfl((int)strip_seed, (int)((ui * P + pl) & 63u), 64) : pix0_u;
        const unsigned int k = pass * nn_eff + kl;   // sample index: i-major, k = i*N + j (kernel.cu:206-208)
        bool active;
        int depth;
        int phase;                     // distributed mode: 0 = radiance ray in flight, 1 = shadow ray in flight
        unsigned int seed;
        v3 ro, rd;
        float tmin, tmax;
        v3 result;                     // payload of this sample's primary ray
        bool any_hit;
        // per-level records, folded innermost-first when the path ends (SURVEY Appendix B)
        v3 lvA[kMaxLevels];            // PATH: w_k = dot(N,Ra)*kd ; distributed: a_k = falloff*diffuse
        int lvPrim[kMaxLevels];        // distributed: primitive of level k (kr, kd re-read at fold time)
        int ended_in = kEndsInZero;    // FOLDLATE: the payload of an ended path, as one word (kEndsIn*, or the emitter's primitive)
        // distributed: state kept across the shadow ray
        v3 sN_r, sRr_r;
        float sDist_r;
        int sPrim_r, sLight_r;
        v3 &sN = SHLDS ? reinterpret_cast<v3*>(s_sh)[0] : sN_r, &sRr = SHLDS ? reinterpret_cast<v3*>(s_sh)[1] : sRr_r;
        float& sDist = SHLDS ? s_sh[6] : sDist_r;
        int &sPrim = SHLDS ? reinterpret_cast<int*>(s_sh)[7] : sPrim_r, &sLight = SHLDS ? reinterpret_cast<int*>(s_sh)[8] : sLight_r;
#include "rtgo_start_sample.inc"

        tl.unit_begin(ui, strip < p.n_hot);
        while (__ballot(active) != 0ull) {
            tl.iter_begin(active);
            const bool was_active = active;
            if (active) {
#include "rtgo_ray_trace.inc"
#include "rtgo_ray_shade.inc"
            }
            tl.iter_end(seed);
            tl.iter_ended(was_active && !active, active, depth);
        }
        if constexpr (FOLDLATE) {
            // the fold the ray loop left out (rtgo_ray_shade.inc): a lane that never started has depth 0 and kEndsInZero, its payload stays 0
            v3 term = mk(0.0f, 0.0f, 0.0f);
            if (ended_in == kEndsInBackground) {
                term = params_here<LEAN>(p_arg).bg;
            } else if (ended_in >= 0) {
                const float4 m5 = s_mat[MS * ended_in + 2];
                term = mk(m5.x, m5.y, m5.z);
            }
            if constexpr (UNIT16) {
                // (bshift is 8: level k's words are s_lv[768 k], [768 k + 256], [768 k + 512], fixed offsets from the lane's own address)
#pragma unroll
                for (int k = kMaxLevels - 1; k >= 0; --k)
                    if (k < depth) term = vmul(mk(s_lv[(k * LVW + 0) * 256], s_lv[(k * LVW + 1) * 256], s_lv[(k * LVW + 2) * 256]), term);
            } else
            for (int k = depth - 1; k >= 0; --k)
                term = vmul(mk(s_lv[(k * LVW + 0) << bshift], s_lv[(k * LVW + 1) << bshift], s_lv[(k * LVW + 2) << bshift]), term);
            result = term;
        }
        // color += payload, in sample order (kernel.cu:232): every lane of a pixel's group walks the group's results
        {
        const LaunchParams& p = params_here<LEAN>(p_arg);
        const unsigned int cnt = (nn - pass * nn_eff) < nn_eff ? (nn - pass * nn_eff) : nn_eff;
        if (__ballot(any_hit) == 0ull) {
            // every primary ray of the unit missed: all payloads are the background colour, no lane exchange needed
            for (unsigned int q = 0; q < cnt; ++q) color = vadd(color, p.bg);
        } else {
            if constexpr (UNIT16) {
                // a pixel's 16 samples are the 16 lanes of a DPP row: the same 16 additions in the same order, the addend read from the
                // row's lane q by the addition itself -- no LDS exchange, no wait.  All 64 lanes run this (the vote above is wave-uniform).
                // (one pass: the sum starts from zero, from a VGPR -- the DPP form of an addition takes no constant for its second operand)
                float zero = 0.0f;
                asm volatile("" : "+v"(zero));
                color = mk(zero, zero, zero);
                row_sum16(color, result);
            } else {
            const unsigned int lane_f = lane_index(), pl_f = LEAN ? lane_f / nn_eff : pl0;
            const unsigned int group_base = LEAN ? (pl_f < P ? pl_f : 0u) * nn_eff : group_base0;
            for (unsigned int q = 0; q < cnt; ++q) {
                const int src = (int)(group_base + q);
                color = vadd(color, mk(__shfl(result.x, src, 64), __shfl(result.y, src, 64), __shfl(result.z, src, 64)));
            }
            }
        }
        }
        }  // pass
        } else {
            // STREAM (frames of more than 16 spp).  The unit's work is a list of TASKS, one per (pixel, sample): task t is sample
            // t / npx of the unit's pixel t % npx.  Any lane whose path has ended takes the next task -- lanes are not tied to a pixel
            // or to a sample slot -- so the samples of the one pixel of the unit that sees the scene spread over all 64 lanes while
            // the pixels that see the background cost one ray each (lock-step: the wave traces the longest path of every pass, sixteen
            // passes at 256 spp, with most lanes idle after the first ray).  New tasks start in batches (>= kRegenBatch idle lanes
            // by __ballot, or nobody active) so that the raygen code runs with lanes to fill it.  A finished path parks its payload
            // in a ring in LDS (slot t % kRing; the slot holds a "pending" pattern from the moment the task is taken); the lanes
            // 0 .. npx-1 own one pixel each and add the payloads of its tasks in task order = sample order (kernel.cu:232) as the
            // completed prefix of the list grows, so the pixel is bit for bit the lock-step one.
            constexpr unsigned int kRing = 64u * (unsigned int)kStreamWindow, kRegenBatch = 4u;
            constexpr unsigned int kPending = 0x7FC0DEADu;   // a NaN no computation produces
            float* s_ring = s_win_base;                      // x at [slot], y at [kRing + slot], z at [2 kRing + slot]
            const unsigned int px_left = p.w - (strip_x0 + ui * P);
            const unsigned int npx = px_left < P ? px_left : P;
            const unsigned int n_tasks = nn * npx;
            unsigned int t_next = 0u, fold_ptr = 0u;   // wave-uniform: tasks taken so far, tasks folded so far
            unsigned int my_slot = 0u;
        bool active;
        int depth;
        int phase;                     // distributed mode: 0 = radiance ray in flight, 1 = shadow ray in flight
        unsigned int seed;
        v3 ro, rd;
        float tmin, tmax;
        v3 result;                     // payload of this sample's primary ray
        bool any_hit;
        // per-level records, folded innermost-first when the path ends (SURVEY Appendix B)
        v3 lvA[kMaxLevels];            // PATH: w_k = dot(N,Ra)*kd ; distributed: a_k = falloff*diffuse
        int lvPrim[kMaxLevels];        // distributed: primitive of level k (kr, kd re-read at fold time)
        int ended_in = kEndsInZero;    // FOLDLATE: the payload of an ended path, as one word (kEndsIn*, or the emitter's primitive)
        // distributed: state kept across the shadow ray
        v3 sN, sRr;
        float sDist;
        int sPrim, sLight;
            active = false;
            depth = 0;
            phase = 0;
            seed = 0u;
            ro = rd = result = sN = sRr = mk(0, 0, 0);
            tmin = tmax = sDist = 0.0f;
            any_hit = false;
            sPrim = sLight = 0;
#pragma unroll
            for (int q = 0; q < kMaxLevels; ++q) {
                lvA[q] = mk(0, 0, 0);
                lvPrim[q] = 0;
            }
            while (fold_ptr < n_tasks) {
                tl.stream_iter_begin();
                // ---- idle lanes take the next tasks, in lane order
                const unsigned long long m_idle = __builtin_amdgcn_ballot_w64(!active), m_act = ~m_idle;
                const unsigned int room = kRing - (t_next - fold_ptr);
                unsigned int n_take = (unsigned int)__popcll(m_idle);
                n_take = n_take < n_tasks - t_next ? n_take : n_tasks - t_next;
                n_take = n_take < room ? n_take : room;
                if (n_take != 0u && (m_act == 0ull || n_take >= kRegenBatch || t_next + n_take == n_tasks)) {
                    const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(m_idle >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m_idle, 0u));
                    // (every lane computes its would-be task: the seed exchange below needs the whole wave)
                    const unsigned int t = t_next + rank;
                    const unsigned int k = npx == 4u ? (t >> 2) : t / npx;   // (the usual unit: four pixels)
                    const unsigned int j = t - k * npx;
                    const unsigned int pix0 = (unsigned int)__shfl((int)strip_seed, (int)((ui * P + j) & 63u), 64);
                    if (!active && rank < n_take) {
                        const float fx = (float)(p.x0 + strip_x0 + ui * P + j);
                        const bool in_range = true;
                        my_slot = t & (kRing - 1u);
                        s_ring[my_slot] = __uint_as_float(kPending);
#include "rtgo_start_sample.inc"
                    }
                    t_next += n_take;
                    tl.stream_regen(n_take);
                }
                tl.stream_regen_done(seed);
                const bool run = active;
                // ---- one ray for every lane that runs
                if (__builtin_amdgcn_ballot_w64(run) != 0ull) {
                    tl.stream_trace_begin(run);
                    census.trace_round(active, room == 0u && m_idle != 0ull && t_next < n_tasks);
                    const bool was = run;
                    if (run) {
#include "rtgo_ray_trace.inc"
                        census.shade_round(hit);
#include "rtgo_ray_shade.inc"
                    }
                    if (was && !active) {
                        s_ring[kRing + my_slot] = result.y;
                        s_ring[2u * kRing + my_slot] = result.z;
                        s_ring[my_slot] = result.x;
                    }
                    tl.stream_trace_done(result.x);   // (trace + shading + the ring write of this iteration)
                }
                // ---- the completed prefix of the task list goes into the pixels
                {
                    const unsigned int probe = fold_ptr + (unsigned int)lane;
                    const bool ready = probe < t_next && __float_as_uint(s_ring[probe & (kRing - 1u)]) != kPending;
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(ready);
                    const unsigned int n_ready = m == ~0ull ? 64u : (unsigned int)__builtin_ctzll(~m);
                    const bool must = t_next == n_tasks || (t_next - fold_ptr) + 64u > kRing;   // nothing left to take / the ring is filling up
                    if (n_ready >= 32u || (must && n_ready != 0u)) {
                        if ((unsigned int)lane < npx) {
                            unsigned int t = fold_ptr + (((unsigned int)lane + npx - fold_ptr % npx) % npx);   // this pixel's first task in the prefix
                            for (; t < fold_ptr + n_ready; t += npx) {
                                const unsigned int slot = t & (kRing - 1u);
                                color = vadd(color, mk(s_ring[slot], s_ring[kRing + slot], s_ring[2u * kRing + slot]));
                            }
                        }
                        fold_ptr += n_ready;
                    }
                }
                tl.stream_fold_done(color.x);   // (the fold of the completed prefix)
            }
            tl.stream_unit_done();
            if ((unsigned int)lane < npx) write_pixel(p, (size_t)lr * p.w + strip_x0 + ui * P + (unsigned int)lane, vscale(color, inv_nn()), frame_ratio());
        }

        if constexpr (BATCH) {
            // every lane of a pixel's group holds the pixel's sum: lane ui * P + j of the wave takes pixel j of the unit from the group's
            // first lane and steps its average
            const v3 px = vscale(color, inv_nn());
            const unsigned int j = lane_index() - ui * P;   // (wraps for the lanes before the unit's)
            const int src = (int)((j * nn_eff) & 63u);
            const v3 cur = mk(__shfl(px.x, src, 64), __shfl(px.y, src, 64), __shfl(px.z, src, 64));
            if (j < P) mean = mean_step(mean, cur, p.frame + fk);
        } else if constexpr (!STREAM) {
            const LaunchParams& p = params_here<LEAN>(p_arg);
            const unsigned int lane_w = lane_index(), pl = LEAN ? lane_w / nn_eff : pl0, kl = LEAN ? lane_w - pl * nn_eff : kl0;
            const unsigned int lx = LEAN ? strip_x0 + ui * P + pl : lx_u;
            if ((LEAN ? ((UNIT16 || pl < P) && lx < p.w) : in_range_u) && kl == 0) {
                // kernel.cu:236-246.  float3 / float multiplies by the reciprocal (vec_math.h:479-483)
                write_pixel(p, (size_t)lr * p.w + lx, vscale(color, inv_nn()), frame_ratio());
            }
        }
        tl.unit_done();
        }  // unit
        }  // frame
        if constexpr (BATCH)
            if (mean_lane) store_pixel(p, (size_t)lr * p.w + strip_x0 + lane_index(), mean);
    }
    // the queue has run dry: next frame's seeds
    if constexpr (SEEDS)
        if (params_here<LEAN>(p_arg).seeds_next != nullptr) next_frame_seeds(params_here<LEAN>(p_arg), lane_index(), P, blockIdx.x * wpb + wave_in_block, gridDim.x * wpb);

    tl.write<STREAM>(p, lane);
    // one atomic per wave per counter
    c_rays = wave_sum(c_rays);
    c_occl = wave_sum(c_occl);
    if (COUNT) {
        c_nodes = wave_sum(c_nodes);
        c_tests = wave_sum(c_tests);
        c_hits = wave_sum(c_hits);
    }
    FastCounters::flush<STATS>(p, c_nodes, c_tests, lane);
    census.flush<STATS>(p, lane);
    if (lane == 0) {
        const LaunchParams& p = params_here<LEAN>(p_arg);
        atomicAdd(&p.counters[0], (unsigned long long)c_rays);
        if (!PATH) atomicAdd(&p.counters[1], (unsigned long long)c_occl);
        if (COUNT && p.count_stats) {
            atomicAdd(&p.counters[2], (unsigned long long)c_nodes);
            atomicAdd(&p.counters[3], (unsigned long long)c_tests);
            atomicAdd(&p.counters[4], (unsigned long long)c_hits);
        }
    }
