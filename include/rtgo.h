/*
 * rtgo.h -- C ABI of librtgo_hip.so: the MI355X (gfx950) replacement for the OptiX-7 host API as RayTracinGO's
 * Renderer uses it.  Plain pointers and sizes only; no torch, HIP or C++ types cross this boundary.
 *
 * Every entry point names the reference interface it replaces (paths relative to the reference tree).  The way a
 * reference maintainer binds them from engine/renderer.cpp is shown in INTEGRATION.md.
 *
 * Conventions:
 *   - every function returns 0 on success, otherwise a non-zero code (RTGO_E_*; HIP errors are passed through as
 *     RTGO_E_HIP_BASE + hipError_t).  rtgo_last_error() gives the text.  The C++ Renderer re-throws as
 *     std::runtime_error, which is what OPTIX_CHECK / CUDA_CHECK do in the reference (sutil/Exception.h:93-157).
 *   - the context owns all device memory it allocates; host pointers passed in are copied before the call returns.
 *   - a context is not thread-safe; one context per GPU (the reference is single-threaded, renderer.cpp:213-215).
 *   - rtgo_launch is asynchronous on the context's stream; rtgo_sync blocks (optixLaunch + cudaStreamSynchronize,
 *     renderer.cpp:761-773, CUDAOutputBuffer.h:247-250).
 *   - there is NO CPU fallback: without a gfx950 device rtgo_create fails loudly.
 */
#ifndef RTGO_H
#define RTGO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTGO_ABI_VERSION 6
#define RTGO_MAX_PRIMS 512  /* scene staged whole in LDS (largest reference scene: checkered, 390) */
#define RTGO_MAX_SCENE_PRIMS (1 << 20)  /* rtgo_set_large_scene: scene built and walked in global memory */
#define RTGO_MAX_LIGHTS 10  /* Params::MAX_LIGHTS, engine/params.h:115 */

enum {
    RTGO_OK = 0,
    RTGO_E_INVALID = 1,      /* bad argument */
    RTGO_E_NO_DEVICE = 2,    /* no HIP device / not gfx950 */
    RTGO_E_STATE = 3,        /* call order: scene / camera / output missing */
    RTGO_E_UNSUPPORTED = 4,  /* scene outside the LDS-resident design limits */
    RTGO_E_HIP_BASE = 1000   /* + hipError_t */
};

/* engine/primitive.h:16-22 PRIMITIVE_TYPE (selects the intersection program, primitive.cpp:12-15, 81-98) */
enum { RTGO_CYLINDER = 0, RTGO_DISK = 1, RTGO_RECTANGLE = 2, RTGO_SPHERE = 3 };

/* One hit-group record: PRIMITIVE_TYPE + device::HitGroupData (engine/params.h:103-110) =
   row-major model matrix + device::BasicMaterial (params.h:61-71).  Replaces HitGroupSbtRecord (params.h:143-155). */
typedef struct rtgo_prim {
    uint32_t type;
    float model[16];
    float kd[3];
    float kr[3];
    float specularity;
    float Le[3];
} rtgo_prim;

/* OptixAabb as filled by Primitive::GetAabb (engine/primitive.cpp:100-115) */
typedef struct rtgo_aabb {
    float minX, minY, minZ, maxX, maxY, maxZ;
} rtgo_aabb;

/* device::SurfaceLight (engine/params.h:73-87) as written by Renderer::WriteLights (renderer.cpp:655-677) */
typedef struct rtgo_light {
    float corner[3];
    float v1[3];
    float v2[3];
    float normal[3];
    float color[3];
    float falloff;
} rtgo_light;

/* Per-launch constants: device::Params (engine/params.h:112-140) minus the pointers, plus the framebuffer window
   this GPU renders (multi-GPU tiling).  Pixel seeds and ray directions always use the FULL
   image_width/image_height (kernel.cu:187-217), so any window/band split is bitwise identical to a whole-image launch. */
typedef struct rtgo_frame {
    uint32_t image_width;      /* Params::image_width  (full image) */
    uint32_t image_height;     /* Params::image_height (full image) */
    int32_t sqrt_spp;          /* Params::sqrtSamplePerPixel (--sample=N, N*N spp) */
    int32_t max_trace_depth;   /* Params::maxTraceDepth (5: renderer.cpp:616) */
    uint32_t frame_count;      /* Params::frameCount */
    uint32_t path_tracing;     /* Params::enablePathTracing */
    uint32_t use_ambient;      /* Params::useAmbientLight */
    uint32_t x0, y0, w, h;     /* window in global pixel coordinates; w = h = 0 means the full image */
    uint32_t band_h;           /* row-band height of the interleave inside the window (0 = 4) */
    uint32_t n_ranks, rank;    /* this context renders window rows r with (r / band_h) % n_ranks == rank; 0/1 = all */
    uint32_t collect_stats;    /* 1: also count LBVH node visits / primitive tests / hits over every ray (slower instrumented kernel
                                  on the canonical LBVH, every pixel traced); 2: the same counters over the TRAVERSED rays only
                                  (pixels outside the scene's screen rectangle are answered without a walk, as in timed launches) */
    uint32_t reserve_cus;      /* leave this many CUs' worth of workgroup slots to other streams (the multi-GPU driver's RCCL
                                  gather overlaps the next frame's kernel; persistent workgroups would otherwise hold every CU) */
} rtgo_frame;

typedef struct rtgo_stats {
    uint64_t rays_total;      /* optixTrace equivalents: primary + bounce + shadow (kernel.cu:63-75) */
    uint64_t rays_occlusion;  /* RAY_TYPE_OCCLUSION rays among them */
    uint64_t node_visits;     /* collect_stats only: 32-byte LBVH node records fetched and box-tested */
    uint64_t prim_tests;      /* collect_stats only: intersection-program invocations */
    uint64_t hits;            /* collect_stats only: rays whose closest-hit program ran */
    float last_launch_ms;     /* HIP-event time of the last megakernel launch (valid after rtgo_sync) */
    float total_launch_ms;    /* sum over launches since rtgo_reset_stats */
    uint32_t launches;
    uint32_t lbvh_depth;      /* depth of the on-device LBVH (rtgo_set_scene's or rtgo_set_large_scene's) */
    uint64_t dbg_fast_boxes;  /* diagnostic builds (-DRTGO_FAST_COUNTERS) only: boxes tested by the fast walk, else 0 */
    uint64_t dbg_fast_tests;  /* diagnostic builds only: leaf tests of the fast walk incl. the up-front list, else 0 */
    uint64_t rays_culled;     /* primary rays among rays_total that were answered (as misses) by the screen rectangle of the
                                 scene's bounds instead of a traversal; always 0 for collect_stats launches */
    uint32_t launches_canonical; /* launches since rtgo_reset_stats that walked the canonical LBVH: collect_stats launches, launches
                                    beyond the far-field guard (guard_reach / guard_quadric below; several times slower),
                                    and every launch over a scene of rtgo_set_large_scene */
    uint32_t cuboid_groups;   /* scene property: groups of three rectangle pairs the build certified as the faces of one box or room
                                 (tested by the fast walk's cuboid test); the up-front list's counts as one */
    float guard_reach;        /* last launch: max(|scene bounds|, |eye|), world units -- the far-field guard's first quantity */
    float guard_quadric;      /* last launch: max over spheres / cylinders of D^2 smax / smin^2 (D: farthest ray origin -- eye or scene
                                 bounds -- to the primitive; s: its axis scales) -- the guard's second quantity; 0 without quadrics */
    uint32_t last_variant;    /* last launch: bit 0 streaming loop, bit 1 the second fast-walk structure, bit 2 canonical walk, bit 3 the
                                 launch was one of the launch-time trial's (the first launches of a job time the candidate
                                 (loop, structure) pairs -- same pixels either way -- and the fastest keeps the job), bit 4 the fast walk
                                 over the uniform grid instead of a tree, bit 5 the scene walked from global memory (a scene of
                                 rtgo_set_large_scene; always with bit 2), bit 6 path mode under the last-ray certificate (a path's last
                                 ray tests the emitters and skips the room), bit 7 the last call rendered more than one
                                 frame in one kernel launch (rtgo_launch_frames' batched kernels),
                                 bit 8 the straight-line walk of a two-leaf tree (render_pair_kernel),
                                 bit 9 that walk's kernel at seven waves per SIMD (render_pair7_kernel; always with bit 8),
                                 bit 10 that walk with the slab test of a certified cuboid (render_slab7_kernel; always with bits 8 and 9),
                                 bit 11 that kernel's form for 16 samples per pixel in workgroups of 256 threads (render_unit16_kernel; always with bits 8, 9 and 10),
                                 bit 12 that kernel with the room steered in world axes (render_roomw_kernel; always with bits 8 to 11; RTGO_NO_ROOMW=1: off) */
    uint32_t launches_trial;  /* launches since rtgo_reset_stats that were trial launches */
} rtgo_stats;

typedef struct rtgo_ctx rtgo_ctx;

/* optixInit + cudaSetDevice + optixDeviceContextCreate + module/pipeline creation
   (renderer.cpp:194-273, 613-634).  Fails with RTGO_E_NO_DEVICE when there is no gfx950 GPU. */
int rtgo_create(int device, rtgo_ctx** out);

/* Renderer::CleanUp (renderer.cpp:870-885) */
int rtgo_destroy(rtgo_ctx* ctx);

/* text of the last error on this context (ctx == NULL: last error of a failed rtgo_create) */
const char* rtgo_last_error(const rtgo_ctx* ctx);

/* Use an existing HIP stream (hipStream_t passed as void*) instead of the context's own
   (the reference creates its own: renderer.cpp:215).  NULL restores the context's stream. */
int rtgo_set_stream(rtgo_ctx* ctx, void* hip_stream);

/* Renderer::CreateShapes (renderer.cpp:400-453) = optixAccelBuild over n custom-primitive AABBs (:514-611) + the
   hit-group SBT upload (:636-653).  prims[i] is SBT index i (scene shape order, then primitive order).
   aabbs may be NULL: the boxes are then derived on the device with the CubeBox rule of primitive.cpp:35-79.
   Boxes must contain their primitives (the reference's always do: CubeBox bounds the unit cube's image, padded); the timed
   kernel relies on that and culls with its own tighter per-shape boxes.
   Builds M^-1 per primitive and the canonical LBVH on the device.  Synchronous. */
int rtgo_set_scene(rtgo_ctx* ctx, const rtgo_prim* prims, const rtgo_aabb* aabbs, uint32_t n);

/* optixAccelBuild over any number of primitives (the reference has no size limit): rtgo_set_scene's arguments, checks and error codes,
   for n in [1, RTGO_MAX_SCENE_PRIMS].  Builds the same canonical LBVH as rtgo_set_scene with a multi-workgroup build in global memory and
   renders every launch with the canonical walk over it, straight from global memory (no fast-walk structures, no launch-time trial).
   A tree deeper than the walk's stack (64) is refused with RTGO_E_UNSUPPORTED.  Replaces whatever scene the context holds.  Synchronous.
   A scene within RTGO_MAX_PRIMS renders the same pixels bit for bit through rtgo_set_scene, and faster there. */
int rtgo_set_large_scene(rtgo_ctx* ctx, const rtgo_prim* prims, const rtgo_aabb* aabbs, uint32_t n);

/* flags of rtgo_update_prims, rtgo_whitted_update_meshes_device and rtgo_whitted_set_instances_device */
enum { RTGO_UPDATE_REFIT = 0, RTGO_UPDATE_REBUILD = 1 };

/* optixAccelBuild with OPTIX_BUILD_OPERATION_UPDATE (RTGO_UPDATE_REFIT) or _BUILD (RTGO_UPDATE_REBUILD) over the custom-primitive AABBs,
   plus a rewrite of n_updates hit-group SBT records (no reference counterpart: its Renderer builds once, renderer.cpp:514-611, 636-653).
   Primitive indices[j] (an SBT index) of the analytic scene the context holds becomes prims[j] -- type, model matrix and material -- and
   aabbs[j] its box; aabbs is NULL exactly when the scene was set without boxes (the box is then the CubeBox rule's, as at set time).
   The primitive count, every primitive not named, camera, lights, background, output and stream stay.  Synchronous.
   Afterwards every launch, rtgo_trace_rays and rtgo_shade_rays leaves, bit for bit, what it leaves on a fresh context given the edited
   array through the same set call, the ray counters of rtgo_stats included (any tree over the same primitives returns the same closest
   hit, ties to the lowest SBT index).
   A scene of rtgo_set_scene: both flags run the set call's build again from the inputs already on the device; the context then holds what
   a fresh rtgo_set_scene holds.  A scene of rtgo_set_large_scene: REFIT rewrites the records, the leaves and the boxes of their
   ancestors (one launch per tree level; none when no box changed) -- topology and lbvh_depth stay, so the tree is as good as the edit
   left it; REBUILD sorts and builds again over the boxes on the device, to the nodes of a fresh rtgo_set_large_scene.
   The screen-rectangle mask, the pre-hashed seeds and the launch-time trial are dropped, as by a set call.
   Everything is checked before anything on the device changes, and a refused call leaves the scene as it was.  RTGO_E_STATE: no
   analytic scene (a whitted scene alone does not count).  RTGO_E_INVALID: NULL ctx; unknown flag bits; with n_updates > 0: NULL indices
   or prims, aabbs given or NULL against the scene, an index >= the scene's count, an index named twice, anything the set call refuses of
   a primitive or a box.  RTGO_E_UNSUPPORTED: a structure the set call would refuse (a rebuilt tree deeper than the walk's stack).
   n_updates == 0 with a scene and known flags: RTGO_OK, nothing changes. */
int rtgo_update_prims(rtgo_ctx* ctx, const uint32_t* indices, const rtgo_prim* prims, const rtgo_aabb* aabbs, uint32_t n_updates,
                      uint32_t flags);

/* rtgo_set_scene, rtgo_set_large_scene and rtgo_update_prims for records that are already on the device (under OptiX the AABB buffer of a
   build input and the SBT are device pointers): a particle system's or a rigid-body step's output, a PyTorch-ROCm tensor.  d_prims =
   rtgo_prim[n] (108 bytes each, the host struct's layout), d_aabbs = rtgo_aabb[n] or NULL under the twin's rule, d_indices =
   uint32[n_updates]: DEVICE memory of the context's device, caller-owned, 4-byte aligned, overlapping nothing of the context; the calls read
   them and never write to them.  The caller's writes to them must be complete, or ordered on the context's stream (rtgo_set_stream),
   before the call.  Beyond NULL and alignment the call cannot tell whether a pointer is good: that the buffers are device memory of the
   sizes given is the caller's to vouch for, as in the ray-query calls.
   Afterwards the context holds, array for array, what the host-pointer twin holds after the same data, so frames, rtgo_trace_rays,
   rtgo_shade_rays and the ray counters of rtgo_stats are equal bit for bit; what the twin keeps or drops (camera, lights, background,
   output and stream kept; the screen-rectangle mask, the pre-hashed seeds and the launch-time trial dropped) is kept or dropped alike.
   No copy in proportion to n or n_updates crosses the host in either direction for a scene of rtgo_set_large_scene: the data is checked
   where it lies by one launch (each workgroup stages its 256 records in LDS with coalesced loads), whose verdict -- 32
   bytes: per kind of fault the lowest offending entry -- is read back with one wait; then the twin's own kernels build, refit or rebuild
   from the caller's pointers.  What else crosses is what the twin reads back (the tree's depth, the root box, a refit's `changed` word).
   A scene of rtgo_set_scene (n <= RTGO_MAX_PRIMS) keeps a host copy of its records for its certificates: there, and only there, the
   context's n records are read back once.  The index check of rtgo_update_prims_device keeps one word per primitive on the device,
   allocated by a scene's first such call.
   Refusals are the twins', with the twins' codes.  Decided on the host, before any launch -- RTGO_E_INVALID: NULL ctx, d_prims or
   d_indices, a pointer that is not 4-byte aligned, unknown flag bits, d_aabbs given or NULL against the scene, n_updates above the
   scene's count (an index then repeats or lies beyond it); RTGO_E_UNSUPPORTED: n outside the twin's range; RTGO_E_STATE: no analytic
   scene; n_updates == 0 with a scene and known flags: RTGO_OK, nothing changes.  Found on the device, all RTGO_E_INVALID: an unknown
   type, a value among a record's 26 floats that is not finite, a model matrix the twin calls singular (the same determinant, in double,
   against the same bound), a box that is empty or not finite, an index >= the scene's count, an index named twice.  rtgo_last_error
   names the kind of fault and the number of the lowest offending entry (of an index named twice: of one of the entries that name it).
   A refused call leaves the scene as it was: every check of every entry runs, and its verdict is read, before anything of the scene is
   written -- for the set calls too, which keep the old scene when they refuse an array, as their twins do.  The one refusal known only
   after a build (RTGO_E_UNSUPPORTED, a tree deeper than the walk's stack) behaves as in the twin.  Synchronous. */
int rtgo_set_scene_device(rtgo_ctx* ctx, const void* d_prims, const void* d_aabbs, uint32_t n);
int rtgo_set_large_scene_device(rtgo_ctx* ctx, const void* d_prims, const void* d_aabbs, uint32_t n);
int rtgo_update_prims_device(rtgo_ctx* ctx, const void* d_indices, const void* d_prims, const void* d_aabbs, uint32_t n_updates, uint32_t flags);

/* What became of an update of rtgo_update_prims_device_async */
enum { RTGO_UPDATE_PENDING = 0, RTGO_UPDATE_APPLIED = 1, RTGO_UPDATE_REFUSED = 2 };
typedef struct rtgo_update_status {   /* 16 bytes */
    uint32_t state;   /* RTGO_UPDATE_* */
    uint32_t fault;   /* 0 none; 1 unknown type, 2 value not finite, 3 singular matrix, 4 bad box,
                         5 index beyond the scene, 6 index named twice, 7 box outside `reach` */
    uint32_t entry;   /* REFUSED: the lowest offending entry of the lowest-numbered kind that
                         rtgo_update_prims_device's message would name */
    uint32_t reserved;
} rtgo_update_status;

/* rtgo_update_prims_device with RTGO_UPDATE_REFIT over a scene of rtgo_set_large_scene or rtgo_set_large_scene_device, enqueued on the
   context's stream: it waits for nothing on the host -- not for the stream, a verdict, the refit's `changed` word or the root box -- so a
   loop of "step the simulation, refit, rtgo_launch" on one stream never drains the GPU.  d_indices, d_prims, d_aabbs:
   DEVICE memory of the context's device, caller-owned, 4-byte aligned, overlapping nothing of the context; the call reads them and never
   writes to them.  The caller's writes to them must be complete, or ordered on the context's stream (rtgo_set_stream), before the call;
   they must stay as they are until the update has run (rtgo_sync, or anything later on the stream).
   Decided on the host, at once; each returns its code, enqueues nothing and issues no ticket -- RTGO_E_INVALID: NULL ctx, d_prims,
   d_indices or ticket, a pointer that is not 4-byte aligned, d_aabbs given or NULL against the scene, n_updates above the scene's count,
   a reach that is not finite or has min > max on an axis; RTGO_E_STATE: no analytic scene; RTGO_E_UNSUPPORTED: a scene of rtgo_set_scene
   (its update is a whole build with host readers -- the emitter certificates, the quadric list, the grid -- and stays with the
   synchronous call).  n_updates == 0 with a large scene: RTGO_OK and *ticket = 0, nothing is enqueued.
   Every other call returns RTGO_OK and a ticket, and the six faults rtgo_update_prims_device finds on the device, with a seventh, are
   decided there later.  An update with a fault changes NOTHING of the scene -- no record, box, leaf or mark -- and says so through
   rtgo_update_prims_status; the kernels that write the scene read the check's verdict on the device first.  Updates enqueued after it
   are judged by their own verdicts alone.  An update without a fault leaves, bit for bit, what rtgo_update_prims_device leaves.
   reach replaces the read-back of the root box: a box inside which every updated primitive's box stays (the simulation's domain); NULL:
   the bounds the context holds now.  An entry whose box -- the given one, or without boxes the CubeBox rule's -- does not lie inside it is
   fault 7.  The context's bounds become the union of its bounds and reach, whatever the verdict: pixels, hits, shaded rays and the ray
   counts are unaffected (a pixel culled by the screen rectangle and a pixel traced to a miss are the same bits and the same count);
   rtgo_stats.rays_culled and the collect_stats == 2 counters may differ from those after rtgo_update_prims_device, and nothing else may.
   A later synchronous update that moves a box, or a set call, makes the bounds tight again.  The screen-rectangle mask, the pre-hashed
   seeds and the launch-time trial are dropped as by rtgo_update_prims.
   Allocations: a context's first call allocates its ring of 64 tickets (device words, their pinned copy, events), a scene's first call
   the index check's word per primitive; no other call allocates or frees anything. */
int rtgo_update_prims_device_async(rtgo_ctx* ctx, const void* d_indices, const void* d_prims, const void* d_aabbs, uint32_t n_updates,
                                   const rtgo_aabb* reach, uint64_t* ticket);

/* The state of a ticket of rtgo_update_prims_device_async.  Never blocks: one event query.  PENDING: the check has not finished.
   APPLIED: the check found no fault, and the update is done or ordered on the stream ahead of everything enqueued after its call.
   REFUSED: fault and entry say why; the scene is as it was.  Ticket 0 is APPLIED.  The context keeps its last 64 tickets: an older one, or
   one never issued, is RTGO_E_INVALID (as are a NULL ctx or out); a 65th update enqueued while 64 are in flight waits once for the oldest
   ticket's check, as rtgo_launch's ring of event pairs does.  After rtgo_sync every ticket the context keeps is APPLIED or REFUSED. */
int rtgo_update_prims_status(rtgo_ctx* ctx, uint64_t ticket, rtgo_update_status* out);

/* raygen SBT record: Renderer::CreateRayGen / SyncCameraToSbt (renderer.cpp:321-336, 719-731); device::CameraData */
int rtgo_set_camera(rtgo_ctx* ctx, const float eye[3], const float U[3], const float V[3], const float W[3]);

/* miss SBT record: Renderer::CreateMiss (renderer.cpp:386-398); device::MissData */
int rtgo_set_background(rtgo_ctx* ctx, const float rgb[3]);

/* Renderer::WriteLights (renderer.cpp:655-677); n <= RTGO_MAX_LIGHTS */
int rtgo_set_lights(rtgo_ctx* ctx, const rtgo_light* lights, int n);

/* Allocate context-owned output for `pixels` local pixels: float4 accumulation buffer + uchar4 image
   (cudaMalloc of accum_buffer, renderer.cpp:805-808, 742-746; CUDAOutputBuffer<uchar4>, renderer.cpp:820). */
int rtgo_resize(rtgo_ctx* ctx, size_t pixels);

/* Alternative to rtgo_resize: render into caller-owned DEVICE memory (e.g. buffers the multi-GPU driver hands to
   RCCL): d_accum = float4[pixels], d_image = uchar4[pixels].  The caller keeps ownership. */
int rtgo_bind_output(rtgo_ctx* ctx, void* d_accum, void* d_image, size_t pixels);

/* optixLaunch(pipeline, stream, params, ..., width, height, 1) (renderer.cpp:749-774).  Asynchronous, with one exception: once
   the launch-time trial of a job (same frame geometry, spp and mode) has all its timed launches in flight, the next launch of that
   job waits for them to finish, once, to pick the fastest candidate. */
int rtgo_launch(rtgo_ctx* ctx, const rtgo_frame* frame);

/* n_frames consecutive progressive frames of the frame's window / band share: frame->frame_count, +1, ..., +n_frames-1, over the
   scene, camera, lights and output the context holds now (a frame loop that presents every k-th frame only: no reference counterpart,
   renderer.cpp launches once per frame).  Accumulation buffer and image afterwards are, bit for bit, what n_frames calls of rtgo_launch
   with those frame_counts in turn leave.  Asynchronous on the context's stream.
   Every check of rtgo_launch applies, with its codes; n_frames == 0, or frame_count + n_frames passing 2^32: RTGO_E_INVALID, nothing is
   enqueued.  n_frames == 1 is rtgo_launch(ctx, frame).  A rank that owns no row of the window enqueues nothing and returns RTGO_OK.
   Lock-step launches (at most 16 spp) that take the fast walk over a tree render all their frames in ONE kernel launch: a pixel's
   frame f + 1 needs its frame f alone, so the wave that holds a strip of pixels renders the strip's frames back to back, keeps the
   running averages in registers and writes both outputs once.  Every other launch rtgo_launch accepts (more than 16 spp, the uniform
   grid, beyond the far-field guard, collect_stats, a scene of rtgo_set_large_scene) is n_frames launches enqueued back to back.
   A call with n_frames > 1 takes no part in the launch-time trial and never blocks: it times nothing and leaves the trial as it is.
   When the trial of this very job (rtgo_launch's key) has settled it uses that choice, otherwise the first candidate; pixels do not
   depend on the choice.  (A caller that must never block can therefore render single frames through rtgo_launch_frames' fallback
   only by asking for two at a time; n_frames == 1 is rtgo_launch, trial included.)
   rtgo_stats: the ray counts grow by the sum over the frames, launches by the kernel launches made (1, or n_frames). */
int rtgo_launch_frames(rtgo_ctx* ctx, const rtgo_frame* frame, uint32_t n_frames);

/* cudaStreamSynchronize + CUDA_SYNC_CHECK (CUDAOutputBuffer.h:247-250, renderer.cpp:773) */
int rtgo_sync(rtgo_ctx* ctx);

/* D2H of the output (CUDAOutputBuffer::getHostPointer, CUDAOutputBuffer.h:270-292).  bytes = pixels*4 / pixels*16. */
int rtgo_read_image(rtgo_ctx* ctx, void* host_uchar4, size_t bytes);
int rtgo_read_accum(rtgo_ctx* ctx, void* host_float4, size_t bytes);
/* H2D of an accumulation buffer (resume a progressive render; the reference never saves it: SURVEY section 5) */
int rtgo_write_accum(rtgo_ctx* ctx, const void* host_float4, size_t bytes);

/* ray counters and launch timing (no reference counterpart: the reference only shows an FPS overlay) */
int rtgo_get_stats(rtgo_ctx* ctx, rtgo_stats* out);
int rtgo_reset_stats(rtgo_ctx* ctx);

/* Debug/test access to what rtgo_set_scene or rtgo_set_large_scene built: nodes = 2n-1 records of 32 bytes
   {float bmin[3]; int32 left; float bmax[3]; int32 right} ... see DESIGN.md; inverses = n x 12 floats (rows 0..2). */
int rtgo_read_bvh(rtgo_ctx* ctx, void* host_nodes, size_t node_bytes, void* host_inverses, size_t inv_bytes,
                  void* host_aabbs, size_t aabb_bytes);

/* Multi-GPU presentation step (no reference counterpart: the reference is single-GPU).  d_gathered holds
   n_ranks compact band buffers back to back, rows_pad rows of w elements each (rank g's k-th owned row is row g*rows_pad + k:
   what the ranks' rtgo_bind_output buffers look like after a gather to one root); d_full receives window rows 0..h-1.
   elem_bytes = 4 (uchar4 image) or 16 (float4 accumulation).  Asynchronous on hip_stream (hipStream_t as void*; NULL = the
   context's stream); both pointers are device memory of ctx's device. */
int rtgo_assemble_bands(rtgo_ctx* ctx, void* hip_stream, const void* d_gathered, void* d_full, uint32_t w, uint32_t h,
                        uint32_t band_h, uint32_t n_ranks, uint32_t rows_pad, uint32_t elem_bytes);

/* ---- the "whitted" triangle path: cuda/whitted.cu + the mesh side of sutil/Scene.cpp (no glTF loading: the caller parses its files) ----
   One launch = one subframe of whitted.cu's pipeline: __raygen__pinhole (tea<4> seed, sub-pixel jitter from subframe 1 on, running
   average, gamma-2.2 image), __closesthit__radiance (GGX / Smith / Schlick direct lighting of point lights, one occlusion ray per
   light), __closesthit__occlusion, __miss__constant_radiance.  Camera and output buffers are the context's (rtgo_set_camera,
   rtgo_resize / rtgo_bind_output, rtgo_read_image / rtgo_read_accum). */
#define RTGO_MAX_TRIANGLES 8192

/* MaterialData::Pbr (cuda/MaterialData.h:43-52) without its three texture handles */
typedef struct rtgo_pbr {
    float base_color[4];
    float metallic;
    float roughness;
} rtgo_pbr;

/* Light::Point (cuda/Light.h:47-53) */
typedef struct rtgo_point_light {
    float color[3];
    float intensity;
    float position[3];
    int32_t falloff;   /* Light::Falloff; whitted.cu never reads it */
} rtgo_point_light;

/* sutil::Scene::addMesh + buildMeshAccels (sutil/Scene.cpp): one triangle mesh in world space = GeometryData::TriangleMesh
   (cuda/GeometryData.h:46-52; positions and optional vertex normals, 3 floats per vertex; 32-bit indices, 3 per triangle) with
   one material per triangle (material_of_triangle may be NULL: material 0).  Builds the triangle LBVH on the device.
   n_triangles <= RTGO_MAX_TRIANGLES (a larger mesh goes through rtgo_whitted_set_scene as one identity instance).  Synchronous. */
int rtgo_whitted_set_mesh(rtgo_ctx* ctx, const float* positions, const float* normals, uint32_t n_vertices, const uint32_t* indices,
                          const uint32_t* material_of_triangle, uint32_t n_triangles, const rtgo_pbr* materials, uint32_t n_materials);

/* GeometryData::TriangleMesh::texcoords (cuda/GeometryData.h:46-52): one (u, v) per vertex of the mesh set by rtgo_whitted_set_mesh, or
   NULL for none -- getLocalGeometry then takes the barycentrics as UV (cuda/LocalGeometry.h:88-102).  Call after rtgo_whitted_set_mesh
   (an instanced scene takes its texture coordinates per mesh in rtgo_whitted_set_scene: RTGO_E_STATE). */
int rtgo_whitted_set_texcoords(rtgo_ctx* ctx, const float* uv, uint32_t n_vertices);

/* One image of sutil::Scene::addImage + addSampler (sutil/Scene.cpp:478-538): 8-bit RGBA texels in HOST memory, row 0 first (glTF's
   v = 0 is the first row).  Sampled like the reference's cudaTextureObject_t: normalised coordinates, normalised float reads, no sRGB
   decode, and -- addSampler compares its CUDA enum arguments with GL constants, so whatever the glTF sampler says -- wrap addressing and
   bilinear filtering. */
typedef struct rtgo_texture {
    const void* rgba8;
    uint32_t width, height;
} rtgo_texture;

/* MaterialData::Pbr::base_color_tex / metallic_roughness_tex / normal_tex (cuda/MaterialData.h:43-52) of material `material` of the table
   given to rtgo_whitted_set_mesh or rtgo_whitted_set_scene; NULL = the material has no such texture (whitted.cu:264, 272, 288 test the
   handle).  The texels are copied.  Call after rtgo_whitted_set_mesh / rtgo_whitted_set_scene (which clear every texture). */
int rtgo_whitted_set_material_textures(rtgo_ctx* ctx, uint32_t material, const rtgo_texture* base_color,
                                       const rtgo_texture* metallic_roughness, const rtgo_texture* normal);

/* whitted::LaunchParams::lights (cuda/whitted.h:71); n <= RTGO_MAX_LIGHTS */
int rtgo_whitted_set_lights(rtgo_ctx* ctx, const rtgo_point_light* lights, uint32_t n);

/* whitted::LaunchParams::miss_color (cuda/whitted.h:72) */
int rtgo_whitted_set_miss_color(rtgo_ctx* ctx, const float rgb[3]);

/* optixLaunch of the whitted pipeline over width x height pixels for subframe `subframe_index` (whitted::LaunchParams,
   cuda/whitted.h:59-74), over whichever scene the context holds (rtgo_whitted_set_mesh or rtgo_whitted_set_scene).  Asynchronous on
   the context's stream; rays are added to rtgo_stats (rays_total, rays_occlusion).  = rtgo_whitted_launch_frame over the full image
   and one rank. */
int rtgo_whitted_launch(rtgo_ctx* ctx, uint32_t width, uint32_t height, uint32_t subframe_index);

/* One subframe of a window / row band of the image (no reference counterpart: whitted.cu's launch renders the whole image, one GPU).
   The fields mean what rtgo_frame's do.  Pixels are independent (seed tea<4>(y * image_width + x, subframe), the ray from the full
   image_width x image_height: whitted.cu:196-206), so the shares of a split put back together are the full frame bit for bit. */
typedef struct rtgo_whitted_frame {
    uint32_t image_width;      /* optixGetLaunchDimensions().x of the full image (seeds and ray directions) */
    uint32_t image_height;     /* optixGetLaunchDimensions().y */
    uint32_t subframe_index;   /* whitted::LaunchParams::subframe_index */
    uint32_t x0, y0, w, h;     /* window in global pixel coordinates; w = h = 0 means the full image */
    uint32_t band_h;           /* row-band height of the interleave inside the window (0 = 4) */
    uint32_t n_ranks, rank;    /* this context renders window rows r with (r / band_h) % n_ranks == rank; 0/1 = all.  Its k-th
                                  owned row is row k of a w-pixel-wide output (rtgo_assemble_bands puts the ranks' rows back) */
    uint32_t reserve_cus;      /* leave this many CUs' worth of workgroup slots to other streams (at most half of them, as rtgo_launch) */
} rtgo_whitted_frame;

/* optixLaunch of the whitted pipeline over the frame's share of the image, as rtgo_whitted_launch.  RTGO_E_INVALID: a window outside
   the image, rank >= n_ranks, w x rtgo_local_rows(h, band_h, n_ranks, rank) pixels beyond the output, or reserve_cus >= the device's
   CUs (nothing is enqueued).  A rank that owns no row of the window enqueues nothing and returns RTGO_OK.  Asynchronous. */
int rtgo_whitted_launch_frame(rtgo_ctx* ctx, const rtgo_whitted_frame* frame);

/* n_subframes consecutive subframes of the frame's window / band share: frame->subframe_index, +1, ..., +n_subframes-1, over the scene,
   camera, lights, miss colour and output the context holds now (an offline render of a still view, or a viewer that presents every
   k-th subframe once the camera rests: no reference counterpart, the reference launches once per subframe).  Accumulation buffer and
   image afterwards are, bit for bit, what n_subframes calls of rtgo_whitted_launch_frame with those indices in turn leave; a first index
   above 0 continues from the accumulation buffer as it is, index 0 does not read it.  Asynchronous on the context's stream.
   Every check of rtgo_whitted_launch_frame applies, with its codes; n_subframes == 0, or subframe_index + n_subframes passing 2^32:
   RTGO_E_INVALID, nothing is enqueued.  n_subframes == 1 is rtgo_whitted_launch_frame(ctx, frame).  A rank that owns no row of the
   window enqueues nothing and returns RTGO_OK.
   ONE kernel launch, whatever scene the context holds (one mesh or instances, clustered meshes among them): a pixel's subframe f + 1
   needs its own subframe f alone (whitted.cu:226-239: the running mean reads and writes accum_buffer[image_index] of the launch index
   only; the seed, :196-198, and the jitter, :200-206, depend on the pixel and the subframe index), so a wave gives each pixel of its tile
   several lanes, one subframe to a lane, and one of them folds the radiances into the mean in subframe order.  The 8-bit image is
   written once, from the last mean.
   rtgo_stats: the ray counts grow by the sum over the subframes, launches by 1; last_launch_ms is that launch. */
int rtgo_whitted_launch_frames(rtgo_ctx* ctx, const rtgo_whitted_frame* frame, uint32_t n_subframes);

/* ---- instanced meshes: sutil::Scene's two levels (one GAS per MeshGroup, buildMeshAccels; one OptixInstance per group in an IAS,
   buildInstanceAccel, sutil/Scene.cpp:985-1010) ---- */
#define RTGO_WHITTED_MAX_MESHES 256
#define RTGO_WHITTED_MAX_INSTANCES 8192
/* triangles of one mesh of an instanced scene, and of all its meshes together.  A mesh beyond RTGO_MAX_TRIANGLES is built as a
   clustered mesh: sorted in Morton order on the device, cut into clusters of consecutive triangles, and joined by a mid level over the
   clusters' boxes.  It renders bit for bit like the same triangles cut into contiguous identity instances of at most RTGO_MAX_TRIANGLES. */
#define RTGO_WHITTED_MAX_MESH_TRIANGLES (1 << 24)
#define RTGO_WHITTED_MAX_SCENE_TRIANGLES (1 << 26)

/* one GAS: GeometryData::TriangleMesh (cuda/GeometryData.h:46-52) in OBJECT space */
typedef struct rtgo_whitted_mesh {
    const float* positions;                /* 3 floats per vertex */
    const float* normals;                  /* 3 floats per vertex, or NULL (then N = Ng, LocalGeometry.h:113-116) */
    const float* texcoords;                /* 2 floats per vertex, or NULL (then UV = the barycentrics) */
    uint32_t n_vertices;
    const uint32_t* indices;               /* 3 per triangle */
    const uint32_t* material_of_triangle;  /* NULL: 0 */
    uint32_t n_triangles;                  /* <= RTGO_WHITTED_MAX_MESH_TRIANGLES (beyond RTGO_MAX_TRIANGLES: a clustered mesh) */
} rtgo_whitted_mesh;

/* one OptixInstance as Scene::buildInstanceAccel fills it (sutil/Scene.cpp:995-1005) */
typedef struct rtgo_whitted_instance {
    float transform[12];        /* row-major 3x4 object-to-world matrix (OptixInstance::transform) */
    uint32_t mesh;              /* index into the meshes array (the instance's traversableHandle) */
    uint32_t material_offset;   /* sbtOffset: a triangle's material is material_offset + material_of_triangle[t] */
} rtgo_whitted_instance;

/* A scene of n_meshes meshes drawn by n_instances instances, and one material table for all of them.  Checks every mesh as
   rtgo_whitted_set_mesh does, and every instance: a mesh index inside the array, material_offset + the mesh's largest material index
   inside the table, a finite and invertible transform (RTGO_E_INVALID).  More than RTGO_WHITTED_MAX_MESHES meshes or
   RTGO_WHITTED_MAX_INSTANCES instances, a mesh beyond RTGO_WHITTED_MAX_MESH_TRIANGLES, meshes beyond RTGO_WHITTED_MAX_SCENE_TRIANGLES
   together, or a structure deeper than the walk's stack (top level + mid level + deepest cluster of a clustered mesh):
   RTGO_E_UNSUPPORTED.  Builds both levels on the device; replaces the scene of rtgo_whitted_set_mesh (and that call replaces this
   one); clears every texture.  The closest hit is the smallest t, then the lowest (instance, triangle): an instanced scene renders
   like the concatenation of its instances.  Synchronous; every structure of the call -- the clusters of its clustered meshes (beyond
   RTGO_MAX_TRIANGLES) and its small meshes -- is built by one batched sequence of launches, one workgroup per structure, so the call
   takes time in proportion to its triangles (measured on an MI355X: 42 ms for a mesh of 1 000 000 triangles, of which 27 ms are the
   surface-area pass over its 245 clusters). */
int rtgo_whitted_set_scene(rtgo_ctx* ctx, const rtgo_whitted_mesh* meshes, uint32_t n_meshes, const rtgo_whitted_instance* instances,
                           uint32_t n_instances, const rtgo_pbr* materials, uint32_t n_materials);

/* New transforms, mesh choices or material offsets over the meshes and materials of the last rtgo_whitted_set_scene: rebuilds the top
   level only (meshes and clustered meshes stay as built).  Same checks and limits as rtgo_whitted_set_scene; a refused call leaves the
   scene as it was; textures stay.  Synchronous. */
int rtgo_whitted_set_instances(rtgo_ctx* ctx, const rtgo_whitted_instance* instances, uint32_t n_instances);

/* optixAccelBuild with OPTIX_BUILD_OPERATION_UPDATE: new vertex positions (and normals) for mesh `mesh` of the scene the context
   holds -- 0 for the mesh of rtgo_whitted_set_mesh, an index into the meshes of the last rtgo_whitted_set_scene otherwise.
   Indices, materials, texture coordinates, textures, instances and lights stay.  The structure keeps its topology and its boxes are
   refitted to the moved triangles (in an instanced scene the top level is rebuilt over the mesh's new box): no sort, no hierarchy,
   no surface-area sweep, a fraction of the time of setting the mesh again.  The frame is bit for bit that of a scene set afresh with
   the same vertices (any tree over the same triangles returns the same closest hit); what a refit cannot keep is the quality of the
   tree, so after a deformation that moves neighbouring triangles far apart the walk slows down and building the mesh again
   (rtgo_whitted_rebuild_meshes) pays.
   positions: n_vertices x 3 floats, copied; normals: the same, or NULL to keep the normals the mesh has.  RTGO_E_STATE: no whitted
   scene.  RTGO_E_INVALID: `mesh` beyond the scene's meshes, positions NULL, n_vertices not the mesh's own, non-finite data, normals
   for a mesh that was set without, an instance that now places the mesh beyond the float range.  RTGO_E_UNSUPPORTED: a clustered mesh
   (beyond RTGO_MAX_TRIANGLES: rtgo_whitted_update_meshes refits it), or a top level deeper than the walk's stack.  A refused call
   leaves the scene as it was.  Synchronous. */
int rtgo_whitted_update_mesh(rtgo_ctx* ctx, uint32_t mesh, const float* positions, const float* normals, uint32_t n_vertices);

/* One entry of rtgo_whitted_update_meshes: rtgo_whitted_update_mesh's arguments. */
typedef struct rtgo_whitted_mesh_update {
    uint32_t mesh;            /* as rtgo_whitted_update_mesh's `mesh` */
    const float* positions;   /* n_vertices x 3, copied */
    const float* normals;     /* the same, or NULL: keep the normals the mesh has */
    uint32_t n_vertices;
} rtgo_whitted_mesh_update;

/* rtgo_whitted_update_mesh for every entry of `updates`, as one transaction: every entry is checked before anything on the device
   changes, the instances are laid out again once and the top level is built once, over all the new mesh boxes -- a frame that moves k
   meshes pays for that once, not k times.  Clustered meshes (beyond RTGO_MAX_TRIANGLES) are accepted here: every cluster is refitted
   by one launch (one workgroup per cluster), then the mid level over the clusters' new boxes; topology, Morton order and cluster cut
   stay as built, and the frame is bit for bit that of a scene set afresh with the same vertices.  What stays is what stays under
   rtgo_whitted_update_mesh, and afterwards rtgo_whitted_set_instances, rtgo_whitted_update_mesh and this call work as after a fresh
   rtgo_whitted_set_scene.  n_updates == 0: RTGO_OK, nothing changes.  A scene of rtgo_whitted_set_mesh takes one entry, mesh 0.
   RTGO_E_STATE: no whitted scene.  RTGO_E_INVALID: `updates` NULL with n_updates > 0, a mesh index beyond the scene's meshes, a mesh
   named twice, positions NULL, n_vertices not the mesh's own, non-finite data, normals for a mesh that was set without, an instance
   that now places a mesh beyond the float range.  RTGO_E_UNSUPPORTED: a top level deeper than the walk's stack.  A refused call leaves
   the scene as it was, whichever entry it refuses (a clustered mesh's box is known only once it is refitted: its arrays are saved on
   the device first and put back).  Synchronous.  (rtgo_whitted_update_mesh keeps its own path and its refusal of clustered meshes;
   forwarding it to this call is left for later.) */
int rtgo_whitted_update_meshes(rtgo_ctx* ctx, const rtgo_whitted_mesh_update* updates, uint32_t n_updates);

/* optixAccelBuild with OPTIX_BUILD_OPERATION_BUILD for some meshes of the scene the context holds: every entry's mesh is built again
   over its new vertices -- a fresh Morton order, hierarchy and surface-area records, for a clustered mesh a fresh cluster cut and mid
   level -- in place, and the top level once over all the new boxes.  Afterwards the context holds what a fresh rtgo_whitted_set_scene
   (rtgo_whitted_set_mesh for a one-mesh scene) with the new vertices would hold, array for array; unlike that call it keeps the
   meshes not named, indices, triangle materials, texture coordinates, instances, lights, the miss colour and the textures.  Every
   structure of the call (all clusters of all named clustered meshes, the named small meshes) is built by one batched sequence of
   launches.  Arguments, entry struct and refusals are rtgo_whitted_update_meshes's: n_updates == 0: RTGO_OK, nothing changes; a scene
   of rtgo_whitted_set_mesh takes one entry, mesh 0.  RTGO_E_STATE: no whitted scene.  RTGO_E_INVALID: `updates` NULL with
   n_updates > 0, a mesh index beyond the scene's meshes, a mesh named twice, positions NULL, n_vertices not the mesh's own, non-finite
   data, normals for a mesh that was set without, an instance that now places a mesh beyond the float range.  RTGO_E_UNSUPPORTED: a
   structure deeper than the walk's stack (top level + mid level + deepest cluster).  A refused call leaves the scene as it was,
   whichever entry it refuses (depth and box are known only after the build: what it writes for a named mesh is saved on the device
   first and put back).  Afterwards rtgo_whitted_set_instances, rtgo_whitted_update_mesh, rtgo_whitted_update_meshes and this call
   work as after a fresh rtgo_whitted_set_scene.  Synchronous. */
int rtgo_whitted_rebuild_meshes(rtgo_ctx* ctx, const rtgo_whitted_mesh_update* updates, uint32_t n_updates);

/* rtgo_whitted_update_meshes (flags = RTGO_UPDATE_REFIT) or rtgo_whitted_rebuild_meshes (RTGO_UPDATE_REBUILD) for vertices that are
   already on the device (under OptiX the vertex buffers of a build input are device pointers): a skinning kernel's output, a
   PyTorch-ROCm tensor.  `updates` is a host array; the positions / normals of its entries are DEVICE memory of the context's device,
   n_vertices x 3 floats each (normals NULL: keep the normals the mesh has), caller-owned, 4-byte aligned, overlapping nothing of the
   context; the call reads them and never writes to them.  The caller's writes to them must be complete, or ordered on the context's
   stream (rtgo_set_stream), before the call.  Beyond NULL and alignment the call cannot tell whether a pointer is good: that the
   buffers are device memory of the sizes given is the caller's to vouch for, as in the ray-query calls.
   Afterwards the context holds, array for array, what the host-pointer twin holds after the same vertices, so frames,
   rtgo_whitted_trace_rays and rtgo_whitted_shade_rays are equal bit for bit; what the twin keeps stays (meshes not named, indices,
   triangle materials, texture coordinates, textures, instances, lights, miss colour), and every other update call works afterwards as
   after a fresh rtgo_whitted_set_scene.  A scene of rtgo_whitted_set_mesh takes one entry, mesh 0.
   No copy in proportion to a mesh crosses the host in either direction: the data is checked where it lies (every float of every
   entry, named by a triangle or not), the boxes of the small meshes are taken there through the context's indices (both by one pair of
   launches over all entries, 32 bytes per entry read back, one wait), the vertices move device to device, and all named small meshes
   are refitted by one launch (one workgroup per mesh).  What still crosses is what the twins read back per cluster or structure.
   Refusals are the twins'.  RTGO_E_STATE: no whitted scene.  RTGO_E_INVALID: NULL ctx, unknown flag bits, `updates` NULL with
   n_updates > 0, a mesh index beyond the scene's meshes, a mesh named twice, positions NULL, a pointer that is not 4-byte aligned,
   n_vertices not the mesh's own, normals for a mesh that was set without, non-finite data, an instance that now places a mesh beyond
   the float range.  RTGO_E_UNSUPPORTED: a structure deeper than the walk's stack.  n_updates == 0 with a scene and known flags:
   RTGO_OK, nothing changes.  A refused call leaves the scene as it was, whichever entry it refuses: every check of the entries and of
   their data runs before anything of the context is written, and a refusal known only after a clustered refit or a build puts the
   saved arrays back, as in the twins.  Synchronous. */
int rtgo_whitted_update_meshes_device(rtgo_ctx* ctx, const rtgo_whitted_mesh_update* updates, uint32_t n_updates, uint32_t flags);

/* rtgo_whitted_set_instances for instances that are already on the device (under OptiX the OptixInstance buffer of an IAS build input
   is a device pointer, sutil/Scene.cpp:985-1010): a rigid-body or particle step's output, a PyTorch-ROCm tensor.  d_instances is
   rtgo_whitted_instance[n_instances], 56 bytes each in the host struct's layout, DEVICE memory of the context's device, caller-owned,
   4-byte aligned, overlapping nothing of the context; the call reads it and never writes to it.  The caller's writes to it must be
   complete, or ordered on the context's stream (rtgo_set_stream), before the call.  Beyond NULL and alignment the call cannot tell
   whether the pointer is good: that it is device memory of the size given is the caller's to vouch for, as in
   rtgo_whitted_update_meshes_device.
   flags = RTGO_UPDATE_REBUILD (optixAccelBuild of the IAS with OPTIX_BUILD_OPERATION_BUILD): the twin of rtgo_whitted_set_instances.
   Afterwards the context holds, array for array, what that call holds after the same instances, so frames, rtgo_whitted_trace_rays and
   rtgo_whitted_shade_rays are equal bit for bit; what the twin keeps stays (meshes, clusters, materials, textures, lights, miss
   colour).  The new top level is built aside and swapped in only once all of it succeeded.
   flags = RTGO_UPDATE_REFIT (OPTIX_BUILD_OPERATION_UPDATE): n_instances must be the scene's count and every instance must name the mesh
   it names now; transforms and material offsets may change.  The top level keeps its topology, its leaf order and its depth; its
   records are refitted in place to the new instance boxes, and the per-instance records are rewritten.  Frames, closest hits and shaded
   rays are bit for bit those of a context that took the same instances through rtgo_whitted_set_instances (any tree over the same
   instances returns the same closest hit, lowest (instance, triangle) on ties); what a refit cannot keep is the quality of the tree, so
   after instances have moved far among each other the walk slows down and RTGO_UPDATE_REBUILD pays.
   Every instance is checked where it lies, in double and operation for operation as rtgo_whitted_set_instances checks it, and the
   InstShade records, world boxes and InstWalk records are made on the device; the rebuilt top level's leaf order is read where the
   build wrote it.  What crosses the host: a verdict of a few words, the build's (or refit's) nine meta words, the mesh table up
   (48 bytes per mesh), and the caller's n_instances x 56 bytes read back once (at most 458 KB) -- the allowance rtgo_set_scene_device
   takes for its host copy of the records: the mesh-update calls lay the instances out again from that copy.  Nothing else in proportion
   to n_instances crosses the host.  Every other update call works afterwards as after rtgo_whitted_set_instances.
   RTGO_E_INVALID: NULL ctx, unknown flag bits, d_instances NULL or not 4-byte aligned; an instance whose mesh index lies beyond the
   meshes, whose material_offset + the mesh's largest material index lies beyond the material table, whose transform is non-finite or
   not invertible, or that places its mesh beyond the float range (rtgo_last_error names the lowest such instance and the reason the
   twin would give); under RTGO_UPDATE_REFIT also another count than the scene's, or an instance that names another mesh.
   RTGO_E_STATE: no instanced scene (a scene of rtgo_whitted_set_mesh does not count).  RTGO_E_UNSUPPORTED: n_instances == 0 or beyond
   RTGO_WHITTED_MAX_INSTANCES; under RTGO_UPDATE_REBUILD a top level deeper than the walk's stack, known after the build.  Every other
   refusal is known before anything of the scene is written; a refused call leaves the scene as it was.  Synchronous. */
int rtgo_whitted_set_instances_device(rtgo_ctx* ctx, const void* d_instances, uint32_t n_instances, uint32_t flags);

/* rtgo_whitted_set_instances_device with RTGO_UPDATE_REFIT, enqueued on the context's stream: it waits for nothing on the host -- not for
   the stream, a verdict, the instances' read-back or the refit's grid words -- so a loop of "step the bodies, refit the top level,
   rtgo_whitted_launch" on one stream never drains the GPU ("The refit that waits for nothing").  d_instances: the twin's
   contract -- rtgo_whitted_instance[n_instances], DEVICE memory of the context's device, caller-owned, 4-byte aligned, overlapping
   nothing of the context, read and never written; the caller's writes to it complete, or ordered on the context's stream
   (rtgo_set_stream), before the call -- and one rule more: it must stay as it is until the update has run (rtgo_sync, or anything later
   on the stream).
   Decided on the host, at once; each returns its code, enqueues nothing and issues no ticket (*ticket is not written) --
   RTGO_E_INVALID: NULL ctx, d_instances or ticket, a pointer that is not 4-byte aligned, another count than the scene's;
   RTGO_E_STATE: no instanced scene (a scene of rtgo_whitted_set_mesh does not count); RTGO_E_UNSUPPORTED: n_instances == 0 or beyond
   RTGO_WHITTED_MAX_INSTANCES.
   Every other call returns RTGO_OK and a ticket, and the five faults the twin finds on the device are decided there later and reported
   by rtgo_whitted_refit_instances_status.  An update with a fault changes NOTHING of the scene -- no top-level record, no per-instance
   record, nothing of what the context keeps of the instances; the kernels that write the scene read the check's verdict on the device
   first.  Updates enqueued after it are judged by their own verdicts alone.  An update without a fault leaves, array for array, what
   the synchronous refit leaves after the same instances on the same scene: frames, rtgo_whitted_trace_rays, rtgo_whitted_shade_rays and
   the ray counters are equal bit for bit, and launches and ray queries enqueued after the call see the refitted top level.  Every
   synchronous call works afterwards as after the twin; the first that needs the instances on the host (a mesh update, a rebuild) waits
   for the stream -- as it does anyway -- and reads them back then.
   Allocations: a context's first call allocates its ring of 64 tickets (device words, their pinned copy, events), a scene's first call
   the staging the scene keeps until its top level or the scene is replaced (288 bytes per instance, 4 per top-level record, and 12 KB each for the mesh table and its pinned image);
   no other call allocates or frees anything. */
int rtgo_whitted_refit_instances_device_async(rtgo_ctx* ctx, const void* d_instances, uint32_t n_instances, uint64_t* ticket);

/* The state of a ticket of rtgo_whitted_refit_instances_device_async, in rtgo_update_status as it stands.  Never blocks: one event query.
   PENDING: the check has not finished.  APPLIED: it found no fault, and the update is done or ordered on the stream ahead of everything
   enqueued after its call.  REFUSED: the scene is as it was; fault is 1 a mesh index beyond the meshes, 2 an instance names another mesh
   than it names in the scene, 3 material offset + the mesh's largest material index beyond the table, 4 a non-finite or singular
   transform, 5 a box beyond the float range; entry is the instance rtgo_whitted_set_instances_device's message would name (the lowest
   offending one, of the lowest-numbered kind that names it).  The context keeps its last 64 tickets: an older one, one never issued and
   ticket 0 (never issued) are RTGO_E_INVALID, as are a NULL ctx or out; a 65th update enqueued while 64 are in flight waits once for
   the oldest ticket's check.  After rtgo_sync every ticket the context keeps is APPLIED or REFUSED.
   These tickets and rtgo_update_prims_device_async's come from two rings that count separately: a ticket of one call is RTGO_E_INVALID
   to the other call's status function unless that ring happens to hold the same number, which then names another update. */
int rtgo_whitted_refit_instances_status(rtgo_ctx* ctx, uint64_t ticket, rtgo_update_status* out);

/* rtgo_whitted_set_scene for meshes that are already on the device (under OptiX the vertex and index buffers of a build input are
   device pointers): a marching-cubes or simulation step's output, a PyTorch-ROCm tensor.  `meshes`, `instances` and `materials` are
   host arrays, as in the twin (they are small, and the context keeps a host copy of the instances anyway; a caller whose instances
   are on the device follows up with rtgo_whitted_set_instances_device).  The pointers inside each rtgo_whitted_mesh -- positions,
   normals, texcoords, indices, material_of_triangle, of the sizes the twin reads -- are DEVICE memory of the context's device,
   caller-owned, 4-byte aligned, overlapping nothing of the context; the call reads them and never writes to them, and two meshes may
   name the same buffer.  The caller's writes to them must be complete, or ordered on the context's stream (rtgo_set_stream), before
   the call.  Beyond NULL and alignment the call cannot tell whether a pointer is good: that the buffers are device memory of the sizes
   given is the caller's to vouch for, as in rtgo_whitted_update_meshes_device.
   Afterwards the context holds, array for array, what the twin holds after the same data, so frames, rtgo_whitted_trace_rays and
   rtgo_whitted_shade_rays are equal bit for bit, and every later call (rtgo_whitted_set_instances and its _device form, the mesh
   updates on host and device, rtgo_whitted_set_material_textures) behaves as after the twin.  What the twin drops is dropped alike: the
   old scene and every texture.
   No copy in proportion to a mesh crosses the host in either direction.  Every element of every array is checked where it lies, named
   by a triangle or not, and the meshes' boxes and largest material indices are taken there (one pair of launches over a table of all
   meshes; no vertex is read through an index that has not been compared with n_vertices first); then one launch packs every mesh into
   the context's arrays, and the builds are the twin's.  What crosses: the table up (64 bytes per mesh), a report back (32 bytes per
   mesh, one wait), and what the twin's builds read back per structure.
   Refusals are the twin's, with its codes and its messages under this call's name.  RTGO_E_INVALID: a NULL argument, a mesh without
   positions or indices, a pointer that is not 4-byte aligned; found on the device: an index beyond the vertex array, non-finite
   positions or normals, a non-finite texture coordinate, a material index beyond the table; every refusal of an instance.
   RTGO_E_UNSUPPORTED: every count and limit of the twin.  Where several faults are present the refusal is the one the twin gives: the
   first mesh at fault, and of its faults the first in the twin's order (counts, indices, vertex data, texture coordinates, materials).
   Every check of every mesh runs, and its report is read, before the old scene is dropped: a refused call leaves the scene and the
   caller's buffers as they were.  The one refusal known only after a build -- a structure deeper than the walk's stack -- leaves no
   scene, as in the twin.  Synchronous. */
int rtgo_whitted_set_scene_device(rtgo_ctx* ctx, const rtgo_whitted_mesh* meshes, uint32_t n_meshes, const rtgo_whitted_instance* instances,
                                  uint32_t n_instances, const rtgo_pbr* materials, uint32_t n_materials);

/* rtgo_whitted_set_mesh for a mesh that is already on the device: the one-mesh scene of rtgo_whitted_set_scene_device, under the
   same contract for d_positions, d_normals (or NULL), d_indices and d_material_of_triangle (or NULL) -- DEVICE memory of the context's
   device, caller-owned, 4-byte aligned, overlapping nothing of the context, read and never written, the caller's writes complete or
   ordered on the context's stream; beyond NULL and alignment the call cannot tell whether a pointer is good.  `materials` is a host
   array.  Limits (RTGO_MAX_TRIANGLES), refusals and what the context holds afterwards are rtgo_whitted_set_mesh's; the data is checked
   on the device before the old scene is dropped, and moves device to device.  Synchronous. */
int rtgo_whitted_set_mesh_device(rtgo_ctx* ctx, const void* d_positions, const void* d_normals, uint32_t n_vertices, const void* d_indices,
                                 const void* d_material_of_triangle, uint32_t n_triangles, const rtgo_pbr* materials, uint32_t n_materials);

/* rtgo_whitted_set_texcoords for coordinates that are already on the device: d_uv is n_vertices x 2 floats of DEVICE memory under the
   contract above (4-byte aligned: RTGO_E_INVALID otherwise), or NULL, which removes the coordinates.  State and count refusals are
   rtgo_whitted_set_texcoords's; the finite check runs on the device, before the old coordinates go.  Synchronous. */
int rtgo_whitted_set_texcoords_device(rtgo_ctx* ctx, const void* d_uv, uint32_t n_vertices);

/* ---- ray queries: optixTrace for rays of the caller's own (under OptiX the caller writes a raygen program; here it fills a buffer of
   rays -- picking, visibility between two points, a camera model of its own, baking -- and reads the hits back) ---- */

/* One ray, 32 bytes (2 x float4).  dir is used as given, not normalised; t is in units of dir (optixTrace's semantics).  A ray is INVALID
   when a component is not finite, dir == 0, tmin < 0, or tmax <= tmin (or NaN): it is answered with RTGO_HIT_INVALID and never walked. */
typedef struct rtgo_ray {
    float origin[3];
    float tmin;
    float dir[3];
    float tmax;
} rtgo_ray;

/* One answer, 32 bytes (2 x float4).  A hit is accepted iff tmin < t < tmax; of two accepted hits at the same t the lowest SBT index wins
   (analytic path), or the lowest (instance, triangle) (triangle path): the rules of the render kernels' walks, which these calls run.
     analytic hit   t, prim = SBT index,                        instance = -1,             u = v = 0,        n = world-space normal, not normalised
     triangle hit   t, prim = the mesh's own triangle index,    instance (0 for a mesh of rtgo_whitted_set_mesh), u, v = barycentrics, n = 0
     miss           t = the ray's tmax, prim = RTGO_HIT_MISS,    everything else 0
     invalid ray    prim = RTGO_HIT_INVALID,                     everything else 0 */
typedef struct rtgo_hit {
    float t;
    int32_t prim;
    int32_t instance;
    float u, v;
    float n[3];
} rtgo_hit;

/* flags.  RTGO_TRACE_ANY_HIT: stop at the first accepted hit (OPTIX_RAY_FLAG_TERMINATE_ON_FIRST_HIT): rely on hit-or-miss only, the
   other fields describe SOME accepted hit.  (The analytic path answers with its closest walk: the reference's occlusion rays are
   closest-hit rays too, kernel.cu:539-549.) */
enum { RTGO_TRACE_CLOSEST = 0, RTGO_TRACE_ANY_HIT = 1 };
#define RTGO_HIT_MISS    (-1)
#define RTGO_HIT_INVALID (-2)

/* Trace n rays against the scene of rtgo_set_scene / rtgo_set_large_scene.  d_rays = rtgo_ray[n], d_hits = rtgo_hit[n]: DEVICE memory of
   the context's device, 16-byte aligned, caller-owned, not overlapping.  Asynchronous on the context's stream; needs no camera, lights
   or output.  RTGO_E_INVALID: a NULL or misaligned pointer, unknown flag bits, n > 1 << 30; RTGO_E_STATE: no such scene; n == 0:
   RTGO_OK, nothing is enqueued or written.  rtgo_stats: rays_total grows by n (with RTGO_TRACE_ANY_HIT rays_occlusion too); launches,
   last_launch_ms, last_variant and the launch-time trial are left alone.  Every ray takes the canonical walk.
   The primitives are the reference's intersection programs as the renders run them (kernel.cu:250-416): they report only t above a small
   threshold of their own (1e-4, a cylinder 1e-3; units of dir), a rectangle from its front side only, a sphere at its near root only. */
int rtgo_trace_rays(rtgo_ctx* ctx, const void* d_rays, void* d_hits, uint32_t n, uint32_t flags);

/* The same over the scene of rtgo_whitted_set_mesh / rtgo_whitted_set_scene.  The answer is the brute force over the triangle test
   (closest t, lowest (instance, triangle) on ties) except for that test's phantom hits: where a ray lies within rounding of a triangle's
   plane, or the triangle is a sliver of aspect ~1e4, the float32 test can accept a hit on a ray that does not meet the triangle's bounds;
   the walk, which culls by boxes, may then report the next hit instead. */
int rtgo_whitted_trace_rays(rtgo_ctx* ctx, const void* d_rays, void* d_hits, uint32_t n, uint32_t flags);

/* Shade n rays of the caller's own against the scene of rtgo_whitted_set_mesh / rtgo_whitted_set_scene: __closesthit__radiance and
   __miss__constant_radiance (whitted.cu:243-337) behind a raygen program that is the caller's -- an orthographic or panoramic camera, a
   stereo pair, a reflection or light probe, a baked lightmap.  d_rays = rtgo_ray[n], d_accum = float4[n], d_image = uchar4[n] or NULL:
   DEVICE memory of the context's device, caller-owned, rays and accum 16-byte aligned, the image 4-byte aligned.  Asynchronous on the
   context's stream.  Needs a whitted scene only: no camera, no output buffer; lights never set are zero lights; the miss colour is the
   context's (rtgo_whitted_set_miss_color).  Per ray i:
     invalid ray (rtgo_ray's rule)   sample_index == 0: accum[i] = (0,0,0,0) and image[i] = (0,0,0,0); sample_index > 0: both are left
                                     untouched.  It is never walked.
     valid ray                       result = the miss colour when no hit lies in tmin < t < tmax (the closest walk of the render kernels,
                                     ties broken as there), else the radiance shaded at that hit with the ray's dir, as given, for the
                                     viewing direction.  The occlusion rays are the shader's own: unit direction, 0.001 .. Ldist - 0.001.
                                     acc = result when sample_index == 0, else prev + (result - prev) * (1 / (sample_index + 1)) with prev =
                                     accum[i].xyz (whitted.cu:226-239: the fold of the launches, in float32, operation for operation).
                                     accum[i] = (acc, 1); image[i] = make_color(acc) (:164-173) when d_image is given.
   So the pinhole rays of subframe s (origin the eye, tmin 0.01, tmax 1e16) with sample_index = s leave rtgo_whitted_launch's two buffers,
   bit for bit.  t and the hit's identity are not returned: they come from rtgo_whitted_trace_rays, which runs the same walk.
   RTGO_E_INVALID: NULL ctx, d_rays or d_accum, a misaligned pointer, n > 1 << 30; RTGO_E_STATE: no whitted scene (an analytic scene alone
   does not count); n == 0: RTGO_OK.  In all of these nothing is enqueued or written.  rtgo_stats: rays_total grows by n plus the occlusion
   rays the shader sent, rays_occlusion by those occlusion rays; launches, last_launch_ms and last_variant are left alone, and so are the
   render launches' tile queue and its parity: launches and these calls may alternate freely. */
int rtgo_whitted_shade_rays(rtgo_ctx* ctx, const void* d_rays, void* d_accum, void* d_image, uint32_t n, uint32_t sample_index);

/* What a launch's rtgo_frame says about shading, for rays of the caller's own (rtgo_shade_rays).  16 bytes. */
typedef struct rtgo_shade_options {
    int32_t  max_trace_depth;  /* Params::maxTraceDepth for these rays, [0, 5] */
    uint32_t path_tracing;     /* Params::enablePathTracing, 0 or 1 */
    uint32_t use_ambient;      /* Params::useAmbientLight,  0 or 1 */
    uint32_t sample_index;     /* Params::frameCount of the fold (kernel.cu:239-246) */
} rtgo_shade_options;

/* Shade n rays of the caller's own against the scene of rtgo_set_scene / rtgo_set_large_scene: __closesthit__ch,
   __closesthit__full_occlusion and __miss__ms (kernel.cu:419-549) behind a raygen program that is the caller's -- a panoramic or
   orthographic camera, a light probe, a stereo pair, a baked lightmap.  One ray is one sample of the reference: a trace(...) call of
   __raygen__rg at depth 0.  d_rays = rtgo_ray[n], d_seeds = uint32[n] or NULL, d_accum = float4[n], d_image = uchar4[n] or NULL: DEVICE
   memory of the context's device, caller-owned, rays and accum 16-byte aligned, seeds and image 4-byte aligned.  Asynchronous on the
   context's stream.  Needs an analytic scene, and in distributed mode (path_tracing == 0) the context's surface lights; no camera, no
   output buffer; the miss colour is the context's (rtgo_set_background).
     seed of ray i                   d_seeds[i], handed to the path as trace hands over `seed`: by value, after whatever the caller's
                                     raygen drew.  d_seeds == NULL: tea<16>(i, sample_index), the raygen's own rule with the ray's index
                                     for the pixel's and no jitter draws.
     invalid ray                     rtgo_ray's rule, and in addition dir must be a unit vector, |dot(dir, dir) - 1| <= 1e-5 (the shader
                                     places a hit at o + t d in path mode and at o + t normalize(d) in distributed mode: one point only
                                     for unit directions).  sample_index == 0: accum[i] = (0,0,0,0) and image[i] = (0,0,0,0);
                                     sample_index > 0: both are left untouched.  It is never walked.
     valid ray                       result = the payload of the path that starts with this ray over tmin < t < tmax: the render kernels'
                                     closest walk and ties, the three shading modes, their occlusion rays, bounces while depth <
                                     max_trace_depth; children run over [rayEpsilon, 1e6].  cur = (0 + result) * (1 / 1), the launch's
                                     arithmetic for one sample; acc = cur when sample_index == 0, else prev + (cur - prev) *
                                     (1 / (sample_index + 1)) in float32 with prev = accum[i].xyz (kernel.cu:239-246, operation for
                                     operation).  accum[i] = (acc, 1); image[i] = make_color(acc) (:90-98) when d_image is given.
   So the rays __raygen__rg makes for sqrt_spp 1 and frame f (origin the eye, tmin 0.05, tmax 1e16), with the seeds as they stand after
   the two jitter draws and sample_index = f, leave rtgo_launch's two buffers, bit for bit, in all three modes.  More than one sample
   per result is not offered (the in-order sum of sqrt_spp > 1): a caller folds samples through sample_index.
   RTGO_E_INVALID: NULL ctx, d_rays, d_accum or opt, a misaligned pointer, n > 1 << 30, path_tracing or use_ambient above 1;
   RTGO_E_UNSUPPORTED: max_trace_depth outside [0, 5]; RTGO_E_STATE: no analytic scene (a whitted scene alone does not count),
   distributed mode without a surface light; n == 0 after the checks: RTGO_OK.  In all of these nothing is enqueued or written and no
   counter moves.  rtgo_stats: rays_total grows by n plus the bounce and occlusion rays the paths sent, rays_occlusion by those occlusion
   rays; launches, last_launch_ms, last_variant, launches_trial, the launch-time trial and the render launches' queues are left alone:
   launches and these calls may alternate freely.  Every ray takes the canonical walk. */
int rtgo_shade_rays(rtgo_ctx* ctx, const void* d_rays, const void* d_seeds, void* d_accum, void* d_image, uint32_t n,
                    const rtgo_shade_options* opt);

/* number of window rows a rank owns under the band interleave (pure host arithmetic) */
uint32_t rtgo_local_rows(uint32_t h, uint32_t band_h, uint32_t n_ranks, uint32_t rank);

uint32_t rtgo_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
