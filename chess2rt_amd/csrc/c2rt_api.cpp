/*
 * c2rt_api.cpp — implementation of the C ABI in include/c2rt.h: context,
 * upload of a planned scene (scene_plan.h: SoA tables -> scalar-loadable records in HBM),
 * frame / pixel-probe launches, the ray and plane queries, strip de-interleave and display encode.
 *
 * The hit, shading, occlusion, gather and path planes are one code path: each family is described once (Family<S>: sample
 * sizes, the words of its messages, its options and their refusals) and its entry points are one-line calls of the
 * four faces frame_planes_device / frame_planes_host / ray_planes_device / ray_planes_host.
 *
 * There is no CPU fallback anywhere in this file: without a usable HIP
 * device every entry point fails with C2RT_ERR_NO_DEVICE / C2RT_ERR_HIP.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "c2rt_query.h"
#include "c2rt_denoise.h"
#include "c2rt_denoise_variance.h"
#include "c2rt_temporal.h"
#include "c2rt_paths_counted.h"
#include "scene_plan.h"

using namespace c2rt;

constexpr int kMaxChunks = 16;     /* row chunks of a host-output frame */

/* Per-frame scratch a launch writes before it reads it — the tile-mask table (pre-pass kernel) and the nested-CSG
 * retry list — exists once per STREAM the context has rendered on (up to kScratchSlots of them), keyed by the
 * stream handle (compared, never dereferenced).  Frames on one stream are in order and share a slot; frames on
 * different streams touch different slots, so they need no ordering at all: no event per frame (an event record
 * is a ~2 us gap in the queue: 6 % of a 1080p lecture4 frame) and frames of one context may overlap.  A 17th
 * stream recycles the least recently used slot after a device sync (the one place a single-frame call can block).
 * A batch (c2rt_render_frames_device) uses the same slot with the tables multiplied: n_frames mask tables and retry
 * lists side by side in the same two allocations (a single frame on that stream uses the first of each; the stream
 * orders them), plus the device table of the frames' parameter blocks.  Everything grows, nothing shrinks. */
constexpr int kScratchSlots = 16;
struct FrameScratch {
    const void *key = nullptr;
    bool used = false;
    uint64_t tick = 0;
    uint32_t *tile_masks = nullptr; /* RenderParams::tile_masks: 4 words per tile of the frame's local rows, x 2 tables */
    size_t tile_mask_entries = 0;
    uint32_t *retry_list = nullptr; /* RenderParams::retry_list: [0] count, then tile (block) indices */
    size_t retry_words = 0;
    /* batches: one RenderParams per frame (twice for nested CSG: first pass, retry pass), then one BatchCull per
     * frame, then (c2rt_render_frames_posed) the node, light and shadow-rectangle tables of the frames whose pose
     * changes them, then (c2rt_render_frames_adaptive) one refinement block per frame; uploaded per call with one
     * stream-ordered copy from ctx->batch_host.  A hit-plane batch (c2rt_render_frames_hits) keeps its own table here
     * instead: one block per frame, then the posed frames' node and light tables (hit_batch_table) */
    char *batch_table = nullptr;
    size_t batch_bytes = 0;
};

/* Environment hooks (A/B measurement and test knobs: C2RT_EXACT, C2RT_DEBUG_CULL, C2RT_CSG_FIRST_CAP,
 * C2RT_HOST_DIRECT_STORE) exist in the DIAGNOSTICS build only — chess2rt_amd/libc2rt_diag.so, this file compiled with
 * -DC2RT_DIAG=1 over the same kernel objects (Makefile).  The product library reads no environment variable: a
 * drop-in renderer does not change kernels on a stray variable (tests/test_abi_exports.py checks that libc2rt.so
 * does not even import getenv). */
#ifndef C2RT_DIAG
#define C2RT_DIAG 0
#endif
#if C2RT_DIAG
static const char *diag_env(const char *name) { return std::getenv(name); }
#else
static constexpr const char *diag_env(const char *) { return nullptr; }
#endif

/* the planner's diagnostics switches (scene_plan.h: DiagKnobs), read once; all off in the product library */
static const DiagKnobs &diag_knobs()
{
    static const DiagKnobs k = [] {
        DiagKnobs v;
        if (const char *e = diag_env("C2RT_EXACT")) v.exact = e[0] == '1';
        if (const char *e = diag_env("C2RT_DEBUG_CULL")) v.debug_cull = std::atoi(e);
        if (const char *e = diag_env("C2RT_CSG_FIRST_CAP")) v.csg_first_cap = std::atoi(e);
        if (v.debug_cull) std::fprintf(stderr, "libc2rt: diagnostics hook C2RT_DEBUG_CULL=%d is active (culling partly disabled; frames are unchanged, slower)\n", v.debug_cull);
        if (v.csg_first_cap > 0) std::fprintf(stderr, "libc2rt: test hook C2RT_CSG_FIRST_CAP=%d is active (first-pass CSG hit stacks shrunk; frames are unchanged, nested-CSG scenes are slower)\n", v.csg_first_cap);
        return v;
    }();
    return k;
}

/* C2RT_DEBUG_CULL bit 9 (diagnostics build): no CsgOp is decided by csg_certain.h — every plan this library makes loses
 * its kCsgCertain flags (frames are unchanged, slower).  Bit 10: no tile goes through lean::csg_tile — every plan loses its
 * kNodeCsgTile flags.  Called on every fresh plan, so that plans stay comparable. */
static void apply_plan_knobs(ScenePlan &plan)
{
    if (diag_knobs().debug_cull & 512) drop_csg_certain(plan);
    if (diag_knobs().debug_cull & 1024) drop_csg_tile(plan);
}

struct c2rt_ctx {
    int device = 0;
    /* c2rt_init_multi: the further device slots of this (lead) context, each a complete
     * single-device context of its own; empty for c2rt_init */
    std::vector<c2rt_ctx *> peers;
    bool peer_mapped = true;       /* (peer slot) can store into the lead device's memory */
    hipEvent_t ev_ready = nullptr, ev_done = nullptr; /* cross-device ordering of device-output frames */
    uint64_t scene_gen = 0;        /* c2rt_scene_generation */
    std::string err;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;              /* D2H of finished chunks */
    hipEvent_t chunk_done[kMaxChunks] = {};
    std::vector<std::pair<float *, size_t>> pinned; /* c2rt_pin_host_buffer */

    bool has_scene = false;
    ScenePlan plan;                /* the uploaded scene (scene_plan.h); meaningful while has_scene */
    SceneCopy scene;               /* its description without the texels: what c2rt_update_scene patches and plans again */
    DeviceTables dev;              /* where its tables live on this device */
    uint32_t sphere_flags_mask = ~0u; /* ANDed into every SphereNode::flags (diagnostics: c2rt_debug_sphere_cull) */

    float *frame = nullptr;        /* staging frame for host-output renders */
    size_t frame_floats = 0;
    unsigned long long *counters = nullptr; /* [0..2]: RenderParams::ray_counters (reset per counted frame); [3]: RenderParams::redo_counter (cumulative); [4]: redo_counter[1], ground tiles that left the short chain (cumulative); [5]: redo_counter[2], sphere-interior tiles handed back to the general path (cumulative); [6]: redo_counter[3], ground-and-CsgOp tiles handed back likewise (cumulative); [7]: redo_counter[4], the tiles lean::csg_tile rendered (cumulative; counted by the lane-statistics library only) */
    c2rt_trace_result *probe = nullptr;
    uint8_t *srgb_lut = nullptr;   /* [4097] */
    FrameScratch scratch[kScratchSlots];
    uint64_t scratch_tick = 0;
    /* host image of a batch's device table.  Pageable on purpose: a stream-ordered copy from pageable memory has
     * read its source when the call returns, so the next batch call may overwrite it — no ring, no event */
    std::vector<char> batch_host;
    bool counters_valid = false;
    /* The ray counters are the one per-frame resource shared by all streams: COUNTED frames (opts->count_rays, a
     * test / diagnostics mode) enqueued without a host sync are ordered among themselves and against the counter
     * read-back by ev_inflight, recorded on the caller's stream behind such a frame (the next counted frame waits
     * for it on the device, the blocking entry points and c2rt_get_ray_stats on the host).  The library never
     * keeps a caller's stream handle for use: the stream may be destroyed the moment the call returns.
     * has_inflight: ev_inflight has been recorded and not yet waited for by the host. */
    hipEvent_t ev_inflight = nullptr;
    bool has_inflight = false;
};

namespace {

int fail(c2rt_ctx *ctx, int status, const char *fmt, ...)
{
    if (ctx) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        ctx->err = buf;
    }
    return status;
}

#define HIP_TRY(ctx, call)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) return fail(ctx, C2RT_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

template <typename T>
int upload(c2rt_ctx *ctx, T **dst, const std::vector<T> &src)
{
    if (*dst) { (void)hipFree(*dst); *dst = nullptr; }
    const size_t bytes = (src.empty() ? 1 : src.size()) * sizeof(T);
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(dst), bytes));
    if (!src.empty()) HIP_TRY(ctx, hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return C2RT_OK;
}


/* convertTo8bit_sRGB — rt/color.d:194-207 (note the 12.02) and the 4097-entry
 * cache built by the module constructor rt/color.d:224-228 */
void build_srgb_lut(uint8_t *lut)
{
    for (int i = 0; i < 4097; ++i) {
        float x = i / 4096.0f;
        uint8_t v;
        if (x <= 0) v = 0;
        else if (x >= 1) v = 255;
        else {
            if (x <= 0.0031308f) x = x * 12.02f;
            else x = (float)(1.055 * std::pow((double)x, 1 / 2.4) - 0.055);
            v = (uint8_t)(int)std::floor(x * 255.0f);
        }
        lut[i] = v;
    }
}

int check_frame_args(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *o)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (!cam || !o) return fail(ctx, C2RT_ERR_INVALID_ARG, "null camera or options");
    if (!ctx->has_scene) return fail(ctx, C2RT_ERR_NO_SCENE, "no scene uploaded");
    return check_frame(cam, o, ctx->err);
}

void frame_params(const c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *o, RenderParams &p)
{
    fill_params(ctx->plan, ctx->dev, diag_knobs(), cam, o, p);
}

/* the scratch slot of `stream` (see FrameScratch); never fails: the least recently used slot is recycled after a
 * device sync (whatever still reads its tables has finished then) */
FrameScratch &scratch_for(c2rt_ctx *ctx, hipStream_t stream)
{
    const void *key = static_cast<const void *>(stream);
    FrameScratch *pick = nullptr;
    for (FrameScratch &f : ctx->scratch)
        if (f.used && f.key == key) { pick = &f; break; }
    if (!pick)
        for (FrameScratch &f : ctx->scratch)
            if (!f.used) { pick = &f; break; }
    if (!pick) {
        pick = &ctx->scratch[0];
        for (FrameScratch &f : ctx->scratch)
            if (f.tick < pick->tick) pick = &f;
        (void)hipDeviceSynchronize();
    }
    pick->used = true;
    pick->key = key;
    pick->tick = ++ctx->scratch_tick;
    return *pick;
}

/* grows one of a scratch slot's allocations to `want` elements (never shrinks; hipFree waits for whatever still reads it) */
template <typename T>
hipError_t grow_scratch(T **buf, size_t *have, size_t want, size_t elem_bytes)
{
    if (want <= *have) return hipSuccess;
    if (*buf) { (void)hipFree(*buf); *buf = nullptr; *have = 0; }
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(buf), want * elem_bytes);
    if (e == hipSuccess) *have = want;
    return e;
}

/* The first pass's CSG hit-stack capacity.  Test hook (diagnostics build only): C2RT_CSG_FIRST_CAP=<entries> shrinks
 * it so that the overflow -> retry path runs on ordinary scenes (tests/test_gpu_parity.py); never below 1, never
 * above full. */
int first_cap(int levels, const DiagKnobs &k)
{
    if (k.csg_first_cap > 0 && levels >= 2) return k.csg_first_cap < kCsgFullCap(levels) ? k.csg_first_cap : kCsgFullCap(levels);
    return kCsgFirstCap(levels);
}

/* What one frame like `p` needs of a scratch slot: the entries of a mask table over its local rows (0: the frame has
 * no culling rectangles, hence no table) and the blocks its retry list must hold. */
void frame_needs(RenderParams &p, size_t &entries, size_t &blocks)
{
    p.mask_rows = p.local_rows;
    entries = p.n_cull && p.local_rows ? tile_mask_entries(p) : 0;
    blocks = padded_grid_blocks(p.tiles_y, p.blocks_x);
}

/* Wires frame i of the frames that share scratch slot `sc` (a single frame: i = 0; a batch: n tables and lists side by
 * side, frame_needs of any of them; `plan`: the frame's scene, the context's own unless the frame is posed) into its
 * filled parameter block: first-pass stack capacity, redo counter, mask
 * table over the local rows [row_offset, row_offset + local_rows), retry list.  cull: the tests its pre-pass is given
 * (void_flags_mask: ANDed into every VoidNode::flags, ~0u for frames; the context's sphere_flags_mask likewise).
 * This is the one place a frame's launch state is decided: batch frame i gets the bits of the single-frame call. */
void wire_frame(const c2rt_ctx *ctx, const ScenePlan &plan, RenderParams &p, const FrameScratch &sc, size_t i, size_t entries,
                size_t blocks, uint32_t void_flags_mask, BatchCull &cull)
{
    const int levels = plan.csg_levels;
    p.csg_cap = levels == 0 ? 0u : (uint32_t)first_cap(levels, diag_knobs());
    p.retry_mode = 0;
    p.redo_counter = ctx->counters + 3;
    p.mask_row0 = p.row_offset;
    p.mask_rows = p.local_rows;
    const bool masks = entries && p.n_cull;
    p.tile_masks = masks ? sc.tile_masks + i * entries * 8 : nullptr;
    p.mask_entries = masks ? (uint32_t)entries : 0u;
    cull.v = void_cull_of(plan, p, void_flags_mask);
    cull.s = sphere_cull_of(plan, diag_knobs(), p, ctx->sphere_flags_mask);
    cull.d = dark_cull_of(plan, diag_knobs(), p);
    if (levels >= 2) {
        p.retry_list = sc.retry_list + i * (blocks + 1);
        p.retry_max = (uint32_t)blocks;
    }
}

/* A single frame's scratch, wiring and mask pre-pass: the tiles' culling masks for the local rows [p.row_offset,
 * p.row_offset + p.local_rows), by the pre-pass kernel, in front of the frame kernel on the same stream (a no-op for
 * frames without culling rectangles).  cull_out (nullable): what the pre-pass was given.  Returns a hipError_t. */
int prepare_frame(c2rt_ctx *ctx, RenderParams &p, hipStream_t stream, uint32_t void_flags_mask = ~0u, BatchCull *cull_out = nullptr)
{
    FrameScratch none; /* a frame that needs no scratch claims no slot */
    const bool nested = ctx->plan.csg_levels >= 2;
    size_t entries, blocks;
    frame_needs(p, entries, blocks);
    FrameScratch &sc = entries || nested ? scratch_for(ctx, stream) : none;
    hipError_t e = grow_scratch(&sc.tile_masks, &sc.tile_mask_entries, entries, 8 * sizeof(uint32_t));
    if (e == hipSuccess && nested) e = grow_scratch(&sc.retry_list, &sc.retry_words, blocks + 1, sizeof(uint32_t));
    if (e != hipSuccess) return (int)e;
    BatchCull cull;
    wire_frame(ctx, ctx->plan, p, sc, 0, entries, blocks, void_flags_mask, cull);
    if (cull_out) *cull_out = cull;
    return entries ? launch_tile_masks(p, cull.v, cull.s, cull.d.n ? ctx->dev.dark : nullptr, sc.tile_masks, stream) : 0;
}

/* The frame launch of prepared parameters (a chunked frame: once per chunk, over the chunk's rows).  Scenes with
 * nested CsgOps (depth >= 2) run the kernel with a reduced hit-stack capacity (three waves per SIMD instead of one at
 * depth 4) and then, on the same stream, the full-capacity relaunch over the tiles that overflowed it — none, for trees
 * whose primitives yield their two hits (RenderParams::retry_list; c2rt_kernels.hip, csg_intersect).  Returns a
 * hipError_t. */
int launch_prepared(const c2rt_ctx *ctx, RenderParams &p, const KernelVariant &v, hipStream_t stream)
{
    const int levels = ctx->plan.csg_levels;
    if (levels < 2) return launch_render(p, v, stream);
    const hipError_t e = hipMemsetAsync(p.retry_list, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return (int)e;
    const uint32_t first = p.csg_cap;
    int r = launch_render(p, v, stream);
    if (r != 0 || (int)first >= kCsgFullCap(levels)) return r;
    p.retry_mode = 1;
    p.csg_cap = (uint32_t)kCsgFullCap(levels);
    r = launch_render(p, v, stream);
    p.retry_mode = 0;
    p.csg_cap = first;
    return r;
}

/* One frame: the n == 1 case of wire_frame, launched through the kernel-argument kernels. */
int launch_frame(c2rt_ctx *ctx, RenderParams &p, const KernelVariant &v, hipStream_t stream)
{
    const int e = prepare_frame(ctx, p, stream);
    return e != 0 ? e : launch_prepared(ctx, p, v, stream);
}

int render_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, float *out_dev,
                  hipStream_t stream)
{
    RenderParams p;
    frame_params(ctx, cam, opts, p);
    p.out = out_dev;
    ctx->counters_valid = false;
    if (opts->count_rays) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->counters, 0, 3 * sizeof(unsigned long long), stream));
        p.ray_counters = ctx->counters;
    }
    if (p.local_rows == 0) return C2RT_OK;
    const int e = launch_frame(ctx, p, variant_of(ctx->plan, cam), stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "render kernel launch: %s", hipGetErrorString((hipError_t)e));
    if (opts->count_rays) ctx->counters_valid = true;
    return C2RT_OK;
}

/* The hit-plane and refinement kernels' settings on top of a frame's filled parameter block (hit_params;
 * render_frames_device's refinement blocks): exact:: arithmetic, full-capacity hit stack, no culling rectangles (every
 * mask all ones), no ground node, one tap.  The CSG depth is the geometries', which no pose changes. */
void hit_settings(const c2rt_ctx *ctx, RenderParams &p)
{
    p.force_exact = 1;
    p.taps = 1;
    p.seed = 0;
    p.n_cull = 0;
    p.n_cull_lights = 0;
    p.ground_node = -1;
    p.row_group_start = 0;
    p.csg_cap = ctx->plan.csg_levels == 0 ? 0u : (uint32_t)kCsgFullCap(ctx->plan.csg_levels);
    p.redo_counter = ctx->counters + 3;
}

/* What turns a one-tap batch into an adaptive one (c2rt_render_frames_adaptive*): the flags of frame i at mask_dev +
 * i * width * height. */
struct AdaptiveBatch {
    float threshold;
    uint8_t *mask_dev;
};

/* Why a batch refuses (cams, opts), decided before anything is enqueued; C2RT_OK otherwise. */
int check_batch_args(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts)
{
    if (!cams || !opts) return fail(ctx, C2RT_ERR_INVALID_ARG, "null cameras or options");
    if (n_frames > C2RT_MAX_BATCH_FRAMES)
        return fail(ctx, C2RT_ERR_LIMIT, "%u frames in one batch, at most %u", n_frames, (unsigned)C2RT_MAX_BATCH_FRAMES);
    if (!ctx->peers.empty())
        return fail(ctx, C2RT_ERR_UNSUPPORTED, "a multi-device context renders frame by frame: no batch call");
    if (opts->count_rays) return fail(ctx, C2RT_ERR_UNSUPPORTED, "count_rays: the counters belong to one frame, render counted frames one by one");
    if (opts->prepass_bucket) return fail(ctx, C2RT_ERR_UNSUPPORTED, "prepass_bucket: previews are rendered frame by frame");
    for (uint32_t i = 0; i < n_frames; ++i) {
        if (cams[i].dof) return fail(ctx, C2RT_ERR_UNSUPPORTED, "camera %u has depth of field: render it frame by frame", i);
        if (cams[i].stereo_separation != 0) return fail(ctx, C2RT_ERR_UNSUPPORTED, "camera %u is a stereo camera: render it frame by frame", i);
        if (const int st = check_frame_args(ctx, &cams[i], opts)) return st;
    }
    return C2RT_OK;
}

/* A frame of a posed batch (c2rt_render_frames_posed): its scene as planned for its pose, and which of its three
 * posable tables differ from the context's and therefore travel with the batch. */
struct PosedFrame {
    ScenePlan plan;
    bool own_nodes = false, own_lights = false, own_rects = false;
};

template <typename T>
bool same_bytes(const std::vector<T> &a, const std::vector<T> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

size_t align16(size_t b) { return (b + 15u) & ~(size_t)15u; }

/* Plans frame i of a posed batch for every i: ctx->scene under poses[i], put back afterwards.  posed[i] stays null for
 * a frame of the scene as it is.  The poses have passed check_scene_pose. */
int plan_posed_frames(c2rt_ctx *ctx, const c2rt_scene_pose *poses, uint32_t n_frames, std::vector<std::unique_ptr<PosedFrame>> &posed)
{
    posed.resize(n_frames);
    PoseUndo undo;
    for (uint32_t i = 0; i < n_frames; ++i) {
        if (poses[i].n_nodes == 0 && poses[i].n_lights == 0) continue;
        std::unique_ptr<PosedFrame> f(new PosedFrame());
        std::string err;
        pose_scene(ctx->scene, &poses[i], undo);
        const int st = replan_scene(ctx->scene, f->plan, err);
        if (st == C2RT_OK) apply_plan_knobs(f->plan);
        unpose_scene(ctx->scene, &poses[i], undo);
        if (st != C2RT_OK) return fail(ctx, st, "frame %u: %s", i, err.c_str());
        f->own_nodes = !same_bytes(f->plan.nodes, ctx->plan.nodes);
        f->own_lights = !same_bytes(f->plan.lights, ctx->plan.lights);
        f->own_rects = !same_bytes(f->plan.shadow_rects, ctx->plan.shadow_rects);
        posed[i] = std::move(f);
    }
    return C2RT_OK;
}

/* n_frames frames under one set of options with one mask pre-pass launch and one frame launch (two for
 * nested CSG), frame i into out_dev + i * local_rows * width * 3: the n-frame case of wire_frame, launched through the
 * table kernels.  Each frame's parameter block is what render_device
 * would launch it with — its own culling rectangles, row rotation, exact switch, mask table, retry list and output —
 * so the frames hold the bits of n single-frame calls; the kernels read block blockIdx.y of the table in HBM.
 * The arguments have passed check_batch_args.
 *
 * posed (nullable; c2rt_render_frames_posed): frame i's own scene where posed[i] is set — its block is planned from
 * that plan and names the copies of its changed tables behind the BatchCulls, in the same allocation and the same
 * copy.  One launch runs one instance: the frames are laid out in the table as up to two groups by what the launcher
 * cannot share — the plane instances of a single-light scene (launch_render_batch_level) — and a group that mixes
 * identity-only frames with others runs the general instance (the launcher's copy of a block says so; the instances
 * are held to the same bits: counted frames run the general one, tests/conftest.py).
 *
 * adaptive (nullable; c2rt_render_frames_adaptive, opts->taps == C2RT_TAPS_1, no strips): behind the frames, one
 * detection launch and one refinement launch for all of them.  Frame i's refinement block is what hit_params makes for
 * it — from its own plan, naming its own node and light tables and its own frame — and sits at index i behind the
 * posed tables, in the same allocation and the same copy: the frames, the flags and these blocks go by FRAME, only the
 * one-tap blocks by `order`.  Without it the call enqueues what it always has. */
int render_frames_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const std::vector<std::unique_ptr<PosedFrame>> *posed,
                         uint32_t n_frames, const c2rt_render_opts *opts, float *out_dev, hipStream_t stream,
                         const AdaptiveBatch *adaptive = nullptr)
{
    const int levels = ctx->plan.csg_levels; /* geometries are not posed: the same for every frame */
    const KernelVariant variant = variant_of(ctx->plan, &cams[0]);
    const bool nested = levels >= 2;
    const bool retry = nested && first_cap(levels, diag_knobs()) < kCsgFullCap(levels);
    const auto plan_of = [&](size_t i) -> const ScenePlan & { return posed && (*posed)[i] ? (*posed)[i]->plan : ctx->plan; };
    const auto plane_instance = [&](size_t i) { return plan_of(i).planes_only && plan_of(i).n_lights <= 1; };

    /* table order: the frames that share frame 0's instance first, then the others */
    const size_t n = n_frames;
    std::vector<uint32_t> order;
    order.reserve(n);
    for (uint32_t i = 0; i < n_frames; ++i)
        if (plane_instance(i) == plane_instance(0)) order.push_back(i);
    const size_t n_first = order.size();
    for (uint32_t i = 0; i < n_frames; ++i)
        if (plane_instance(i) != plane_instance(0)) order.push_back(i);

    const size_t n_blocks_tables = retry ? 2 * n : n;
    const size_t culls_at = n_blocks_tables * sizeof(RenderParams);
    size_t bytes = culls_at + n * sizeof(BatchCull);
    static_assert(sizeof(RenderParams) % 8 == 0 && alignof(BatchCull) <= 8, "BatchCull follows the parameter blocks");
    const size_t posed_at = align16(bytes);
    if (posed) {
        bytes = posed_at;
        for (size_t i = 0; i < n; ++i)
            if (const PosedFrame *f = (*posed)[i].get())
                bytes += (f->own_nodes ? align16(f->plan.nodes.size() * sizeof(DevNode)) : 0) +
                         (f->own_lights ? align16(f->plan.lights.size() * sizeof(DevLight)) : 0) +
                         (f->own_rects ? align16(f->plan.shadow_rects.size() * sizeof(double)) : 0);
    }
    const size_t refine_at = align16(bytes);
    if (adaptive) bytes = refine_at + n * sizeof(RenderParams);
    ctx->batch_host.resize(bytes);
    RenderParams *hp = reinterpret_cast<RenderParams *>(ctx->batch_host.data());
    RenderParams *hr = reinterpret_cast<RenderParams *>(ctx->batch_host.data() + refine_at); /* [frame], not [order] */
    BatchCull *hc = reinterpret_cast<BatchCull *>(ctx->batch_host.data() + culls_at);

    for (size_t j = 0; j < n; ++j) fill_params(plan_of(order[j]), ctx->dev, diag_knobs(), &cams[order[j]], opts, hp[j]);
    if (hp[0].local_rows == 0) return C2RT_OK;
    const size_t frame_floats = (size_t)hp[0].local_rows * hp[0].width * 3;
    /* the same for every frame with culling rectangles (one set of options, no depth of field); a posed frame may
     * have none where others do */
    size_t entries = 0, blocks = 0;
    for (size_t j = 0; j < n; ++j) {
        size_t e;
        frame_needs(hp[j], e, blocks);
        if (e > entries) entries = e;
    }
    const bool any_masks = entries != 0;

    FrameScratch &sc = scratch_for(ctx, stream);
    hipError_t e = grow_scratch(&sc.batch_table, &sc.batch_bytes, bytes, 1);
    if (e == hipSuccess) e = grow_scratch(&sc.tile_masks, &sc.tile_mask_entries, entries * n, 8 * sizeof(uint32_t));
    if (e == hipSuccess && nested) e = grow_scratch(&sc.retry_list, &sc.retry_words, (blocks + 1) * n, sizeof(uint32_t));
    if (e != hipSuccess) return fail(ctx, C2RT_ERR_HIP, "batch scratch: %s", hipGetErrorString(e));

    size_t at = posed_at;
    /* one of a posed frame's own tables: into the host image, its device address into the frame's block */
    const auto place = [&](const void *src, size_t table_bytes) {
        std::memcpy(ctx->batch_host.data() + at, src, table_bytes);
        const char *dev = sc.batch_table + at;
        at += align16(table_bytes);
        return dev;
    };
    for (size_t j = 0; j < n; ++j) {
        const size_t i = order[j];
        RenderParams &p = hp[j];
        if (const PosedFrame *f = posed ? (*posed)[i].get() : nullptr) {
            if (f->own_nodes) p.nodes = reinterpret_cast<const DevNode *>(place(f->plan.nodes.data(), f->plan.nodes.size() * sizeof(DevNode)));
            if (f->own_lights) p.lights = reinterpret_cast<const DevLight *>(place(f->plan.lights.data(), f->plan.lights.size() * sizeof(DevLight)));
            if (f->own_rects) p.shadow_rects = reinterpret_cast<const double *>(place(f->plan.shadow_rects.data(), f->plan.shadow_rects.size() * sizeof(double)));
        }
        p.out = out_dev + i * frame_floats;
        if (adaptive) {
            hr[i] = p;
            hit_settings(ctx, hr[i]);
        }
        wire_frame(ctx, plan_of(i), p, sc, j, entries, blocks, ~0u, hc[j]);
        if (retry) {
            hp[n + j] = p;
            hp[n + j].retry_mode = 1;
            hp[n + j].csg_cap = (uint32_t)kCsgFullCap(levels);
        }
    }
    const RenderParams *table_dev = reinterpret_cast<const RenderParams *>(sc.batch_table);
    const BatchCull *culls_dev = reinterpret_cast<const BatchCull *>(sc.batch_table + culls_at);
    HIP_TRY(ctx, hipMemcpyAsync(sc.batch_table, ctx->batch_host.data(), bytes, hipMemcpyHostToDevice, stream));
    int r = 0;
    if (any_masks) r = launch_tile_masks_batch(hp[0], table_dev, culls_dev, n_frames, stream);
    if (r != 0) return fail(ctx, C2RT_ERR_HIP, "tile-mask pre-pass launch: %s", hipGetErrorString((hipError_t)r));
    if (nested) HIP_TRY(ctx, hipMemsetAsync(sc.retry_list, 0, (blocks + 1) * n * sizeof(uint32_t), stream));
    const size_t group_at[3] = {0, n_first, n};
    for (int g = 0; g < 2 && r == 0; ++g) {
        const size_t a = group_at[g], count = group_at[g + 1] - a;
        if (!count) continue;
        /* the launcher's copy of a block of the group: the instance every frame of the group can run */
        RenderParams first = hp[a], again = retry ? hp[n + a] : hp[a];
        for (size_t j = a; j < a + count; ++j)
            if (!hp[j].all_identity) first.all_identity = again.all_identity = 0;
        r = launch_render_batch(first, variant, table_dev + a, (uint32_t)count, stream);
        if (r == 0 && retry) r = launch_render_batch(again, variant, table_dev + n + a, (uint32_t)count, stream);
    }
    if (r != 0) return fail(ctx, C2RT_ERR_HIP, "render kernel launch: %s", hipGetErrorString((hipError_t)r));
    if (!adaptive) return C2RT_OK;
    r = launch_aa_detect(out_dev, adaptive->mask_dev, hr[0].width, hr[0].height, n_frames, adaptive->threshold, stream);
    if (r != 0) return fail(ctx, C2RT_ERR_HIP, "adaptive AA detection kernel launch: %s", hipGetErrorString((hipError_t)r));
    r = launch_aa_refine_batch(hr[0], levels, reinterpret_cast<const RenderParams *>(sc.batch_table + refine_at), n_frames, adaptive->mask_dev, stream);
    if (r != 0) return fail(ctx, C2RT_ERR_HIP, "adaptive AA refinement kernel launch: %s", hipGetErrorString((hipError_t)r));
    return C2RT_OK;
}

/* Why a posed batch refuses its poses (after check_batch_args), naming the frame; C2RT_OK otherwise. */
int check_posed_args(c2rt_ctx *ctx, const c2rt_scene_pose *poses, uint32_t n_frames)
{
    if (!poses) return fail(ctx, C2RT_ERR_INVALID_ARG, "null poses");
    for (uint32_t i = 0; i < n_frames; ++i) {
        std::string err;
        if (const int st = check_scene_pose(ctx->scene, &poses[i], err)) return fail(ctx, st, "frame %u: %s", i, err.c_str());
    }
    return C2RT_OK;
}

/* One device slot's half of c2rt_update_scene: plans the posed scene (update_scene_plan), then copies to the device,
 * in stream order, the node records, the light table, the shadow rectangles and the dark-tile table whose bytes changed.  The sources are
 * pageable: the runtime has read them when each call returns. */
int update_one(c2rt_ctx *c, const c2rt_scene_pose *pose, hipStream_t stream)
{
    const std::vector<DevNode> nodes = c->plan.nodes;
    const std::vector<DevLight> lights = c->plan.lights;
    const std::vector<double> rects = c->plan.shadow_rects;
    const DarkCull dark = c->plan.dark;
    if (const int st = update_scene_plan(c->scene, c->plan, pose, c->err)) return st;
    apply_plan_knobs(c->plan);
    HIP_TRY(c, hipSetDevice(c->device));
    const std::vector<DevNode> &now = c->plan.nodes;
    for (size_t a = 0; a < now.size();) { /* runs of changed records */
        if (std::memcmp(&now[a], &nodes[a], sizeof(DevNode)) == 0) { ++a; continue; }
        size_t b = a + 1;
        while (b < now.size() && std::memcmp(&now[b], &nodes[b], sizeof(DevNode)) != 0) ++b;
        HIP_TRY(c, hipMemcpyAsync(c->dev.nodes + a, &now[a], (b - a) * sizeof(DevNode), hipMemcpyHostToDevice, stream));
        a = b;
    }
    if (!same_bytes(c->plan.lights, lights))
        HIP_TRY(c, hipMemcpyAsync(c->dev.lights, c->plan.lights.data(), lights.size() * sizeof(DevLight), hipMemcpyHostToDevice, stream));
    if (!same_bytes(c->plan.shadow_rects, rects))
        HIP_TRY(c, hipMemcpyAsync(c->dev.shadow_rects, c->plan.shadow_rects.data(), rects.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    if (std::memcmp(&c->plan.dark, &dark, sizeof dark) != 0)
        HIP_TRY(c, hipMemcpyAsync(c->dev.dark, &c->plan.dark, sizeof dark, hipMemcpyHostToDevice, stream));
    return C2RT_OK;
}

} // namespace

extern "C" {

uint32_t c2rt_abi_version(void) { return C2RT_ABI_VERSION; }

const char *c2rt_status_string(int status)
{
    switch (status) {
    case C2RT_OK: return "ok";
    case C2RT_ERR_INVALID_ARG: return "invalid argument";
    case C2RT_ERR_NO_DEVICE: return "no usable GPU (this library has no CPU fallback)";
    case C2RT_ERR_HIP: return "HIP runtime error";
    case C2RT_ERR_UNSUPPORTED: return "unsupported feature";
    case C2RT_ERR_LIMIT: return "device-path limit exceeded";
    case C2RT_ERR_NO_SCENE: return "no scene uploaded";
    case C2RT_ERR_CANCELLED: return "cancelled";
    case C2RT_ERR_IO: return "I/O error";
    case C2RT_ERR_PARSE: return "parse error";
    default: return "unknown status";
    }
}

const char *c2rt_last_error(const c2rt_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int c2rt_init(int device, c2rt_ctx **out)
{
    if (!out) return C2RT_ERR_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return C2RT_ERR_NO_DEVICE;
    if (device >= count) return C2RT_ERR_NO_DEVICE;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return C2RT_ERR_NO_DEVICE;
    c2rt_ctx *ctx = new c2rt_ctx();
    ctx->device = device;
    *out = ctx; /* handed out even on failure below so that c2rt_last_error works */
    HIP_TRY(ctx, hipSetDevice(device));
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < kMaxChunks; ++i) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->chunk_done[i], hipEventDisableTiming));
    HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_ready, hipEventDisableTiming));
    HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_done, hipEventDisableTiming));
    HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_inflight, hipEventDisableTiming));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->counters), 8 * sizeof(unsigned long long)));
    HIP_TRY(ctx, hipMemset(ctx->counters, 0, 8 * sizeof(unsigned long long)));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->probe), sizeof(c2rt_trace_result)));
    uint8_t lut[4097];
    build_srgb_lut(lut);
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->srgb_lut), sizeof lut));
    HIP_TRY(ctx, hipMemcpy(ctx->srgb_lut, lut, sizeof lut, hipMemcpyHostToDevice));
    return C2RT_OK;
}

int c2rt_init_multi(int device_count_or_0, const int *device_ids, c2rt_ctx **out)
{
    if (!out) return C2RT_ERR_INVALID_ARG;
    *out = nullptr;
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0) return C2RT_ERR_NO_DEVICE;
    if (device_count_or_0 < 0 || device_count_or_0 > 64) return C2RT_ERR_INVALID_ARG;
    const int n = device_count_or_0 == 0 ? visible : device_count_or_0;
    std::vector<int> ids(n);
    for (int i = 0; i < n; ++i) {
        /* device_count_or_0 == 0 means "every visible device": the caller's list (which may be empty) is not read */
        ids[i] = (device_ids && device_count_or_0 > 0) ? device_ids[i] : i;
        if (ids[i] < 0 || ids[i] >= visible) return C2RT_ERR_NO_DEVICE;
    }
    c2rt_ctx *lead = nullptr;
    int st = c2rt_init(ids[0], &lead);
    *out = lead;
    if (st != C2RT_OK) return st;
    for (int i = 1; i < n; ++i) {
        c2rt_ctx *peer = nullptr;
        st = c2rt_init(ids[i], &peer);
        if (peer) lead->peers.push_back(peer);
        if (st != C2RT_OK) return fail(lead, st, "device slot %d (HIP device %d): %s", i, ids[i], peer ? peer->err.c_str() : "init failed");
        if (ids[i] != ids[0]) {
            /* the slot's kernels store into the lead device's frame (c2rt_render_frame_device) */
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, ids[i], ids[0]) != hipSuccess || !can) {
                peer->peer_mapped = false;
            } else {
                const hipError_t e = hipDeviceEnablePeerAccess(ids[0], 0); /* current device = ids[i] (c2rt_init) */
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) peer->peer_mapped = false;
                (void)hipGetLastError();
            }
        }
    }
    HIP_TRY(lead, hipSetDevice(lead->device));
    return C2RT_OK;
}

int c2rt_device_count(const c2rt_ctx *ctx) { return ctx ? 1 + (int)ctx->peers.size() : 0; }

#if defined(C2RT_TILE_STATS) && C2RT_TILE_STATS
/* Diagnostics hook, in the diagnostics build only (make VARIANT=tilestats EXTRA_HIPFLAGS=-DC2RT_TILE_STATS=1;
 * the product library does not export it and include/c2rt.h does not declare it): the frame kernel writes
 * {wave cycles, class bits} per tile (tiles_x * tiles_y pairs of uint32) to this device buffer.
 * scripts/tile_stats.py. */
void c2rt_debug_set_tile_stats(c2rt_ctx *ctx, uint32_t *dev_buffer)
{
    if (ctx) ctx->dev.tile_stats = dev_buffer;
}
#endif

uint64_t c2rt_scene_generation(const c2rt_ctx *ctx) { return ctx && ctx->has_scene ? ctx->scene_gen : 0; }

void c2rt_destroy(c2rt_ctx *ctx)
{
    if (!ctx) return;
    for (c2rt_ctx *p : ctx->peers) c2rt_destroy(p);
    ctx->peers.clear();
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize(); /* frames may still be in flight on callers' streams */
    if (ctx->ev_ready) (void)hipEventDestroy(ctx->ev_ready);
    if (ctx->ev_done) (void)hipEventDestroy(ctx->ev_done);
    if (ctx->ev_inflight) (void)hipEventDestroy(ctx->ev_inflight);
    if (ctx->stream) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamDestroy(ctx->stream); }
    if (ctx->copy_stream) { (void)hipStreamSynchronize(ctx->copy_stream); (void)hipStreamDestroy(ctx->copy_stream); }
    for (hipEvent_t e : ctx->chunk_done)
        if (e) (void)hipEventDestroy(e);
    for (const auto &pb : ctx->pinned) (void)hipHostUnregister(pb.first);
    void *bufs[] = {ctx->dev.geoms, ctx->dev.nodes, ctx->dev.shaders, ctx->dev.textures, ctx->dev.lights, ctx->dev.texels,
                    ctx->frame, ctx->counters, ctx->probe, ctx->srgb_lut, ctx->dev.shadow_rects, ctx->dev.dark};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    for (FrameScratch &f : ctx->scratch) {
        if (f.tile_masks) (void)hipFree(f.tile_masks);
        if (f.retry_list) (void)hipFree(f.retry_list);
        if (f.batch_table) (void)hipFree(f.batch_table);
    }
    delete ctx;
}

static int upload_one(c2rt_ctx *ctx, const c2rt_scene_desc *s);

int c2rt_upload_scene(c2rt_ctx *ctx, const c2rt_scene_desc *s)
{
    static std::atomic<uint64_t> next_gen{1};
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    int st = upload_one(ctx, s);
    /* every device slot holds its own copy of the (small) tables and textures */
    for (size_t i = 0; i < ctx->peers.size() && st == C2RT_OK; ++i) {
        st = upload_one(ctx->peers[i], s);
        if (st != C2RT_OK) {
            ctx->has_scene = false;
            return fail(ctx, st, "device slot %zu: %s", i + 1, ctx->peers[i]->err.c_str());
        }
    }
    if (st == C2RT_OK) ctx->scene_gen = next_gen.fetch_add(1);
    if (!ctx->peers.empty()) (void)hipSetDevice(ctx->device);
    return st;
}

/* Plans the scene on the host (scene_plan.h), then replaces this device's tables.  A refused scene leaves the context
 * without a scene and touches nothing else of it. */
static int upload_one(c2rt_ctx *ctx, const c2rt_scene_desc *s)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    int st;
    if ((st = check_scene_desc(s, ctx->err)) != C2RT_OK) return st;
    ctx->has_scene = false;
    ScenePlan plan;
    if ((st = plan_scene(s, plan, ctx->err)) != C2RT_OK) return st;
    apply_plan_knobs(plan);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    /* frames enqueued on callers' streams may still be reading the tables about to be replaced */
    HIP_TRY(ctx, hipDeviceSynchronize());
    if ((st = upload(ctx, &ctx->dev.shadow_rects, plan.shadow_rects)) != C2RT_OK) return st;
    if ((st = upload(ctx, &ctx->dev.dark, std::vector<DarkCull>(1, plan.dark))) != C2RT_OK) return st;
    if ((st = upload(ctx, &ctx->dev.geoms, plan.geoms)) != C2RT_OK) return st;
    if ((st = upload(ctx, &ctx->dev.textures, plan.textures)) != C2RT_OK) return st;
    if ((st = upload(ctx, &ctx->dev.texels, plan.texels4)) != C2RT_OK) return st;
    if ((st = upload(ctx, &ctx->dev.shaders, plan.shaders)) != C2RT_OK) return st;
    if ((st = upload(ctx, &ctx->dev.lights, plan.lights)) != C2RT_OK) return st;
    if ((st = upload(ctx, &ctx->dev.nodes, plan.nodes)) != C2RT_OK) return st;
    ctx->plan = std::move(plan);
    ctx->scene.assign(s);
    ctx->has_scene = true;
    ctx->err.clear();
    return C2RT_OK;
}

int c2rt_update_scene(c2rt_ctx *ctx, const c2rt_scene_pose *pose, void *hip_stream)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (!ctx->has_scene) return fail(ctx, C2RT_ERR_NO_SCENE, "no scene uploaded");
    if (const int st = check_scene_pose(ctx->scene, pose, ctx->err)) return st;
    if (!ctx->peers.empty() && hip_stream)
        return fail(ctx, C2RT_ERR_INVALID_ARG, "a multi-device context orders every slot's copies on the slot's own stream: hip_stream must be null");
    if (pose->n_nodes == 0 && pose->n_lights == 0) return C2RT_OK;
    int st = update_one(ctx, pose, static_cast<hipStream_t>(hip_stream));
    if (st != C2RT_OK) return st;
    /* no stream named: the next frame may be a host-output one, which runs on the context's own stream and is not
     * ordered behind the default stream: the copies are waited for (that one stream only) */
    if (!hip_stream) HIP_TRY(ctx, hipStreamSynchronize(nullptr));
    for (size_t i = 0; i < ctx->peers.size() && st == C2RT_OK; ++i) {
        c2rt_ctx *c = ctx->peers[i];
        st = update_one(c, pose, c->stream);
        if (st != C2RT_OK) st = fail(ctx, st, "device slot %zu: %s", i + 1, c->err.c_str());
    }
    (void)hipSetDevice(ctx->device);
    return st;
}

/* Host-output frames (c2rt_render_frame: float RGB; c2rt_render_frame_rgb32: Color.toRGB32 words).
 * Into a buffer page-locked with c2rt_pin_host_buffer the frame is rendered in up to 8 row chunks:
 * chunk i streams back over PCIe (copy stream) while chunk i+1 renders (and is encoded), and the
 * stop flag is polled between chunks (finer than the reference's between-pass polling).  Into
 * pageable memory: one launch, one copy — chunked copies into pageable memory are slower than one
 * (measured).  ctx->frame (ensure_staging) holds the float rows OR the display words, whichever is asked for;
 * a frame the kernel stores straight into the page-locked destination has no staging buffer at all. */
/* Host-output pipeline, measured on MI355X (profiles/r03_variants.md).  Chunk size, 4K float frame (99.5 MB), ms by
 * chunk count: 10 chunks 2.12, 9 2.04, 8 (this) 1.96, 7 1.98, 6 1.98, 5 2.02, 4 2.19 (copy alone: 1.75).  A smaller
 * first chunk and a second copy stream: no gain (the pipeline is copy-bound from the first copy on). */
constexpr size_t kHostChunkBytes = 13u << 20;
struct HostKnobs {
    /* kernel stores straight into the page-locked frame: 0 never, 1 the display-word frame (4 B/pixel: 1.30 ms
     * against 1.60 chunked; the float frame's 12-byte stores reach only 44 GB/s: 2.27 against 2.02), 2 both.
     * C2RT_HOST_DIRECT_STORE sets it in the diagnostics build (tests/test_gpu_parity.py) */
    int direct_store = 1;
};
static const HostKnobs &host_knobs()
{
    static const HostKnobs k = [] {
        HostKnobs v;
        if (const char *e = diag_env("C2RT_HOST_DIRECT_STORE")) v.direct_store = std::atoi(e);
        return v;
    }();
    return k;
}

static int ensure_staging(c2rt_ctx *c, size_t bytes)
{
    const size_t floats = (bytes + sizeof(float) - 1) / sizeof(float);
    if (floats > c->frame_floats) {
        if (c->frame) { (void)hipFree(c->frame); c->frame = nullptr; c->frame_floats = 0; }
        HIP_TRY(c, hipMalloc(reinterpret_cast<void **>(&c->frame), floats * sizeof(float)));
        c->frame_floats = floats;
    }
    return C2RT_OK;
}

/* host wait for the last COUNTED stream-async frame (the ray counters are shared by all streams; everything else a
 * frame writes is per stream, FrameScratch) */
static int drain_inflight(c2rt_ctx *ctx)
{
    if (!ctx->has_inflight) return C2RT_OK;
    /* cleared whatever the wait returns: an error of the earlier frame is reported ONCE, here, and the context
     * stays usable (round-3 advisor: a failed sync used to leave has_inflight set for good) */
    ctx->has_inflight = false;
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_inflight));
    return C2RT_OK;
}

static int render_to_host(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, float *out_rgb,
                          uint32_t *out_rgb32, const volatile uint8_t *stop_flag)
{
    if (opts->count_rays)
        if (const int st = drain_inflight(ctx)) return st;
    RenderParams p;
    frame_params(ctx, cam, opts, p);
    ctx->counters_valid = false;
    if (opts->count_rays) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->counters, 0, 3 * sizeof(unsigned long long), ctx->stream));
        p.ray_counters = ctx->counters;
    }
    const uint32_t rows = p.local_rows;
    const size_t row_px = opts->width;
    /* the display frame leaves the render kernel encoded (RenderParams::out_rgb32): 4 B per pixel in the
     * staging buffer, no float frame, no second kernel */
    const size_t px_bytes = out_rgb ? 3 * sizeof(float) : sizeof(uint32_t);
    if (!out_rgb) {
        p.out = nullptr;
        p.srgb_lut = ctx->srgb_lut;
    }
    char *dst = out_rgb ? reinterpret_cast<char *>(out_rgb) : reinterpret_cast<char *>(out_rgb32);
    const size_t dst_row_bytes = row_px * px_bytes;
    bool is_pinned = false;
    for (const auto &pb : ctx->pinned)
        is_pinned = is_pinned || (dst >= reinterpret_cast<char *>(pb.first) &&
                                  dst + (size_t)rows * dst_row_bytes <= reinterpret_cast<char *>(pb.first) + pb.second);
    const KernelVariant variant = variant_of(ctx->plan, cam);
    const HostKnobs &knobs = host_knobs();
    if (is_pinned && knobs.direct_store >= (out_rgb ? 2 : 1)) {
        /* the kernel stores straight into the page-locked host frame over PCIe while it renders: one launch,
         * no staging buffer; the stop flag is polled once, before the launch (include/c2rt.h) */
        void *mapped = nullptr;
        if (hipHostGetDevicePointer(&mapped, dst, 0) == hipSuccess && mapped) {
            if (out_rgb) p.out = static_cast<float *>(mapped); else p.out_rgb32 = static_cast<uint32_t *>(mapped);
            if (stop_flag && *stop_flag) return fail(ctx, C2RT_ERR_CANCELLED, "stop requested during the frame");
            const int e = launch_frame(ctx, p, variant, ctx->stream);
            if (e != 0) return fail(ctx, C2RT_ERR_HIP, "render kernel launch: %s", hipGetErrorString((hipError_t)e));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (opts->count_rays) ctx->counters_valid = true;
            return C2RT_OK;
        }
        (void)hipGetLastError();
    }
    /* staging frame on the device: 12 B per pixel of float rows, or 4 B per pixel of display words */
    if (const int st = ensure_staging(ctx, (size_t)rows * row_px * px_bytes)) return st;
    char *staging = reinterpret_cast<char *>(ctx->frame);
    if (out_rgb) p.out = ctx->frame; else p.out_rgb32 = reinterpret_cast<uint32_t *>(ctx->frame);
    /* Into a page-locked frame: equal row chunks, chunk i crossing PCIe on the copy stream while chunk i+1 renders.
     * The copy (99.5 MB of float frame at ~57 GB/s = 1.75 ms at 4K) is longer than the render (1.15 ms), so
     * the frame time is the first chunk's render + the copies back to back.  Into pageable memory: one launch,
     * one copy (chunked copies into pageable memory are slower than one, measured).  The stop flag is polled
     * between chunks. */
    const size_t total_bytes = (size_t)rows * dst_row_bytes;
    uint32_t want = (uint32_t)((total_bytes + kHostChunkBytes - 1) / kHostChunkBytes);
    if (want < 1) want = 1;
    if (want > (uint32_t)kMaxChunks - 1) want = kMaxChunks - 1;
    uint32_t chunk = is_pinned ? ((rows + want - 1) / want + kTileH - 1) / kTileH * kTileH : rows;
    if (chunk < 64) chunk = 64;
    bool cancelled = false;
    int n_chunks = 0;
    { /* one mask table for the whole frame: every chunk's launch reads its rows of it */
        const int e = prepare_frame(ctx, p, ctx->stream);
        if (e != 0) return fail(ctx, C2RT_ERR_HIP, "tile-mask pre-pass launch: %s", hipGetErrorString((hipError_t)e));
    }
    for (uint32_t off = 0; off < rows && n_chunks < kMaxChunks; ++n_chunks) {
        if (stop_flag && *stop_flag) { cancelled = true; break; }
        uint32_t n = chunk;
        if (n > rows - off || n_chunks == kMaxChunks - 1) n = rows - off;
        p.row_offset = off;
        p.local_rows = n;
        p.tiles_y = (n + kTileH - 1) / kTileH;
        if (n < rows) p.row_group_start = 0; /* the rotation is relative to the whole frame's rows */
        const int e = launch_prepared(ctx, p, variant, ctx->stream);
        if (e != 0) return fail(ctx, C2RT_ERR_HIP, "render kernel launch: %s", hipGetErrorString((hipError_t)e));
        HIP_TRY(ctx, hipEventRecord(ctx->chunk_done[n_chunks], ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->chunk_done[n_chunks], 0));
        HIP_TRY(ctx, hipMemcpyAsync(dst + (size_t)off * dst_row_bytes, staging + (size_t)off * dst_row_bytes, (size_t)n * dst_row_bytes,
                                    hipMemcpyDeviceToHost, ctx->copy_stream));
        off += n;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (cancelled) return fail(ctx, C2RT_ERR_CANCELLED, "stop requested during the frame");
    if (opts->count_rays) ctx->counters_valid = true;
    return C2RT_OK;
}


/* Interleaved strips of a multi-device context: kTileH rows (one tile row) — the finest deal the
 * kernel's tiling allows, which balances the sky / floor / object mix best. */
constexpr uint32_t kMultiStrip = kTileH;

/* Host-output frame of a MULTI-DEVICE context (c2rt_init_multi): slot d renders strips d, d+G, ...
 * into its own staging buffer and copies them straight into the caller's frame with ONE strided 2-D
 * copy (row = one strip, destination pitch = G strips) over its own PCIe link — every device's copy
 * engine works in parallel and nothing is assembled on a device.  (RGB32: each slot encodes first.) */
static int render_to_host_multi(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, float *out_rgb,
                                uint32_t *out_rgb32, const volatile uint8_t *stop_flag)
{
    if (opts->count_rays)
        if (const int st = drain_inflight(ctx)) return st;
    const uint32_t G = 1u + (uint32_t)ctx->peers.size();
    const uint32_t sh = kMultiStrip, H = opts->height, W = opts->width;
    const uint32_t n_strips = (H + sh - 1) / sh, rem = H % sh; /* rem > 0: the last strip is partial */
    char *dst = out_rgb ? reinterpret_cast<char *>(out_rgb) : reinterpret_cast<char *>(out_rgb32);
    const size_t px_bytes = out_rgb ? 3 * sizeof(float) : sizeof(uint32_t);
    const size_t strip_bytes = (size_t)sh * W * px_bytes;
    const KernelVariant variant = variant_of(ctx->plan, cam);
    ctx->counters_valid = false;
    int st = C2RT_OK;
    bool cancelled = false;
    uint32_t launched = 0;
    for (uint32_t d = 0; d < G && st == C2RT_OK; ++d) {
        c2rt_ctx *c = d == 0 ? ctx : ctx->peers[d - 1];
        if (stop_flag && *stop_flag) { cancelled = true; break; }
        launched = d + 1;
        c2rt_render_opts o = *opts;
        o.strip_height = sh;
        o.strip_rank = d;
        o.strip_world = G;
        RenderParams p;
        frame_params(c, cam, &o, p);
        const uint32_t rows = p.local_rows;
        if (rows == 0) continue;
        if (hipSetDevice(c->device) != hipSuccess) { st = fail(ctx, C2RT_ERR_HIP, "hipSetDevice(%d)", c->device); break; }
        const size_t px = (size_t)rows * W;
        if ((st = ensure_staging(c, px * px_bytes)) != C2RT_OK) { st = fail(ctx, st, "slot %u: %s", d, c->err.c_str()); break; }
        if (out_rgb) {
            p.out = c->frame;
        } else { /* display words straight out of the render kernel (RenderParams::out_rgb32) */
            p.out = nullptr;
            p.out_rgb32 = reinterpret_cast<uint32_t *>(c->frame);
            p.srgb_lut = c->srgb_lut;
        }
        if (opts->count_rays) {
            if (hipMemsetAsync(c->counters, 0, 3 * sizeof(unsigned long long), c->stream) != hipSuccess) { st = fail(ctx, C2RT_ERR_HIP, "counter reset"); break; }
            p.ray_counters = c->counters;
        }
        const int e = launch_frame(c, p, variant, c->stream);
        if (e != 0) { st = fail(ctx, C2RT_ERR_HIP, "render kernel launch (slot %u): %s", d, hipGetErrorString((hipError_t)e)); break; }
        const char *src = reinterpret_cast<const char *>(c->frame);
        /* this slot's strips: d, d+G, ...; all full except possibly the frame's last strip */
        const uint32_t mine = (n_strips - d + G - 1) / G;
        const bool owns_partial = rem != 0 && (n_strips - 1) % G == d;
        const uint32_t full = owns_partial ? mine - 1 : mine;
        hipError_t he = hipSuccess;
        if (full)
            he = hipMemcpy2DAsync(dst + (size_t)d * strip_bytes, (size_t)G * strip_bytes, src, strip_bytes, strip_bytes, full,
                                  hipMemcpyDeviceToHost, c->stream);
        if (he == hipSuccess && owns_partial)
            he = hipMemcpyAsync(dst + (size_t)(n_strips - 1) * strip_bytes, src + (size_t)full * strip_bytes, (size_t)rem * W * px_bytes,
                                hipMemcpyDeviceToHost, c->stream);
        if (he != hipSuccess) st = fail(ctx, C2RT_ERR_HIP, "strip copy (slot %u): %s", d, hipGetErrorString(he));
    }
    for (uint32_t d = 0; d < launched; ++d) {
        c2rt_ctx *c = d == 0 ? ctx : ctx->peers[d - 1];
        (void)hipSetDevice(c->device);
        const hipError_t he = hipStreamSynchronize(c->stream);
        if (he != hipSuccess && st == C2RT_OK) st = fail(ctx, C2RT_ERR_HIP, "slot %u: %s", d, hipGetErrorString(he));
    }
    (void)hipSetDevice(ctx->device);
    if (st != C2RT_OK) return st;
    if (cancelled) return fail(ctx, C2RT_ERR_CANCELLED, "stop requested during the frame");
    if (opts->count_rays) ctx->counters_valid = true;
    return C2RT_OK;
}

/* Device-output frame of a multi-device context: every slot's kernel stores its strips straight
 * into `out_dev` on the lead device (RenderParams::frame_rows; peers reach it over xGMI through
 * peer access).  Ordered on the caller's stream: the peers start after what that stream has queued
 * so far (they overwrite the frame) and the stream continues after the last peer kernel. */
static int render_device_multi(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, float *out_dev,
                               hipStream_t stream)
{
    const uint32_t G = 1u + (uint32_t)ctx->peers.size();
    for (c2rt_ctx *c : ctx->peers)
        if (!c->peer_mapped)
            return fail(ctx, C2RT_ERR_UNSUPPORTED, "HIP device %d cannot map device %d's memory: use the host-output entry points", c->device, ctx->device);
    const KernelVariant variant = variant_of(ctx->plan, cam);
    ctx->counters_valid = false;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_ready, stream));
    /* A failure half way through must not leave a peer as the current device, nor peers that were already
     * launched still storing into `out_dev` unordered against the caller's stream: whatever happens, the lead
     * device is current again and `stream` waits for the ev_done of every peer launched so far. */
    uint32_t launched = 0; /* peers whose ev_done has been recorded */
    int st = C2RT_OK;
    const auto step = [&](hipError_t e, const char *what, uint32_t d) {
        if (e != hipSuccess && st == C2RT_OK) st = fail(ctx, C2RT_ERR_HIP, "%s (slot %u): %s", what, d, hipGetErrorString(e));
        return e == hipSuccess;
    };
    for (uint32_t d = 0; d < G && st == C2RT_OK; ++d) {
        c2rt_ctx *c = d == 0 ? ctx : ctx->peers[d - 1];
        c2rt_render_opts o = *opts;
        o.strip_height = kMultiStrip;
        o.strip_rank = d;
        o.strip_world = G;
        RenderParams p;
        frame_params(c, cam, &o, p);
        p.out = out_dev;
        p.frame_rows = 1;
        if (!step(hipSetDevice(c->device), "hipSetDevice", d)) break;
        hipStream_t s = d == 0 ? stream : c->stream;
        if (d != 0 && !step(hipStreamWaitEvent(s, ctx->ev_ready, 0), "hipStreamWaitEvent", d)) break;
        if (opts->count_rays) {
            if (!step(hipMemsetAsync(c->counters, 0, 3 * sizeof(unsigned long long), s), "counter reset", d)) break;
            p.ray_counters = c->counters;
        }
        if (p.local_rows) {
            const int e = launch_frame(c, p, variant, s);
            if (e != 0) { step((hipError_t)e, "render kernel launch", d); /* fall through: order what was queued */ }
        }
        if (d != 0) {
            if (!step(hipEventRecord(c->ev_done, s), "hipEventRecord", d)) break;
            launched = d;
        }
    }
    (void)hipSetDevice(ctx->device);
    for (uint32_t d = 1; d <= launched; ++d) {
        const hipError_t e = hipStreamWaitEvent(stream, ctx->peers[d - 1]->ev_done, 0);
        if (e != hipSuccess && st == C2RT_OK) st = fail(ctx, C2RT_ERR_HIP, "hipStreamWaitEvent (slot %u): %s", d, hipGetErrorString(e));
    }
    if (st != C2RT_OK) return st;
    if (opts->count_rays) ctx->counters_valid = true;
    return C2RT_OK;
}

static int check_multi_opts(c2rt_ctx *ctx, const c2rt_render_opts *opts)
{
    if (!ctx->peers.empty() && opts->strip_world > 1)
        return fail(ctx, C2RT_ERR_INVALID_ARG, "a multi-device context shards the frame itself: strip_world must be <= 1");
    return C2RT_OK;
}

uint32_t c2rt_local_rows(const c2rt_render_opts *opts)
{
    if (!opts) return 0;
    if (opts->strip_world > 1 && opts->strip_rank >= opts->strip_world) return 0;
    return local_rows_of(opts, opts->strip_world > 1 ? opts->strip_rank : 0);
}

int c2rt_render_frame_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                             float *out_rgb_dev, void *hip_stream)
{
    int st = check_frame_args(ctx, cam, opts);
    if (st != C2RT_OK) return st;
    if (!out_rgb_dev) return fail(ctx, C2RT_ERR_INVALID_ARG, "null output");
    if ((st = check_multi_opts(ctx, opts)) != C2RT_OK) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    /* Frames on one stream run in order; frames of this context on OTHER streams use other scratch slots
     * (FrameScratch) and are independent of this one.  Only a counted frame shares something — the ray counters —
     * and is ordered behind the previous counted frame on the device; the call never waits on the host. */
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (opts->count_rays && ctx->has_inflight) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->ev_inflight, 0));
    st = !ctx->peers.empty() ? render_device_multi(ctx, cam, opts, out_rgb_dev, stream)
                             : render_device(ctx, cam, opts, out_rgb_dev, stream);
    if (opts->count_rays) {
        /* also after a failed launch: whatever did get queued is ordered before the next counted frame */
        const hipError_t rec = hipEventRecord(ctx->ev_inflight, stream);
        if (rec == hipSuccess) ctx->has_inflight = true;
        else if (st == C2RT_OK) st = fail(ctx, C2RT_ERR_HIP, "hipEventRecord(ev_inflight): %s", hipGetErrorString(rec));
    }
    return st;
}

int c2rt_render_frame(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, float *out_rgb,
                      const volatile uint8_t *stop_flag)
{
    int st = check_frame_args(ctx, cam, opts);
    if (st != C2RT_OK) return st;
    if (!out_rgb) return fail(ctx, C2RT_ERR_INVALID_ARG, "null output");
    /* isStopReq() before the pass — rt/renderer.d:129 */
    if (stop_flag && *stop_flag) return fail(ctx, C2RT_ERR_CANCELLED, "stop requested before the frame");
    if ((st = check_multi_opts(ctx, opts)) != C2RT_OK) return st;
    if (!ctx->peers.empty()) return render_to_host_multi(ctx, cam, opts, out_rgb, nullptr, stop_flag);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return render_to_host(ctx, cam, opts, out_rgb, nullptr, stop_flag);
}

int c2rt_render_frames_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts,
                              float *out_rgb_dev, void *hip_stream)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (n_frames == 0) return C2RT_OK;
    if (const int st = check_batch_args(ctx, cams, n_frames, opts)) return st;
    if (!out_rgb_dev) return fail(ctx, C2RT_ERR_INVALID_ARG, "null output");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->counters_valid = false;
    return render_frames_device(ctx, cams, nullptr, n_frames, opts, out_rgb_dev, static_cast<hipStream_t>(hip_stream));
}

int c2rt_render_frames(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts,
                       float *out_rgb, const volatile uint8_t *stop_flag)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (n_frames == 0) return C2RT_OK;
    if (const int st = check_batch_args(ctx, cams, n_frames, opts)) return st;
    if (!out_rgb) return fail(ctx, C2RT_ERR_INVALID_ARG, "null output");
    if (stop_flag && *stop_flag) return fail(ctx, C2RT_ERR_CANCELLED, "stop requested before the batch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n_frames * c2rt_local_rows(opts) * opts->width * 3 * sizeof(float);
    if (bytes == 0) return C2RT_OK;
    if (const int st = ensure_staging(ctx, bytes)) return st;
    ctx->counters_valid = false;
    if (const int st = render_frames_device(ctx, cams, nullptr, n_frames, opts, ctx->frame, ctx->stream)) return st;
    HIP_TRY(ctx, hipMemcpyAsync(out_rgb, ctx->frame, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return C2RT_OK;
}

int c2rt_render_frames_posed_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, uint32_t n_frames,
                                    const c2rt_render_opts *opts, float *out_rgb_dev, void *hip_stream)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (n_frames == 0) return C2RT_OK;
    if (const int st = check_batch_args(ctx, cams, n_frames, opts)) return st;
    if (const int st = check_posed_args(ctx, poses, n_frames)) return st;
    if (!out_rgb_dev) return fail(ctx, C2RT_ERR_INVALID_ARG, "null output");
    std::vector<std::unique_ptr<PosedFrame>> posed;
    if (const int st = plan_posed_frames(ctx, poses, n_frames, posed)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->counters_valid = false;
    return render_frames_device(ctx, cams, &posed, n_frames, opts, out_rgb_dev, static_cast<hipStream_t>(hip_stream));
}

int c2rt_render_frames_posed(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, uint32_t n_frames,
                             const c2rt_render_opts *opts, float *out_rgb, const volatile uint8_t *stop_flag)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (n_frames == 0) return C2RT_OK;
    if (const int st = check_batch_args(ctx, cams, n_frames, opts)) return st;
    if (const int st = check_posed_args(ctx, poses, n_frames)) return st;
    if (!out_rgb) return fail(ctx, C2RT_ERR_INVALID_ARG, "null output");
    if (stop_flag && *stop_flag) return fail(ctx, C2RT_ERR_CANCELLED, "stop requested before the batch");
    std::vector<std::unique_ptr<PosedFrame>> posed;
    if (const int st = plan_posed_frames(ctx, poses, n_frames, posed)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n_frames * c2rt_local_rows(opts) * opts->width * 3 * sizeof(float);
    if (bytes == 0) return C2RT_OK;
    if (const int st = ensure_staging(ctx, bytes)) return st;
    ctx->counters_valid = false;
    if (const int st = render_frames_device(ctx, cams, &posed, n_frames, opts, ctx->frame, ctx->stream)) return st;
    HIP_TRY(ctx, hipMemcpyAsync(out_rgb, ctx->frame, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return C2RT_OK;
}

/* nothing of this context (any stream of any device slot) may still be copying into a buffer whose pages are
 * about to be unlocked */
static int quiesce(c2rt_ctx *ctx)
{
    ctx->has_inflight = false;
    HIP_TRY(ctx, hipDeviceSynchronize()); /* the context's own streams and whatever callers' streams hold */
    for (c2rt_ctx *c : ctx->peers) {
        HIP_TRY(ctx, hipSetDevice(c->device));
        HIP_TRY(ctx, hipDeviceSynchronize());
    }
    if (!ctx->peers.empty()) HIP_TRY(ctx, hipSetDevice(ctx->device));
    return C2RT_OK;
}

int c2rt_pin_host_buffer(c2rt_ctx *ctx, float *out_rgb, size_t bytes)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (!out_rgb || bytes == 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (size_t i = 0; i < ctx->pinned.size(); ++i)
        if (ctx->pinned[i].first == out_rgb) {
            if (ctx->pinned[i].second == bytes) return C2RT_OK;
            /* the same address with another size (a re-allocated frame buffer): register afresh, so that
             * the recorded range is exactly what is page-locked */
            if (const int st = quiesce(ctx)) return st;
            HIP_TRY(ctx, hipHostUnregister(out_rgb));
            ctx->pinned.erase(ctx->pinned.begin() + (long)i);
            break;
        }
    /* portable: page-locked for every device slot of a multi-device context */
    HIP_TRY(ctx, hipHostRegister(out_rgb, bytes, hipHostRegisterPortable | hipHostRegisterMapped));
    ctx->pinned.emplace_back(out_rgb, bytes);
    return C2RT_OK;
}

int c2rt_unpin_host_buffer(c2rt_ctx *ctx, float *out_rgb)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (size_t i = 0; i < ctx->pinned.size(); ++i)
        if (ctx->pinned[i].first == out_rgb) {
            if (const int st = quiesce(ctx)) return st;
            HIP_TRY(ctx, hipHostUnregister(out_rgb));
            ctx->pinned.erase(ctx->pinned.begin() + (long)i);
            return C2RT_OK;
        }
    return fail(ctx, C2RT_ERR_INVALID_ARG, "buffer was not pinned through this context");
}

int c2rt_get_ray_stats(c2rt_ctx *ctx, c2rt_ray_stats *out)
{
    if (!ctx || !out) return C2RT_ERR_INVALID_ARG;
    if (!ctx->counters_valid) return fail(ctx, C2RT_ERR_INVALID_ARG, "last render did not count rays");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const int st = drain_inflight(ctx)) return st; /* a counted device-output frame may still be running */
    unsigned long long h[2];
    HIP_TRY(ctx, hipMemcpy(h, ctx->counters, sizeof h, hipMemcpyDeviceToHost));
    out->primary_rays = h[0];
    out->shadow_rays = h[1];
    for (c2rt_ctx *c : ctx->peers) { /* every slot counted its own strips */
        HIP_TRY(ctx, hipSetDevice(c->device));
        HIP_TRY(ctx, hipStreamSynchronize(c->stream));
        HIP_TRY(ctx, hipMemcpy(h, c->counters, sizeof h, hipMemcpyDeviceToHost));
        out->primary_rays += h[0];
        out->shadow_rays += h[1];
    }
    if (!ctx->peers.empty()) HIP_TRY(ctx, hipSetDevice(ctx->device));
    return C2RT_OK;
}

/* One counter of the context, summed over its device slots.  counted: the counter is the ray counts' (only a counting
 * render leaves it valid, and a counted device-output frame may still be running: drain it, then each peer's stream);
 * otherwise every render writes it, on whatever stream: wait for the devices. */
static int get_counter(c2rt_ctx *ctx, int index, bool counted, uint64_t *out)
{
    if (!ctx || !out) return C2RT_ERR_INVALID_ARG;
    if (counted && !ctx->counters_valid) return fail(ctx, C2RT_ERR_INVALID_ARG, "last render did not count rays");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (counted) {
        if (const int st = drain_inflight(ctx)) return st;
    } else
        HIP_TRY(ctx, hipDeviceSynchronize());
    unsigned long long h = 0;
    HIP_TRY(ctx, hipMemcpy(&h, ctx->counters + index, sizeof h, hipMemcpyDeviceToHost));
    *out = h;
    for (c2rt_ctx *c : ctx->peers) {
        HIP_TRY(ctx, hipSetDevice(c->device));
        if (counted)
            HIP_TRY(ctx, hipStreamSynchronize(c->stream));
        else
            HIP_TRY(ctx, hipDeviceSynchronize());
        HIP_TRY(ctx, hipMemcpy(&h, c->counters + index, sizeof h, hipMemcpyDeviceToHost));
        *out += h;
    }
    if (!ctx->peers.empty()) HIP_TRY(ctx, hipSetDevice(ctx->device));
    return C2RT_OK;
}

int c2rt_get_csg_truncations(c2rt_ctx *ctx, uint64_t *out) { return get_counter(ctx, 2, true, out); }
int c2rt_get_exact_redos(c2rt_ctx *ctx, uint64_t *out) { return get_counter(ctx, 3, false, out); }
int c2rt_get_ground_bails(c2rt_ctx *ctx, uint64_t *out) { return get_counter(ctx, 4, false, out); }
int c2rt_get_sphere_bails(c2rt_ctx *ctx, uint64_t *out) { return get_counter(ctx, 5, false, out); }
int c2rt_get_csg_tile_bails(c2rt_ctx *ctx, uint64_t *out) { return get_counter(ctx, 6, false, out); }
int c2rt_get_csg_tiles(c2rt_ctx *ctx, uint64_t *out) { return get_counter(ctx, 7, false, out); }

int c2rt_render_pixel(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, int x, int y,
                      c2rt_trace_result *out)
{
    int st = check_frame_args(ctx, cam, opts);
    if (st != C2RT_OK) return st;
    if (!out) return fail(ctx, C2RT_ERR_INVALID_ARG, "null output");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    frame_params(ctx, cam, opts, p);
    p.n_cull = 0; /* the probe launch has no tile: never cull */
    p.ground_fast = 0;
    p.ground_certain_cq = 0;
    p.n_cull_lights = 0;
    p.csg_cap = (uint32_t)kCsgFullCap(C2RT_MAX_CSG_DEPTH); /* the probe instance handles every depth */
    p.probe_x = x;
    p.probe_y = y;
    p.probe_out = ctx->probe;
    HIP_TRY(ctx, hipMemsetAsync(ctx->probe, 0, sizeof(c2rt_trace_result), ctx->stream));
    const int e = launch_probe(p, variant_of(ctx->plan, cam), ctx->stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "probe kernel launch: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->probe, sizeof *out, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return C2RT_OK;
}

/* ---- ray queries (c2rt_rays.hip) ------------------------------------------------------------------------------ */

/* What the query kernels read of a parameter block: the scene's tables and constants, the full-capacity hit stack
 * (it cannot overflow: one launch, no retry list) and nothing of a frame — no camera, no culling rectangles
 * (n_cull = 0: every mask is all ones), no ground node, no scratch. */
static void query_params(const c2rt_ctx *ctx, RenderParams &p)
{
    std::memset(&p, 0, sizeof p);
    p.geoms = ctx->dev.geoms;
    p.nodes = ctx->dev.nodes;
    p.shaders = ctx->dev.shaders;
    p.textures = ctx->dev.textures;
    p.lights = ctx->dev.lights;
    p.texels = ctx->dev.texels;
    p.n_nodes = ctx->plan.n_nodes;
    p.n_lights = ctx->plan.n_lights;
    std::memcpy(p.ambient, ctx->plan.ambient, sizeof p.ambient);
    p.max_trace_depth = ctx->plan.max_trace_depth;
    p.force_exact = 1;
    p.ground_node = -1;
    p.csg_cap = ctx->plan.csg_levels == 0 ? 0u : (uint32_t)kCsgFullCap(ctx->plan.csg_levels);
    p.redo_counter = ctx->counters + 3;
}

/* the refusals shared by the four entry points, in the documented order; `in`: the input array, out_ok: a required
 * output is there.  > 0: return that status; 0: go on; -1: n == 0, return C2RT_OK */
static int check_query_args(c2rt_ctx *ctx, const void *in, uint64_t n, bool out_ok)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (n == 0) return -1;
    if (!in) return fail(ctx, C2RT_ERR_INVALID_ARG, "null input array");
    if (!out_ok) return fail(ctx, C2RT_ERR_INVALID_ARG, "null output");
    if (n > (uint64_t)C2RT_MAX_RAYS) return fail(ctx, C2RT_ERR_LIMIT, "%llu rays in one call (at most %u)", (unsigned long long)n, (unsigned)C2RT_MAX_RAYS);
    if (!ctx->has_scene) return fail(ctx, C2RT_ERR_NO_SCENE, "no scene uploaded");
    return 0;
}

int c2rt_trace_rays_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n, c2rt_ray_hit *hits_dev, float *rgb_dev,
                           void *hip_stream)
{
    if (const int st = check_query_args(ctx, rays_dev, n, hits_dev || rgb_dev)) return st < 0 ? C2RT_OK : st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    query_params(ctx, p);
    const int e = launch_trace_rays(p, ctx->plan.csg_levels, rays_dev, n, hits_dev, rgb_dev, hip_stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "ray query kernel launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

int c2rt_test_visibility_device(c2rt_ctx *ctx, const c2rt_segment *seg_dev, uint64_t n, uint8_t *visible_dev, void *hip_stream)
{
    if (const int st = check_query_args(ctx, seg_dev, n, visible_dev != nullptr)) return st < 0 ? C2RT_OK : st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    query_params(ctx, p);
    const int e = launch_test_visibility(p, ctx->plan.csg_levels, seg_dev, n, visible_dev, hip_stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "visibility query kernel launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

/* Host variants: chunks of at most kQueryChunk samples through ONE staging allocation (the context's, shared with the
 * host-output frames: calls on a context are serialised) laid out [inputs | output after output] for the chunk size and
 * only for the outputs asked for, 256-byte aligned — for c2rt_trace_rays 12 MiB + 20 MiB + 3 MiB at most, whatever n
 * is.  Copies from and to pageable memory are staged by the runtime; each chunk ends with a stream sync, so the call
 * blocks as documented. */
constexpr uint64_t kQueryChunk = 1u << 18;
static size_t align256(size_t b) { return (b + 255u) & ~(size_t)255u; }

extern "C++" { /* templates */

/* A plane family, described once; the generic faces under "plane families" below are written against it.  bytes: the
 * struct as the host code sees it, member k a pointer to samples of bytes[k] bytes (kPlanes<S> of them, c2rt_query.h).
 * The words its messages are built from: which planes ("the %s planes"), what a pixel holds ("a pixel's %s one
 * ray's"), how many pointers of which struct, the kernel of the launch error.  Opts and check_opts: the options in front
 * of the planes and their refusals, in the documented order (NoOpts: none).  The launches are the overloads
 * launch_plane_rows / launch_plane_rays of c2rt_query.h on S. */
template <class S> struct Family;
template <> struct Family<c2rt_hit_planes> {
    static constexpr size_t bytes[] = {4, 4, 8, 16, 24, 24, 12}; /* 92 B per sample */
    static constexpr const char *planes = "hit", *holds = "record is", *count = "seven", *name = "c2rt_hit_planes", *what = "hit plane";
    using Opts = NoOpts;
    static int check_opts(c2rt_ctx *, const Opts *) { return C2RT_OK; }
};
template <> struct Family<c2rt_shade_planes> {
    static constexpr size_t bytes[] = {4, 12, 12, 12, 4, 12}; /* 56 B per sample */
    static constexpr const char *planes = "shading", *holds = "terms are", *count = "six", *name = "c2rt_shade_planes", *what = "shading plane";
    using Opts = NoOpts;
    static int check_opts(c2rt_ctx *, const Opts *) { return C2RT_OK; }
};
template <> struct Family<c2rt_occlusion_planes> {
    static constexpr size_t bytes[] = {4, 8, 4, 24}; /* 40 B per sample */
    static constexpr const char *planes = "occlusion", *holds = "occlusion is", *count = "four", *name = "c2rt_occlusion_planes", *what = "occlusion plane";
    using Opts = c2rt_occlusion_opts;
    static int check_opts(c2rt_ctx *ctx, const Opts *occ)
    {
        if (!occ) return fail(ctx, C2RT_ERR_INVALID_ARG, "null occlusion options");
        if (!(occ->radius > 0) || !std::isfinite(occ->radius))
            return fail(ctx, C2RT_ERR_INVALID_ARG, "occlusion radius %g: a finite length above 0", occ->radius);
        if (occ->samples == 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "occlusion samples is 0: at least one sample");
        if (occ->reserved != 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "c2rt_occlusion_opts.reserved is %u: must be 0", (unsigned)occ->reserved);
        if (occ->samples > C2RT_MAX_OCCLUSION_SAMPLES)
            return fail(ctx, C2RT_ERR_LIMIT, "%u occlusion samples (at most %u)", (unsigned)occ->samples, (unsigned)C2RT_MAX_OCCLUSION_SAMPLES);
        return C2RT_OK;
    }
};
template <> struct Family<c2rt_gather_planes> {
    static constexpr size_t bytes[] = {4, 8, 12, 12}; /* 36 B per sample */
    static constexpr const char *planes = "gather", *holds = "gather is", *count = "four", *name = "c2rt_gather_planes", *what = "gather plane";
    using Opts = c2rt_gather_opts;
    static int check_opts(c2rt_ctx *ctx, const Opts *g)
    {
        if (!g) return fail(ctx, C2RT_ERR_INVALID_ARG, "null gather options");
        if (g->samples == 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "gather samples is 0: at least one sample");
        if (g->reserved != 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "c2rt_gather_opts.reserved is %u: must be 0", (unsigned)g->reserved);
        if (g->samples > C2RT_MAX_GATHER_SAMPLES)
            return fail(ctx, C2RT_ERR_LIMIT, "%u gather samples (at most %u)", (unsigned)g->samples, (unsigned)C2RT_MAX_GATHER_SAMPLES);
        return C2RT_OK;
    }
};
template <> struct Family<c2rt_path_planes> {
    static constexpr size_t bytes[] = {4, 4, 12, 12, 12}; /* 44 B per sample */
    static constexpr const char *planes = "path", *holds = "paths are", *count = "five", *name = "c2rt_path_planes", *what = "path plane";
    using Opts = c2rt_path_opts;
    static int check_opts(c2rt_ctx *ctx, const Opts *g)
    {
        if (!g) return fail(ctx, C2RT_ERR_INVALID_ARG, "null path options");
        if (g->paths == 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "paths is 0: at least one path");
        if (g->bounces == 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "bounces is 0: at least one bounce");
        if (g->paths > C2RT_MAX_PATHS) return fail(ctx, C2RT_ERR_LIMIT, "%u paths (at most %u)", (unsigned)g->paths, (unsigned)C2RT_MAX_PATHS);
        if (g->bounces > C2RT_MAX_PATH_BOUNCES)
            return fail(ctx, C2RT_ERR_LIMIT, "%u bounces (at most %u)", (unsigned)g->bounces, (unsigned)C2RT_MAX_PATH_BOUNCES);
        return C2RT_OK;
    }
};
static_assert(sizeof Family<c2rt_hit_planes>::bytes == kPlanes<c2rt_hit_planes> * sizeof(size_t) &&
              sizeof Family<c2rt_shade_planes>::bytes == kPlanes<c2rt_shade_planes> * sizeof(size_t) &&
              sizeof Family<c2rt_occlusion_planes>::bytes == kPlanes<c2rt_occlusion_planes> * sizeof(size_t) &&
              sizeof Family<c2rt_gather_planes>::bytes == kPlanes<c2rt_gather_planes> * sizeof(size_t) &&
              sizeof Family<c2rt_path_planes>::bytes == kPlanes<c2rt_path_planes> * sizeof(size_t), "a sample size for every plane");
static constexpr NoOpts kNoOpts = {};

/* What a host variant stages: its outputs in staging order.  An output is `layers` slices (layer-major on both sides)
 * of samples of `bytes` bytes each; `host` null: not asked for, takes no room.  lay_out places them. */
struct Staging {
    struct Output {
        char *host;
        size_t bytes;
        uint32_t layers;
        char *dev;
    };
    Output out[8];
    int n = 0;

    void add(void *host, size_t bytes, uint32_t layers = 1) { out[n++] = {static_cast<char *>(host), bytes, layers, nullptr}; }
    template <class S>
    void add_planes(const S &planes_host, uint32_t layers = 1)
    {
        char *host[kPlanes<S>];
        std::memcpy(host, &planes_host, sizeof host);
        for (int k = 0; k < kPlanes<S>; ++k) add(host[k], Family<S>::bytes[k], layers);
    }
    /* the device-side struct of the planes added as outputs first, first + 1, ... */
    template <class S>
    S planes(int first = 0) const
    {
        char *dev[kPlanes<S>];
        for (int k = 0; k < kPlanes<S>; ++k) dev[k] = out[first + k].dev;
        S d;
        std::memcpy(&d, dev, sizeof d);
        return d;
    }
    template <class T>
    T *dev(int k) const { return reinterpret_cast<T *>(out[k].dev); }
};

/* The staging allocation for `in_bytes` of inputs and one chunk of `chunk` samples of every output asked for */
static int lay_out(c2rt_ctx *ctx, Staging &outs, size_t in_bytes, size_t chunk)
{
    size_t off[8], at = align256(in_bytes), end = in_bytes;
    for (int k = 0; k < outs.n; ++k) {
        off[k] = at;
        if (!outs.out[k].host) continue;
        end = at + chunk * outs.out[k].layers * outs.out[k].bytes;
        at = align256(end);
    }
    if (const int e = ensure_staging(ctx, end)) return e;
    for (int k = 0; k < outs.n; ++k) outs.out[k].dev = outs.out[k].host ? reinterpret_cast<char *>(ctx->frame) + off[k] : nullptr;
    return C2RT_OK;
}

/* Samples [first, first + m) of every layer of every output from the chunk's staging to their place in the caller's
 * arrays: layers host_stride samples apart there, `chunk` samples apart in the staging */
static int copy_back(c2rt_ctx *ctx, const Staging &outs, size_t first, size_t m, size_t host_stride, size_t chunk)
{
    for (int k = 0; k < outs.n; ++k) {
        const Staging::Output &o = outs.out[k];
        for (uint32_t l = 0; o.host && l < o.layers; ++l)
            HIP_TRY(ctx, hipMemcpyAsync(o.host + (l * host_stride + first) * o.bytes, o.dev + l * chunk * o.bytes, m * o.bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    return C2RT_OK;
}

/* The ray faces: n input records (c2rt_ray, c2rt_segment) in chunks of at most `cap`.  launch(p, records_dev, first, m,
 * chunk) enqueues the `what` kernel over m staged records, `first` the index in the caller's array of the first of them,
 * the layer stride of its outputs being `chunk`.  more_in, more_fixed: bytes per sample and per chunk of further inputs and
 * scratch behind the chunk's records, which the launch places and stages itself (the counted path planes' counts and order). */
template <class Launch>
static int ray_chunks(c2rt_ctx *ctx, const void *in, uint64_t n, uint64_t cap, Staging &outs, const char *what, Launch launch, size_t more_in = 0, size_t more_fixed = 0)
{
    static_assert(sizeof(c2rt_ray) == sizeof(c2rt_segment), "one input record size");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t chunk = n < cap ? n : cap;
    if (const int e = lay_out(ctx, outs, chunk * (sizeof(c2rt_ray) + more_in) + more_fixed, chunk)) return e;
    c2rt_ray *in_dev = reinterpret_cast<c2rt_ray *>(ctx->frame);
    RenderParams p;
    query_params(ctx, p);
    for (uint64_t i = 0; i < n; i += chunk) {
        const uint64_t m = n - i < chunk ? n - i : chunk;
        HIP_TRY(ctx, hipMemcpyAsync(in_dev, static_cast<const c2rt_ray *>(in) + i, m * sizeof(c2rt_ray), hipMemcpyHostToDevice, ctx->stream));
        const int e = launch(p, in_dev, i, m, chunk);
        if (e != 0) return fail(ctx, C2RT_ERR_HIP, "%s kernel launch: %s", what, hipGetErrorString((hipError_t)e));
        if (const int st = copy_back(ctx, outs, i, m, n, chunk)) return st;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return C2RT_OK;
}

/* The frame faces: the local rows of the frame `p` describes in chunks of whole rows, at most kQueryChunk / layers
 * pixels each but one row at least (width <= 2^16: with one layer that is four rows or more).  launch(r0, m, chunk_px)
 * enqueues the `what` kernel over rows [r0, r0 + m) into the staging, whose layers are chunk_px pixels apart.  in_per_px,
 * in_fixed: bytes per pixel and per chunk of inputs and scratch at the head of the buffer, which the launch places and stages
 * itself (the counted path planes' counts and order). */
template <class Launch>
static int row_chunks(c2rt_ctx *ctx, const RenderParams &p, uint32_t layers, Staging &outs, const char *what, Launch launch, size_t in_per_px = 0, size_t in_fixed = 0)
{
    const uint32_t rows = p.local_rows, width = p.width;
    uint32_t chunk_rows = (uint32_t)(kQueryChunk / layers / width);
    if (chunk_rows == 0) chunk_rows = 1;
    if (chunk_rows > rows) chunk_rows = rows;
    const size_t chunk_px = (size_t)chunk_rows * width;
    if (const int e = lay_out(ctx, outs, in_per_px * chunk_px + in_fixed, chunk_px)) return e;
    for (uint32_t r0 = 0; r0 < rows; r0 += chunk_rows) {
        const uint32_t m = rows - r0 < chunk_rows ? rows - r0 : chunk_rows;
        const int e = launch(r0, m, chunk_px);
        if (e != 0) return fail(ctx, C2RT_ERR_HIP, "%s kernel launch: %s", what, hipGetErrorString((hipError_t)e));
        if (const int st = copy_back(ctx, outs, (size_t)r0 * width, (size_t)m * width, (size_t)rows * width, chunk_px)) return st;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return C2RT_OK;
}

} /* extern "C++" */

int c2rt_trace_rays(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n, c2rt_ray_hit *hits, float *rgb)
{
    if (const int st = check_query_args(ctx, rays, n, hits || rgb)) return st < 0 ? C2RT_OK : st;
    Staging outs;
    outs.add(hits, sizeof(c2rt_ray_hit));
    outs.add(rgb, 3 * sizeof(float));
    return ray_chunks(ctx, rays, n, kQueryChunk, outs, "ray query", [&](const RenderParams &p, const c2rt_ray *rays_dev, uint64_t, uint64_t m, uint64_t) {
        return launch_trace_rays(p, ctx->plan.csg_levels, rays_dev, m, outs.dev<c2rt_ray_hit>(0), outs.dev<float>(1), ctx->stream);
    });
}

int c2rt_test_visibility(c2rt_ctx *ctx, const c2rt_segment *seg, uint64_t n, uint8_t *visible)
{
    if (const int st = check_query_args(ctx, seg, n, visible != nullptr)) return st < 0 ? C2RT_OK : st;
    Staging outs;
    outs.add(visible, 1);
    return ray_chunks(ctx, seg, n, kQueryChunk, outs, "visibility query", [&](const RenderParams &p, const c2rt_ray *seg_dev, uint64_t, uint64_t m, uint64_t) {
        return launch_test_visibility(p, ctx->plan.csg_levels, reinterpret_cast<const c2rt_segment *>(seg_dev), m, outs.dev<uint8_t>(0), ctx->stream);
    });
}

/* ---- plane families: hit, shading, occlusion, gather and path planes of a camera frame or of a caller's rays --------- */
/* (c2rt_hit_planes.hip, c2rt_shade_planes.hip, c2rt_occlusion.hip, c2rt_gather.hip, c2rt_paths.hip; each described by its Family above) */

/* The refusals of the modes in which a pixel is not one ray, in the documented order; `holds`: what a pixel holds in the
 * call ("record is", "terms are"), `planes`: which planes it fills ("hit", "shading") */
static int check_one_ray_per_pixel(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const char *holds, const char *planes)
{
    if (cam->dof) return fail(ctx, C2RT_ERR_UNSUPPORTED, "depth of field: a pixel's %s one ray's, a lens has many per pixel", holds);
    if (cam->stereo_separation != 0) return fail(ctx, C2RT_ERR_UNSUPPORTED, "stereo: a pixel's %s one ray's, a stereo camera has two per pixel", holds);
    if (opts->count_rays) return fail(ctx, C2RT_ERR_UNSUPPORTED, "count_rays: the %s planes do not count rays", planes);
    if (opts->prepass_bucket) return fail(ctx, C2RT_ERR_UNSUPPORTED, "prepass_bucket: a preview's pixels share the sample of their block");
    return C2RT_OK;
}

/* The frame's parameter block for its camera, strips and size, with the query settings on top (query_params): exact::
 * arithmetic, full-capacity hit stack, no culling rectangles (every mask all ones), no ground node, one tap. */
static void hit_params(const c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, RenderParams &p)
{
    frame_params(ctx, cam, opts, p);
    hit_settings(ctx, p);
}

extern "C++" { /* templates: the four faces of a family S, `o` its options (&kNoOpts where it has none) */

/* the family's own refusals, behind the frame call's or the ray call's, in the documented order: the options', then the
 * planes' */
template <class S>
static int check_planes(c2rt_ctx *ctx, const typename Family<S>::Opts *o, const S *planes)
{
    if (const int st = Family<S>::check_opts(ctx, o)) return st;
    if (!planes) return fail(ctx, C2RT_ERR_INVALID_ARG, "null planes");
    if (!any_plane(*planes))
        return fail(ctx, C2RT_ERR_INVALID_ARG, "no plane asked for: all %s pointers of %s are null", Family<S>::count, Family<S>::name);
    return C2RT_OK;
}

/* the refusals of both frame faces, in the documented order: a frame call's, then the family's, then the modes in which
 * a pixel is not one ray */
template <class S>
static int check_frame_planes(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const typename Family<S>::Opts *o, const S *planes)
{
    if (const int st = check_frame_args(ctx, cam, opts)) return st;
    if (const int st = check_planes(ctx, o, planes)) return st;
    return check_one_ray_per_pixel(ctx, cam, opts, Family<S>::holds, Family<S>::planes);
}

template <class S>
static int frame_planes_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const typename Family<S>::Opts *o,
                               const S *planes_dev, void *hip_stream)
{
    if (const int st = check_frame_planes(ctx, cam, opts, o, planes_dev)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    hit_params(ctx, cam, opts, p);
    if (p.local_rows == 0) return C2RT_OK;
    const int e = launch_plane_rows(p, ctx->plan.csg_levels, *o, *planes_dev, 0, p.local_rows, hip_stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "%s kernel launch: %s", Family<S>::what, hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

/* Host variant: chunks of whole rows, at most kQueryChunk pixels each (row_chunks), plane after plane for the chunk size
 * and only for the planes asked for — 92 / 56 / 40 / 36 / 44 B per pixel, 23 / 14 / 10 / 9 / 11 MiB at most, whatever the frame
 * size.  A chunk's pixels draw the samples of their place in the frame. */
template <class S>
static int frame_planes_host(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const typename Family<S>::Opts *o,
                             const S *planes_host)
{
    if (const int st = check_frame_planes(ctx, cam, opts, o, planes_host)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    hit_params(ctx, cam, opts, p);
    if (p.local_rows == 0) return C2RT_OK;
    Staging outs;
    outs.add_planes(*planes_host);
    return row_chunks(ctx, p, 1, outs, Family<S>::what, [&](uint32_t r0, uint32_t m, size_t) {
        return launch_plane_rows(p, ctx->plan.csg_levels, *o, outs.planes<S>(), r0, m, ctx->stream);
    });
}

template <class S>
static int ray_planes_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n, const typename Family<S>::Opts *o, const S *planes_dev, void *hip_stream)
{
    if (const int st = check_query_args(ctx, rays_dev, n, true)) return st < 0 ? C2RT_OK : st;
    if (const int st = check_planes(ctx, o, planes_dev)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    query_params(ctx, p);
    const int e = launch_plane_rays(p, ctx->plan.csg_levels, rays_dev, n, 0, *o, *planes_dev, hip_stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "%s kernel launch: %s", Family<S>::what, hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

/* Host variant: c2rt_trace_rays' staging, [rays | planes asked for] for chunks of at most kQueryChunk rays; a chunk's rays
 * draw the samples of their place in the caller's array (ray_chunks' `first`) */
template <class S>
static int ray_planes_host(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n, const typename Family<S>::Opts *o, const S *planes_host)
{
    if (const int st = check_query_args(ctx, rays, n, true)) return st < 0 ? C2RT_OK : st;
    if (const int st = check_planes(ctx, o, planes_host)) return st;
    Staging outs;
    outs.add_planes(*planes_host);
    return ray_chunks(ctx, rays, n, kQueryChunk, outs, Family<S>::what, [&](const RenderParams &p, const c2rt_ray *rays_dev, uint64_t first, uint64_t m, uint64_t) {
        return launch_plane_rays(p, ctx->plan.csg_levels, rays_dev, m, first, *o, outs.planes<S>(), ctx->stream);
    });
}

} /* extern "C++" */

int c2rt_render_hits_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                            const c2rt_hit_planes *planes_dev, void *hip_stream)
{
    return frame_planes_device(ctx, cam, opts, &kNoOpts, planes_dev, hip_stream);
}

int c2rt_render_hits(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_hit_planes *planes_host)
{
    return frame_planes_host(ctx, cam, opts, &kNoOpts, planes_host);
}

int c2rt_render_shading_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                               const c2rt_shade_planes *planes_dev, void *hip_stream)
{
    return frame_planes_device(ctx, cam, opts, &kNoOpts, planes_dev, hip_stream);
}

int c2rt_render_shading(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_shade_planes *planes_host)
{
    return frame_planes_host(ctx, cam, opts, &kNoOpts, planes_host);
}

int c2rt_trace_rays_shading_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n, const c2rt_shade_planes *planes_dev, void *hip_stream)
{
    return ray_planes_device(ctx, rays_dev, n, &kNoOpts, planes_dev, hip_stream);
}

int c2rt_trace_rays_shading(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n, const c2rt_shade_planes *planes_host)
{
    return ray_planes_host(ctx, rays, n, &kNoOpts, planes_host);
}

int c2rt_render_occlusion_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_occlusion_opts *occ,
                                 const c2rt_occlusion_planes *planes_dev, void *hip_stream)
{
    return frame_planes_device(ctx, cam, opts, occ, planes_dev, hip_stream);
}

int c2rt_render_occlusion(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_occlusion_opts *occ,
                          const c2rt_occlusion_planes *planes_host)
{
    return frame_planes_host(ctx, cam, opts, occ, planes_host);
}

int c2rt_trace_rays_occlusion_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n, const c2rt_occlusion_opts *occ,
                                     const c2rt_occlusion_planes *planes_dev, void *hip_stream)
{
    return ray_planes_device(ctx, rays_dev, n, occ, planes_dev, hip_stream);
}

int c2rt_trace_rays_occlusion(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n, const c2rt_occlusion_opts *occ,
                              const c2rt_occlusion_planes *planes_host)
{
    return ray_planes_host(ctx, rays, n, occ, planes_host);
}

int c2rt_render_gather_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_gather_opts *g,
                              const c2rt_gather_planes *planes_dev, void *hip_stream)
{
    return frame_planes_device(ctx, cam, opts, g, planes_dev, hip_stream);
}

int c2rt_render_gather(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_gather_opts *g,
                       const c2rt_gather_planes *planes_host)
{
    return frame_planes_host(ctx, cam, opts, g, planes_host);
}

int c2rt_trace_rays_gather_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n, const c2rt_gather_opts *g, const c2rt_gather_planes *planes_dev,
                                  void *hip_stream)
{
    return ray_planes_device(ctx, rays_dev, n, g, planes_dev, hip_stream);
}

int c2rt_trace_rays_gather(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n, const c2rt_gather_opts *g, const c2rt_gather_planes *planes_host)
{
    return ray_planes_host(ctx, rays, n, g, planes_host);
}

int c2rt_render_paths_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_path_opts *g,
                             const c2rt_path_planes *planes_dev, void *hip_stream)
{
    return frame_planes_device(ctx, cam, opts, g, planes_dev, hip_stream);
}

int c2rt_render_paths(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_path_opts *g,
                      const c2rt_path_planes *planes_host)
{
    return frame_planes_host(ctx, cam, opts, g, planes_host);
}

int c2rt_trace_rays_paths_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n, const c2rt_path_opts *g, const c2rt_path_planes *planes_dev,
                                 void *hip_stream)
{
    return ray_planes_device(ctx, rays_dev, n, g, planes_dev, hip_stream);
}

int c2rt_trace_rays_paths(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n, const c2rt_path_opts *g, const c2rt_path_planes *planes_host)
{
    return ray_planes_host(ctx, rays, n, g, planes_host);
}

/* ---- counted path planes: the path planes with a count per sample (c2rt_paths_counted.hip) ---------------------------- */

/* what the counted calls refuse behind the path call's own, in the documented order; aligned: the _device variants */
static int check_counts(c2rt_ctx *ctx, const uint8_t *counts, const void *scratch, bool aligned)
{
    if (!counts) return fail(ctx, C2RT_ERR_INVALID_ARG, "null counts");
    if (aligned && reinterpret_cast<uintptr_t>(scratch) % 16 != 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "the count-order scratch is not 16-byte aligned");
    return C2RT_OK;
}

size_t c2rt_paths_counted_scratch_bytes(uint64_t n_samples) { return counted_scratch_bytes(n_samples); }

int c2rt_render_paths_counted_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_path_opts *g,
                                     const uint8_t *counts_dev, const c2rt_path_planes *planes_dev, void *scratch_dev, void *hip_stream)
{
    if (const int st = check_frame_planes(ctx, cam, opts, g, planes_dev)) return st;
    if (const int st = check_counts(ctx, counts_dev, scratch_dev, true)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    hit_params(ctx, cam, opts, p);
    if (p.local_rows == 0) return C2RT_OK;
    const int e = launch_counted_rows(p, ctx->plan.csg_levels, *g, counts_dev, *planes_dev, 0, p.local_rows, scratch_dev, hip_stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "counted path plane kernel launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

/* Host variants: the path planes' chunks with the chunk's counts staged beside them — at the head of the buffer for a
 * frame, behind the rays for a ray call — and behind the counts the scratch of count order, which every chunk runs in: it
 * took 0.43 to 0.76 of natural order's time on the three uneven planes measured and 1.07 on an even one
 * (profiles/paths_counted.md).  [counts: chunk bytes | to the next multiple of 16 | counted_scratch_bytes(chunk)] */
constexpr size_t kCountedPerSample = 1 + 4, kCountedFixed = kCountedHeadBytes + 32;
static void *counted_scratch(uint8_t *counts_dev, size_t chunk)
{
    return reinterpret_cast<void *>((reinterpret_cast<uintptr_t>(counts_dev) + chunk + 15u) & ~(uintptr_t)15u);
}
static_assert(15 + kCountedHeadBytes + 15 <= kCountedFixed, "the padding in front of the scratch and the rounding of its order fit what a chunk reserves");

int c2rt_render_paths_counted(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_path_opts *g, const uint8_t *counts,
                              const c2rt_path_planes *planes_host)
{
    if (const int st = check_frame_planes(ctx, cam, opts, g, planes_host)) return st;
    if (const int st = check_counts(ctx, counts, nullptr, false)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    hit_params(ctx, cam, opts, p);
    if (p.local_rows == 0) return C2RT_OK;
    Staging outs;
    outs.add_planes(*planes_host);
    return row_chunks(ctx, p, 1, outs, "counted path plane", [&](uint32_t r0, uint32_t m, size_t chunk_px) {
        uint8_t *counts_dev = reinterpret_cast<uint8_t *>(ctx->frame);
        if (const hipError_t e = hipMemcpyAsync(counts_dev, counts + (size_t)r0 * p.width, (size_t)m * p.width, hipMemcpyHostToDevice, ctx->stream)) return (int)e;
        return launch_counted_rows(p, ctx->plan.csg_levels, *g, counts_dev, outs.planes<c2rt_path_planes>(), r0, m, counted_scratch(counts_dev, chunk_px), ctx->stream);
    }, kCountedPerSample, kCountedFixed);
}

int c2rt_trace_rays_paths_counted_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n, const c2rt_path_opts *g, const uint8_t *counts_dev,
                                         const c2rt_path_planes *planes_dev, void *scratch_dev, void *hip_stream)
{
    if (const int st = check_query_args(ctx, rays_dev, n, true)) return st < 0 ? C2RT_OK : st;
    if (const int st = check_planes(ctx, g, planes_dev)) return st;
    if (const int st = check_counts(ctx, counts_dev, scratch_dev, true)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    query_params(ctx, p);
    const int e = launch_counted_rays(p, ctx->plan.csg_levels, rays_dev, n, 0, *g, counts_dev, *planes_dev, scratch_dev, hip_stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "counted path plane kernel launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

int c2rt_trace_rays_paths_counted(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n, const c2rt_path_opts *g, const uint8_t *counts,
                                  const c2rt_path_planes *planes_host)
{
    if (const int st = check_query_args(ctx, rays, n, true)) return st < 0 ? C2RT_OK : st;
    if (const int st = check_planes(ctx, g, planes_host)) return st;
    if (const int st = check_counts(ctx, counts, nullptr, false)) return st;
    Staging outs;
    outs.add_planes(*planes_host);
    return ray_chunks(ctx, rays, n, kQueryChunk, outs, "counted path plane", [&](const RenderParams &p, const c2rt_ray *rays_dev, uint64_t first, uint64_t m, uint64_t chunk) {
        uint8_t *counts_dev = reinterpret_cast<uint8_t *>(ctx->frame) + chunk * sizeof(c2rt_ray);
        if (const hipError_t e = hipMemcpyAsync(counts_dev, counts + first, m, hipMemcpyHostToDevice, ctx->stream)) return (int)e;
        return launch_counted_rays(p, ctx->plan.csg_levels, rays_dev, m, first, *g, counts_dev, outs.planes<c2rt_path_planes>(), counted_scratch(counts_dev, chunk), ctx->stream);
    }, kCountedPerSample, kCountedFixed);
}

/* ---- denoise: the a-trous filter over full-frame planes (c2rt_denoise.hip) ------------------------------------------- */

/* the options' own refusals, in the documented order (`ctx` null: the status alone) */
static int check_denoise_opts(c2rt_ctx *ctx, const c2rt_denoise_opts *o)
{
    if (!o->width || !o->height) return fail(ctx, C2RT_ERR_INVALID_ARG, "denoise frame of %u x %u pixels: both must be above 0", (unsigned)o->width, (unsigned)o->height);
    if (o->channels != 1 && o->channels != 3) return fail(ctx, C2RT_ERR_INVALID_ARG, "denoise channels is %u: 1 or 3", (unsigned)o->channels);
    if (!(o->sigma_plane > 0) || !std::isfinite(o->sigma_plane))
        return fail(ctx, C2RT_ERR_INVALID_ARG, "sigma_plane %g: a finite length above 0", (double)o->sigma_plane);
    if (!(o->sigma_colour >= 0) || !std::isfinite(o->sigma_colour))
        return fail(ctx, C2RT_ERR_INVALID_ARG, "sigma_colour %g: finite and not negative", (double)o->sigma_colour);
    if (o->reserved != 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "c2rt_denoise_opts.reserved is %u: must be 0", (unsigned)o->reserved);
    if (o->levels > C2RT_MAX_DENOISE_LEVELS)
        return fail(ctx, C2RT_ERR_LIMIT, "%u denoise levels (at most %u)", (unsigned)o->levels, (unsigned)C2RT_MAX_DENOISE_LEVELS);
    if (o->normal_power_log2 > 7) return fail(ctx, C2RT_ERR_LIMIT, "normal_power_log2 is %u (at most 7)", (unsigned)o->normal_power_log2);
    return C2RT_OK;
}

/* every refusal of c2rt_denoise_device, in the documented order; with_scratch false: the host variant, whose scratch is
 * the library's own */
static int check_denoise(c2rt_ctx *ctx, const c2rt_denoise_guides *g, const c2rt_denoise_opts *o, const float *in, const float *out,
                         const void *scratch, bool with_scratch)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (!o) return fail(ctx, C2RT_ERR_INVALID_ARG, "null denoise options");
    if (!g) return fail(ctx, C2RT_ERR_INVALID_ARG, "null denoise guides");
    if (const int st = check_denoise_opts(ctx, o)) return st;
    if (!g->node) return fail(ctx, C2RT_ERR_INVALID_ARG, "null guide: node");
    if (!g->normal) return fail(ctx, C2RT_ERR_INVALID_ARG, "null guide: normal");
    if (!g->p) return fail(ctx, C2RT_ERR_INVALID_ARG, "null guide: p");
    if (!in) return fail(ctx, C2RT_ERR_INVALID_ARG, "null denoise input");
    if (!out) return fail(ctx, C2RT_ERR_INVALID_ARG, "null denoise output");
    if (out == in) return fail(ctx, C2RT_ERR_INVALID_ARG, "denoise output is the input: the filter does not run in place");
    if (!with_scratch) return C2RT_OK;
    if (scratch && out == scratch) return fail(ctx, C2RT_ERR_INVALID_ARG, "denoise output is the scratch");
    if (scratch && in == scratch) return fail(ctx, C2RT_ERR_INVALID_ARG, "denoise input is the scratch");
    if (!scratch && c2rt_denoise_scratch_bytes(o) != 0)
        return fail(ctx, C2RT_ERR_INVALID_ARG, "null denoise scratch: these options need %zu bytes", c2rt_denoise_scratch_bytes(o));
    if (reinterpret_cast<uintptr_t>(scratch) % 16 != 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "denoise scratch is not 16-byte aligned");
    return C2RT_OK;
}

/* the contract's per-call and per-level factors, in fp32, and the launches */
static int denoise_enqueue(c2rt_ctx *ctx, const c2rt_denoise_guides &g, const c2rt_denoise_opts &o, const float *in, float *out, void *scratch,
                           void *stream)
{
    const float inv_plane = 1.0f / o.sigma_plane;
    float inv_c2[C2RT_MAX_DENOISE_LEVELS] = {};
    for (uint32_t l = 0; l < o.levels; ++l) {
        const volatile float sc = o.sigma_colour * std::ldexp(1.0f, -(int)l);
        const volatile float sc2 = sc * sc;
        inv_c2[l] = 1.0f / sc2;
    }
    const int e = launch_denoise(g, o, inv_plane, inv_c2, in, out, scratch, stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "denoise kernel launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

size_t c2rt_denoise_scratch_bytes(const c2rt_denoise_opts *o)
{
    if (!o || check_denoise_opts(nullptr, o) != C2RT_OK) return 0;
    return denoise_guide_bytes(*o) + denoise_plane_bytes(*o);
}

int c2rt_denoise_device(c2rt_ctx *ctx, const c2rt_denoise_guides *guides_dev, const c2rt_denoise_opts *o, const float *in_dev, float *out_dev,
                        void *scratch_dev, void *hip_stream)
{
    if (const int st = check_denoise(ctx, guides_dev, o, in_dev, out_dev, scratch_dev, true)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return denoise_enqueue(ctx, *guides_dev, *o, in_dev, out_dev, scratch_dev, hip_stream);
}

int c2rt_denoise(c2rt_ctx *ctx, const c2rt_denoise_guides *guides_host, const c2rt_denoise_opts *o, const float *in, float *out)
{
    if (const int st = check_denoise(ctx, guides_host, o, in, out, nullptr, false)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)o->width * o->height, colour = (size_t)o->channels * sizeof(float);
    /* [node | normal | p | albedo | base | in | out | scratch], each 256-byte aligned */
    const void *host[6] = {guides_host->node, guides_host->normal, guides_host->p, guides_host->albedo, guides_host->base, in};
    const size_t bytes[8] = {px * 4, px * 24, px * 24, guides_host->albedo ? px * colour : 0, guides_host->base ? px * colour : 0, px * colour,
                             px * colour, c2rt_denoise_scratch_bytes(o)};
    size_t off[8], at = 0;
    for (int k = 0; k < 8; ++k) {
        off[k] = at;
        at = align256(at + bytes[k]);
    }
    if (const int e = ensure_staging(ctx, at)) return e;
    char *dev = reinterpret_cast<char *>(ctx->frame);
    for (int k = 0; k < 6; ++k)
        if (bytes[k]) HIP_TRY(ctx, hipMemcpyAsync(dev + off[k], host[k], bytes[k], hipMemcpyHostToDevice, ctx->stream));
    c2rt_denoise_guides g;
    g.node = reinterpret_cast<const int32_t *>(dev + off[0]);
    g.normal = reinterpret_cast<const double *>(dev + off[1]);
    g.p = reinterpret_cast<const double *>(dev + off[2]);
    g.albedo = bytes[3] ? reinterpret_cast<const float *>(dev + off[3]) : nullptr;
    g.base = bytes[4] ? reinterpret_cast<const float *>(dev + off[4]) : nullptr;
    if (const int st = denoise_enqueue(ctx, g, *o, reinterpret_cast<const float *>(dev + off[5]), reinterpret_cast<float *>(dev + off[6]),
                                       bytes[7] ? dev + off[7] : nullptr, ctx->stream))
        return st;
    HIP_TRY(ctx, hipMemcpyAsync(out, dev + off[6], bytes[6], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return C2RT_OK;
}

/* every refusal of c2rt_render_paths_denoised ahead of the filter options' own, in the documented order (the sequence
 * calls start with them); have_opts: the filter's options of either kind are given, (width, height, channels) theirs */
static int check_paths_filtered(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_path_opts *pg, bool have_opts,
                                uint32_t width, uint32_t height, uint32_t channels, const float *out_rgb)
{
    if (const int st = check_frame_args(ctx, cam, opts)) return st;
    if (const int st = Family<c2rt_path_planes>::check_opts(ctx, pg)) return st;
    if (!have_opts) return fail(ctx, C2RT_ERR_INVALID_ARG, "null denoise options");
    if (!out_rgb) return fail(ctx, C2RT_ERR_INVALID_ARG, "null output");
    if (const int st = check_one_ray_per_pixel(ctx, cam, opts, "paths are", "path")) return st;
    if (opts->strip_world > 1)
        return fail(ctx, C2RT_ERR_UNSUPPORTED, "strip_world is %u: the filter reads its neighbours, it needs the whole frame", (unsigned)opts->strip_world);
    if (width != opts->width || height != opts->height)
        return fail(ctx, C2RT_ERR_INVALID_ARG, "denoise options for %u x %u pixels, the frame has %u x %u", (unsigned)width, (unsigned)height,
                    (unsigned)opts->width, (unsigned)opts->height);
    if (channels != 3) return fail(ctx, C2RT_ERR_INVALID_ARG, "denoise channels is %u: a frame has 3", (unsigned)channels);
    return C2RT_OK;
}

static int check_paths_denoised(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_path_opts *pg,
                                const c2rt_denoise_opts *d, const float *out_rgb)
{
    if (const int st = check_paths_filtered(ctx, cam, opts, pg, d != nullptr, d ? d->width : 0, d ? d->height : 0, d ? d->channels : 0, out_rgb)) return st;
    return check_denoise_opts(ctx, d);
}

int c2rt_render_paths_denoised(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_path_opts *pg,
                               const c2rt_denoise_opts *d, float *out_rgb)
{
    if (const int st = check_paths_denoised(ctx, cam, opts, pg, d, out_rgb)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    hit_params(ctx, cam, opts, p);
    const size_t px = (size_t)opts->width * opts->height;
    /* [node | normal | p | rgb | albedo | indirect | out | scratch], each 256-byte aligned */
    const size_t bytes[8] = {px * 4, px * 24, px * 24, px * 12, px * 12, px * 12, px * 12, c2rt_denoise_scratch_bytes(d)};
    size_t off[8], at = 0;
    for (int k = 0; k < 8; ++k) {
        off[k] = at;
        at = align256(at + bytes[k]);
    }
    if (const int e = ensure_staging(ctx, at)) return e;
    char *dev = reinterpret_cast<char *>(ctx->frame);
    c2rt_hit_planes hits = {};
    hits.node = reinterpret_cast<int32_t *>(dev + off[0]);
    hits.normal = reinterpret_cast<double *>(dev + off[1]);
    hits.p = reinterpret_cast<double *>(dev + off[2]);
    hits.rgb = reinterpret_cast<float *>(dev + off[3]);
    c2rt_shade_planes shade = {};
    shade.albedo = reinterpret_cast<float *>(dev + off[4]);
    c2rt_path_planes paths = {};
    paths.indirect = reinterpret_cast<float *>(dev + off[5]);
    int e = launch_plane_rows(p, ctx->plan.csg_levels, kNoOpts, hits, 0, p.local_rows, ctx->stream);
    if (e == 0) e = launch_plane_rows(p, ctx->plan.csg_levels, kNoOpts, shade, 0, p.local_rows, ctx->stream);
    if (e == 0) e = launch_plane_rows(p, ctx->plan.csg_levels, *pg, paths, 0, p.local_rows, ctx->stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "denoised path frame, plane kernel launch: %s", hipGetErrorString((hipError_t)e));
    c2rt_denoise_guides g = {hits.node, hits.normal, hits.p, shade.albedo, hits.rgb};
    if (const int st = denoise_enqueue(ctx, g, *d, paths.indirect, reinterpret_cast<float *>(dev + off[6]), bytes[7] ? dev + off[7] : nullptr, ctx->stream))
        return st;
    HIP_TRY(ctx, hipMemcpyAsync(out_rgb, dev + off[6], bytes[6], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return C2RT_OK;
}

/* ---- temporal accumulation: reprojection of the previous frame's history (c2rt_temporal.hip) -------------------------- */

/* the options' own refusals, in the documented order (`ctx` null: the status alone); check_temporal_frame_opts: all but
 * max_age's, for the calls that do not accumulate (c2rt_path_counts*) */
static int check_temporal_frame_opts(c2rt_ctx *ctx, const c2rt_temporal_opts *o)
{
    if (!o->width || !o->height) return fail(ctx, C2RT_ERR_INVALID_ARG, "temporal frame of %u x %u pixels: both must be above 0", (unsigned)o->width, (unsigned)o->height);
    if (o->channels != 1 && o->channels != 3) return fail(ctx, C2RT_ERR_INVALID_ARG, "temporal channels is %u: 1 or 3", (unsigned)o->channels);
    if (!std::isfinite(o->min_normal_dot) || !(o->min_normal_dot >= 0) || !(o->min_normal_dot < 1))
        return fail(ctx, C2RT_ERR_INVALID_ARG, "min_normal_dot %g: finite, at least 0 and below 1", (double)o->min_normal_dot);
    if (!std::isfinite(o->max_plane_dist) || !(o->max_plane_dist > 0))
        return fail(ctx, C2RT_ERR_INVALID_ARG, "max_plane_dist %g: a finite length above 0", (double)o->max_plane_dist);
    if (o->reserved[0] != 0 || o->reserved[1] != 0)
        return fail(ctx, C2RT_ERR_INVALID_ARG, "c2rt_temporal_opts.reserved is %u, %u: must be 0", (unsigned)o->reserved[0], (unsigned)o->reserved[1]);
    return C2RT_OK;
}

static int check_temporal_opts(c2rt_ctx *ctx, const c2rt_temporal_opts *o)
{
    if (const int st = check_temporal_frame_opts(ctx, o)) return st;
    if (o->max_age == 0 || o->max_age > (uint32_t)C2RT_MAX_TEMPORAL_AGE)
        return fail(ctx, C2RT_ERR_LIMIT, "max_age is %u (1 .. %u)", (unsigned)o->max_age, (unsigned)C2RT_MAX_TEMPORAL_AGE);
    return C2RT_OK;
}

/* the contract's "per call, on the host" for the previous camera; returns det */
static double temporal_camera(const c2rt_camera_frame &prev, const c2rt_temporal_opts &o, TemporalCamera &k)
{
    double A[3], U[3], V[3];
    for (int c = 0; c < 3; ++c) {
        k.pos[c] = prev.pos[c];
        A[c] = prev.up_left[c] - prev.pos[c];
        U[c] = prev.up_right[c] - prev.up_left[c];
        V[c] = prev.down_left[c] - prev.up_left[c];
    }
    const auto cross = [](const double *a, const double *b, double *out) {
        out[0] = a[1] * b[2] - a[2] * b[1];
        out[1] = a[2] * b[0] - a[0] * b[2];
        out[2] = a[0] * b[1] - a[1] * b[0];
    };
    cross(U, V, k.na);
    cross(V, A, k.nb);
    cross(A, U, k.nc);
    const double det = (A[0] * k.na[0] + A[1] * k.na[1]) + A[2] * k.na[2];
    k.wd = (double)o.width;
    k.hd = (double)o.height;
    k.det_positive = det > 0 ? 1u : 0u;
    return det;
}

static int check_previous_camera(c2rt_ctx *ctx, const c2rt_camera_frame &prev, const c2rt_temporal_opts &o, TemporalCamera &k)
{
    const double det = temporal_camera(prev, o, k);
    if (!std::isfinite(det) || det == 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "degenerate previous camera: its corners span no volume with its eye (det %g)", det);
    return C2RT_OK;
}

/* the contract's "per moved node, on the host": record m of `tm` from the two poses of entry m, in fp64 */
static void motion_record(uint32_t index, const double *prev, const double *cur, TemporalMotion &tm)
{
    const double *Tc = cur, *Ic = cur + 9, *oc = cur + 27, *Tp = prev, *TIp = prev + 18, *op = prev + 27;
    double *w = tm.rec[tm.n];
    tm.index[tm.n++] = index;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            w[3 * i + j] = (Ic[3 * i] * Tp[j] + Ic[3 * i + 1] * Tp[3 + j]) + Ic[3 * i + 2] * Tp[6 + j];
            w[9 + 3 * i + j] = (Tc[i] * TIp[j] + Tc[3 + i] * TIp[3 + j]) + Tc[6 + i] * TIp[6 + j];
        }
    for (int c = 0; c < 3; ++c) {
        w[18 + c] = oc[c];
        w[21 + c] = op[c];
    }
}

/* the refusals c2rt_temporal_accumulate_motion* add, in the documented order, and the records of a list that passes */
static int check_temporal_motion(c2rt_ctx *ctx, const c2rt_temporal_motion *motion, TemporalMotion &tm)
{
    tm.n = 0;
    if (!motion) return C2RT_OK;
    if (motion->reserved != 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "c2rt_temporal_motion.reserved is %u: must be 0", (unsigned)motion->reserved);
    if (motion->n_nodes > (uint32_t)C2RT_MAX_MOTION_NODES)
        return fail(ctx, C2RT_ERR_LIMIT, "%u moved nodes (at most %u)", (unsigned)motion->n_nodes, (unsigned)C2RT_MAX_MOTION_NODES);
    if (motion->n_nodes == 0) return C2RT_OK;
    if (!motion->node_index) return fail(ctx, C2RT_ERR_INVALID_ARG, "motion: %u nodes with a null node_index", (unsigned)motion->n_nodes);
    if (!motion->prev_transform) return fail(ctx, C2RT_ERR_INVALID_ARG, "motion: %u nodes with a null prev_transform", (unsigned)motion->n_nodes);
    if (!motion->cur_transform) return fail(ctx, C2RT_ERR_INVALID_ARG, "motion: %u nodes with a null cur_transform", (unsigned)motion->n_nodes);
    for (uint32_t i = 1; i < motion->n_nodes; ++i)
        for (uint32_t j = 0; j < i; ++j)
            if (motion->node_index[i] == motion->node_index[j])
                return fail(ctx, C2RT_ERR_INVALID_ARG, "motion: node_index[%u] = %u is listed twice", (unsigned)i, (unsigned)motion->node_index[i]);
    for (uint32_t i = 0; i < motion->n_nodes; ++i)
        motion_record(motion->node_index[i], motion->prev_transform + 30 * (size_t)i, motion->cur_transform + 30 * (size_t)i, tm);
    return C2RT_OK;
}

/* every refusal of c2rt_temporal_accumulate_device, in the documented order; aligned false: the host variant, whose
 * histories are staged; `k`: the previous camera's constants where there is a history; `tm` (nullable: the static calls):
 * the motion call's refusals behind "null planes", and its records */
static int check_temporal(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *g, const c2rt_temporal_opts *o, const float *in,
                          const void *history_prev, const void *history_out, const c2rt_temporal_planes *planes, bool aligned, TemporalCamera &k,
                          const c2rt_temporal_motion *motion = nullptr, TemporalMotion *tm = nullptr)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (!o) return fail(ctx, C2RT_ERR_INVALID_ARG, "null temporal options");
    if (!g) return fail(ctx, C2RT_ERR_INVALID_ARG, "null temporal guides");
    if (const int st = check_temporal_opts(ctx, o)) return st;
    if (!g->node) return fail(ctx, C2RT_ERR_INVALID_ARG, "null guide: node");
    if (!g->normal) return fail(ctx, C2RT_ERR_INVALID_ARG, "null guide: normal");
    if (!g->p) return fail(ctx, C2RT_ERR_INVALID_ARG, "null guide: p");
    if (!in) return fail(ctx, C2RT_ERR_INVALID_ARG, "null temporal input");
    if (!history_out) return fail(ctx, C2RT_ERR_INVALID_ARG, "null history out");
    if (!planes) return fail(ctx, C2RT_ERR_INVALID_ARG, "null temporal planes");
    if (tm)
        if (const int st = check_temporal_motion(ctx, motion, *tm)) return st;
    if (history_prev && !prev_cam) return fail(ctx, C2RT_ERR_INVALID_ARG, "a previous history without its camera: null prev_cam");
    if (history_prev)
        if (const int st = check_previous_camera(ctx, *prev_cam, *o, k)) return st;
    if (history_out == history_prev) return fail(ctx, C2RT_ERR_INVALID_ARG, "history out is the previous history: the caller swaps two");
    if (planes->colour == in) return fail(ctx, C2RT_ERR_INVALID_ARG, "temporal colour plane is the input");
    if (aligned && (reinterpret_cast<uintptr_t>(history_out) % 16 != 0 || reinterpret_cast<uintptr_t>(history_prev) % 16 != 0))
        return fail(ctx, C2RT_ERR_INVALID_ARG, "a history is not 16-byte aligned");
    return C2RT_OK;
}

static int temporal_enqueue(c2rt_ctx *ctx, const c2rt_temporal_guides &g, const c2rt_temporal_opts &o, const TemporalCamera *k, const float *in,
                            const void *history_prev, void *history_out, const c2rt_temporal_planes &planes, void *stream,
                            const TemporalMotion *tm = nullptr)
{
    const int e = launch_temporal(g, o, history_prev ? k : nullptr, in, history_prev, history_out, planes, stream, tm);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "temporal kernel launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

size_t c2rt_temporal_history_bytes(const c2rt_temporal_opts *o)
{
    if (!o || check_temporal_opts(nullptr, o) != C2RT_OK) return 0;
    return temporal_history_bytes(*o);
}

int c2rt_temporal_accumulate_device(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *guides_dev, const c2rt_temporal_opts *o,
                                    const float *in_dev, const void *history_prev_dev, void *history_out_dev, const c2rt_temporal_planes *planes_dev,
                                    void *hip_stream)
{
    TemporalCamera k = {};
    if (const int st = check_temporal(ctx, prev_cam, guides_dev, o, in_dev, history_prev_dev, history_out_dev, planes_dev, true, k)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return temporal_enqueue(ctx, *guides_dev, *o, &k, in_dev, history_prev_dev, history_out_dev, *planes_dev, hip_stream);
}

int c2rt_temporal_accumulate_motion_device(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *guides_dev,
                                           const c2rt_temporal_opts *o, const c2rt_temporal_motion *motion, const float *in_dev,
                                           const void *history_prev_dev, void *history_out_dev, const c2rt_temporal_planes *planes_dev, void *hip_stream)
{
    TemporalCamera k = {};
    TemporalMotion tm;
    if (const int st = check_temporal(ctx, prev_cam, guides_dev, o, in_dev, history_prev_dev, history_out_dev, planes_dev, true, k, motion, &tm)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return temporal_enqueue(ctx, *guides_dev, *o, &k, in_dev, history_prev_dev, history_out_dev, *planes_dev, hip_stream, &tm);
}

/* the two host variants behind their checks: staged whole through the context's staging buffer (`tm` null: the static call) */
static int temporal_to_host(c2rt_ctx *ctx, const TemporalCamera &k, const c2rt_temporal_guides *guides_host, const c2rt_temporal_opts *o,
                            const float *in, const void *history_prev, void *history_out, const c2rt_temporal_planes *planes_host, const TemporalMotion *tm)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)o->width * o->height, colour = (size_t)o->channels * sizeof(float), hist = temporal_history_bytes(*o);
    /* [node | normal | p | in | history_prev | history_out | colour | variance | age], each 256-byte aligned */
    const void *host[5] = {guides_host->node, guides_host->normal, guides_host->p, in, history_prev};
    void *back[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, history_out, planes_host->colour, planes_host->variance, planes_host->age};
    const size_t bytes[9] = {px * 4, px * 24, px * 24, px * colour, history_prev ? hist : 0, hist, planes_host->colour ? px * colour : 0,
                             planes_host->variance ? px * 4 : 0, planes_host->age ? px * 4 : 0};
    size_t off[9], at = 0;
    for (int i = 0; i < 9; ++i) {
        off[i] = at;
        at = align256(at + bytes[i]);
    }
    /* what may still be in flight where the buffer grows: as for c2rt_denoise — every host variant that wrote the staging
     * ended in a sync of ctx->stream, hipFree waits for the device, no device variant touches ctx->frame */
    if (const int e = ensure_staging(ctx, at)) return e;
    char *dev = reinterpret_cast<char *>(ctx->frame);
    for (int i = 0; i < 5; ++i)
        if (bytes[i]) HIP_TRY(ctx, hipMemcpyAsync(dev + off[i], host[i], bytes[i], hipMemcpyHostToDevice, ctx->stream));
    c2rt_temporal_guides g;
    g.node = reinterpret_cast<const int32_t *>(dev + off[0]);
    g.normal = reinterpret_cast<const double *>(dev + off[1]);
    g.p = reinterpret_cast<const double *>(dev + off[2]);
    c2rt_temporal_planes planes;
    planes.colour = bytes[6] ? reinterpret_cast<float *>(dev + off[6]) : nullptr;
    planes.variance = bytes[7] ? reinterpret_cast<float *>(dev + off[7]) : nullptr;
    planes.age = bytes[8] ? reinterpret_cast<uint32_t *>(dev + off[8]) : nullptr;
    if (const int st = temporal_enqueue(ctx, g, *o, &k, reinterpret_cast<const float *>(dev + off[3]), bytes[4] ? dev + off[4] : nullptr, dev + off[5],
                                        planes, ctx->stream, tm))
        return st;
    for (int i = 5; i < 9; ++i)
        if (bytes[i]) HIP_TRY(ctx, hipMemcpyAsync(back[i], dev + off[i], bytes[i], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return C2RT_OK;
}

int c2rt_temporal_accumulate(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *guides_host, const c2rt_temporal_opts *o,
                             const float *in, const void *history_prev, void *history_out, const c2rt_temporal_planes *planes_host)
{
    TemporalCamera k = {};
    if (const int st = check_temporal(ctx, prev_cam, guides_host, o, in, history_prev, history_out, planes_host, false, k)) return st;
    return temporal_to_host(ctx, k, guides_host, o, in, history_prev, history_out, planes_host, nullptr);
}

int c2rt_temporal_accumulate_motion(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *guides_host, const c2rt_temporal_opts *o,
                                    const c2rt_temporal_motion *motion, const float *in, const void *history_prev, void *history_out,
                                    const c2rt_temporal_planes *planes_host)
{
    TemporalCamera k = {};
    TemporalMotion tm;
    if (const int st = check_temporal(ctx, prev_cam, guides_host, o, in, history_prev, history_out, planes_host, false, k, motion, &tm)) return st;
    return temporal_to_host(ctx, k, guides_host, o, in, history_prev, history_out, planes_host, &tm);
}

/* ---- path counts: the count rule over the previous history (c2rt_path_counts.hip) --------------------------------------- */

/* the count options' own refusals, in the documented order */
static int check_path_count_opts(c2rt_ctx *ctx, const c2rt_path_count_opts *pc)
{
    const unsigned most = C2RT_MAX_PATHS;
    if (pc->min_paths == 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "min_paths is 0: a pixel traced with no path folds a zero into the temporal mean");
    if (pc->min_paths > most) return fail(ctx, C2RT_ERR_LIMIT, "min_paths is %u (at most %u)", (unsigned)pc->min_paths, most);
    if (pc->max_paths < pc->min_paths) return fail(ctx, C2RT_ERR_INVALID_ARG, "max_paths is %u: below min_paths %u", (unsigned)pc->max_paths, (unsigned)pc->min_paths);
    if (pc->max_paths > most) return fail(ctx, C2RT_ERR_LIMIT, "max_paths is %u (at most %u)", (unsigned)pc->max_paths, most);
    if (pc->young_paths == 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "young_paths is 0: at least one path");
    if (pc->young_paths > most) return fail(ctx, C2RT_ERR_LIMIT, "young_paths is %u (at most %u)", (unsigned)pc->young_paths, most);
    if (pc->min_age > (uint32_t)C2RT_MAX_TEMPORAL_AGE) return fail(ctx, C2RT_ERR_LIMIT, "min_age is %u (at most %u)", (unsigned)pc->min_age, (unsigned)C2RT_MAX_TEMPORAL_AGE);
    if (pc->prev_paths == 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "prev_paths is 0: at least one path");
    if (pc->prev_paths > most) return fail(ctx, C2RT_ERR_LIMIT, "prev_paths is %u (at most %u)", (unsigned)pc->prev_paths, most);
    if (!std::isfinite(pc->paths_per_variance) || !(pc->paths_per_variance > 0))
        return fail(ctx, C2RT_ERR_INVALID_ARG, "paths_per_variance %g: finite and above 0", (double)pc->paths_per_variance);
    if (pc->reserved[0] != 0 || pc->reserved[1] != 0)
        return fail(ctx, C2RT_ERR_INVALID_ARG, "c2rt_path_count_opts.reserved is %u, %u: must be 0", (unsigned)pc->reserved[0], (unsigned)pc->reserved[1]);
    return C2RT_OK;
}

/* every refusal of c2rt_path_counts_device, in the documented order; aligned false: the host variant */
static int check_path_counts(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *g, const c2rt_temporal_opts *o,
                             const c2rt_path_count_opts *pc, const void *history_prev, const uint8_t *counts, bool aligned, TemporalCamera &k)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (!o) return fail(ctx, C2RT_ERR_INVALID_ARG, "null temporal options");
    if (!g) return fail(ctx, C2RT_ERR_INVALID_ARG, "null temporal guides");
    if (const int st = check_temporal_frame_opts(ctx, o)) return st;
    if (!pc) return fail(ctx, C2RT_ERR_INVALID_ARG, "null path count options");
    if (const int st = check_path_count_opts(ctx, pc)) return st;
    if (!g->node) return fail(ctx, C2RT_ERR_INVALID_ARG, "null guide: node");
    if (!g->normal) return fail(ctx, C2RT_ERR_INVALID_ARG, "null guide: normal");
    if (!g->p) return fail(ctx, C2RT_ERR_INVALID_ARG, "null guide: p");
    if (!counts) return fail(ctx, C2RT_ERR_INVALID_ARG, "null counts");
    if (history_prev && !prev_cam) return fail(ctx, C2RT_ERR_INVALID_ARG, "a previous history without its camera: null prev_cam");
    if (history_prev)
        if (const int st = check_previous_camera(ctx, *prev_cam, *o, k)) return st;
    if (aligned && reinterpret_cast<uintptr_t>(history_prev) % 16 != 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "a history is not 16-byte aligned");
    return C2RT_OK;
}

static int path_counts_enqueue(c2rt_ctx *ctx, const c2rt_temporal_guides &g, const c2rt_temporal_opts &o, const c2rt_path_count_opts &pc,
                               const TemporalCamera *k, const void *history_prev, const uint8_t *prev_counts, uint8_t *counts, float *variance,
                               uint32_t *age, void *stream)
{
    const int e = launch_path_counts(g, o, pc, history_prev ? k : nullptr, history_prev, prev_counts, counts, variance, age, stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "path count kernel launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

int c2rt_path_counts_device(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *guides_dev, const c2rt_temporal_opts *o,
                            const c2rt_path_count_opts *pc, const void *history_prev_dev, const uint8_t *prev_counts_dev, uint8_t *counts_dev,
                            float *variance_dev, uint32_t *age_dev, void *hip_stream)
{
    TemporalCamera k = {};
    if (const int st = check_path_counts(ctx, prev_cam, guides_dev, o, pc, history_prev_dev, counts_dev, true, k)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return path_counts_enqueue(ctx, *guides_dev, *o, *pc, &k, history_prev_dev, prev_counts_dev, counts_dev, variance_dev, age_dev, hip_stream);
}

int c2rt_path_counts(c2rt_ctx *ctx, const c2rt_camera_frame *prev_cam, const c2rt_temporal_guides *guides_host, const c2rt_temporal_opts *o,
                     const c2rt_path_count_opts *pc, const void *history_prev, const uint8_t *prev_counts, uint8_t *counts, float *variance, uint32_t *age)
{
    TemporalCamera k = {};
    if (const int st = check_path_counts(ctx, prev_cam, guides_host, o, pc, history_prev, counts, false, k)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)o->width * o->height;
    /* [node | normal | p | history_prev | prev_counts | counts | variance | age], each 256-byte aligned, whole */
    const void *host[5] = {guides_host->node, guides_host->normal, guides_host->p, history_prev, history_prev ? prev_counts : nullptr};
    void *back[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, counts, variance, age};
    const size_t bytes[8] = {px * 4, px * 24, px * 24, history_prev ? temporal_history_bytes(*o) : 0, host[4] ? px : 0, px, variance ? px * 4 : 0, age ? px * 4 : 0};
    size_t off[8], at = 0;
    for (int i = 0; i < 8; ++i) {
        off[i] = at;
        at = align256(at + bytes[i]);
    }
    if (const int e = ensure_staging(ctx, at)) return e; /* what may be in flight where it grows: as for c2rt_temporal_accumulate */
    char *dev = reinterpret_cast<char *>(ctx->frame);
    for (int i = 0; i < 5; ++i)
        if (bytes[i]) HIP_TRY(ctx, hipMemcpyAsync(dev + off[i], host[i], bytes[i], hipMemcpyHostToDevice, ctx->stream));
    c2rt_temporal_guides g;
    g.node = reinterpret_cast<const int32_t *>(dev + off[0]);
    g.normal = reinterpret_cast<const double *>(dev + off[1]);
    g.p = reinterpret_cast<const double *>(dev + off[2]);
    if (const int st = path_counts_enqueue(ctx, g, *o, *pc, &k, bytes[3] ? dev + off[3] : nullptr, bytes[4] ? reinterpret_cast<const uint8_t *>(dev + off[4]) : nullptr,
                                           reinterpret_cast<uint8_t *>(dev + off[5]), bytes[6] ? reinterpret_cast<float *>(dev + off[6]) : nullptr,
                                           bytes[7] ? reinterpret_cast<uint32_t *>(dev + off[7]) : nullptr, ctx->stream))
        return st;
    for (int i = 5; i < 8; ++i)
        if (bytes[i]) HIP_TRY(ctx, hipMemcpyAsync(back[i], dev + off[i], bytes[i], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return C2RT_OK;
}

/* ---- variance-guided denoise: the filter steered by the temporal planes (c2rt_denoise_variance.hip) ---------------------- */

/* the options' own refusals, in the documented order (`ctx` null: the status alone) */
static int check_denoise_variance_opts(c2rt_ctx *ctx, const c2rt_denoise_variance_opts *o)
{
    if (!o->width || !o->height)
        return fail(ctx, C2RT_ERR_INVALID_ARG, "variance denoise frame of %u x %u pixels: both must be above 0", (unsigned)o->width, (unsigned)o->height);
    if (o->channels != 1 && o->channels != 3) return fail(ctx, C2RT_ERR_INVALID_ARG, "variance denoise channels is %u: 1 or 3", (unsigned)o->channels);
    if (!(o->sigma_plane > 0) || !std::isfinite(o->sigma_plane))
        return fail(ctx, C2RT_ERR_INVALID_ARG, "sigma_plane %g: a finite length above 0", (double)o->sigma_plane);
    if (!(o->sigma_lum >= 0) || !std::isfinite(o->sigma_lum))
        return fail(ctx, C2RT_ERR_INVALID_ARG, "sigma_lum %g: finite and not negative", (double)o->sigma_lum);
    if (!(o->var_floor > 0) || !std::isfinite(o->var_floor)) return fail(ctx, C2RT_ERR_INVALID_ARG, "var_floor %g: finite and above 0", (double)o->var_floor);
    if (o->reserved != 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "c2rt_denoise_variance_opts.reserved is %u: must be 0", (unsigned)o->reserved);
    if (o->levels > C2RT_MAX_DENOISE_LEVELS)
        return fail(ctx, C2RT_ERR_LIMIT, "%u denoise levels (at most %u)", (unsigned)o->levels, (unsigned)C2RT_MAX_DENOISE_LEVELS);
    if (o->normal_power_log2 > 7) return fail(ctx, C2RT_ERR_LIMIT, "normal_power_log2 is %u (at most 7)", (unsigned)o->normal_power_log2);
    if (o->min_age > (uint32_t)C2RT_MAX_VARIANCE_MIN_AGE)
        return fail(ctx, C2RT_ERR_LIMIT, "min_age is %u (at most %u)", (unsigned)o->min_age, (unsigned)C2RT_MAX_VARIANCE_MIN_AGE);
    return C2RT_OK;
}

/* every refusal of c2rt_denoise_variance_device, in the documented order; with_scratch false: the host variant, whose
 * scratch is the library's own */
static int check_denoise_variance(c2rt_ctx *ctx, const c2rt_denoise_guides *g, const c2rt_denoise_variance_opts *o, const float *variance, const float *in,
                                  const float *out, const float *variance_out, const void *scratch, bool with_scratch)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (!o) return fail(ctx, C2RT_ERR_INVALID_ARG, "null variance denoise options");
    if (!g) return fail(ctx, C2RT_ERR_INVALID_ARG, "null denoise guides");
    if (const int st = check_denoise_variance_opts(ctx, o)) return st;
    if (!g->node) return fail(ctx, C2RT_ERR_INVALID_ARG, "null guide: node");
    if (!g->normal) return fail(ctx, C2RT_ERR_INVALID_ARG, "null guide: normal");
    if (!g->p) return fail(ctx, C2RT_ERR_INVALID_ARG, "null guide: p");
    if (!variance) return fail(ctx, C2RT_ERR_INVALID_ARG, "null variance plane");
    if (!in) return fail(ctx, C2RT_ERR_INVALID_ARG, "null denoise input");
    if (!out) return fail(ctx, C2RT_ERR_INVALID_ARG, "null denoise output");
    if (out == in) return fail(ctx, C2RT_ERR_INVALID_ARG, "denoise output is the input: the filter does not run in place");
    if (variance_out == variance) return fail(ctx, C2RT_ERR_INVALID_ARG, "variance output is the variance plane: the filter does not run in place");
    if (!with_scratch) return C2RT_OK;
    if (scratch && out == scratch) return fail(ctx, C2RT_ERR_INVALID_ARG, "denoise output is the scratch");
    if (scratch && variance_out == scratch) return fail(ctx, C2RT_ERR_INVALID_ARG, "variance output is the scratch");
    if (!scratch && c2rt_denoise_variance_scratch_bytes(o) != 0)
        return fail(ctx, C2RT_ERR_INVALID_ARG, "null denoise scratch: these options need %zu bytes", c2rt_denoise_variance_scratch_bytes(o));
    if (reinterpret_cast<uintptr_t>(scratch) % 16 != 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "denoise scratch is not 16-byte aligned");
    if (scratch && in == scratch) return fail(ctx, C2RT_ERR_INVALID_ARG, "denoise input is the scratch");
    if (scratch && variance == scratch) return fail(ctx, C2RT_ERR_INVALID_ARG, "variance plane is the scratch");
    return C2RT_OK;
}

/* the contract's per-call factors, in fp32, and the launches */
static int denoise_variance_enqueue(c2rt_ctx *ctx, const c2rt_denoise_guides &g, const c2rt_denoise_variance_opts &o, const float *variance,
                                    const uint32_t *age, const float *in, float *out, float *variance_out, void *scratch, void *stream)
{
    const float inv_plane = 1.0f / o.sigma_plane;
    const volatile float sl2 = o.sigma_lum * o.sigma_lum;
    const int e = launch_denoise_variance(g, o, inv_plane, sl2, variance, age, in, out, variance_out, scratch, stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "variance denoise kernel launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

size_t c2rt_denoise_variance_scratch_bytes(const c2rt_denoise_variance_opts *o)
{
    if (!o || check_denoise_variance_opts(nullptr, o) != C2RT_OK) return 0;
    return denoise_variance_scratch_bytes(*o);
}

int c2rt_denoise_variance_device(c2rt_ctx *ctx, const c2rt_denoise_guides *guides_dev, const c2rt_denoise_variance_opts *o, const float *variance_dev,
                                 const uint32_t *age_dev, const float *in_dev, float *out_dev, float *variance_out_dev, void *scratch_dev, void *hip_stream)
{
    if (const int st = check_denoise_variance(ctx, guides_dev, o, variance_dev, in_dev, out_dev, variance_out_dev, scratch_dev, true)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return denoise_variance_enqueue(ctx, *guides_dev, *o, variance_dev, age_dev, in_dev, out_dev, variance_out_dev, scratch_dev, hip_stream);
}

int c2rt_denoise_variance(c2rt_ctx *ctx, const c2rt_denoise_guides *guides_host, const c2rt_denoise_variance_opts *o, const float *variance,
                          const uint32_t *age, const float *in, float *out, float *variance_out)
{
    if (const int st = check_denoise_variance(ctx, guides_host, o, variance, in, out, variance_out, nullptr, false)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)o->width * o->height, colour = (size_t)o->channels * sizeof(float);
    /* [node | normal | p | albedo | base | variance | age | in | out | variance_out | scratch], each 256-byte aligned */
    const void *host[8] = {guides_host->node, guides_host->normal, guides_host->p, guides_host->albedo, guides_host->base, variance, age, in};
    const size_t bytes[11] = {px * 4, px * 24, px * 24, guides_host->albedo ? px * colour : 0, guides_host->base ? px * colour : 0, px * 4,
                              age ? px * 4 : 0, px * colour, px * colour, variance_out ? px * 4 : 0, c2rt_denoise_variance_scratch_bytes(o)};
    size_t off[11], at = 0;
    for (int k = 0; k < 11; ++k) {
        off[k] = at;
        at = align256(at + bytes[k]);
    }
    if (const int e = ensure_staging(ctx, at)) return e;
    char *dev = reinterpret_cast<char *>(ctx->frame);
    for (int k = 0; k < 8; ++k)
        if (bytes[k]) HIP_TRY(ctx, hipMemcpyAsync(dev + off[k], host[k], bytes[k], hipMemcpyHostToDevice, ctx->stream));
    c2rt_denoise_guides g;
    g.node = reinterpret_cast<const int32_t *>(dev + off[0]);
    g.normal = reinterpret_cast<const double *>(dev + off[1]);
    g.p = reinterpret_cast<const double *>(dev + off[2]);
    g.albedo = bytes[3] ? reinterpret_cast<const float *>(dev + off[3]) : nullptr;
    g.base = bytes[4] ? reinterpret_cast<const float *>(dev + off[4]) : nullptr;
    if (const int st = denoise_variance_enqueue(ctx, g, *o, reinterpret_cast<const float *>(dev + off[5]),
                                                bytes[6] ? reinterpret_cast<const uint32_t *>(dev + off[6]) : nullptr,
                                                reinterpret_cast<const float *>(dev + off[7]), reinterpret_cast<float *>(dev + off[8]),
                                                bytes[9] ? reinterpret_cast<float *>(dev + off[9]) : nullptr, bytes[10] ? dev + off[10] : nullptr, ctx->stream))
        return st;
    HIP_TRY(ctx, hipMemcpyAsync(out, dev + off[8], bytes[8], hipMemcpyDeviceToHost, ctx->stream));
    if (bytes[9]) HIP_TRY(ctx, hipMemcpyAsync(variance_out, dev + off[9], bytes[9], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return C2RT_OK;
}

/* The scene states of a posed sequence (c2rt_render_paths_sequence_posed*): the base's posable values, and for frame i
 * the update that takes the context from frame i - 1's scene (the base's for i == 0) to the base patched by poses[i] —
 * every node and light either pose names, with its value in frame i's scene — and the motion list of its accumulation. */
struct PosedSequence {
    std::vector<double> node_transform, light_pos; /* the base's */
    std::vector<float> light_color, light_power;
    std::vector<TemporalMotion> motion;            /* [n_frames]; motion[0] empty */

    struct Step {
        std::vector<uint32_t> node_index, light_index;
        std::vector<double> node_transform, light_pos;
        std::vector<float> light_color, light_power;
        c2rt_scene_pose pose{};
    };

    /* `named` in ascending order without repeats: what either pose lists */
    static std::vector<uint32_t> named(const uint32_t *a, uint32_t na, const uint32_t *b, uint32_t nb)
    {
        std::vector<uint32_t> v(a, a + na);
        v.insert(v.end(), b, b + nb);
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        return v;
    }
    static const double *transform_under(const c2rt_scene_pose *pose, uint32_t node, const std::vector<double> &base)
    {
        if (pose)
            for (uint32_t k = 0; k < pose->n_nodes; ++k)
                if (pose->node_index[k] == node) return pose->node_transform + 30 * (size_t)k;
        return &base[30 * (size_t)node];
    }

    /* the update that names every node and light `from` or `to` names (either may be null) and gives each its value under
     * `target` (null: the base's).  Frame i: (poses[i - 1], poses[i], poses[i]); the way back: (.., .., null). */
    void step(const c2rt_scene_pose *from, const c2rt_scene_pose *to, const c2rt_scene_pose *target, Step &s) const
    {
        s.node_index = named(from ? from->node_index : nullptr, from ? from->n_nodes : 0, to ? to->node_index : nullptr, to ? to->n_nodes : 0);
        s.light_index = named(from ? from->light_index : nullptr, from ? from->n_lights : 0, to ? to->light_index : nullptr, to ? to->n_lights : 0);
        s.node_transform.resize(30 * s.node_index.size());
        for (size_t k = 0; k < s.node_index.size(); ++k)
            std::memcpy(&s.node_transform[30 * k], transform_under(target, s.node_index[k], node_transform), 30 * sizeof(double));
        s.light_pos.resize(3 * s.light_index.size());
        s.light_color.resize(3 * s.light_index.size());
        s.light_power.resize(s.light_index.size());
        for (size_t k = 0; k < s.light_index.size(); ++k) {
            const size_t l = s.light_index[k];
            std::memcpy(&s.light_pos[3 * k], &light_pos[3 * l], 3 * sizeof(double));
            std::memcpy(&s.light_color[3 * k], &light_color[3 * l], 3 * sizeof(float));
            s.light_power[k] = light_power[l];
            for (uint32_t j = 0; target && j < target->n_lights; ++j) {
                if (target->light_index[j] != l) continue;
                if (target->light_pos) std::memcpy(&s.light_pos[3 * k], target->light_pos + 3 * (size_t)j, 3 * sizeof(double));
                if (target->light_color) std::memcpy(&s.light_color[3 * k], target->light_color + 3 * (size_t)j, 3 * sizeof(float));
                if (target->light_power) s.light_power[k] = target->light_power[j];
            }
        }
        s.pose = c2rt_scene_pose{};
        s.pose.n_nodes = (uint32_t)s.node_index.size();
        s.pose.node_index = s.node_index.data();
        s.pose.node_transform = s.node_transform.data();
        s.pose.n_lights = (uint32_t)s.light_index.size();
        s.pose.light_index = s.light_index.data();
        s.pose.light_pos = s.light_pos.data();
        s.pose.light_color = s.light_color.data();
        s.pose.light_power = s.light_power.data();
    }
};

/* The posed sequence's own refusals, behind the unposed call's, and its plan: the poses checked and planned
 * (plan_posed_frames: what c2rt_update_scene would answer to each), the motion list of every frame. */
static int plan_posed_sequence(c2rt_ctx *ctx, const c2rt_scene_pose *poses, uint32_t n_frames, PosedSequence &seq)
{
    if (const int st = check_posed_args(ctx, poses, n_frames)) return st;
    {
        std::vector<std::unique_ptr<PosedFrame>> posed;
        if (const int st = plan_posed_frames(ctx, poses, n_frames, posed)) return st;
    }
    seq.node_transform = ctx->scene.node_transform;
    seq.light_pos = ctx->scene.light_pos;
    seq.light_color = ctx->scene.light_color;
    seq.light_power = ctx->scene.light_power;
    seq.motion.assign(n_frames, TemporalMotion{});
    for (uint32_t i = 1; i < n_frames; ++i) {
        const c2rt_scene_pose &a = poses[i - 1], &b = poses[i];
        uint32_t listed = 0;
        for (const uint32_t node : PosedSequence::named(a.node_index, a.n_nodes, b.node_index, b.n_nodes)) {
            const double *prev = PosedSequence::transform_under(&a, node, seq.node_transform), *cur = PosedSequence::transform_under(&b, node, seq.node_transform);
            if (std::memcmp(prev, cur, 30 * sizeof(double)) == 0) continue;
            if (++listed > (uint32_t)C2RT_MAX_MOTION_NODES) continue;
            motion_record(node, prev, cur, seq.motion[i]);
        }
        if (listed > (uint32_t)C2RT_MAX_MOTION_NODES)
            return fail(ctx, C2RT_ERR_LIMIT, "frame %u: %u nodes moved since frame %u (at most %u)", (unsigned)i, (unsigned)listed, (unsigned)(i - 1),
                        (unsigned)C2RT_MAX_MOTION_NODES);
    }
    return C2RT_OK;
}

/* the five sequence calls: `d` the plain filter's options or `dv` the variance-guided one's, the other null; `posed`: the
 * posed calls, `poses` theirs; `adaptive`: c2rt_render_paths_sequence_adaptive, `pc` its count options */
static int paths_sequence(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts, const c2rt_path_opts *pg,
                          const c2rt_temporal_opts *t, const c2rt_denoise_opts *d, const c2rt_denoise_variance_opts *dv, float *out_rgb,
                          const c2rt_scene_pose *poses = nullptr, bool posed = false, bool adaptive = false, const c2rt_path_count_opts *pc = nullptr)
{
    if (n_frames == 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "n_frames is 0: a sequence has at least one frame");
    if (!t) return fail(ctx, C2RT_ERR_INVALID_ARG, "null temporal options");
    if (t->width != opts->width || t->height != opts->height)
        return fail(ctx, C2RT_ERR_INVALID_ARG, "temporal options for %u x %u pixels, the frame has %u x %u", (unsigned)t->width, (unsigned)t->height,
                    (unsigned)opts->width, (unsigned)opts->height);
    if (t->channels != 3) return fail(ctx, C2RT_ERR_INVALID_ARG, "temporal channels is %u: a frame has 3", (unsigned)t->channels);
    if (const int st = check_temporal_opts(ctx, t)) return st;
    TemporalCamera k = {};
    for (uint32_t i = 1; i < n_frames; ++i) {
        if (cams[i].dof) return fail(ctx, C2RT_ERR_UNSUPPORTED, "camera %u: depth of field: a pixel's paths are one ray's, a lens has many per pixel", (unsigned)i);
        if (cams[i].stereo_separation != 0)
            return fail(ctx, C2RT_ERR_UNSUPPORTED, "camera %u: stereo: a pixel's paths are one ray's, a stereo camera has two per pixel", (unsigned)i);
    }
    for (uint32_t i = 0; i + 1 < n_frames; ++i)
        if (const int st = check_previous_camera(ctx, cams[i], *t, k)) return st;
    PosedSequence seq;
    if (posed)
        if (const int st = plan_posed_sequence(ctx, poses, n_frames, seq)) return st;
    if (adaptive) {
        if (!pc) return fail(ctx, C2RT_ERR_INVALID_ARG, "null path count options");
        if (const int st = check_path_count_opts(ctx, pc)) return st;
        if (pc->max_paths > pg->paths)
            return fail(ctx, C2RT_ERR_INVALID_ARG, "max_paths is %u: above the cap, paths = %u", (unsigned)pc->max_paths, (unsigned)pg->paths);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)opts->width * opts->height, hist = temporal_history_bytes(*t);
    /* [node | normal | p | rgb | albedo | indirect | out | scratch | history 0 | history 1 | variance | age | counts 0 |
     * counts 1 | order], each 256-byte aligned; the accumulated plane the filter reads is the colour plane of the history
     * just written; variance and age for the variance-guided filter only, the two count planes and the count-order scratch
     * for the adaptive call only */
    const size_t bytes[15] = {px * 4, px * 24, px * 24, px * 12, px * 12, px * 12, px * 12, d ? c2rt_denoise_scratch_bytes(d) : c2rt_denoise_variance_scratch_bytes(dv),
                              hist, hist, dv ? px * 4 : 0, dv ? px * 4 : 0, adaptive ? px : 0, adaptive ? px : 0, adaptive ? counted_scratch_bytes(px) : 0};
    size_t off[15], at = 0;
    for (int i = 0; i < 15; ++i) {
        off[i] = at;
        at = align256(at + bytes[i]);
    }
    /* once, before the first launch: the buffer does not move under the sequence, and the call ends in a sync */
    if (const int e = ensure_staging(ctx, at)) return e;
    char *dev = reinterpret_cast<char *>(ctx->frame);
    c2rt_hit_planes hits = {};
    hits.node = reinterpret_cast<int32_t *>(dev + off[0]);
    hits.normal = reinterpret_cast<double *>(dev + off[1]);
    hits.p = reinterpret_cast<double *>(dev + off[2]);
    hits.rgb = reinterpret_cast<float *>(dev + off[3]);
    c2rt_shade_planes shade = {};
    shade.albedo = reinterpret_cast<float *>(dev + off[4]);
    c2rt_path_planes paths = {};
    paths.indirect = reinterpret_cast<float *>(dev + off[5]);
    const c2rt_temporal_guides tg = {hits.node, hits.normal, hits.p};
    const c2rt_denoise_guides dg = {hits.node, hits.normal, hits.p, shade.albedo, hits.rgb};
    c2rt_temporal_planes tp = {};
    if (dv) {
        tp.variance = reinterpret_cast<float *>(dev + off[10]);
        tp.age = reinterpret_cast<uint32_t *>(dev + off[11]);
    }
    const auto frame = [&](uint32_t i) -> int {
        RenderParams p;
        hit_params(ctx, &cams[i], opts, p);
        c2rt_path_opts pgi = *pg;
        pgi.seed = pg->seed + i;
        int e = launch_plane_rows(p, ctx->plan.csg_levels, kNoOpts, hits, 0, p.local_rows, ctx->stream);
        if (e == 0) e = launch_plane_rows(p, ctx->plan.csg_levels, kNoOpts, shade, 0, p.local_rows, ctx->stream);
        char *h_out = dev + off[8 + (i & 1u)], *h_prev = i ? dev + off[8 + ((i - 1) & 1u)] : nullptr;
        if (i) (void)temporal_camera(cams[i - 1], *t, k);
        if (adaptive) { /* the frame's counts: young_paths everywhere, or the rule over the history before this frame is folded in */
            uint8_t *counts = reinterpret_cast<uint8_t *>(dev + off[12 + (i & 1u)]), *counts_prev = reinterpret_cast<uint8_t *>(dev + off[12 + ((i - 1) & 1u)]);
            if (e == 0 && i == 0) e = (int)hipMemsetAsync(counts, (int)pc->young_paths, px, ctx->stream);
            if (e == 0 && i != 0) e = launch_path_counts(tg, *t, *pc, &k, h_prev, counts_prev, counts, nullptr, nullptr, ctx->stream);
            /* frame 0's counts are even: natural order; the rule's are not: count order (profiles/paths_counted.md) */
            if (e == 0) e = launch_counted_rows(p, ctx->plan.csg_levels, pgi, counts, paths, 0, p.local_rows, i ? dev + off[14] : nullptr, ctx->stream);
        } else if (e == 0) e = launch_plane_rows(p, ctx->plan.csg_levels, pgi, paths, 0, p.local_rows, ctx->stream);
        if (e != 0) return fail(ctx, C2RT_ERR_HIP, "path sequence, frame %u, plane kernel launch: %s", (unsigned)i, hipGetErrorString((hipError_t)e));
        if (const int st = temporal_enqueue(ctx, tg, *t, &k, paths.indirect, h_prev, h_out, tp, ctx->stream, posed ? &seq.motion[i] : nullptr)) return st;
        const float *acc = reinterpret_cast<const float *>(h_out + px * 32);
        float *out = reinterpret_cast<float *>(dev + off[6]);
        void *scratch = bytes[7] ? dev + off[7] : nullptr;
        if (const int st = d ? denoise_enqueue(ctx, dg, *d, acc, out, scratch, ctx->stream)
                             : denoise_variance_enqueue(ctx, dg, *dv, tp.variance, tp.age, acc, out, nullptr, scratch, ctx->stream))
            return st;
        HIP_TRY(ctx, hipMemcpyAsync(out_rgb + (size_t)i * px * 3, dev + off[6], bytes[6], hipMemcpyDeviceToHost, ctx->stream));
        return C2RT_OK;
    };
    if (!posed) {
        for (uint32_t i = 0; i < n_frames; ++i)
            if (const int st = frame(i)) return st;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return C2RT_OK;
    }
    /* posed: the scene follows the frames on the same stream (c2rt_update_scene's own path, update_one) and is put back
     * behind the last one — also behind a frame that failed, with that frame's status and message.  The way back names
     * what the last two poses touched: whichever of them the context holds, wholly or in part, it holds the base after. */
    PosedSequence::Step step;
    int st = C2RT_OK;
    const c2rt_scene_pose *before = nullptr, *last = nullptr;
    for (uint32_t i = 0; i < n_frames && st == C2RT_OK; ++i) {
        before = last;
        last = &poses[i];
        seq.step(before, last, last, step);
        if ((st = update_one(ctx, &step.pose, ctx->stream)) == C2RT_OK) st = frame(i);
    }
    const std::string err = ctx->err;
    seq.step(before, last, nullptr, step);
    const int undo = update_one(ctx, &step.pose, ctx->stream);
    if (st != C2RT_OK) ctx->err = err;
    else st = undo;
    if (st != C2RT_OK) return st;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return C2RT_OK;
}

int c2rt_render_paths_sequence(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts, const c2rt_path_opts *pg,
                               const c2rt_temporal_opts *t, const c2rt_denoise_opts *d, float *out_rgb)
{
    if (const int st = check_paths_denoised(ctx, cams, opts, pg, d, out_rgb)) return st;
    return paths_sequence(ctx, cams, n_frames, opts, pg, t, d, nullptr, out_rgb);
}

int c2rt_render_paths_sequence_variance(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts,
                                        const c2rt_path_opts *pg, const c2rt_temporal_opts *t, const c2rt_denoise_variance_opts *dv, float *out_rgb)
{
    if (const int st = check_paths_filtered(ctx, cams, opts, pg, dv != nullptr, dv ? dv->width : 0, dv ? dv->height : 0, dv ? dv->channels : 0, out_rgb))
        return st;
    if (const int st = check_denoise_variance_opts(ctx, dv)) return st;
    return paths_sequence(ctx, cams, n_frames, opts, pg, t, nullptr, dv, out_rgb);
}

int c2rt_render_paths_sequence_adaptive(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts,
                                        const c2rt_path_opts *pg, const c2rt_temporal_opts *t, const c2rt_denoise_variance_opts *dv,
                                        const c2rt_path_count_opts *pc, float *out_rgb)
{
    if (const int st = check_paths_filtered(ctx, cams, opts, pg, dv != nullptr, dv ? dv->width : 0, dv ? dv->height : 0, dv ? dv->channels : 0, out_rgb))
        return st;
    if (const int st = check_denoise_variance_opts(ctx, dv)) return st;
    return paths_sequence(ctx, cams, n_frames, opts, pg, t, nullptr, dv, out_rgb, nullptr, false, true, pc);
}

int c2rt_render_paths_sequence_posed(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, uint32_t n_frames,
                                     const c2rt_render_opts *opts, const c2rt_path_opts *pg, const c2rt_temporal_opts *t, const c2rt_denoise_opts *d,
                                     float *out_rgb)
{
    if (const int st = check_paths_denoised(ctx, cams, opts, pg, d, out_rgb)) return st;
    return paths_sequence(ctx, cams, n_frames, opts, pg, t, d, nullptr, out_rgb, poses, true);
}

int c2rt_render_paths_sequence_posed_variance(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, uint32_t n_frames,
                                              const c2rt_render_opts *opts, const c2rt_path_opts *pg, const c2rt_temporal_opts *t,
                                              const c2rt_denoise_variance_opts *dv, float *out_rgb)
{
    if (const int st = check_paths_filtered(ctx, cams, opts, pg, dv != nullptr, dv ? dv->width : 0, dv ? dv->height : 0, dv ? dv->channels : 0, out_rgb))
        return st;
    if (const int st = check_denoise_variance_opts(ctx, dv)) return st;
    return paths_sequence(ctx, cams, n_frames, opts, pg, t, nullptr, dv, out_rgb, poses, true);
}

/* ---- hit layers: every surface along a ray or pixel (c2rt_layers.hip) --------------------------------------------- */

/* the refusals the two faces share, behind the single-hit call's own; out_ok: some output is there */
static int check_layer_args(c2rt_ctx *ctx, uint32_t max_layers, bool out_ok)
{
    if (max_layers == 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "max_layers is 0: at least one layer");
    if (max_layers > (uint32_t)C2RT_MAX_HIT_LAYERS)
        return fail(ctx, C2RT_ERR_LIMIT, "%u layers in one call (at most %u)", (unsigned)max_layers, (unsigned)C2RT_MAX_HIT_LAYERS);
    if (!out_ok) return fail(ctx, C2RT_ERR_INVALID_ARG, "no output asked for: every output pointer is null");
    return C2RT_OK;
}

int c2rt_trace_rays_layers_device(c2rt_ctx *ctx, const c2rt_ray *rays_dev, uint64_t n, uint32_t max_layers, c2rt_ray_hit *hits_dev,
                                  float *rgb_dev, uint8_t *count_dev, void *hip_stream)
{
    if (const int st = check_query_args(ctx, rays_dev, n, true)) return st < 0 ? C2RT_OK : st;
    if (const int st = check_layer_args(ctx, max_layers, hits_dev || rgb_dev || count_dev)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    query_params(ctx, p);
    const int e = launch_trace_ray_layers(p, ctx->plan.csg_levels, rays_dev, n, max_layers, n, hits_dev, rgb_dev, count_dev, hip_stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "hit layer kernel launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

/* Host variant: c2rt_trace_rays' staging with kQueryChunk / max_layers rays per chunk, the chunk's layers side by side
 * (layer stride = chunk size), so [inputs | hits | colours | counts] is never larger than that call's buffer plus the
 * counts.  Each layer's slice of a chunk goes to its place in the caller's layer-major arrays. */
int c2rt_trace_rays_layers(c2rt_ctx *ctx, const c2rt_ray *rays, uint64_t n, uint32_t max_layers, c2rt_ray_hit *hits, float *rgb, uint8_t *count)
{
    if (const int st = check_query_args(ctx, rays, n, true)) return st < 0 ? C2RT_OK : st;
    if (const int st = check_layer_args(ctx, max_layers, hits || rgb || count)) return st;
    Staging outs;
    outs.add(hits, sizeof(c2rt_ray_hit), max_layers);
    outs.add(rgb, 3 * sizeof(float), max_layers);
    outs.add(count, 1);
    return ray_chunks(ctx, rays, n, kQueryChunk / max_layers, outs, "hit layer", [&](const RenderParams &p, const c2rt_ray *rays_dev, uint64_t, uint64_t m, uint64_t chunk) {
        return launch_trace_ray_layers(p, ctx->plan.csg_levels, rays_dev, m, max_layers, chunk, outs.dev<c2rt_ray_hit>(0), outs.dev<float>(1), outs.dev<uint8_t>(2),
                                       ctx->stream);
    });
}

/* the refusals of the frame face, in the documented order: a frame call's, null planes, the layers', then the modes in
 * which a pixel is not one ray, worded as check_frame_planes words them for the hit planes */
static int check_hit_layer_args(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, uint32_t max_layers,
                                const c2rt_hit_planes *planes, const uint8_t *count)
{
    if (const int st = check_frame_args(ctx, cam, opts)) return st;
    if (!planes) return fail(ctx, C2RT_ERR_INVALID_ARG, "null planes");
    if (const int st = check_layer_args(ctx, max_layers, any_plane(*planes) || count)) return st;
    return check_one_ray_per_pixel(ctx, cam, opts, Family<c2rt_hit_planes>::holds, Family<c2rt_hit_planes>::planes);
}

int c2rt_render_hit_layers_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, uint32_t max_layers,
                                  const c2rt_hit_planes *planes_dev, uint8_t *count_dev, void *hip_stream)
{
    if (const int st = check_hit_layer_args(ctx, cam, opts, max_layers, planes_dev, count_dev)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    hit_params(ctx, cam, opts, p);
    if (p.local_rows == 0) return C2RT_OK;
    const int e = launch_hit_layers(p, ctx->plan.csg_levels, *planes_dev, count_dev, max_layers, (size_t)p.local_rows * p.width, 0, p.local_rows, hip_stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "hit layer kernel launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

/* Host variant: c2rt_render_hits' staging with chunks of whole rows of at most kQueryChunk / max_layers pixels (one row
 * at least), the chunk's layers side by side in every plane (layer stride = chunk pixels), then the counts. */
int c2rt_render_hit_layers(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, uint32_t max_layers,
                           const c2rt_hit_planes *planes_host, uint8_t *count_host)
{
    if (const int st = check_hit_layer_args(ctx, cam, opts, max_layers, planes_host, count_host)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    hit_params(ctx, cam, opts, p);
    if (p.local_rows == 0) return C2RT_OK;
    Staging outs;
    outs.add_planes(*planes_host, max_layers);
    outs.add(count_host, 1);
    return row_chunks(ctx, p, max_layers, outs, "hit layer", [&](uint32_t r0, uint32_t m, size_t chunk_px) {
        return launch_hit_layers(p, ctx->plan.csg_levels, outs.planes<c2rt_hit_planes>(), outs.dev<uint8_t>(kPlanes<c2rt_hit_planes>), max_layers, chunk_px, r0, m,
                                 ctx->stream);
    });
}

/* ---- hit planes of a batch of frames (c2rt_hit_planes.hip: hit_planes_batch_kernel) ------------------------------- */

/* The refusals of the four batch entry points, in the documented order: a batch call's (depth of field, stereo,
 * count_rays, prepass_bucket and a multi-device context are among them), then the planes', then, for the posed calls
 * (poses_given), the poses'. */
static int check_hit_batch_args(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, bool poses_given,
                                uint32_t n_frames, const c2rt_render_opts *opts, const c2rt_hit_planes *planes)
{
    if (const int st = check_batch_args(ctx, cams, n_frames, opts)) return st;
    if (const int st = check_planes(ctx, &kNoOpts, planes)) return st;
    if (poses_given)
        if (const int st = check_posed_args(ctx, poses, n_frames)) return st;
    return C2RT_OK;
}

/* The batch's device table, built in ctx->batch_host and copied with one stream-ordered copy into the scratch slot of
 * `stream` (FrameScratch::batch_table, as render_frames_device's): n_frames parameter blocks, block i what hit_params
 * makes for frame i from its own plan — by FRAME, there is no `order` here: the query kernels have one instance per CSG
 * depth and light count, which no pose changes, so every frame runs the same kernel whatever its pose (no plane and no
 * identity instances: c2rt_query.inc) — then the node and light tables of the posed frames whose pose changes them,
 * which is all of a posed plan the query kernels read (the shadow rectangles and the dark-tile table are the mask
 * pre-pass's).  No tile-mask table, no retry list.  p0: the host copy of block 0.  The arguments have passed
 * check_hit_batch_args; local_rows is not 0. */
static int hit_batch_table(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const std::vector<std::unique_ptr<PosedFrame>> *posed,
                           uint32_t n_frames, const c2rt_render_opts *opts, hipStream_t stream, const RenderParams **table_dev,
                           RenderParams &p0)
{
    const size_t n = n_frames;
    const auto own = [&](size_t i) { return posed ? (*posed)[i].get() : nullptr; };
    const size_t posed_at = align16(n * sizeof(RenderParams));
    size_t bytes = posed_at;
    for (size_t i = 0; i < n; ++i)
        if (const PosedFrame *f = own(i))
            bytes += (f->own_nodes ? align16(f->plan.nodes.size() * sizeof(DevNode)) : 0) +
                     (f->own_lights ? align16(f->plan.lights.size() * sizeof(DevLight)) : 0);
    ctx->batch_host.resize(bytes);
    RenderParams *hp = reinterpret_cast<RenderParams *>(ctx->batch_host.data());

    FrameScratch &sc = scratch_for(ctx, stream);
    const hipError_t e = grow_scratch(&sc.batch_table, &sc.batch_bytes, bytes, 1);
    if (e != hipSuccess) return fail(ctx, C2RT_ERR_HIP, "batch scratch: %s", hipGetErrorString(e));

    size_t at = posed_at;
    /* one of a posed frame's own tables: into the host image, its device address into the frame's block */
    const auto place = [&](const void *src, size_t table_bytes) {
        std::memcpy(ctx->batch_host.data() + at, src, table_bytes);
        const char *dev = sc.batch_table + at;
        at += align16(table_bytes);
        return dev;
    };
    for (size_t i = 0; i < n; ++i) {
        const PosedFrame *f = own(i);
        RenderParams &p = hp[i];
        fill_params(f ? f->plan : ctx->plan, ctx->dev, diag_knobs(), &cams[i], opts, p);
        hit_settings(ctx, p);
        if (f && f->own_nodes) p.nodes = reinterpret_cast<const DevNode *>(place(f->plan.nodes.data(), f->plan.nodes.size() * sizeof(DevNode)));
        if (f && f->own_lights) p.lights = reinterpret_cast<const DevLight *>(place(f->plan.lights.data(), f->plan.lights.size() * sizeof(DevLight)));
    }
    HIP_TRY(ctx, hipMemcpyAsync(sc.batch_table, ctx->batch_host.data(), bytes, hipMemcpyHostToDevice, stream));
    *table_dev = reinterpret_cast<const RenderParams *>(sc.batch_table);
    p0 = hp[0];
    return C2RT_OK;
}

/* Both device variants (poses_given: the posed one): the table copy and ONE launch for all frames on `hip_stream`. */
static int hit_batch_to_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, bool poses_given,
                               uint32_t n_frames, const c2rt_render_opts *opts, const c2rt_hit_planes *planes_dev, void *hip_stream)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (n_frames == 0) return C2RT_OK;
    if (const int st = check_hit_batch_args(ctx, cams, poses, poses_given, n_frames, opts, planes_dev)) return st;
    std::vector<std::unique_ptr<PosedFrame>> posed;
    if (poses_given)
        if (const int st = plan_posed_frames(ctx, poses, n_frames, posed)) return st;
    const uint32_t rows = c2rt_local_rows(opts);
    if (rows == 0) return C2RT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const RenderParams *table_dev = nullptr;
    RenderParams p0;
    if (const int st = hit_batch_table(ctx, cams, poses_given ? &posed : nullptr, n_frames, opts, static_cast<hipStream_t>(hip_stream), &table_dev, p0)) return st;
    const int e = launch_hit_planes_batch(p0, ctx->plan.csg_levels, table_dev, n_frames, (size_t)rows * opts->width, *planes_dev, 0, rows, hip_stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "hit plane batch kernel launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

/* Both host variants, on the context's stream through the context's staging allocation, which holds one chunk of at
 * most kQueryChunk pixels of the planes asked for, plane after plane (92 B per pixel, 23 MiB at most, as
 * c2rt_render_hits).  A frame of at most kQueryChunk pixels: a chunk is as many WHOLE frames as fit — one launch, one
 * copy back per plane (the frames are contiguous on both sides), one stream sync.  A larger frame: frame by frame in
 * chunks of whole rows, as c2rt_render_hits, each a launch over one block of the table.  The table goes up once. */
static int hit_batch_to_host(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, bool poses_given,
                             uint32_t n_frames, const c2rt_render_opts *opts, const c2rt_hit_planes *planes_host)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (n_frames == 0) return C2RT_OK;
    if (const int st = check_hit_batch_args(ctx, cams, poses, poses_given, n_frames, opts, planes_host)) return st;
    std::vector<std::unique_ptr<PosedFrame>> posed;
    if (poses_given)
        if (const int st = plan_posed_frames(ctx, poses, n_frames, posed)) return st;
    const uint32_t rows = c2rt_local_rows(opts), width = opts->width;
    if (rows == 0) return C2RT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t frame_px = (size_t)rows * width;
    const bool whole = frame_px <= kQueryChunk;
    /* whole frames per chunk, or rows of one frame per chunk (width <= 2^16: at least four rows) */
    uint32_t chunk_frames = whole ? (uint32_t)(kQueryChunk / frame_px) : 1u;
    if (chunk_frames > n_frames) chunk_frames = n_frames;
    uint32_t chunk_rows = whole ? rows : (uint32_t)(kQueryChunk / width);
    if (chunk_rows > rows) chunk_rows = rows;
    const size_t chunk_px = (size_t)chunk_frames * chunk_rows * width;
    Staging outs;
    outs.add_planes(*planes_host);
    if (const int e = lay_out(ctx, outs, 0, chunk_px)) return e;
    const c2rt_hit_planes d = outs.planes<c2rt_hit_planes>();
    const RenderParams *table_dev = nullptr;
    RenderParams p0;
    if (const int st = hit_batch_table(ctx, cams, poses_given ? &posed : nullptr, n_frames, opts, ctx->stream, &table_dev, p0)) return st;
    for (uint32_t f0 = 0; f0 < n_frames; f0 += chunk_frames) {
        const uint32_t nf = n_frames - f0 < chunk_frames ? n_frames - f0 : chunk_frames;
        for (uint32_t r0 = 0; r0 < rows; r0 += chunk_rows) {
            const uint32_t m = rows - r0 < chunk_rows ? rows - r0 : chunk_rows;
            /* whole frames: the staged slices are frame_px apart, as the caller's; row chunks: one frame, no stride */
            const int e = launch_hit_planes_batch(p0, ctx->plan.csg_levels, table_dev + f0, nf, frame_px, d, r0, m, ctx->stream);
            if (e != 0) return fail(ctx, C2RT_ERR_HIP, "hit plane batch kernel launch: %s", hipGetErrorString((hipError_t)e));
            const size_t first = (size_t)f0 * frame_px + (size_t)r0 * width, px = (size_t)(nf - 1) * frame_px + (size_t)m * width;
            if (const int st = copy_back(ctx, outs, first, px, 0, 0)) return st;
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    return C2RT_OK;
}

int c2rt_render_frames_hits_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts,
                                   const c2rt_hit_planes *planes_dev, void *hip_stream)
{
    return hit_batch_to_device(ctx, cams, nullptr, false, n_frames, opts, planes_dev, hip_stream);
}

int c2rt_render_frames_hits(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts,
                            const c2rt_hit_planes *planes_host)
{
    return hit_batch_to_host(ctx, cams, nullptr, false, n_frames, opts, planes_host);
}

int c2rt_render_frames_posed_hits_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, uint32_t n_frames,
                                         const c2rt_render_opts *opts, const c2rt_hit_planes *planes_dev, void *hip_stream)
{
    return hit_batch_to_device(ctx, cams, poses, true, n_frames, opts, planes_dev, hip_stream);
}

int c2rt_render_frames_posed_hits(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, uint32_t n_frames,
                                  const c2rt_render_opts *opts, const c2rt_hit_planes *planes_host)
{
    return hit_batch_to_host(ctx, cams, poses, true, n_frames, opts, planes_host);
}

/* ---- adaptive anti-aliasing (c2rt_adaptive.hip) ------------------------------------------------------------------- */

/* What every adaptive call refuses behind its own first checks, in the documented order: the threshold and the outputs,
 * then the modes in which a pixel is not five rays of its own or its neighbours are not in this frame.  cam null: a
 * batch call, whose own refusals (check_batch_args) have covered all of those modes but the strips. */
static int check_adaptive_tail(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, float threshold, const void *out_rgb,
                               bool mask_ok)
{
    if (!(threshold >= 0.0f)) return fail(ctx, C2RT_ERR_INVALID_ARG, "threshold %g: neither negative nor NaN", (double)threshold);
    if (!out_rgb) return fail(ctx, C2RT_ERR_INVALID_ARG, "null output");
    if (!mask_ok) return fail(ctx, C2RT_ERR_INVALID_ARG, "null needs_aa: the device variant keeps the flags in the caller's buffer");
    if (cam) {
        if (cam->dof) return fail(ctx, C2RT_ERR_UNSUPPORTED, "depth of field: the flags compare one ray per pixel, a lens has many");
        if (cam->stereo_separation != 0) return fail(ctx, C2RT_ERR_UNSUPPORTED, "stereo: the flags compare one ray per pixel, a stereo camera has two");
        if (opts->count_rays) return fail(ctx, C2RT_ERR_UNSUPPORTED, "count_rays: the refinement does not count rays");
        if (opts->prepass_bucket) return fail(ctx, C2RT_ERR_UNSUPPORTED, "prepass_bucket: a preview's pixels share the sample of their block");
    }
    if (opts->strip_world > 1) return fail(ctx, C2RT_ERR_UNSUPPORTED, "strip_world > 1: the rows above and below a strip belong to other ranks");
    if (cam && !ctx->peers.empty()) return fail(ctx, C2RT_ERR_UNSUPPORTED, "multi-device context: the rows above and below a strip are on other devices");
    return C2RT_OK;
}

/* the refusals of both entry points, in the documented order: a frame call's, then the arguments of this call, then the
 * modes in which a pixel is not five rays of its own or its neighbours are not in this frame */
static int check_adaptive_args(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, float threshold,
                               const void *out_rgb, bool mask_ok)
{
    if (const int st = check_frame_args(ctx, cam, opts)) return st;
    if (opts->taps != C2RT_TAPS_REF5) return fail(ctx, C2RT_ERR_INVALID_ARG, "adaptive anti-aliasing refines to C2RT_TAPS_REF5: taps is %u", (unsigned)opts->taps);
    return check_adaptive_tail(ctx, cam, opts, threshold, out_rgb, mask_ok);
}

/* The three steps on `stream`, device pointers: the one-tap frame through the frame path as it is (pre-pass, lean / exact
 * redo, nested-CSG retry, the stream's scratch slot), the flags, the refinement of the flagged pixels in place.  The
 * caller's mask is the only buffer between detection and refinement: no scratch of this call's own.  `taps` null: the
 * reference's four extra taps (c2rt_adaptive.hip); otherwise taps 1 .. n-1 of the caller's table (c2rt_sample_taps.hip). */
static int adaptive_enqueue(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_tap_table *taps, float threshold,
                            float *out_dev, uint8_t *mask_dev, hipStream_t stream)
{
    c2rt_render_opts one = *opts;
    one.taps = C2RT_TAPS_1;
    if (const int st = render_device(ctx, cam, &one, out_dev, stream)) return st;
    int e = launch_aa_detect(out_dev, mask_dev, opts->width, opts->height, 1, threshold, stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "adaptive AA detection kernel launch: %s", hipGetErrorString((hipError_t)e));
    RenderParams p;
    hit_params(ctx, cam, &one, p);
    e = taps ? launch_aa_refine_taps(p, ctx->plan.csg_levels, *taps, out_dev, mask_dev, stream) : launch_aa_refine(p, ctx->plan.csg_levels, out_dev, mask_dev, stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "adaptive AA refinement kernel launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

int c2rt_render_frame_adaptive_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, float threshold,
                                      float *out_rgb_dev, uint8_t *needs_aa_dev, void *hip_stream)
{
    if (const int st = check_adaptive_args(ctx, cam, opts, threshold, out_rgb_dev, needs_aa_dev != nullptr)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return adaptive_enqueue(ctx, cam, opts, nullptr, threshold, out_rgb_dev, needs_aa_dev, static_cast<hipStream_t>(hip_stream));
}

/* The tail of every adaptive host variant: the px pixels of the frame(s) at the head of the staging allocation and, where
 * asked for, their flags at mask_dev back to the caller, one copy per output, then a stream sync */
static int adaptive_copy_back(c2rt_ctx *ctx, size_t px, const uint8_t *mask_dev, float *out_rgb, uint8_t *needs_aa)
{
    HIP_TRY(ctx, hipMemcpyAsync(out_rgb, ctx->frame, px * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (needs_aa) HIP_TRY(ctx, hipMemcpyAsync(needs_aa, mask_dev, px, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return C2RT_OK;
}

/* Both host variants, the arguments checked: frame and mask side by side in the context's staging allocation, on the
 * context's stream; one copy back per output, then a stream sync. */
static int adaptive_to_host(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_tap_table *taps, float threshold,
                            float *out_rgb, uint8_t *needs_aa, const volatile uint8_t *stop_flag)
{
    /* isStopReq() before the pass — rt/renderer.d:129 */
    if (stop_flag && *stop_flag) return fail(ctx, C2RT_ERR_CANCELLED, "stop requested before the frame");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)opts->width * opts->height;
    const size_t off_mask = align256(px * 3 * sizeof(float));
    if (const int st = ensure_staging(ctx, off_mask + px)) return st;
    uint8_t *mask_dev = reinterpret_cast<uint8_t *>(ctx->frame) + off_mask;
    if (const int st = adaptive_enqueue(ctx, cam, opts, taps, threshold, ctx->frame, mask_dev, ctx->stream)) return st;
    return adaptive_copy_back(ctx, px, mask_dev, out_rgb, needs_aa);
}

int c2rt_render_frame_adaptive(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, float threshold,
                               float *out_rgb, uint8_t *needs_aa, const volatile uint8_t *stop_flag)
{
    if (const int st = check_adaptive_args(ctx, cam, opts, threshold, out_rgb, true)) return st;
    return adaptive_to_host(ctx, cam, opts, nullptr, threshold, out_rgb, needs_aa, stop_flag);
}

/* ---- sample tables: N-tap frames, whole and adaptive (c2rt_sample_taps.hip) ---------------------------------------- */

/* the table's own refusals, behind the frame call's, in the documented order */
static int check_tap_table(c2rt_ctx *ctx, const c2rt_tap_table *taps)
{
    if (!taps) return fail(ctx, C2RT_ERR_INVALID_ARG, "null taps");
    if (taps->n == 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "taps: n is 0 (1 .. %u)", (unsigned)C2RT_MAX_SAMPLE_TAPS);
    if (taps->n > C2RT_MAX_SAMPLE_TAPS) return fail(ctx, C2RT_ERR_LIMIT, "taps: n is %u (at most %u)", (unsigned)taps->n, (unsigned)C2RT_MAX_SAMPLE_TAPS);
    if (taps->reserved != 0) return fail(ctx, C2RT_ERR_INVALID_ARG, "taps: reserved is %u, not 0", (unsigned)taps->reserved);
    for (uint32_t s = 0; s < taps->n; ++s)
        if (!std::isfinite(taps->offset[s][0]) || !std::isfinite(taps->offset[s][1]))
            return fail(ctx, C2RT_ERR_INVALID_ARG, "taps: the offset of tap %u is not finite", (unsigned)s);
    return C2RT_OK;
}

/* the refusals of both whole-frame entry points, in the documented order */
static int check_frame_taps_args(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_tap_table *taps,
                                 const void *out_rgb)
{
    if (const int st = check_frame_args(ctx, cam, opts)) return st;
    if (const int st = check_tap_table(ctx, taps)) return st;
    if (!out_rgb) return fail(ctx, C2RT_ERR_INVALID_ARG, "null output");
    if (cam->dof) return fail(ctx, C2RT_ERR_UNSUPPORTED, "depth of field: a tap is one ray, a lens has many per tap");
    if (cam->stereo_separation != 0) return fail(ctx, C2RT_ERR_UNSUPPORTED, "stereo: a tap is one ray, a stereo camera has two per tap");
    if (opts->count_rays) return fail(ctx, C2RT_ERR_UNSUPPORTED, "count_rays: the sample-table frames do not count rays");
    if (opts->prepass_bucket) return fail(ctx, C2RT_ERR_UNSUPPORTED, "prepass_bucket: a preview's pixels share the sample of their block");
    return C2RT_OK;
}

int c2rt_render_frame_taps_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_tap_table *taps,
                                  float *out_rgb_dev, void *hip_stream)
{
    if (const int st = check_frame_taps_args(ctx, cam, opts, taps, out_rgb_dev)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    hit_params(ctx, cam, opts, p);
    if (p.local_rows == 0) return C2RT_OK;
    const int e = launch_frame_taps(p, ctx->plan.csg_levels, *taps, out_rgb_dev, 0, p.local_rows, hip_stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "sample-table frame kernel launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

/* Host variant: c2rt_render_hits' chunks of whole rows, 12 B per pixel — 3 MiB at most. */
int c2rt_render_frame_taps(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_tap_table *taps, float *out_rgb)
{
    if (const int st = check_frame_taps_args(ctx, cam, opts, taps, out_rgb)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    hit_params(ctx, cam, opts, p);
    if (p.local_rows == 0) return C2RT_OK;
    Staging outs;
    outs.add(out_rgb, 3 * sizeof(float));
    return row_chunks(ctx, p, 1, outs, "sample-table frame", [&](uint32_t r0, uint32_t m, size_t) {
        return launch_frame_taps(p, ctx->plan.csg_levels, *taps, outs.dev<float>(0), r0, m, ctx->stream);
    });
}

/* the refusals of both adaptive entry points, in the documented order: a frame call's, then the table's and the other
 * arguments of this call, then c2rt_render_frame_adaptive's unsupported modes in its wording */
static int check_adaptive_taps_args(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_tap_table *taps,
                                    float threshold, const void *out_rgb, bool mask_ok)
{
    if (const int st = check_frame_args(ctx, cam, opts)) return st;
    if (const int st = check_tap_table(ctx, taps)) return st;
    if (taps->n < 2) return fail(ctx, C2RT_ERR_INVALID_ARG, "taps: n is %u, adaptive refinement needs at least 2", (unsigned)taps->n);
    if (taps->offset[0][0] != 0.0 || taps->offset[0][1] != 0.0)
        return fail(ctx, C2RT_ERR_INVALID_ARG, "taps: tap 0 is (%g, %g), the one-tap frame samples (0, 0)", taps->offset[0][0], taps->offset[0][1]);
    return check_adaptive_tail(ctx, cam, opts, threshold, out_rgb, mask_ok);
}

int c2rt_render_frame_adaptive_taps_device(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_tap_table *taps,
                                           float threshold, float *out_rgb_dev, uint8_t *needs_aa_dev, void *hip_stream)
{
    if (const int st = check_adaptive_taps_args(ctx, cam, opts, taps, threshold, out_rgb_dev, needs_aa_dev != nullptr)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return adaptive_enqueue(ctx, cam, opts, taps, threshold, out_rgb_dev, needs_aa_dev, static_cast<hipStream_t>(hip_stream));
}

int c2rt_render_frame_adaptive_taps(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, const c2rt_tap_table *taps,
                                    float threshold, float *out_rgb, uint8_t *needs_aa, const volatile uint8_t *stop_flag)
{
    if (const int st = check_adaptive_taps_args(ctx, cam, opts, taps, threshold, out_rgb, true)) return st;
    return adaptive_to_host(ctx, cam, opts, taps, threshold, out_rgb, needs_aa, stop_flag);
}

/* The refusals of the four batch entry points, in the documented order: a batch call's, then the arguments of this
 * call, then strips; for the posed calls (poses_given), then the poses'.  Depth of field, stereo, count_rays,
 * prepass_bucket and a multi-device context are among the batch call's. */
static int check_adaptive_batch_args(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, bool poses_given,
                                     uint32_t n_frames, const c2rt_render_opts *opts, float threshold, const void *out_rgb, bool mask_ok)
{
    if (const int st = check_batch_args(ctx, cams, n_frames, opts)) return st;
    if (opts->taps != C2RT_TAPS_REF5) return fail(ctx, C2RT_ERR_INVALID_ARG, "adaptive anti-aliasing refines to C2RT_TAPS_REF5: taps is %u", (unsigned)opts->taps);
    if (const int st = check_adaptive_tail(ctx, nullptr, opts, threshold, out_rgb, mask_ok)) return st;
    if (poses_given)
        if (const int st = check_posed_args(ctx, poses, n_frames)) return st;
    return C2RT_OK;
}

/* Both device variants; poses_given: the posed one.  The arguments have passed check_adaptive_batch_args. */
static int adaptive_batch_enqueue(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, bool poses_given,
                                  uint32_t n_frames, const c2rt_render_opts *opts, float threshold, float *out_dev, uint8_t *mask_dev,
                                  hipStream_t stream)
{
    std::vector<std::unique_ptr<PosedFrame>> posed;
    if (poses_given)
        if (const int st = plan_posed_frames(ctx, poses, n_frames, posed)) return st;
    c2rt_render_opts one = *opts;
    one.taps = C2RT_TAPS_1;
    const AdaptiveBatch adaptive = {threshold, mask_dev};
    ctx->counters_valid = false;
    return render_frames_device(ctx, cams, poses_given ? &posed : nullptr, n_frames, &one, out_dev, stream, &adaptive);
}

/* Both host variants: frames and masks side by side in the context's staging allocation, on the context's stream; one
 * copy back per output, then a stream sync. */
static int adaptive_batch_to_host(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, bool poses_given,
                                  uint32_t n_frames, const c2rt_render_opts *opts, float threshold, float *out_rgb, uint8_t *needs_aa,
                                  const volatile uint8_t *stop_flag)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (n_frames == 0) return C2RT_OK;
    if (const int st = check_adaptive_batch_args(ctx, cams, poses, poses_given, n_frames, opts, threshold, out_rgb, true)) return st;
    if (stop_flag && *stop_flag) return fail(ctx, C2RT_ERR_CANCELLED, "stop requested before the batch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)n_frames * opts->width * opts->height;
    const size_t off_mask = align256(px * 3 * sizeof(float));
    if (const int st = ensure_staging(ctx, off_mask + px)) return st;
    uint8_t *mask_dev = reinterpret_cast<uint8_t *>(ctx->frame) + off_mask;
    if (const int st = adaptive_batch_enqueue(ctx, cams, poses, poses_given, n_frames, opts, threshold, ctx->frame, mask_dev, ctx->stream)) return st;
    return adaptive_copy_back(ctx, px, mask_dev, out_rgb, needs_aa);
}

static int adaptive_batch_to_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, bool poses_given,
                                    uint32_t n_frames, const c2rt_render_opts *opts, float threshold, float *out_rgb_dev,
                                    uint8_t *needs_aa_dev, void *hip_stream)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (n_frames == 0) return C2RT_OK;
    if (const int st = check_adaptive_batch_args(ctx, cams, poses, poses_given, n_frames, opts, threshold, out_rgb_dev, needs_aa_dev != nullptr)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return adaptive_batch_enqueue(ctx, cams, poses, poses_given, n_frames, opts, threshold, out_rgb_dev, needs_aa_dev, static_cast<hipStream_t>(hip_stream));
}

int c2rt_render_frames_adaptive_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts,
                                       float threshold, float *out_rgb_dev, uint8_t *needs_aa_dev, void *hip_stream)
{
    return adaptive_batch_to_device(ctx, cams, nullptr, false, n_frames, opts, threshold, out_rgb_dev, needs_aa_dev, hip_stream);
}

int c2rt_render_frames_adaptive(c2rt_ctx *ctx, const c2rt_camera_frame *cams, uint32_t n_frames, const c2rt_render_opts *opts,
                                float threshold, float *out_rgb, uint8_t *needs_aa, const volatile uint8_t *stop_flag)
{
    return adaptive_batch_to_host(ctx, cams, nullptr, false, n_frames, opts, threshold, out_rgb, needs_aa, stop_flag);
}

int c2rt_render_frames_posed_adaptive_device(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, uint32_t n_frames,
                                             const c2rt_render_opts *opts, float threshold, float *out_rgb_dev, uint8_t *needs_aa_dev,
                                             void *hip_stream)
{
    return adaptive_batch_to_device(ctx, cams, poses, true, n_frames, opts, threshold, out_rgb_dev, needs_aa_dev, hip_stream);
}

int c2rt_render_frames_posed_adaptive(c2rt_ctx *ctx, const c2rt_camera_frame *cams, const c2rt_scene_pose *poses, uint32_t n_frames,
                                      const c2rt_render_opts *opts, float threshold, float *out_rgb, uint8_t *needs_aa,
                                      const volatile uint8_t *stop_flag)
{
    return adaptive_batch_to_host(ctx, cams, poses, true, n_frames, opts, threshold, out_rgb, needs_aa, stop_flag);
}

static int deinterleave_words(c2rt_ctx *ctx, const float *gathered_dev, float *frame_dev, uint32_t width, uint32_t height,
                              uint32_t strip_height, uint32_t world, uint32_t words_per_pixel, void *hip_stream)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (!gathered_dev || !frame_dev || width == 0 || height == 0 || world == 0)
        return fail(ctx, C2RT_ERR_INVALID_ARG, "bad de-interleave arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    c2rt_render_opts o;
    std::memset(&o, 0, sizeof o);
    o.width = width;
    o.height = height;
    o.strip_height = strip_height;
    o.strip_world = world;
    const uint32_t sh = strip_h(&o);
    const uint32_t rows_pad = world > 1 ? local_rows_of(&o, 0) : height; /* rank 0 always owns the most rows */
    const int e = launch_deinterleave(gathered_dev, frame_dev, width, height, sh, world, rows_pad, words_per_pixel, hip_stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "de-interleave launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

int c2rt_deinterleave_strips(c2rt_ctx *ctx, const float *gathered_dev, float *frame_dev, uint32_t width,
                             uint32_t height, uint32_t strip_height, uint32_t world, void *hip_stream)
{
    return deinterleave_words(ctx, gathered_dev, frame_dev, width, height, strip_height, world, 3, hip_stream);
}

int c2rt_deinterleave_strips_rgb32(c2rt_ctx *ctx, const uint32_t *gathered_dev, uint32_t *frame_dev, uint32_t width,
                                   uint32_t height, uint32_t strip_height, uint32_t world, void *hip_stream)
{
    return deinterleave_words(ctx, reinterpret_cast<const float *>(gathered_dev), reinterpret_cast<float *>(frame_dev), width,
                              height, strip_height, world, 1, hip_stream);
}

int c2rt_render_frame_rgb32(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                            uint32_t *out_rgb32, const volatile uint8_t *stop_flag)
{
    int st = check_frame_args(ctx, cam, opts);
    if (st != C2RT_OK) return st;
    if (!out_rgb32) return fail(ctx, C2RT_ERR_INVALID_ARG, "null output");
    if (stop_flag && *stop_flag) return fail(ctx, C2RT_ERR_CANCELLED, "stop requested before the frame");
    if ((st = check_multi_opts(ctx, opts)) != C2RT_OK) return st;
    if (!ctx->peers.empty()) return render_to_host_multi(ctx, cam, opts, nullptr, out_rgb32, stop_flag);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return render_to_host(ctx, cam, opts, nullptr, out_rgb32, stop_flag);
}

int c2rt_encode_rgb32(c2rt_ctx *ctx, const float *frame_dev, uint32_t *out_dev, uint64_t n_pixels, void *hip_stream)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    if (!frame_dev || !out_dev) return fail(ctx, C2RT_ERR_INVALID_ARG, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_pixels == 0) return C2RT_OK;
    const int e = launch_encode_rgb32(frame_dev, out_dev, n_pixels, ctx->srgb_lut, hip_stream);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "encode launch: %s", hipGetErrorString((hipError_t)e));
    return C2RT_OK;
}

#if C2RT_DIAG
/* Diagnostics hook, in the diagnostics build only (the product library does not export it and include/c2rt.h does
 * not declare it): the mask pre-pass of one frame, exactly as c2rt_render_frame runs it on this context's stream
 * (fill_params, prepare_frame), except that every VoidNode::flags of the frame is ANDed with void_flags_mask
 * (0: no void test, 1: primary only, 3: as shipped).  Copies the FIRST table (4 words per entry, in the
 * tile_mask_slot layout, mask_entries entries) to `out` and reports
 *   info[0..5] = {tile columns (blocks_x * kWavesPerBlock), tile rows, mask_row0, mask_rows, tile rows per row class,
 *                 mask_entries}
 * and the VoidCull the pre-pass was given (`void_cull`, void_cull_bytes == sizeof(VoidCull)).  A frame without a
 * table (no culled node, depth of field, stereo) returns C2RT_ERR_UNSUPPORTED; `out` too small: C2RT_ERR_LIMIT.
 * tests/csg_void_device.py. */
int c2rt_debug_tile_masks(c2rt_ctx *ctx, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, uint32_t void_flags_mask,
                          uint32_t *out, size_t out_words, uint32_t info[6], void *void_cull, size_t void_cull_bytes)
{
    int st = check_frame_args(ctx, cam, opts);
    if (st != C2RT_OK) return st;
    if (!out || !info || !void_cull) return fail(ctx, C2RT_ERR_INVALID_ARG, "null output");
    if (void_cull_bytes != sizeof(VoidCull)) return fail(ctx, C2RT_ERR_INVALID_ARG, "VoidCull is %zu bytes, not %zu", sizeof(VoidCull), void_cull_bytes);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    frame_params(ctx, cam, opts, p);
    BatchCull cull;
    const int e = prepare_frame(ctx, p, ctx->stream, void_flags_mask, &cull);
    if (e != 0) return fail(ctx, C2RT_ERR_HIP, "tile-mask pre-pass launch: %s", hipGetErrorString((hipError_t)e));
    if (!p.tile_masks) return fail(ctx, C2RT_ERR_UNSUPPORTED, "this frame has no tile-mask table");
    const size_t words = (size_t)p.mask_entries * 4;
    if (out_words < words) return fail(ctx, C2RT_ERR_LIMIT, "the table has %zu words, the buffer %zu", words, out_words);
    HIP_TRY(ctx, hipMemcpyAsync(out, p.tile_masks, words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    info[0] = p.blocks_x * kWavesPerBlock;
    info[1] = (p.mask_rows + kTileH - 1) / kTileH;
    info[2] = p.mask_row0;
    info[3] = p.mask_rows;
    info[4] = (info[1] + 7u) / 8u;
    info[5] = p.mask_entries;
    std::memcpy(void_cull, &cull.v, sizeof cull.v);
    return C2RT_OK;
}

/* Diagnostics hook: the sphere test's switch.  Every SphereNode::flags of the frames and pre-passes this context
 * runs from now on is ANDed with `sphere_flags_mask` (0: no sphere test — the tables of the CsgDiff void test alone;
 * 1: primary only; 3: as shipped, the initial value unless C2RT_DEBUG_CULL has bit 3 set), independently of
 * c2rt_debug_tile_masks' void_flags_mask.  Writes the SphereCull a pre-pass of (cam, opts) is given under that mask
 * to `sphere_cull` (nullable; sphere_cull_bytes == sizeof(SphereCull)).  tests/sphere_cull_device.py. */
int c2rt_debug_sphere_cull(c2rt_ctx *ctx, uint32_t sphere_flags_mask, const c2rt_camera_frame *cam, const c2rt_render_opts *opts,
                           void *sphere_cull, size_t sphere_cull_bytes)
{
    if (!ctx) return C2RT_ERR_INVALID_ARG;
    ctx->sphere_flags_mask = sphere_flags_mask;
    if (!sphere_cull) return C2RT_OK;
    int st = check_frame_args(ctx, cam, opts);
    if (st != C2RT_OK) return st;
    if (sphere_cull_bytes != sizeof(SphereCull)) return fail(ctx, C2RT_ERR_INVALID_ARG, "SphereCull is %zu bytes, not %zu", sizeof(SphereCull), sphere_cull_bytes);
    RenderParams p;
    frame_params(ctx, cam, opts, p);
    size_t entries, blocks;
    frame_needs(p, entries, blocks);
    BatchCull cull;
    wire_frame(ctx, ctx->plan, p, FrameScratch(), 0, entries, blocks, ~0u, cull); /* (the mask is the context's, set above) */
    std::memcpy(sphere_cull, &cull.s, sizeof cull.s);
    return C2RT_OK;
}
#endif

} /* extern "C" */
