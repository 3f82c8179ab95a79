/*
 * c2rt_adaptive.hip — adaptive anti-aliasing (c2rt_render_frame_adaptive*): Renderer.renderRT's three passes with the third one run where
 * the second raised its flag, which is what rt/renderer.d:150-188 computes the flag for and then does not do.  The
 * one-tap frame is the frame kernels' (c2rt_api.cpp calls the frame path with taps = 1); this file holds the two
 * kernels behind it on the same stream.
 *
 * aa_detect_kernel — rt/renderer.d:154-177 with tooDifferent (rt/color.d:18-23): one lane per pixel over 8x8 tiles,
 * fifteen floats in (the pixel and its four neighbours, clamped at the frame's edges as the reference clamps them), one
 * byte out.  fp32 in the reference's order, no fma (the build has contraction off).  Memory-bound: 12 B read and 1 B
 * written per pixel from HBM, the neighbours come out of the caches.
 *
 * aa_refine_kernel — renderPixelAA (rt/renderer.d:233-251) for the flagged pixels: the hit-plane kernel's wave (one
 * wavefront per workgroup, one 8x8 tile, exact:: arithmetic, every culling mask all ones, full-capacity hit stack, no
 * ground shortcut) with the work items of the tile PACKED into lanes.  A tile with k flagged pixels has 4k items
 * (pixel j, tap 1 + i % 4); lane l of round r takes item 64 r + l, so a tile with up to 16 flagged pixels — an edge
 * crossing it — is ONE round of the trace at 4k / 64 occupancy instead of four rounds at k / 64.  The list of flagged
 * lanes is built in LDS from the ballot's prefix count; each item leaves its colour in an LDS array [pixel][tap] (3 KiB,
 * behind the hit stack), and the pixel's own lane then adds the four to out[y][x] in tap order and divides by 5.0f:
 * render_tile's statements (c2rt_trace.inc), hence the bits of the C2RT_TAPS_REF5 frame.  Lanes without an item are
 * masked out by control flow before the trace, as the query kernel masks its tail.  All plain vector stores.
 *
 * Detection is a launch of its own: it reads the neighbours' ONE-TAP values, and refinement overwrites pixels in
 * place; the caller's mask is the buffer between the two.  Refinement reads and writes its own pixel and the mask only.
 *
 * Batches (c2rt_render_frames_adaptive*): detection takes a frame stride and blockIdx.y = frame (stride 0 and one row of
 * blocks in the single-frame call); aa_refine_batch_kernel is the same wave over a TABLE of parameter blocks in HBM, one
 * per frame, read through a constant-address-space pointer as render_kernel_batch reads its own (c2rt_kernels.hip):
 * scalar loads, no VGPR.  A frame's block names the frame (RenderParams::out); its flags are the frame's slice of the
 * batch's mask.  The flagged tiles of every frame share one grid, so one tile's trace latency overlaps the others'.
 *
 * The plain variant — every flagged lane loops over its four taps, the others sit out — was measured against the packed
 * one and rejected (profiles/adaptive_aa.md; DESIGN.md, "Adaptive anti-aliasing"); it was a build switch up to commit
 * f0eed4f, c2rt_kernels.hip.
 */
#define C2RT_TRACE_EXACT_ONLY
#include "c2rt_trace_common.inc"
#include "c2rt_query.inc"

namespace c2rt {
namespace {

static_assert(kTileW * kTileH == kWave, "one wavefront, one tile");
constexpr int kAaDetectWaves = 4; /* tiles (wavefronts) per workgroup of the detection kernel */

__global__ void __launch_bounds__(kWave * kAaDetectWaves)
aa_detect_kernel(const float *__restrict__ frames, uint8_t *__restrict__ masks, const size_t frame_px, const uint32_t width,
                 const uint32_t height, const uint32_t tiles_x, const uint32_t n_tiles, const float threshold)
{
    /* blockIdx.y = frame; frame_px = pixels from one frame (and its flags) to the next, 0 in the single-frame call.  The
     * neighbours below are clamped at this frame's own edges */
    const float *__restrict__ frame = frames + (size_t)blockIdx.y * frame_px * 3;
    uint8_t *__restrict__ needs_aa = masks + (size_t)blockIdx.y * frame_px;
    const uint32_t tile = blockIdx.x * kAaDetectWaves + threadIdx.x / kWave;
    if (tile >= n_tiles) return;
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t x = (tile % tiles_x) * kTileW + lane % kTileW, y = (tile / tiles_x) * kTileH + lane / kTileW;
    if (x >= width || y >= height) return;
    const uint32_t xs[5] = {x, x > 0 ? x - 1 : x, x + 1 < width ? x + 1 : x, x, x};
    const uint32_t ys[5] = {y, y, y, y > 0 ? y - 1 : y, y + 1 < height ? y + 1 : y};
    float n[5][3];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const float *q = frame + ((size_t)ys[i] * width + xs[i]) * 3;
        n[i][0] = q[0];
        n[i][1] = q[1];
        n[i][2] = q[2];
    }
    bool flag = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float average = 0.0f; /* Color average = Color(0, 0, 0); foreach: average += neighs[i] */
#pragma unroll
        for (int i = 0; i < 5; ++i) average = average + n[i][c];
        average = average / 5.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i) flag = flag | (fabsf(n[i][c] - average) > threshold); /* a NaN compares false */
    }
    needs_aa[(size_t)y * width + x] = flag ? (uint8_t)1 : (uint8_t)0;
}

constexpr size_t kAaColourBytes = (size_t)kWave * 4 * 3 * sizeof(float), kAaListBytes = kWave;

/* The packed wave over tile blockIdx.x of the frame `P` describes: one body for both entry points below, which only
 * produce (P, K, frame, needs_aa). */
template <int LEVELS, bool MLC>
DEV void aa_refine_body(const RenderParams &P, KArgs K, float *__restrict__ frame, const uint8_t *__restrict__ needs_aa,
                        const uint32_t tiles_x)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const uint32_t x0 = (blockIdx.x % tiles_x) * kTileW, y0 = (blockIdx.x / tiles_x) * kTileH; /* the grid is tiles_x * tiles_y */
    const uint32_t x = x0 + (uint32_t)(lane % kTileW), y = y0 + (uint32_t)(lane / kTileW);
    const size_t idx = (size_t)y * P.width + x;
    const bool flagged = x < P.width && y < P.height && needs_aa[idx] != 0;
    const unsigned long long flags = __ballot(flagged);
    if (!flags) return;
    const size_t stack = (size_t)P.csg_cap * kCsgLdsPerEntry;
    float *colour = reinterpret_cast<float *>(lds + stack); /* [pixel's lane][tap - 1][3] */
    Ctx cx;
    query_ctx(cx, P, K, lds, lane);
    uint8_t *list = reinterpret_cast<uint8_t *>(lds + stack + kAaColourBytes); /* the flagged lanes, ascending */
    if (flagged) list[__popcll(flags & ((1ull << lane) - 1ull))] = (uint8_t)lane;
    __builtin_amdgcn_wave_barrier(); /* LDS operations of one wave complete in order; the workgroup is this wave */
    const int items = 4 * __popcll(flags);
#pragma unroll 1
    for (int first = 0; first < items; first += kWave) {
        const int i = first + lane;
        if (i < items) {
            const int pl = (int)list[i >> 2], t = 1 + (i & 3);
            const uint32_t px = x0 + (uint32_t)(pl % kTileW), py = y0 + (uint32_t)(pl / kTileW);
            D3 o, d;
            pixel_ray(cx, P, (double)px + k_aa_x[t], (double)py + k_aa_y[t], o, d);
            Hit best;
            Surf surf;
            Mat mat;
            const int closest = trace_closest<LEVELS>(cx, o, d, false, best, surf, mat);
            const F3 c = sample_colour<LEVELS, MLC>(P, cx, closest, mat, d, surf);
            float *slot = colour + (pl * 4 + (t - 1)) * 3;
            slot[0] = c.r;
            slot[1] = c.g;
            slot[2] = c.b;
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (flagged) {
        /* renderPixelAA: accum = the pixel's one-tap colour, += the four samples in tap order, / 5 — Color / float */
        float *out = frame + idx * 3;
        const f3_t v0 = *reinterpret_cast<const f3_t *>(out);
        F3 accum = mkf(v0.x, v0.y, v0.z);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float *slot = colour + (lane * 4 + t) * 3;
            accum = accum + mkf(slot[0], slot[1], slot[2]);
        }
        accum = accum / 5.0f;
        store_colour(out, accum);
    }
}

template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_QUERY(LEVELS, MLC)
aa_refine_kernel(const RenderParams P, float *__restrict__ frame, const uint8_t *__restrict__ needs_aa, const uint32_t tiles_x)
{
    aa_refine_body<LEVELS, MLC>(P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), frame, needs_aa, tiles_x);
}

/* The same over a batch: blockIdx.y = frame, blockIdx.x = tile.  frame_px = the pixels of one frame. */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_QUERY(LEVELS, MLC)
aa_refine_batch_kernel(const RenderParams *table, const uint8_t *__restrict__ masks, const size_t frame_px, const uint32_t tiles_x)
{
    const KArgs K = batch_block(table);
    const RenderParams &P = *(const RenderParams *)K;
    aa_refine_body<LEVELS, MLC>(P, K, P.out, masks + (size_t)blockIdx.y * frame_px, tiles_x);
}

/* table_dev null: the single-frame kernel with `p` as its argument, into `frame`; otherwise the n_frames blocks at
 * table_dev, of which `p` is any one's host copy (the grid, the stack and the instance are the same for all of them) */
int launch_refine(const RenderParams &p, int csg_levels, const RenderParams *table_dev, uint32_t n_frames, float *frame, const uint8_t *needs_aa,
                  hipStream_t s)
{
    static_assert(kTileW == kQueryTileW && kTileH == kQueryTileH, "the refinement walks the frames' tiles");
    uint32_t tiles_x;
    const dim3 grid = tile_grid(p, p.height, tiles_x, n_frames);
    const size_t lds = stack_lds(p) + kAaColourBytes + kAaListBytes, frame_px = (size_t)p.width * p.height;
    return for_csg_levels(csg_levels, [&](auto L) {
        constexpr int LEVELS = decltype(L)::value;
        if (table_dev)
            return launch_query(p, aa_refine_batch_kernel<LEVELS, true>, aa_refine_batch_kernel<LEVELS, false>, grid, lds, s, table_dev, needs_aa, frame_px, tiles_x);
        return launch_query(p, aa_refine_kernel<LEVELS, true>, aa_refine_kernel<LEVELS, false>, grid, lds, s, p, frame, needs_aa, tiles_x);
    });
}

} // namespace

/* needs_aa[y][x] of the n_frames whole width x height frames side by side at `frames`, their flags side by side at
 * `needs_aa` (device pointers), in one launch. */
int launch_aa_detect(const float *frames, uint8_t *needs_aa, uint32_t width, uint32_t height, uint32_t n_frames, float threshold, void *stream)
{
    if (!width || !height || !n_frames || n_frames > C2RT_MAX_BATCH_FRAMES || !frames || !needs_aa) return (int)hipErrorInvalidValue;
    const uint32_t tiles_x = (width + kTileW - 1) / kTileW, n_tiles = tiles_x * ((height + kTileH - 1) / kTileH);
    const size_t frame_px = n_frames > 1 ? (size_t)width * height : 0;
    hipLaunchKernelGGL(aa_detect_kernel, dim3((n_tiles + kAaDetectWaves - 1) / kAaDetectWaves, n_frames), dim3(kWave * kAaDetectWaves), 0,
                       static_cast<hipStream_t>(stream), frames, needs_aa, frame_px, width, height, tiles_x, n_tiles, threshold);
    return (int)hipGetLastError();
}

/* The flagged pixels of the whole frame `p` describes (hit_params' settings: exact::, csg_cap = kCsgFullCap(csg_levels),
 * no culling, no ground node; no strips) from their one-tap to their five-tap value, in place. */
int launch_aa_refine(const RenderParams &p, int csg_levels, float *frame, const uint8_t *needs_aa, void *stream)
{
    if (!p.width || !p.height || !frame || !needs_aa) return (int)hipErrorInvalidValue;
    return launch_refine(p, csg_levels, nullptr, 1, frame, needs_aa, static_cast<hipStream_t>(stream));
}

/* The same for the n_frames frames of a batch in one launch: table_dev holds their blocks (p0: any one's host copy),
 * block i names frame i (RenderParams::out); needs_aa holds their flags side by side. */
int launch_aa_refine_batch(const RenderParams &p0, int csg_levels, const RenderParams *table_dev, uint32_t n_frames, const uint8_t *needs_aa,
                           void *stream)
{
    if (!p0.width || !p0.height || !table_dev || !n_frames || n_frames > C2RT_MAX_BATCH_FRAMES || !needs_aa) return (int)hipErrorInvalidValue;
    return launch_refine(p0, csg_levels, table_dev, n_frames, nullptr, needs_aa, static_cast<hipStream_t>(stream));
}

} // namespace c2rt
