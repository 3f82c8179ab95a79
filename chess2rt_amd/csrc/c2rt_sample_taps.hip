/*
 * c2rt_sample_taps.hip — sample tables (c2rt_render_frame_taps*, c2rt_render_frame_adaptive_taps*): a frame whose
 * pixels are the average of the caller's n taps (1 .. C2RT_MAX_SAMPLE_TAPS) instead of one of the built-in patterns, and
 * the adaptive frame that spends taps 1 .. n-1 only on the pixels the edge test flags.  The hit-plane kernel's wave
 * (c2rt_hit_planes.hip) and the packed refinement's (c2rt_adaptive.hip) with the tap table as a kernel argument behind
 * the parameter block: 264 bytes of the argument segment, no copy, no scratch slot.  What it shares with the other
 * query kernels: c2rt_query.inc.
 *
 * frame_taps_kernel — one wave per 8x8 tile, one pixel per lane; a loop over the taps that is NOT unrolled, the colour
 * accumulated in registers with render_tile's statements (c2rt_trace.inc): accum = c_0, accum = accum + c_s in tap
 * order, accum / (float)n for n > 1 — hence the bits of the C2RT_TAPS_REF5 / _4 / _1 frames for their tables.  The tap
 * index is wave-uniform: the two offsets are scalar loads from the argument segment, read through a pointer the
 * optimiser cannot see through in every iteration (as render_tile reads its arguments), so that nothing of the table
 * lives in registers across the trace.
 *
 * aa_refine_taps_kernel — aa_refine_kernel with n - 1 taps per flagged pixel, in passes of at most kTapsPerPass = 8 taps:
 * a pass over taps 1 + t0 .. t0 + m of a tile with k flags has m k items (pixel i / m, tap 1 + t0 + i % m); lane l of
 * round r takes item 64 r + l.  Each item leaves its colour in an LDS array [pixel's lane][tap of the pass][3] behind the
 * hit stack (768 bytes per held tap: 6 KiB), and after the pass the pixel's own lane adds them, in tap order, to a running
 * sum that starts as out[y][x]; after the last pass it divides by (float)n.  An item's tap varies per lane, so the
 * offsets are copied once from the argument segment into LDS (256 bytes) and read from there.
 * Measured at 16 taps (scripts/sample_taps_rate.py --adaptive-only, the whole adaptive call, lecture5 1080p / 4K,
 * lecture4 1080p / 4K; profiles/sample_taps.md): all 15 taps in one pass (11.25 KiB) 258.6 / 440.7 / 180.8 / 423.1 us,
 * passes of 8: 260.5 / 425.3 / 173.3 / 397.9, passes of 4 (the reference refinement's array) 267.3 / 435.3 / 190.6 /
 * 442.9 — fewer samples held means more tiles in flight beside the 10 .. 40 KiB hit stack, shorter passes mean more
 * half-empty rounds; 8 is the best of the three on three shapes and within 1 % on the fourth.
 *
 * Detection is c2rt_adaptive.hip's aa_detect_kernel as it is: it does not depend on the table.
 */
#define C2RT_TRACE_EXACT_ONLY
#include "c2rt_trace_common.inc"
#include "c2rt_query.inc"

namespace c2rt {
namespace {

static_assert(sizeof(c2rt_tap_table) == 264 && __builtin_offsetof(c2rt_tap_table, offset) == 8 && alignof(c2rt_tap_table) == 8,
              "ABI layout of c2rt_tap_table");
/* the table follows the parameter block in the argument segment (both 8-aligned), then a pointer or two and 12 bytes */
static_assert(sizeof(RenderParams) % 8 == 0 && alignof(RenderParams) <= 8, "the tap table follows the parameter block");
static_assert(sizeof(RenderParams) + sizeof(c2rt_tap_table) + 32 <= 4096, "the kernel-argument segment holds at most 4 KiB");
static_assert(kTileW == kQueryTileW && kTileH == kQueryTileH && kTileW * kTileH == kWave, "one wavefront, one tile of the frames'");

typedef const c2rt_tap_table __attribute__((address_space(4))) *TapArgs;
/* the table of a kernel whose arguments begin (RenderParams, c2rt_tap_table, ...) */
DEV TapArgs tap_args(KArgs K) { return (TapArgs)(K + 1); }

template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_QUERY(LEVELS, MLC)
frame_taps_kernel(const RenderParams P, const c2rt_tap_table taps, float *__restrict__ out, const uint32_t row0, const uint32_t rows,
                  const uint32_t tiles_x)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    const KArgs K = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = (int)threadIdx.x;
    const TilePixel px = tile_pixel(P, lane, rows, tiles_x);
    Ctx cx;
    query_ctx(cx, P, K, lds, lane);
    if (px.live) {
        const double x = (double)px.x, y = (double)px.y(P, row0);
        const uint32_t n = taps.n;
        F3 accum = mkf(0, 0, 0);
#pragma unroll 1
        for (uint32_t s = 0; s < n; ++s) {
            KArgs Kt = K;
            asm volatile("" : "+s"(Kt));
            const TapArgs T = tap_args(Kt);
            const double dx = T->offset[s][0], dy = T->offset[s][1];
            D3 o, d;
            pixel_ray(cx, P, x + dx, y + dy, o, d);
            Hit best;
            Surf surf;
            Mat mat;
            const int closest = trace_closest<LEVELS>(cx, o, d, false, best, surf, mat);
            const F3 c = sample_colour<LEVELS, MLC>(P, cx, closest, mat, d, surf);
            accum = s == 0 ? c : accum + c;
        }
        if (n > 1) accum = accum / (float)n; /* Color / float */
        store_colour(out + px.idx * 3, accum);
    }
}

constexpr int kTapsPerPass = 8; /* taps 1 .. n-1 of a flagged pixel go in passes of at most this many (measured: above) */
constexpr size_t kTapOffsetBytes = sizeof(double) * 2 * C2RT_MAX_SAMPLE_TAPS, kTapListBytes = kWave;
/* the samples of a tile's pass: [pixel's lane][tap of the pass][3] floats */
inline size_t tap_colour_bytes(uint32_t n) { return (size_t)kWave * (n - 1 < (uint32_t)kTapsPerPass ? n - 1 : (uint32_t)kTapsPerPass) * 3 * sizeof(float); }

template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_QUERY(LEVELS, MLC)
aa_refine_taps_kernel(const RenderParams P, const c2rt_tap_table taps, float *__restrict__ frame, const uint8_t *__restrict__ needs_aa,
                      const uint32_t tiles_x)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    const KArgs K = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = (int)threadIdx.x;
    const uint32_t x0 = (blockIdx.x % tiles_x) * kTileW, y0 = (blockIdx.x / tiles_x) * kTileH; /* the grid is tiles_x * tiles_y */
    const uint32_t x = x0 + (uint32_t)(lane % kTileW), y = y0 + (uint32_t)(lane / kTileW);
    const size_t idx = (size_t)y * P.width + x;
    const bool flagged = x < P.width && y < P.height && needs_aa[idx] != 0;
    const unsigned long long flags = __ballot(flagged);
    if (!flags) return;
    const int extra = (int)taps.n - 1; /* taps per flagged pixel: 1 .. C2RT_MAX_SAMPLE_TAPS - 1 */
    const int held = extra < kTapsPerPass ? extra : kTapsPerPass; /* samples the LDS array holds per pixel */
    const size_t stack = (size_t)P.csg_cap * kCsgLdsPerEntry;
    double *offs = reinterpret_cast<double *>(lds + stack);                        /* [tap][2], read per lane below */
    float *colour = reinterpret_cast<float *>(lds + stack + kTapOffsetBytes);      /* [pixel's lane][tap of the pass][3] */
    uint8_t *list = reinterpret_cast<uint8_t *>(colour + kWave * held * 3);        /* the flagged lanes, ascending */
    Ctx cx;
    query_ctx(cx, P, K, lds, lane);
    if (lane < 2 * (extra + 1)) offs[lane] = tap_args(K)->offset[lane >> 1][lane & 1];
    if (flagged) list[__popcll(flags & ((1ull << lane) - 1ull))] = (uint8_t)lane;
    __builtin_amdgcn_wave_barrier(); /* LDS operations of one wave complete in order; the workgroup is this wave */
    float *out = frame + idx * 3;
    F3 accum = mkf(0, 0, 0);
#pragma unroll 1
    for (int t0 = 0; t0 < extra; t0 += held) { /* a pass: taps 1 + t0 .. t0 + m of every flagged pixel */
        const int m = extra - t0 < held ? extra - t0 : held;
        const int items = m * __popcll(flags);
#pragma unroll 1
        for (int first = 0; first < items; first += kWave) {
            const int i = first + lane;
            if (i < items) {
                const int j = i / m, t = i - j * m; /* tap 1 + t0 + t of the j-th flagged pixel */
                const int pl = (int)list[j];
                const uint32_t px = x0 + (uint32_t)(pl % kTileW), py = y0 + (uint32_t)(pl / kTileW);
                const double dx = offs[2 * (t0 + t + 1)], dy = offs[2 * (t0 + t + 1) + 1];
                D3 o, d;
                pixel_ray(cx, P, (double)px + dx, (double)py + dy, o, d);
                Hit best;
                Surf surf;
                Mat mat;
                const int closest = trace_closest<LEVELS>(cx, o, d, false, best, surf, mat);
                const F3 c = sample_colour<LEVELS, MLC>(P, cx, closest, mat, d, surf);
                float *slot = colour + (pl * held + t) * 3;
                slot[0] = c.r;
                slot[1] = c.g;
                slot[2] = c.b;
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (flagged) {
            /* accum = the pixel's one-tap colour, += the samples in tap order */
            if (t0 == 0) {
                const f3_t v0 = *reinterpret_cast<const f3_t *>(out);
                accum = mkf(v0.x, v0.y, v0.z);
            }
#pragma unroll 1
            for (int t = 0; t < m; ++t) {
                const float *slot = colour + (lane * held + t) * 3;
                accum = accum + mkf(slot[0], slot[1], slot[2]);
            }
        }
        __builtin_amdgcn_wave_barrier(); /* the next pass overwrites the array */
    }
    if (flagged) store_colour(out, accum / (float)(extra + 1)); /* / n — Color / float */
}

bool table_ok(const c2rt_tap_table &taps, uint32_t least) { return taps.n >= least && taps.n <= C2RT_MAX_SAMPLE_TAPS; }

} // namespace

/* Rows [row0, row0 + rows) of the local rows of the frame `p` describes (hit_params' settings), every pixel the average
 * of the table's taps, into `out` whose first row is row0; 1 <= taps.n <= C2RT_MAX_SAMPLE_TAPS, rows > 0. */
int launch_frame_taps(const RenderParams &p, int csg_levels, const c2rt_tap_table &taps, float *out, uint32_t row0, uint32_t rows, void *stream)
{
    if (!rows || !p.width || !out || !table_ok(taps, 1)) return (int)hipErrorInvalidValue;
    uint32_t tiles_x;
    const dim3 grid = tile_grid(p, rows, tiles_x);
    return for_csg_levels(csg_levels, [&](auto L) {
        constexpr int LEVELS = decltype(L)::value;
        return launch_query(p, frame_taps_kernel<LEVELS, true>, frame_taps_kernel<LEVELS, false>, grid, stack_lds(p), static_cast<hipStream_t>(stream), p, taps,
                            out, row0, rows, tiles_x);
    });
}

/* The flagged pixels of the whole frame `p` describes (hit_params' settings; no strips) from their one-tap value to the
 * average of the table's taps, in place; 2 <= taps.n <= C2RT_MAX_SAMPLE_TAPS, taps.offset[0] is not read. */
int launch_aa_refine_taps(const RenderParams &p, int csg_levels, const c2rt_tap_table &taps, float *frame, const uint8_t *needs_aa, void *stream)
{
    if (!p.width || !p.height || !frame || !needs_aa || !table_ok(taps, 2)) return (int)hipErrorInvalidValue;
    uint32_t tiles_x;
    const dim3 grid = tile_grid(p, p.height, tiles_x);
    const size_t lds = stack_lds(p) + kTapOffsetBytes + tap_colour_bytes(taps.n) + kTapListBytes;
    return for_csg_levels(csg_levels, [&](auto L) {
        constexpr int LEVELS = decltype(L)::value;
        return launch_query(p, aa_refine_taps_kernel<LEVELS, true>, aa_refine_taps_kernel<LEVELS, false>, grid, lds, static_cast<hipStream_t>(stream), p, taps,
                            frame, needs_aa, tiles_x);
    });
}

} // namespace c2rt
