/*
 * c2rt_paths_counted.hip — path planes with a path count per sample (c2rt_render_paths_counted*,
 * c2rt_trace_rays_paths_counted*): c2rt_paths.hip's flat loop with the number of paths read per lane from a plane of
 * bytes, c = min(counts[i], g->paths).  Path p of sample idx draws rng_key(seed, idx, j) with sample p whatever the count
 * is, so a sample given c >= 1 paths has the bits of the uniform call with paths = c (include/c2rt.h), and a sample given
 * 0 is the contract's "miss" line: its node, its primary colour, nothing drawn.
 *
 * counted_sample is path_sample of c2rt_paths.hip restated, statement for statement, with what is new behind `NP`: the
 * uniform kernels keep their code to the instruction (scripts/isa_equal.py), which sharing the function as one template
 * would have had to be shown for twenty instances.  The register budget is occ_paths()'s of that unit; the lane's count
 * is one more register across the loop (profiles/paths_counted.md has every instance's figures).
 *
 * Two launch orders, the same bits (no sample's value depends on where it ran):
 *   natural — the path call's lane mapping, one kernel, nothing else enqueued.  A wave runs as long as its heaviest lane.
 *   count   — a counting sort of the sample indices by c, heaviest class first, leaves a permutation in the caller's
 *             scratch (count_hist_kernel, count_scan_kernel, count_scatter_kernel: a histogram over the 65 classes in
 *             LDS, one global atomic per block and class, an exclusive scan, then the scatter by the rank the LDS atomic
 *             returned), and lane i of the path kernel takes sample order[i]; a camera call derives the pixel from the
 *             index.  The waves of one class run the same trip count; what is lost is the 8x8 tile's coherence.
 *             Class 0 rides at the tail of the same launch.  Measured: profiles/paths_counted.md.
 *
 * Stores: each lane its own values at its sample's own place, as c2rt_paths.hip; the sort's order[] and counters are plain
 * vector stores and vector atomics.
 */
#define C2RT_TRACE_EXACT_ONLY
#include "c2rt_trace_common.inc"
#include "c2rt_query.inc"
#include "c2rt_paths_counted.h"

namespace c2rt {
namespace {

/* c2rt_paths.hip's budget and its start state in LDS at depth 1 (the comment above occ_paths() there) */
template <int LEVELS, bool MLC>
constexpr int occ_paths() { return LEVELS >= 2 || (LEVELS == 1 && MLC) ? 2 : 3; }
template <int LEVELS> constexpr bool kStartInLds = LEVELS == 1;
constexpr size_t kStartLds = (size_t)kWave * 6 * sizeof(double);
#define C2RT_WAVES_PATHS(L, M) __attribute__((amdgpu_waves_per_eu(occ_paths<L, M>(), occ_paths<L, M>())))

/* what a call draws its paths with (wave-uniform: kernel arguments); `order` null: natural order */
struct CountedArgs {
    uint64_t seed;
    uint32_t cap, bounces;
    const uint8_t *counts;
    const uint32_t *order;
};

DEV F3 albedo_of(const RenderParams &P, const Mat &mat, const Surf &surf)
{
    return mat.tex_type >= 0 ? tex_color(P, mat, surf.u, surf.v) : mat.color;
}

DEV double *start_of(const RenderParams &P, char *lds, const int lane)
{
    return reinterpret_cast<double *>(lds + (size_t)P.csg_cap * kCsgLdsPerEntry) + lane;
}

/* path_sample (c2rt_paths.hip) with the lane's own number of paths: NP = min(counts[at], cap), 0 .. 64 */
template <int LEVELS, bool MLC>
DEV void counted_sample(const RenderParams &P, const Ctx &cx, const c2rt_path_planes &out, const CountedArgs &g, const size_t at, const uint64_t idx, D3 o,
                        D3 d, double *start)
{
    using namespace exact;
    /* wave-uniform: kernel arguments */
    const bool want_colour = out.indirect || out.bounce || out.radiance;
    const bool want_albedo = out.bounce || out.radiance;
    Hit best;
    Surf surf;
    Mat mat;
    const int closest = trace_closest<LEVELS>(cx, o, d, false, best, surf, mat);
    if (out.node) out.node[at] = closest;
    if (!(out.segments || want_colour)) return; /* `node` alone traces no path */
    const uint32_t given = g.counts[at];
    const uint32_t NP = given < g.cap ? given : g.cap; /* per lane */
    const uint32_t beff = g.bounces < P.max_trace_depth ? g.bounces : P.max_trace_depth;
    const bool hit = closest >= 0;
    const bool live = hit && NP != 0; /* a sample given no path is a miss to everything below */
    if (out.radiance) store_colour(out.radiance + at * 3, sample_colour<LEVELS, MLC>(P, cx, closest, mat, d, surf));
    uint32_t segments = 0;
    F3 sum = mkf(0, 0, 0), a0 = mkf(0, 0, 0);
    if (beff != 0 && __ballot(live) != 0) { /* a wave with no path to trace draws nothing */
        if (live) {
            const D3 N0 = dot(d, surf.n) < 0 ? surf.n : -surf.n; /* faceforward — rt/imported_types.d:69-73 */
            const D3 from0 = surf.p + N0 * 1e-6;
            if (want_albedo) a0 = albedo_of(P, mat, surf);
            D3 N = N0, from = from0;
            if constexpr (kStartInLds<LEVELS>) {
                start[0 * kWave] = from0.x, start[1 * kWave] = from0.y, start[2 * kWave] = from0.z;
                start[3 * kWave] = N0.x, start[4 * kWave] = N0.y, start[5 * kWave] = N0.z;
            }
            F3 T = mkf(0, 0, 0);
            uint32_t p = 0, j = 0; /* the cursor: path, depth */
            for (;;) {             /* at most NP * beff iterations: every one advances the cursor */
                const D3 res = hemisphere_sample(rng_key(g.seed, idx, j), p, N);
                if (want_colour) {
                    const float w = (float)(2.0 * dot(res, N));
                    T = j == 0 ? mkf(w, w, w) : T * w;
                }
                Hit sbest;
                Surf ssurf;
                Mat smat;
                const int c = trace_closest<LEVELS>(cx, from, res, false, sbest, ssurf, smat);
                if (want_colour) sum = sum + sample_colour<LEVELS, MLC>(P, cx, c, smat, res, ssurf) * T;
                if (c >= 0) ++segments;
                if (c >= 0 && j + 1 < beff) { /* on along the path */
                    if (want_colour) T = T * albedo_of(P, smat, ssurf);
                    N = dot(res, ssurf.n) < 0 ? ssurf.n : -ssurf.n;
                    from = ssurf.p + N * 1e-6;
                    ++j;
                } else { /* the path ends: the next one starts at the primary hit */
                    if (++p == NP) break;
                    j = 0;
                    if constexpr (kStartInLds<LEVELS>) {
                        from = mk(start[0 * kWave], start[1 * kWave], start[2 * kWave]);
                        N = mk(start[3 * kWave], start[4 * kWave], start[5 * kWave]);
                    } else {
                        N = N0;
                        from = from0;
                    }
                }
            }
        }
    }
    if (out.segments) out.segments[at] = segments;
    const F3 indirect = NP != 0 ? sum / (float)NP : sum; /* no path: sum is +0 */
    const F3 bounce = a0 * indirect;
    if (out.indirect) store_colour(out.indirect + at * 3, indirect);
    if (out.bounce) store_colour(out.bounce + at * 3, bounce);
    if (out.radiance && live && beff != 0) { /* elsewhere the colour stays as it is */
        float *rad = out.radiance + at * 3;
        store_colour(rad, mkf(rad[0], rad[1], rad[2]) + bounce);
    }
}

/* path_planes_kernel's pixel, or — in count order, the grid being ray_grid(rows * width) — the pixel whose place in the
 * launch's rows is order[i] */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_PATHS(LEVELS, MLC)
path_planes_counted_kernel(const RenderParams P, const c2rt_path_planes out, const CountedArgs g, const uint32_t row0, const uint32_t rows,
                           const uint32_t tiles_x)
{
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    TilePixel px;
    if (g.order) { /* wave-uniform: a kernel argument */
        const uint64_t n = (uint64_t)rows * P.width, i = (uint64_t)blockIdx.x * kWave + (uint64_t)lane;
        const uint32_t s = i < n ? g.order[i] : 0u;
        px.live = i < n && s < n; /* a permutation of 0 .. n - 1; nothing is stored beyond the planes whatever it holds */
        px.r = s / P.width;
        px.x = s - px.r * P.width;
        px.idx = s;
    } else {
        px = tile_pixel(P, lane, rows, tiles_x);
    }
    Ctx cx;
    query_ctx(cx, P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    if (px.live) {
        const uint32_t y = px.y(P, row0);
        D3 o, d;
        pixel_ray(cx, P, (double)px.x, (double)y, o, d);
        counted_sample<LEVELS, MLC>(P, cx, out, g, px.idx, (uint64_t)y * P.width + px.x, o, d, start_of(P, lds, lane));
    }
}

/* trace_rays_paths_kernel's ray, or ray order[i] */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_PATHS(LEVELS, MLC)
trace_rays_paths_counted_kernel(const RenderParams P, const c2rt_path_planes out, const CountedArgs g, const c2rt_ray *__restrict__ rays, const uint64_t n,
                                const uint64_t base)
{
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kWave + (uint64_t)lane; /* the grid is ceil(n / 64) */
    Ctx cx;
    query_ctx(cx, P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    if (i < n) {
        const uint64_t s = g.order ? (uint64_t)g.order[i] : i;
        if (s < n) {
            D3 o, d;
            load6(rays + s, o, d);
            counted_sample<LEVELS, MLC>(P, cx, out, g, (size_t)s, base + s, o, d, start_of(P, lds, lane));
        }
    }
}

static_assert(sizeof(RenderParams) + sizeof(c2rt_path_planes) + sizeof(CountedArgs) + 24 <= 4096, "the kernel-argument segment holds at most 4 KiB");

/* ---- count order: the permutation ---- */

constexpr int kClasses = C2RT_MAX_PATHS + 1;        /* c = 0 .. 64 */
constexpr int kSortLanes = 256, kSortPerLane = 4;   /* a block sorts 1024 consecutive samples */
constexpr uint32_t kSortBlock = kSortLanes * kSortPerLane;
static_assert(kClasses <= kSortLanes && kClasses * sizeof(uint32_t) <= kCountedHeadBytes, "a lane and a counter per class");

DEV uint32_t class_of(const uint8_t *counts, const uint64_t i, const uint32_t cap)
{
    const uint32_t given = counts[i];
    return given < cap ? given : cap;
}

/* head[c] += the samples of class c (head zeroed by the launch) */
__global__ void __launch_bounds__(kSortLanes)
count_hist_kernel(const uint8_t *__restrict__ counts, const uint64_t n, const uint32_t cap, uint32_t *__restrict__ head)
{
    __shared__ uint32_t h[kClasses];
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t)kClasses) h[t] = 0;
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x * kSortBlock + t;
#pragma unroll
    for (int k = 0; k < kSortPerLane; ++k) {
        const uint64_t i = first + (uint64_t)k * kSortLanes;
        if (i < n) atomicAdd(&h[class_of(counts, i, cap)], 1u);
    }
    __syncthreads();
    if (t < (uint32_t)kClasses && h[t] != 0) atomicAdd(&head[t], h[t]);
}

/* head[c] = where class c starts, heaviest class first: 65 additions, one lane */
__global__ void __launch_bounds__(kWave)
count_scan_kernel(uint32_t *__restrict__ head)
{
    if (threadIdx.x != 0) return;
    uint32_t run = 0;
    for (int c = kClasses - 1; c >= 0; --c) {
        const uint32_t v = head[c];
        head[c] = run;
        run += v;
    }
}

/* order[start of the sample's class + its rank there] = the sample; the rank inside a class is the atomics' */
__global__ void __launch_bounds__(kSortLanes)
count_scatter_kernel(const uint8_t *__restrict__ counts, const uint64_t n, const uint32_t cap, uint32_t *__restrict__ head, uint32_t *__restrict__ order)
{
    __shared__ uint32_t h[kClasses];
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t)kClasses) h[t] = 0;
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x * kSortBlock + t;
    uint32_t cls[kSortPerLane], rank[kSortPerLane];
#pragma unroll
    for (int k = 0; k < kSortPerLane; ++k) {
        const uint64_t i = first + (uint64_t)k * kSortLanes;
        cls[k] = 0;
        rank[k] = 0;
        if (i < n) {
            cls[k] = class_of(counts, i, cap);
            rank[k] = atomicAdd(&h[cls[k]], 1u);
        }
    }
    __syncthreads();
    if (t < (uint32_t)kClasses && h[t] != 0) h[t] = atomicAdd(&head[t], h[t]); /* the block's run of the class */
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSortPerLane; ++k) {
        const uint64_t i = first + (uint64_t)k * kSortLanes;
        if (i < n) {
            const uint64_t at = (uint64_t)h[cls[k]] + rank[k];
            if (at < n) order[at] = (uint32_t)i; /* always, unless the plane changed between the two passes */
        }
    }
}

/* The permutation of the n samples of `counts` into `scratch` ([head | order[n]]); null where the launch runs in natural
 * order: no scratch, or more samples than an index of 32 bits names */
int enqueue_order(const uint8_t *counts, uint64_t n, uint32_t cap, void *scratch, hipStream_t s, const uint32_t *&order)
{
    order = nullptr;
    if (!scratch || n > 0xffffffffull) return 0;
    uint32_t *head = static_cast<uint32_t *>(scratch), *ord = reinterpret_cast<uint32_t *>(static_cast<char *>(scratch) + kCountedHeadBytes);
    if (const hipError_t e = hipMemsetAsync(head, 0, kCountedHeadBytes, s)) return (int)e;
    const dim3 grid((uint32_t)((n + kSortBlock - 1) / kSortBlock));
    hipLaunchKernelGGL(count_hist_kernel, grid, dim3(kSortLanes), 0, s, counts, n, cap, head);
    hipLaunchKernelGGL(count_scan_kernel, dim3(1), dim3(kWave), 0, s, head);
    hipLaunchKernelGGL(count_scatter_kernel, grid, dim3(kSortLanes), 0, s, counts, n, cap, head, ord);
    order = ord;
    return (int)hipGetLastError();
}

inline bool counted_args(const c2rt_path_opts &g, const uint8_t *counts, CountedArgs &a)
{
    a.seed = g.seed;
    a.cap = g.paths;
    a.bounces = g.bounces;
    a.counts = counts;
    a.order = nullptr;
    return counts && g.paths >= 1 && g.paths <= C2RT_MAX_PATHS && g.bounces >= 1 && g.bounces <= C2RT_MAX_PATH_BOUNCES;
}

} // namespace

/* launch_plane_rows of the path planes with counts[rows][width] beside the planes; scratch: null (natural order) or
 * counted_scratch_bytes(rows * width) bytes, 16-byte aligned (count order) */
int launch_counted_rows(const RenderParams &p, int csg_levels, const c2rt_path_opts &g, const uint8_t *counts, const c2rt_path_planes &out, uint32_t row0,
                        uint32_t rows, void *scratch, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    CountedArgs a;
    return launch_rows_of(p, csg_levels, out, counted_args(g, counts, a), rows, [&](auto L, dim3 grid, uint32_t tiles_x) {
        constexpr int LEVELS = decltype(L)::value;
        const uint64_t n = (uint64_t)rows * p.width;
        if (out.segments || out.indirect || out.bounce || out.radiance) /* `node` alone reads no count */
            if (const int e = enqueue_order(counts, n, a.cap, scratch, s, a.order)) return e;
        if (a.order) grid = ray_grid(n);
        return launch_query(p, path_planes_counted_kernel<LEVELS, true>, path_planes_counted_kernel<LEVELS, false>, grid, stack_lds(p) + (kStartInLds<LEVELS> ? kStartLds : 0), s, p, out, a, row0, rows, tiles_x);
    });
}

/* launch_plane_rays of the path planes with counts[n] beside the planes; scratch as above, for n samples */
int launch_counted_rays(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, uint64_t base, const c2rt_path_opts &g,
                        const uint8_t *counts, const c2rt_path_planes &out, void *scratch, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    CountedArgs a;
    return launch_rays_of(csg_levels, rays, n, out, counted_args(g, counts, a), [&](auto L, dim3 grid) {
        constexpr int LEVELS = decltype(L)::value;
        if (out.segments || out.indirect || out.bounce || out.radiance)
            if (const int e = enqueue_order(counts, n, a.cap, scratch, s, a.order)) return e;
        return launch_query(p, trace_rays_paths_counted_kernel<LEVELS, true>, trace_rays_paths_counted_kernel<LEVELS, false>, grid, stack_lds(p) + (kStartInLds<LEVELS> ? kStartLds : 0), s, p, out, a, rays, n, base);
    });
}

} // namespace c2rt
