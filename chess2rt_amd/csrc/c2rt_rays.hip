/*
 * c2rt_rays.hip — ray and visibility queries (c2rt_trace_rays*, c2rt_test_visibility*): the caller's rays instead of a camera's.
 * One ray per lane, 64 consecutive rays per wavefront, one wavefront per workgroup — the frame kernels' shape with
 * the tile replaced by a run of the caller's array, so the trace below it is the same wave-synchronous code: scalar
 * node loop, scalar record loads, one surface pass per distinct closest node.  What it shares with the other query
 * kernels (exact:: arithmetic, no culling, the full-capacity hit stack and its occupancy): c2rt_query.inc.
 *
 * Lanes past n (the tail wave) are masked out by ordinary control flow BEFORE the trace, as the frame kernels mask the
 * lanes past the frame's edge: __all / __ballot / readfirstlane below only ever see live lanes, so a dead lane can
 * neither store nor steer a wave-uniform decision.  A lane holding garbage (NaN, zero direction, 1e300) is live and
 * goes through the same bounded loops as a frame's lane does; what it computes stays in its own registers.
 *
 * Memory: the ABI is array-of-structures.  Rays: three 16-byte loads per lane at a 48-byte stride — every 128-byte
 * line a wave touches is consumed whole by the three loads together, the second and third hit in the vector L1, and
 * nothing is written, so no transposition.  Colours: one 12-byte store per lane, 768 contiguous bytes per wave, as
 * the frame kernels store pixels.  Hit records: 80 bytes per lane; stored by the lane itself that would be ten 8-byte
 * stores at an 80-byte stride, each store instruction of the wave dirtying 8 of every 80 bytes of 40 lines.  Instead
 * the wave stages its records in LDS — in the hit stack, which is dead between the closest-hit search and the first
 * shadow ray — and writes them out as rows: lane l stores words l, l + 64, ... of the wave's 640 8-byte words, so each
 * of the ten store instructions covers 512 contiguous bytes, four whole lines.  (8-byte rather than 16-byte rows:
 * c2rt_ray_hit is only 8-byte aligned for a C caller.)  All of them plain vector stores.
 */
#define C2RT_TRACE_EXACT_ONLY
#include "c2rt_trace_common.inc"
#include "c2rt_query.inc"

namespace c2rt {
namespace {

/* Ray i = trace(ray, TraceType.Ray), rt/renderer.d:325-376, depth 0.  hits / rgb: nullable, not both (wave-uniform). */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_QUERY(LEVELS, MLC)
trace_rays_kernel(const RenderParams P, const c2rt_ray *__restrict__ rays, const uint64_t n, c2rt_ray_hit *__restrict__ hits, float *__restrict__ rgb)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * kWave; /* < n: the grid is ceil(n / 64) */
    const uint64_t i = first + (uint64_t)lane;
    const bool live = i < n;
    Ctx cx;
    query_ctx(cx, P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    D3 o = mk(0, 0, 0), d = mk(0, 0, 0);
    Hit best;
    Surf surf;
    Mat mat;
    int closest = -1;
    unsigned long long *stage = reinterpret_cast<unsigned long long *>(lds); /* [64][kHitWords] */
    if (live) {
        load6(rays + i, o, d);
        closest = trace_closest<LEVELS>(cx, o, d, hits != nullptr, best, surf, mat);
        if (hits) store_record(stage + lane * kHitWords, closest, best, surf);
    }
    if (hits) {
        /* every lane of the wave, live or not: the rows of the records of the live lanes (LDS operations of one
         * wave complete in order; the workgroup is this wave) */
        __builtin_amdgcn_wave_barrier();
        const uint64_t left = n - first;
        const uint32_t words = (uint32_t)(left < (uint64_t)kWave ? left : (uint64_t)kWave) * (uint32_t)kHitWords;
        unsigned long long *out = reinterpret_cast<unsigned long long *>(hits + first);
#pragma unroll
        for (int k = 0; k < kHitWords; ++k) {
            const uint32_t w = (uint32_t)lane + (uint32_t)(k * kWave);
            if (w < words) out[w] = stage[w];
        }
        __builtin_amdgcn_wave_barrier(); /* the shadow rays below reuse the stack */
    }
    if (live && rgb) {
        /* sample_colour's statements, written out: through the function the depth 1 - 4 instances come out with two
         * register pairs exchanged; like this the unit's code is the measured one (profiles/query_shared.md) */
        F3 c = mkf(0, 0, 0); /* Environment.getEnvironment — rt/environment.d:7-10 */
        uint32_t shadow_rays = 0;
        if (closest >= 0) c = shade<LEVELS, MLC, 0>(P, cx, mat, d, surf, shadow_rays);
        store_colour(rgb + i * 3, c);
    }
}

/* Segment i = Scene.testVisibility(from, to), rt/scene.d:62-78: full node mask, no ground shortcut */
template <int LEVELS>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_QUERY(LEVELS, false)
test_visibility_kernel(const RenderParams P, const c2rt_segment *__restrict__ seg, const uint64_t n, uint8_t *__restrict__ visible)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kWave + (uint64_t)lane;
    if (i >= n) return; /* nothing after the trace needs the whole wave */
    Ctx cx;
    query_ctx(cx, P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    D3 from, to;
    load6(seg + i, from, to);
    const bool vis = test_visibility<LEVELS, 0>(cx, from, to, 0xFFFFFFFFu, false);
    visible[i] = vis ? (uint8_t)1 : (uint8_t)0;
}

} // namespace

/* the instance of the scene's CSG depth, as the frame kernels are chosen at upload; p.csg_cap = kCsgFullCap(levels) */
int launch_trace_rays(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, c2rt_ray_hit *hits, float *rgb, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!n || n > C2RT_MAX_RAYS || (!hits && !rgb)) return (int)hipErrorInvalidValue;
    /* the staged records share the LDS with the hit stack, which a scene without CSG does not have */
    const size_t stage = hits ? (size_t)kWave * sizeof(c2rt_ray_hit) : 0, lds = stack_lds(p) > stage ? stack_lds(p) : stage;
    return for_csg_levels(csg_levels, [&](auto L) {
        constexpr int LEVELS = decltype(L)::value;
        return launch_query(p, trace_rays_kernel<LEVELS, true>, trace_rays_kernel<LEVELS, false>, ray_grid(n), lds, s, p, rays, n, hits, rgb);
    });
}

int launch_test_visibility(const RenderParams &p, int csg_levels, const c2rt_segment *seg, uint64_t n, uint8_t *visible, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!n || n > C2RT_MAX_RAYS) return (int)hipErrorInvalidValue;
    return for_csg_levels(csg_levels, [&](auto L) {
        hipLaunchKernelGGL((test_visibility_kernel<decltype(L)::value>), ray_grid(n), dim3(kWave), stack_lds(p), s, p, seg, n, visible);
        return (int)hipGetLastError();
    });
}

} // namespace c2rt
