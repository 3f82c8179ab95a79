/*
 * c2rt_occlusion.hip — occlusion planes (c2rt_render_occlusion*, c2rt_trace_rays_occlusion*): for the closest hit of one
 * sample, K short visibility tests over the hemisphere around its faceforwarded normal — Lambert.spawnRay's origin and
 * hemisphereSample (rt/shader.d:118-135, 156-174) with Scene.testVisibility (rt/scene.d:62-78) in the place of the
 * recursion — as a bit mask, its open fraction and the sum of the open directions, beside the closest node.  The hit
 * planes' wave (c2rt_hit_planes.hip) for a camera, the ray query's (c2rt_rays.hip) for a caller's rays; the definition a
 * CPU restates bit for bit is in include/c2rt.h.  What the unit shares with the other query kernels: c2rt_query.inc.
 *
 * One lane keeps its sample from the trace to the stores: from, N, bent, the mask (two registers) and the key stay in
 * registers across the sample loop, nothing is staged.  The loop is wave-uniform (K is a kernel argument); lanes without
 * a hit are masked by control flow behind trace_closest, and a wave without any hit skips the loop on one ballot.
 * test_visibility is the visibility query's call: full node mask, no ground shortcut, the full-capacity hit stack.
 * `node` alone traces no sample (wave-uniform flag on the kernel arguments).  What is written to a plane does not depend
 * on which others are asked for.  Nothing is shaded, so the kernels template on LEVELS only, as test_visibility_kernel.
 *
 * Stores: each lane its own values — 4 bytes (node), 8 (open), 4 (ao), three 8-byte stores at a 24-byte stride (bent,
 * as the hit planes store p); all plain vector stores.
 */
#define C2RT_TRACE_EXACT_ONLY
#include "c2rt_trace_common.inc"
#include "c2rt_query.inc"

namespace c2rt {
namespace {

static_assert(sizeof(c2rt_occlusion_planes) == 32 && sizeof(c2rt_occlusion_opts) == 24, "ABI layout of the occlusion structs");
static_assert(C2RT_MAX_OCCLUSION_SAMPLES == 64, "the mask is one 64-bit word");

/* what a call draws its samples with: c2rt_occlusion_opts without its padding (wave-uniform: kernel arguments) */
struct OccArgs {
    double radius;
    uint64_t seed;
    uint32_t samples;
};

/* The planes of sample `idx` — the ray (o, d) of a live lane — stored at element `at` of each plane */
template <int LEVELS>
DEV void occlusion_sample(const Ctx &cx, const c2rt_occlusion_planes &out, const OccArgs &occ, const size_t at, const uint64_t idx, D3 o, D3 d)
{
    using namespace exact;
    Hit best;
    Surf surf;
    Mat mat;
    const int closest = trace_closest<LEVELS>(cx, o, d, false, best, surf, mat);
    if (out.node) out.node[at] = closest;
    if (!(out.open || out.ao || out.bent)) return; /* wave-uniform: `node` alone traces no sample */
    const uint32_t K = occ.samples;                               /* 1 .. 64 */
    unsigned long long open = ~0ull >> (64u - K);                 /* a miss: nothing occludes the sky; never a shift by 64 */
    D3 bent = mk(0, 0, 0);
    const bool hit = closest >= 0;
    if (__ballot(hit) != 0) { /* a wave of misses draws nothing */
        if (hit) {
            const D3 N = dot(d, surf.n) < 0 ? surf.n : -surf.n; /* faceforward — rt/imported_types.d:69-73 */
            const D3 from = surf.p + N * 1e-6;
            const uint32_t key = rng_key(occ.seed, idx, 0);
            open = 0;
            for (uint32_t s = 0; s < K; ++s) { /* wave-uniform trip count */
                const D3 res = hemisphere_sample(key, s, N);
                const D3 to = from + res * occ.radius;
                if (test_visibility<LEVELS, 0>(cx, from, to, 0xFFFFFFFFu, false)) {
                    open |= 1ull << s;
                    bent = bent + res;
                }
            }
        }
    }
    if (out.open) out.open[at] = open;
    if (out.ao) out.ao[at] = (float)__popcll(open) / (float)K;
    if (out.bent) {
        out.bent[at * 3 + 0] = bent.x;
        out.bent[at * 3 + 1] = bent.y;
        out.bent[at * 3 + 2] = bent.z;
    }
}

/* Pixel (x, y) of rows [row0, row0 + rows) of the frame `P` describes: hit_planes_kernel's tile, ray and row mapping;
 * the sample index is the pixel's place in the WHOLE frame, so strips and host chunks draw the same directions */
template <int LEVELS>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_QUERY(LEVELS, false)
occlusion_planes_kernel(const RenderParams P, const c2rt_occlusion_planes out, const OccArgs occ, const uint32_t row0, const uint32_t rows,
                        const uint32_t tiles_x)
{
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const TilePixel px = tile_pixel(P, lane, rows, tiles_x);
    Ctx cx;
    query_ctx(cx, P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    if (px.live) { /* lanes past the edge: masked out before the trace */
        const uint32_t y = px.y(P, row0);
        D3 o, d;
        pixel_ray(cx, P, (double)px.x, (double)y, o, d);
        occlusion_sample<LEVELS>(cx, out, occ, px.idx, (uint64_t)y * P.width + px.x, o, d);
    }
}

/* Ray i of c2rt_trace_rays, `dir` as given: 64 consecutive rays per wave, the tail masked out before the trace; the
 * sample index is base + i, the ray's place in the caller's array when the launch is a host chunk of it */
template <int LEVELS>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_QUERY(LEVELS, false)
trace_rays_occlusion_kernel(const RenderParams P, const c2rt_occlusion_planes out, const OccArgs occ, const c2rt_ray *__restrict__ rays,
                            const uint64_t n, const uint64_t base)
{
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kWave + (uint64_t)lane; /* the grid is ceil(n / 64) */
    Ctx cx;
    query_ctx(cx, P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    if (i < n) {
        D3 o, d;
        load6(rays + i, o, d);
        occlusion_sample<LEVELS>(cx, out, occ, (size_t)i, base + i, o, d);
    }
}

/* (the longest argument list of the unit, against c2rt_query.inc's bound for the others) */
static_assert(sizeof(RenderParams) + sizeof(c2rt_occlusion_planes) + sizeof(OccArgs) + 24 <= 4096, "the kernel-argument segment holds at most 4 KiB");

inline bool occ_args(const c2rt_occlusion_opts &occ, OccArgs &a)
{
    a.radius = occ.radius;
    a.seed = occ.seed;
    a.samples = occ.samples;
    return occ.samples >= 1 && occ.samples <= C2RT_MAX_OCCLUSION_SAMPLES;
}

} // namespace

/* Rows [row0, row0 + rows) of the local rows of the frame `p` describes (hit_params, c2rt_api.cpp) into planes whose
 * first row is row0; device pointers, at least one of them non-null, rows > 0, 1 <= occ.samples <= 64. */
int launch_plane_rows(const RenderParams &p, int csg_levels, const c2rt_occlusion_opts &occ, const c2rt_occlusion_planes &out, uint32_t row0,
                      uint32_t rows, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    OccArgs a;
    return launch_rows_of(p, csg_levels, out, occ_args(occ, a), rows, [&](auto L, dim3 grid, uint32_t tiles_x) {
        hipLaunchKernelGGL((occlusion_planes_kernel<decltype(L)::value>), grid, dim3(kWave), stack_lds(p), s, p, out, a, row0, rows, tiles_x);
        return (int)hipGetLastError();
    });
}

/* The planes [n] of the caller's rays, ray i drawing the samples of index base + i; p: query_params (c2rt_api.cpp),
 * 0 < n <= C2RT_MAX_RAYS */
int launch_plane_rays(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, uint64_t base, const c2rt_occlusion_opts &occ,
                      const c2rt_occlusion_planes &out, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    OccArgs a;
    return launch_rays_of(csg_levels, rays, n, out, occ_args(occ, a), [&](auto L, dim3 grid) {
        hipLaunchKernelGGL((trace_rays_occlusion_kernel<decltype(L)::value>), grid, dim3(kWave), stack_lds(p), s, p, out, a, rays, n, base);
        return (int)hipGetLastError();
    });
}

} // namespace c2rt
