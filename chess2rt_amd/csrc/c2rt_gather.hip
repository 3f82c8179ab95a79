/*
 * c2rt_gather.hip — gather planes (c2rt_render_gather*, c2rt_trace_rays_gather*): one-bounce indirect diffuse light of
 * the closest hit of one sample.  K rays from Lambert.spawnRay's origin along hemisphereSample (rt/shader.d:118-135,
 * 156-174) — the occlusion planes' draws, bit for bit (hemisphere_sample, c2rt_query.inc) — each traced and shaded as
 * c2rt_trace_rays traces and shades a caller's ray (Renderer.raytrace: direct light by shadow rays), weighted with
 * pathtrace_impl's brdfEval / pdf without the albedo (rt/renderer.d:451-460) and averaged; beside the closest node: a
 * bit mask of the spawned rays that hit something, the mean, and the mean times the hit's albedo.  The hit planes' wave
 * (c2rt_hit_planes.hip) for a camera, the ray query's (c2rt_rays.hip) for a caller's rays; the definition a CPU restates
 * bit for bit is in include/c2rt.h.  What the unit shares with the other query kernels: c2rt_query.inc.
 *
 * One lane keeps its sample from the trace to the stores: from, N, the three float sums, the mask (two registers), the
 * key and — when `bounce` is asked for — the albedo stay in registers across the sample loop; no ray is read or written.
 * The loop is wave-uniform (K is a kernel argument); lanes without a hit are masked by control flow behind the primary
 * trace_closest, a wave without any hit skips the loop on one ballot, a scene with max_trace_depth == 0 skips it
 * wave-uniformly (the spawned ray would have depth 1: trace() returns black before intersecting, rt/renderer.d:330).
 * The spawned rays see the full node mask and no ground shortcut, as query_ctx sets the context up — a frame tile's
 * masks say nothing about rays that start on a surface.  They are shaded, so the kernels template on MLC as well.
 * Wave-uniform flags on the kernel arguments: `node` alone traces no sample, `node` + `hits` alone cast no shadow ray,
 * `indirect` without `bounce` fetches no primary albedo.  What is written to a plane does not depend on which others
 * are asked for.
 *
 * Stores: each lane its own values — 4 bytes (node), 8 (hits), 12 and 12 (store_colour); all plain vector stores.
 */
#define C2RT_TRACE_EXACT_ONLY
#include "c2rt_trace_common.inc"
#include "c2rt_query.inc"

namespace c2rt {
namespace {

static_assert(sizeof(c2rt_gather_planes) == 32 && sizeof(c2rt_gather_opts) == 16, "ABI layout of the gather structs");
static_assert(C2RT_MAX_GATHER_SAMPLES == 64, "the mask is one 64-bit word");

/* The register budget: C2RT_WAVES_QUERY's, except where two inlined closest-hit searches and a shade do not fit its 128
 * registers — at four waves per SIMD the depth-0 several-lights instances spill 2 VGPRs and the depth-1 one-light
 * instances 30 / 39 to scratch; at three (168 registers) nothing does (profiles/gather.md) */
template <int LEVELS, bool MLC>
constexpr int occ_gather() { return LEVELS >= 2 ? occ_query<LEVELS, MLC>() : (LEVELS == 1 || MLC ? 3 : 4); }
#define C2RT_WAVES_GATHER(L, M) __attribute__((amdgpu_waves_per_eu(occ_gather<L, M>(), occ_gather<L, M>())))

/* what a call draws its samples with: c2rt_gather_opts without its padding (wave-uniform: kernel arguments) */
struct GatherArgs {
    uint64_t seed;
    uint32_t samples;
};

/* The planes of sample `idx` — the ray (o, d) of a live lane — stored at element `at` of each plane */
template <int LEVELS, bool MLC>
DEV void gather_sample(const RenderParams &P, const Ctx &cx, const c2rt_gather_planes &out, const GatherArgs &g, const size_t at, const uint64_t idx,
                       D3 o, D3 d)
{
    using namespace exact;
    /* wave-uniform: kernel arguments */
    const bool want_colour = out.indirect || out.bounce;
    const bool want_albedo = out.bounce != nullptr;
    Hit best;
    Surf surf;
    Mat mat;
    const int closest = trace_closest<LEVELS>(cx, o, d, false, best, surf, mat);
    if (out.node) out.node[at] = closest;
    if (!(out.hits || want_colour)) return; /* `node` alone traces no sample */
    const uint32_t K = g.samples;           /* 1 .. 64 */
    unsigned long long hits = 0;
    F3 sum = mkf(0, 0, 0), albedo = mkf(0, 0, 0);
    const bool hit = closest >= 0;
    if (P.max_trace_depth != 0 && __ballot(hit) != 0) { /* a wave of misses draws nothing */
        if (hit) {
            const D3 N = dot(d, surf.n) < 0 ? surf.n : -surf.n; /* faceforward — rt/imported_types.d:69-73 */
            const D3 from = surf.p + N * 1e-6;
            const uint32_t key = rng_key(g.seed, idx, 0);
            /* the primary hit's diffuseColor, as shade takes it: before the loop, three registers across it where
             * mat, u and v would be more */
            if (want_albedo) albedo = mat.tex_type >= 0 ? tex_color(P, mat, surf.u, surf.v) : mat.color;
            for (uint32_t s = 0; s < K; ++s) { /* wave-uniform trip count */
                const D3 res = hemisphere_sample(key, s, N);
                const float w = (float)(2.0 * dot(res, N)); /* ((1 / PI) * cos) / (1 / (2 PI)) */
                Hit sbest;
                Surf ssurf;
                Mat smat;
                const int c = trace_closest<LEVELS>(cx, from, res, false, sbest, ssurf, smat);
                if (c >= 0) hits |= 1ull << s;
                if (want_colour) sum = sum + sample_colour<LEVELS, MLC>(P, cx, c, smat, res, ssurf) * w;
            }
        }
    }
    if (out.hits) out.hits[at] = hits;
    const F3 indirect = sum / (float)K;
    if (out.indirect) store_colour(out.indirect + at * 3, indirect);
    if (out.bounce) store_colour(out.bounce + at * 3, albedo * indirect);
}

/* Pixel (x, y) of rows [row0, row0 + rows) of the frame `P` describes: hit_planes_kernel's tile, ray and row mapping;
 * the sample index is the pixel's place in the WHOLE frame, so strips and host chunks draw the same directions */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_GATHER(LEVELS, MLC)
gather_planes_kernel(const RenderParams P, const c2rt_gather_planes out, const GatherArgs g, const uint32_t row0, const uint32_t rows,
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
        gather_sample<LEVELS, MLC>(P, cx, out, g, px.idx, (uint64_t)y * P.width + px.x, o, d);
    }
}

/* Ray i of c2rt_trace_rays, `dir` as given: 64 consecutive rays per wave, the tail masked out before the trace; the
 * sample index is base + i, the ray's place in the caller's array when the launch is a host chunk of it */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_GATHER(LEVELS, MLC)
trace_rays_gather_kernel(const RenderParams P, const c2rt_gather_planes out, const GatherArgs g, const c2rt_ray *__restrict__ rays, const uint64_t n,
                         const uint64_t base)
{
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kWave + (uint64_t)lane; /* the grid is ceil(n / 64) */
    Ctx cx;
    query_ctx(cx, P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    if (i < n) {
        D3 o, d;
        load6(rays + i, o, d);
        gather_sample<LEVELS, MLC>(P, cx, out, g, (size_t)i, base + i, o, d);
    }
}

static_assert(sizeof(RenderParams) + sizeof(c2rt_gather_planes) + sizeof(GatherArgs) + 24 <= 4096, "the kernel-argument segment holds at most 4 KiB");

inline bool gather_args(const c2rt_gather_opts &g, GatherArgs &a)
{
    a.seed = g.seed;
    a.samples = g.samples;
    return g.samples >= 1 && g.samples <= C2RT_MAX_GATHER_SAMPLES;
}

} // namespace

/* Rows [row0, row0 + rows) of the local rows of the frame `p` describes (hit_params, c2rt_api.cpp) into planes whose
 * first row is row0; device pointers, at least one of them non-null, rows > 0, 1 <= g.samples <= 64. */
int launch_plane_rows(const RenderParams &p, int csg_levels, const c2rt_gather_opts &g, const c2rt_gather_planes &out, uint32_t row0, uint32_t rows,
                      void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    GatherArgs a;
    return launch_rows_of(p, csg_levels, out, gather_args(g, a), rows, [&](auto L, dim3 grid, uint32_t tiles_x) {
        constexpr int LEVELS = decltype(L)::value;
        return launch_query(p, gather_planes_kernel<LEVELS, true>, gather_planes_kernel<LEVELS, false>, grid, stack_lds(p), s, p, out, a, row0, rows, tiles_x);
    });
}

/* The planes [n] of the caller's rays, ray i drawing the samples of index base + i; p: query_params (c2rt_api.cpp),
 * 0 < n <= C2RT_MAX_RAYS */
int launch_plane_rays(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, uint64_t base, const c2rt_gather_opts &g,
                      const c2rt_gather_planes &out, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    GatherArgs a;
    return launch_rays_of(csg_levels, rays, n, out, gather_args(g, a), [&](auto L, dim3 grid) {
        constexpr int LEVELS = decltype(L)::value;
        return launch_query(p, trace_rays_gather_kernel<LEVELS, true>, trace_rays_gather_kernel<LEVELS, false>, grid, stack_lds(p), s, p, out, a, rays, n, base);
    });
}

} // namespace c2rt
