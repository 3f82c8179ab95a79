/*
 * c2rt_paths.hip — path planes (c2rt_render_paths*, c2rt_trace_rays_paths*): multi-bounce indirect diffuse light of the
 * closest hit of one sample, renderSampleGI's pathsPerPixel paths of up to maxTraceDepth bounces (rt/renderer.d:289-301,
 * pathtrace_impl 378-463) in the build-defined reading of include/c2rt.h: P paths from Lambert.spawnRay's origin along
 * hemisphereSample (rt/shader.d:118-135, 156-174), every vertex continued as Lambert continues it, every segment traced
 * and shaded as c2rt_trace_rays traces and shades a caller's ray (Renderer.raytrace: direct light by shadow rays) and
 * weighted with the path's throughput: 2 cos at the first vertex, times (albedo of the vertex left) * 2 cos behind it.
 * Beside the closest node: how many spawned segments hit a node, the mean over the paths, the mean times the primary
 * albedo, and the frame's colour plus that.  With one bounce the planes are the gather planes' (c2rt_gather.hip).  The hit
 * planes' wave (c2rt_hit_planes.hip) for a camera, the ray query's (c2rt_rays.hip) for a caller's rays; the definition a
 * CPU restates bit for bit is in include/c2rt.h.  What the unit shares with the other query kernels: c2rt_query.inc.
 *
 * The loop is FLAT: a lane walks its own cursor (path p, depth j) and one iteration traces one segment of every live
 * lane.  A lane whose path ends — at a miss, or at the last depth — takes (from0, N0) back and starts its next path in
 * the same iteration; a lane leaves when its P paths are used up and the wave when every lane has.  So the wave's trip
 * count is the largest number of segments any of its lanes traces, not P times the deepest path of any lane: in
 * lecture5 one spawned ray in seven hits anything, and a nest "for path, for bounce" would walk every depth some lane
 * still lives at with most lanes masked off (measured: profiles/paths.md).  The bound is P * Beff iterations by construction, whatever
 * a trace returns: a lane of NaNs ends like any other.  The order of a lane's fp32 sum is path-major, bounce-minor either
 * way, so the bits do not depend on the loop's shape.
 *
 * Across the loop a lane keeps from0, N0 (in LDS at depth 1: occ_paths below), from, N, the throughput (with the albedo
 * of the vertex left already in it), the sum and — when asked for — the primary albedo, the cursor and the count; the
 * primary colour waits in its plane; no ray is read or written.  Wave-uniform flags on the kernel arguments: `node` alone traces no path, `node` + `segments` alone cast no shadow ray and fetch no
 * albedo, only `radiance` shades the primary hit.  What is written to a plane does not depend on which others are asked
 * for.
 *
 * Stores: each lane its own values — 4 bytes (node), 4 (segments), 12, 12 and 12 (store_colour); all plain vector stores.
 */
#define C2RT_TRACE_EXACT_ONLY
#include "c2rt_trace_common.inc"
#include "c2rt_query.inc"

namespace c2rt {
namespace {

static_assert(sizeof(c2rt_path_planes) == 40 && sizeof(c2rt_path_opts) == 16, "ABI layout of the path structs");

/* The register budget: the gather kernel's (two inlined closest-hit searches and a shade) with the path's state on top —
 * from0 and N0 above all, twelve registers the gather loop does not hold.  Depth 0 takes three waves per SIMD (151 .. 153
 * of 168 registers; four would leave 128).  Depth 1 with everything in registers does not fit three (13 / 11 VGPRs
 * spilled, 64 / 48 B of scratch per lane) and at two (180 / 177 registers) a one-bounce call on lecture5 is 32 % behind
 * the gather planes, which run at three.  So at depth 1 from0 and N0 wait in LDS behind the hit stack — six doubles per
 * lane, component-major, 3 KiB per wave on top of the stack's 10, which still leaves twelve waves per CU their LDS — and
 * the one-light instances fit three waves (167 registers, no spill); the several-lights instances still spill two
 * registers there and take two waves (profiles/paths.md) */
template <int LEVELS, bool MLC>
constexpr int occ_paths() { return LEVELS >= 2 || (LEVELS == 1 && MLC) ? 2 : 3; }
template <int LEVELS> constexpr bool kStartInLds = LEVELS == 1;
constexpr size_t kStartLds = (size_t)kWave * 6 * sizeof(double);
static_assert(occ_query<2, true>() == 2 && occ_query<4, false>() == 2, "the nested instances keep the query kernels' budget");
#define C2RT_WAVES_PATHS(L, M) __attribute__((amdgpu_waves_per_eu(occ_paths<L, M>(), occ_paths<L, M>())))

/* what a call draws its paths with: c2rt_path_opts (wave-uniform: kernel arguments) */
struct PathArgs {
    uint64_t seed;
    uint32_t paths, bounces;
};

/* diffuseColor of a hit, as shade takes it (the shading planes' `albedo`) */
DEV F3 albedo_of(const RenderParams &P, const Mat &mat, const Surf &surf)
{
    return mat.tex_type >= 0 ? tex_color(P, mat, surf.u, surf.v) : mat.color;
}

/* the lane's slot of the start state behind the wave's hit stack (the launch adds kStartLds where kStartInLds) */
DEV double *start_of(const RenderParams &P, char *lds, const int lane)
{
    return reinterpret_cast<double *>(lds + (size_t)P.csg_cap * kCsgLdsPerEntry) + lane;
}

/* The planes of sample `idx` — the ray (o, d) of a live lane — stored at element `at` of each plane */
template <int LEVELS, bool MLC>
DEV void path_sample(const RenderParams &P, const Ctx &cx, const c2rt_path_planes &out, const PathArgs &g, const size_t at, const uint64_t idx, D3 o,
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
    const uint32_t NP = g.paths;                /* 1 .. 64 */
    /* the spawned ray at vertex j has depth j + 1: trace() returns black before intersecting beyond max_trace_depth */
    const uint32_t beff = g.bounces < P.max_trace_depth ? g.bounces : P.max_trace_depth;
    const bool hit = closest >= 0;
    /* the primary hit's shadow rays; the colour waits in its plane, not in three registers across the loop */
    if (out.radiance) store_colour(out.radiance + at * 3, sample_colour<LEVELS, MLC>(P, cx, closest, mat, d, surf));
    uint32_t segments = 0;
    F3 sum = mkf(0, 0, 0), a0 = mkf(0, 0, 0);
    if (beff != 0 && __ballot(hit) != 0) { /* a wave of misses draws nothing */
        if (hit) {
            const D3 N0 = dot(d, surf.n) < 0 ? surf.n : -surf.n; /* faceforward — rt/imported_types.d:69-73 */
            const D3 from0 = surf.p + N0 * 1e-6;
            if (want_albedo) a0 = albedo_of(P, mat, surf);
            D3 N = N0, from = from0;
            if constexpr (kStartInLds<LEVELS>) {
                start[0 * kWave] = from0.x, start[1 * kWave] = from0.y, start[2 * kWave] = from0.z;
                start[3 * kWave] = N0.x, start[4 * kWave] = N0.y, start[5 * kWave] = N0.z;
            }
            F3 T = mkf(0, 0, 0); /* behind the first vertex: the throughput times the albedo of the vertex just left */
            uint32_t p = 0, j = 0; /* the cursor: path, depth */
            for (;;) {             /* at most NP * beff iterations: every one advances the cursor */
                const D3 res = hemisphere_sample(rng_key(g.seed, idx, j), p, N);
                if (want_colour) { /* before the trace: N is not kept across it */
                    const float w = (float)(2.0 * dot(res, N)); /* ((1 / PI) * cos) / (1 / (2 PI)) */
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
    const F3 indirect = sum / (float)NP;
    const F3 bounce = a0 * indirect;
    if (out.indirect) store_colour(out.indirect + at * 3, indirect);
    if (out.bounce) store_colour(out.bounce + at * 3, bounce);
    if (out.radiance && hit && beff != 0) { /* elsewhere the colour stays as it is */
        float *rad = out.radiance + at * 3;
        store_colour(rad, mkf(rad[0], rad[1], rad[2]) + bounce);
    }
}

/* Pixel (x, y) of rows [row0, row0 + rows) of the frame `P` describes: hit_planes_kernel's tile, ray and row mapping;
 * the sample index is the pixel's place in the WHOLE frame, so strips and host chunks draw the same directions */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_PATHS(LEVELS, MLC)
path_planes_kernel(const RenderParams P, const c2rt_path_planes out, const PathArgs g, const uint32_t row0, const uint32_t rows, const uint32_t tiles_x)
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
        path_sample<LEVELS, MLC>(P, cx, out, g, px.idx, (uint64_t)y * P.width + px.x, o, d, start_of(P, lds, lane));
    }
}

/* Ray i of c2rt_trace_rays, `dir` as given: 64 consecutive rays per wave, the tail masked out before the trace; the
 * sample index is base + i, the ray's place in the caller's array when the launch is a host chunk of it */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_PATHS(LEVELS, MLC)
trace_rays_paths_kernel(const RenderParams P, const c2rt_path_planes out, const PathArgs g, const c2rt_ray *__restrict__ rays, const uint64_t n,
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
        path_sample<LEVELS, MLC>(P, cx, out, g, (size_t)i, base + i, o, d, start_of(P, lds, lane));
    }
}

static_assert(sizeof(RenderParams) + sizeof(c2rt_path_planes) + sizeof(PathArgs) + 24 <= 4096, "the kernel-argument segment holds at most 4 KiB");

inline bool path_args(const c2rt_path_opts &g, PathArgs &a)
{
    a.seed = g.seed;
    a.paths = g.paths;
    a.bounces = g.bounces;
    return g.paths >= 1 && g.paths <= C2RT_MAX_PATHS && g.bounces >= 1 && g.bounces <= C2RT_MAX_PATH_BOUNCES;
}

} // namespace

/* Rows [row0, row0 + rows) of the local rows of the frame `p` describes (hit_params, c2rt_api.cpp) into planes whose
 * first row is row0; device pointers, at least one of them non-null, rows > 0, g within its limits. */
int launch_plane_rows(const RenderParams &p, int csg_levels, const c2rt_path_opts &g, const c2rt_path_planes &out, uint32_t row0, uint32_t rows,
                      void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    PathArgs a;
    return launch_rows_of(p, csg_levels, out, path_args(g, a), rows, [&](auto L, dim3 grid, uint32_t tiles_x) {
        constexpr int LEVELS = decltype(L)::value;
        return launch_query(p, path_planes_kernel<LEVELS, true>, path_planes_kernel<LEVELS, false>, grid, stack_lds(p) + (kStartInLds<LEVELS> ? kStartLds : 0), s, p, out, a, row0, rows, tiles_x);
    });
}

/* The planes [n] of the caller's rays, ray i drawing the paths of index base + i; p: query_params (c2rt_api.cpp),
 * 0 < n <= C2RT_MAX_RAYS */
int launch_plane_rays(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, uint64_t base, const c2rt_path_opts &g,
                      const c2rt_path_planes &out, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    PathArgs a;
    return launch_rays_of(csg_levels, rays, n, out, path_args(g, a), [&](auto L, dim3 grid) {
        constexpr int LEVELS = decltype(L)::value;
        return launch_query(p, trace_rays_paths_kernel<LEVELS, true>, trace_rays_paths_kernel<LEVELS, false>, grid, stack_lds(p) + (kStartInLds<LEVELS> ? kStartLds : 0), s, p, out, a, rays, n, base);
    });
}

} // namespace c2rt
