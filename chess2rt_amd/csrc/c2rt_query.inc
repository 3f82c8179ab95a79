/*
 * c2rt_query.inc — what the query kernels share (c2rt_rays.hip, c2rt_hit_planes.hip, c2rt_layers.hip,
 * c2rt_shade_planes.hip, c2rt_occlusion.hip, c2rt_gather.hip, c2rt_paths.hip, c2rt_paths_counted.hip, c2rt_adaptive.hip, c2rt_sample_taps.hip): a lane traces
 * ONE ray that is not a frame tile's — the caller's, or the camera's through a pixel — with exact:: arithmetic (the probe's choice; bit-equal to what the frames compute), every
 * culling mask all ones (query_ctx, c2rt_trace_shared.inc), no ground-tile shortcut, and a full-capacity CSG hit stack:
 * kCsgFullCap(LEVELS) entries in one launch, which cannot overflow, so there is no retry list and no per-stream scratch.
 * That is 10 / 20 / 30 / 40 KiB of LDS per wave at depth 1 / 2 / 3 / 4: the LDS, not the registers, bounds the
 * occupancy of the nested instances (8 / 5 / 4 workgroups per CU), hence two waves per SIMD as their register budget
 * (DESIGN.md, "Ray queries").  One wavefront per workgroup.  Included at file scope, after c2rt_trace_common.inc with
 * C2RT_TRACE_EXACT_ONLY.
 *
 * Each piece once, in this order: the ABI layout the lane code relies on; the register budget; where a lane's sample
 * comes from (load6 for a caller's record, tile_pixel and pixel_ray for a camera's pixel; hemisphere_sample for the
 * directions the occlusion, gather and path planes draw behind a hit); where its result goes
 * (store_colour, store_record, sample_colour, store_hit_planes); the host side of a launch (ray_grid, tile_grid,
 * launch_query; launch_rows_of and launch_rays_of, the two launch shapes of the plane families).
 */
#include "c2rt_query.h"

namespace c2rt {
namespace {

constexpr int kHitWords = (int)(sizeof(c2rt_ray_hit) / 8);
static_assert(sizeof(c2rt_ray) == 48 && sizeof(c2rt_segment) == 48 && sizeof(c2rt_ray_hit) == 80 && kHitWords * 8 == sizeof(c2rt_ray_hit), "ABI layout of the query records");
static_assert(__builtin_offsetof(c2rt_ray_hit, leaf_geom) == 4 && __builtin_offsetof(c2rt_ray_hit, dist) == 8 &&
              __builtin_offsetof(c2rt_ray_hit, p) == 32 && __builtin_offsetof(c2rt_ray_hit, normal) == 56, "ABI layout of c2rt_ray_hit");
static_assert(sizeof(c2rt_hit_planes) == 56 && sizeof(c2rt_shade_planes) == 48, "ABI layout of the plane structs");
/* (the longest argument list behind the parameter block is hit_layers_kernel's: the planes and 40 bytes) */
static_assert(sizeof(RenderParams) + sizeof(c2rt_hit_planes) + 40 <= 4096, "the kernel-argument segment holds at most 4 KiB");

template <int LEVELS, bool MLC>
constexpr int occ_query() { return LEVELS >= 2 ? 2 : occ_of<LEVELS, 0, MLC>(); }
#define C2RT_WAVES_QUERY(L, M) __attribute__((amdgpu_waves_per_eu(occ_query<L, M>(), occ_query<L, M>())))

/* six doubles of an array-of-structures input record (c2rt_ray, c2rt_segment): three 16-byte loads where the
 * hardware takes them at 8-byte alignment */
typedef double __attribute__((ext_vector_type(2), aligned(8))) d2_t;
DEV void load6(const void *rec, D3 &a, D3 &b)
{
    const d2_t *q = static_cast<const d2_t *>(rec);
    const d2_t q0 = q[0], q1 = q[1], q2 = q[2];
    a = mk(q0.x, q0.y, q1.x);
    b = mk(q1.y, q2.x, q2.y);
}

/* Pixel -> lane of the kernels that take their rays from a camera (the output does not depend on it): the frames' 8x8
 * tile.  Measured for the hit planes against a run of 64 pixels of one row — every store instruction of a scalar plane
 * covers 256 / 512 contiguous bytes — and against 16x4: lecture5.sdl 1080p, all seven planes / node + dist / all but
 * rgb: 117.9 / 62.6 / 65.3 us for the run, 112.8 / 60.1 / 62.0 for the 8x8 tile, 112.5 / 59.9 / 62.1 for 16x4
 * (profiles/hit_planes.md): coherent rays and fewer distinct closest nodes per wave are worth more than the wider
 * stores. */
constexpr int kQueryTileW = 8, kQueryTileH = kWave / kQueryTileW;

/* The pixel of lane `lane` of tile blockIdx.x of a launch over `rows` local rows of the frame `P` describes (the grid is
 * tile_grid's): column x, row r within the launch, idx = r * width + x.  A lane past the right or bottom edge is not
 * live: the caller masks it out by control flow before the trace, as the ray kernels mask their tail. */
struct TilePixel {
    uint32_t x, r;
    bool live;
    size_t idx;
    /* the frame row of a live lane, row0 the launch's first local row: local row -> frame row under interleaved
     * strips, as render_tile maps it */
    DEV uint32_t y(const RenderParams &P, const uint32_t row0) const
    {
        const uint32_t lr = r + row0;
        if (P.strip_world <= 1) return lr;
        const uint32_t sh = P.strip_height;
        return ((lr / sh) * P.strip_world + P.strip_rank) * sh + lr % sh;
    }
};
DEV TilePixel tile_pixel(const RenderParams &P, const int lane, const uint32_t rows, const uint32_t tiles_x)
{
    const uint32_t trow = blockIdx.x / tiles_x, tcol = blockIdx.x % tiles_x;
    TilePixel t;
    t.x = tcol * kQueryTileW + (uint32_t)(lane % kQueryTileW);
    t.r = trow * kQueryTileH + (uint32_t)(lane / kQueryTileW);
    t.live = t.x < P.width && t.r < rows;
    t.idx = (size_t)t.r * P.width + t.x;
    return t;
}

/* The ray through the screen point (x, y) — a pixel's integer corner, plus its tap offset where there is one — of the
 * camera of `P`: Camera.getScreenRay, then raytrace()'s normalisation (rt/camera.d:144-147) — the operations the
 * frame kernels and the probe apply to (x, y). */
DEV void pixel_ray(const Ctx &cx, const RenderParams &P, double x, double y, D3 &o, D3 &d)
{
    Rng rng = {0u, 0, 0};
    D3 raw;
    exact::screen_ray<false>(cx.bad, P, x, y, 0, rng, o, raw);
    d = exact::normalized(cx.bad, raw);
}

/* hemisphereSample(N), rt/shader.d:156-174, draw s of the sample whose key is `key` (the occlusion, gather and path planes):
 * theta = 2 pi u, phi = acos(w) - pi / 2 with w = 2 v - 1, so sin(phi) = -w and cos(phi) = sqrt(1 - w^2) — IEEE +, *,
 * sqrt and lens_sincos2pi only, no libm (include/c2rt.h, the definition of a sample under "occlusion planes") */
DEV D3 hemisphere_sample(const uint32_t key, const uint32_t s, const D3 N)
{
    const double u = rng_uniform(key, s, 0), v = rng_uniform(key, s, 1);
    double sn, cs;
    lens_sincos2pi(u, sn, cs);
    const double w = 2.0 * v - 1.0;
    const double c = sqrt(1.0 - w * w);
    const D3 res = mk(cs * c, -w, sn * c);
    return dot(res, N) < 0 ? -res : res;
}

/* one 12-byte store per lane, as the frame kernels store pixels */
typedef float __attribute__((ext_vector_type(3), aligned(4))) f3_t;
DEV void store_colour(float *rgb, F3 c)
{
    f3_t v3;
    v3.x = c.r;
    v3.y = c.g;
    v3.z = c.b;
    *reinterpret_cast<f3_t *>(rgb) = v3;
}

/* The ten 8-byte words of the c2rt_ray_hit of a traced ray at `rec`, in LDS or in HBM; a miss holds leaf -1 and what
 * trace_closest left in best.dist and surf. */
DEV void store_record(unsigned long long *rec, const int closest, const Hit &best, const Surf &surf)
{
    const int leaf = closest >= 0 ? best.g : -1;
    rec[0] = (unsigned long long)(uint32_t)closest | ((unsigned long long)(uint32_t)leaf << 32);
    rec[1] = (unsigned long long)__double_as_longlong(best.dist);
    rec[2] = (unsigned long long)__double_as_longlong(surf.u);
    rec[3] = (unsigned long long)__double_as_longlong(surf.v);
    rec[4] = (unsigned long long)__double_as_longlong(surf.p.x);
    rec[5] = (unsigned long long)__double_as_longlong(surf.p.y);
    rec[6] = (unsigned long long)__double_as_longlong(surf.p.z);
    rec[7] = (unsigned long long)__double_as_longlong(surf.n.x);
    rec[8] = (unsigned long long)__double_as_longlong(surf.n.y);
    rec[9] = (unsigned long long)__double_as_longlong(surf.n.z);
}

/* The colour of the sample whose closest-hit search returned `closest`: trace(ray, TraceType.Ray) behind the search,
 * rt/renderer.d:339-376 at depth 0 */
template <int LEVELS, bool MLC>
DEV F3 sample_colour(const RenderParams &P, const Ctx &cx, const int closest, const Mat &mat, const D3 &d, const Surf &surf)
{
    F3 c = mkf(0, 0, 0); /* Environment.getEnvironment — rt/environment.d:7-10 */
    uint32_t shadow_rays = 0;
    if (closest >= 0) c = exact::shade<LEVELS, MLC, 0>(P, cx, mat, d, surf, shadow_rays);
    return c;
}

/* The same record as the seven hit planes at sample `idx`, those asked for (wave-uniform: kernel arguments).  Each lane
 * stores its own values, the three-component planes as three 8-byte stores at a 24-byte stride, uv as one 16-byte store
 * declared 8-aligned (a batch's slice of an odd-sized frame is aligned to nothing but its element); the colour is
 * evaluated only when its plane is there.  All plain vector stores. */
template <int LEVELS, bool MLC>
DEV void store_hit_planes(const RenderParams &P, const Ctx &cx, const c2rt_hit_planes &out, const size_t idx, const int closest,
                          const Hit &best, const Surf &surf, const Mat &mat, const D3 &d)
{
    if (out.node) out.node[idx] = closest;
    if (out.leaf) out.leaf[idx] = closest >= 0 ? best.g : -1;
    if (out.dist) out.dist[idx] = best.dist;
    if (out.uv) {
        d2_t uv;
        uv.x = surf.u;
        uv.y = surf.v;
        *reinterpret_cast<d2_t *>(out.uv + idx * 2) = uv;
    }
    if (out.p) {
        out.p[idx * 3 + 0] = surf.p.x;
        out.p[idx * 3 + 1] = surf.p.y;
        out.p[idx * 3 + 2] = surf.p.z;
    }
    if (out.normal) {
        out.normal[idx * 3 + 0] = surf.n.x;
        out.normal[idx * 3 + 1] = surf.n.y;
        out.normal[idx * 3 + 2] = surf.n.z;
    }
    if (out.rgb) store_colour(out.rgb + idx * 3, sample_colour<LEVELS, MLC>(P, cx, closest, mat, d, surf));
}

/* ---- host side: one launch of a query kernel ---- */

/* one wave per 64 consecutive records of the caller's array */
inline dim3 ray_grid(uint64_t n) { return dim3((uint32_t)((n + kWave - 1) / kWave)); }

/* one wave per tile of `rows` rows of the frame, n_frames frames side by side: at most 2^16 x 2^16 pixels / 64, and
 * n_frames <= C2RT_MAX_BATCH_FRAMES */
inline dim3 tile_grid(const RenderParams &p, uint32_t rows, uint32_t &tiles_x, uint32_t n_frames = 1)
{
    tiles_x = (p.width + kQueryTileW - 1) / kQueryTileW;
    return dim3(tiles_x * ((rows + kQueryTileH - 1) / kQueryTileH), n_frames);
}

/* the hit stack of one wave: the dynamic LDS of every query kernel (c2rt_rays.hip and c2rt_adaptive.hip keep more there) */
inline size_t stack_lds(const RenderParams &p) { return (size_t)p.csg_cap * kCsgLdsPerEntry; }

/* `several` for a scene with more than one light, `one` otherwise (the two MLC instances of one kernel), one wavefront
 * per workgroup */
template <class K, class... A>
int launch_query(const RenderParams &p, K *several, K *one, dim3 grid, size_t lds, hipStream_t s, const A &...args)
{
    hipLaunchKernelGGL(p.n_lights > 1 ? several : one, grid, dim3(kWave), lds, s, args...);
    return (int)hipGetLastError();
}

/* The two launch shapes of the plane families (launch_plane_rows / launch_plane_rays of each unit): refuse, size the grid,
 * pick the CSG depth.  opts_ok: the unit's option struct converted (OccArgs, GatherArgs, PathArgs; true where there is none).
 * launch(L, grid, tiles_x) / launch(L, grid) enqueues the unit's kernel of depth decltype(L)::value, so a unit names
 * only the instances it had before, whether its kernels template on LEVELS alone or on LEVELS and MLC. */
template <class S, class Launch>
int launch_rows_of(const RenderParams &p, int csg_levels, const S &out, bool opts_ok, uint32_t rows, Launch launch)
{
    if (!rows || !p.width || !any_plane(out) || !opts_ok) return (int)hipErrorInvalidValue;
    uint32_t tiles_x;
    const dim3 grid = tile_grid(p, rows, tiles_x);
    return for_csg_levels(csg_levels, [&](auto L) { return launch(L, grid, tiles_x); });
}
template <class S, class Launch>
int launch_rays_of(int csg_levels, const c2rt_ray *rays, uint64_t n, const S &out, bool opts_ok, Launch launch)
{
    if (!n || n > C2RT_MAX_RAYS || !rays || !any_plane(out) || !opts_ok) return (int)hipErrorInvalidValue;
    return for_csg_levels(csg_levels, [&](auto L) { return launch(L, ray_grid(n)); });
}

} // namespace
} // namespace c2rt
