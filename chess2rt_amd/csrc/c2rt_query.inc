/*
 * c2rt_query.inc — what the query kernels share (c2rt_rays.hip, c2rt_hit_planes.hip, c2rt_adaptive.hip): a lane traces
 * ONE ray that is not a frame tile's — the caller's, or the camera's through a pixel — with exact:: arithmetic (the
 * probe's choice; bit-equal to what the frames compute), every culling mask all ones (query_ctx,
 * c2rt_trace_shared.inc), no ground-tile shortcut, and a full-capacity CSG hit stack: kCsgFullCap(LEVELS) entries in one
 * launch, which cannot overflow, so there is no retry list and no per-stream scratch.  That is 10 / 20 / 30 / 40 KiB
 * of LDS per wave at depth 1 / 2 / 3 / 4: the LDS, not the registers, bounds the occupancy of the nested instances
 * (8 / 5 / 4 workgroups per CU), hence two waves per SIMD as their register budget (DESIGN.md, "Ray queries").
 * One wavefront per workgroup.  Included at file scope, after c2rt_trace_common.inc with C2RT_TRACE_EXACT_ONLY.
 */
#include "c2rt_query.h"

namespace c2rt {
namespace {

static_assert(sizeof(RenderParams) + 64 <= 4096, "the kernel-argument segment holds at most 4 KiB");

template <int LEVELS, bool MLC>
constexpr int occ_query() { return LEVELS >= 2 ? 2 : occ_of<LEVELS, 0, MLC>(); }
#define C2RT_WAVES_QUERY(L, M) __attribute__((amdgpu_waves_per_eu(occ_query<L, M>(), occ_query<L, M>())))


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

} // namespace
} // namespace c2rt
