/*
 * c2rt_trace_common.inc — what a device translation unit needs before it can write a kernel: the HIP runtime header and
 * the device tables, the out-of-line libm wrappers, the register budget per instance (occ_of), the diagnostics knobs,
 * the trace itself and the host helper that picks an instance by CSG depth.  Included once, at file
 * scope, by the frame file (c2rt_kernels.hip: lean:: and exact::) and by the query files (c2rt_rays.hip,
 * c2rt_hit_planes.hip, c2rt_adaptive.hip), which define C2RT_TRACE_EXACT_ONLY first: they run exact:: arithmetic only
 * and need no lean:: copy of the trace (the emitted code is the same either way, and so is the compile time, about
 * 25 s per query object: the unused copy is only parsed).
 *
 * The trace comes in two halves.  What does not depend on the arithmetic mode is defined once, at c2rt:: scope:
 * c2rt_trace_shared.inc (types, vectors, records, Ctx, textures, RNG, pixel store) and c2rt_tile_mask.inc (the
 * pre-pass classifier).  What does is c2rt_trace.inc, included into namespace lean (kLean = true) and again into
 * namespace exact (kLean = false).  The rule: a definition is in c2rt_trace.inc if and only if it reads kLean or
 * calls or instantiates something that does (the few exceptions are named in that file's header); only such names
 * are ever written lean:: or exact::.
 */
#include <hip/hip_runtime.h>

#include <type_traits>

#include "c2rt_device.h"
#include "csg_certain.h"
#include "f32_certain.h"
#include "fp64_lean.h"
#include "ground_certain.h"
#include "x87.h"

/* Leaf CsgOps decided by csg_certain.h (c2rt_trace.inc: csg_intersect_leaf) exist in the FRAME units only.  A query unit
 * (C2RT_TRACE_EXACT_ONLY) compiles the text it compiled before that route existed, token for token — the route's
 * declarations, the `own` / `self` arguments that carry a shadow ray's source node down, Ctx::csg_certain — so that its
 * kernels stay the instructions they were (scripts/isa_equal.py): an argument that is never read still moved their
 * scalar registers. */
#ifdef C2RT_TRACE_EXACT_ONLY
#define C2RT_CSG_CERTAIN 0
#define C2RT_OWN(NEED) false
#define C2RT_SELF
#else
#define C2RT_CSG_CERTAIN 1
#define C2RT_OWN(NEED) ((NEED) == kBool && own)
#define C2RT_SELF , self
#endif
/* Likewise the straight-line path for tiles that hold the ground and one leaf CsgOp node (c2rt_trace.inc:
 * lean::csg_tile, called from render_tile): frame units only, so that a query unit does not even parse it. */
#ifdef C2RT_TRACE_EXACT_ONLY
#define C2RT_CSG_TILE 0
#else
#define C2RT_CSG_TILE 1
#endif

namespace c2rt {
namespace {

#define DEV __device__ __forceinline__

/* fp64 libm is only reached by a few lanes (sphere u,v, the Phong lobe,
 * Procedure2) but, inlined, its ~70 live registers set the whole kernel's
 * budget; as real calls the trace stays under 168 VGPRs without spills. */
__device__ __noinline__ double c2_sin(double a) { return sin(a); }
/* Sphere.intersect's u,v (rt/geometry.d:118-120) out of line as well: the x87 emulation (x87.h) is ~500 integer
 * instructions with ~40 live registers, reached by textured sphere hits only; inlined (twice: lean:: and exact::)
 * it was where the headline instance spilled. */
struct UV { double u, v; };
__device__ __noinline__ UV c2_sphere_uv(double dx, double dz, double w)
{
    constexpr double PI = 3.14159265358979323846;
    const double angle = atan2(dz, dx);
    const double as = asin(w);
    UV r;
    r.u = fabs(angle) <= 4.0 ? x87_sphere_u(angle) : (PI + angle) / (2 * PI);
    r.v = fabs(as) <= 2.0 ? x87_sphere_v(as) : 1.0 - (PI / 2 + as) / PI;
    return r;
}
/* The two of them that are converted to float at once by their readers in a frame (f32_certain.h): the cheap expression wherever the float that
 * comes out of it is certain to be the one above gives, the routine above for the other lanes (a divergent branch
 * the wave skips when no lane needs it: one lane in a few million does).
 * c2_pow_f32: (float)pow(a, b), the Phong lobe of shade() — its only reader, so there is no double-valued twin. */
__device__ __noinline__ float c2_pow_f32(double a, double b)
{
    float f;
    if (pow_f32_certain(a, b, &f)) return f;
    return (float)pow(a, b);
}
/* c2_sphere_uv_bitmap: u, v for BitmapTexture.getTexColor with scaling s, which reads (float)(u*s - floor(u*s)) and
 * nothing else: doubles from which bitmap_color computes the floats it computes from c2_sphere_uv's — NOT those
 * doubles themselves (they differ by up to 2^-51), so nothing that reports u, v may call it. */
__device__ __noinline__ UV c2_sphere_uv_bitmap(double dx, double dz, double w, double s_uniform)
{
    /* The scaling must be WAVE-UNIFORM (it is: one texture per call, hit_surface runs per distinct closest node).  Held
     * in scalar registers it is not live in a vector pair across atan2 and asin; with that and the sequential tests
     * below the function needs the 22 VGPRs of c2_sphere_uv, not 25 — a count every calling kernel's budget includes. */
    const double s = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(s_uniform)), __builtin_amdgcn_readfirstlane(__double2loint(s_uniform)));
    const double angle = atan2(dz, dx);
    const double as = asin(w);
    UV r;
    /* (one coordinate after the other, each behind a branch: tested side by side they add three VGPRs to this function) */
    bool certain = sphere_uv_fast(angle, as, &r.u, &r.v) != 0;
    if (certain) certain = uv_float_certain(r.u, F32C_UV_DELTA, s) != 0;
    if (certain) certain = uv_float_certain(r.v, F32C_UV_DELTA, s) != 0;
    if (!certain) {
        constexpr double PI = 3.14159265358979323846;
        r.u = fabs(angle) <= 4.0 ? x87_sphere_u(angle) : (PI + angle) / (2 * PI);
        r.v = fabs(as) <= 2.0 ? x87_sphere_v(as) : 1.0 - (PI / 2 + as) / PI;
    }
    return r;
}
/* Register budget per kernel instance, as waves per SIMD (512 VGPRs per lane and SIMD: 128 at 4 waves,
 * 168 at 3, 256 at 2).  With no hint hipcc takes all 512 registers and runs one wave per SIMD (1.8x
 * slower).  Chosen per instance from the compiler's resource remarks (`make resource-usage`; profiles/r04_resource_usage.md)
 * so that NO instance spills VGPRs to scratch, except where a measurement says otherwise:
 *   depth 0 (no CSG), planes-only: 4 waves (111-127 VGPRs);
 *   depth 1, at most one light: 4 waves — 128 VGPRs since the cube / sphere face tables moved to the upload
 *     and the hit's lighting terms are evaluated before the shadow test (was 149 at 3 waves);
 *   depth 1, several lights (the hit stays live across the light loop) and depth-1 DOF: 3 waves (144-162);
 *   depth 2 / 3 / 4: THREE waves (168 VGPRs) although they then spill (depth 4 multi-light: 136 VGPRs, 240 B of
 *     scratch per lane; at two waves it needs 230 and spills none): a wave of these instances issues one
 *     instruction at a time and a third of its instructions are scalar, so with two waves per SIMD the VALU idles
 *     half the time (VALU busy 0.53) — the third wave is worth more than the spills cost: csg_stress.sdl cut to
 *     depth 2 / 3 / 4: 2.33 -> 1.88, 4.60 -> 3.97, 10.21 -> 8.53 ms (scripts/depth_occupancy.sh; four waves:
 *     2.59 / 5.48 / 10.5).  The hit stacks have to fit three workgroups per CU too: kCsgFirstCap, c2rt_device.h. */
template <int LEVELS, int DOF, bool MLC>
constexpr int occ_of()
{
    return LEVELS == 0 ? 4 : (LEVELS == 1 ? ((DOF || MLC) ? 3 : 4) : 3);
}
#define C2RT_WAVES_OF(L, D, M) __attribute__((amdgpu_waves_per_eu(occ_of<L, D, M>(), occ_of<L, D, M>())))
#ifndef C2RT_TILE_STATS
#define C2RT_TILE_STATS 0 /* diagnostics: per-tile wave cycles + class (RenderParams::tile_stats) */
#endif

/* the arithmetic-independent half, once; then the half that reads kLean, once per namespace */
#include "c2rt_trace_shared.inc"
#include "c2rt_tile_mask.inc"

#ifndef C2RT_TRACE_EXACT_ONLY
namespace lean {
constexpr bool kLean = true;
#include "c2rt_trace.inc"
} // namespace lean
#endif
namespace exact {
constexpr bool kLean = false;
#include "c2rt_trace.inc"
} // namespace exact

/* The instance of a scene's CSG depth (KernelVariant::csg_levels, chosen at upload): f(std::integral_constant<int, L>)
 * for L = levels, an error for a depth no instance was built for.  Host side. */
template <int L = 0, class F>
int for_csg_levels(int levels, F &&f)
{
    if (levels == L) return f(std::integral_constant<int, L>{});
    if constexpr (L < C2RT_MAX_CSG_DEPTH) return for_csg_levels<L + 1>(levels, f);
    else return (int)hipErrorInvalidValue;
}

} // namespace
} // namespace c2rt
