/*
 * c2rt_shade_planes.hip — shading planes (c2rt_render_shading*, c2rt_trace_rays_shading*): the terms of the closest
 * node's Lambert.shade / Phong.shade (rt/shader.d:67-105, 197-250) of one sample, one plane per term — diffuseColor,
 * lightContrib, Phong's specular, which lights passed the visibility condition — beside the closest node and the colour
 * the terms make.  The hit planes' wave (c2rt_hit_planes.hip) for a camera, the ray query's (c2rt_rays.hip) for a
 * caller's rays, with exact::shade taken apart: shade_parts below is that function's statement sequence composed from
 * the same pieces (tex_color, light_terms, test_visibility, c2_pow_f32) — the same operations on the same operands in
 * the same order, contraction off, so the same bits — returning the three sums and the visibility word where shade
 * returns their combination.  The colour is then formed as shade forms it, so `rgb` has the hit planes' bits and the
 * planes satisfy rgb == albedo * light (+ specular for Phong) bit for bit.  What the unit shares with the other query
 * kernels: c2rt_query.inc.
 *
 * Work skipped, by wave-uniform flags on the kernel arguments (as rgb == NULL in the hit planes): `node` and `albedo`
 * alone cast no shadow ray and evaluate no light; the texture is read only when `albedo` or `rgb` is asked for.  What
 * is written to a plane does not depend on which others are asked for.
 *
 * Stores: each lane its own values — one 12-byte store per float plane (store_colour), one 4-byte store for `node` and
 * for `visible`; all plain vector stores.  The planes are a kernel argument of their own behind the parameter block.
 */
#define C2RT_TRACE_EXACT_ONLY
#include "c2rt_trace_common.inc"
#include "c2rt_query.inc"

namespace c2rt {
namespace {

/* the three locals of the reference's shade() at its return, and bit l: light l < 32 passed
 * `lightColor.intensity() != 0 && scene.testVisibility(p + N * 1e-6, lightPos)` */
struct ShadeParts {
    F3 albedo, light, specular;
    uint32_t visible;
};

/* exact::shade<LEVELS, MLC, 0> (c2rt_trace.inc) statement for statement, its three sums kept apart.  lit (wave-uniform):
 * the lights are evaluated; false leaves light / specular / visible at their initial values, which nobody stores. */
template <int LEVELS, bool MLC>
DEV ShadeParts shade_parts(const RenderParams &P, const Ctx &cx, const Mat &mat, D3 rd, const Surf &h, bool want_albedo, bool lit)
{
    using namespace exact;
    ShadeParts r;
    const bool phong = mat.shader_type == C2RT_SHADER_PHONG;
    const D3 N = dot(rd, h.n) < 0 ? h.n : -h.n; /* faceforward — rt/imported_types.d:69-73 */
    r.albedo = mkf(0, 0, 0);
    if (want_albedo) r.albedo = mat.tex_type >= 0 ? tex_color(P, mat, h.u, h.v) : mat.color;
    F3 lightContrib = mkf(P.ambient[0], P.ambient[1], P.ambient[2]);
    F3 specular = mkf(0, 0, 0);
    uint32_t word = 0;
    if (lit) {
        if constexpr (!MLC) {
            if (P.n_lights) {
                LightP L = (LightP)P.lights;
                F3 avgColor = mkf(0, 0, 0), avgSpecular = mkf(0, 0, 0);
                if (L->lit & 1u) {
                    const D3 lightPos = ld3(L->pos);
                    const D3 from = h.p + N * 1e-6;
                    double cosTheta, cosGamma;
                    F3 baseLight;
                    light_terms(cx.bad, L, lightPos, h.p, N, rd, phong, cosTheta, baseLight, cosGamma);
                    const bool visible = test_visibility<LEVELS, 0>(cx, from, lightPos, cx.shadow_mask0, cx.shadow_ground_only);
                    if (visible) {
                        word = 1u;
                        if (cosTheta > 0) avgColor = avgColor + baseLight * (float)cosTheta;
                        if (phong & (cosGamma > 0))
                            avgSpecular = avgSpecular + baseLight * c2_pow_f32(cosGamma, mat.exponent) * mat.strength;
                    }
                }
                lightContrib = lightContrib + avgColor;
                specular = specular + avgSpecular;
            }
        } else {
            const D3 p = h.p;
            const double exponent = mat.exponent;
            const float strength = mat.strength;
            const uint32_t nl = P.n_lights;
            for (uint32_t l0 = 0; l0 < nl; l0 += 32u) {
                const uint32_t l1 = l0 + 32u < nl ? l0 + 32u : nl;
                uint32_t vis = 0;
                for (uint32_t l = l0; l < l1; ++l) {
                    LightP L = (LightP)P.lights + l;
                    if (L->lit & 1u) {
                        const D3 from = p + N * 1e-6;
                        if (test_visibility<LEVELS, 0>(cx, from, ld3(L->pos), l == 0 ? cx.shadow_mask0 : light_shadow_mask(P, cx.mask_slot, l), l == 0 && cx.shadow_ground_only))
                            vis |= 1u << (l - l0);
                    }
                }
                if (l0 == 0) word = vis; /* lights 0..31: the `visible` plane; later lights have no bit */
                for (uint32_t l = l0; l < l1; ++l) {
                    LightP L = (LightP)P.lights + l;
                    F3 avgColor = mkf(0, 0, 0), avgSpecular = mkf(0, 0, 0);
                    if ((L->lit & 1u) && ((vis >> (l - l0)) & 1u)) {
                        double cosTheta, cosGamma;
                        F3 baseLight;
                        light_terms(cx.bad, L, ld3(L->pos), p, N, rd, phong, cosTheta, baseLight, cosGamma);
                        if (cosTheta > 0) avgColor = avgColor + baseLight * (float)cosTheta;
                        if (phong & (cosGamma > 0))
                            avgSpecular = avgSpecular + baseLight * c2_pow_f32(cosGamma, exponent) * strength;
                    }
                    lightContrib = lightContrib + avgColor;
                    specular = specular + avgSpecular;
                }
            }
        }
    }
    r.light = lightContrib;
    r.specular = specular;
    r.visible = word;
    return r;
}

/* The planes of sample `idx` — the ray (o, d) of a live lane — after the closest-hit search; a miss holds node -1,
 * visible 0 and +0 in every float (rgb: Environment.getEnvironment, rt/environment.d:7-10). */
template <int LEVELS, bool MLC>
DEV void shade_sample(const RenderParams &P, const Ctx &cx, const c2rt_shade_planes &out, const size_t idx, D3 o, D3 d)
{
    using namespace exact;
    /* wave-uniform: kernel arguments */
    const bool lit = out.light || out.specular || out.visible || out.rgb;
    const bool want_albedo = out.albedo || out.rgb;
    Hit best;
    Surf surf;
    Mat mat;
    const int closest = trace_closest<LEVELS>(cx, o, d, false, best, surf, mat);
    if (out.node) out.node[idx] = closest;
    if (!(lit || want_albedo)) return;
    ShadeParts s;
    s.albedo = s.light = s.specular = mkf(0, 0, 0);
    s.visible = 0;
    F3 c = mkf(0, 0, 0);
    if (closest >= 0) {
        s = shade_parts<LEVELS, MLC>(P, cx, mat, d, surf, want_albedo, lit);
        const F3 res = s.albedo * s.light; /* shade's last two statements */
        c = mat.shader_type == C2RT_SHADER_PHONG ? res + s.specular : res;
    }
    if (out.albedo) store_colour(out.albedo + idx * 3, s.albedo);
    if (out.light) store_colour(out.light + idx * 3, s.light);
    if (out.specular) store_colour(out.specular + idx * 3, s.specular);
    if (out.visible) out.visible[idx] = s.visible;
    if (out.rgb) store_colour(out.rgb + idx * 3, c);
}

/* Pixel (x, y) of rows [row0, row0 + rows) of the frame `P` describes: hit_planes_kernel's tile, ray and row mapping */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_QUERY(LEVELS, MLC)
shade_planes_kernel(const RenderParams P, const c2rt_shade_planes out, const uint32_t row0, const uint32_t rows, const uint32_t tiles_x)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const TilePixel px = tile_pixel(P, lane, rows, tiles_x);
    Ctx cx;
    query_ctx(cx, P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    if (px.live) { /* lanes past the edge: masked out before the trace */
        D3 o, d;
        pixel_ray(cx, P, (double)px.x, (double)px.y(P, row0), o, d);
        shade_sample<LEVELS, MLC>(P, cx, out, px.idx, o, d);
    }
}

/* Ray i of c2rt_trace_rays, `dir` as given: 64 consecutive rays per wave, the tail masked out before the trace */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_QUERY(LEVELS, MLC)
trace_rays_shade_kernel(const RenderParams P, const c2rt_shade_planes out, const c2rt_ray *__restrict__ rays, const uint64_t n)
{
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kWave + (uint64_t)lane; /* the grid is ceil(n / 64) */
    Ctx cx;
    query_ctx(cx, P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    if (i < n) {
        D3 o, d;
        load6(rays + i, o, d);
        shade_sample<LEVELS, MLC>(P, cx, out, (size_t)i, o, d);
    }
}

} // namespace

/* Rows [row0, row0 + rows) of the local rows of the frame `p` describes (hit_params, c2rt_api.cpp) into planes whose
 * first row is row0; device pointers, at least one of them non-null, rows > 0. */
int launch_plane_rows(const RenderParams &p, int csg_levels, const NoOpts &, const c2rt_shade_planes &out, uint32_t row0, uint32_t rows, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return launch_rows_of(p, csg_levels, out, true, rows, [&](auto L, dim3 grid, uint32_t tiles_x) {
        constexpr int LEVELS = decltype(L)::value;
        return launch_query(p, shade_planes_kernel<LEVELS, true>, shade_planes_kernel<LEVELS, false>, grid, stack_lds(p), s, p, out, row0, rows, tiles_x);
    });
}

/* The planes [n] of the caller's rays (no samples are drawn: `base` is not read); p: query_params (c2rt_api.cpp),
 * 0 < n <= C2RT_MAX_RAYS */
int launch_plane_rays(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, uint64_t, const NoOpts &, const c2rt_shade_planes &out,
                      void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return launch_rays_of(csg_levels, rays, n, out, true, [&](auto L, dim3 grid) {
        constexpr int LEVELS = decltype(L)::value;
        return launch_query(p, trace_rays_shade_kernel<LEVELS, true>, trace_rays_shade_kernel<LEVELS, false>, grid, stack_lds(p), s, p, out, rays, n);
    });
}

} // namespace c2rt
