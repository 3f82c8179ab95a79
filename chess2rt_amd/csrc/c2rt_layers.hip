/*
 * c2rt_layers.hip — hit layers (c2rt_trace_rays_layers*, c2rt_render_hit_layers*): every surface along a ray, in order,
 * in one launch.  The reference's CsgOp.findAllIntersections (rt/geometry.d:271-290) with the scene's `trace`
 * (rt/renderer.d:325-338) in the place of geom.intersect: layer k of a ray is the closest hit of the ray that starts
 * 1e-6 directions behind layer k - 1's point, its `dist` accumulated without the steps; the walk ends with the first
 * miss, which is stored, or at max_layers (include/c2rt.h, "hit layers", is the contract).
 *
 * Two kernels, the two single-hit query kernels with a loop around the trace:
 *   trace_ray_layers_kernel — c2rt_rays.hip's trace_rays_kernel: 64 consecutive rays of the caller's array per wave;
 *   hit_layers_kernel       — c2rt_hit_planes.hip's hit_planes_kernel: one 8x8 tile of a camera frame per wave, the ray
 *                             from pixel_ray, strips as there.
 * What they share with the other query kernels (exact:: arithmetic, no culling, the full-capacity hit stack, its
 * occupancy): c2rt_query.inc.  Outputs are layer-major — layer k's slice of every output is the output of the single-hit
 * kernel, `layer_stride` records or pixels behind layer k - 1's —, so each layer's stores are those kernels' stores.
 *
 * The loop is wave-synchronous.  A lane WALKS while it has a ray to trace: it starts walking when it is inside the
 * array / the frame, and stops when it misses.  Everything between two loop heads is inside `if (walking)`: a lane that
 * is past the end or that has missed is out by control flow before the next trace_closest, so the __all / __ballot /
 * readfirstlane of the trace only ever see lanes with a ray, as in the single-hit kernels.  The loop ends when the
 * ballot of the walking lanes is zero or at max_layers; both are wave-uniform, the loop branch is scalar.
 * trace_closest's `record` is set whenever the caller reads a record field OR another layer may follow (k + 1 <
 * max_layers): surf.p seeds the next origin and best.dist the total.  With max_layers == 1 it is the single-hit
 * kernel's flag.  (The bits of a record do not depend on it.)
 *
 * A lane of NaNs, zeros or 1e300 walks like any other through the bounded loops of the trace; a step that does not move
 * it (p + d * 1e-6 == p) finds the same surface again until max_layers ends it.  What it computes stays in its own
 * registers and slots.
 *
 * Record stores of the ray kernel: each walking lane stores its own ten words, 8-byte stores at an 80-byte stride.  No
 * LDS, no barrier, and a lane that does not walk stores nothing, so a slot behind a ray's final miss is not touched.
 * trace_rays_kernel's way — the walking lanes stage their records in the hit stack while it is dead and the whole wave
 * writes them as rows, word w belonging to lane w / kHitWords and the layer's ballot saying whether that lane stored —
 * was built and measured against it (profiles/hit_layers.md): 240.0 against 231.8 us for hits + colour at 4 layers
 * (151.5 against 148.0 at one), 168.3 against 171.9 us for hits alone.  The rows win what they win in trace_rays_kernel
 * only while nothing else is stored; with colours the LDS round trip and the two barriers per layer cost more, and
 * the ten rows in flight needed eight more VGPRs.  The plain store is kept.
 * The frame kernel stores as hit_planes_kernel does (store_hit_planes), each lane its own values: measured faster there.
 * All stores are plain vector stores.
 */
#define C2RT_TRACE_EXACT_ONLY
#include "c2rt_trace_common.inc"
#include "c2rt_query.inc"

namespace c2rt {
namespace {

static_assert(C2RT_MAX_HIT_LAYERS <= 255, "a ray's count is one byte");

/* The register budget: the query kernels' (C2RT_WAVES_QUERY), but for the depth-1 instance with one light.  That one
 * has four waves per SIMD there, 128 VGPRs, of which trace_rays_kernel uses 109; with the origin, the total, the count
 * and the loop on top the compiler spilled 22 to 24 VGPRs to scratch at that budget.  Three waves per SIMD, the budget
 * of its several-lights twin: no scratch — and one wave in four less, which one layer of a depth-1, one-light scene
 * pays with 20 % over the single-hit call (profiles/hit_layers.md). */
template <int LEVELS, bool MLC>
constexpr int occ_layers() { return LEVELS == 1 ? 3 : occ_query<LEVELS, MLC>(); }
#define C2RT_WAVES_LAYERS(L, M) __attribute__((amdgpu_waves_per_eu(occ_layers<L, M>(), occ_layers<L, M>())))

/* One layer's bookkeeping behind trace_closest, for a walking lane: temp.dist += currentLength; currentLength =
 * temp.dist (rt/geometry.d:283-284) for a hit — one addition, the steps not counted — and the count. */
DEV void layer_account(const int closest, Hit &best, double &total, uint32_t &cnt)
{
    if (closest >= 0) {
        best.dist = best.dist + total;
        total = best.dist;
        ++cnt;
    }
}

/* The direction never changes, and the optimiser knows: it would compute everything of a layer that depends on `d`
 * alone (make_ray's magnitude and reciprocals, the shaders' terms) once ahead of the loop and keep it in registers
 * across every layer — registers the single-hit kernels do not hold and the budget does not have: 24 VGPRs spilled in
 * the depth-0 frame kernel, 48 at depth 1.  The empty asm makes each layer's `d` a value of its own: the layer is the single-hit kernel's code on the
 * single-hit kernel's registers, plus the origin, the total and the count. */
DEV void layer_dir(D3 &d)
{
    asm volatile("" : "+v"(d.x), "+v"(d.y), "+v"(d.z));
}

/* the next layer's origin: p + dir * 1e-6, componentwise, product then sum (the build does not contract) */
DEV D3 layer_step(const D3 &p, const D3 &d)
{
    return mk(p.x + d.x * 1e-6, p.y + d.y * 1e-6, p.z + d.z * 1e-6);
}

/* Ray i, layers 0 .. max_layers - 1.  hits / rgb / count: nullable, not all three (wave-uniform); layer k's record of ray
 * i at hits[k * layer_stride + i], its colour at rgb[(k * layer_stride + i) * 3]; 1 <= max_layers. */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_LAYERS(LEVELS, MLC)
trace_ray_layers_kernel(const RenderParams P, const c2rt_ray *__restrict__ rays, const uint64_t n, const uint32_t max_layers,
                        const uint64_t layer_stride, c2rt_ray_hit *__restrict__ hits, float *__restrict__ rgb, uint8_t *__restrict__ count)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * kWave; /* < n: the grid is ceil(n / 64) */
    const uint64_t i = first + (uint64_t)lane;
    Ctx cx;
    query_ctx(cx, P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    D3 o = mk(0, 0, 0), d = mk(0, 0, 0);
    bool walking = i < n;
    if (walking) load6(rays + i, o, d);
    double total = 0.0;
    uint32_t cnt = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < max_layers; ++k) {
        if (!__ballot(walking)) break;
        const bool record = hits != nullptr || k + 1 < max_layers; /* wave-uniform */
        const uint64_t slot = (uint64_t)k * layer_stride;
        if (walking) {
            Hit best;
            Surf surf;
            Mat mat;
            layer_dir(d);
            const int closest = trace_closest<LEVELS>(cx, o, d, record, best, surf, mat);
            layer_account(closest, best, total, cnt);
            if (hits) store_record(reinterpret_cast<unsigned long long *>(hits + slot + i), closest, best, surf);
            if (rgb) store_colour(rgb + (slot + i) * 3, sample_colour<LEVELS, MLC>(P, cx, closest, mat, d, surf));
            if (closest < 0) walking = false;
            else o = layer_step(surf.p, d);
        }
    }
    if (i < n && count) count[i] = (uint8_t)cnt;
}

/* Pixel (x, r) of rows [row0, row0 + rows) of the frame `P` describes, layers 0 .. max_layers - 1: hit_planes_body with
 * the loop around the trace.  Layer k's slice of a plane starts k * layer_px * components elements behind its pointer;
 * `out` and `count` point at row row0. */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_LAYERS(LEVELS, MLC)
hit_layers_kernel(const RenderParams P, const c2rt_hit_planes out, uint8_t *__restrict__ count, const uint32_t max_layers,
                  const size_t layer_px, const uint32_t row0, const uint32_t rows, const uint32_t tiles_x)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const TilePixel px = tile_pixel(P, lane, rows, tiles_x);
    const bool fields = out.dist || out.uv || out.p || out.normal; /* wave-uniform */
    Ctx cx;
    query_ctx(cx, P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    D3 o = mk(0, 0, 0), d = mk(0, 0, 0);
    bool walking = px.live;
    if (walking) pixel_ray(cx, P, (double)px.x, (double)px.y(P, row0), o, d);
    double total = 0.0;
    uint32_t cnt = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < max_layers; ++k) {
        if (!__ballot(walking)) break;
        const bool record = fields || k + 1 < max_layers; /* wave-uniform */
        const size_t idx = (size_t)k * layer_px + px.idx;
        if (walking) {
            Hit best;
            Surf surf;
            Mat mat;
            layer_dir(d);
            const int closest = trace_closest<LEVELS>(cx, o, d, record, best, surf, mat);
            layer_account(closest, best, total, cnt);
            store_hit_planes<LEVELS, MLC>(P, cx, out, idx, closest, best, surf, mat, d);
            if (closest < 0) walking = false;
            else o = layer_step(surf.p, d);
        }
    }
    if (px.live && count) count[px.idx] = (uint8_t)cnt;
}

} // namespace

int launch_trace_ray_layers(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, uint32_t max_layers, uint64_t layer_stride,
                            c2rt_ray_hit *hits, float *rgb, uint8_t *count, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!n || n > C2RT_MAX_RAYS || !max_layers || max_layers > C2RT_MAX_HIT_LAYERS || layer_stride < n || (!hits && !rgb && !count))
        return (int)hipErrorInvalidValue;
    return for_csg_levels(csg_levels, [&](auto L) {
        constexpr int LEVELS = decltype(L)::value;
        return launch_query(p, trace_ray_layers_kernel<LEVELS, true>, trace_ray_layers_kernel<LEVELS, false>, ray_grid(n), stack_lds(p), s, p, rays, n,
                            max_layers, layer_stride, hits, rgb, count);
    });
}

int launch_hit_layers(const RenderParams &p, int csg_levels, const c2rt_hit_planes &out, uint8_t *count, uint32_t max_layers, size_t layer_px,
                      uint32_t row0, uint32_t rows, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!rows || !p.width || !max_layers || max_layers > C2RT_MAX_HIT_LAYERS || layer_px < (size_t)rows * p.width || !(any_plane(out) || count))
        return (int)hipErrorInvalidValue;
    uint32_t tiles_x;
    const dim3 grid = tile_grid(p, rows, tiles_x);
    return for_csg_levels(csg_levels, [&](auto L) {
        constexpr int LEVELS = decltype(L)::value;
        return launch_query(p, hit_layers_kernel<LEVELS, true>, hit_layers_kernel<LEVELS, false>, grid, stack_lds(p), s, p, out, count, max_layers, layer_px,
                            row0, rows, tiles_x);
    });
}

} // namespace c2rt
