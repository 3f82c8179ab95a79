/*
 * c2rt_kernels.hip — the per-pixel ray-trace hot path of Chess2RT, written
 * for gfx950 (MI355X, CDNA4).  Not a port: the reference is a D class
 * hierarchy with virtual dispatch over a linear node list; this is a
 * wave-synchronous trace where
 *
 *   - one 64-lane wavefront owns one 8x8 pixel tile (one workgroup = one
 *     wave; the grid has >>256 workgroups, dealt round-robin to the 8 XCDs, and
 *     the block -> tile map gives each XCD every 8th tile ROW so that texel
 *     reuse stays inside one XCD's L2 while all XCDs see the same sky/floor mix);
 *   - every lane walks the SAME node / geometry / light at the same time, so
 *     the scene records are read with scalar loads into SGPRs and the type
 *     dispatch is a scalar branch, never a divergent one;
 *   - CSG hit lists live in LDS, one per-lane stack per wave shared by the
 *     nesting levels ([entry][lane]: bank = lane, conflict-free for any per-lane
 *     entry index); only (dist, tag) is kept per hit and the winning hit is
 *     re-derived: 16 entries = 10 KiB per wave at depth 1 and 2, 20 entries = 12.5 KiB at depth 3 and 4 on the
 *     first pass (kCsgFirstCap, c2rt_device.h; 16 x depth on the rare full-capacity retry pass);
 *   - geometry is fp64 and colour fp32 in the reference's operation order
 *     (built with -ffp-contract=off), because checker edges, shadow
 *     terminators and CSG boundaries flip on 1-ulp differences.
 *
 * This file holds the kernel entry points and launchers.  The trace itself is
 * c2rt_trace.inc, included twice below: lean:: (divide / sqrt / normalise through
 * the shortened correctly rounded sequences of fp64_lean.h, optimistically) and
 * exact:: (the compiler's IEEE expansions); render_one() runs a tile through
 * lean:: and again through exact:: when an operand left the lean windows.
 *
 * What each function restates is cited as file:line of /root/reference/source.
 */
#include <hip/hip_runtime.h>

#include "c2rt_device.h"
#include "fp64_lean.h"
#include "x87.h"

namespace c2rt {
namespace {

#define DEV __device__ __forceinline__

/* fp64 libm is only reached by a few lanes (sphere u,v, the Phong lobe,
 * Procedure2) but, inlined, its ~70 live registers set the whole kernel's
 * budget; as real calls the trace stays under 168 VGPRs without spills. */
__device__ __noinline__ double c2_pow(double a, double b) { return pow(a, b); }
__device__ __noinline__ double c2_atan2(double a, double b) { return atan2(a, b); }
__device__ __noinline__ double c2_asin(double a) { return asin(a); }
__device__ __noinline__ double c2_sin(double a) { return sin(a); }
__device__ __noinline__ double c2_cos(double a) { return cos(a); }
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
#ifndef C2RT_OCC_U1
#define C2RT_OCC_U1 4
#endif
#ifndef C2RT_OCC_DEEP
#define C2RT_OCC_DEEP 3
#endif
#ifndef C2RT_OCC_U2
#define C2RT_OCC_U2 3
#endif
#ifndef C2RT_OCC_U3
#define C2RT_OCC_U3 C2RT_OCC_DEEP
#endif
template <int LEVELS, int DOF, bool MLC>
constexpr int occ_of()
{
#ifndef C2RT_OCC_U0
#define C2RT_OCC_U0 4
#endif
    return LEVELS == 0 ? (DOF ? 4 : C2RT_OCC_U0) : (LEVELS == 1 ? ((DOF || MLC) ? 3 : C2RT_OCC_U1) : (LEVELS == 2 ? C2RT_OCC_U2 : (LEVELS == 3 ? C2RT_OCC_U3 : C2RT_OCC_DEEP)));
}
#define C2RT_OCC_OF(L, D, M) __attribute__((amdgpu_waves_per_eu(occ_of<L, D, M>(), occ_of<L, D, M>())))
#ifndef C2RT_TILE_STATS
#define C2RT_TILE_STATS 0 /* diagnostics: per-tile wave cycles + class (RenderParams::tile_stats) */
#endif
#ifndef C2RT_XCD_SWIZZLE
#define C2RT_XCD_SWIZZLE 1
#endif

namespace lean {
constexpr bool kLean = true;
#include "c2rt_trace.inc"
} // namespace lean
namespace exact {
constexpr bool kLean = false;
#include "c2rt_trace.inc"
} // namespace exact

#ifndef C2RT_LEAN
#define C2RT_LEAN 1 /* 0: the production instances run exact:: only (A/B builds) */
#endif
/* The deepest CSG nesting whose instances carry the lean:: copy.  Depth 4 does not: measured with and without it
 * at two waves per SIMD (10.39 / 10.42 ms on csg_stress) and at three (8.60 / 8.56) — no difference, twice the
 * code. */
#ifndef C2RT_LEAN_MAX_LEVELS
#define C2RT_LEAN_MAX_LEVELS 3
#endif
typedef const RenderParams __attribute__((address_space(4))) *KArgs;

/* One tile: optimistically through lean::, and again through exact:: — by the same wave, with all of its
 * lanes — if a lane reported an operand outside a lean window (c2rt_trace.inc).  The instances launched when
 * rays are being counted (CNT; tests/conftest.py renders every counted frame with BOTH instances and insists
 * on the same bits) run exact:: only, so that suite compares the two. */
/* 1: in the instances named below the cold half reads its arguments through a kernarg pointer the optimiser
 * cannot see through, so that nothing but that pointer and the tile index stays live across the lean half on its
 * behalf.  Without it values both halves use (kernel arguments, table pointers) are kept in SGPRs from the top
 * of the kernel and the lean half spills around them: render_kernel_idn<1> holds 254 v_writelane / v_readlane in
 * its lean half without, 191 with (lean:: compiled alone: 184); lecture5.sdl 4K at 1 sample per pixel 0.245 ->
 * 0.239 ms, 1080p 72 -> 71 us, 4K x5 0.999 -> 0.996 ms.  Depth-of-field, plane-only and nested-CSG instances
 * are allocated no better or worse with it (profiles/r04_variants.md, step 12) and keep the plain call. */
#ifndef C2RT_REDO_OPAQUE
#define C2RT_REDO_OPAQUE 1
#endif

template <int LEVELS, int DOF, bool MLC, int PO, bool CNT>
DEV void render_one(const RenderParams &P, KArgs K, const uint32_t b)
{
    if constexpr (CNT || !C2RT_LEAN || LEVELS > C2RT_LEAN_MAX_LEVELS) {
        exact::render_tile<LEVELS, DOF, MLC, PO, CNT>(P, (exact::KArgs)K, b);
    } else {
        if (!P.force_exact) { /* wave-uniform */
            const bool redo = lean::render_tile<LEVELS, DOF, MLC, PO, false>(P, (lean::KArgs)K, b);
            if (!__ballot(redo)) return;
            if (threadIdx.x % kWave == 0) atomicAdd(P.redo_counter, 1ull); /* c2rt_get_exact_redos */
        }
        if constexpr (C2RT_REDO_OPAQUE && LEVELS <= 1 && !DOF && PO != lean::kSpecPlanes) {
            KArgs K2 = K;
            uint32_t b2 = b;
            asm volatile("" : "+s"(K2), "+s"(b2));
            exact::render_tile<LEVELS, DOF, MLC, PO, false>(*(const RenderParams *)K2, (exact::KArgs)K2, b2);
        } else {
            exact::render_tile<LEVELS, DOF, MLC, PO, false>(P, (exact::KArgs)K, b);
        }
    }
}

/* One tile per workgroup; in retry mode (RenderParams::retry_mode: the full-capacity relaunch of
 * the nested-CSG instances) a fixed grid walks the list of tiles whose hit stacks overflowed.
 * Either way the tile code is inlined once. */
template <int LEVELS, int DOF, bool MLC, int PO, bool CNT>
DEV void render_body(const RenderParams &P, KArgs K)
{
    if constexpr (LEVELS >= 2) {
        uint32_t i = blockIdx.x;
        do {
            uint32_t b = i;
            if (P.retry_mode) {
                const uint32_t listed = P.retry_list[0];
                if (i >= (listed < P.retry_max ? listed : P.retry_max)) break;
                b = P.retry_list[1 + i];
            }
            render_one<LEVELS, DOF, MLC, PO, CNT>(P, K, b);
            i += gridDim.x;
        } while (P.retry_mode);
    } else {
        render_one<LEVELS, DOF, MLC, PO, CNT>(P, K, blockIdx.x);
    }
}

template <int LEVELS, int DOF, bool MLC, bool CNT>
__global__ void __launch_bounds__(kBlockThreads) C2RT_OCC_OF(LEVELS, DOF, MLC) render_kernel(const RenderParams P)
{
    render_body<LEVELS, DOF, MLC, 0, CNT>(P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr());
}

/* The same for scenes in which every node's matrix is the identity (RenderParams::all_identity: every scene the
 * reference ships) with at most one light and no depth of field: lean::kSpecIdentity (c2rt_trace.inc) — production
 * instances only; counted frames run the general instance, and the tests compare the two. */
template <int LEVELS>
__global__ void __launch_bounds__(kBlockThreads) C2RT_OCC_OF(LEVELS, 0, false) render_kernel_idn(const RenderParams P)
{
    render_body<LEVELS, 0, false, lean::kSpecIdentity, false>(P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr());
}

/* The depth-of-field / stereo instance carries the lens sampling state on top of
 * the tracer's and has its own register budget (C2RT_OCC_DOF). */
template <int LEVELS, bool MLC, int MODE, bool CNT>
__global__ void __launch_bounds__(kBlockThreads) C2RT_OCC_OF(LEVELS, MODE, MLC) render_kernel_dof(const RenderParams P)
{
    render_body<LEVELS, MODE, MLC, 0, CNT>(P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr());
}

/* Scenes made of axis planes only (RenderParams::planes_only — lecture4.sdl, zaphod.sdl): the
 * instances in which a plane's miss is decided before the ray is normalised (plane_points_away). */
template <int DOF, bool CNT>
__global__ void __launch_bounds__(kBlockThreads) C2RT_OCC_OF(0, DOF, false) render_kernel_planes(const RenderParams P)
{
    render_body<0, DOF, false, lean::kSpecPlanes, CNT>(P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr()); /* at most one light (launch_render_level); planes have no boxes, hence no culling masks */
}
/* (no identity-matrix variant of these: single-plane scenes take the straight-line ground trace, which has no matrix
 * code to lose — measured: zaphod x4 0.601 vs 0.606 ms, DOF 4.583 vs 4.582) */

/* Batch entries (c2rt_render_frames_device): the same trace over a TABLE of parameter blocks in HBM, one per frame,
 * blockIdx.y = frame.  A tile's whole identity is (parameter block, block index): blockIdx.x is what it is in the
 * single-frame launch of that frame (so the tile lands on the same XCD class), and the block is read through a
 * constant-address-space pointer exactly as the single-frame kernels re-read their kernel-argument segment — scalar
 * loads, no VGPR.  The pointer goes through an empty asm so that the optimiser cannot fold the address-space casts
 * back to the global pointer it was made from (loads through that one would be vector loads: the kernel stores to
 * global memory, so nothing proves them invariant).  Only the instances a batch can reach: no counting, no depth of
 * field.  Register budget, scratch and occupancy equal the single-frame twins' (profiles/frame_batch.md). */
DEV KArgs batch_block(const RenderParams *table)
{
    KArgs K = (KArgs)table + blockIdx.y;
    asm volatile("" : "+s"(K));
    return K;
}

template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kBlockThreads) C2RT_OCC_OF(LEVELS, 0, MLC) render_kernel_batch(const RenderParams *table)
{
    const KArgs K = batch_block(table);
    render_body<LEVELS, 0, MLC, 0, false>(*(const RenderParams *)K, K);
}

template <int LEVELS>
__global__ void __launch_bounds__(kBlockThreads) C2RT_OCC_OF(LEVELS, 0, false) render_kernel_idn_batch(const RenderParams *table)
{
    const KArgs K = batch_block(table);
    render_body<LEVELS, 0, false, lean::kSpecIdentity, false>(*(const RenderParams *)K, K);
}

#if C2RT_UNIT == 0 /* (not a template: it would be compiled into every unit) */
__global__ void __launch_bounds__(kBlockThreads) C2RT_OCC_OF(0, 0, false) render_kernel_planes_batch(const RenderParams *table)
{
    const KArgs K = batch_block(table);
    render_body<0, 0, false, lean::kSpecPlanes, false>(*(const RenderParams *)K, K);
}
#endif

/* renderPixel — rt/renderer.d:46-57: one lane, one sample, full trace result */
template <int LEVELS, int DOF>
__global__ void __launch_bounds__(kWave) probe_kernel(const RenderParams P)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    if (threadIdx.x != 0) return;
    Ctx cx;
    cx.geoms = (GeomP)P.geoms;
    cx.nodes = (NodeP)P.nodes;
    cx.n_nodes = P.n_nodes;
    cx.kargs = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    cx.lds = lds;
    cx.lane = 0;
    cx.csg_cap = (int)P.csg_cap;
    cx.overflow = false;
    oob_init(cx.bad);
    cx.trunc_counter = nullptr;
#if C2RT_TILE_STATS
    cx.lane_stats = nullptr;
#endif
    cx.block = 0;
    cx.mask_slot = 0;
    cx.primary_mask = 0xFFFFFFFFu;
    cx.shadow_mask0 = 0xFFFFFFFFu;
    cx.shadow_ground_only = false;
    cx.primary_ground_only = false;
    cx.ground_y = 0;
    Counters cnt = {0, 0};
    const uint64_t pixel = (uint64_t)P.probe_y * P.width + (uint64_t)P.probe_x;
    const F3 c = render_sample<LEVELS, DOF, true, false>(P, cx, (double)P.probe_x, (double)P.probe_y, 1, 1, pixel, 0, cnt, P.probe_out); /* MLC: any number of lights (n_cull = 0: no masks) */
    P.probe_out->color[0] = c.r;
    P.probe_out->color[1] = c.g;
    P.probe_out->color[2] = c.b;
}

#if C2RT_UNIT == 5
/* Rank-major strip buffers, each `rows_pad` rows (what a gather of equal-sized
 * per-rank buffers leaves on rank 0) -> full frame.  blockIdx.y
 * = frame row; float4 copies when a row is a multiple of 16 B. */
__global__ void deinterleave_kernel(const float *__restrict__ gathered, float *__restrict__ frame,
                                    uint32_t row_floats, uint32_t strip_height, uint32_t world, uint32_t rows_pad)
{
    const uint32_t y = blockIdx.y;
    const uint32_t strip = y / strip_height;
    const uint32_t rank = strip % world;
    const uint32_t lr = (strip / world) * strip_height + y % strip_height;
    const float *src = gathered + ((size_t)rank * rows_pad + lr) * (size_t)row_floats;
    float *dst = frame + (size_t)y * row_floats;
    if ((row_floats & 3u) == 0) {
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < row_floats / 4; i += gridDim.x * blockDim.x) d4[i] = s4[i];
    } else {
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < row_floats; i += gridDim.x * blockDim.x) dst[i] = src[i];
    }
}

/* Color.toRGB32 via convertTo8bit_sRGB_Cached — rt/color.d:154-162,209-214 */
__global__ void encode_rgb32_kernel(const float *__restrict__ frame, uint32_t *__restrict__ out, uint64_t n,
                                    const uint8_t *__restrict__ lut)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t ch[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = frame[3 * i + c];
            ch[c] = !(x > 0) ? 0u : (x >= 1 ? 255u : (uint32_t)lut[(int)(x * 4096.0f)]);
        }
        out[i] = ch[2] | (ch[1] << 8) | (ch[0] << 16);
    }
}

/* The culling masks of every tile of a frame's local rows, one lane per tile (c2rt_trace.inc: tile_mask_entry,
 * tile_mask_slot).  Runs once per frame whose camera leaves culling rectangles, in front of the frame kernel's
 * launch(es), on the same stream.  One body for both entry points below, which only produce (P, K, V, S, table,
 * tile_rows). */
DEV void tile_masks_body(const RenderParams &P, KArgs K, const VoidCull &V, const SphereCull &S, uint32_t *table, uint32_t tile_rows)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t cols = P.blocks_x * kWavesPerBlock;
    const uint32_t trow = i / cols, tcol = i % cols;
    if (trow >= tile_rows) return;
    uint32_t m[8];
    exact::tile_mask_entry(P, (exact::KArgs)K, V, S, trow, tcol, m);
    typedef uint32_t __attribute__((ext_vector_type(4))) u4_t;
    u4_t v, w;
    v.x = m[0]; v.y = m[1]; v.z = m[2]; v.w = m[3];
    w.x = m[4]; w.y = m[5]; w.z = m[6]; w.w = m[7];
    const size_t slot = exact::tile_mask_slot(P, trow, tcol);
    reinterpret_cast<u4_t *>(table)[slot] = v;
    if (P.n_cull_lights > 1u) reinterpret_cast<u4_t *>(table)[(size_t)P.mask_entries + slot] = w; /* lights 1..3 */
}

static_assert(sizeof(RenderParams) + sizeof(VoidCull) + sizeof(SphereCull) + 16 <= 4096, "the kernel-argument segment holds at most 4 KiB");
__global__ void __launch_bounds__(256) tile_masks_kernel(const RenderParams P, const VoidCull V, const SphereCull S,
                                                         uint32_t *__restrict__ table, uint32_t tile_rows)
{
    tile_masks_body(P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), V, S, table, tile_rows);
}

/* The same for every frame of a batch in one launch: blockIdx.y = frame; the frame's RenderParams and its VoidCull /
 * SphereCull come from the tables (scalar loads, as from the kernel-argument segment above), its mask table from its
 * own RenderParams::tile_masks.  Frames without culling rectangles have no table and return at once. */
__global__ void __launch_bounds__(256) tile_masks_batch_kernel(const RenderParams *table, const BatchCull *culls)
{
    const KArgs K = batch_block(table);
    const BatchCull C2RT_K *C = (const BatchCull C2RT_K *)culls + blockIdx.y;
    asm volatile("" : "+s"(C));
    const RenderParams &P = *(const RenderParams *)K;
    if (!P.n_cull || !P.tile_masks) return;
    const BatchCull &B = *(const BatchCull *)C;
    tile_masks_body(P, K, B.v, B.s, const_cast<uint32_t *>(P.tile_masks), (P.mask_rows + kTileH - 1) / kTileH);
}
#endif /* C2RT_UNIT == 5 */

} // namespace

/*
 * Instantiation is split over translation units so that the (slow) device
 * compiles run in parallel: the Makefile builds this file once per
 * C2RT_UNIT = 0..4 (the frame kernel for that many CSG nesting levels) and
 * once with C2RT_UNIT = 5 (probe, de-interleave, encode, dispatcher), once
 * with C2RT_UNIT = 6 (the ray and visibility queries, c2rt_trace_rays) and once
 * with C2RT_UNIT = 7 (the hit planes of a camera frame, c2rt_render_hits) and once
 * with C2RT_UNIT = 8 (adaptive anti-aliasing, c2rt_render_frame_adaptive).
 */
#ifndef C2RT_UNIT
#error "compile with -DC2RT_UNIT=0..8 (see Makefile)"
#endif

#if C2RT_UNIT >= 0 && C2RT_UNIT <= C2RT_MAX_CSG_DEPTH

/* launch geometry of a frame kernel, single frame or batch: the grid's x extent (retry mode: a fixed grid walks the
 * overflow list, render_body) and the LDS of the hit stacks */
static uint32_t frame_grid_x(const RenderParams &p)
{
#if C2RT_XCD_SWIZZLE
    const uint32_t tiles_y_pad = (p.tiles_y + 7u) / 8u * 8u;
#else
    const uint32_t tiles_y_pad = p.tiles_y;
#endif
    return p.retry_mode ? 2048u : p.blocks_x * tiles_y_pad;
}
static size_t frame_lds(const RenderParams &p) { return (size_t)p.csg_cap * kCsgLdsPerEntry * kWavesPerBlock; }

template <>
int launch_render_level<C2RT_UNIT>(const RenderParams &p, bool dof_or_stereo, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(frame_grid_x(p)), block(kBlockThreads);
    const size_t lds = frame_lds(p);
    const bool stereo = p.cam.stereo_separation != 0;
    const bool multi = p.n_lights > 1;
    /* identity matrices throughout and not a counted frame: the instances specialised for that */
    const bool idn = p.all_identity && !p.ray_counters;
#define C2RT_LAUNCH(KERNEL, ...)                                                                        \
    do {                                                                                                \
        if (p.ray_counters) hipLaunchKernelGGL((KERNEL<__VA_ARGS__, true>), grid, block, lds, s, p);    \
        else hipLaunchKernelGGL((KERNEL<__VA_ARGS__, false>), grid, block, lds, s, p);                  \
    } while (0)
#if C2RT_UNIT == 0
    if (p.planes_only && !multi) { /* (planes + several lights: the general instances below) */
        if (dof_or_stereo && stereo) C2RT_LAUNCH(render_kernel_planes, 2);
        else if (dof_or_stereo) C2RT_LAUNCH(render_kernel_planes, 1);
        else C2RT_LAUNCH(render_kernel_planes, 0);
        return (int)hipGetLastError();
    }
#endif
    if (dof_or_stereo) {
        /* stereo cameras are rare: one instance (any number of lights) */
        if (stereo) C2RT_LAUNCH(render_kernel_dof, C2RT_UNIT, true, 2);
        else if (multi) C2RT_LAUNCH(render_kernel_dof, C2RT_UNIT, true, 1);
        else C2RT_LAUNCH(render_kernel_dof, C2RT_UNIT, false, 1);
    } else if (multi) {
        C2RT_LAUNCH(render_kernel, C2RT_UNIT, 0, true);
    } else if (idn) {
        hipLaunchKernelGGL((render_kernel_idn<C2RT_UNIT>), grid, block, lds, s, p);
    } else {
        C2RT_LAUNCH(render_kernel, C2RT_UNIT, 0, false);
    }
#undef C2RT_LAUNCH
    return (int)hipGetLastError();
}

/* One launch for the frames of a batch: p0 = any frame's block (host copy; the grid, the stack size and the instance
 * are the same for all of them: one scene, one set of options, no depth of field), table_dev = the n_frames blocks in
 * HBM.  The instance is the one launch_render_level picks for an uncounted frame without depth of field. */
template <>
int launch_render_batch_level<C2RT_UNIT>(const RenderParams &p0, const RenderParams *table_dev, uint32_t n_frames, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(frame_grid_x(p0), n_frames), block(kBlockThreads);
    const size_t lds = frame_lds(p0);
#if C2RT_UNIT == 0
    if (p0.planes_only && p0.n_lights <= 1) {
        hipLaunchKernelGGL(render_kernel_planes_batch, grid, block, lds, s, table_dev);
        return (int)hipGetLastError();
    }
#endif
    if (p0.n_lights > 1) hipLaunchKernelGGL((render_kernel_batch<C2RT_UNIT, true>), grid, block, lds, s, table_dev);
    else if (p0.all_identity) hipLaunchKernelGGL((render_kernel_idn_batch<C2RT_UNIT>), grid, block, lds, s, table_dev);
    else hipLaunchKernelGGL((render_kernel_batch<C2RT_UNIT, false>), grid, block, lds, s, table_dev);
    return (int)hipGetLastError();
}

#elif C2RT_UNIT == 5

int launch_render_batch(const RenderParams &p0, const KernelVariant &v, const RenderParams *table_dev, uint32_t n_frames, void *stream)
{
    if (v.dof_or_stereo || p0.ray_counters || !n_frames || n_frames > 65535u) return (int)hipErrorInvalidValue;
    switch (v.csg_levels) {
    case 0: return launch_render_batch_level<0>(p0, table_dev, n_frames, stream);
    case 1: return launch_render_batch_level<1>(p0, table_dev, n_frames, stream);
    case 2: return launch_render_batch_level<2>(p0, table_dev, n_frames, stream);
    case 3: return launch_render_batch_level<3>(p0, table_dev, n_frames, stream);
    case 4: return launch_render_batch_level<4>(p0, table_dev, n_frames, stream);
    default: return (int)hipErrorInvalidValue;
    }
}

int launch_tile_masks_batch(const RenderParams &p0, const RenderParams *table_dev, const BatchCull *culls_dev, uint32_t n_frames, void *stream)
{
    const uint32_t tile_rows = (p0.mask_rows + kTileH - 1) / kTileH;
    const uint32_t lanes = tile_rows * p0.blocks_x * kWavesPerBlock;
    if (!lanes || !n_frames) return 0;
    hipLaunchKernelGGL(tile_masks_batch_kernel, dim3((lanes + 255u) / 256u, n_frames), dim3(256), 0, static_cast<hipStream_t>(stream), table_dev, culls_dev);
    return (int)hipGetLastError();
}

int launch_render(const RenderParams &p, const KernelVariant &v, void *stream)
{
    switch (v.csg_levels) {
    case 0: return launch_render_level<0>(p, v.dof_or_stereo, stream);
    case 1: return launch_render_level<1>(p, v.dof_or_stereo, stream);
    case 2: return launch_render_level<2>(p, v.dof_or_stereo, stream);
    case 3: return launch_render_level<3>(p, v.dof_or_stereo, stream);
    case 4: return launch_render_level<4>(p, v.dof_or_stereo, stream);
    default: return (int)hipErrorInvalidValue;
    }
}

size_t tile_mask_entries(const RenderParams &p)
{
    const uint32_t tile_rows = (p.mask_rows + kTileH - 1) / kTileH;
    return (size_t)((tile_rows + 7u) / 8u * 8u) * p.blocks_x * kWavesPerBlock;
}

int launch_tile_masks(const RenderParams &p, const VoidCull &vc, const SphereCull &sc, uint32_t *table, void *stream)
{
    const uint32_t tile_rows = (p.mask_rows + kTileH - 1) / kTileH;
    const uint32_t lanes = tile_rows * p.blocks_x * kWavesPerBlock;
    if (!lanes) return 0;
    hipLaunchKernelGGL(tile_masks_kernel, dim3((lanes + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream), p, vc, sc, table, tile_rows);
    return (int)hipGetLastError();
}

/* the probe is not a hot path: one instance that handles every scene */
int launch_probe(const RenderParams &p, const KernelVariant &, void *stream)
{
    const size_t lds = (size_t)p.csg_cap * kCsgLdsPerEntry;
    hipLaunchKernelGGL((probe_kernel<C2RT_MAX_CSG_DEPTH, 2>), dim3(1), dim3(kWave), lds,
                       static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

int launch_deinterleave(const float *gathered, float *frame, uint32_t width, uint32_t height,
                        uint32_t strip_height, uint32_t world, uint32_t rows_pad, uint32_t words_per_pixel, void *stream)
{
    const uint32_t row_floats = width * words_per_pixel; /* 3: float RGB, 1: packed RGB32 */
    const uint32_t per_row = (row_floats & 3u) == 0 ? row_floats / 4 : row_floats;
    const dim3 block(256), grid((per_row + 255) / 256 > 16 ? 16 : (per_row + 255) / 256, height);
    hipLaunchKernelGGL(deinterleave_kernel, grid, block, 0, static_cast<hipStream_t>(stream), gathered, frame,
                       row_floats, strip_height, world, rows_pad);
    return (int)hipGetLastError();
}

int launch_encode_rgb32(const float *frame, uint32_t *out, uint64_t n_pixels, const uint8_t *lut_dev, void *stream)
{
    const uint64_t blocks = (n_pixels + 255) / 256;
    const dim3 block(256), grid((uint32_t)(blocks > 4096 ? 4096 : (blocks ? blocks : 1)));
    hipLaunchKernelGGL(encode_rgb32_kernel, grid, block, 0, static_cast<hipStream_t>(stream), frame, out, n_pixels,
                       lut_dev);
    return (int)hipGetLastError();
}

#elif C2RT_UNIT == 6 || C2RT_UNIT == 7 || C2RT_UNIT == 8 /* the query units: what they share, then one of them */

/*
 * Ray and visibility queries (c2rt_trace_rays*, c2rt_test_visibility*): the caller's rays instead of a camera's.
 * One ray per lane, 64 consecutive rays per wavefront, one wavefront per workgroup — the frame kernels' shape with
 * the tile replaced by a run of the caller's array, so the trace below it is the same wave-synchronous code: scalar
 * node loop, scalar record loads, one surface pass per distinct closest node.  exact:: arithmetic only (the probe's
 * choice; bit-equal to what the frames compute), every culling mask all ones, no ground-tile shortcut.
 *
 * Lanes past n (the tail wave) are masked out by ordinary control flow BEFORE the trace, as the frame kernels mask the
 * lanes past the frame's edge: __all / __ballot / readfirstlane below only ever see live lanes, so a dead lane can
 * neither store nor steer a wave-uniform decision.  A lane holding garbage (NaN, zero direction, 1e300) is live and
 * goes through the same bounded loops as a frame's lane does; what it computes stays in its own registers.
 *
 * CSG hit stack: kCsgFullCap(LEVELS) entries in one launch — it cannot overflow, so there is no retry list and no
 * per-stream scratch.  That is 10 / 20 / 30 / 40 KiB of LDS per wave at depth 1 / 2 / 3 / 4: the LDS, not the
 * registers, bounds the occupancy of the nested instances (8 / 5 / 4 workgroups per CU), hence two waves per SIMD as
 * their register budget ("Ray queries").
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
namespace {

constexpr int kHitWords = (int)(sizeof(c2rt_ray_hit) / 8);
static_assert(sizeof(c2rt_ray) == 48 && sizeof(c2rt_segment) == 48 && sizeof(c2rt_ray_hit) == 80 && kHitWords * 8 == sizeof(c2rt_ray_hit), "ABI layout of the query records");
static_assert(__builtin_offsetof(c2rt_ray_hit, leaf_geom) == 4 && __builtin_offsetof(c2rt_ray_hit, dist) == 8 &&
              __builtin_offsetof(c2rt_ray_hit, p) == 32 && __builtin_offsetof(c2rt_ray_hit, normal) == 56, "ABI layout of c2rt_ray_hit");
static_assert(sizeof(RenderParams) + 64 <= 4096, "the kernel-argument segment holds at most 4 KiB");

template <int LEVELS, bool MLC>
constexpr int occ_query() { return LEVELS >= 2 ? 2 : occ_of<LEVELS, 0, MLC>(); }
#define C2RT_OCC_QUERY(L, M) __attribute__((amdgpu_waves_per_eu(occ_query<L, M>(), occ_query<L, M>())))

DEV void query_ctx(exact::Ctx &cx, const RenderParams &P, exact::KArgs K, char *lds, int lane)
{
    cx.geoms = (exact::GeomP)P.geoms;
    cx.nodes = (exact::NodeP)P.nodes;
    cx.n_nodes = P.n_nodes;
    cx.kargs = K;
    cx.lds = lds;
    cx.lane = lane;
    cx.csg_cap = (int)P.csg_cap;
    cx.overflow = false;
    exact::oob_init(cx.bad);
    cx.trunc_counter = nullptr;
#if C2RT_TILE_STATS
    cx.lane_stats = nullptr;
#endif
    cx.block = 0;
    cx.mask_slot = 0;
    cx.primary_mask = 0xFFFFFFFFu;
    cx.shadow_mask0 = 0xFFFFFFFFu;
    cx.shadow_ground_only = false;
    cx.primary_ground_only = false;
    cx.ground_y = 0;
}

} // namespace

#if C2RT_UNIT == 6
namespace {

/* six doubles of an array-of-structures input record (c2rt_ray, c2rt_segment): three 16-byte loads where the
 * hardware takes them at 8-byte alignment */
typedef double __attribute__((ext_vector_type(2), aligned(8))) d2_t;
DEV void load6(const void *rec, exact::D3 &a, exact::D3 &b)
{
    const d2_t *q = static_cast<const d2_t *>(rec);
    const d2_t q0 = q[0], q1 = q[1], q2 = q[2];
    a = exact::mk(q0.x, q0.y, q1.x);
    b = exact::mk(q1.y, q2.x, q2.y);
}

/* Ray i = trace(ray, TraceType.Ray), rt/renderer.d:325-376, depth 0.  hits / rgb: nullable, not both (wave-uniform). */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_OCC_QUERY(LEVELS, MLC)
trace_rays_kernel(const RenderParams P, const c2rt_ray *__restrict__ rays, const uint64_t n, c2rt_ray_hit *__restrict__ hits, float *__restrict__ rgb)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * kWave; /* < n: the grid is ceil(n / 64) */
    const uint64_t i = first + (uint64_t)lane;
    const bool live = i < n;
    Ctx cx;
    query_ctx(cx, P, (exact::KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    D3 o = mk(0, 0, 0), d = mk(0, 0, 0);
    Hit best;
    Surf surf;
    Mat mat;
    int closest = -1;
    unsigned long long *stage = reinterpret_cast<unsigned long long *>(lds); /* [64][kHitWords] */
    if (live) {
        load6(rays + i, o, d);
        closest = trace_closest<LEVELS>(cx, o, d, hits != nullptr, best, surf, mat);
        if (hits) {
            unsigned long long *rec = stage + lane * kHitWords;
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
        F3 c = mkf(0, 0, 0); /* Environment.getEnvironment — rt/environment.d:7-10 */
        uint32_t shadow_rays = 0;
        if (closest >= 0) c = shade<LEVELS, MLC, 0>(P, cx, mat, d, surf, shadow_rays);
        typedef float __attribute__((ext_vector_type(3), aligned(4))) f3_t;
        f3_t v3;
        v3.x = c.r;
        v3.y = c.g;
        v3.z = c.b;
        *reinterpret_cast<f3_t *>(rgb + i * 3) = v3;
    }
}

/* Segment i = Scene.testVisibility(from, to), rt/scene.d:62-78: full node mask, no ground shortcut */
template <int LEVELS>
__global__ void __launch_bounds__(kWave) C2RT_OCC_QUERY(LEVELS, false)
test_visibility_kernel(const RenderParams P, const c2rt_segment *__restrict__ seg, const uint64_t n, uint8_t *__restrict__ visible)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * kWave + (uint64_t)lane;
    if (i >= n) return; /* nothing after the trace needs the whole wave */
    Ctx cx;
    query_ctx(cx, P, (exact::KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    D3 from, to;
    load6(seg + i, from, to);
    const bool vis = test_visibility<LEVELS, 0>(cx, from, to, 0xFFFFFFFFu, false);
    visible[i] = vis ? (uint8_t)1 : (uint8_t)0;
}

template <int LEVELS>
int launch_trace_rays_level(const RenderParams &p, const c2rt_ray *rays, uint64_t n, c2rt_ray_hit *hits, float *rgb, hipStream_t s)
{
    const dim3 grid((uint32_t)((n + kWave - 1) / kWave)), block(kWave);
    const size_t stack = (size_t)p.csg_cap * kCsgLdsPerEntry, stage = hits ? (size_t)kWave * sizeof(c2rt_ray_hit) : 0;
    const size_t lds = stack > stage ? stack : stage;
    if (p.n_lights > 1) hipLaunchKernelGGL((trace_rays_kernel<LEVELS, true>), grid, block, lds, s, p, rays, n, hits, rgb);
    else hipLaunchKernelGGL((trace_rays_kernel<LEVELS, false>), grid, block, lds, s, p, rays, n, hits, rgb);
    return (int)hipGetLastError();
}

template <int LEVELS>
int launch_test_visibility_level(const RenderParams &p, const c2rt_segment *seg, uint64_t n, uint8_t *visible, hipStream_t s)
{
    const dim3 grid((uint32_t)((n + kWave - 1) / kWave)), block(kWave);
    hipLaunchKernelGGL((test_visibility_kernel<LEVELS>), grid, block, (size_t)p.csg_cap * kCsgLdsPerEntry, s, p, seg, n, visible);
    return (int)hipGetLastError();
}

} // namespace

/* the instance of the scene's CSG depth, as the frame kernels are chosen at upload; p.csg_cap = kCsgFullCap(levels) */
int launch_trace_rays(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, c2rt_ray_hit *hits, float *rgb, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!n || n > C2RT_MAX_RAYS || (!hits && !rgb)) return (int)hipErrorInvalidValue;
    switch (csg_levels) {
    case 0: return launch_trace_rays_level<0>(p, rays, n, hits, rgb, s);
    case 1: return launch_trace_rays_level<1>(p, rays, n, hits, rgb, s);
    case 2: return launch_trace_rays_level<2>(p, rays, n, hits, rgb, s);
    case 3: return launch_trace_rays_level<3>(p, rays, n, hits, rgb, s);
    case 4: return launch_trace_rays_level<4>(p, rays, n, hits, rgb, s);
    default: return (int)hipErrorInvalidValue;
    }
}

int launch_test_visibility(const RenderParams &p, int csg_levels, const c2rt_segment *seg, uint64_t n, uint8_t *visible, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!n || n > C2RT_MAX_RAYS) return (int)hipErrorInvalidValue;
    switch (csg_levels) {
    case 0: return launch_test_visibility_level<0>(p, seg, n, visible, s);
    case 1: return launch_test_visibility_level<1>(p, seg, n, visible, s);
    case 2: return launch_test_visibility_level<2>(p, seg, n, visible, s);
    case 3: return launch_test_visibility_level<3>(p, seg, n, visible, s);
    case 4: return launch_test_visibility_level<4>(p, seg, n, visible, s);
    default: return (int)hipErrorInvalidValue;
    }
}

#elif C2RT_UNIT == 7

/*
 * Hit planes (c2rt_render_hits*): the closest-hit record of the ray through the integer corner of every pixel of a
 * camera frame, one plane per field.  The query kernel above with the caller's ray array replaced by the camera: the
 * lane builds its own screen ray (screen_ray<false>, normalized — the operations the frame kernels and the probe
 * apply to (x, y)), so nothing is read but the scene, and only the planes asked for are written.  exact:: arithmetic,
 * every culling mask all ones, full-capacity hit stack, one wavefront per workgroup, no scratch.
 *
 * Pixel -> lane (C2RT_HIT_MAP; the output does not depend on it): 0 = a run of 64 pixels of one row — every store
 * instruction of a scalar plane covers 256 / 512 contiguous bytes; 1 = the frames' 8x8 tile (kept); 2 = 16x4.
 * lecture5.sdl 1080p, all seven planes / node + dist / all but rgb: 117.9 / 62.6 / 65.3 us for the run, 112.8 / 60.1 /
 * 62.0 for the 8x8 tile, 112.5 / 59.9 / 62.1 for 16x4 (profiles/hit_planes.md): coherent rays and fewer distinct
 * closest nodes per wave are worth more than the wider stores.  Lanes past the right or bottom edge are masked out by
 * control flow before the trace, as the query kernel masks its tail.
 *
 * Stores (C2RT_HIT_ROWSTORE): 0 = each lane stores its own values, the three-component planes as three 8-byte stores
 * at a 24-byte stride (kept); 1 = uv / p / normal are staged in the dead hit stack and written as rows, lane l storing
 * words l, l + 64, ... of each tile row's contiguous run (the query kernel's record store) — SLOWER here, 67.2
 * against 62.0 us for all but rgb (8x8), 70.1 against 65.3 (run of 64): a plane's values of a tile row are already
 * adjacent lanes' and the L2 merges the partial lines, so the LDS round trip and the two barriers per plane buy
 * nothing.  All plain vector stores.
 *
 * The planes and the row window of a host chunk are kernel arguments of their own behind the parameter block:
 * RenderParams is the frame kernels' and does not change.  `out` points at row `row0` of the (compact) planes.
 */
#ifndef C2RT_HIT_MAP
#define C2RT_HIT_MAP 1
#endif
#ifndef C2RT_HIT_ROWSTORE
#define C2RT_HIT_ROWSTORE 0
#endif
namespace {

constexpr int kHitTileW = C2RT_HIT_MAP == 0 ? 64 : (C2RT_HIT_MAP == 1 ? 8 : 16), kHitTileH = kWave / kHitTileW;
constexpr size_t kHitStageBytes = C2RT_HIT_ROWSTORE ? (size_t)kWave * 3 * 8 : 0;
static_assert(sizeof(RenderParams) + sizeof(c2rt_hit_planes) + 16 <= 4096, "the kernel-argument segment holds at most 4 KiB");
static_assert(sizeof(c2rt_hit_planes) == 56, "ABI layout of c2rt_hit_planes");

/* one C-component plane of doubles, as rows: the wave's tile is kHitTileH runs of kHitTileW * C contiguous words.
 * Every lane of the wave takes part, live or not; words of dead pixels are not stored (they were never staged). */
template <int C>
DEV void store_rows(double *plane, unsigned long long *stage, int lane, bool live, const double (&v)[C],
                    uint32_t width, uint32_t rows, uint32_t x0, uint32_t r0)
{
    if (live) {
#pragma unroll
        for (int k = 0; k < C; ++k) stage[lane * C + k] = (unsigned long long)__double_as_longlong(v[k]);
    }
    __builtin_amdgcn_wave_barrier(); /* LDS operations of one wave complete in order; the workgroup is this wave */
    unsigned long long *out = reinterpret_cast<unsigned long long *>(plane);
    constexpr uint32_t run = (uint32_t)kHitTileW * C;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const uint32_t w = (uint32_t)lane + (uint32_t)(k * kWave);
        const uint32_t tr = w / run, c = w % run;
        const uint32_t r = r0 + tr, col = x0 * C + c;
        if (r < rows && col < width * C) out[(size_t)r * width * C + col] = stage[w];
    }
    __builtin_amdgcn_wave_barrier(); /* the next plane, then the shadow rays, reuse the stack */
}

template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_OCC_QUERY(LEVELS, MLC)
hit_planes_kernel(const RenderParams P, const c2rt_hit_planes out, const uint32_t row0, const uint32_t rows, const uint32_t tiles_x)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const uint32_t trow = blockIdx.x / tiles_x, tcol = blockIdx.x % tiles_x; /* the grid is tiles_x * ceil(rows / kHitTileH) */
    const uint32_t x0 = tcol * kHitTileW, r0 = trow * kHitTileH;
    const uint32_t x = x0 + (uint32_t)(lane % kHitTileW);
    const uint32_t r = r0 + (uint32_t)(lane / kHitTileW); /* row within this launch */
    const bool live = x < P.width && r < rows;
    const bool record = out.dist || out.uv || out.p || out.normal; /* wave-uniform: best.dist and the surface are read */
    Ctx cx;
    query_ctx(cx, P, (exact::KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    D3 d = mk(0, 0, 0);
    Hit best;
    Surf surf;
    Mat mat;
    int closest = -1;
    const size_t idx = (size_t)r * P.width + x;
    if (live) {
        /* local row -> frame row under interleaved strips, as render_tile maps it */
        const uint32_t lr = r + row0;
        uint32_t y = lr;
        if (P.strip_world > 1) {
            const uint32_t sh = P.strip_height;
            y = ((lr / sh) * P.strip_world + P.strip_rank) * sh + lr % sh;
        }
        Rng rng = {0u, 0, 0};
        D3 o, raw;
        screen_ray<false>(cx.bad, P, (double)x, (double)y, 0, rng, o, raw);
        d = normalized(cx.bad, raw); /* raytrace(): rt/camera.d:144-147 */
        closest = trace_closest<LEVELS>(cx, o, d, record, best, surf, mat);
        if (out.node) out.node[idx] = closest;
        if (out.leaf) out.leaf[idx] = closest >= 0 ? best.g : -1;
        if (out.dist) out.dist[idx] = best.dist;
#if !C2RT_HIT_ROWSTORE
        if (out.uv) {
            typedef double __attribute__((ext_vector_type(2), aligned(8))) d2_t;
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
#endif
    }
#if C2RT_HIT_ROWSTORE
    {
        unsigned long long *stage = reinterpret_cast<unsigned long long *>(lds); /* [64][3] */
        if (out.uv) {
            const double v[2] = {surf.u, surf.v};
            store_rows<2>(out.uv, stage, lane, live, v, P.width, rows, x0, r0);
        }
        if (out.p) {
            const double v[3] = {surf.p.x, surf.p.y, surf.p.z};
            store_rows<3>(out.p, stage, lane, live, v, P.width, rows, x0, r0);
        }
        if (out.normal) {
            const double v[3] = {surf.n.x, surf.n.y, surf.n.z};
            store_rows<3>(out.normal, stage, lane, live, v, P.width, rows, x0, r0);
        }
    }
#endif
    if (live && out.rgb) {
        F3 c = mkf(0, 0, 0); /* Environment.getEnvironment — rt/environment.d:7-10 */
        uint32_t shadow_rays = 0;
        if (closest >= 0) c = shade<LEVELS, MLC, 0>(P, cx, mat, d, surf, shadow_rays);
        typedef float __attribute__((ext_vector_type(3), aligned(4))) f3_t;
        f3_t v3;
        v3.x = c.r;
        v3.y = c.g;
        v3.z = c.b;
        *reinterpret_cast<f3_t *>(out.rgb + idx * 3) = v3;
    }
}

template <int LEVELS>
int launch_hit_planes_level(const RenderParams &p, const c2rt_hit_planes &out, uint32_t row0, uint32_t rows, hipStream_t s)
{
    const uint32_t tiles_x = (p.width + kHitTileW - 1) / kHitTileW, tiles_y = (rows + kHitTileH - 1) / kHitTileH;
    const dim3 grid(tiles_x * tiles_y), block(kWave); /* at most 2^16 x 2^16 pixels / 64 */
    const size_t stack = (size_t)p.csg_cap * kCsgLdsPerEntry;
    const size_t lds = stack > kHitStageBytes ? stack : kHitStageBytes;
    if (p.n_lights > 1) hipLaunchKernelGGL((hit_planes_kernel<LEVELS, true>), grid, block, lds, s, p, out, row0, rows, tiles_x);
    else hipLaunchKernelGGL((hit_planes_kernel<LEVELS, false>), grid, block, lds, s, p, out, row0, rows, tiles_x);
    return (int)hipGetLastError();
}

} // namespace

/* Rows [row0, row0 + rows) of the local rows of the frame `p` describes (frame_params with the query settings on top:
 * force_exact, csg_cap = kCsgFullCap(csg_levels), no culling, no ground node) into planes whose first row is row0;
 * device pointers, at least one of them non-null, rows > 0.  Declared in c2rt_api.cpp: c2rt_device.h is the frame
 * units' and stays as it is. */
int launch_hit_planes(const RenderParams &p, int csg_levels, const c2rt_hit_planes &out, uint32_t row0, uint32_t rows, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!rows || !p.width || !(out.node || out.leaf || out.dist || out.uv || out.p || out.normal || out.rgb)) return (int)hipErrorInvalidValue;
    switch (csg_levels) {
    case 0: return launch_hit_planes_level<0>(p, out, row0, rows, s);
    case 1: return launch_hit_planes_level<1>(p, out, row0, rows, s);
    case 2: return launch_hit_planes_level<2>(p, out, row0, rows, s);
    case 3: return launch_hit_planes_level<3>(p, out, row0, rows, s);
    case 4: return launch_hit_planes_level<4>(p, out, row0, rows, s);
    default: return (int)hipErrorInvalidValue;
    }
}

#else /* C2RT_UNIT == 8 */

/*
 * Adaptive anti-aliasing (c2rt_render_frame_adaptive*): Renderer.renderRT's three passes with the third one run where
 * the second raised its flag, which is what rt/renderer.d:150-188 computes the flag for and then does not do.  The
 * one-tap frame is the frame kernels' (c2rt_api.cpp calls the frame path with taps = 1); this unit holds the two
 * kernels behind it on the same stream.
 *
 * aa_detect_kernel — rt/renderer.d:154-177 with tooDifferent (rt/color.d:18-23): one lane per pixel over 8x8 tiles,
 * fifteen floats in (the pixel and its four neighbours, clamped at the frame's edges as the reference clamps them), one
 * byte out.  fp32 in the reference's order, no fma (the build has contraction off).  Memory-bound: 12 B read and 1 B
 * written per pixel from HBM, the neighbours come out of the caches.
 *
 * aa_refine_kernel — renderPixelAA (rt/renderer.d:233-251) for the flagged pixels: the hit-plane kernel's wave (one
 * wavefront per workgroup, one 8x8 tile, exact:: arithmetic, every culling mask all ones, full-capacity hit stack, no
 * ground shortcut) with the work items of the tile PACKED into lanes.  A tile with k flagged pixels has 4k items
 * (pixel j, tap 1 + i % 4); lane l of round r takes item 64 r + l, so a tile with up to 16 flagged pixels — an edge
 * crossing it — is ONE round of the trace at 4k / 64 occupancy instead of four rounds at k / 64.  The list of flagged
 * lanes is built in LDS from the ballot's prefix count; each item leaves its colour in an LDS array [pixel][tap] (3 KiB,
 * behind the hit stack), and the pixel's own lane then adds the four to out[y][x] in tap order and divides by 5.0f:
 * render_tile's statements (c2rt_trace.inc), hence the bits of the C2RT_TAPS_REF5 frame.  Lanes without an item are
 * masked out by control flow before the trace, as the query kernel masks its tail.  All plain vector stores.
 *
 * Detection is a launch of its own: it reads the neighbours' ONE-TAP values, and refinement overwrites pixels in
 * place; the caller's mask is the buffer between the two.  Refinement reads and writes its own pixel and the mask only.
 *
 * C2RT_AA_PACKED = 0 builds the plain variant instead: every flagged lane loops over its four taps, the others sit out
 * (A/B: profiles/adaptive_aa.md).
 */
#ifndef C2RT_AA_PACKED
#define C2RT_AA_PACKED 1
#endif
namespace {

static_assert(sizeof(RenderParams) + 64 <= 4096, "the kernel-argument segment holds at most 4 KiB");
static_assert(kTileW * kTileH == kWave, "one wavefront, one tile");
constexpr int kAaDetectWaves = 4; /* tiles (wavefronts) per workgroup of the detection kernel */

__global__ void __launch_bounds__(kWave * kAaDetectWaves)
aa_detect_kernel(const float *__restrict__ frame, uint8_t *__restrict__ needs_aa, const uint32_t width, const uint32_t height,
                 const uint32_t tiles_x, const uint32_t n_tiles, const float threshold)
{
    const uint32_t tile = blockIdx.x * kAaDetectWaves + threadIdx.x / kWave;
    if (tile >= n_tiles) return;
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t x = (tile % tiles_x) * kTileW + lane % kTileW, y = (tile / tiles_x) * kTileH + lane / kTileW;
    if (x >= width || y >= height) return;
    const uint32_t xs[5] = {x, x > 0 ? x - 1 : x, x + 1 < width ? x + 1 : x, x, x};
    const uint32_t ys[5] = {y, y, y, y > 0 ? y - 1 : y, y + 1 < height ? y + 1 : y};
    float n[5][3];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const float *q = frame + ((size_t)ys[i] * width + xs[i]) * 3;
        n[i][0] = q[0];
        n[i][1] = q[1];
        n[i][2] = q[2];
    }
    bool flag = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float average = 0.0f; /* Color average = Color(0, 0, 0); foreach: average += neighs[i] */
#pragma unroll
        for (int i = 0; i < 5; ++i) average = average + n[i][c];
        average = average / 5.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i) flag = flag | (fabsf(n[i][c] - average) > threshold); /* a NaN compares false */
    }
    needs_aa[(size_t)y * width + x] = flag ? (uint8_t)1 : (uint8_t)0;
}

constexpr size_t kAaColourBytes = (size_t)kWave * 4 * 3 * sizeof(float), kAaListBytes = kWave;

template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_OCC_QUERY(LEVELS, MLC)
aa_refine_kernel(const RenderParams P, float *__restrict__ frame, const uint8_t *__restrict__ needs_aa, const uint32_t tiles_x)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const uint32_t x0 = (blockIdx.x % tiles_x) * kTileW, y0 = (blockIdx.x / tiles_x) * kTileH; /* the grid is tiles_x * tiles_y */
    const uint32_t x = x0 + (uint32_t)(lane % kTileW), y = y0 + (uint32_t)(lane / kTileW);
    const size_t idx = (size_t)y * P.width + x;
    const bool flagged = x < P.width && y < P.height && needs_aa[idx] != 0;
    const unsigned long long flags = __ballot(flagged);
    if (!flags) return;
    const size_t stack = (size_t)P.csg_cap * kCsgLdsPerEntry;
    float *colour = reinterpret_cast<float *>(lds + stack); /* [pixel's lane][tap - 1][3] */
    Ctx cx;
    query_ctx(cx, P, (exact::KArgs)__builtin_amdgcn_kernarg_segment_ptr(), lds, lane);
    Rng rng = {0u, 0, 0};
#if C2RT_AA_PACKED
    uint8_t *list = reinterpret_cast<uint8_t *>(lds + stack + kAaColourBytes); /* the flagged lanes, ascending */
    if (flagged) list[__popcll(flags & ((1ull << lane) - 1ull))] = (uint8_t)lane;
    __builtin_amdgcn_wave_barrier(); /* LDS operations of one wave complete in order; the workgroup is this wave */
    const int items = 4 * __popcll(flags);
#pragma unroll 1
    for (int first = 0; first < items; first += kWave) {
        const int i = first + lane;
        if (i < items) {
            const int pl = (int)list[i >> 2], t = 1 + (i & 3);
            const uint32_t px = x0 + (uint32_t)(pl % kTileW), py = y0 + (uint32_t)(pl / kTileW);
            D3 o, raw;
            screen_ray<false>(cx.bad, P, (double)px + k_aa_x[t], (double)py + k_aa_y[t], 0, rng, o, raw);
            const D3 d = normalized(cx.bad, raw); /* raytrace(): rt/camera.d:144-147 */
            Hit best;
            Surf surf;
            Mat mat;
            const int closest = trace_closest<LEVELS>(cx, o, d, false, best, surf, mat);
            F3 c = mkf(0, 0, 0); /* Environment.getEnvironment — rt/environment.d:7-10 */
            uint32_t shadow_rays = 0;
            if (closest >= 0) c = shade<LEVELS, MLC, 0>(P, cx, mat, d, surf, shadow_rays);
            float *slot = colour + (pl * 4 + (t - 1)) * 3;
            slot[0] = c.r;
            slot[1] = c.g;
            slot[2] = c.b;
        }
    }
    __builtin_amdgcn_wave_barrier();
#else
    if (flagged) {
#pragma unroll 1
        for (int t = 1; t <= 4; ++t) {
            D3 o, raw;
            screen_ray<false>(cx.bad, P, (double)x + k_aa_x[t], (double)y + k_aa_y[t], 0, rng, o, raw);
            const D3 d = normalized(cx.bad, raw);
            Hit best;
            Surf surf;
            Mat mat;
            const int closest = trace_closest<LEVELS>(cx, o, d, false, best, surf, mat);
            F3 c = mkf(0, 0, 0);
            uint32_t shadow_rays = 0;
            if (closest >= 0) c = shade<LEVELS, MLC, 0>(P, cx, mat, d, surf, shadow_rays);
            float *slot = colour + (lane * 4 + (t - 1)) * 3;
            slot[0] = c.r;
            slot[1] = c.g;
            slot[2] = c.b;
        }
    }
#endif
    if (flagged) {
        /* renderPixelAA: accum = the pixel's one-tap colour, += the four samples in tap order, / 5 — Color / float */
        typedef float __attribute__((ext_vector_type(3), aligned(4))) f3_t;
        f3_t *out = reinterpret_cast<f3_t *>(frame + idx * 3);
        const f3_t v0 = *out;
        F3 accum = mkf(v0.x, v0.y, v0.z);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float *slot = colour + (lane * 4 + t) * 3;
            accum = accum + mkf(slot[0], slot[1], slot[2]);
        }
        accum = accum / 5.0f;
        f3_t v3;
        v3.x = accum.r;
        v3.y = accum.g;
        v3.z = accum.b;
        *out = v3;
    }
}

template <int LEVELS>
int launch_aa_refine_level(const RenderParams &p, float *frame, const uint8_t *needs_aa, hipStream_t s)
{
    const uint32_t tiles_x = (p.width + kTileW - 1) / kTileW, tiles_y = (p.height + kTileH - 1) / kTileH;
    const dim3 grid(tiles_x * tiles_y), block(kWave); /* at most 2^16 x 2^16 pixels / 64 */
    const size_t lds = (size_t)p.csg_cap * kCsgLdsPerEntry + kAaColourBytes + kAaListBytes;
    if (p.n_lights > 1) hipLaunchKernelGGL((aa_refine_kernel<LEVELS, true>), grid, block, lds, s, p, frame, needs_aa, tiles_x);
    else hipLaunchKernelGGL((aa_refine_kernel<LEVELS, false>), grid, block, lds, s, p, frame, needs_aa, tiles_x);
    return (int)hipGetLastError();
}

} // namespace

/* needs_aa[y][x] of the whole width x height frame at `frame` (device pointers).  Declared in c2rt_api.cpp, as
 * launch_hit_planes is. */
int launch_aa_detect(const float *frame, uint8_t *needs_aa, uint32_t width, uint32_t height, float threshold, void *stream)
{
    if (!width || !height || !frame || !needs_aa) return (int)hipErrorInvalidValue;
    const uint32_t tiles_x = (width + kTileW - 1) / kTileW, n_tiles = tiles_x * ((height + kTileH - 1) / kTileH);
    hipLaunchKernelGGL(aa_detect_kernel, dim3((n_tiles + kAaDetectWaves - 1) / kAaDetectWaves), dim3(kWave * kAaDetectWaves), 0,
                       static_cast<hipStream_t>(stream), frame, needs_aa, width, height, tiles_x, n_tiles, threshold);
    return (int)hipGetLastError();
}

/* The flagged pixels of the whole frame `p` describes (hit_params' settings: exact::, csg_cap = kCsgFullCap(csg_levels),
 * no culling, no ground node; no strips) from their one-tap to their five-tap value, in place. */
int launch_aa_refine(const RenderParams &p, int csg_levels, float *frame, const uint8_t *needs_aa, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!p.width || !p.height || !frame || !needs_aa) return (int)hipErrorInvalidValue;
    switch (csg_levels) {
    case 0: return launch_aa_refine_level<0>(p, frame, needs_aa, s);
    case 1: return launch_aa_refine_level<1>(p, frame, needs_aa, s);
    case 2: return launch_aa_refine_level<2>(p, frame, needs_aa, s);
    case 3: return launch_aa_refine_level<3>(p, frame, needs_aa, s);
    case 4: return launch_aa_refine_level<4>(p, frame, needs_aa, s);
    default: return (int)hipErrorInvalidValue;
    }
}

#endif /* C2RT_UNIT == 6 / 7 / 8 */

#else
#error "C2RT_UNIT out of range"
#endif

} // namespace c2rt
