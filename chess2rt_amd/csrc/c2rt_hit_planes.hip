/*
 * c2rt_hit_planes.hip — hit planes (c2rt_render_hits*): the closest-hit record of the ray through the integer corner of
 * every pixel of a camera frame, one plane per field.  The ray query kernel (c2rt_rays.hip) with the caller's ray array
 * replaced by the camera: the lane builds its own screen ray (pixel_ray), so nothing is read but the
 * scene, and only the planes asked for are written.  What it shares with the other query kernels: c2rt_query.inc.
 *
 * Pixel -> lane: the 8x8 tile of c2rt_query.inc (tile_pixel, where the measurement that chose it is told).
 *
 * Stores (store_hit_planes, c2rt_query.inc): each lane stores its own values, the three-component planes as three 8-byte
 * stores at a 24-byte stride.
 * Staging uv / p / normal in the dead hit stack and writing them as rows, lane l storing words l, l + 64, ... of each
 * tile row's contiguous run (the ray query kernel's record store), was SLOWER here — 67.2 against 62.0 us for all but
 * rgb (8x8), 70.1 against 65.3 (run of 64): a plane's values of a tile row are already adjacent lanes' and the L2 merges
 * the partial lines, so the LDS round trip and the two barriers per plane buy nothing.  All plain vector stores.
 * (Both rejected arms were build switches up to commit f0eed4f, c2rt_kernels.hip.)
 *
 * The planes and the row window of a host chunk are kernel arguments of their own behind the parameter block:
 * RenderParams is the frame kernels' and does not change.  `out` points at row `row0` of the (compact) planes.
 *
 * Batches (c2rt_render_frames_hits*, c2rt_render_frames_posed_hits*): hit_planes_batch_kernel is the same wave — one
 * body, hit_planes_body, for both kernels, which only produce (P, K, out) — over a TABLE of parameter blocks in HBM, one
 * per frame, read through a constant-address-space pointer as aa_refine_batch_kernel reads its own (c2rt_adaptive.hip):
 * scalar loads, no VGPR.  blockIdx.y = frame; the frame's slice of a plane starts blockIdx.y * frame_px * components
 * elements behind the plane's pointer (frame_px = local_rows * width: no padding, so with an odd width a slice is
 * aligned to nothing but its element — the 16-byte uv store is declared 8-aligned for the single frame already).  The
 * tiles of every frame share one grid: no launch gap and no grid tail between frames.
 */
#define C2RT_TRACE_EXACT_ONLY
#include "c2rt_trace_common.inc"
#include "c2rt_query.inc"

namespace c2rt {
namespace {

/* The wave over tile blockIdx.x of rows [row0, row0 + rows) of the frame `P` describes: one body for both entry points
 * below, which only produce (P, K, out). */
template <int LEVELS, bool MLC>
DEV void hit_planes_body(const RenderParams &P, KArgs K, const c2rt_hit_planes &out, const uint32_t row0, const uint32_t rows,
                         const uint32_t tiles_x)
{
    using namespace exact;
    extern __shared__ __align__(16) char lds[];
    const int lane = (int)threadIdx.x;
    const TilePixel px = tile_pixel(P, lane, rows, tiles_x);
    const bool record = out.dist || out.uv || out.p || out.normal; /* wave-uniform: best.dist and the surface are read */
    Ctx cx;
    query_ctx(cx, P, K, lds, lane);
    if (px.live) {
        D3 o, d;
        pixel_ray(cx, P, (double)px.x, (double)px.y(P, row0), o, d);
        Hit best;
        Surf surf;
        Mat mat;
        const int closest = trace_closest<LEVELS>(cx, o, d, record, best, surf, mat);
        store_hit_planes<LEVELS, MLC>(P, cx, out, px.idx, closest, best, surf, mat, d);
    }
}

template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_QUERY(LEVELS, MLC)
hit_planes_kernel(const RenderParams P, const c2rt_hit_planes out, const uint32_t row0, const uint32_t rows, const uint32_t tiles_x)
{
    hit_planes_body<LEVELS, MLC>(P, (KArgs)__builtin_amdgcn_kernarg_segment_ptr(), out, row0, rows, tiles_x);
}

/* The same over a batch: blockIdx.y = frame, blockIdx.x = tile of the row window.  `planes` are the batch's: frame
 * blockIdx.y's slice of each starts frame_px * components elements per frame behind it (wave-uniform address
 * arithmetic on kernel arguments: scalar).  A null plane stays null. */
template <int LEVELS, bool MLC>
__global__ void __launch_bounds__(kWave) C2RT_WAVES_QUERY(LEVELS, MLC)
hit_planes_batch_kernel(const RenderParams *table, const c2rt_hit_planes planes, const size_t frame_px, const uint32_t row0,
                        const uint32_t rows, const uint32_t tiles_x)
{
    const KArgs K = batch_block(table);
    const RenderParams &P = *(const RenderParams *)K;
    const size_t first = (size_t)blockIdx.y * frame_px;
    c2rt_hit_planes out;
    out.node = planes.node ? planes.node + first : nullptr;
    out.leaf = planes.leaf ? planes.leaf + first : nullptr;
    out.dist = planes.dist ? planes.dist + first : nullptr;
    out.uv = planes.uv ? planes.uv + first * 2 : nullptr;
    out.p = planes.p ? planes.p + first * 3 : nullptr;
    out.normal = planes.normal ? planes.normal + first * 3 : nullptr;
    out.rgb = planes.rgb ? planes.rgb + first * 3 : nullptr;
    hit_planes_body<LEVELS, MLC>(P, K, out, row0, rows, tiles_x);
}

/* table_dev null: the single-frame kernel with `p` as its argument; otherwise the n_frames blocks at table_dev, of which
 * `p` is any one's host copy (the grid, the stack and the instance are the same for all of them), frame_px pixels from
 * one frame's slice of a plane to the next's */
int launch_planes(const RenderParams &p, int csg_levels, const RenderParams *table_dev, uint32_t n_frames, size_t frame_px,
                  const c2rt_hit_planes &out, uint32_t row0, uint32_t rows, hipStream_t s)
{
    uint32_t tiles_x;
    const dim3 grid = tile_grid(p, rows, tiles_x, n_frames);
    return for_csg_levels(csg_levels, [&](auto L) {
        constexpr int LEVELS = decltype(L)::value;
        if (table_dev)
            return launch_query(p, hit_planes_batch_kernel<LEVELS, true>, hit_planes_batch_kernel<LEVELS, false>, grid, stack_lds(p), s, table_dev, out,
                                frame_px, row0, rows, tiles_x);
        return launch_query(p, hit_planes_kernel<LEVELS, true>, hit_planes_kernel<LEVELS, false>, grid, stack_lds(p), s, p, out, row0, rows, tiles_x);
    });
}

} // namespace

/* Rows [row0, row0 + rows) of the local rows of the frame `p` describes (frame_params with the query settings on top:
 * force_exact, csg_cap = kCsgFullCap(csg_levels), no culling, no ground node) into planes whose first row is row0;
 * device pointers, at least one of them non-null, rows > 0. */
int launch_plane_rows(const RenderParams &p, int csg_levels, const NoOpts &, const c2rt_hit_planes &out, uint32_t row0, uint32_t rows, void *stream)
{
    if (!rows || !p.width || !any_plane(out)) return (int)hipErrorInvalidValue;
    return launch_planes(p, csg_levels, nullptr, 1, 0, out, row0, rows, static_cast<hipStream_t>(stream));
}

/* The same rows of the n_frames frames of a batch in one launch: table_dev holds their blocks (p0: any one's host copy;
 * all share size, strips and light count); `out` holds the frames' slices side by side, frame i's frame_px * components
 * elements behind the plane's pointer, each slice starting at row row0.  No block's RenderParams::out is read. */
int launch_hit_planes_batch(const RenderParams &p0, int csg_levels, const RenderParams *table_dev, uint32_t n_frames, size_t frame_px,
                            const c2rt_hit_planes &out, uint32_t row0, uint32_t rows, void *stream)
{
    if (!rows || !p0.width || !table_dev || !n_frames || n_frames > C2RT_MAX_BATCH_FRAMES || !any_plane(out)) return (int)hipErrorInvalidValue;
    return launch_planes(p0, csg_levels, table_dev, n_frames, frame_px, out, row0, rows, static_cast<hipStream_t>(stream));
}

} // namespace c2rt
