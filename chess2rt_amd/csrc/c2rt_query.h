/*
 * c2rt_query.h — launch interface of the query kernels (c2rt_rays.hip, c2rt_hit_planes.hip, c2rt_layers.hip, c2rt_shade_planes.hip, c2rt_occlusion.hip, c2rt_gather.hip, c2rt_paths.hip, c2rt_paths_counted.hip (its launches: c2rt_paths_counted.h), c2rt_adaptive.hip, c2rt_sample_taps.hip), shared
 * by those files and c2rt_api.cpp.  A header of its own: c2rt_device.h is a prerequisite of every frame-kernel object,
 * and query work should not rebuild them.  All return hipError_t as int; every pointer is a device pointer.
 *
 * `p` is the frame path's parameter block with the query settings on top (c2rt_api.cpp: query_params / hit_params):
 * force_exact, csg_cap = kCsgFullCap(csg_levels), no culling, no ground node, no scratch.
 */
#ifndef C2RT_QUERY_H
#define C2RT_QUERY_H

#include "c2rt_device.h"
#include <cstring>

namespace c2rt {

/* A plane struct (c2rt_hit_planes, c2rt_shade_planes, c2rt_occlusion_planes, c2rt_gather_planes, c2rt_path_planes) as the host code sees
 * it: nothing but pointers, kPlanes<S> of them (c2rt_api.cpp keeps the sample size of each next to the family's words) */
template <class S> constexpr int kPlanes = 0;
template <> inline constexpr int kPlanes<c2rt_hit_planes> = 7;
template <> inline constexpr int kPlanes<c2rt_shade_planes> = 6;
template <> inline constexpr int kPlanes<c2rt_occlusion_planes> = 4;
template <> inline constexpr int kPlanes<c2rt_gather_planes> = 4;
template <> inline constexpr int kPlanes<c2rt_path_planes> = 5;
static_assert(sizeof(c2rt_hit_planes) == kPlanes<c2rt_hit_planes> * sizeof(void *) &&
              sizeof(c2rt_shade_planes) == kPlanes<c2rt_shade_planes> * sizeof(void *) &&
              sizeof(c2rt_occlusion_planes) == kPlanes<c2rt_occlusion_planes> * sizeof(void *) &&
              sizeof(c2rt_gather_planes) == kPlanes<c2rt_gather_planes> * sizeof(void *) &&
              sizeof(c2rt_path_planes) == kPlanes<c2rt_path_planes> * sizeof(void *), "the plane structs are arrays of pointers");

/* "at least one plane asked for": what the launches below and the entry points of c2rt_api.cpp both refuse without */
template <class S>
inline bool any_plane(const S &o)
{
    const void *plane[kPlanes<S>];
    std::memcpy(plane, &o, sizeof plane);
    for (const void *q : plane)
        if (q) return true;
    return false;
}

/* The plane families launch alike: launch_plane_rows (rows of a camera frame) and launch_plane_rays (a caller's rays,
 * ray i drawing the samples of index base + i) are overloaded on the planes type, the family's options in front of the
 * planes.  NoOpts: the options of a family that has none (the hit and shading planes, which ignore `base` too). */
struct NoOpts {};

/* Ray and visibility queries (c2rt_trace_rays*, c2rt_test_visibility*): no camera; 0 < n <= C2RT_MAX_RAYS; hits / rgb
 * nullable, not both */
int launch_trace_rays(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, c2rt_ray_hit *hits, float *rgb, void *stream);
int launch_test_visibility(const RenderParams &p, int csg_levels, const c2rt_segment *seg, uint64_t n, uint8_t *visible, void *stream);
/* Hit planes (c2rt_render_hits*): rows [row0, row0 + rows) of the local rows of the frame `p` describes, into planes
 * whose first row is row0; at least one plane non-null, rows > 0 */
int launch_plane_rows(const RenderParams &p, int csg_levels, const NoOpts &, const c2rt_hit_planes &out, uint32_t row0, uint32_t rows, void *stream);
/* Hit planes of a batch (c2rt_render_frames_hits*, c2rt_render_frames_posed_hits*): the same rows of the n_frames frames
 * whose blocks are at table_dev (p0: the host copy of one of them), in one launch; frame i's slice of a plane starts
 * i * frame_px * components elements behind the plane's pointer, at row row0 */
int launch_hit_planes_batch(const RenderParams &p0, int csg_levels, const RenderParams *table_dev, uint32_t n_frames, size_t frame_px,
                            const c2rt_hit_planes &out, uint32_t row0, uint32_t rows, void *stream);
/* Hit layers (c2rt_trace_rays_layers*, c2rt_render_hit_layers*; c2rt_layers.hip): the single-hit queries with the walk
 * along the ray around the trace, 1 <= max_layers <= C2RT_MAX_HIT_LAYERS.  Layer k's slice of an output starts
 * k * layer_stride records (k * layer_px pixels) behind its pointer: n (the frame's local_rows * width) for a caller's
 * arrays, the chunk size for a host chunk.  hits / rgb / count (the planes / count): nullable, not all of them. */
int launch_trace_ray_layers(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, uint32_t max_layers, uint64_t layer_stride,
                            c2rt_ray_hit *hits, float *rgb, uint8_t *count, void *stream);
int launch_hit_layers(const RenderParams &p, int csg_levels, const c2rt_hit_planes &out, uint8_t *count, uint32_t max_layers, size_t layer_px,
                      uint32_t row0, uint32_t rows, void *stream);
/* Shading planes (c2rt_render_shading*, c2rt_trace_rays_shading*; c2rt_shade_planes.hip): the hit planes' rows, or the
 * ray query's rays, with the terms of the closest node's shade() one plane each; at least one plane non-null */
int launch_plane_rows(const RenderParams &p, int csg_levels, const NoOpts &, const c2rt_shade_planes &out, uint32_t row0, uint32_t rows, void *stream);
int launch_plane_rays(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, uint64_t base, const NoOpts &, const c2rt_shade_planes &out,
                      void *stream);
/* Occlusion planes (c2rt_render_occlusion*, c2rt_trace_rays_occlusion*; c2rt_occlusion.hip): the hit planes' rows, or the
 * ray query's rays, with occ.samples hemisphere visibility tests behind every hit; at least one plane non-null,
 * 1 <= occ.samples <= C2RT_MAX_OCCLUSION_SAMPLES.  Ray i draws the samples of index base + i (a host chunk's first ray) */
int launch_plane_rows(const RenderParams &p, int csg_levels, const c2rt_occlusion_opts &occ, const c2rt_occlusion_planes &out, uint32_t row0,
                      uint32_t rows, void *stream);
int launch_plane_rays(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, uint64_t base, const c2rt_occlusion_opts &occ,
                      const c2rt_occlusion_planes &out, void *stream);
/* Gather planes (c2rt_render_gather*, c2rt_trace_rays_gather*; c2rt_gather.hip): the hit planes' rows, or the ray query's
 * rays, with g.samples rays spawned over the hemisphere behind every hit, traced and shaded as c2rt_trace_rays' are; at
 * least one plane non-null, 1 <= g.samples <= C2RT_MAX_GATHER_SAMPLES.  Ray i draws the samples of index base + i */
int launch_plane_rows(const RenderParams &p, int csg_levels, const c2rt_gather_opts &g, const c2rt_gather_planes &out, uint32_t row0, uint32_t rows,
                      void *stream);
int launch_plane_rays(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, uint64_t base, const c2rt_gather_opts &g,
                      const c2rt_gather_planes &out, void *stream);
/* Path planes (c2rt_render_paths*, c2rt_trace_rays_paths*; c2rt_paths.hip): the hit planes' rows, or the ray query's rays,
 * with g.paths paths of at most g.bounces segments behind every hit, each segment traced and shaded as c2rt_trace_rays'
 * rays are; at least one plane non-null, 1 <= g.paths <= C2RT_MAX_PATHS, 1 <= g.bounces <= C2RT_MAX_PATH_BOUNCES.  Ray
 * i draws the paths of index base + i */
int launch_plane_rows(const RenderParams &p, int csg_levels, const c2rt_path_opts &g, const c2rt_path_planes &out, uint32_t row0, uint32_t rows,
                      void *stream);
int launch_plane_rays(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, uint64_t base, const c2rt_path_opts &g,
                      const c2rt_path_planes &out, void *stream);
/* Adaptive anti-aliasing (c2rt_render_frame[s]_adaptive*): the flag images needs_aa[i][y][x] of n_frames whole one-tap
 * frames side by side, then the flagged pixels of the whole frame `p` describes (no strips) from their one-tap to their
 * five-tap value, in place; launch_aa_refine_batch: the same for the n_frames frames whose blocks are at table_dev (p0:
 * the host copy of one of them), block i naming frame i as its RenderParams::out, flags side by side at needs_aa */
int launch_aa_detect(const float *frames, uint8_t *needs_aa, uint32_t width, uint32_t height, uint32_t n_frames, float threshold, void *stream);
int launch_aa_refine(const RenderParams &p, int csg_levels, float *frame, const uint8_t *needs_aa, void *stream);
int launch_aa_refine_batch(const RenderParams &p0, int csg_levels, const RenderParams *table_dev, uint32_t n_frames, const uint8_t *needs_aa,
                           void *stream);
/* Sample tables (c2rt_render_frame_taps*, c2rt_render_frame_adaptive_taps*; c2rt_sample_taps.hip): the hit planes' rows
 * with every pixel the average of the table's taps (1 <= taps.n <= C2RT_MAX_SAMPLE_TAPS) into `out`, whose first row is
 * row0; and launch_aa_refine with taps 1 .. taps.n - 1 of the table in the place of the reference's four (taps.n >= 2) */
int launch_frame_taps(const RenderParams &p, int csg_levels, const c2rt_tap_table &taps, float *out, uint32_t row0, uint32_t rows, void *stream);
int launch_aa_refine_taps(const RenderParams &p, int csg_levels, const c2rt_tap_table &taps, float *frame, const uint8_t *needs_aa, void *stream);

} // namespace c2rt
#endif
