/*
 * c2rt_paths_counted.h — launch interface of the counted path planes (c2rt_paths_counted.hip) and of the count rule that
 * feeds them (c2rt_path_counts.hip), shared by those files and c2rt_api.cpp.  HIP-free; the launches return hipError_t as
 * int; every pointer is a device pointer.
 */
#ifndef C2RT_PATHS_COUNTED_H
#define C2RT_PATHS_COUNTED_H

#include "c2rt_query.h"
#include "c2rt_temporal.h"

namespace c2rt {

/* The scratch of count order: [head: one counter per class, 512 bytes | order: n indices of 32 bits], a multiple of 16 */
constexpr size_t kCountedHeadBytes = 512;
inline size_t counted_scratch_bytes(uint64_t n) { return kCountedHeadBytes + (((size_t)n * 4 + 15u) & ~(size_t)15u); }

/* launch_plane_rows / launch_plane_rays of the path planes (c2rt_query.h) with one count per sample beside the planes:
 * counts[rows][width], first row row0 as the planes', or counts[n].  scratch null: natural order, ONE kernel.  Otherwise
 * counted_scratch_bytes(samples of the launch) bytes, 16-byte aligned: count order — a memset, three sort kernels, then
 * the path kernel; a launch of 2^32 samples or more runs in natural order all the same. */
int launch_counted_rows(const RenderParams &p, int csg_levels, const c2rt_path_opts &g, const uint8_t *counts, const c2rt_path_planes &out, uint32_t row0,
                        uint32_t rows, void *scratch, void *stream);
int launch_counted_rays(const RenderParams &p, int csg_levels, const c2rt_ray *rays, uint64_t n, uint64_t base, const c2rt_path_opts &g,
                        const uint8_t *counts, const c2rt_path_planes &out, void *scratch, void *stream);

/* c2rt_path_counts*: ONE kernel.  `o` and `pc` have passed the entry point's checks; `cam` and `history_prev` are both
 * null (every hit pixel is young) or both given; prev_counts, variance and age nullable. */
int launch_path_counts(const c2rt_temporal_guides &g, const c2rt_temporal_opts &o, const c2rt_path_count_opts &pc, const TemporalCamera *cam,
                       const void *history_prev, const uint8_t *prev_counts, uint8_t *counts, float *variance, uint32_t *age, void *stream);

} // namespace c2rt
#endif
