/*
 * c2rt_temporal.h — launch interface of the temporal accumulation (c2rt_temporal.hip), shared by that file and
 * c2rt_api.cpp.  A header of its own, as c2rt_denoise.h is: the stage traces nothing and needs none of the query
 * headers.  HIP-free; the launch returns hipError_t as int; every pointer is a device pointer.
 */
#ifndef C2RT_TEMPORAL_H
#define C2RT_TEMPORAL_H

#include "../../include/c2rt.h"
#include <cstddef>
#include <cstdint>

namespace c2rt {

/* The history of include/c2rt.h, planar over px = width * height pixels:
 *   [g0: px float4 | g1: px float4 | c: px * channels float | m: px float2], 32 + 4 * channels + 8 bytes per pixel.
 * g0 and g1 are 16-byte aligned with the blob; c and m are only 4-byte aligned (44 px is no multiple of 8 for odd px). */
inline size_t temporal_history_bytes(const c2rt_temporal_opts &o) { return (size_t)o.width * o.height * (32 + 4 * (size_t)o.channels + 8); }

/* The contract's "per call, on the host": what inverts the previous camera's screen ray, computed in fp64 by
 * c2rt_api.cpp (no contraction there either) and passed by value. */
struct TemporalCamera {
    double pos[3], na[3], nb[3], nc[3];
    double wd, hd;
    uint32_t det_positive; /* det > 0 */
};

/* The moved nodes of c2rt_temporal_accumulate_motion, as the kernel takes them: the contract's "per moved node, on the
 * host", composed in fp64 by c2rt_api.cpp and passed by value.  rec[m] = R[9] | N[9] | off_cur[3] | off_prev[3]. */
constexpr int kMaxMotionNodes = C2RT_MAX_MOTION_NODES;
struct TemporalMotion {
    uint32_t n; /* 0 .. kMaxMotionNodes */
    uint32_t index[kMaxMotionNodes];
    double rec[kMaxMotionNodes][24];
};

/* The whole call on `stream`: ONE kernel.  `o` has passed c2rt_temporal_accumulate_device's checks; `cam` and
 * `history_prev` are both null (first frame: every hit pixel restarts) or both given.  `motion` null, empty or without a
 * history: the kernel of the static call. */
int launch_temporal(const c2rt_temporal_guides &g, const c2rt_temporal_opts &o, const TemporalCamera *cam, const float *in,
                    const void *history_prev, void *history_out, const c2rt_temporal_planes &planes, void *stream,
                    const TemporalMotion *motion = nullptr);

} // namespace c2rt
#endif
