/*
 * c2rt_denoise.h — launch interface of the edge-aware a-trous filter (c2rt_denoise.hip), shared by that file and
 * c2rt_api.cpp.  A header of its own, apart from c2rt_query.h: that one is a prerequisite of every query-kernel object, and
 * the filter traces nothing.  HIP-free; all launches return hipError_t as int; every pointer is a device pointer.
 */
#ifndef C2RT_DENOISE_H
#define C2RT_DENOISE_H

#include "../../include/c2rt.h"
#include <cstddef>
#include <cstdint>

namespace c2rt {

/* The guides of one pixel as the level kernels read them: what the contract converts "per pixel, once" (c2rt.h), packed
 * by the first launch of a call.  g0 = (nf.x, nf.y, nf.z, the bits of node), g1 = (pf.x, pf.y, pf.z, 0). */
constexpr size_t kDenoiseGuideBytes = 32;

/* Layout of c2rt_denoise_device's scratch for valid options: [packed guides, 32 B per pixel | ping-pong plane,
 * 4 * channels B per pixel].  No level: nothing.  One level: in -> out, no ping-pong plane. */
inline size_t denoise_guide_bytes(const c2rt_denoise_opts &o) { return o.levels ? (size_t)o.width * o.height * kDenoiseGuideBytes : 0; }
inline size_t denoise_plane_bytes(const c2rt_denoise_opts &o) { return o.levels > 1 ? (size_t)o.width * o.height * o.channels * sizeof(float) : 0; }

/* The whole call on `stream`: the packing launch and one launch per level (levels == 0: one launch of the two closing
 * steps alone), at most levels + 1 kernels.  `o` has passed c2rt_denoise_device's checks; inv_c2[l] is the contract's
 * per-level colour factor (unused with sigma_colour == 0), inv_plane its plane factor. */
int launch_denoise(const c2rt_denoise_guides &g, const c2rt_denoise_opts &o, float inv_plane, const float *inv_c2, const float *in, float *out,
                   void *scratch, void *stream);

} // namespace c2rt
#endif
