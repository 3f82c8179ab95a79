/*
 * c2rt_denoise_variance.h — launch interface of the variance-guided a-trous filter (c2rt_denoise_variance.hip), shared by
 * that file and c2rt_api.cpp.  HIP-free; all launches return hipError_t as int; every pointer is a device pointer.
 */
#ifndef C2RT_DENOISE_VARIANCE_H
#define C2RT_DENOISE_VARIANCE_H

#include "c2rt_denoise.h"

namespace c2rt {

/* Layout of c2rt_denoise_variance_device's scratch for valid options: [packed guides, 32 B per pixel (c2rt_denoise.h) |
 * colour ping-pong plane, 4 * channels B | variance plane A (V0), 4 B | variance plane B, 4 B | g, the 3x3-blurred variance
 * of the level about to run, 4 B].  The guides are there for the levels and for the spatial estimate; the colour plane and
 * plane B for levels > 1; plane A and g for levels > 0. */
inline size_t denoise_variance_guide_bytes(const c2rt_denoise_variance_opts &o)
{
    return o.levels || o.min_age ? (size_t)o.width * o.height * kDenoiseGuideBytes : 0;
}
inline size_t denoise_variance_colour_bytes(const c2rt_denoise_variance_opts &o)
{
    return o.levels > 1 ? (size_t)o.width * o.height * o.channels * sizeof(float) : 0;
}
inline size_t denoise_variance_plane_bytes(const c2rt_denoise_variance_opts &o, int plane)
{
    return o.levels > (uint32_t)plane ? (size_t)o.width * o.height * sizeof(float) : 0;
}
inline size_t denoise_variance_preblur_bytes(const c2rt_denoise_variance_opts &o)
{
    return o.levels ? (size_t)o.width * o.height * sizeof(float) : 0;
}
inline size_t denoise_variance_scratch_bytes(const c2rt_denoise_variance_opts &o)
{
    return denoise_variance_guide_bytes(o) + denoise_variance_colour_bytes(o) + denoise_variance_plane_bytes(o, 0) +
           denoise_variance_plane_bytes(o, 1) + denoise_variance_preblur_bytes(o);
}

/* The whole call on `stream`: the packing launch, stage A and per level the blur of V (sigma_lum > 0) and the level itself
 * (levels == 0: the closing steps alone, behind stage A where variance_out is given).  `o` has passed
 * c2rt_denoise_variance_device's checks; inv_plane and sl2 are the contract's per-call factors. */
int launch_denoise_variance(const c2rt_denoise_guides &g, const c2rt_denoise_variance_opts &o, float inv_plane, float sl2, const float *variance,
                            const uint32_t *age, const float *in, float *out, float *variance_out, void *scratch, void *stream);

} // namespace c2rt
#endif
