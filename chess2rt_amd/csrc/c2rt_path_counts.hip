/*
 * c2rt_path_counts.hip — how many paths each pixel of the NEXT path launch gets, from what the previous history says about
 * the variance at the point the pixel sees now (c2rt_path_counts*; the arithmetic is the contract in include/c2rt.h,
 * restated in numpy by tests/path_counts_reference.py).  It is the first half of temporal_kernel (c2rt_temporal.hip): the
 * reprojection in fp64 and the four-tap gather of (M1, M2, age), statement for statement, without the colour, without the
 * fold and without a history out; beside the moments a tap brings the count its last sample was traced with.  The count
 * rule follows the gather.  It traces nothing and needs no scene.
 *
 * path_counts_kernel — one lane per pixel, 64 consecutive pixels per wave in row order, as temporal_kernel (the 8x8 tile
 * lost there: profiles/temporal.md).  A lane reads 52 bytes of guides, up to four taps of 16 + 16 + 8 (+ 1) bytes, and
 * writes 1 + 4 + 4 bytes: a fraction of the accumulation's traffic.
 *
 * Built with the project's arithmetic flags: no contraction, IEEE divide, no libm call.  All plain vector stores.
 */
#include <hip/hip_runtime.h>

#include "c2rt_paths_counted.h"

namespace c2rt {
namespace {

constexpr int kLanes = 256; /* lanes per workgroup */

struct CountArgs {
    const int32_t *node; /* the current frame's guides */
    const double *normal, *p;
    const float4 *h0, *h1; /* the previous history (h0 null: none) */
    const float *hm;
    const uint8_t *prev_counts; /* nullable */
    uint8_t *counts;
    float *variance; /* nullable */
    uint32_t *age;   /* nullable */
    TemporalCamera cam;
    uint32_t width, height;
    float min_normal_dot, max_plane_dist;
    uint32_t min_paths, max_paths, young_paths, min_age, prev_paths;
    float paths_per_variance;
};

__global__ void __launch_bounds__(kLanes)
path_counts_kernel(const CountArgs a)
{
    const size_t q = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (q >= (size_t)a.width * a.height) return;
    const int nd = a.node[q];
    uint32_t count = 0, age = 0;
    float var = 0.0f;
    if (nd >= 0) {
        count = a.young_paths; /* no history, until the taps say otherwise */
        if (a.h0) {
            const double *n = a.normal + q * 3, *r = a.p + q * 3;
            const double p0 = r[0], p1 = r[1], p2 = r[2];
            const float nx = (float)n[0], ny = (float)n[1], nz = (float)n[2];
            const float px = (float)p0, py = (float)p1, pz = (float)p2;
            const TemporalCamera &k = a.cam;
            const double rx = p0 - k.pos[0], ry = p1 - k.pos[1], rz = p2 - k.pos[2];
            const double ka = (rx * k.na[0] + ry * k.na[1]) + rz * k.na[2];
            const double kb = (rx * k.nb[0] + ry * k.nb[1]) + rz * k.nb[2];
            const double kc = (rx * k.nc[0] + ry * k.nc[1]) + rz * k.nc[2];
            const double s = k.det_positive ? ka : -ka;
            if (s > 0.0) {
                const double sx = (kb / ka) * k.wd, sy = (kc / ka) * k.hd;
                if (sx > -1.0 && sx < k.wd && sy > -1.0 && sy < k.hd) {
                    const double x0d = floor(sx), y0d = floor(sy);
                    const float fx = (float)(sx - x0d), fy = (float)(sy - y0d);
                    const long long x0 = (long long)x0d, y0 = (long long)y0d; /* -1 .. width - 1, -1 .. height - 1 */
                    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
                    float sumw = 0.0f, s1 = 0.0f, s2 = 0.0f;
                    uint32_t amin = 0xffffffffu, cprev = 0;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const long long tx = x0 + i, ty = y0 + j;
                            if (tx < 0 || tx >= (long long)a.width || ty < 0 || ty >= (long long)a.height) continue;
                            const float w = wx[i] * wy[j];
                            if (!(w > 0.0f)) continue;
                            const size_t t = (size_t)ty * a.width + (size_t)tx;
                            const float4 t0 = a.h0[t];
                            if (__float_as_int(t0.w) != nd) continue;
                            const float dn = (nx * t0.x + ny * t0.y) + nz * t0.z;
                            if (!(dn > a.min_normal_dot)) continue;
                            const float4 t1 = a.h1[t];
                            const float h1m = a.hm[2 * t], h2m = a.hm[2 * t + 1];
                            const uint32_t hcount = a.prev_counts ? (uint32_t)a.prev_counts[t] : a.prev_paths;
                            const float dx = t1.x - px, dy = t1.y - py, dz = t1.z - pz;
                            const float dp = (nx * dx + ny * dy) + nz * dz;
                            if (!(fabsf(dp) <= a.max_plane_dist)) continue;
                            sumw = sumw + w;
                            s1 = s1 + w * h1m;
                            s2 = s2 + w * h2m;
                            const uint32_t hage = __float_as_uint(t1.w);
                            amin = hage < amin ? hage : amin;
                            cprev = hcount > cprev ? hcount : cprev;
                        }
                    }
                    if (sumw > 0.0f) {
                        age = amin;
                        if (!(amin < a.min_age)) {
                            if (cprev == 0) cprev = 1;
                            const float m1 = s1 / sumw, m2 = s2 / sumw;
                            const float v = m2 - m1 * m1;
                            var = v <= 0.0f ? 0.0f : v; /* a NaN stays, and takes max_paths below */
                            const float t = (var * (float)cprev) * a.paths_per_variance;
                            if (!(t < (float)a.max_paths)) count = a.max_paths; /* NaN and infinity land here */
                            else {
                                uint32_t c = (uint32_t)t;
                                if ((float)c < t) c += 1;
                                count = c > a.min_paths ? c : a.min_paths;
                            }
                        }
                    }
                }
            }
        }
    }
    a.counts[q] = (uint8_t)count;
    if (a.variance) a.variance[q] = var;
    if (a.age) a.age[q] = age;
}

} // namespace

int launch_path_counts(const c2rt_temporal_guides &g, const c2rt_temporal_opts &o, const c2rt_path_count_opts &pc, const TemporalCamera *cam,
                       const void *history_prev, const uint8_t *prev_counts, uint8_t *counts, float *variance, uint32_t *age, void *stream)
{
    if (!o.width || !o.height || (o.channels != 1 && o.channels != 3) || !g.node || !g.normal || !g.p || !counts || (history_prev != nullptr) != (cam != nullptr))
        return (int)hipErrorInvalidValue;
    const size_t px = (size_t)o.width * o.height;
    CountArgs a = {};
    a.node = g.node;
    a.normal = g.normal;
    a.p = g.p;
    if (history_prev) {
        const char *h = static_cast<const char *>(history_prev);
        a.h0 = reinterpret_cast<const float4 *>(h);
        a.h1 = reinterpret_cast<const float4 *>(h + px * 16);
        a.hm = reinterpret_cast<const float *>(h + px * (32 + 4 * (size_t)o.channels));
        a.cam = *cam;
    }
    a.prev_counts = prev_counts;
    a.counts = counts;
    a.variance = variance;
    a.age = age;
    a.width = o.width;
    a.height = o.height;
    a.min_normal_dot = o.min_normal_dot;
    a.max_plane_dist = o.max_plane_dist;
    a.min_paths = pc.min_paths;
    a.max_paths = pc.max_paths;
    a.young_paths = pc.young_paths;
    a.min_age = pc.min_age;
    a.prev_paths = pc.prev_paths;
    a.paths_per_variance = pc.paths_per_variance;
    hipLaunchKernelGGL(path_counts_kernel, dim3((uint32_t)((px + kLanes - 1) / kLanes)), dim3(kLanes), 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

} // namespace c2rt
