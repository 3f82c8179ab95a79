/*
 * c2rt_temporal.hip — temporal accumulation of a Monte-Carlo plane: every pixel's world point is projected into the
 * previous camera, the previous frame's accumulated value is fetched there where the surface is the same one, and the new
 * sample is folded into a running mean (c2rt_temporal_accumulate*; the arithmetic is the contract in include/c2rt.h,
 * restated in numpy by tests/temporal_reference.py).  Like the filter it traces nothing: a gather in fp32 behind a short
 * fp64 chain whose cost is memory traffic.
 *
 * temporal_kernel — one lane per pixel.  The lane converts its guides to fp32 (they are the first two words of the history
 * it writes), reprojects its point (three fp64 dots, two divides), and reads up to four taps of the previous history: a
 * tap's first guide word is one 16-byte load; its second word, colour and moments are loaded behind the node test and the
 * normal test, together, so that the plane test waits for one round trip and not two.  The four taps are unrolled in the
 * contract's order.  The packed guides leave as two float4 stores.
 *
 * Lane mapping: a wavefront owns 64 consecutive pixels in row order, so that every plane it reads and writes is one run of
 * memory.  Measured against a wavefront per 8x8 tile, whose taps share more cache lines but whose streams break into eight
 * pieces: profiles/temporal.md, DESIGN.md 4.24.  The tile took 43 % longer and is gone.
 *
 * Built with the project's arithmetic flags: no contraction, IEEE divide, no libm call.  All plain vector stores.
 */
#include <hip/hip_runtime.h>

#include "c2rt_temporal.h"

namespace c2rt {
namespace {

constexpr int kLanes = 256; /* lanes per workgroup */

struct TemporalArgs {
    const int32_t *node; /* the current frame's guides */
    const double *normal, *p;
    const float *in;
    const float4 *h0, *h1; /* the previous history (h0 null: none) */
    const float *hc, *hm;
    float4 *o0, *o1;       /* the history out */
    float *oc, *om;
    float *colour, *variance; /* the planes, each nullable */
    uint32_t *age;
    TemporalCamera cam;
    uint32_t width, height, max_age;
    float min_normal_dot, max_plane_dist;
};

template <int CH>
__global__ void __launch_bounds__(kLanes)
temporal_kernel(const TemporalArgs a)
{
    const size_t q = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (q >= (size_t)a.width * a.height) return;
    const int nd = a.node[q];
    const double *n = a.normal + q * 3, *r = a.p + q * 3;
    const double p0 = r[0], p1 = r[1], p2 = r[2];
    const float nx = (float)n[0], ny = (float)n[1], nz = (float)n[2];
    const float px = (float)p0, py = (float)p1, pz = (float)p2;
    float in[CH], col[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) col[c] = in[c] = a.in[q * CH + c];
    float M1 = 0.0f, M2 = 0.0f, var = 0.0f;
    uint32_t age = 0;
    if (nd >= 0) {
        float lum;
        if constexpr (CH == 3) lum = (0.2126f * in[0] + 0.7152f * in[1]) + 0.0722f * in[2];
        else lum = in[0];
        const float lum2 = lum * lum;
        M1 = lum; /* no history, until the taps say otherwise */
        M2 = lum2;
        age = 1;
        if (a.h0) {
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
                    float sumw = 0.0f, sum[CH], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
                    for (int c = 0; c < CH; ++c) sum[c] = 0.0f;
                    uint32_t amin = 0xffffffffu;
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
                            float hc[CH];
#pragma unroll
                            for (int c = 0; c < CH; ++c) hc[c] = a.hc[t * CH + c];
                            const float h1m = a.hm[2 * t], h2m = a.hm[2 * t + 1];
                            const float dx = t1.x - px, dy = t1.y - py, dz = t1.z - pz;
                            const float dp = (nx * dx + ny * dy) + nz * dz;
                            if (!(fabsf(dp) <= a.max_plane_dist)) continue;
                            sumw = sumw + w;
#pragma unroll
                            for (int c = 0; c < CH; ++c) sum[c] = sum[c] + w * hc[c];
                            s1 = s1 + w * h1m;
                            s2 = s2 + w * h2m;
                            const uint32_t hage = __float_as_uint(t1.w);
                            amin = hage < amin ? hage : amin;
                        }
                    }
                    if (sumw > 0.0f) {
                        const float m1 = s1 / sumw, m2 = s2 / sumw;
                        const uint32_t cnt = amin >= a.max_age ? a.max_age : amin + 1u; /* min(amin + 1, max_age), no wrap */
                        const float f = 1.0f / (float)cnt;
#pragma unroll
                        for (int c = 0; c < CH; ++c) {
                            const float h = sum[c] / sumw;
                            col[c] = h + (in[c] - h) * f;
                        }
                        M1 = m1 + (lum - m1) * f;
                        M2 = m2 + (lum2 - m2) * f;
                        const float v = M2 - M1 * M1;
                        var = v > 0.0f ? v : 0.0f;
                        age = cnt;
                    }
                }
            }
        }
    }
    a.o0[q] = make_float4(nx, ny, nz, __int_as_float(nd));
    a.o1[q] = make_float4(px, py, pz, __uint_as_float(age));
#pragma unroll
    for (int c = 0; c < CH; ++c) a.oc[q * CH + c] = col[c];
    a.om[2 * q] = M1;
    a.om[2 * q + 1] = M2;
    if (a.colour) {
#pragma unroll
        for (int c = 0; c < CH; ++c) a.colour[q * CH + c] = col[c];
    }
    if (a.variance) a.variance[q] = var;
    if (a.age) a.age[q] = age;
}

} // namespace

int launch_temporal(const c2rt_temporal_guides &g, const c2rt_temporal_opts &o, const TemporalCamera *cam, const float *in,
                    const void *history_prev, void *history_out, const c2rt_temporal_planes &planes, void *stream)
{
    if (!o.width || !o.height || (o.channels != 1 && o.channels != 3) || !g.node || !g.normal || !g.p || !in || !history_out ||
        (history_prev != nullptr) != (cam != nullptr))
        return (int)hipErrorInvalidValue;
    const size_t px = (size_t)o.width * o.height;
    TemporalArgs a = {};
    a.node = g.node;
    a.normal = g.normal;
    a.p = g.p;
    a.in = in;
    if (history_prev) {
        const char *h = static_cast<const char *>(history_prev);
        a.h0 = reinterpret_cast<const float4 *>(h);
        a.h1 = reinterpret_cast<const float4 *>(h + px * 16);
        a.hc = reinterpret_cast<const float *>(h + px * 32);
        a.hm = reinterpret_cast<const float *>(h + px * (32 + 4 * (size_t)o.channels));
        a.cam = *cam;
    }
    char *h = static_cast<char *>(history_out);
    a.o0 = reinterpret_cast<float4 *>(h);
    a.o1 = reinterpret_cast<float4 *>(h + px * 16);
    a.oc = reinterpret_cast<float *>(h + px * 32);
    a.om = reinterpret_cast<float *>(h + px * (32 + 4 * (size_t)o.channels));
    a.colour = planes.colour;
    a.variance = planes.variance;
    a.age = planes.age;
    a.width = o.width;
    a.height = o.height;
    a.max_age = o.max_age;
    a.min_normal_dot = o.min_normal_dot;
    a.max_plane_dist = o.max_plane_dist;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((uint32_t)((px + kLanes - 1) / kLanes));
    if (o.channels == 3) hipLaunchKernelGGL(temporal_kernel<3>, grid, dim3(kLanes), 0, s, a);
    else hipLaunchKernelGGL(temporal_kernel<1>, grid, dim3(kLanes), 0, s, a);
    return (int)hipGetLastError();
}

} // namespace c2rt
