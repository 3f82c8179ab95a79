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
 * temporal_motion_kernel — the same lane with a list of moved nodes (c2rt_temporal_accumulate_motion*): the up to 16 node
 * indices and their records (R, N, the two offsets: 24 doubles each, composed on the host) are kernel arguments, as the
 * sample tables are.  A lane compares its node with the indices — wave-uniform scalars — and, where one matches, loads
 * that record from the kernel-argument segment (every lane of a node reads the same 192 bytes: one line per load),
 * carries point and normal back through the node's motion and runs the chain on them; the whole block sits behind one
 * branch that a wave with no lane on a moved node does not enter.  A moved lane's two tap tests are the squared ones,
 * chosen per lane.  The records read from a table in device memory instead were measured against this and are gone:
 * profiles/temporal_motion.md, DESIGN.md 4.26.  It is a kernel of its own and not a flag of temporal_kernel's: sharing the
 * pixel as one inlined function changed the operand order of two address adds in temporal_kernel, whose code stays what
 * it was to the instruction.
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

struct TemporalMotionArgs {
    TemporalArgs a;
    TemporalMotion m;
};
static_assert(sizeof(TemporalMotionArgs) <= 4096, "the motion records travel as kernel arguments");

/* temporal_kernel's pixel, statement for statement, with the moved nodes in it: what is new stands behind `moved` */
template <int CH>
__global__ void __launch_bounds__(kLanes)
temporal_motion_kernel(const TemporalMotionArgs ma)
{
    const TemporalArgs &a = ma.a;
    const TemporalMotion *mo = &ma.m;
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
            /* what is reprojected and tested: the pixel's own point and normal, or a moved node's carried back */
            double r0 = p0, r1 = p1, r2 = p2;
            float tnx = nx, tny = ny, tnz = nz, tpx = px, tpy = py, tpz = pz, l2 = 0.0f;
            bool moved = false;
            {
                int m = -1; /* the lane's record; n and the indices are wave-uniform scalars, the list is distinct */
#pragma unroll
                for (int i = 0; i < kMaxMotionNodes; ++i)
                    if ((uint32_t)i < mo->n && (uint32_t)nd == mo->index[i]) m = i;
                if (m >= 0) {
                    const double *w = mo->rec[m]; /* R[9] | N[9] | off_cur[3] | off_prev[3] */
                    const double e0 = p0 - w[18], e1 = p1 - w[19], e2 = p2 - w[20];
                    r0 = ((e0 * w[0] + e1 * w[3]) + e2 * w[6]) + w[21];
                    r1 = ((e0 * w[1] + e1 * w[4]) + e2 * w[7]) + w[22];
                    r2 = ((e0 * w[2] + e1 * w[5]) + e2 * w[8]) + w[23];
                    const double n0 = n[0], n1 = n[1], n2 = n[2];
                    tnx = (float)((n0 * w[9] + n1 * w[12]) + n2 * w[15]);
                    tny = (float)((n0 * w[10] + n1 * w[13]) + n2 * w[16]);
                    tnz = (float)((n0 * w[11] + n1 * w[14]) + n2 * w[17]);
                    tpx = (float)r0;
                    tpy = (float)r1;
                    tpz = (float)r2;
                    l2 = (tnx * tnx + tny * tny) + tnz * tnz;
                    moved = true;
                }
            }
            const float mn2 = a.min_normal_dot * a.min_normal_dot, mp2 = a.max_plane_dist * a.max_plane_dist;
            const double rx = r0 - k.pos[0], ry = r1 - k.pos[1], rz = r2 - k.pos[2];
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
                            const float dn = (tnx * t0.x + tny * t0.y) + tnz * t0.z;
                            if (moved) {
                                if (!(dn > 0.0f && dn * dn > mn2 * l2)) continue;
                            } else if (!(dn > a.min_normal_dot)) continue;
                            const float4 t1 = a.h1[t];
                            float hc[CH];
#pragma unroll
                            for (int c = 0; c < CH; ++c) hc[c] = a.hc[t * CH + c];
                            const float h1m = a.hm[2 * t], h2m = a.hm[2 * t + 1];
                            const float dx = t1.x - tpx, dy = t1.y - tpy, dz = t1.z - tpz;
                            const float dp = (tnx * dx + tny * dy) + tnz * dz;
                            if (moved) {
                                if (!(dp * dp <= mp2 * l2)) continue;
                            } else if (!(fabsf(dp) <= a.max_plane_dist)) continue;
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
                    const void *history_prev, void *history_out, const c2rt_temporal_planes &planes, void *stream, const TemporalMotion *motion)
{
    if (motion && motion->n > (uint32_t)kMaxMotionNodes) return (int)hipErrorInvalidValue;
    if (!o.width || !o.height || (o.channels != 1 && o.channels != 3) || !g.node || !g.normal || !g.p || !in || !history_out ||
        (history_prev != nullptr) != (cam != nullptr))
        return (int)hipErrorInvalidValue;
    const size_t px = (size_t)o.width * o.height;
    TemporalMotionArgs ma = {};
    TemporalArgs &a = ma.a;
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
    if (motion && motion->n && history_prev) { /* without a history nothing is reprojected */
        ma.m = *motion;
        if (o.channels == 3) hipLaunchKernelGGL(temporal_motion_kernel<3>, grid, dim3(kLanes), 0, s, ma);
        else hipLaunchKernelGGL(temporal_motion_kernel<1>, grid, dim3(kLanes), 0, s, ma);
        return (int)hipGetLastError();
    }
    if (o.channels == 3) hipLaunchKernelGGL(temporal_kernel<3>, grid, dim3(kLanes), 0, s, a);
    else hipLaunchKernelGGL(temporal_kernel<1>, grid, dim3(kLanes), 0, s, a);
    return (int)hipGetLastError();
}

} // namespace c2rt
