/*
 * c2rt_denoise_variance.hip — the a-trous filter steered by the temporal stage's variance (c2rt_denoise_variance*; the
 * arithmetic is the contract in include/c2rt.h, restated in numpy by tests/denoise_variance_reference.py).  Like
 * c2rt_denoise.hip it traces nothing: fp32 stencils whose cost is memory traffic.
 *
 * variance_pack_kernel, variance_finish_kernel — c2rt_denoise.hip's packing and closing-steps kernels, restated here.  A
 * shared header was tried, included where the kernels stood: c2rt_denoise.o then differs from its earlier self in 213
 * bytes of unchanged size (the compilation-unit id hipcc derives from the source), and that object is to stay byte for
 * byte what it was.  So these 40 lines are kept twice.
 *
 * variance_estimate_kernel — stage A.  A workgroup owns 32 x 8 pixels.  A miss stores +0f and a pixel old enough its
 * temporal variance: one 4-byte load of `node`, one of `age`, one of `variance`.  Where a workgroup holds a young pixel it
 * stages the 38 x 14 pixels around its tile in LDS — packed guides and the luminance of `in`, 36 B each — and the young
 * lanes walk their 7x7 out of LDS; a workgroup without one leaves after the early-out.  The form without LDS, every young
 * lane reading its 49 taps from global memory, was measured and lost in both states: profiles/denoise_variance.md.
 *
 * variance_level_kernel — one level, in the form of c2rt_denoise.hip's level kernel: a workgroup owns kTW x kTH pixels of
 * ONE residue class modulo the step, stages the (kTW + 4) x (kTH + 4) class pixels around them — guides, colour and now
 * the variance, 48 B each with three channels, 34 KiB of LDS — and every lane filters two pixels out of LDS.  The
 * luminance of a tap is computed from the staged colour behind the node and normal tests (staging it as a fourth array
 * was measured and lost).
 *
 * variance_blur_kernel — the 3x3 prefilter of the variance reads ADJACENT pixels, which for a step above 1 are not in the
 * staged class image: one launch ahead of each level blurs V into a plane of its own, one lane per pixel in row order, and
 * the level kernel reads one float per hit pixel.  Nine loads of V inside the level kernel, whose neighbouring lanes are
 * `step` pixels apart, were measured and lost: profiles/denoise_variance.md, DESIGN.md 4.25.
 *
 * Built with the project's arithmetic flags: no contraction, IEEE divide, no libm call.  All plain vector stores.
 */
#include <hip/hip_runtime.h>

#include "c2rt_denoise_variance.h"

namespace c2rt {
namespace {

constexpr int kFlat = 256; /* lanes per workgroup of the per-pixel kernels */
/* a level's tile of one class, the staged neighbourhood around it, lanes per workgroup (two pixels each) */
constexpr int kTW = 32, kTH = 16, kHW = kTW + 4, kHH = kTH + 4, kHalo = kHW * kHH, kClassThreads = 256;

struct VarLevelArgs {
    const float4 *g;     /* packed guides, two per pixel */
    const float *src;    /* C */
    float *dst;          /* D */
    const float *vsrc;   /* V */
    float *vdst;         /* V', nullable: the last level of a call without variance_out */
    const float *gpre;   /* g: the 3x3-blurred V (sigma_lum > 0) */
    const float *albedo; /* the closing steps (last level only), nullable */
    const float *base;
    uint32_t width, height, step, power;
    float inv_plane, sl2, var_floor;
    uint32_t lum;        /* sigma_lum > 0 */
};

struct EstimateArgs {
    const int32_t *node;
    const float4 *g;     /* packed guides; read for young pixels only */
    const float *variance;
    const uint32_t *age; /* null: no spatial estimate */
    const float *in;
    float *v0;
    uint32_t width, height, power, min_age;
    float inv_plane;
};

template <int CH>
__device__ __forceinline__ float lum(const float *c)
{
    if constexpr (CH == 3) return (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2];
    else return c[0];
}

__global__ void __launch_bounds__(kFlat)
variance_pack_kernel(const int32_t *__restrict__ node, const double *__restrict__ normal, const double *__restrict__ p, float4 *__restrict__ g,
                     const size_t px)
{
    const size_t q = (size_t)blockIdx.x * kFlat + threadIdx.x;
    if (q >= px) return;
    const double *n = normal + q * 3, *r = p + q * 3;
    g[2 * q] = make_float4((float)n[0], (float)n[1], (float)n[2], __int_as_float(node[q]));
    g[2 * q + 1] = make_float4((float)r[0], (float)r[1], (float)r[2], 0.0f);
}

/* the two closing steps on the value a pixel is about to store */
template <int CH>
__device__ __forceinline__ void finish(float (&v)[CH], const float *__restrict__ albedo, const float *__restrict__ base, const size_t q)
{
    if (albedo) {
#pragma unroll
        for (int c = 0; c < CH; ++c) v[c] = albedo[q * CH + c] * v[c];
    }
    if (base) {
#pragma unroll
        for (int c = 0; c < CH; ++c) v[c] = base[q * CH + c] + v[c];
    }
}

template <int CH>
__global__ void __launch_bounds__(kFlat)
variance_finish_kernel(const float *__restrict__ in, float *__restrict__ out, const float *__restrict__ albedo, const float *__restrict__ base,
                       const size_t px)
{
    const size_t q = (size_t)blockIdx.x * kFlat + threadIdx.x;
    if (q >= px) return;
    float v[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) v[c] = in[q * CH + c];
    finish<CH>(v, albedo, base, q);
#pragma unroll
    for (int c = 0; c < CH; ++c) out[q * CH + c] = v[c];
}

/* stage A, the neighbourhood in LDS: a workgroup owns kAW x kAH pixels; where one of them is young it stages the
 * (kAW + 6) x (kAH + 6) pixels around them — packed guides and the luminance of `in`, 36 B each, 19 KiB — and its young
 * lanes walk their 49 taps out of LDS.  A workgroup without a young pixel leaves after the three loads of the early-out. */
constexpr int kAW = 32, kAH = 8, kAHW = kAW + 6, kAHH = kAH + 6, kAHalo = kAHW * kAHH;

template <int CH>
__global__ void __launch_bounds__(kFlat)
variance_estimate_kernel(const EstimateArgs a)
{
    __shared__ float4 s0[kAHalo], s1[kAHalo];
    __shared__ float sl[kAHalo];
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * kAW, y0 = (int)blockIdx.y * kAH;
    const int lx = tid % kAW, ly = tid / kAW, x = x0 + lx, y = y0 + ly;
    const bool inside = x < (int)a.width && y < (int)a.height;
    const size_t q = inside ? (size_t)y * a.width + (size_t)x : 0;
    int node = -1;
    uint32_t age = a.min_age;
    bool young = false;
    if (inside) {
        node = a.node[q];
        if (node < 0) {
            a.v0[q] = 0.0f;
        } else {
            if (a.age && a.min_age) age = a.age[q];
            young = age < a.min_age;
            if (!young) a.v0[q] = a.variance[q];
        }
    }
    if (!__syncthreads_or(young ? 1 : 0)) return; /* (uniform) */
    for (int k = tid; k < kAHalo; k += kFlat) {
        const int u = x0 + k % kAHW - 3, v = y0 + k / kAHW - 3;
        if (u >= 0 && u < (int)a.width && v >= 0 && v < (int)a.height) {
            const size_t t = (size_t)v * a.width + (size_t)u;
            s0[k] = a.g[2 * t];
            s1[k] = a.g[2 * t + 1];
            float c[CH];
#pragma unroll
            for (int n = 0; n < CH; ++n) c[n] = a.in[t * CH + n];
            sl[k] = lum<CH>(c);
        } else {
            s0[k] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)); /* never a young pixel's node; s1 and sl are not read behind it */
        }
    }
    __syncthreads();
    if (!young) return;
    const int centre = (ly + 3) * kAHW + lx + 3;
    const float4 q0 = s0[centre], q1 = s1[centre];
    float sumw = 0.0f, m1s = 0.0f, m2s = 0.0f;
#pragma unroll 1
    for (int j = -3; j <= 3; ++j) {
#pragma unroll
        for (int i = -3; i <= 3; ++i) {
            const int k = centre + j * kAHW + i;
            float w = 1.0f;
            if (i != 0 || j != 0) {
                const float4 t0 = s0[k];
                if (__float_as_int(t0.w) != node) continue; /* another node, no node, or outside the frame */
                const float dn = (q0.x * t0.x + q0.y * t0.y) + q0.z * t0.z;
                if (!(dn > 0.0f)) continue;
                float wn = dn;
                for (uint32_t n = 0; n < a.power; ++n) wn = wn * wn;
                const float4 t1 = s1[k];
                const float dx = t1.x - q1.x, dy = t1.y - q1.y, dz = t1.z - q1.z;
                const float dp = (q0.x * dx + q0.y * dy) + q0.z * dz;
                const float e = dp * a.inv_plane;
                const float wp = 1.0f / (1.0f + e * e);
                w = wn * wp;
                if (!(w > 0.0f)) continue;
            }
            const float l = sl[k];
            m1s = m1s + w * l;
            m2s = m2s + w * (l * l);
            sumw = sumw + w;
        }
    }
    const float m1 = m1s / sumw, m2 = m2s / sumw;
    float v = m2 - m1 * m1;
    v = v > 0.0f ? v : 0.0f;
    a.v0[q] = v * ((float)a.min_age / (float)(age > 1u ? age : 1u));
}

/* g of the contract for every pixel: the 3x3 Gaussian of V over ADJACENT pixels, clipped at the frame */
__global__ void __launch_bounds__(kFlat)
variance_blur_kernel(const float *__restrict__ v, float *__restrict__ g, const uint32_t width, const uint32_t height)
{
    constexpr float G[3] = {0.25f, 0.5f, 0.25f}; /* the contract's G[j][i] = G[j] * G[i]: {1/16, 1/8, 1/16; 1/8, 1/4, 1/8; ...}, exact */
    const size_t px = (size_t)width * height, q = (size_t)blockIdx.x * kFlat + threadIdx.x;
    if (q >= px) return;
    const int x = (int)(q % width), y = (int)(q / width);
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            const int tx = x + i, ty = y + j;
            if (tx < 0 || tx >= (int)width || ty < 0 || ty >= (int)height) continue;
            const float gij = G[j + 1] * G[i + 1];
            gs = gs + gij * v[(size_t)ty * width + (size_t)tx];
            gw = gw + gij;
        }
    }
    g[q] = gs / gw;
}

/* The contract's level for one hit pixel out of the staged neighbourhood: s0 / s1 the guide words, sc[c * kHalo + k] the
 * colour, sv[k] the variance, `centre` the pixel's place in them, (x, y) its place in the frame; v: C[q] in, D[q] out;
 * var: V[q] in, V'[q] out. */
template <int CH>
__device__ __forceinline__ void filter_pixel(const VarLevelArgs &a, const float4 *s0, const float4 *s1, const float *sc, const float *sv, const int centre,
                                             const int x, const int y, float (&v)[CH], float &var)
{
    constexpr float K[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float4 q0 = s0[centre], q1 = s1[centre];
    const int node = __float_as_int(q0.w);
    float inv_l = 0.0f, lq = 0.0f;
    if (a.lum) {
        const float g = a.gpre[(size_t)y * a.width + (size_t)x];
        inv_l = 1.0f / (a.sl2 * g + a.var_floor);
        lq = lum<CH>(v);
    }
    float sumw = 0.0f, sumv = 0.0f, sum[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) sum[c] = 0.0f;
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            float w, vt, ct[CH];
            if (i == 0 && j == 0) {
                w = K[2] * K[2];
                vt = var;
#pragma unroll
                for (int c = 0; c < CH; ++c) ct[c] = v[c];
            } else {
                const int k = centre + j * kHW + i;
                const float4 t0 = s0[k];
                if (__float_as_int(t0.w) != node) continue; /* another node, no node, or outside the frame */
                const float dn = (q0.x * t0.x + q0.y * t0.y) + q0.z * t0.z;
                if (!(dn > 0.0f)) continue;
                float wn = dn;
                for (uint32_t n = 0; n < a.power; ++n) wn = wn * wn;
                const float4 t1 = s1[k];
#pragma unroll
                for (int c = 0; c < CH; ++c) ct[c] = sc[c * kHalo + k];
                vt = sv[k];
                const float dx = t1.x - q1.x, dy = t1.y - q1.y, dz = t1.z - q1.z;
                const float dp = (q0.x * dx + q0.y * dy) + q0.z * dz;
                const float e = dp * a.inv_plane;
                const float wp = 1.0f / (1.0f + e * e);
                w = ((K[i + 2] * K[j + 2]) * wn) * wp;
                if (a.lum) {
                    const float dl = lum<CH>(ct) - lq;
                    w = w * (1.0f / (1.0f + (dl * dl) * inv_l));
                }
                if (!(w > 0.0f)) continue;
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) sum[c] = sum[c] + w * ct[c];
            sumw = sumw + w;
            sumv = sumv + (w * w) * vt;
        }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) v[c] = sum[c] / sumw;
    var = sumv / (sumw * sumw);
}

/* blockIdx.z: the class, cy * step + cx; blockIdx.x / .y: the tile of that class's image */
template <int CH, bool LAST>
__global__ void __launch_bounds__(kClassThreads)
variance_level_kernel(const VarLevelArgs a)
{
    __shared__ float4 s0[kHalo], s1[kHalo];
    __shared__ float sc[CH * kHalo]; /* one array per channel: neighbouring lanes, neighbouring banks */
    __shared__ float sv[kHalo];
    const uint32_t s = a.step, cx = blockIdx.z % s, cy = blockIdx.z / s;
    if (cx >= a.width || cy >= a.height) return; /* (uniform) a class without a pixel: the step exceeds the frame */
    const int wc = (int)((a.width - cx + s - 1) / s), hc = (int)((a.height - cy + s - 1) / s);
    const int u0 = (int)blockIdx.x * kTW, v0 = (int)blockIdx.y * kTH;
    if (u0 >= wc || v0 >= hc) return;            /* (uniform) the grid is sized for class (0, 0), the largest */
    const int tid = (int)threadIdx.x;
    for (int k = tid; k < kHalo; k += kClassThreads) {
        const int u = u0 + k % kHW - 2, v = v0 + k / kHW - 2;
        if (u >= 0 && u < wc && v >= 0 && v < hc) { /* hence cx + u s < width, cy + v s < height */
            const size_t t = (size_t)(cy + (uint32_t)v * s) * a.width + (cx + (uint32_t)u * s);
            s0[k] = a.g[2 * t];
            s1[k] = a.g[2 * t + 1];
#pragma unroll
            for (int c = 0; c < CH; ++c) sc[c * kHalo + k] = a.src[t * CH + c];
            sv[k] = a.vsrc[t];
        } else {
            s0[k] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)); /* never a centre; s1, sc and sv are not read behind it */
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        const int lx = tid % kTW, ly = tid / kTW + half * (kTH / 2), u = u0 + lx, v = v0 + ly;
        if (u >= wc || v >= hc) continue;
        const int centre = (ly + 2) * kHW + lx + 2;
        const int x = (int)(cx + (uint32_t)u * s), y = (int)(cy + (uint32_t)v * s);
        const size_t q = (size_t)y * a.width + (size_t)x;
        float val[CH], var = sv[centre];
#pragma unroll
        for (int c = 0; c < CH; ++c) val[c] = sc[c * kHalo + centre];
        if (__float_as_int(s0[centre].w) >= 0) filter_pixel<CH>(a, s0, s1, sc, sv, centre, x, y, val, var);
        if (LAST) finish<CH>(val, a.albedo, a.base, q);
#pragma unroll
        for (int c = 0; c < CH; ++c) a.dst[q * CH + c] = val[c];
        if (a.vdst) a.vdst[q] = var;
    }
}

template <int CH>
void launch_level(const VarLevelArgs &a, bool last, hipStream_t s)
{
    const uint32_t wc = (a.width + a.step - 1) / a.step, hc = (a.height + a.step - 1) / a.step; /* class (0, 0) */
    const dim3 grid((wc + kTW - 1) / kTW, (hc + kTH - 1) / kTH, a.step * a.step), block(kClassThreads);
    if (last) hipLaunchKernelGGL((variance_level_kernel<CH, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((variance_level_kernel<CH, false>), grid, block, 0, s, a);
}

} // namespace

int launch_denoise_variance(const c2rt_denoise_guides &gd, const c2rt_denoise_variance_opts &o, float inv_plane, float sl2, const float *variance,
                            const uint32_t *age, const float *in, float *out, float *variance_out, void *scratch, void *stream)
{
    if (!o.width || !o.height || (o.channels != 1 && o.channels != 3) || o.levels > C2RT_MAX_DENOISE_LEVELS || !in || !out || !variance || !gd.node ||
        !gd.normal || !gd.p || (denoise_variance_scratch_bytes(o) && !scratch))
        return (int)hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t px = (size_t)o.width * o.height;
    const uint32_t flat_blocks = (uint32_t)((px + kFlat - 1) / kFlat);
    const bool spatial = age && o.min_age;
    char *at = static_cast<char *>(scratch);
    float4 *g = reinterpret_cast<float4 *>(at);
    at += denoise_variance_guide_bytes(o);
    float *plane = reinterpret_cast<float *>(at);
    at += denoise_variance_colour_bytes(o);
    float *va = reinterpret_cast<float *>(at);
    at += denoise_variance_plane_bytes(o, 0);
    float *vb = reinterpret_cast<float *>(at);
    at += denoise_variance_plane_bytes(o, 1);
    float *gpre = reinterpret_cast<float *>(at);
    float *v0 = o.levels ? va : variance_out;
    if (o.levels || (v0 && spatial)) {
        hipLaunchKernelGGL(variance_pack_kernel, dim3(flat_blocks), dim3(kFlat), 0, s, gd.node, gd.normal, gd.p, g, px);
        if (const hipError_t e = hipGetLastError()) return (int)e;
    }
    if (v0) {
        EstimateArgs a;
        a.node = gd.node;
        a.g = g;
        a.variance = variance;
        a.age = spatial ? age : nullptr;
        a.in = in;
        a.v0 = v0;
        a.width = o.width;
        a.height = o.height;
        a.power = o.normal_power_log2;
        a.min_age = o.min_age;
        a.inv_plane = inv_plane;
        const dim3 tiles((o.width + kAW - 1) / kAW, (o.height + kAH - 1) / kAH);
        if (o.channels == 3) hipLaunchKernelGGL(variance_estimate_kernel<3>, tiles, dim3(kFlat), 0, s, a);
        else hipLaunchKernelGGL(variance_estimate_kernel<1>, tiles, dim3(kFlat), 0, s, a);
        if (const hipError_t e = hipGetLastError()) return (int)e;
    }
    if (o.levels == 0) {
        if (o.channels == 3) hipLaunchKernelGGL(variance_finish_kernel<3>, dim3(flat_blocks), dim3(kFlat), 0, s, in, out, gd.albedo, gd.base, px);
        else hipLaunchKernelGGL(variance_finish_kernel<1>, dim3(flat_blocks), dim3(kFlat), 0, s, in, out, gd.albedo, gd.base, px);
        return (int)hipGetLastError();
    }
    /* in -> ... -> out as in launch_denoise; V0 in plane A -> B -> A ..., the last level into variance_out (or nowhere) */
    const float *src = in, *vsrc = va;
    for (uint32_t l = 0; l < o.levels; ++l) {
        const bool last = l + 1 == o.levels;
        float *dst = (o.levels - 1 - l) % 2 == 0 ? out : plane;
        float *vdst = last ? variance_out : (l % 2 == 0 ? vb : va);
        VarLevelArgs a;
        a.g = g;
        a.src = src;
        a.dst = dst;
        a.vsrc = vsrc;
        a.vdst = vdst;
        a.gpre = gpre;
        if (o.sigma_lum > 0) {
            hipLaunchKernelGGL(variance_blur_kernel, dim3(flat_blocks), dim3(kFlat), 0, s, vsrc, gpre, o.width, o.height);
            if (const hipError_t e = hipGetLastError()) return (int)e;
        }
        a.albedo = last ? gd.albedo : nullptr;
        a.base = last ? gd.base : nullptr;
        a.width = o.width;
        a.height = o.height;
        a.step = 1u << l;
        a.power = o.normal_power_log2;
        a.inv_plane = inv_plane;
        a.sl2 = sl2;
        a.var_floor = o.var_floor;
        a.lum = o.sigma_lum > 0 ? 1u : 0u;
        if (o.channels == 3) launch_level<3>(a, last, s);
        else launch_level<1>(a, last, s);
        if (const hipError_t e = hipGetLastError()) return (int)e;
        src = dst;
        vsrc = vdst;
    }
    return (int)hipSuccess;
}

} // namespace c2rt
