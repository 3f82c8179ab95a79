/*
 * c2rt_denoise.hip — edge-aware a-trous filter of a Monte-Carlo plane, guided by the hit planes (c2rt_denoise*; the
 * arithmetic is the contract in include/c2rt.h, restated in numpy by tests/denoise_reference.py).  The first unit of the
 * library that traces nothing: an fp32 stencil of 25 taps per pixel and level whose cost is memory traffic.
 *
 * denoise_pack_kernel — the contract's "per pixel, once": node, normal and p of the hit planes (52 B) to two float4
 * (32 B: nf and the bits of node, pf), one lane per pixel.  Every later read of a guide is one or two 16-byte loads.
 *
 * denoise_level_kernel — one level.  At step s the pixels (cx + u s, cy + v s) of one residue class (cx, cy) modulo s
 * are an image of their own in which the 25 taps are the 5x5 neighbours.  A workgroup owns kTW x kTH pixels of ONE class,
 * stages the (kTW + 4) x (kTH + 4) class pixels around them once — guides and colour, 44 B each with three channels,
 * 31 KiB of LDS — and every lane filters two pixels out of LDS: a pixel is fetched 1.41 times per level, not 25 times.  A
 * pixel outside the frame is staged as node -1, which no centre's node equals.  A tap's second guide word and its colour
 * are read only behind the node test and the normal test.  The 25 taps are unrolled in the contract's order; the kernel
 * weights K[i] * K[j] are compile-time constants.  The last level applies the two closing steps to what it stores.
 *
 * denoise_finish_kernel — levels == 0: the two closing steps alone.
 *
 * Measured against the form that reads every tap from global memory (one lane per pixel, a wavefront = 64 pixels of a row)
 * and against reading the hit planes unpacked at every tap: profiles/denoise.md, DESIGN.md 4.23.  Both lost and are gone.
 *
 * Built with the project's arithmetic flags: no contraction, IEEE divide, no libm call.  All plain vector stores.
 */
#include <hip/hip_runtime.h>

#include "c2rt_denoise.h"

namespace c2rt {
namespace {

constexpr int kFlat = 256; /* lanes per workgroup of the per-pixel kernels */
/* a level's tile of one class, the staged neighbourhood around it, lanes per workgroup (two pixels each) */
constexpr int kTW = 32, kTH = 16, kHW = kTW + 4, kHH = kTH + 4, kHalo = kHW * kHH, kClassThreads = 256;

struct LevelArgs {
    const float4 *g;     /* packed guides, two per pixel */
    const float *src;    /* C */
    float *dst;          /* D */
    const float *albedo; /* the closing steps (last level only), nullable */
    const float *base;
    uint32_t width, height, step, power;
    float inv_plane, inv_c2;
    uint32_t colour;     /* sigma_colour > 0 */
};

__global__ void __launch_bounds__(kFlat)
denoise_pack_kernel(const int32_t *__restrict__ node, const double *__restrict__ normal, const double *__restrict__ p, float4 *__restrict__ g,
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
denoise_finish_kernel(const float *__restrict__ in, float *__restrict__ out, const float *__restrict__ albedo, const float *__restrict__ base,
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

/* The contract's level for one hit pixel out of the staged neighbourhood: s0 / s1 the guide words, sc[c * kHalo + k] the
 * colour, `centre` the pixel's place in them; v: C[q] in, D[q] out. */
template <int CH>
__device__ __forceinline__ void filter_pixel(const LevelArgs &a, const float4 *s0, const float4 *s1, const float *sc, const int centre, float (&v)[CH])
{
    constexpr float K[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float4 q0 = s0[centre], q1 = s1[centre];
    const int node = __float_as_int(q0.w);
    float sumw = 0.0f, sum[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) sum[c] = 0.0f;
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            float w, ct[CH];
            if (i == 0 && j == 0) {
                w = K[2] * K[2];
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
                const float dx = t1.x - q1.x, dy = t1.y - q1.y, dz = t1.z - q1.z;
                const float dp = (q0.x * dx + q0.y * dy) + q0.z * dz;
                const float e = dp * a.inv_plane;
                const float wp = 1.0f / (1.0f + e * e);
                w = ((K[i + 2] * K[j + 2]) * wn) * wp;
                if (a.colour) {
                    float d2 = 0.0f;
                    if constexpr (CH == 3) {
                        const float dr = ct[0] - v[0], dg = ct[1] - v[1], db = ct[2] - v[2];
                        d2 = (dr * dr + dg * dg) + db * db;
                    } else {
                        const float dc = ct[0] - v[0];
                        d2 = dc * dc;
                    }
                    w = w * (1.0f / (1.0f + d2 * a.inv_c2));
                }
                if (!(w > 0.0f)) continue;
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) sum[c] = sum[c] + w * ct[c];
            sumw = sumw + w;
        }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) v[c] = sum[c] / sumw;
}

/* blockIdx.z: the class, cy * step + cx; blockIdx.x / .y: the tile of that class's image */
template <int CH, bool LAST>
__global__ void __launch_bounds__(kClassThreads)
denoise_level_kernel(const LevelArgs a)
{
    __shared__ float4 s0[kHalo], s1[kHalo];
    __shared__ float sc[CH * kHalo]; /* one array per channel: neighbouring lanes, neighbouring banks */
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
        } else {
            s0[k] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)); /* never a centre; s1 and sc are not read behind it */
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        const int lx = tid % kTW, ly = tid / kTW + half * (kTH / 2), u = u0 + lx, v = v0 + ly;
        if (u >= wc || v >= hc) continue;
        const int centre = (ly + 2) * kHW + lx + 2;
        const size_t q = (size_t)(cy + (uint32_t)v * s) * a.width + (cx + (uint32_t)u * s);
        float val[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) val[c] = sc[c * kHalo + centre];
        if (__float_as_int(s0[centre].w) >= 0) filter_pixel<CH>(a, s0, s1, sc, centre, val);
        if (LAST) finish<CH>(val, a.albedo, a.base, q);
#pragma unroll
        for (int c = 0; c < CH; ++c) a.dst[q * CH + c] = val[c];
    }
}

template <int CH>
void launch_level(const LevelArgs &a, bool last, hipStream_t s)
{
    const uint32_t wc = (a.width + a.step - 1) / a.step, hc = (a.height + a.step - 1) / a.step; /* class (0, 0) */
    const dim3 grid((wc + kTW - 1) / kTW, (hc + kTH - 1) / kTH, a.step * a.step), block(kClassThreads);
    if (last) hipLaunchKernelGGL((denoise_level_kernel<CH, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((denoise_level_kernel<CH, false>), grid, block, 0, s, a);
}

} // namespace

int launch_denoise(const c2rt_denoise_guides &gd, const c2rt_denoise_opts &o, float inv_plane, const float *inv_c2, const float *in, float *out,
                   void *scratch, void *stream)
{
    if (!o.width || !o.height || (o.channels != 1 && o.channels != 3) || o.levels > C2RT_MAX_DENOISE_LEVELS || !in || !out ||
        (o.levels && (!scratch || !gd.node || !gd.normal || !gd.p)))
        return (int)hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t px = (size_t)o.width * o.height;
    const uint32_t flat_blocks = (uint32_t)((px + kFlat - 1) / kFlat);
    if (o.levels == 0) {
        if (o.channels == 3) hipLaunchKernelGGL(denoise_finish_kernel<3>, dim3(flat_blocks), dim3(kFlat), 0, s, in, out, gd.albedo, gd.base, px);
        else hipLaunchKernelGGL(denoise_finish_kernel<1>, dim3(flat_blocks), dim3(kFlat), 0, s, in, out, gd.albedo, gd.base, px);
        return (int)hipGetLastError();
    }
    float4 *g = static_cast<float4 *>(scratch);
    float *plane = reinterpret_cast<float *>(static_cast<char *>(scratch) + denoise_guide_bytes(o));
    hipLaunchKernelGGL(denoise_pack_kernel, dim3(flat_blocks), dim3(kFlat), 0, s, gd.node, gd.normal, gd.p, g, px);
    if (const hipError_t e = hipGetLastError()) return (int)e;
    /* in -> ... -> out, alternating between `out` and the ping-pong plane so that the last level stores into `out` */
    const float *src = in;
    for (uint32_t l = 0; l < o.levels; ++l) {
        const bool last = l + 1 == o.levels;
        float *dst = (o.levels - 1 - l) % 2 == 0 ? out : plane;
        LevelArgs a;
        a.g = g;
        a.src = src;
        a.dst = dst;
        a.albedo = last ? gd.albedo : nullptr;
        a.base = last ? gd.base : nullptr;
        a.width = o.width;
        a.height = o.height;
        a.step = 1u << l;
        a.power = o.normal_power_log2;
        a.inv_plane = inv_plane;
        a.inv_c2 = inv_c2[l];
        a.colour = o.sigma_colour > 0 ? 1u : 0u;
        if (o.channels == 3) launch_level<3>(a, last, s);
        else launch_level<1>(a, last, s);
        if (const hipError_t e = hipGetLastError()) return (int)e;
        src = dst;
    }
    return (int)hipSuccess;
}

} // namespace c2rt
