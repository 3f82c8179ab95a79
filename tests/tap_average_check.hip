/*
 * tap_average_check.hip — device check of the two fp32 pieces lean::ground_tile_certain has of its own
 * (chess2rt_amd/csrc/c2rt_trace_shared.inc) against what they stand in for, ON the device.  Test infrastructure.
 *
 *   tap average:  tap_average(bad, accum, n)  ==  accum / n as the compiler divides (IEEE, correctly rounded), float
 *                 for float, for every channel it lets through — +0 and the positive floats in [2^-60, 2^60) —, and it
 *                 lets through exactly those: `bad` is raised for every other bit pattern (negative, -0, smaller,
 *                 larger, infinite, NaN) and for nothing inside.  N numerators (random bit patterns inside the window,
 *                 structured significands, +0, the window's four edge patterns and their outer neighbours, patterns
 *                 outside it), each over the divisors 2, 3, 4 and 5 (the API's tap counts are 1, 4 and 5; 1 is a no-op);
 *   texel blend:  bitmap_filtered_uniform(pool, offset, w, h, x, y)  ==  bitmap_filtered(pool + offset, w, h, x, y),
 *                 float for float, over N / 4 random texel quads and coordinates — bitmaps of 509 x 251, 800 x 400,
 *                 1 x 1, 2 x 3 and 3 x 2 texels at odd offsets of one pool of random finite floats; coordinates
 *                 anywhere in the bitmap, on and next to integer texels, in the last row and column (both wraps), and
 *                 invalid ones (beyond the bitmap, NaN: the reference's red).
 *
 *   tap_average_check [log2(numerators)]     default 26
 * exit code 0 = all holds.  Prints one JSON line.
 */
#define C2RT_TRACE_EXACT_ONLY
#include "../chess2rt_amd/csrc/c2rt_trace_common.inc"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x)                                                                                      \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; }   \
    } while (0)

namespace c2rt {
namespace {

enum { kAvgInside, kAvgMismatch, kAvgRefusedInside, kAvgOutside, kAvgAcceptedOutside, kAvgZero, kAvgEdge,
       kTexQuads, kTexMismatch, kTexInvalid, kTexWrapX, kTexWrapY, kNCount };
struct Report {
    unsigned long long n[kNCount];
    uint32_t first_avg[2], first_tex[4];
};

__host__ __device__ inline uint64_t mix64(uint64_t z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

constexpr uint32_t kLoBits = (uint32_t)(127 - 60) << 23; /* 2^-60 */
constexpr uint32_t kHiBits = (uint32_t)(127 + 60) << 23; /* 2^60: the first pattern above the window */

/* the window, restated on the float's value: +0, or a positive finite float in [2^-60, 2^60) */
__device__ inline bool admitted(uint32_t bits)
{
    const float x = __uint_as_float(bits);
    return bits == 0u || (x >= 0x1p-60f && x < 0x1p60f);
}

__device__ inline uint32_t numerator(uint64_t h, unsigned long long &zero, unsigned long long &edge)
{
    const unsigned kind = (unsigned)(h & 31);
    const uint32_t r = (uint32_t)(h >> 32);
    const uint32_t inside = kLoBits + r % (kHiBits - kLoBits);
    switch (kind) {
    case 0: zero += 1; return 0u;
    case 1: edge += 1; return kLoBits + ((r & 1) ? 0u : 1u);                     /* the lower edge and its inner neighbour */
    case 2: edge += 1; return kHiBits - 1u - (r & 1);                            /* the last two patterns inside */
    case 3: edge += 1; return (r & 1) ? kLoBits - 1u : kHiBits;                  /* the outer neighbours */
    case 4: return 0x80000000u | ((r & 1) ? 0u : inside);                        /* -0, negative floats of the window's magnitudes */
    case 5: return r;                                                            /* any bit pattern */
    case 6: return (r & 3) == 0 ? 0x7f800000u : ((r & 3) == 1 ? 0x7fc00000u : (r >> 9)); /* inf, NaN, subnormals */
    case 7: return inside & 0xff800000u;                                         /* powers of two */
    case 8: return inside | 0x007fffffu;                                         /* significands of all ones */
    case 9: return (inside & 0xff800000u) | (r & 0xffu);                         /* a few low bits */
    default: return inside;
    }
}

__global__ void average_kernel(Report *rep, uint64_t seed, uint64_t per_thread)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long inside = 0, mismatch = 0, refused = 0, outside = 0, accepted = 0, zero = 0, edge = 0;
    for (uint64_t i = 0; i < per_thread; ++i) {
        const uint64_t key = seed + (t * per_thread + i) * 3;
        const uint32_t a = numerator(mix64(key), zero, edge);
        /* the two other channels are admitted values of their own: the verdict is a's */
        unsigned long long z2 = 0, e2 = 0;
        const uint32_t b1 = kLoBits + (uint32_t)(mix64(key + 1) >> 32) % (kHiBits - kLoBits);
        const uint32_t b2 = (mix64(key + 2) & 1) ? 0u : numerator(mix64(key + 2) | 31u, z2, e2);
#pragma unroll 1
        for (int n = 2; n <= 5; ++n) {
            const float fn = (float)n;
            const int slot = (int)((key + (uint64_t)n) % 3u); /* the channel under test changes place */
            F3 acc = mkf(__uint_as_float(slot == 0 ? a : b1), __uint_as_float(slot == 1 ? a : (slot == 0 ? b1 : b2)),
                         __uint_as_float(slot == 2 ? a : b2));
            const F3 ref = acc / fn; /* the compiler's IEEE division */
            Oob bad;
            oob_init(bad);
            tap_average(bad, acc, fn);
            const float got = slot == 0 ? acc.r : (slot == 1 ? acc.g : acc.b), want = slot == 0 ? ref.r : (slot == 1 ? ref.g : ref.b);
            if (admitted(a)) {
                inside += 1;
                refused += oob_any(bad);
                /* all three channels are admitted here: all three quotients must be the division's */
                const bool same = __float_as_uint(acc.r) == __float_as_uint(ref.r) && __float_as_uint(acc.g) == __float_as_uint(ref.g) &&
                                  __float_as_uint(acc.b) == __float_as_uint(ref.b);
                if (!same) {
                    if (!mismatch++ && !atomicAdd(&rep->n[kAvgMismatch], 0ull)) { rep->first_avg[0] = __float_as_uint(got); rep->first_avg[1] = __float_as_uint(want); }
                }
            } else {
                outside += 1;
                accepted += !oob_any(bad);
            }
        }
    }
    atomicAdd(&rep->n[kAvgInside], inside);
    atomicAdd(&rep->n[kAvgMismatch], mismatch);
    atomicAdd(&rep->n[kAvgRefusedInside], refused);
    atomicAdd(&rep->n[kAvgOutside], outside);
    atomicAdd(&rep->n[kAvgAcceptedOutside], accepted);
    atomicAdd(&rep->n[kAvgZero], zero);
    atomicAdd(&rep->n[kAvgEdge], edge);
}

/* the bitmaps of the blend check: {width, height, first texel}; the pool holds kPoolTexels texels */
constexpr uint32_t kPoolTexels = 1u << 19;
__constant__ uint32_t kShape[5][3] = {{509, 251, 12345}, {800, 400, 200001}, {1, 1, 7}, {2, 3, 11}, {3, 2, 19}};
static_assert(12345 + 509 * 251 <= 200001 && 200001 + 800 * 400 <= (1 << 19) && 19 + 3 * 2 <= 12345, "the bitmaps lie in the pool");

__global__ void texel_kernel(Report *rep, const float *pool, uint64_t seed, uint64_t per_thread)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long quads = 0, mismatch = 0, invalid = 0, wrapx = 0, wrapy = 0;
    for (uint64_t i = 0; i < per_thread; ++i) {
        const uint64_t key = seed + (t * per_thread + i) * 3;
        const uint64_t h = mix64(key);
        /* wave-uniform bitmap, as bitmap_filtered_uniform requires: the same for every thread of a trip */
        const int shape = (int)(i % 5);
        const uint32_t w = kShape[shape][0], hgt = kShape[shape][1], off = kShape[shape][2];
        const float rx = (float)(mix64(key + 1) >> 40) * 0x1p-24f, ry = (float)(mix64(key + 2) >> 40) * 0x1p-24f; /* [0, 1) */
        float x = rx * (float)w, y = ry * (float)hgt; /* as bitmap_color forms them: a float in [0, 1) times the side */
        switch ((unsigned)(h & 15)) {
        case 0: x = floorf(x); break;                                 /* on an integer texel */
        case 1: y = floorf(y); x = nextafterf(floorf(x) + 1.0f, 0.0f); break; /* just below the next one */
        case 2: x = (float)(w - 1) + rx; break;                       /* the last column: tx + 1 wraps */
        case 3: y = (float)(hgt - 1) + ry; break;                     /* the last row: ty + 1 wraps */
        case 4: x = (float)(w - 1) + rx; y = (float)(hgt - 1) + ry; break;
        case 5: x = (float)w; break;                                  /* invalid: red */
        case 6: y = (float)hgt + ry; break;
        case 7: x = (h >> 8) & 1 ? __uint_as_float(0x7fc00000u) : x; y = (h >> 8) & 1 ? y : __uint_as_float(0x7fc00000u); break;
        default: break;
        }
        const bool valid = x < (float)w && y < (float)hgt;
        const F3 a = bitmap_filtered_uniform(pool, off, w, hgt, x, y);
        const F3 b = bitmap_filtered(reinterpret_cast<const float4 *>(pool) + off, w, hgt, x, y);
        quads += 1;
        invalid += !valid;
        wrapx += valid && (uint32_t)floorf(x) + 1 == w;
        wrapy += valid && (uint32_t)floorf(y) + 1 == hgt;
        const bool same = __float_as_uint(a.r) == __float_as_uint(b.r) && __float_as_uint(a.g) == __float_as_uint(b.g) &&
                          __float_as_uint(a.b) == __float_as_uint(b.b);
        if (!same) {
            if (!mismatch++ && !atomicAdd(&rep->n[kTexMismatch], 0ull)) {
                rep->first_tex[0] = (uint32_t)shape; rep->first_tex[1] = __float_as_uint(x); rep->first_tex[2] = __float_as_uint(y);
                rep->first_tex[3] = __float_as_uint(a.r) ^ __float_as_uint(b.r);
            }
        }
    }
    atomicAdd(&rep->n[kTexQuads], quads);
    atomicAdd(&rep->n[kTexMismatch], mismatch);
    atomicAdd(&rep->n[kTexInvalid], invalid);
    atomicAdd(&rep->n[kTexWrapX], wrapx);
    atomicAdd(&rep->n[kTexWrapY], wrapy);
}

} // namespace
} // namespace c2rt

int main(int argc, char **argv)
{
    using namespace c2rt;
    const int lg = argc > 1 ? atoi(argv[1]) : 26;
    if (lg < 16 || lg > 34) { fprintf(stderr, "log2(numerators) in [16, 34]\n"); return 2; }
    const uint64_t total = 1ull << lg, threads = 1ull << 16, per_thread = total / threads;

    /* the pool: random finite floats, any sign, magnitudes in [2^-20, 2^20): no product or sum of the blend overflows */
    std::vector<float> pool((size_t)kPoolTexels * 4);
    for (size_t i = 0; i < pool.size(); ++i) {
        const uint64_t h = mix64(0xabcdefull + i);
        const uint32_t bits = (uint32_t)(h & 0x807fffffu) | ((107u + (uint32_t)((h >> 32) % 40u)) << 23);
        memcpy(&pool[i], &bits, 4);
    }
    float *dpool;
    Report *drep, rep;
    CHECK(hipMalloc(&dpool, pool.size() * sizeof(float)));
    CHECK(hipMemcpy(dpool, pool.data(), pool.size() * sizeof(float), hipMemcpyHostToDevice));
    CHECK(hipMalloc(&drep, sizeof(Report)));
    CHECK(hipMemset(drep, 0, sizeof(Report)));
    hipLaunchKernelGGL(average_kernel, dim3((unsigned)(threads / 256)), dim3(256), 0, 0, drep, 0x5eedull, per_thread);
    CHECK(hipGetLastError());
    hipLaunchKernelGGL(texel_kernel, dim3((unsigned)(threads / 256)), dim3(256), 0, 0, drep, dpool, 0x7e8e1ull, per_thread / 4 ? per_thread / 4 : 1);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(&rep, drep, sizeof(Report), hipMemcpyDeviceToHost));
    CHECK(hipFree(dpool));
    CHECK(hipFree(drep));

    printf("{\"numerators\": %llu, \"average_inside\": %llu, \"average_mismatches\": %llu, \"average_refused_inside\": %llu, "
           "\"average_outside\": %llu, \"average_accepted_outside\": %llu, \"average_zero\": %llu, \"average_edge\": %llu, "
           "\"first_average\": [%u, %u], "
           "\"texel_quads\": %llu, \"texel_mismatches\": %llu, \"texel_invalid\": %llu, \"texel_wrap_x\": %llu, \"texel_wrap_y\": %llu, "
           "\"first_texel\": [%u, %u, %u, %u]}\n",
           (unsigned long long)total, rep.n[kAvgInside], rep.n[kAvgMismatch], rep.n[kAvgRefusedInside], rep.n[kAvgOutside],
           rep.n[kAvgAcceptedOutside], rep.n[kAvgZero], rep.n[kAvgEdge], rep.first_avg[0], rep.first_avg[1], rep.n[kTexQuads],
           rep.n[kTexMismatch], rep.n[kTexInvalid], rep.n[kTexWrapX], rep.n[kTexWrapY], rep.first_tex[0], rep.first_tex[1],
           rep.first_tex[2], rep.first_tex[3]);
    const bool ok = rep.n[kAvgMismatch] == 0 && rep.n[kAvgRefusedInside] == 0 && rep.n[kAvgAcceptedOutside] == 0 && rep.n[kTexMismatch] == 0;
    return ok ? 0 : 1;
}
