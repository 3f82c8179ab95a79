/*
 * certain_f32_check.hip — device check of the certain-float routes (chess2rt_amd/csrc/f32_certain.h and its two
 * out-of-line wrappers in c2rt_trace_common.inc) against the routines they stand in for, ON the device: its own
 * atan2 / asin / pow, the x87 emulation, the compiler's float conversions.  Test infrastructure.
 *
 *   u,v:  c2_sphere_uv_bitmap(dx, dz, w, s) followed by BitmapTexture's float pipeline  ==  c2_sphere_uv(dx, dz, w)
 *         followed by the same pipeline, float for float;
 *   pow:  c2_pow_f32(a, b)  ==  (float)pow(a, b), float for float;
 * over N operands per routine, structured and random, drawn on the device from a counter hash.  It also counts the
 * random lanes that take the fallback, and holds a set of operands CONSTRUCTED on the host to land on a float
 * midpoint or a floor jump: of those that do land within 2 x 2^-53 of one (tested here with exact arithmetic, not
 * with the routine under test), every one must be refused and must come back as the exact routine's doubles.
 *
 *   certain_f32_check [log2(operands per routine)]     default 26
 * exit code 0 = all holds.  Prints one JSON line.
 */
#define C2RT_TRACE_EXACT_ONLY
#include "../chess2rt_amd/csrc/c2rt_trace_common.inc"

#include <cmath>
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

enum { kUvMismatch, kUvRandom, kUvRandomFallback, kPowMismatch, kPowRandom, kPowRandomFallback, kPowOtherRoute,
       kConUvQualified, kConUvAccepted, kConUvNotExact, kConUvMismatch, kConPowQualified, kConPowAccepted, kConPowMismatch, kNCount };
struct Report {
    unsigned long long n[kNCount];
    double first_uv[4], first_pow[2];
};

__host__ __device__ inline uint64_t mix64(uint64_t z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ inline double unit(uint64_t h) { return (double)(h >> 11) * 0x1p-53; }
/* sign, exponent in [lo, hi), significand random or structured */
__device__ inline double draw(uint64_t key, int lo, int hi)
{
    const uint64_t a = mix64(key), b = mix64(key ^ 0x1234567890abcdefull);
    const int e = lo + (int)((a >> 8) % (uint64_t)(hi - lo));
    uint64_t m = b & 0xFFFFFFFFFFFFFull;
    switch (a & 31) {
    case 0: m = 0; break;
    case 1: m = 0xFFFFFFFFFFFFFull; break;
    case 2: m = 1ull << ((a >> 40) % 52); break;
    case 3: m = 0x5555555555555ull; break;
    case 4: m = b & 0xFF; break;
    case 5: m = 0xFFFFFFFFFFFFFull - (b & 0xFF); break;
    default: break;
    }
    return __longlong_as_double((long long)((b & (1ull << 63)) | ((uint64_t)(e + 1023) << 52) | m));
}
/* BitmapTexture.getTexColor's use of a coordinate, as bitmap_color (c2rt_trace_shared.inc) writes it */
__device__ inline uint32_t pipeline_bits(double u, double s)
{
    u *= s;
    u = u - floor(u);
    return __float_as_uint((float)u);
}
/* (a NaN coordinate — asin outside [-1, 1], an infinite component — is a NaN on both routes) */
__device__ inline bool coord_same(double a, double b, double s) { return pipeline_bits(a, s) == pipeline_bits(b, s) || (a != a && b != b); }
__device__ inline bool uv_same(UV a, UV b, double s) { return coord_same(a.u, b.u, s) && coord_same(a.v, b.v, s); }
/* does c2_sphere_uv_bitmap take its fallback for this operand?  (its own predicate, on the same device libm) */
__device__ inline bool uv_falls_back(double dx, double dz, double w, double s)
{
    double u, v;
    const int ok = sphere_uv_fast(atan2(dz, dx), asin(w), &u, &v);
    return !(ok & uv_float_certain(u, F32C_UV_DELTA, s) & uv_float_certain(v, F32C_UV_DELTA, s));
}
__device__ inline void note(Report *rep, int what) { atomicAdd(&rep->n[what], 1ull); }

__constant__ double kScale[8] = {1.0, 4.0, 0.005, -1.0, 3.7, 1.0, 0.25, 16.0};
__constant__ double kExpo[16] = {1, 2, 3, 59, 60, 80, 1023, 1024, 60, 80, 4, 7, 100, 255, 256, 512};
__constant__ double kOther[8] = {1025, 2.5, 0, 0.5, -1, 60.5, 1e6, -60};

__global__ void check_kernel(Report *rep, uint64_t seed, uint64_t per_thread)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long uv_bad = 0, uv_fb = 0, uv_rand = 0, pw_bad = 0, pw_fb = 0, pw_rand = 0, pw_other = 0;
    for (uint64_t i = 0; i < per_thread; ++i) {
        const uint64_t key = seed + (t * per_thread + i) * 4;
        const uint64_t h = mix64(key);
        /* ---- u, v ---- */
        {
            double dx, dz, w;
            const unsigned kind = (unsigned)(h & 15);
            const double r1 = 2 * unit(mix64(key + 1)) - 1, r2 = 2 * unit(mix64(key + 2)) - 1;
            bool random = false;
            if (kind < 8) { /* a random point of the sphere: any direction, any height */
                double sn, cs;
                sincos(r1 * 3.14159265358979323846, &sn, &cs);
                const double rad = 0.25 + 4 * unit(mix64(key + 3));
                dx = cs * rad; dz = sn * rad; w = r2;
                random = true;
            } else if (kind < 11) { /* components of any magnitude, structured significands */
                dx = draw(key + 1, -40, 40); dz = draw(key + 2, -40, 40); w = draw(key + 3, -60, 0);
            } else if (kind == 11) { /* the seam: angle near +-pi, and the poles */
                dx = -fabs(draw(key + 1, -2, 3)); dz = draw(key + 2, -1070, -20); w = r2 < 0 ? -1.0 + ldexp(fabs(r1), -(int)((h >> 8) % 54)) : 1.0 - ldexp(fabs(r1), -(int)((h >> 8) % 54));
            } else if (kind == 12) { /* the axes, signed zeros */
                const double z = (h >> 9) & 1 ? 0.0 : -0.0;
                dx = (h >> 10) & 1 ? z : r1; dz = (h >> 11) & 1 ? z : ((h >> 12) & 1 ? -z : r2); w = (h >> 13) & 1 ? z : ((h >> 14) & 1 ? 1.0 : -1.0);
            } else if (kind == 13) { /* u near 1/4, 1/2, 3/4: floor jumps of the scaled coordinate */
                dx = (h >> 9) & 1 ? draw(key + 1, -1070, -30) : r1; dz = (h >> 9) & 1 ? r2 : draw(key + 2, -1070, -30); w = draw(key + 3, -1070, -30);
            } else if (kind == 14) { /* out of range: asin is NaN, or an infinite component — both routes give the same bits */
                dx = r1; dz = r2; w = (h >> 9) & 1 ? 1.0 + fabs(r1) : __longlong_as_double(0x7ff0000000000000ll);
                if ((h >> 10) & 1) dx = __longlong_as_double(0x7ff0000000000000ll);
            } else {
                dx = r1; dz = r2; w = r1 * r2;
                random = true;
            }
            const double s = kScale[i & 7]; /* wave-uniform, as c2_sphere_uv_bitmap requires: the same for every thread */
            const UV a = c2_sphere_uv_bitmap(dx, dz, w, s), b = c2_sphere_uv(dx, dz, w);
            if (!uv_same(a, b, s)) {
                if (!uv_bad++ && !atomicAdd(&rep->n[kUvMismatch], 0ull)) { rep->first_uv[0] = dx; rep->first_uv[1] = dz; rep->first_uv[2] = w; rep->first_uv[3] = s; }
            }
            if (random) {
                uv_rand += 1;
                uv_fb += uv_falls_back(dx, dz, w, s);
            }
        }
        /* ---- pow ---- */
        {
            const uint64_t g = mix64(key + 3);
            const double r01 = unit(mix64(g));
            const unsigned route = (unsigned)((g >> 40) & 15);
            double b = route < 12 ? kExpo[(g >> 44) & 15] : (route < 14 ? (double)(1 + (g >> 44) % 1024) : kOther[(g >> 44) & 7]);
            const double n = b >= 1 ? b : 60;
            double a;
            bool random = true;
            switch (g & 7) {
            case 0: a = r01; break;
            case 1: a = ldexp(0.5 + r01 / 2, -(int)((g >> 8) % 300)); break;
            case 2: a = 1.0 - ldexp(r01, -(int)((g >> 8) % 53)); break;
            case 3: a = 1.0 + ldexp(r01, -20 - (int)((g >> 8) % 33)); break;
            case 4: a = exp2(-(149.0 + 60.0 * (r01 - 0.5)) / n); break;       /* a^n around the least float */
            case 5: a = 1.0 - ldexp(r01, -10); break;                          /* highlights */
            case 6: a = ldexp(0.5 + r01 / 2, -(int)((g >> 8) % 4)); break;
            default: /* outside the fast route's range, specials: the pow route */
                random = false;
                switch ((g >> 8) & 7) {
                case 0: a = 0.0; break;
                case 1: a = 1.0 + ldexp(1.0 + r01, -20); break;
                case 2: a = ldexp(1.0 + r01, -320 - (int)((g >> 12) % 700)); break;
                case 3: a = 1.0 + r01 * 4; break;
                case 4: a = __longlong_as_double(0x7ff0000000000000ll); break;
                case 5: a = __longlong_as_double(0x7ff8000000000000ll); break;
                case 6: a = 0x1p-300; break;
                default: a = 1.0 + 0x1p-20; break;
                }
            }
            /* (shade() calls with cosGamma > 0 only; negative bases go to pow all the same) */
            if (((g >> 60) & 15) == 0) a = -a;
            const float got = c2_pow_f32(a, b), want = (float)pow(a, b);
            const bool same = __float_as_uint(got) == __float_as_uint(want) || (got != got && want != want);
            if (!same) {
                if (!pw_bad++ && !atomicAdd(&rep->n[kPowMismatch], 0ull)) { rep->first_pow[0] = a; rep->first_pow[1] = b; }
            }
            float f;
            const bool certain = pow_f32_certain(a, b, &f);
            if (route >= 14 && certain) pw_other += 1; /* exponents of the pow route must be refused */
            if (route < 14 && random && a > 0) {
                pw_rand += 1;
                pw_fb += !certain;
            }
        }
    }
    if (uv_bad) atomicAdd(&rep->n[kUvMismatch], uv_bad);
    if (pw_bad) atomicAdd(&rep->n[kPowMismatch], pw_bad);
    atomicAdd(&rep->n[kUvRandom], uv_rand);
    atomicAdd(&rep->n[kUvRandomFallback], uv_fb);
    atomicAdd(&rep->n[kPowRandom], pw_rand);
    atomicAdd(&rep->n[kPowRandomFallback], pw_fb);
    if (pw_other) atomicAdd(&rep->n[kPowOtherRoute], pw_other);
}

/* |x - the nearest midpoint of two neighbouring floats|, exact: x in [2^-20, 1), the midpoints are doubles and the
 * differences of such close doubles are exact */
__device__ inline double dist_to_float_midpoint(double x)
{
    const float f = (float)x;
    const float up = __uint_as_float(__float_as_uint(f) + 1), dn = __uint_as_float(__float_as_uint(f) - 1);
    const double m1 = ((double)f + (double)up) / 2, m0 = ((double)f + (double)dn) / 2;
    return fmin(fabs(x - m1), fabs(x - m0));
}

/* constructed u,v operands: cand = (dx, dz, w, unused), n of them, all for the one scaling s (wave-uniform) */
__global__ void constructed_uv_kernel(Report *rep, const double *cand, uint32_t n, double s)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double dx = cand[4 * i], dz = cand[4 * i + 1], w = cand[4 * i + 2];
    double u, v;
    if (!sphere_uv_fast(atan2(dz, dx), asin(w), &u, &v)) return;
    /* lands on an ambiguity: scale 1 — within 2 x 2^-53 of a float midpoint; other scales — u*s within 2 x 2^-53 * |s|
     * of an integer (u*s itself is rounded by at most 2 x 2^-53 below 4: still inside delta * |s| = 4 x 2^-53 * |s|) */
    bool q;
    if (s == 1.0) q = (u > 0x1p-20 && u < 1 && dist_to_float_midpoint(u) <= 0x1p-52) || (v > 0x1p-20 && v < 1 && dist_to_float_midpoint(v) <= 0x1p-52);
    else q = fabs(u * s - rint(u * s)) <= 0x1p-52 * fabs(s) || fabs(v * s - rint(v * s)) <= 0x1p-52 * fabs(s);
    if (!q) return;
    note(rep, kConUvQualified);
    if (!uv_falls_back(dx, dz, w, s)) note(rep, kConUvAccepted);
    const UV a = c2_sphere_uv_bitmap(dx, dz, w, s), b = c2_sphere_uv(dx, dz, w);
    if (__double_as_longlong(a.u) != __double_as_longlong(b.u) || __double_as_longlong(a.v) != __double_as_longlong(b.v)) note(rep, kConUvNotExact);
    if (!uv_same(a, b, s)) note(rep, kConUvMismatch);
}

/* constructed powers: cand = (a, n) */
__global__ void constructed_pow_kernel(Report *rep, const double *cand, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = cand[2 * i], b = cand[2 * i + 1];
    const double r = pow_int_chain(a, (int)b);
    if (!(r > 0x1p-100 && r < 1 && dist_to_float_midpoint(r) <= r * 0x1p-52)) return;
    note(rep, kConPowQualified);
    float f;
    if (pow_f32_certain(a, b, &f)) note(rep, kConPowAccepted);
    if (__float_as_uint(c2_pow_f32(a, b)) != __float_as_uint((float)pow(a, b))) note(rep, kConPowMismatch);
}

} // namespace
} // namespace c2rt

using namespace c2rt;

static double step(double d, long k)
{
    long long i;
    memcpy(&i, &d, 8);
    i += d > 0 ? k : -k;
    memcpy(&d, &i, 8);
    return d;
}

int main(int argc, char **argv)
{
    const int lg = argc > 1 ? atoi(argv[1]) : 26;
    const uint64_t total = 1ull << lg;
    const uint32_t blocks = 2048, threads = 256;
    const uint64_t nthreads = (uint64_t)blocks * threads;
    const uint64_t per_thread = (total + nthreads - 1) / nthreads;
    Report *rep;
    CHECK(hipMalloc(&rep, sizeof(Report)));
    CHECK(hipMemset(rep, 0, sizeof(Report)));
    /* launches of at most 2^24 operands each, so that no launch runs for long */
    const uint64_t chunk = (1ull << 24) / nthreads > 0 ? (1ull << 24) / nthreads : 1;
    for (uint64_t done = 0, launch = 0; done < per_thread; ++launch) {
        const uint64_t n = per_thread - done < chunk ? per_thread - done : chunk;
        hipLaunchKernelGGL(check_kernel, dim3(blocks), dim3(threads), 0, 0, rep, 0xF32Cull + (launch << 44), n);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        done += n;
    }

    /* constructed operands (host, long double): targets t = a float midpoint (scale 1) or k / s (scales 4, 3.7);
     * u = t at angle = 2 pi t - pi, v = t at asin = pi/2 - pi t; a few neighbours of each */
    const long double PI = 3.14159265358979323846264338327950288L;
    std::vector<double> cus[3], cp; /* u,v candidates per scaling */
    const double scalings[3] = {1.0, 4.0, 3.7};
    for (int j = 0; j < 6000; ++j) {
        const uint64_t h = mix64(77000 + j);
        const int kind = j % 3;
        long double t;
        double s;
        if (kind == 0) {
            const float f = 0.05f + 0.9f * (float)((h >> 11) * 0x1p-53);
            t = ((long double)f + (long double)nextafterf(f, 2.0f)) / 2;
            s = 1.0;
        } else {
            s = kind == 1 ? 4.0 : 3.7;
            t = (long double)(1 + (int)(h % 3)) / (long double)s;
        }
        const long double ang = 2 * PI * t - PI, as = PI / 2 - PI * t;
        std::vector<double> &cu = cus[kind];
        for (long k = -4; k <= 4; ++k) {
            /* u: the direction of `ang`, its z component a few doubles either way */
            const double dx = (double)cosl(ang), dz = (double)sinl(ang);
            cu.insert(cu.end(), {dx, dz == 0 ? 0.0 : step(dz, k), 0.3, s});
            /* v: the height sin(as), a few doubles either way */
            const double w = (double)sinl(as);
            cu.insert(cu.end(), {0.6, 0.7, w == 0 ? 0.0 : step(w, k), s});
        }
        /* a^n on a float midpoint: a = m^(1/n) and neighbours */
        const float f = 0.01f + 0.98f * (float)((mix64(h) >> 11) * 0x1p-53);
        const long double m = ((long double)f + (long double)nextafterf(f, 2.0f)) / 2;
        static const int ns[] = {1, 2, 3, 60};
        const int n = ns[j & 3];
        const double a0 = (double)powl(m, 1.0L / n);
        for (long k = -2; k <= 2; ++k) cp.insert(cp.end(), {step(a0, k), (double)n});
    }
    double *d_cu[3], *d_cp;
    uint32_t nu = 0;
    for (int k = 0; k < 3; ++k) {
        const uint32_t n = (uint32_t)(cus[k].size() / 4);
        CHECK(hipMalloc(&d_cu[k], cus[k].size() * sizeof(double)));
        CHECK(hipMemcpy(d_cu[k], cus[k].data(), cus[k].size() * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(constructed_uv_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, rep, d_cu[k], n, scalings[k]);
        CHECK(hipGetLastError());
        nu += n;
    }
    CHECK(hipMalloc(&d_cp, cp.size() * sizeof(double)));
    CHECK(hipMemcpy(d_cp, cp.data(), cp.size() * sizeof(double), hipMemcpyHostToDevice));
    const uint32_t np = (uint32_t)(cp.size() / 2);
    hipLaunchKernelGGL(constructed_pow_kernel, dim3((np + 255) / 256), dim3(256), 0, 0, rep, d_cp, np);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());

    Report h;
    CHECK(hipMemcpy(&h, rep, sizeof h, hipMemcpyDeviceToHost));
    static const char *names[kNCount] = {"uv_mismatches", "uv_random", "uv_random_fallback", "pow_mismatches", "pow_random", "pow_random_fallback",
                                         "pow_route_accepted", "constructed_uv", "constructed_uv_accepted", "constructed_uv_not_exact_doubles",
                                         "constructed_uv_mismatches", "constructed_pow", "constructed_pow_accepted", "constructed_pow_mismatches"};
    printf("{\"operands_per_routine\": %llu, \"constructed_uv_candidates\": %u, \"constructed_pow_candidates\": %u", (unsigned long long)(per_thread * nthreads), nu, np);
    for (int i = 0; i < kNCount; ++i) printf(", \"%s\": %llu", names[i], h.n[i]);
    printf("}\n");
    if (h.n[kUvMismatch]) fprintf(stderr, "u,v: first mismatch at dx %a dz %a w %a s %a\n", h.first_uv[0], h.first_uv[1], h.first_uv[2], h.first_uv[3]);
    if (h.n[kPowMismatch]) fprintf(stderr, "pow: first mismatch at a %a b %a\n", h.first_pow[0], h.first_pow[1]);
    const bool bad = h.n[kUvMismatch] || h.n[kPowMismatch] || h.n[kPowOtherRoute] || h.n[kConUvAccepted] || h.n[kConUvNotExact] || h.n[kConUvMismatch] ||
                     h.n[kConPowAccepted] || h.n[kConPowMismatch] || !h.n[kConUvQualified] || !h.n[kConPowQualified] ||
                     h.n[kUvRandomFallback] > 1e-4 * h.n[kUvRandom] || h.n[kPowRandomFallback] > 1e-4 * h.n[kPowRandom];
    return bad ? 1 : 0;
}
