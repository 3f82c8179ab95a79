/*
 * f32_certain_check.c — host check of chess2rt_amd/csrc/f32_certain.h against x87.h (the exact u, v) and the
 * compiler's `long double` (the exact power).  tests/test_f32_certain_host.py builds and runs it:
 *
 *     f32_certain_check N_RANDOM DELTA_SCALE
 *
 * DELTA_SCALE 1 is the check; DELTA_SCALE 0 is the mutation "delta = 0", under which the soundness sections must
 * REPORT mismatches (the constructed operands sit on a float midpoint / a floor boundary within an ulp or two).
 * Exit status 0 iff every section holds (with DELTA_SCALE 1) — the caller reads the printed counts as well.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../chess2rt_amd/csrc/f32_certain.h"
#include "../chess2rt_amd/csrc/x87.h"

#define NS 5
static const double kScales[NS] = {1.0, 4.0, 0.005, -1.0, 3.7};
static const long double kPiL = 3.14159265358979323846264338327950288L;

static uint64_t mix(uint64_t x)
{
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
static double unit(uint64_t h) { return (double)(h >> 11) * 0x1p-53; } /* [0, 1) */
static uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static double dnext(double d, long k) /* k doubles up (down) from d, d != 0 */
{
    int64_t i;
    memcpy(&i, &d, 8);
    i += d > 0 ? k : -k;
    memcpy(&d, &i, 8);
    return d;
}
static int same_pipeline(double a, double b, double s)
{
    double fa, fb;
    const float xa = uv_bitmap_float(a, s, &fa), xb = uv_bitmap_float(b, s, &fb);
    return fa == fb && fbits(xa) == fbits(xb);
}

typedef struct {
    long long n, bound_viol, certain[2], mismatch[2];
    long double max_u, max_v; /* units of 2^-53 */
} Tally;

/* one angle: `which` 0: as atan2's result (u), 1: as asin's result (v) */
static void one(double x, int which, double delta, Tally *t)
{
    double u, v;
    const int ok = which == 0 ? sphere_uv_fast(x, 0.0, &u, &v) : sphere_uv_fast(0.0, x, &u, &v);
    if (!ok) return;
    const double fast = which == 0 ? u : v;
    const double exact = which == 0 ? x87_sphere_u(x) : x87_sphere_v(x);
    const long double err = fabsl((long double)fast - (long double)exact) * 0x1p53L;
    t->n += 1;
    if (which == 0 && err > t->max_u) t->max_u = err;
    if (which == 1 && err > t->max_v) t->max_v = err;
    if (err > (long double)F32C_UV_DELTA * 0x1p53L) t->bound_viol += 1;
    for (int i = 0; i < NS; ++i)
        if (uv_float_certain(fast, delta, kScales[i])) {
            t->certain[which] += 1;
            if (!same_pipeline(fast, exact, kScales[i])) t->mismatch[which] += 1;
        }
}
static void add(Tally *a, const Tally *b)
{
    a->n += b->n; a->bound_viol += b->bound_viol;
    for (int i = 0; i < 2; ++i) { a->certain[i] += b->certain[i]; a->mismatch[i] += b->mismatch[i]; }
    if (b->max_u > a->max_u) a->max_u = b->max_u;
    if (b->max_v > a->max_v) a->max_v = b->max_v;
}
static void both_signs(double x, double delta, Tally *t)
{
    one(x, 0, delta, t); one(-x, 0, delta, t);
    one(x, 1, delta, t); one(-x, 1, delta, t);
}

/* every binade up to 4 with tie patterns in the low and the high bits of the significand, both signs */
static void structured(double delta, Tally *t)
{
    static const uint64_t pat[] = {0, 1, 2, 3, 0x3ff, 0x400, 0x401, 0x7ff, 0x800, 0x801, 0xfff, 0x1000,
                                   0x8000000000000ull, 0x8000000000001ull, 0x7ffffffffffffull, 0xfffffffffffffull,
                                   0xffffffffffffeull, 0x5555555555555ull, 0xaaaaaaaaaaaaaull, 0xc000000000000ull};
    for (int ex = 0; ex <= 1024; ++ex) /* biased exponent 0 (subnormals) .. 1024: values up to 4 */
        for (unsigned i = 0; i < sizeof pat / sizeof *pat; ++i) {
            const uint64_t b = ((uint64_t)ex << 52) | pat[i];
            double x;
            memcpy(&x, &b, 8);
            both_signs(x, delta, t);
        }
    both_signs(0.0, delta, t);
    /* the ends of atan2's and asin's ranges and their neighbours, zero's neighbours */
    const double centres[] = {3.14159265358979323846, 1.57079632679489661923, 4.0, 2.0, 1.0, 0.5, 0x1p-1022, 0x1p-60};
    for (unsigned c = 0; c < sizeof centres / sizeof *centres; ++c)
        for (long k = -3000; k <= 3000; ++k) both_signs(dnext(centres[c], k), delta, t);
}

/* Operands constructed to be ambiguous: angles at which u (v) lies within an ulp or two of (i) the midpoint of two
 * neighbouring floats (scale 1) and (ii) a jump of floor(u * s) for s = 4 and 3.7.  A correct uv_float_certain
 * refuses (nearly) all of them; with delta = 0 it accepts them and the pipeline on u' differs from the exact one. */
static void constructed(double delta, long long out[2][3] /* [midpoint, floor][n, refused, mismatch] */)
{
    memset(out, 0, sizeof(long long) * 6);
    for (int kind = 0; kind < 2; ++kind)
        for (int j = 0; j < 4000; ++j) {
            long double target; /* the u (v) to land on */
            double s;
            if (kind == 0) {
                const float f = 0.05f + 0.9f * (float)unit(mix(1000 + j));
                target = ((long double)f + (long double)nextafterf(f, 2.0f)) / 2;
                s = 1.0;
            } else {
                s = (j & 1) ? 4.0 : 3.7;
                const int k = 1 + (int)(mix(5000 + j) % 3); /* floor jumps at u * s = 1, 2, 3 */
                target = (long double)k / (long double)s;
            }
            for (int which = 0; which < 2; ++which) {
                /* u = (pi + angle) / (2 pi);  v = 1 - (pi/2 + as) / pi */
                const long double x0 = which == 0 ? target * 2 * kPiL - kPiL : (1 - target) * kPiL - kPiL / 2;
                for (long k = -6; k <= 6; ++k) {
                    const double x = dnext((double)x0 == 0 ? 0x1p-60 : (double)x0, k);
                    double u, v;
                    if (!(which == 0 ? sphere_uv_fast(x, 0.0, &u, &v) : sphere_uv_fast(0.0, x, &u, &v))) continue;
                    const double fast = which == 0 ? u : v, exact = which == 0 ? x87_sphere_u(x) : x87_sphere_v(x);
                    out[kind][0] += 1;
                    if (!uv_float_certain(fast, delta, s)) out[kind][1] += 1;
                    else if (!same_pipeline(fast, exact, s)) out[kind][2] += 1;
                }
            }
        }
}

static int check_pow(long long n_per)
{
    static const int ns[] = {1, 2, 3, 59, 60, 80, 1023, 1024};
    int bad = 0;
    for (unsigned i = 0; i < sizeof ns / sizeof *ns; ++i) {
        const int n = ns[i];
        long double max_err = 0;
        long long viol = 0, underflowed = 0, certain = 0, float_mismatch = 0;
#pragma omp parallel for reduction(+ : viol, underflowed, certain, float_mismatch) reduction(max : max_err) num_threads(8)
        for (long long k = 0; k < n_per; ++k) {
            const uint64_t h = mix((uint64_t)k * 8 + i);
            const double r01 = unit(mix(h));
            double a;
            switch (h & 7) { /* classes of a over [2^-300, 1 + 2^-20] */
            case 0: a = r01; break;                                              /* uniform */
            case 1: a = ldexp(0.5 + r01 / 2, -(int)((h >> 8) % 300)); break;     /* log-uniform down to 2^-300 */
            case 2: a = 1.0 - ldexp(r01, -(int)((h >> 8) % 53)); break;          /* below 1, at every distance */
            case 3: a = 1.0 + ldexp(r01, -20 - (int)((h >> 8) % 33)); break;     /* (1, 1 + 2^-20] */
            case 4: a = ldexp(0.5 + r01 / 2, -(int)((h >> 8) % 4)); break;       /* [1/16, 1): where lobes live */
            case 5: a = exp2(-(149.0 + 60.0 * (r01 - 0.5)) / n); break;          /* a^n around the least float */
            case 6: a = exp2(-(1022.0 + 8.0 * (r01 - 0.5)) / n); break;          /* a^n around the least normal double */
            default: a = 1.0 - ldexp(r01, -10) ; break;                          /* highlights: cos close to 1 */
            }
            if (!(a >= 0x1p-300 && a <= 1.0 + 0x1p-20)) a = 0x1p-300;
            const double r = pow_int_chain(a, n);
            const long double p = powl((long double)a, (long double)n);
            if (r >= 0x1p-200) {
                const long double err = fabsl((long double)r - p) / p * 0x1p53L;
                if (err > max_err) max_err = err;
                /* (n - 1) x 2^-53, plus what powl itself may be off by: 2^-63 relative */
                if (fabsl((long double)r - p) > ((long double)(n - 1) * 0x1p-53L + 0x1p-63L) * p) viol += 1;
            } else {
                underflowed += 1;
                if (!(p < 0x1p-199L)) viol += 1; /* a small chain result means a small power: both floats are +0 */
            }
            float f;
            if (pow_f32_certain(a, (double)n, &f)) {
                certain += 1;
                if (fbits(f) != fbits((float)p)) float_mismatch += 1;
            }
        }
        printf("pow n=%d samples=%lld max_err=%.2Lf x 2^-53 bound=%d violations=%lld chain_below_2^-200=%lld certain=%lld ambiguous=%lld float_mismatches=%lld\n",
               n, n_per, max_err, n - 1, viol, underflowed, certain, n_per - certain, float_mismatch);
        bad += viol != 0 || float_mismatch != 0;
    }
    return bad;
}

static int check_refusals(void)
{
    int bad = 0;
    float f;
    const double nan_ = NAN, inf_ = INFINITY;
    const double bad_b[] = {0.5, 2.5, 59.999999, 60.000001, 0.0, -0.0, -1.0, -60.0, 1025.0, 1024.5, 2048.0, 1e300, 0x1p-1074, nan_, inf_, -inf_};
    for (unsigned i = 0; i < sizeof bad_b / sizeof *bad_b; ++i)
        if (pow_f32_certain(0.5, bad_b[i], &f)) { printf("refusal: accepted exponent %a\n", bad_b[i]); bad += 1; }
    const double bad_a[] = {0.0, -0.0, -0.5, 0x1p-301, 0x1p-1074, 0x1.fffffffffffffp-301, 1.0 + 0x1p-19, 0x1.0000100000001p+0, 2.0, 1e300, inf_, -inf_, nan_};
    for (unsigned i = 0; i < sizeof bad_a / sizeof *bad_a; ++i)
        if (pow_f32_certain(bad_a[i], 60.0, &f)) { printf("refusal: accepted base %a\n", bad_a[i]); bad += 1; }
    /* and what it must accept, with the value */
    const struct { double a, b; float want; } good[] = {
        {0.5, 1.0, 0.5f}, {0.5, 2.0, 0.25f}, {1.0, 1024.0, 1.0f}, {0.5, 1024.0, 0.0f}, {0x1p-300, 1.0, 0.0f},
        {0x1p-300, 1024.0, 0.0f}, {0.5, 149.0, 0x1p-149f}, {0.5, 151.0, 0.0f}, {0.25, 60.0, 0x1p-120f}};
    for (unsigned i = 0; i < sizeof good / sizeof *good; ++i)
        if (!pow_f32_certain(good[i].a, good[i].b, &f) || fbits(f) != fbits(good[i].want)) {
            printf("refusal: %a ^ %a not certain or not %a\n", good[i].a, good[i].b, (double)good[i].want);
            bad += 1;
        }
    /* u, v: NaN anywhere, s zero or not finite, |angle| > 4, |asin| > 2 */
    const double bad_s[] = {0.0, -0.0, inf_, -inf_, nan_};
    for (unsigned i = 0; i < sizeof bad_s / sizeof *bad_s; ++i)
        if (uv_float_certain(0.3, F32C_UV_DELTA, bad_s[i])) { printf("refusal: accepted scale %a\n", bad_s[i]); bad += 1; }
    if (uv_float_certain(nan_, F32C_UV_DELTA, 1.0) || uv_float_certain(inf_, F32C_UV_DELTA, 1.0) || uv_float_certain(0.3, nan_, 1.0)) { printf("refusal: accepted a NaN / infinite coordinate\n"); bad += 1; }
    if (!uv_float_certain(0.3, F32C_UV_DELTA, 1.0) || !uv_float_certain(0.3, F32C_UV_DELTA, -3.7)) { printf("refusal: 0.3 not certain\n"); bad += 1; }
    double u, v;
    const double bad_angle[] = {4.0000000000000009, -4.0000000000000009, 1e300, inf_, -inf_, nan_};
    for (unsigned i = 0; i < sizeof bad_angle / sizeof *bad_angle; ++i)
        if (sphere_uv_fast(bad_angle[i], 0.0, &u, &v) || sphere_uv_fast(0.0, bad_angle[i], &u, &v)) { printf("refusal: accepted angle %a\n", bad_angle[i]); bad += 1; }
    if (sphere_uv_fast(0.0, 2.0000000000000004, &u, &v) || !sphere_uv_fast(4.0, 2.0, &u, &v) || !sphere_uv_fast(-4.0, -2.0, &u, &v)) { printf("refusal: the range's ends\n"); bad += 1; }
    printf("refusals failures=%d\n", bad);
    return bad;
}

int main(int argc, char **argv)
{
    const long long n_random = argc > 1 ? atoll(argv[1]) : 100000000ll;
    const double scale = argc > 2 ? atof(argv[2]) : 1.0;
    const double delta = F32C_UV_DELTA * scale;
    int bad = 0;

    Tally t;
    memset(&t, 0, sizeof t);
    structured(delta, &t);
    /* random: uniform over atan2's and asin's ranges, the whole admitted range, and the neighbourhoods of +-pi, +-pi/2, 0 */
#pragma omp parallel num_threads(8)
    {
        Tally mine;
        memset(&mine, 0, sizeof mine);
#pragma omp for
        for (long long k = 0; k < n_random; ++k) {
            const uint64_t h = mix((uint64_t)k);
            const double r = 2 * unit(mix(h)) - 1; /* [-1, 1) */
            const int which = (int)(h & 1);
            const double full = which == 0 ? 3.14159265358979323846 : 1.57079632679489661923;
            double x;
            switch ((h >> 1) % 8) {
            case 0: case 1: case 2: x = r * full; break;
            case 3: x = r * (which == 0 ? 4.0 : 2.0); break;
            case 4: x = (r < 0 ? -full : full) - r * 1e-6; break;  /* within 1e-6 of the ends, inside and outside */
            case 5: x = (r < 0 ? -full : full) / 2 + r * 1e-6; break; /* +-pi/2 for u */
            case 6: x = r * 1e-9; break;
            default: x = ldexp(r, -(int)((h >> 8) % 1000)); break;  /* every binade */
            }
            one(x, which, delta, &mine);
        }
#pragma omp critical
        add(&t, &mine);
    }
    printf("uv angles=%lld max_err_u=%.3Lf max_err_v=%.3Lf x 2^-53 delta=%.1f bound_violations=%lld\n", t.n, t.max_u, t.max_v,
           F32C_UV_DELTA * 0x1p53, t.bound_viol);
    printf("uv soundness delta_scale=%g: u certain=%lld mismatches=%lld; v certain=%lld mismatches=%lld\n", scale, t.certain[0],
           t.mismatch[0], t.certain[1], t.mismatch[1]);
    bad += t.bound_viol != 0 || t.mismatch[0] != 0 || t.mismatch[1] != 0;

    long long c[2][3];
    constructed(delta, c);
    printf("uv constructed delta_scale=%g: midpoint n=%lld refused=%lld mismatches=%lld; floor n=%lld refused=%lld mismatches=%lld\n", scale,
           c[0][0], c[0][1], c[0][2], c[1][0], c[1][1], c[1][2]);
    bad += c[0][2] != 0 || c[1][2] != 0;

    bad += check_pow(n_random / 50 > 100000 ? n_random / 50 : 100000);
    bad += check_refusals();
    printf("%s\n", bad ? "FAILED" : "ALL OK");
    return bad ? 1 : 0;
}
