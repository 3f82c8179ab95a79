/*
 * f32_certain.h — two fp64 values of the shading path whose only reader in a frame converts them to `float` at
 * once, computed the cheap way where the float that comes out is CERTAIN to be the one the expensive way gives:
 *
 *     Sphere.intersect's u, v (rt/geometry.d:119-120; x87.h), read by BitmapTexture.getTexColor as
 *         (float)(u*s - floor(u*s))                                          — rt/texture.d:116-126
 *     the Phong lobe  (float)pow(cosGamma, exponent)                         — rt/shader.d:101, 241
 *
 * The pattern is lean:: / exact:: once more (fp64_lean.h): compute optimistically with a PROVEN error bound, test
 * that every double inside the bound converts to the same float, and otherwise run the routine the frame has always
 * run.  The pixel is then the same pixel by construction, not "nearly always".  Plain arithmetic, host and device:
 * tests/f32_certain_check.c holds it to x87.h and `long double` on the host, tests/certain_f32_check.hip to the
 * device's own pow / atan2 / asin path.  No fused multiply-add may be formed from these expressions
 * (-ffp-contract=off, as everywhere in this project): the bounds count one rounding per written operation.
 *
 * Units below: 1 u = 2^-53.
 */
#ifndef C2RT_F32_CERTAIN_H
#define C2RT_F32_CERTAIN_H

#include <math.h>

#if defined(__HIPCC__)
#define F32C_FN static __host__ __device__ __forceinline__
#else
#define F32C_FN static inline
#endif

/* RN(pi), RN(1/(2 pi)), RN(1/pi) as doubles */
#define F32C_PI 3.14159265358979323846
#define F32C_INV_2PI 0.15915494309189533577
#define F32C_INV_PI 0.31830988618379067154

/* What u', v' below may differ by from x87_sphere_u / x87_sphere_v: 2^-51 = 4 u, ABSOLUTE (the sum cancels at
 * angle = -pi, so no relative bound exists).  Derivation, for |angle| <= 4 and |asin_value| <= 2 (where today's
 * code takes the x87 expressions; atan2 and asin return no more than RN(pi) and RN(pi/2), the first line of each
 * table; the second line is the rest of the admitted range, where results pass 1 and an ulp doubles).
 *
 *   x87 side.  U = RN53(RN64(RN64(PI_x + angle) / (2 PI_x))), PI_x the 64-bit pi.  The sum is below 8: half an
 *   ulp64 there is 2^-62, which the division shrinks to 0.0003 u; the quotient's rounding: 2^-65 = 0.0003 u; that
 *   the divisor is 2 PI_x and not 2 pi: 2^-64 relative, 0.0005 u; the rounding to double of a value in [0, 1]:
 *   2^-54 = 0.5 u (in (1, 1.14): 1 u).  So U = (PI_x + angle) / (2 pi) + e, |e| <= 0.502 u (1.002 u).  V has one
 *   more 64-bit rounding, 1 - q: the same figures.
 *
 *   u' = RN(RN(PI_d + angle) * C), PI_d = RN53(pi), C = RN53(1 / (2 pi)), in units of u:
 *                      PI_d - PI_x       RN(PI_d + angle)        C: half an ulp is     RN(sum * C)    x87    total
 *                      = 1.2246e-16,     half an ulp 2^-51,      2^-56, times the      half an ulp    side
 *                      over 2 pi         over 2 pi               sum
 *     angle <= PI_d    0.18              0.64                    0.79 (sum < 6.2832)   0.5            0.502  2.62
 *     angle <= 4       0.18              0.64                    0.90 (sum < 7.15)     1.0            1.002  3.73
 *
 *   v' = RN(1 - RN(RN(PI_d/2 + as) * C')), C' = RN53(1 / pi); PI_d / 2 is exact:
 *                      (PI_d - PI_x)/2   RN(PI_d/2 + as)         C': 2^-55 times       RN(sum * C')   RN(1 - P)   x87    total
 *                      over pi           half an ulp over pi     the sum                                          side
 *     |as| <= PI_d/2   0.18              0.64 (2^-52)            0.79 (sum < 3.1416)   0.5 (1.0 if    0.5         0.502  3.62
 *                                                                                      P rounds to 1+)
 *     as in (.., 2]    0.18              0.64                    0.90 (sum < 3.58)     1.0            0.5         0.502  3.73
 *     as in [-2, ..)   0.18              0.08 (|sum| < 0.43)     0.11                  0.13           1.0         1.002  2.51
 *
 * All below 4 u = 2^-51.  (Measured by tests/test_f32_certain_host.py over 1e8 angles, every binade and the
 * neighbourhoods of +-pi, +-pi/2 and 0 among them: 2.00 u and 2.02 u.) */
#define F32C_UV_DELTA 0x1p-51

/* u', v'.  Returns whether the bound above applies: false for NaN operands and outside |angle| <= 4,
 * |asin_value| <= 2 (the caller then takes today's route, which evaluates the plain expression out there). */
F32C_FN int sphere_uv_fast(double angle, double asin_value, double *u, double *v)
{
    *u = (F32C_PI + angle) * F32C_INV_2PI;
    *v = 1.0 - (F32C_PI / 2 + asin_value) * F32C_INV_PI;
    return (fabs(angle) <= 4.0) & (fabs(asin_value) <= 2.0);
}

/* BitmapTexture.getTexColor's use of a coordinate: a = U*s; a - floor(a); (float).  *fl: the floor. */
F32C_FN float uv_bitmap_float(double U, double s, double *fl)
{
    const double a = U * s;
    *fl = floor(a);
    return (float)(a - *fl);
}

/* True iff every double T with |T - U| <= delta goes through uv_bitmap_float(T, s) to the same floor and the
 * same float as U does.  T -> RN(T*s) is monotone (rising for s > 0, falling for s < 0); while the floor f stays
 * the same a -> RN(a - f) is monotone, and so is the conversion to float: equal floors and equal floats at the two
 * ends are equal floors and floats at every double between them.  The ends U -+ delta are rounded to doubles here;
 * rounding is monotone as well, so a double T <= U + delta (as reals) is <= RN(U + delta): no T escapes.
 * A NaN anywhere makes a comparison false (a - f is never -0, so equal floats are equal bits); s == 0 and
 * non-finite s are refused by name. */
F32C_FN int uv_float_certain(double U, double delta, double s)
{
    double f0, f1;
    const float x0 = uv_bitmap_float(U - delta, s, &f0);
    const float x1 = uv_bitmap_float(U + delta, s, &f1);
    return (s != 0.0) & (fabs(s) < INFINITY) & (f0 == f1) & (x0 == x1);
}

/* a^n by square-and-multiply, n in [1, 1024]: at most 10 squarings, and only the powers of set bits enter r (the
 * first of them by assignment), so a^n is the product of n factors a taken with n - 1 roundings in all.  Every value
 * computed is an ancestor of the result. */
F32C_FN double pow_int_chain(double a, int n)
{
    double base = a, r = 1.0;
    int first = 1;
    for (;;) {
        if (n & 1) {
            r = first ? base : r * base;
            first = 0;
        }
        n >>= 1;
        if (!n) break;
        base = base * base;
    }
    return r;
}

/* (float)pow(a, b) without pow, where the float is certain: true and *out set, or false (the caller calls pow).
 *
 * Fast route for b an integer n in [1, 1024] and a finite in [2^-300, 1 + 2^-20]; r = pow_int_chain(a, n).
 * Every factor of the chain is at most (1 + 2^-20)^1024 * (1 + tiny) < 1.001, so nothing overflows, and a value
 * of the chain that comes out below 2^-1022 (where a product stops being relatively exact) drags everything
 * computed from it below 1.001^11 * 2^-1022: r >= 2^-200 proves that NO intermediate left the normal range.  Then
 * r = a^n (1 + e) with |e| <= (1 + u)^(n-1) - 1 < (n - 1) u (1 + 2^-43).  The device's pow is documented within
 * 1 ulp, at most 2 u relative; the products r * (1 -+ d) round by 0.5 u each.  With d = (n + 4) u the interval
 * [r (1 - d), r (1 + d)] therefore holds both a^n and pow's double, with 2.5 u to spare; conversion to float is
 * monotone, so equal floats at its ends are the float of everything inside.
 * r < 2^-200: either no intermediate was subnormal, and a^n <= r (1 + n u) < 2^-199; or one was, the computed
 * a^m < 2^-1022 of an exact-to-(m u) chain, so the true a^m < 2^-1021 with a < 1, and a^n <= a^m.  Either way a^n
 * and its 1-ulp neighbours lie far below 2^-150, half the least float: both routines convert to +0. */
F32C_FN int pow_f32_certain(double a, double b, float *out)
{
    if (!((b >= 1.0) & (b <= 1024.0) & (a >= 0x1p-300) & (a <= 1.0 + 0x1p-20))) return 0; /* NaN: false */
    const int n = (int)b;
    if ((double)n != b) return 0;
    const double r = pow_int_chain(a, n);
    if (r < 0x1p-200) {
        *out = 0.0f;
        return 1;
    }
    const double d = (double)(n + 4) * 0x1p-53;
    const float lo = (float)(r * (1.0 - d)), hi = (float)(r * (1.0 + d));
    *out = lo;
    return lo == hi;
}

#endif /* C2RT_F32_CERTAIN_H */
