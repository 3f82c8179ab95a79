/*
 * ground_certain.h — a sample that hits the ground plane, computed through a short fp64 chain wherever the floats
 * and decisions the pixel reads of it are CERTAIN to be the ones the reference's long chain gives.
 *
 * The reference (exact:: in c2rt_trace.inc, which lean:: equals inside its windows) reaches the hit point through
 * normalize(raw), Node.intersect's second normalize, mult = (o.y - gy) / -dn.y and p = o + dn * mult, then takes
 * lightPos - p, its squared length, a square root and a reciprocal.  On a ground-only tile no reader keeps any of
 * those doubles: each is compared or converted to `float` at once.  So, as in f32_certain.h: compute the cheap
 * way with a PROVEN bound against the reference's value, keep the result only where every double inside the bound
 * gives the same float / the same decision, and report `unsure` otherwise (the caller then runs the parent's
 * routine for the whole tile).  Plain arithmetic, host and device; tests/ground_certain_check.c holds every bound and
 * every "certain" to the reference chain written out in IEEE doubles.  Fused multiply-adds are written explicitly
 * (GC_FMA); the project builds with contraction off, and each written operation is one rounding below.
 *
 * Units: 1 u = 2^-53; RN(x) = x (1 + e), |e| <= u for every normal result.  "tiny" is below 2^-40 relative.
 *
 * ---- domain (gc_plan refuses a frame outside it; gc_hit reports a lane outside it as unsure) --------------------
 *   eye above the floor, A = RN(o.y - gy) in [2^-40, 2^20];  |o.x|, |o.z| <= 2^40;  |gy| <= 2^20;  limit > 0 or NaN (the scene files' planes: no limit);
 *   light (if lit) above the floor, h = RN(L.y - gy) in [2^-17, 2^20], |L.x|, |L.z| <= 2^40, and neither the eye's
 *   height nor |gy| above 16 h (the rounding of the hit height stays small against h: DY below);  the bitmap's scaling finite, nonzero, |s| in [2^-40, 2^40];
 *   m1 = |raw.x| + |raw.y| + |raw.z| in [2^-90, 2^90) per lane, so that |raw| in [m1 / sqrt 3, m1], sqmag(raw) lies far
 *   inside lean::'s window [2^-240, 2^240), normalize() yields finite components and the sign of d.y is raw.y's.
 *
 * ---- the reference's hit point -----------------------------------------------------------------------------------
 *   d = raw * inv, dn = d * inv2 (inv, inv2 the two rounded reciprocal lengths, common to x, y and z), so
 *   dn.x = raw.x inv inv2 (1+e1)(1+e2), dn.y = raw.y inv inv2 (1+e3)(1+e4), mult = A / -dn.y (1+e5) and
 *   RN(dn.x * mult) = X (1+e1)(1+e2)(1+e5)(1+e6) / ((1+e3)(1+e4)),  X = raw.x A / -raw.y as a real:
 *   the reciprocal lengths cancel.  Six roundings: within 6.01 u |X| of X.  p_ref.x = RN(o.x + that): one more, u |p_ref.x|.
 *   y: RN(dn.y * mult) = -A (1+e5)(1+e6'), and o.y - A = gy - (o.y - gy) eA, so
 *   |p_ref.y - gy| <= 3.02 u A + u |gy| (1 + tiny)  <=  BY = 3.1 u A + 1.01 u |gy|.
 *
 * ---- the short chain ---------------------------------------------------------------------------------------------
 *   r = gc_rcp(-raw.y) = 1 / -raw.y (1 + er), |er| <= 1.01 u (below); t = RN(A r); p'.x = RN(raw.x t + o.x) (one fma).
 *   p'.x = (X (1+er)(1+e7) + o.x)(1+e8), hence
 *   |p_ref.x - p'.x| <= (6.01 + 2.02) u |X| + u |p_ref.x| + u |p'.x| <= 10.1 u (|X| + |o.x|) <= 10.2 u (|p'.x| + 2 |o.x|)
 *   since |X| <= (|p'.x| + |o.x|)(1 + 3 u) — while no product underflows.  raw.x == 0 gives p.x = o.x on both sides, exactly
 *   (the pixel column under the eye: p.x * s is then often an integer, and the interval must not straddle it); with
 *   |raw.x| >= 2^-800 every product of either chain is normal; in between |X| <= |raw.x| 2^140 and both chains stay within
 *   |raw.x| 2^142 of o.x.  All three in one term, E0 = min(|raw.x| 2^150, 2^-650):
 *         |p_ref.x - p'.x|  <=  BX = 12 u (|p'.x| + 2 |o.x|) + E0,   BZ likewise
 *   (GC_KP = 12; 10.2 proven, the rest is slack for the three roundings of BX and for those of the tests that use it.)
 *   The light's bounds take one magnitude for both axes: Q = |p'.x| + |p'.z| + cq, cq >= 2 |o.x| + 2 |o.z| + |L.x| + |L.z| + 2^-100;
 *   Q as computed (two rounded additions) is at least Q (1 - 2 u), and BX, BZ <= 12 u Q =: BQ.
 *   gc_rcp: seed r0 = 1/b (1 + e0), |e0| <= 2^-20 (AMD's ISA manuals give v_rcp_f64 and v_rsq_f64 2^29 ulp, 2^-23; the host check perturbs
 *   an exact seed by up to that); e = RN(1 - b r0) is the fma's single rounding of ee = -e0, off by at most
 *   2^-73; r1 = RN(r0 + r0 (e + e^2)) = 1/b (1 - ee^3 + ..)(1 + u): |er| <= u + 2^-60 + 2^-72 <= 1.01 u.
 *
 * ---- decisions ---------------------------------------------------------------------------------------------------
 *   away (eye above): dn.y > -1e-9.  raw.y >= 0 gives dn.y >= 0 (or a zero): certainly away.  raw.y < 0 and
 *   -raw.y > 1.001e-9 m1 (m1 as computed, >= |raw| (1 - 2 u)) gives |dn.y| >= 1.001e-9 (1 - 10 u) > 1e-9: certainly
 *   hit, and |raw.y| >= 2^-120, a denominator gc_rcp and the parent's rcp_refined both accept.  Otherwise unsure.
 *   mult > 1e99 * len: mult <= 2^20 / 1e-9 (1 + tiny) and len = 1 + tiny: certainly false.
 *   |p.x| > limit: RN(|p'.x| + BX) < limit gives |p_ref.x| < limit (the slack of 1.8 u |p'.x| in BX exceeds the rounding of
 *   that sum); RN(|p'.x| - BX) > limit gives |p_ref.x| > limit; anything else is unsure.  A NaN limit (what a plane
 *   read from a scene file has) makes the reference's comparison false for every p: certainly inside (p' is finite).
 *   d.y < 0 (faceforward): true on every certainly-hit lane.
 *   test_visibility's pre-check: from_y = RN(p_ref.y + 1e-6) >= RN(gy - BY + 1e-6) > gy because BY < 2^-31 and an ulp
 *   of gy is at most 2^-33; raw_y = RN(L.y - from_y) >= h - 1.01e-6 - BY > 2^-18: rises; |lv.x|, |lv.z| < 2^42: sane.
 *   Certain for the whole frame (gc_plan).
 *
 * ---- texture ------------------------------------------------------------------------------------------------------
 *   (float)(a - floor(a)), a = RN(p s): f32_certain.h's uv_float_certain argument, with U = p'.x, delta = BX: equal
 *   floors and equal floats at RN(U - BX) and RN(U + BX) are the floor and the float of every double between them.
 *
 * ---- light --------------------------------------------------------------------------------------------------------
 *   reference: lv = L - p_ref (three rounded differences), r2 = RN(RN(lv.x^2 + lv.y^2) + lv.z^2) with rounded squares,
 *   len = RN(sqrt r2), rinv = RN(1 / len), cosTheta = RN(lv.y rinv) (faceforward leaves the normal (0, 1, 0)).
 *   short: lvx' = RN(L.x - p'.x), lvz' likewise, h for lv.y, r2' = fma(lvx', lvx', fma(lvz', lvz', RN(h h))).
 *   |lv.x - lvx'| <= BQ + u |lv.x| + u |lvx'| <= 14.1 u Q  (|lvx'| <= (|L.x| + |p'.x|)(1 + u) <= Q (1 + 4 u)).
 *   |lv.y - h| <= BY + 2.01 u h <= (3.1 * 16 + 1.01 * 16 + 2.01) u h < DY = 68 u h  (A, |gy| <= 16 h: gc_plan).
 *   Squares: sum over x, z of 2 |lv'| d + d^2 <= 56.5 u Q^2; y: 2 h DY + DY^2 <= 2.01 h DY.  Roundings: three each
 *   side, 3 u r2 + 3 u r2'.  Together
 *         |r2 - r2'| <= B = 6.1 u r2' + E,   E = 58 u Q^2 + CY,   CY = 138 u RN(h h)  (2.02 * 68 = 137.4).
 *   (float)r2: certain when (float)RN(r2' - B) == (float)RN(r2' + B); base_light reads nothing else of r2.
 *   gc_rsq: seed y0 = x^-1/2 (1 + e0), |e0| <= 2^-20; t = RN(x y0), e = RN(1 - t y0) = ee + eta with ee = 1 - x y0^2,
 *   |eta| <= 1.01 u; x^-1/2 = y0 (1 + ee/2 + 3 ee^2/8 + 5 ee^3/16 + ..), y1 = RN(y0 + y0 RN(RN(0.5 + 0.375 e) e)):
 *   y1 = x^-1/2 (1 + ey), |ey| <= u + 0.505 u + 5/16 2^-57 + tiny <= 1.6 u.
 *   cosTheta' = RN(h y1) = h r2'^-1/2 (1 + 2.61 u); reference: lv.y r2^-1/2 (1 + 3.02 u) with lv.y = h (1 + DY/h) and
 *   r2^-1/2 = r2'^-1/2 (1 + 0.501 B / r2') for B / r2' <= 2^-20.  1 / r2' <= y1^2 (1 + 4 u).  So
 *         |cosTheta - cosTheta'| <= cosTheta' REL,   REL = CU + 0.504 E y1^2,   CU = 79 u  (DY / h + 10.2 u = 78.2 u),
 *   provided REL < 2^-22 (which gives E / r2' < 2^-21 and B / r2' < 2^-20); REL >= 2^-22 is unsure.  cosTheta > 0 holds
 *   on both sides: h > 0, lv.y >= h (1 - 68 u) > 0, no product underflows.  (float)cosTheta: certain when the
 *   floats of RN(c' - c' REL) and RN(c' + c' REL) agree.
 */
#ifndef C2RT_GROUND_CERTAIN_H
#define C2RT_GROUND_CERTAIN_H

#include <math.h>

#if defined(__HIPCC__)
#define GC_FN static __host__ __device__ __forceinline__
#else
#define GC_FN static inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define GC_FMA(a, b, c) __builtin_fma((a), (b), (c))
#define GC_RCP_SEED(b) __builtin_amdgcn_rcp(b)
#define GC_RSQ_SEED(x) __builtin_amdgcn_rsq(x)
#else
#define GC_FMA(a, b, c) fma((a), (b), (c))
/* host: seeds off by GC_SEED_SCALE - 1, which the check program sets (a variable of its own) anywhere within 2^-20 */
#ifndef GC_SEED_SCALE
#define GC_SEED_SCALE (1.0 + 0x1p-24)
#endif
#define GC_RCP_SEED(b) ((1.0 / (b)) * (GC_SEED_SCALE))
#define GC_RSQ_SEED(x) ((1.0 / sqrt(x)) * (GC_SEED_SCALE))
#endif

#define GC_U 0x1p-53
#define GC_KP 12.0  /* BX = GC_KP u (|p'.x| + 2 |o.x|) + E0 <= GC_KP u Q */
#define GC_KQ2 58.0 /* E = GC_KQ2 u Q^2 + CY */
#define GC_KR2 6.1  /* B = GC_KR2 u r2' + E */
#define GC_KH 16.0  /* the eye's height and |gy| are at most GC_KH h */
#define GC_KCY 138.0
#define GC_KCU 79.0

/* what gc_hit says of a lane */
enum { GC_HIT = 0, GC_MISS = 1, GC_UNSURE = 2 };

/* What a frame's samples share.  cq is the one constant the host hands over (RenderParams::ground_certain_cq, a
 * float rounded UP: gc_plan); h = RN(L.y - gy) and h2 = RN(h h) are evaluated where they are used. */
typedef struct {
    double cq;    /* >= 2 |o.x| + 2 |o.z| + |L.x| + |L.z| + 2^-100 */
    double h, h2; /* 0 without a light that shines */
} gc_frame;

/* 1 / b (1 + er), |er| <= 1.01 u, for 2^-120 <= |b| < 2^120 */
GC_FN double gc_rcp(double b)
{
    const double r0 = GC_RCP_SEED(b);
    const double e = GC_FMA(-b, r0, 1.0);
    const double p = GC_FMA(e, e, e);
    return GC_FMA(r0, p, r0);
}

/* x^-1/2 (1 + ey), |ey| <= 1.6 u, for 2^-200 <= x < 2^200 */
GC_FN double gc_rsq(double x)
{
    const double y0 = GC_RSQ_SEED(x);
    const double t = x * y0;
    const double e = GC_FMA(-t, y0, 1.0);
    const double p = GC_FMA(e, 0.375, 0.5);
    const double pe = p * e;
    return GC_FMA(y0, pe, y0);
}

/* Does the frame lie in the domain?  o: the eye; gy, limit: the ground plane; lit: a light whose intensity is not zero
 * reaches the floor's shade, L its position; textured: a bitmap floor with scaling s.  Returns cq as a float that is not
 * below it (> 0), or 0 for a frame outside the domain (a NaN anywhere fails a comparison). */
GC_FN float gc_plan(const double o[3], double gy, double limit, int lit, const double L[3], int textured, double s)
{
    const double A = o[1] - gy;
    if (!((A >= 0x1p-40) & (A <= 0x1p20) & (fabs(o[0]) <= 0x1p40) & (fabs(o[2]) <= 0x1p40) & (fabs(gy) <= 0x1p20) & !(limit <= 0))) return 0;
    if (textured && !((fabs(s) >= 0x1p-40) & (fabs(s) <= 0x1p40))) return 0;
    double cq = 2 * fabs(o[0]) + 2 * fabs(o[2]) + 0x1p-100;
    if (lit) {
        const double h = L[1] - gy;
        if (!((h >= 0x1p-17) & (h <= 0x1p20) & (fabs(L[0]) <= 0x1p40) & (fabs(L[2]) <= 0x1p40) & (A <= GC_KH * h) & (fabs(gy) <= GC_KH * h))) return 0;
        cq += fabs(L[0]) + fabs(L[2]);
    }
    return (float)(cq * (1 + 0x1p-20)); /* the conversion rounds by 2^-24 at most */
}

/* a frame's shared values from cq and, with a light that shines, its height ly */
GC_FN gc_frame gc_frame_of(double cq, int lit, double ly, double gy)
{
    gc_frame f;
    f.cq = cq;
    f.h = lit ? ly - gy : 0.0;
    f.h2 = f.h * f.h;
    return f;
}

/* The plane hit of the screen ray raw from the eye (ox, ., oz), A = RN(o.y - gy) above the floor.
 * GC_HIT: *px, *pz within *bx, *bz of the reference's p.x, p.z, and inside `limit`; GC_MISS: the reference's ray certainly
 * misses (points away, or lands beyond limit); GC_UNSURE otherwise.  *q: Q as computed (gc_light's bounds read it). */
GC_FN int gc_hit(double ox, double oz, double A, double rx, double ry, double rz, double cq, double limit,
                 double *px, double *pz, double *bx, double *bz, double *q)
{
    const double m1 = fabs(rx) + fabs(ry) + fabs(rz);
    const int win = (m1 >= 0x1p-90) & (m1 < 0x1p90); /* false for NaN */
    const int away = ry >= 0;
    const int hit = -ry > 1.001e-9 * m1;
    const double t = A * gc_rcp(-ry);
    *px = GC_FMA(rx, t, ox);
    *pz = GC_FMA(rz, t, oz);
    const double ax = fabs(*px), az = fabs(*pz);
    *bx = GC_FMA(ax, GC_KP * GC_U, GC_FMA(fabs(ox), 2 * GC_KP * GC_U, fmin(fabs(rx) * 0x1p150, 0x1p-650)));
    *bz = GC_FMA(az, GC_KP * GC_U, GC_FMA(fabs(oz), 2 * GC_KP * GC_U, fmin(fabs(rz) * 0x1p150, 0x1p-650)));
    *q = ax + az + cq;
    const int in = !((ax + *bx >= limit) | (az + *bz >= limit)); /* (true for a NaN limit) */
    const int out = (ax - *bx > limit) | (az - *bz > limit);
    if (!win) return GC_UNSURE;
    if (away) return GC_MISS;
    if (!hit) return GC_UNSURE;
    return in ? GC_HIT : (out ? GC_MISS : GC_UNSURE);
}

/* BitmapTexture.getTexColor's float of one coordinate, (float)(a - floor(a)) with a = RN(p s), for the reference's p
 * anywhere within b of pp: true and *out set where it is certain. */
GC_FN int gc_tex_float(double pp, double b, double s, float *out)
{
    const double a0 = (pp - b) * s, a1 = (pp + b) * s;
    const double f0 = floor(a0), f1 = floor(a1);
    const float x0 = (float)(a0 - f0), x1 = (float)(a1 - f1);
    *out = x0;
    return (f0 == f1) & (x0 == x1);
}

/* The light's two floats at a GC_HIT lane: (float)r2 and (float)cosTheta (which is > 0), certain where this returns
 * true.  lx, lz: the light's position; px, pz, q: from gc_hit.  dbg (the check program's; the kernels pass locals
 * nobody reads): r2', B, cosTheta' and its bound. */
GC_FN int gc_light(double px, double pz, double q, double lx, double lz, const gc_frame *f, float *r2f, float *cosf, double dbg[4])
{
    const double lvx = lx - px, lvz = lz - pz;
    const double r2 = GC_FMA(lvx, lvx, GC_FMA(lvz, lvz, f->h2));
    const double E = GC_FMA(q * q, GC_KQ2 * GC_U, f->h2 * (GC_KCY * GC_U));
    const double B = GC_FMA(r2, GC_KR2 * GC_U, E);
    const float lo = (float)(r2 - B), hi = (float)(r2 + B);
    const double y1 = gc_rsq(r2);
    const double c = f->h * y1;
    const double rel = GC_FMA(E * (y1 * y1), 0.504, GC_KCU * GC_U);
    const double bc = c * rel;
    const float clo = (float)(c - bc), chi = (float)(c + bc);
    dbg[0] = r2;
    dbg[1] = B;
    dbg[2] = c;
    dbg[3] = bc;
    *r2f = lo;
    *cosf = clo;
    return (lo == hi) & (rel < 0x1p-22) & (clo == chi);
}

#endif /* C2RT_GROUND_CERTAIN_H */
