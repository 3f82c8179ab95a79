/*
 * csg_certain.h — which hit a leaf CsgOp reports for one ray, decided from the closed-form intervals of its two
 * children wherever that decision is CERTAIN to be the one the reference's stepped lists give.
 *
 * The reference (CsgOp.intersect, rt/geometry.d:292-332; csg_intersect_leaf in c2rt_trace.inc) finds every hit of each
 * child by stepping — intersect, restart 1e-6 behind the hit, intersect again, until a miss —, sorts both lists and walks
 * them with two in/out toggles; the first entry after which the operator is on wins.  All of that produces a DECISION —
 * no hit, or "hit k of child `side`" — plus that one hit's record.  As in f32_certain.h and ground_certain.h: compute the
 * cheap way with a bound, keep the decision only where every value inside the bound gives the same one, and report
 * `unsure` otherwise.  The caller produces the record itself with the literal primitive code on the literal operands (so
 * its bits are the reference's by construction) and runs the literal evaluation for an unsure lane.  Plain arithmetic,
 * host and device; tests/csg_certain_check.cpp is the host build, tests/test_csg_certain_host.py holds every certain
 * answer to the literal lists of tests/geom_reference.py.
 *
 * Serves a CsgOp (Union, Inter, Diff) whose children are two DISTINCT primitives, each a Sphere or a finite Cube (the
 * planner's flag kCsgCertain, scene_plan.cpp: csg_certain_ok, which also bounds the geometry: every centre coordinate
 * within 2^20, radius / side in [2^-10, 2^20]).  The ray is the object-space ray csg_intersect_leaf receives: origin o,
 * direction d with |d| = 1 up to a few ulp.  A lane whose origin lies beyond 2^24 (1-norm), or with a non-finite
 * operand, is unsure (every test below is written so that a NaN makes it false).
 *
 * `ms` scales every margin: 1 in the product, 0 in the test that shows the ray sets can fail.
 *
 * ---- a child's list: four classes -----------------------------------------------------------------------------------
 *   EMPTY   the stepping finds nothing;
 *   TWO     exactly two hits, recorded within `del` of the interval's ends a0 < a1;
 *   ONE     exactly one hit (the origin inside), recorded within `del` of the exit a1;
 *   UNSURE  anything else.
 * What the restarts do to a recorded distance: the second hit is found from p0 + d 1e-6 and its own distance added to the
 * first's, so it comes out up to 1e-6 short of a1 (the step itself is not added back).  del carries 4e-6 for that, which
 * is four steps where at most one happens.
 *
 * Sphere (c, R).  H = o - c, b = H.d, C = |H|^2 - R^2, disc = b^2 - C (a quarter of the reference's discriminant for
 * A = |d|^2 = 1), h = sqrt(disc) the half chord, roots -b -+ h.
 *   E2 = 2^-44 (|H|^2 + R^2): every rounding of b^2, C and disc, in this chain and in the reference's (B = 2b, 4AC, the
 *   node offset's subtraction, |d|^2 = 1 +- 4u) is a few ulp of |H|^2 + R^2 — at most 20 u; E2 is 512 u.
 *   m = 3e-5, M2 = 2 R m + m^2: a point with C > M2 + E2 is more than m outside the ball, with C < -(M2 + E2) more than m
 *   inside (up to m^2).
 *   EMPTY: disc < -(M2 + E2) — the ray passes more than m outside, the reference's discriminant is negative —; or the
 *   origin outside by m and b > 0 (moving away): both roots are negative.  The reference then either leaves through its
 *   own shortcut (Dscr < BB (1 - 1e-8)) or evaluates the roots, and (-B + sq) / 2A is negative unless BB - 4AC rounds to
 *   BB; C > 2^-45 b^2 keeps 4AC above an ulp of BB (and the square root's rounding) by a factor 2^7.
 *   TWO: the origin outside by m, b < 0, h > hmin = 1e-3 + 4e6 E2.  First call: both roots positive, the near one
 *   reported.  The restart 1e-6 along d moves the origin INSIDE by 2 h 1e-6 in C (dC/dt = 2 b = -2h at the entry), against
 *   an uncertainty of the recorded point of a few E2 (the root's error E2 / h along the ray changes C by 2 h times that;
 *   the point's and C's own roundings are below E2): 2 h 1e-6 > 8 E2.  Second call: C < 0 certainly, the near root is
 *   negative, the far one, 2h - 1e-6, reported.  Third call: outside by the same 2 h 1e-6, moving away at b = h: EMPTY's
 *   argument, with 4AC = 8 h 1e-6 against an ulp of 4 h^2: h < 2^30, which the domain gives.
 *   ONE: the origin inside by m (then h >= sqrt(2 R m) already), h > hmin: the far root, then the third call's argument.
 *   del = 4e-6 + 2^-38 (|b| + h) + 2 E2 / h: restarts; the refined square root (2^-40 relative, CC_RSQ) and the
 *   reference's division; the discriminant's error through the root.
 *
 * Cube [lo, hi] (the planner's face planes, DevGeom::q).  Slab parameters tn_i <= tf_i per axis, a0 = max tn (axis e),
 * a1 = min tf (axis x).  Every |d_i| must exceed 1e-6 (the reference skips an axis pair below 1e-9; near that threshold,
 * and for a ray nearly parallel to a face, nothing is claimed): all six faces are candidates of every call.
 *   Ept = 2^-48 S1, S1 = |o|_1 + the box's largest coordinates: 32 ulp of any coordinate that occurs — a candidate's point
 *   o + d mult, a numerator o_i - face.  mp = 3e-5 + 2^10 Ept is the margin in POINT space.  A gap in t says nothing
 *   for a grazing ray: all conditions are distances of points from planes.
 *   What decides a call (rt/geometry.d:198-235): a face candidate is taken iff its mult >= 0 and its point lies within
 *   the other two slabs; the smallest mult wins.  A candidate on face plane j at t_j:
 *    - t_j in (a0, a1) is impossible (inside the box the ray crosses no face plane);
 *    - t_j <= a0, j not e: the entry point lies more than mp inside slab j (the edge condition, below), so t_j is at
 *      least mp / |d_j| >= mp before a0 and the candidate's point more than |d_e| mp outside slab e: rejected, whatever
 *      the sign of a tiny mult — provided |d_e| mp is above the rounding, which the restart condition gives with a
 *      factor 100;  t_j >= a1, j not x: likewise outside slab x.
 *   TWO: a0 < a1; the origin more than mp outside slab e (a0 |d_e| > mp: the entry candidate's mult is positive); the
 *   entry point more than mp inside both other slabs and the exit point likewise (no edge, no corner, and the chord's
 *   extent along some axis exceeds mp); 1e-6 |d_e| > 4 Ept and 1e-6 |d_x| > 4 Ept: the restart certainly lands beyond the
 *   face it left.  First call: the entry face wins.  Second call: the origin is inside slab e by 1e-6 |d_e|, more than
 *   mp - 1e-6 inside the others: the entry face's numerator has the sign that makes mult negative, the exit face is
 *   taken.  Third call: the origin beyond face x and moving away: Cube.intersect returns false exactly (c2rt_trace.inc,
 *   the comment on the rejected early-out).
 *   ONE: the origin more than mp inside every slab — taken from the parameters alone: the faces behind the origin lie at
 *   |tn_i| |d_i| >= |a0| dmin, those ahead at tf_i |d_i| >= a1 dmin (dmin = min |d_i|), so a0 dmin < -mp and a1 dmin > mp
 *   suffice, with no operand the other classes do not have already (a form with the six differences o_i - face cost the
 *   frame kernel the registers it has left) —; the exit point's edge condition and restart condition.  The argument is
 *   TWO's from its second call on: the faces behind the origin have the numerator sign that makes mult negative, by mp.
 *   EMPTY: a0 > a1 and min(|d_e|, |d_x|) (a0 - a1) / 2 > mp — a candidate at t <= (a0 + a1) / 2 lies that far outside
 *   slab e, a later one outside slab x; the candidates of axis e itself have t >= a0 (outside x by |d_x| (a0 - a1)),
 *   those of x t <= a1 —; or a1 < 0 and |d_x| (-a1) > mp: a candidate with t >= 0 (or a rounding below it) lies that far
 *   outside slab x, every other one is behind the origin.
 *   del = 4.3e-6 + 2^-38 (|a0| + |a1|): restarts; the numerator's rounding over |d|, below 2.5e-7 by the restart
 *   condition; the refined reciprocal (2^-40 relative, CC_RCP) against the reference's division.
 *   As evaluated, |d_e| and |d_x| are both replaced by dmin = min |d_i| (every condition above only gets harder), and
 *   "the other two slabs" by the middle one of the three inside-distances of the point (the smallest is the face's own,
 *   zero up to rounding): no axis index is tracked — the frame kernel has no registers to spare where this runs.
 *
 * ---- the walk -------------------------------------------------------------------------------------------------------
 * At most four events.  Two events of different children must be further apart than the sum of their bounds, else
 * unsure (a tie, or an order the sort could see either way).  Each child's own events are in order by construction.
 * inL / inR start as "list length odd" (ONE); event k of a child toggles its state k + 1 times from the start, and the
 * other child's state as often as that child has events in front of it; the winner is the nearest event after which
 * the operator is on — rt/geometry.d:303-329 literally, on certain inputs.  Its index k in its child's list is what
 * the caller's stepping loop needs: 0 for the only hit of a ONE child.
 */
#ifndef C2RT_CSG_CERTAIN_H
#define C2RT_CSG_CERTAIN_H

#include <math.h>

#if defined(__HIPCC__)
#define CC_FN static __host__ __device__ __forceinline__
#else
#define CC_FN static inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define CC_RCP_SEED(b) __builtin_amdgcn_rcp(b)
#define CC_RSQ_SEED(x) __builtin_amdgcn_rsq(x)
#define CC_FMA(a, b, c) __builtin_fma((a), (b), (c))
#else
/* host: seeds off by CC_SEED_SCALE - 1 (the device's are within 2^-20) */
#ifndef CC_SEED_SCALE
#define CC_SEED_SCALE (1.0 + 0x1p-24)
#endif
#define CC_RCP_SEED(b) ((1.0 / (b)) * (CC_SEED_SCALE))
#define CC_RSQ_SEED(x) ((1.0 / sqrt(x)) * (CC_SEED_SCALE))
#define CC_FMA(a, b, c) fma((a), (b), (c))
#endif

namespace c2rt {

enum { CC_EMPTY = 0, CC_ONE = 1, CC_TWO = 2, CC_UNSURE = 3 };
enum { CC_R_UNSURE = 0, CC_R_NOHIT = 1, CC_R_HIT = 2 };
enum { CC_OP_UNION = 0, CC_OP_INTER = 1, CC_OP_DIFF = 2 };

constexpr double kCcM = 3e-5;        /* m: margin of a point against a surface */
constexpr double kCcE2 = 0x1p-44;    /* E2 / (|H|^2 + R^2) */
constexpr double kCcHmin = 1e-3;     /* half chord: absolute part */
constexpr double kCcHE2 = 4e6;       /* ... and per E2: 2 h 1e-6 > 8 E2 */
constexpr double kCcSafeC = 0x1p-45; /* |C| against b^2 */
constexpr double kCcDmin = 1e-6;     /* every |d_i| of a cube's ray */
constexpr double kCcEpt = 0x1p-48;   /* Ept / S1 */
constexpr double kCcStep = 4e-6;     /* restarts, in del */
constexpr double kCcRel = 0x1p-38;   /* relative part of del */
constexpr double kCcOmax = 0x1p24;   /* |o|_1 */

struct CcChild {
    int st;            /* CC_EMPTY / ONE / TWO / UNSURE */
    double a0, a1;     /* TWO: both; ONE: a1 */
    double del;
};

struct CcResult {
    int kind;          /* CC_R_UNSURE / NOHIT / HIT */
    int side, k;       /* HIT: the child (0 left, 1 right) and the index of the hit in its list */
    double dist, del;  /* HIT: the recorded distance is within del of dist */
};

CC_FN double cc_abs(double x) { return x < 0 ? -x : x; }
CC_FN double cc_min(double a, double b) { return a < b ? a : b; }
CC_FN double cc_max(double a, double b) { return a > b ? a : b; }

/* 1 / b within 2^-39 relative: one Newton step on a seed within 2^-20 */
CC_FN double cc_rcp(double b)
{
    const double r0 = CC_RCP_SEED(b);
    return CC_FMA(CC_FMA(-b, r0, 1.0), r0, r0);
}

/* sqrt(x), x > 0, within 2^-39 relative; *y: 1 / sqrt(x) within 2^-19 */
CC_FN double cc_sqrt(double x, double *y)
{
    const double y0 = CC_RSQ_SEED(x);
    const double h0 = x * y0;
    *y = y0;
    return CC_FMA(0.5 * y0, CC_FMA(-h0, h0, x), h0);
}

CC_FN CcChild cc_sphere(const double o[3], const double d[3], const double c[3], double R, double ms)
{
    CcChild r;
    const double H0 = o[0] - c[0], H1 = o[1] - c[1], H2 = o[2] - c[2];
    const double b = H0 * d[0] + H1 * d[1] + H2 * d[2];
    const double hh = H0 * H0 + H1 * H1 + H2 * H2;
    const double R2 = R * R;
    const double C = hh - R2;
    const double disc = b * b - C;
    const double E2 = ms * kCcE2 * (hh + R2);
    const double m = ms * kCcM;
    const double M = 2 * R * m + m * m + E2;
    double y;
    const double h = cc_sqrt(disc, &y);
    const double hmin = ms * (kCcHmin + kCcHE2 * E2);
    const bool dom = hh < kCcOmax * kCcOmax;
    const bool out = C > M, in = C < -M;
    const bool big = (disc > 0) & (h > hmin);
    const bool safe = cc_abs(C) > ms * kCcSafeC * (b * b);
    const bool empty = (disc < -M) | (out & (b > 0) & safe);
    const bool two = out & (b < 0) & big;
    const bool one = in & big;
    r.st = !dom ? CC_UNSURE : (empty ? CC_EMPTY : (two ? CC_TWO : (one ? CC_ONE : CC_UNSURE)));
    r.a0 = -b - h;
    r.a1 = -b + h;
    r.del = ms * (kCcStep + kCcRel * (cc_abs(b) + h) + 2 * E2 * y * (1 + 0x1p-18));
    return r;
}

/* the middle one of three */
CC_FN double cc_mid3(double a, double b, double c) { return cc_max(cc_min(a, b), cc_min(cc_max(a, b), c)); }

/* rinv: null, or the three reciprocals 1 / d[i] within 2^-39 relative, where the caller has them */
CC_FN CcChild cc_cube(const double o[3], const double d[3], const double lo[3], const double hi[3], double ms, const double *rinv = nullptr)
{
    CcChild r;
    double a0 = -1e300, a1 = 1e300, dmin = 1e300, S1 = 0;
    for (int i = 0; i < 3; ++i) {
        dmin = cc_min(dmin, cc_abs(d[i]));
        const double ri = rinv ? rinv[i] : cc_rcp(d[i]);
        const double t1 = (lo[i] - o[i]) * ri, t2 = (hi[i] - o[i]) * ri;
        a0 = cc_max(a0, cc_min(t1, t2));
        a1 = cc_min(a1, cc_max(t1, t2));
        S1 += cc_abs(o[i]) + cc_max(cc_abs(lo[i]), cc_abs(hi[i]));
    }
    const double Ept = ms * kCcEpt * S1;
    const double mp = ms * kCcM + 4096 * Ept;
    /* how far the entry point and the exit point lie inside each slab; the smallest of the three is the face's own,
     * zero up to rounding: the middle one is the distance from the nearest edge */
    double q0[3], q1[3];
    for (int i = 0; i < 3; ++i) {
        const double p0 = CC_FMA(d[i], a0, o[i]), p1 = CC_FMA(d[i], a1, o[i]);
        q0[i] = cc_min(p0 - lo[i], hi[i] - p0);
        q1[i] = cc_min(p1 - lo[i], hi[i] - p1);
    }
    const double qe = cc_mid3(q0[0], q0[1], q0[2]), qx = cc_mid3(q1[0], q1[1], q1[2]);
    const bool dom = (dmin > ms * kCcDmin) & (S1 < kCcOmax);
    const bool step = 1e-6 * dmin > 4 * Ept;
    const bool two = (a0 < a1) & (a0 * dmin > mp) & (qe > mp) & (qx > mp) & step;
    const bool one = (a0 * dmin < -mp) & (a1 * dmin > mp) & (qx > mp) & step;
    const bool empty = ((a0 > a1) & (dmin * (a0 - a1) * 0.5 > mp)) | ((a1 < 0) & (dmin * -a1 > mp));
    r.st = !dom ? CC_UNSURE : (empty ? CC_EMPTY : (two ? CC_TWO : (one ? CC_ONE : CC_UNSURE)));
    r.a0 = a0;
    r.a1 = a1;
    r.del = ms * (kCcStep + 3e-7 + kCcRel * (cc_abs(a0) + cc_abs(a1)));
    return r;
}

CC_FN bool cc_op(int op, bool inL, bool inR) { return op == CC_OP_UNION ? (inL | inR) : (op == CC_OP_INTER ? (inL & inR) : (inL & !inR)); }

/* the walk over two certain lists (neither UNSURE) */
CC_FN CcResult cc_walk(int op, const CcChild &L, const CcChild &R)
{
    CcResult w;
    w.kind = CC_R_NOHIT;
    w.side = 0;
    w.k = 0;
    w.dist = 0;
    w.del = 0;
    /* events: [0], [1] the left child's first and second, [2], [3] the right child's */
    const CcChild *ch[2] = {&L, &R};
    double ed[4];
    bool ep[4];
    for (int s = 0; s < 2; ++s) {
        const int st = ch[s]->st;
        ed[2 * s] = st == CC_TWO ? ch[s]->a0 : ch[s]->a1;
        ed[2 * s + 1] = ch[s]->a1;
        ep[2 * s] = st != CC_EMPTY;
        ep[2 * s + 1] = st == CC_TWO;
    }
    const double sep = L.del + R.del;
    bool sure = true, have = false;
    double best = 1e300;
    for (int i = 0; i < 4; ++i) {
        const int s = i >> 1, k = i & 1, t = 1 - s;
        int before = 0; /* events of the other child in front of this one */
        for (int j = 0; j < 2; ++j) {
            const double gap = ed[i] - ed[2 * t + j];
            const bool both = ep[i] & ep[2 * t + j];
            sure = sure & (!both | (gap > sep) | (gap < -sep));
            before += (both & (gap > 0)) ? 1 : 0;
        }
        const bool in_s = (ch[s]->st == CC_ONE) ^ (((k + 1) & 1) != 0);
        const bool in_t = (ch[t]->st == CC_ONE) ^ ((before & 1) != 0);
        const bool on = cc_op(op, s == 0 ? in_s : in_t, s == 0 ? in_t : in_s);
        if (ep[i] & on & (ed[i] < best)) {
            best = ed[i];
            have = true;
            w.side = s;
            w.k = k;
            w.del = ch[s]->del;
        }
    }
    w.dist = best;
    w.kind = !sure ? CC_R_UNSURE : (have ? CC_R_HIT : CC_R_NOHIT);
    return w;
}

/* The whole decision, staged: a certainly empty left child under short_a (Inter / Diff) answers before the right child
 * is looked at, a certainly empty right child under short_b (Inter) likewise (GeomFlags: kCsgShortA / B).  left() and
 * right() classify a child (the device reads the child's record there, with scalar loads; the host build has it in
 * memory). */
template <class FL, class FR>
CC_FN CcResult cc_decide_with(int op, bool short_a, bool short_b, FL left, FR right)
{
    CcResult w;
    w.kind = CC_R_UNSURE;
    w.side = w.k = 0;
    w.dist = w.del = 0;
    const CcChild L = left();
    if (L.st == CC_UNSURE) return w;
    if (L.st == CC_EMPTY && short_a) { w.kind = CC_R_NOHIT; return w; }
    const CcChild R = right();
    if (R.st == CC_UNSURE) return w;
    if (R.st == CC_EMPTY && short_b) { w.kind = CC_R_NOHIT; return w; }
    return cc_walk(op, L, R);
}

/* One primitive child from its parameters: a Sphere (p: centre, R) or a Cube (q: lo, hi; DevGeom::q) */
CC_FN CcChild cc_child(bool is_sphere, const double o[3], const double d[3], const double *p, const double *q, double ms)
{
    if (is_sphere) return cc_sphere(o, d, p, p[3], ms);
    return cc_cube(o, d, q, q + 3, ms);
}

CC_FN CcResult cc_decide(int op, bool short_a, bool short_b, bool l_sphere, const double *lp, const double *lq, bool r_sphere,
                         const double *rp, const double *rq, const double o[3], const double d[3], double ms)
{
    return cc_decide_with(op, short_a, short_b, [&] { return cc_child(l_sphere, o, d, lp, lq, ms); },
                          [&] { return cc_child(r_sphere, o, d, rp, rq, ms); });
}

} // namespace c2rt

#endif
