/*
 * csg_void.h — per-tile "void" test for a CsgDiff(L, Sphere) node, and silhouette test for a Sphere node (further
 * down): the tile's rays provably get no hit on it.  Shared by the mask pre-pass (c2rt_tile_mask.inc: tile_mask_entry),
 * the host that fills VoidCull and SphereCull (c2rt_api.cpp: prepare_tile_masks) and the host check libraries of the
 * tests (tests/csg_void_check.cpp, tests/sphere_cull_check.cpp).
 *
 * Why a void ray gets no hit: CsgOp.intersect for Diff(L, R) (rt/geometry.d:292-332), R a Sphere.  Suppose that
 * for one ray (1) findAllIntersections(R) yields exactly two hits R0 < R1, or one hit R1 with the origin inside
 * the sphere, and (2) every hit of L, however many (grazing included), has a distance strictly inside (R0, R1)
 * (resp. (0, R1)).  The walk starts with inR = (|R| odd): false before R0 / true from the origin; the first sorted
 * event is R0 (or an L event while inR is already true), so inR is true at every L event and boolOp = inL && !inR
 * stays false.  At R1 inL has been flipped |L| times from (|L| odd), so it is false, and the walk ends with no hit.
 * No tie and no leaf-identity question arises: the L distances lie strictly between the R events.
 *
 * Sufficient condition for a whole tile: every point of box(L) inside the set the tile's rays sweep lies in the
 * ball B(c, R - m).  Every L hit point is in box(L) (the padded world box, c2rt_api.cpp) on one of the rays, so it
 * lies at least m inside the sphere, and the ray passes at least sqrt(2 R m) inside the sphere's rim: R0 and R1
 * are far from a tangent, and the three 1e-6 steps of findAllIntersections (which shorten the recorded distances
 * by at most 3e-6) and fp64 rounding of the distances (relative 1e-15 at the scene's scale, amplified by at most
 * scale / sqrt(2 R m)) keep every L distance strictly between R0 and R1.  m = 1e-5 + 1e-6 * scale covers both
 * with orders of magnitude to spare (void_margin).
 *
 * The swept set is a pyramid {apex + sum_k s_k dir_k, s_k >= 0} with four edge directions in cyclic order:
 *  - primary rays: apex = eye, edges = the tile's corner rays widened by 1 px (the AA taps reach 0.6 px), exactly
 *    the rays of the ground footprint (tile_mask_entry);
 *  - shadow rays towards light 0 of a ground tile: they start within 1e-6 of the tile's footprint quad on the
 *    ground and end at the light; the pyramid with apex = light through the padded footprint rectangle holds
 *    them up to the light.  Beyond the light a shadow ray is outside that pyramid — its L hits there would break
 *    the parity in (2) — so the shadow test requires the box to lie strictly on the ground's side of the light's
 *    height (VoidNode::flags bit 1, host), where no ray continues after passing the light.
 * box ∩ pyramid is bounded by a thick segment around the pyramid's axis (pyramid_void), which must lie in the ball.
 */
#ifndef C2RT_CSG_VOID_H
#define C2RT_CSG_VOID_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define C2RT_VOID_FN __host__ __device__ inline
#else
#define C2RT_VOID_FN inline
#endif

namespace c2rt {

constexpr int kMaxVoidNodes = 4; /* CsgDiff(L, Sphere) nodes tested per frame (the first ones among the culled) */

struct VoidNode {
    double lo[3], hi[3];           /* padded world box of the node (node_box: identity matrix => axis-aligned) */
    double c[3];                   /* the subtracted sphere's world centre (object centre + node offset) */
    double r2;                     /* (R - m)^2, m = void_margin */
    uint32_t node;                 /* node index (< kMaxCullNodes) */
    uint32_t flags;                /* bit 0: primary test; bit 1: shadow test towards light 0 (see above) */
};

/* the per-frame argument of the mask pre-pass (tile_masks_kernel) */
struct VoidCull {
    uint32_t n, pad;
    double light0[3];              /* light 0 (the shadow pyramid's apex) */
    VoidNode v[kMaxVoidNodes];
};

C2RT_VOID_FN double void_abs(double x) { return x < 0 ? -x : x; }

/* margin of the ball for coordinates of magnitude up to `scale` (sum of |centre|, R, |eye|, |light| max-norms) */
C2RT_VOID_FN double void_margin(double scale) { return 1e-5 + 1e-6 * scale; }

/* The circular cone around a pyramid (apex, dir[0..3]): u = the pyramid's axis (unit: the normalised sum of the unit
 * edges), tan_t = max over the four edges of lateral / axial component.  The cone of that half angle around u is
 * convex and holds the four edges, hence the pyramid.  ok = false for a pyramid of 90 degrees or more (an edge with
 * axial component <= 0, or non-finite edges): every test refuses.  A tile computes it once per pyramid. */
struct PyramidCone {
    double u[3];
    double tan_t;
    bool ok;
};

C2RT_VOID_FN PyramidCone pyramid_cone(const double dir[4][3])
{
    PyramidCone k;
    double u[3] = {0, 0, 0};
    for (int e = 0; e < 4; ++e) {
        const double l2 = dir[e][0] * dir[e][0] + dir[e][1] * dir[e][1] + dir[e][2] * dir[e][2];
        const double il = 1.0 / sqrt(l2);
        for (int i = 0; i < 3; ++i) u[i] += dir[e][i] * il;
    }
    {
        const double il = 1.0 / sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        for (int i = 0; i < 3; ++i) u[i] *= il;
    }
    double tan_t = 0;
    bool ok = true;
    for (int e = 0; e < 4; ++e) {
        const double a = dir[e][0] * u[0] + dir[e][1] * u[1] + dir[e][2] * u[2];
        const double e0 = dir[e][0] - a * u[0], e1 = dir[e][1] - a * u[1], e2 = dir[e][2] - a * u[2];
        const double lat = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
        ok = ok && a > 0;
        const double t = lat / a;
        tan_t = t > tan_t ? t : tan_t;
    }
    for (int i = 0; i < 3; ++i) k.u[i] = u[i];
    k.tan_t = tan_t;
    k.ok = ok;
    return k;
}

/* true if every point of box(v) inside the pyramid (apex, cone k around it) lies in the ball (c, sqrt(r2)): the rays
 * of the pyramid get no hit on the node (header comment).  false = keep the node.
 *
 * The test bounds box ∩ pyramid by a thick segment (a vertex enumeration of the polytope is exact but ~20x the
 * work, a latency chain the single-lane-per-tile pre-pass cannot hide).  A point p of the pyramid at depth
 * t = (p - apex).u is within rho(t) = t tan_t of q = apex + t u (pyramid_cone).  If p is also in the box, t <= t_far
 * (the deepest box corner) and q lies in the box grown by rho = t_far tan_t on every axis, so on the axis' slab
 * interval [t0, t1] of that grown box.  Every such p therefore lies in the conical frustum around the axis between
 * the depths t0 and t1, of radius rho(t) = t tan_t at depth t: a convex set whose extreme points are its two rim
 * circles, and a point of the rim at t_e is within |q(t_e) - c| + rho(t_e) of c.  The ball is convex: |q(t_e) - c|
 * <= R - m - rho(t_e) at both ends puts the frustum, and every such p, within R - m.  (Until round 6 both ends were
 * tested against rho(t_far), the cylinder around the frustum: 2.7 % fewer void tiles on lecture5 at 4K,
 * profiles/r06_variants.md.)  The apex in the grown box, an empty or non-finite interval, or a pyramid of 90 degrees
 * or more refuse. */
C2RT_VOID_FN bool pyramid_void(const double apex[3], const PyramidCone &k, const VoidNode &v)
{
    if (!k.ok) return false;
    const double *u = k.u;
    const double tan_t = k.tan_t;
    double t_far = 0;
    for (int q = 0; q < 8; ++q) {
        const double t = ((q & 1) ? v.hi[0] : v.lo[0]) * u[0] - apex[0] * u[0] + ((q & 2) ? v.hi[1] : v.lo[1]) * u[1] -
                         apex[1] * u[1] + ((q & 4) ? v.hi[2] : v.lo[2]) * u[2] - apex[2] * u[2];
        t_far = t > t_far ? t : t_far;
    }
    /* rounding of u, tan_t and t_far: relative 1e-15 each; 1e-9 relative and an absolute 1e-9 to spare */
    const double rho = t_far * tan_t * (1 + 1e-9) + 1e-9 * t_far;
    double t0 = 0, t1 = 1e300;
    bool apex_in = true;
    for (int i = 0; i < 3; ++i) {
        const double lo = v.lo[i] - rho, hi = v.hi[i] + rho;
        apex_in = apex_in && apex[i] >= lo && apex[i] <= hi;
        if (u[i] == 0) {
            if (!(apex[i] >= lo && apex[i] <= hi)) return false; /* parallel and outside: the pyramid misses the box */
        } else {
            double ta = (lo - apex[i]) / u[i], tb = (hi - apex[i]) / u[i];
            if (ta > tb) { const double x = ta; ta = tb; tb = x; }
            t0 = ta > t0 ? ta : t0;
            t1 = tb < t1 ? tb : t1;
        }
    }
    if (apex_in || !(t0 <= t1) || !(t1 < 1e300)) return false;
    bool ok = true;
    for (int e = 0; e < 2; ++e) {
        const double t = e ? t1 : t0;
        const double r = sqrt(v.r2) - (t * tan_t * (1 + 1e-9) + 1e-9 * t); /* R - m - rho(t_e) */
        if (!(r > 0)) return false;
        const double d0 = apex[0] + u[0] * t - v.c[0], d1 = apex[1] + u[1] * t - v.c[1], d2 = apex[2] + u[2] * t - v.c[2];
        ok = ok && d0 * d0 + d1 * d1 + d2 * d2 <= r * r * (1 - 1e-12);
    }
    return ok;
}

C2RT_VOID_FN bool pyramid_void(const double apex[3], const double dir[4][3], const VoidNode &v)
{
    return pyramid_void(apex, pyramid_cone(dir), v);
}

/* ---- Sphere silhouette ---------------------------------------------------------------------------------------
 * A node whose root geometry is a Sphere (c, R) under an identity matrix: the tile's rays provably get no hit on it
 * when none of them passes within R + m of c.
 *
 * Why such a ray gets no hit: Sphere.intersect (rt/geometry.d:92-125) solves A t^2 + B t + C = 0 with A = dir.dir,
 * B = 2 dir.(o - c), C = |o - c|^2 - R^2 and reports no hit when B^2 - 4 A C is negative.  For a unit direction the
 * exact value is -4 (d^2 - R^2), d the ray's distance from c; d >= R + m makes it <= -4 (2 R m + m^2) < -8 R m.
 * The computed value differs by the rounding of B^2 and 4 A C, each a few ulp of 4 |o - c|^2, of the direction's
 * normalisation (|dir|^2 = 1 +- 1e-15: relative, the same order) and of the node offset's subtraction from the
 * origin (1e-16 |o| in o, 1e-16 |o| |o - c| in C): together below 1e-14 |o - c|^2.  With scale = the frame's sum of
 * max-norms (the largest R + |c| of the tested balls, the eye, light 0: SphereCull::reach), a primary ray has
 * |o - c| <= scale; a shadow ray starts on the tile's footprint, which near the horizon is arbitrarily far away, so
 * the shadow test refuses footprints that reach beyond `reach` from the origin (|o - c| <= 2 scale).  m >= 1e-9
 * scale^2 / R puts 8 R m >= 8e-9 scale^2, five orders of magnitude above 4e-14 scale^2; the terms of void_margin
 * (1e-5 + 1e-6 scale) on top cover the shadow origins' 1e-6 step off the ground and the rays' own rounding as they
 * do for the void test.  The margin grows with scale^2 / R: a small ball far from the origin is culled late or
 * not at all, never wrongly.
 *
 * The rays: the same two pyramids as the void test's — primary: apex = eye, the tile's corner rays widened by 1 px
 * (tile_corner_dirs; the AA taps reach 0.6 px); shadow towards light 0 of a primary-ground tile: apex = light
 * through the padded footprint (footprint_dirs), which holds the shadow segments up to the light.  Beyond the light
 * a shadow ray leaves that pyramid (Sphere.intersect itself does not stop at the light), so the shadow test is only granted where the padded
 * ball lies strictly on the ground's side of the light's height (SphereNode::flags bit 1, host): no ray continues
 * into it after passing the light.  Each pyramid lies in its circular cone (pyramid_cone); cone_misses_ball decides
 * for the cone. */
constexpr int kMaxSphereNodes = 4; /* Sphere nodes tested per frame (the first ones among the culled) */

struct SphereNode {
    double c[3];                   /* world centre (object centre + node offset) */
    double rp;                     /* R + m, m = sphere_margin */
    uint32_t node;                 /* node index (< kMaxCullNodes) */
    uint32_t flags;                /* bit 0: primary test; bit 1: shadow test towards light 0 */
};

/* the per-frame sphere argument of the mask pre-pass (tile_masks_kernel), next to VoidCull (whose light0 it uses) */
struct SphereCull {
    uint32_t n;
    /* bit k: node k (an entry of s[]) may be claimed as the one sphere of a sphere-interior tile ("Sphere-interior tiles",
     * below): the frame can take lean::sphere_tile and the node's material is one that path carries (host:
     * sphere_cull_of).  Sits in what was padding. */
    uint32_t interior;
    double reach;                  /* the scale the margins were derived for: the shadow test's footprint limit */
    SphereNode s[kMaxSphereNodes];
};

/* margin of a ball of radius R for coordinates of magnitude up to `scale` (derivation above) */
C2RT_VOID_FN double sphere_margin(double scale, double R) { return void_margin(scale) + 1e-9 * scale * scale / R; }

/* true only if no ray of the cone k around `apex` (any point apex + t w, t >= 0, w within the cone's half angle of
 * u) passes within rp of c: the distance from c to the solid cone exceeds rp.  In the plane through the axis and c,
 * with a = (c - apex).u and lat = the distance of c from the axis, the cone's rim is the ray (cos, sin) of the half
 * angle theta, tan(theta) = tan_t.  Where c projects onto that rim ray (a + lat tan_t >= 0) its distance from the
 * cone is lat cos - a sin = (lat - a tan_t) / sqrt(1 + tan_t^2) — which is > rp exactly when the angle between
 * c - apex and u exceeds theta + asin(rp / |c - apex|) — and where it projects behind the apex (the ball lies
 * wholly behind it) the distance is |c - apex|.  No inverse trigonometry.  Refuses (false = keep the node): the
 * apex inside the padded ball, a pyramid of 90 degrees or more, any non-finite operand.  Rounding of u, tan_t, a
 * and lat is relative 1e-15 of |c - apex|: 1e-9 relative and 1e-9 |c - apex| absolute to spare. */
C2RT_VOID_FN bool cone_misses_ball(const double apex[3], const PyramidCone &k, const double c[3], double rp)
{
    if (!k.ok) return false;
    const double w0 = c[0] - apex[0], w1 = c[1] - apex[1], w2 = c[2] - apex[2];
    const double a = w0 * k.u[0] + w1 * k.u[1] + w2 * k.u[2];
    const double e0 = w0 - a * k.u[0], e1 = w1 - a * k.u[1], e2 = w2 - a * k.u[2];
    const double lat = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    const double d = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double sec = sqrt(1.0 + k.tan_t * k.tan_t);
    if (!(d < 1e150) || !(rp < 1e150) || !(rp > 0) || !(sec < 1e150)) return false; /* non-finite or absurd */
    const double need = rp * (1 + 1e-9) + 1e-9 * d;
    if (!(d > need)) return false; /* the apex in (or at) the padded ball */
    if (a + lat * k.tan_t >= 0) return lat - a * k.tan_t > need * sec;
    return true; /* behind the apex, and farther from it than rp */
}

/* One tile's primary pyramid: the eye and the four corner rays of the pixel rectangle [x0 - 1, x1 + 1] x
 * [y0 - 1, y1 + 1] (x1 = tx0 + kTileW, y1 = ty1 + 1: the tile's right / bottom pixel edges), in cyclic order —
 * the same directions as tile_mask_entry's ground footprint. */
C2RT_VOID_FN void tile_corner_dirs(const double pos[3], const double ul[3], const double du[3], const double dv[3],
                                   double fw, double fh, int tx0, int tx1, int ty0, int ty1p1, double dir[4][3])
{
    for (int k = 0; k < 4; ++k) {
        const bool right = k == 1 || k == 2, bottom = k >= 2;
        const double sx = right ? (double)(tx1 + 1) : (double)(tx0 - 1);
        const double sy = bottom ? (double)(ty1p1 + 1) : (double)(ty0 - 1);
        const double cfx = sx / fw, cfy = sy / fh;
        for (int i = 0; i < 3; ++i) dir[k][i] = ul[i] + du[i] * cfx + dv[i] * cfy - pos[i];
    }
}

/* One ground tile's shadow pyramid towards light `L`: apex L, edges through the corners of the footprint rectangle
 * [fx0, fx1] x [fz0, fz1] on the plane y = gy, grown by the shadow origins' 1e-6 offset along the normal seen
 * from the light (1e-6 * horizontal / vertical extent) with a factor 10 to spare. */
C2RT_VOID_FN void footprint_dirs(const double L[3], double gy, double fx0, double fx1, double fz0, double fz1, double dir[4][3])
{
    const double h = void_abs(L[1] - gy);
    const double ext = void_abs(fx0 - L[0]) + void_abs(fx1 - L[0]) + void_abs(fz0 - L[2]) + void_abs(fz1 - L[2]);
    const double pad = 1e-5 * (1.0 + ext / h) + 1e-9 * (void_abs(fx0) + void_abs(fx1) + void_abs(fz0) + void_abs(fz1));
    const double x0 = fx0 - pad, x1 = fx1 + pad, z0 = fz0 - pad, z1 = fz1 + pad;
    for (int k = 0; k < 4; ++k) {
        const bool hx = k == 1 || k == 2, hz = k >= 2;
        dir[k][0] = (hx ? x1 : x0) - L[0];
        dir[k][1] = gy - L[1];
        dir[k][2] = (hz ? z1 : z0) - L[2];
    }
}

/* ---- Dark ground tiles ---------------------------------------------------------------------------------------
 * The opposite claim: EVERY shadow ray towards light 0 from a primary-ground tile gets a hit on one and the same node
 * before the light, so testVisibility (rt/scene.d:62-78) is false for every sample of the tile and the light adds
 * nothing to it.  (Whatever the nodes in front of that one in the scene's list report: a hit ends the loop with the
 * same answer, a miss leaves the distance limit alone.)
 *
 * The tool.  Let h = light.y - ground_y > 0 (h < 0: mirrored), K a convex set with ground_y + m < y < light.y - m for
 * all its points, and K_m its erosion by m (the points whose m-ball lies in K).  Central projection from the light
 * onto the ground plane is a projective map that is regular on the half space y < light.y, so the ground points g
 * whose segment light -> g meets K_m form a convex set.  If it holds the four corners of the tile's padded footprint
 * rectangle (footprint_dirs: the rectangle grown by ten times what the shadow origins' 1e-6 step off the ground
 * moves a projected point), it holds the rectangle.  A shadow ray starts at from = p + N * 1e-6, p in the footprint;
 * the line light -> from meets the ground plane at a point g of the padded rectangle, from lies on the segment
 * light -> g, below every point of K, so the point q of K_m on that segment lies between `from` and the light, at
 * least m from either along the ray.  The ray therefore has a chord of at least 2 m around q inside K, all of it in
 * front of the light.  The tests below clip against K eroded by 2 m: the second m pays for their own rounding
 * (relative 1e-15 of the scale, against m >= 1e-5 + 1e-6 scale).
 *
 * Sphere node (identity matrix, offset allowed), K = the ball (c, R), m = sphere_margin: the ray passes within R - m
 * of c, so the exact discriminant of Sphere.intersect is 4 (R^2 - d^2) >= 4 (2 R m - m^2) > 4 R m for a unit
 * direction, against a rounding below 1e-14 |o - c|^2 (cone_misses_ball's bound, |o - c| <= 2 scale for footprints
 * within `reach`) — the same five orders of magnitude.  Both ends of the ray's segment lie outside the ball by more
 * than m (the ground below it, the light above it), so both roots lie in (m, |light - from| - m); the near root is
 * positive, below the distance limit, and the hit is reported.
 *
 * CsgDiff(Cube, Sphere) node (identity matrix, offset allowed), m = void_margin.  The solid is not convex; for a
 * corner s in {-1, +1}^3 of the cube, n = s / sqrt(3),
 *     K = {p in the cube shrunk by pad (the node box's padding) : n.(p - c) >= R + m}
 * is convex (a box cut by a half space: a tetrahedron at the corner when the ball swallows the cube's edges), lies in
 * the cube and outside the subtracted ball by m.  Take a ray with a point q of K_m on it, and let every ray of the
 * tile satisfy n.w > 0, w its direction towards the light (linear in the origin: tested at the four corners).
 * CsgOp.intersect (rt/geometry.d:292-332) walks the sorted events of both children, starting from inL = |L| odd,
 * inR = |R| odd, and reports the first event after which inL && !inR:
 *  - R, the ball.  Every recorded event point lies on the sphere up to rounding, so n.(p - c) <= R + 1e-9, while
 *    n.(q - c) >= R + m: with n.w > 0 every R event precedes q by at least m - 1e-9 in distance (n.w <= 1).  So
 *    however many events findAllIntersections recorded (none; one, the origin inside the ball — on lecture5 the
 *    subtracted ball dips below the floor; two; any other small number for a grazing ray whose 1e-6 steps land on
 *    either side of the sphere; the device's cap of 8 is not approached), all of them are flipped before q and inR,
 *    having started at their parity, is false at q.
 *  - L, the cube.  The origin is outside it: the box lies above the ground by more than m, the origin within 1e-6 of
 *    it.  q is at least m from every face, so the face the ray enters (leaves) through is crossed with a direction
 *    component of at least m / diameter >= 5e-7 (Cube.intersect skips an axis only below 1e-9), and the 1e-6 step
 *    past the entry carries the origin 5e-13 past that face, far above the rounding of the recorded point: exactly
 *    two events, the entry before q by at least m and the exit after it.  inL starts false and is true at q.
 *  So just before q the state is inL && !inR, and the walk — which stops at the first event that produces that state —
 *  has stopped at an event at or before q: a hit at a distance below dist(q) <= |light - from| - m, the distance
 *  limit of the shadow ray.  Equal distances need no tie rule: every order ends in that state before q.
 *
 * One corner per tile: the one whose octant (about the ball's centre) holds the point where the footprint centre's
 * segment from the light enters the shrunk cube — with n.w > 0 the corner pieces towards the light are the ones
 * that can qualify.
 *
 * Host (scene_plan.cpp: plan_dark_nodes, dark_cull_of): light 0 lit and finite, eye and light on the same side of the
 * ground, every K strictly between the ground and the light's height by more than m; the margins are derived once per
 * scene, for a scale that covers every eye within DarkCull::eye_max of the origin.  The result does not depend on the
 * void or silhouette tests' switches; the pre-pass sets the bit for primary-ground tiles only. */
constexpr int kMaxDarkNodes = 8; /* kMaxSphereNodes + kMaxVoidNodes */

struct DarkNode {
    double lo[3], hi[3];           /* kind 1: the Cube shrunk by pad + 2 m */
    double c[3];                   /* kind 0: the ball's centre; kind 1: the subtracted ball's */
    double r;                      /* kind 0: R - 2 m; kind 1: R + 2 m, the cuts' distance from the ball's centre */
    uint32_t node;                 /* node index (< kMaxCullNodes) */
    uint32_t kind;                 /* 0: Sphere node, 1: CsgDiff(Cube, Sphere) node */
};

/* the dark-tile table of the mask pre-pass, next to VoidCull (whose light0 it uses).  It does not fit the kernel-argument
 * segment beside the other two: a scene table in device memory, or part of a batch frame's BatchCull */
struct DarkCull {
    uint32_t n, pad;
    double reach;                  /* the scale the margins were derived for: footprint limit of the Sphere kind */
    double eye_max;                /* ... with the eye within this max-norm of the origin (host: dark_cull_of) */
    DarkNode d[kMaxDarkNodes];
};

/* the segment light -> light + d passes within r of c */
C2RT_VOID_FN bool segment_meets_ball(const double L[3], const double d[3], const double c[3], double r)
{
    const double w0 = c[0] - L[0], w1 = c[1] - L[1], w2 = c[2] - L[2];
    const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    double t = (w0 * d[0] + w1 * d[1] + w2 * d[2]) / dd;
    if (!(t >= 0)) t = 0; /* (NaN: refused below) */
    if (t > 1) t = 1;
    const double e0 = w0 - t * d[0], e1 = w1 - t * d[1], e2 = w2 - t * d[2];
    return r > 0 && dd > 0 && e0 * e0 + e1 * e1 + e2 * e2 <= r * r * (1 - 1e-9);
}

/* the parameter interval [t0, t1] of the segment light -> light + d inside the box [lo, hi]; false: empty */
C2RT_VOID_FN bool segment_clip_box(const double L[3], const double d[3], const double lo[3], const double hi[3], double &t0, double &t1)
{
    t0 = 0;
    t1 = 1;
    for (int i = 0; i < 3; ++i) {
        if (d[i] == 0) {
            if (!(L[i] >= lo[i] && L[i] <= hi[i])) return false;
        } else {
            double ta = (lo[i] - L[i]) / d[i], tb = (hi[i] - L[i]) / d[i];
            if (ta > tb) { const double x = ta; ta = tb; tb = x; }
            if (!(ta <= tb)) return false; /* non-finite */
            t0 = ta > t0 ? ta : t0;
            t1 = tb < t1 ? tb : t1;
        }
    }
    return t0 <= t1;
}

/* the cuts of kind 1: the corner's own normal (1, 1, 1) and its neighbours, signs by the corner */
constexpr int kDarkCuts = 10;

/* One primary-ground tile with the shadow pyramid's edges sdir (footprint_dirs: light -> the padded footprint's
 * corners) and the footprint's reach measure (tile_mask_entry: in_reach): every shadow ray of the tile towards
 * `light` is occluded by node k (derivation above). */
C2RT_VOID_FN bool tile_dark_by(const double light[3], const double sdir[4][3], bool in_reach, const DarkNode &k)
{
    if (k.kind == 0u) {
        if (!in_reach) return false;
        bool ok = true;
        for (int e = 0; e < 4; ++e) ok = ok && segment_meets_ball(light, sdir[e], k.c, k.r);
        return ok;
    }
    double mid[3], sg[3], t0, t1;
    for (int i = 0; i < 3; ++i) mid[i] = 0.25 * (sdir[0][i] + sdir[1][i] + sdir[2][i] + sdir[3][i]);
    if (!segment_clip_box(light, mid, k.lo, k.hi, t0, t1)) return false;
    for (int i = 0; i < 3; ++i) sg[i] = light[i] + t0 * mid[i] >= k.c[i] ? 1.0 : -1.0;
    const double w[kDarkCuts][3] = {{1, 1, 1}, {2, 1, 1}, {1, 2, 1}, {1, 1, 2}, {2, 2, 1}, {2, 1, 2}, {1, 2, 2}, {3, 1, 1}, {1, 3, 1}, {1, 1, 3}};
    const double len[kDarkCuts] = {1.7320508075688774, 2.4494897427831783, 2.4494897427831783, 2.4494897427831783, 3, 3, 3,
                                   3.3166247903554, 3.3166247903554, 3.3166247903554};
    /* Per corner segment e, once: its interval [te0, te1] inside the shrunk cube.  Per cut, with s not normalised and r
     * scaled to match: the segment meets {s.(p - c) >= r} inside that interval iff a + t b >= 0 at t = te0, given b =
     * s.d < 0 (towards the light the ray climbs along s: the n.w > 0 of the derivation, with 1e-5 relative to spare for
     * the origins' 1e-6 step) — no division in the loop: the pre-pass evaluates this in one lane per tile. */
    double te0[4];
    for (int e = 0; e < 4; ++e) {
        double te1;
        if (!segment_clip_box(light, sdir[e], k.lo, k.hi, te0[e], te1)) return false;
    }
    double rel[3]; /* light - c */
    for (int i = 0; i < 3; ++i) rel[i] = light[i] - k.c[i];
    bool dark = false;
    for (int q = 0; q < kDarkCuts; ++q) {
        const double s0 = sg[0] * w[q][0], s1 = sg[1] * w[q][1], s2 = sg[2] * w[q][2];
        const double a = s0 * rel[0] + s1 * rel[1] + s2 * rel[2] - k.r * len[q] * (1 + 1e-12);
        bool ok = true;
        for (int e = 0; e < 4; ++e) {
            const double b0 = s0 * sdir[e][0], b1 = s1 * sdir[e][1], b2 = s2 * sdir[e][2];
            const double b = b0 + b1 + b2;
            ok = ok && b < -1e-5 * (void_abs(b0) + void_abs(b1) + void_abs(b2)) && a + te0[e] * b >= 0;
        }
        dark = dark || ok;
    }
    return dark;
}

/* ---- Sphere-interior tiles -----------------------------------------------------------------------------------
 * The third claim about a Sphere node (c, R) under an identity matrix: EVERY primary ray of the tile gets its closest
 * hit on it, and no other node can occlude the tile's shadow rays towards light 0 — bit 3 of the mask table's third
 * word; lean::sphere_tile (c2rt_trace.inc) renders such a tile with that one sphere and nothing else.  m = sphere_margin
 * = rp - R, rp = SphereNode::rp, R from the node's own record.
 *
 * (a) Every ray hits, in front of the eye (cone_inside_ball).  The tile's pyramid lies in its cone (pyramid_cone): axis
 * u, half angle theta.  With d = |c - eye| and phi the angle between u and c - eye, a ray of the cone makes an angle psi
 * in [max(0, phi - theta), phi + theta] with c - eye and passes the centre at d sin(psi).  phi + theta < 90 degrees and
 * d sin(phi + theta) <= R - m put every ray within R - m of c: the exact discriminant of Sphere.intersect is
 * 4 (R^2 - d'^2) >= 4 (2 R m - m^2) > 4 R m for a unit direction, against a rounding below 1e-14 |o - c|^2 (the
 * silhouette test's bound, sign reversed; |o - c| <= scale for a primary ray, and m >= 1e-9 scale^2 / R).  d >= R + m
 * keeps the eye outside: C > 0, both roots positive, the reference reports the near one, t(psi) = d cos(psi) -
 * sqrt(R^2 - d^2 sin^2(psi)), which grows with psi — the hit points lie at ray parameters [t_lo, t_hi] = [t(psi_min),
 * t(psi_max)].  Sines and cosines come from the addition theorems: no inverse trigonometry.
 *
 * (b) Nothing is nearer.  The caller (tile_mask_entry) grants the claim only where the primary mask, after every other
 * test, holds this node, the ground plane and nothing else; unboxed nodes never leave the mask.  Ground: the eye above
 * the plane and the padded ball strictly above it (c.y - rp > ground_y + tol): a ray that reaches the plane at all
 * enters the ball at least rp - R = m earlier, so whichever of the two Node.intersect sees first, `mult > dist`
 * (Plane) resp. `sol > dist` (Sphere) keeps the sphere's hit.
 *
 * (c) Shadow rays towards light 0.  They start at p + N 1e-6, p a hit point: eye + t w, t in [t_lo, t_hi], w within theta
 * of u.  |t w - tm u| <= t |w - u| + |t - tm| <= t_hi tan(theta) + (t_hi - t_lo) / 2 for tm the interval's middle, so the
 * origins lie in the ball (q, rho), q = eye + tm u, rho = that + 2 m (the 1e-6 step, the rounding of p and of this
 * bound, with orders of magnitude to spare).  The segments from that ball to the light lie in the cone with apex L
 * around q - L of half angle asin(rho / |q - L|) (patch_shadow_cone); another node cannot occlude when the cone misses
 * its padded ball (Sphere: shadow_cone_misses_ball with its rp; a CsgDiff candidate: the ball around its padded box, grown by
 * m, which is at least void_margin).  Beyond the light a ray leaves that cone, so — as for the ground tiles' shadow tests — the other node must
 * lie strictly on the ground's side of the light's height (its flags bit 1) and so must the patch (q.y + rho < L.y -
 * tol): every ray climbs to the light and none continues into the node.  The ground: patch and light strictly above the
 * plane, so Plane.intersect either sees the ray leave (dir.y > -1e-9) or finds the crossing beyond the light.  The sphere
 * itself is not part of the claim: the path tests it per sample.
 * Only the arrangement "eye, ball and light above the ground" is claimed; the mirrored one stays on the general path. */

/* (a): true if every ray of the cone k around `apex` passes within R - m of c and starts outside the ball (c, R + m);
 * [t_lo, t_hi] then bound the near root along every such ray.  1e-9 relative and 1e-9 d absolute to spare, as in
 * cone_misses_ball.  Refuses a cone of 90 degrees or more and any non-finite operand. */
C2RT_VOID_FN bool cone_inside_ball(const double apex[3], const PyramidCone &k, const double c[3], double R, double m, double &t_lo,
                                   double &t_hi)
{
    t_lo = t_hi = 0;
    if (!k.ok) return false;
    const double w0 = c[0] - apex[0], w1 = c[1] - apex[1], w2 = c[2] - apex[2];
    const double a = w0 * k.u[0] + w1 * k.u[1] + w2 * k.u[2];
    const double e0 = w0 - a * k.u[0], e1 = w1 - a * k.u[1], e2 = w2 - a * k.u[2];
    const double lat = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    const double d = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double sec = sqrt(1.0 + k.tan_t * k.tan_t);
    if (!(d < 1e150) || !(R < 1e150) || !(R > 0) || !(m > 0) || !(m < R) || !(sec < 1e150) || !(a > 0)) return false;
    if (!(d >= (R + m) * (1 + 1e-9))) return false; /* the eye in (or at) the padded ball */
    const double inv_d = 1.0 / d, ct = 1.0 / sec; /* (two divisions for four quotients: the pre-pass is a latency chain) */
    const double sp = lat * inv_d, cp = a * inv_d, st = k.tan_t * ct;
    const double s_hi = sp * ct + cp * st, c_hi = cp * ct - sp * st; /* phi + theta */
    if (!(c_hi > 1e-9)) return false;
    if (!(d * s_hi * (1 + 1e-9) + 1e-9 * d <= R - m)) return false;
    double s_lo = sp * ct - cp * st, c_lo = cp * ct + sp * st; /* phi - theta, or 0 where the axis' own ray is inside */
    if (!(s_lo > 0)) { s_lo = 0; c_lo = 1; }
    t_lo = d * c_lo - sqrt(R * R - d * d * s_lo * s_lo);
    t_hi = d * c_hi - sqrt(R * R - d * d * s_hi * s_hi);
    return t_lo > 0 && t_hi >= t_lo && t_hi < 1e150;
}

/* (c): the ball (q, rho) that holds every shadow origin of the tile, and the cone from `light` that holds the segments
 * from it to the light.  false: the light in (or near) that ball, or non-finite. */
struct ShadowCone {
    double u[3];
    double tan_t, sec; /* of the half angle: rho / sqrt(D^2 - rho^2) and D / sqrt(D^2 - rho^2), rounded up by 1e-9 */
    bool ok;
};

C2RT_VOID_FN bool patch_shadow_cone(const double apex[3], const PyramidCone &k, double t_lo, double t_hi, double m, const double light[3],
                                    double q[3], double &rho, ShadowCone &sc)
{
    const double tm = 0.5 * (t_lo + t_hi);
    rho = (0.5 * (t_hi - t_lo) + t_hi * k.tan_t) * (1 + 1e-9) + 2 * m + 1e-9 * t_hi;
    double v[3], D2 = 0;
    for (int i = 0; i < 3; ++i) {
        q[i] = apex[i] + tm * k.u[i];
        v[i] = q[i] - light[i];
        D2 += v[i] * v[i];
    }
    const double D = sqrt(D2);
    sc.ok = false;
    if (!(D < 1e150) || !(rho < 1e150) || !(D > 2 * rho)) return false;
    const double inv_D = 1.0 / D, inv_h = 1.0 / sqrt(D2 - rho * rho);
    for (int i = 0; i < 3; ++i) sc.u[i] = v[i] * inv_D;
    sc.tan_t = rho * inv_h * (1 + 1e-9);
    sc.sec = D * inv_h * (1 + 1e-9);
    sc.ok = sc.tan_t < 1e150 && sc.sec < 1e150;
    return sc.ok;
}

/* cone_misses_ball for the shadow cone, without a square root: the pre-pass evaluates it in one lane per tile, once per
 * node left in the shadow mask, behind everything else the tile's wave has to do.  The same geometry — the distance
 * from c to the solid cone exceeds rp — with the two lengths compared by their squares: d is bounded from above by the
 * 1-norm in the padding term (a larger `need`: never a wrong miss), the apex-in-ball test is d^2 > need^2, "c projects
 * onto the rim ray" is a >= 0 or lat^2 tan^2 >= a^2, and lat > x is lat^2 > x^2 for x > 0 and true for x <= 0. */
C2RT_VOID_FN bool shadow_cone_misses_ball(const double apex[3], const ShadowCone &k, const double c[3], double rp)
{
    if (!k.ok) return false;
    const double w0 = c[0] - apex[0], w1 = c[1] - apex[1], w2 = c[2] - apex[2];
    const double a = w0 * k.u[0] + w1 * k.u[1] + w2 * k.u[2];
    const double e0 = w0 - a * k.u[0], e1 = w1 - a * k.u[1], e2 = w2 - a * k.u[2];
    const double lat2 = e0 * e0 + e1 * e1 + e2 * e2, d2 = w0 * w0 + w1 * w1 + w2 * w2;
    const double d1 = void_abs(w0) + void_abs(w1) + void_abs(w2);
    if (!(d1 < 1e150) || !(rp < 1e150) || !(rp > 0)) return false; /* non-finite or absurd */
    const double need = rp * (1 + 1e-9) + 1e-9 * d1;
    if (!(d2 > need * need * (1 + 1e-9))) return false; /* the apex in (or at) the padded ball */
    if (a >= 0 || lat2 * k.tan_t * k.tan_t >= a * a) {
        const double x = (a * k.tan_t + need * k.sec) * (1 + 1e-9);
        return !(x > 0) || lat2 > x * x * (1 + 1e-9);
    }
    return true; /* behind the apex, and farther from it than rp */
}

/* the ball around a CsgDiff candidate's padded box (VoidNode: lo, hi), grown by m */
C2RT_VOID_FN void box_ball(const VoidNode &v, double m, double c[3], double &rp)
{
    double r2 = 0;
    for (int i = 0; i < 3; ++i) {
        c[i] = 0.5 * (v.lo[i] + v.hi[i]);
        const double h = 0.5 * (v.hi[i] - v.lo[i]);
        r2 += h * h;
    }
    rp = sqrt(r2) * (1 + 1e-9) + m;
}

/* (b) and (c) for a tile whose cone has passed (a) with the entry depths [t_lo, t_hi] (m = the sphere's margin): the ground
 * below the padded ball and the eye, and every other node of the shadow mask missed by the cone from the light. */
C2RT_VOID_FN bool sphere_interior_rest(const double eye[3], const PyramidCone &k, const SphereCull &S, uint32_t self, double m, double t_lo,
                                       double t_hi, const VoidCull &V, uint32_t smask0, uint32_t n_nodes, int ground_node,
                                       double ground_y, bool has_light)
{
    const SphereNode &sn = S.s[self];
    const double tol = 1e-6 + 1e-9 * (void_abs(ground_y) + void_abs(sn.c[1]) + sn.rp + void_abs(eye[1]));
    if (ground_node >= 0 && !(eye[1] > ground_y + tol && sn.c[1] - sn.rp > ground_y + tol)) return false;
    if (!has_light) return true;
    const double *L = V.light0;
    double q[3], rho;
    ShadowCone sc;
    if (!patch_shadow_cone(eye, k, t_lo, t_hi, m, L, q, rho, sc)) return false;
    const double ltol = 1e-6 + 1e-9 * (void_abs(L[1]) + void_abs(q[1]) + rho + void_abs(ground_y));
    if (ground_node >= 0 && !(L[1] > ground_y + ltol)) return false;
    uint32_t others = smask0 & (n_nodes >= 32u ? 0xFFFFFFFFu : ((1u << n_nodes) - 1u)) & ~(1u << sn.node);
    if (ground_node >= 0) others &= ~(1u << ground_node);
    if (!others) return true;
    if (!(q[1] + rho < L[1] - ltol)) return false; /* the patch strictly below the light's height */
    for (uint32_t j = 0; j < S.n; ++j) {
        const SphereNode &o = S.s[j];
        if (j == self || !((others >> o.node) & 1u)) continue;
        if (!(o.flags & 2u) || !shadow_cone_misses_ball(L, sc, o.c, o.rp)) return false;
        others &= ~(1u << o.node);
    }
    for (uint32_t j = 0; j < V.n; ++j) {
        const VoidNode &o = V.v[j];
        if (!((others >> o.node) & 1u)) continue;
        double bc[3], brp;
        box_ball(o, m, bc, brp);
        if (!(o.flags & 2u) || !shadow_cone_misses_ball(L, sc, bc, brp)) return false;
        others &= ~(1u << o.node);
    }
    return others == 0u; /* a node neither table knows: no claim */
}

/* One tile, cone k of its primary pyramid around `eye`: the claim above for entry `self` of S (radius R from the node's
 * record), given the shadow mask smask0 the other tests left (bits at and above n_nodes ignored), the ground node (-1:
 * none; then the scene must have no unboxed node at all, which the caller's primary-mask condition implies) and light 0
 * (has_light = false: no shadow ray is cast).  The primary-mask condition (b) is the caller's. */
C2RT_VOID_FN bool sphere_interior_tile(const double eye[3], const PyramidCone &k, const SphereCull &S, uint32_t self, double R,
                                       const VoidCull &V, uint32_t smask0, uint32_t n_nodes, int ground_node, double ground_y,
                                       bool has_light)
{
    const SphereNode &sn = S.s[self];
    const double m = sn.rp - R;
    double t_lo, t_hi;
    if (!cone_inside_ball(eye, k, sn.c, R, m, t_lo, t_hi)) return false;
    return sphere_interior_rest(eye, k, S, self, m, t_lo, t_hi, V, smask0, n_nodes, ground_node, ground_y, has_light);
}

} // namespace c2rt

#endif
