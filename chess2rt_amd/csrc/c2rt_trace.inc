/*
 * c2rt_trace.inc — the half of the trace that depends on the arithmetic mode: divide / sqrt / normalise, primitives,
 * CSG, nodes, surface, visibility, shading, the camera ray and the per-tile renderer (SURVEY.md section 8(a),
 * rows a1-a26).
 *
 * The rule: a definition lives here if it reads kLean, or calls or instantiates something that does.  Everything
 * else — types, vectors, the window accumulator, hit records, Ctx, CSG tags, u,v, textures, RNG, pixel store — is
 * defined ONCE, at c2rt:: scope, in c2rt_trace_shared.inc, and the tile-mask classifier in c2rt_tile_mask.inc;
 * c2rt_trace_common.inc includes both in front of this file.  (Kept here although they do not reach kLean, beside
 * the code they serve: ORay, misses_bound, geom_is_inside, RayW, and the AA tap tables k_aa_x / k_aa_y, which are
 * one device symbol per namespace.)
 *
 * Included by c2rt_trace_common.inc into two namespaces (the frame file c2rt_kernels.hip takes both, the query files
 * c2rt_rays.hip, c2rt_hit_planes.hip and c2rt_adaptive.hip exact:: only):
 *   lean::  (kLean = true)   divide / sqrt / normalise through fp64_lean.h, OPTIMISTICALLY: every use tests
 *           its operands' window with two integer instructions and folds the outcome into Ctx::bad instead of
 *           branching to a fallback; results of a lane whose operand was outside a window are garbage (never
 *           a fault: the reference's own arithmetic meets NaNs and infinities on this path).
 *   exact:: (kLean = false)  the compiler's IEEE expansions of `/` and `sqrt`, as in rounds 1-2.
 * A frame kernel renders its tile with lean::render_tile; a tile in which any lane raised `bad` writes nothing
 * and is rendered again, by the same wave, with exact::render_tile (cold code at the end of the kernel).
 * On a sane scene that never happens; a zero numerator (camera exactly on a cube's face plane), a NaN
 * direction or coordinates beyond 1e+-70 take the exact path for the tiles they touch, with the same bits
 * as before.  Having the fallbacks anywhere near the hot code was measured twice and lost both times
 * (profiles/r03_variants.md: inline +20 % instructions, as calls +11 % and 7 spilled VGPRs).
 */
/* ------------------------------------------------------------------ */
/* fp64 divide / sqrt: lean:: optimistic forms, exact:: the compiler's    */
/* ------------------------------------------------------------------ */
/* lean:: (kLean) — fp64_lean.h's sequences: the same correctly rounded results as the compiler's expansions
 * from fewer (and fewer quarter-rate) instructions, valid when the operands lie in windows that a
 * short integer test on the high word checks (Oob, c2rt_trace_shared.inc: three instructions, two for a sum of squares).  Nothing branches on the test: it is folded into `bad` (Ctx::bad)
 * and a tile with a bad lane is thrown away and rendered again through exact:: (render_tile's
 * return value).  exact:: — `/` and `sqrt` as hipcc expands them. */

/* len = sqrt(s) and inv = 1.0 / len: gfm's magnitude() and the factor normalize() multiplies by.  In
 * lean:: len is den_ok and inv is the correctly rounded reciprocal that div_r accepts for a later
 * division by len (sqrt_ok's window is the square of den_ok's). */
DEV void len_inv(Oob &bad, double s, double &len, double &inv)
{
    if constexpr (kLean) {
        oob_note_nonneg(bad, s); /* every caller's s is a sum of squares */
        inv_len(s, len, inv); /* a significand of all ones: fp64_lean.h */
    } else {
        len = sqrt(s);
        inv = 1.0 / len;
    }
}
/* the same for the squared length of a vector that is already unit up to rounding (a second normalize):
 * integer arithmetic on its distance from 1 in ulps when every lane is within 64 (it always is, on a
 * vector that came out of a normalisation; tests/fp64_lean_check.hip) */
DEV void len_inv_unit(Oob &bad, double s, double &len, double &inv)
{
    if constexpr (kLean) {
        if (__all(near_one(s))) {
            unit_len(s, len, inv);
            return;
        }
    }
    len_inv(bad, s, len, inv);
}
DEV double sqrt_g(Oob &bad, double x)
{
    if constexpr (kLean) {
        oob_note(bad, x);
        return sqrt_lean(x);
    } else {
        return sqrt(x);
    }
}
/* a / b; lean:: through a reciprocal r of b that div_with accepts — rcp_refined(b), or the correctly
 * rounded 1 / b — for a denominator that is den_ok by construction at every site (a component of a finite
 * unit direction that the test has already compared with 1e-9, |d|^2 of such a direction, a length from
 * len_inv) */
DEV double div_r(Oob &bad, double a, double b, double r)
{
    if constexpr (kLean) {
        oob_note(bad, a);
        return div_with(a, b, r);
    } else {
        return a / b;
    }
}
DEV D3 normalized(Oob &bad, D3 a)
{
    double len, inv;
    len_inv(bad, sqmag(a), len, inv);
    return mk(a.x * inv, a.y * inv, a.z * inv);
}
/* A ray in some object space: origin, unit direction and A = |d|^2 exactly as
 * Sphere.intersect computes it (rt/geometry.d:96) — the direction is shared by
 * every geometry under a node and by all steps of findAllIntersections, so A
 * is evaluated once per direction instead of once per sphere test. */
struct ORay {
    D3 o, d;
    double A;
    /* lean:: — every test along a direction divides by the same few numbers: a plane / cube face by
     * -d.y (-d.x, -d.z), a sphere root by 2A.  The refined reciprocals the compiler's division would compute
     * each time are evaluated once per direction (prep_dir) and every division is div_r's three
     * instructions — the same bits (fp64_lean.h).  Only the fields the node's geometry type needs are filled;
     * exact:: leaves them alone. */
    double rx, ry, rz, rA2;
};
enum { kPrepY = 1, kPrepXZ = 2, kPrepA = 4 };
DEV void prep_dir(ORay &r, int what)
{
    if constexpr (!kLean) return;
    if (what & kPrepY) r.ry = rcp_refined(-r.d.y);
    if (what & kPrepXZ) { r.rx = rcp_refined(-r.d.x); r.rz = rcp_refined(-r.d.z); }
    if (what & kPrepA) r.rA2 = rcp_refined(2 * r.A);
}

/* ------------------------------------------------------------------ */
/* primitives                                                           */
/* ------------------------------------------------------------------ */

/* Plane.intersect — rt/geometry.d:30-59 */
template <int NEED>
DEV bool plane_intersect(Oob &bad, GeomP G, int gid, const ORay &r, Hit &h, bool full)
{
    const D3 o = r.o, d = r.d;
    const double y = G->p[0], limit = G->p[1];
    /* (bitwise forms of the reference's conditions: same truth table incl. NaN, one branch each) */
    if (((o.y > y) & (d.y > -1e-9)) | ((o.y < y) & (d.y < 1e-9))) return false;
    const double mult = div_r(bad, o.y - y, -d.y, r.ry);
    const D3 p = o + d * mult;
    if ((mult > h.dist) | (fabs(p.x) > limit) | (fabs(p.z) > limit)) return false;
    h.dist = mult;
    if (NEED >= kPoint) { h.p = p; h.g = gid; }
    if (C2RT_WANT_FULL(NEED, full)) h.code = 0;
    return true;
}

/* Sphere.intersect — rt/geometry.d:92-125 */
template <int NEED>
DEV bool sphere_intersect(Oob &bad, GeomP G, int gid, const ORay &r, Hit &h, bool full)
{
    const D3 o = r.o, d = r.d;
    const D3 c = ld3(G->p);
    const D3 H = o - c;
    const double A = r.A;
    const double B = 2 * dot(H, d);
    const double C = sqmag(H) - G->q[0]; /* R * R, from the table */
    const double BB = B * B;
    const double Dscr = BB - 4 * A * C;
    /* Dscr < 0: no real root.  Or: outside the sphere and moving away — sqrt(Dscr) < B
     * by a margin far above rounding, so both roots are negative: the reference
     * returns false after a sqrt and two divisions; skip them.  (Near-degenerate
     * cases fall through to the literal evaluation.)  One branch for both. */
    if ((Dscr < 0) | ((C > 0) & (B > 0) & (Dscr < BB * (1 - 1e-8)))) return false;
    const double sq = sqrt_g(bad, Dscr);
    const double A2 = 2 * A;
    /* x1 = (-B + sq) / (2A) is only read when x2 < 0 */
    double sol = div_r(bad, -B - sq, A2, r.rA2);
    if (sol < 0) sol = div_r(bad, -B + sq, A2, r.rA2);
    if ((sol < 0) | (sol > h.dist)) return false;
    h.dist = sol;
    if (NEED >= kPoint) {
        const D3 p = o + d * sol;
        h.p = p;
        h.g = gid;
        if (C2RT_WANT_FULL(NEED, full)) h.code = 0;
    }
    return true;
}

/* Cube.intersectCubeSide — rt/geometry.d:198-235, for the face pair whose
 * axis is `ay` after the project() permutation; (ax, az) are the other two
 * axes in permuted order.  Arithmetic is component-wise, so it is evaluated
 * in place instead of permuting (project/unproject, rt/imported_types.d:44-60).
 * `mult < 0` is decided from the operand signs (an IEEE quotient is negative
 * iff exactly one operand is and the numerator is non-zero), which skips the
 * division for every face behind the origin. */
template <int NEED, int AXIS>
DEV bool cube_sides(Oob &bad, double oy, double dy, double rden, double ylo, double yhi, double ox, double dx, double xlo, double xhi,
                    double oz, double dz, double zlo, double zhi, D3 o, D3 d, Hit &h, bool full)
{
    if (fabs(dy) < 1e-9) return false;
    bool found = false;
    const double den = -dy;
    /* face planes and bounds come from the table (DevGeom::q): `center + side * halfSide` and
     * `center -+ halfSide` are the same for every ray */
#pragma unroll
    for (int side = -1; side <= 1; side += 2) {
        const double num = oy - (side < 0 ? ylo : yhi);
        /* lean:: — one multiply and one compare instead of four compares: the product is negative exactly
         * when the signs differ and neither operand is zero or NaN, except that it may underflow to -0 for a
         * numerator below 2^-1045 (|den| >= 1e-9) — which then reaches the division, where the window test
         * refuses it and the tile is redone. */
        const bool negative = kLean ? (num * den < 0) : (((num < 0) & (den > 0)) | ((num > 0) & (den < 0)));
        if (negative) continue;          /* mult < 0 */
        const double mult = div_r(bad, num, den, rden); /* rden: lean::'s refined reciprocal of -dy (prep_dir) */
        const double px = ox + dx * mult, pz = oz + dz * mult;
        /* the reference's four rejections (mult < 0 kept for NaN / zero corner cases) as ONE
         * predicate: one divergent branch per face instead of four.  (lean::: a numerator inside the
         * window over a denominator of the same sign gives a positive quotient, so `mult < 0` is dead;
         * any other numerator has already voided the tile.) */
        const bool reject = (!kLean & (mult < 0)) | (mult > h.dist) | (px < xlo) | (px > xhi) | (pz < zlo) | (pz > zhi);
        if (reject) continue;
        h.dist = mult;
        /* Vector(0, side, 0) un-permuted is the face normal along AXIS; u = px - cx, v = pz - cz are
         * components of p - center (px, pz are h.p's permuted components): hit_surface */
        if (C2RT_WANT_FULL(NEED, full)) h.code = AXIS | (side > 0 ? kCodeSide : 0);
        found = true;
    }
    return found;
}

/* Cube.intersect — rt/geometry.d:172-196 (an early-out in front of it was measured and rejected: see below) */
template <int NEED>
DEV bool cube_intersect(Oob &bad, GeomP G, int gid, const ORay &r, Hit &h, bool full)
{
    const D3 o = r.o, d = r.d;
    const D3 lo = ld3(G->q), hi = ld3(G->q + 3);
    /* Y faces; X faces = project(1,0,2): (y,x,z); Z faces = project(0,2,1): (x,z,y) */
    bool found = cube_sides<NEED, 1>(bad, o.y, d.y, r.ry, lo.y, hi.y, o.x, d.x, lo.x, hi.x, o.z, d.z, lo.z, hi.z, o, d, h, full);
    found |= cube_sides<NEED, 0>(bad, o.x, d.x, r.rx, lo.x, hi.x, o.y, d.y, lo.y, hi.y, o.z, d.z, lo.z, hi.z, o, d, h, full);
    found |= cube_sides<NEED, 2>(bad, o.z, d.z, r.rz, lo.z, hi.z, o.x, d.x, lo.x, hi.x, o.y, d.y, lo.y, hi.y, o, d, h, full);
    if (found) {
        /* the point of the face that won, once per cube instead of once per accepted face: the same
         * `o + d * mult` on the same operands (h.dist IS that face's mult) */
        if (NEED >= kPoint) h.p = o + d * h.dist;
        if (NEED >= kPoint) h.g = gid;
    }
    return found;
}

/* MEASURED AND REJECTED: an early-out in front of Cube.intersect for the stepping loops of a CsgOp.
 * Cube.intersect returns false — EXACTLY, not conservatively — for a ray whose origin lies beyond one face pair's
 * slab and which moves further away along that axis (o.x > hi.x and d.x > 0, or the mirror image, on any axis):
 *   faces of that axis (rt/geometry.d:208-216): both numerators o.x - face are > 0 (the difference of distinct doubles
 *     is never zero; lo <= hi, or the cube is empty and nothing is ever accepted) over the denominator -d.x < 0:
 *     `mult < 0`, both skipped;
 *   faces of the other two axes: an accepted candidate has 0 <= mult <= +inf (NaN excluded below), so d.x * mult >= 0
 *     and px = RN(o.x + d.x * mult) >= o.x > hi.x by the monotonicity of rounding: rejected by `px > xhi`.
 * The premise is ordered arithmetic: a NaN origin component, direction component or face plane makes the literal
 * code ACCEPT candidates (every comparison with NaN is false), so the shortcut was only taken for finite cubes
 * (kGeomFinite, scalar) and lanes whose origin and direction are finite (one class test on their sum: a finite sum
 * has no NaN or infinite term).  This is the step on which findAllIntersections (rt/geometry.d:271-290) ends after a
 * ray has left a cube — a third of all Cube.intersect calls under a CsgOp: ~16 instructions instead of ~70.
 * Exact and bit-identical on the whole suite (profiles/r04_variants.md, step 1), but the kernels are slower with
 * it — lecture5 4K x5 1.010 -> 1.054 ms, csg_stress 8.40 -> 9.11 ms: the headline instance goes from 122 to 124 VGPRs
 * and from 151 to 190 SGPRs spilled to VGPR lanes (the cube's six face planes live across the stepping loop), which
 * costs more than the ~55 instructions the early-out saves per evaluation.  Three placements were tried: on the
 * terminating step of a child's stepping loop, also on its first step, and inside cube_intersect itself (where no
 * face plane lives longer than it already does).  The code (cube_away and its three call sites) is in commit
 * f0eed4f. */

/* Conservative reject: true when the ray cannot reach the geometry's padded
 * bounding sphere (DevGeom::bound), in which case Geometry.intersect would
 * return false after doing all of its work.  |d| = 1 up to rounding and the
 * radius is padded by 1e-6 relative, so the test only ever errs towards
 * "may hit". */
DEV bool misses_bound(GeomP G, const ORay &r)
{
    const D3 H = r.o - ld3(G->bound);
    const double b = dot(H, r.d);
    const double c = sqmag(H) - G->bound[3];
    return (c > 0) & ((b > 0) | (b * b < c));
}

/* isInside — rt/geometry.d:25-28,127-130,165-170,334-337 */
template <int LEVEL>
DEV bool geom_is_inside(const Ctx &cx, int gid, D3 p)
{
    GeomP G = cx.geoms + gid;
    const int type = G->type;
    if (type == C2RT_GEOM_SPHERE) {
        return sqmag(ld3(G->p) - p) < G->q[0];
    } else if (type == C2RT_GEOM_CUBE) {
        const double hs = G->p[3] * 0.5;
        return (fabs(p.x - G->p[0]) <= hs) & (fabs(p.y - G->p[1]) <= hs) & (fabs(p.z - G->p[2]) <= hs);
    } else if (type == C2RT_GEOM_PLANE) {
        return false;
    } else {
        if constexpr (LEVEL > 0) {
            const bool a = geom_is_inside<LEVEL - 1>(cx, G->left, p);
            const bool b = geom_is_inside<LEVEL - 1>(cx, G->right, p);
            return type == C2RT_GEOM_CSG_UNION ? (a | b) : (type == C2RT_GEOM_CSG_INTER ? (a & b) : (a & !b));
        } else {
            return false;
        }
    }
}

/* ------------------------------------------------------------------ */
/* CSG — rt/geometry.d:243-403                                          */
/* ------------------------------------------------------------------ */

template <int LEVEL, int NEED>
__device__ __forceinline__ bool geom_intersect(const Ctx &cx, int gid, const ORay &r, Hit &h, bool full, int base);

/* CsgOp.intersect (+ CsgDiff.intersect) for a CSG whose subtree has at most
 * LEVEL nesting levels.  The hit lists of findAllIntersections
 * (rt/geometry.d:271-290) are kept in this level's LDS slab as
 * (dist, 16-bit tag = leaf<<4 | side<<3 | k); they are concatenated left-then-right
 * and shell-sorted exactly as util/array.d:95-111 does (same tie behaviour),
 * walked with the in/out toggles of rt/geometry.d:303-329 (including the
 * `current.g is left` leaf-identity test), and the winning hit is then
 * re-derived by replaying its child's stepping up to k.
 *
 * The four child-stepping loops (collect left, collect right, replay left,
 * replay right) run as ONE wave-uniform loop with a SINGLE call site for the
 * level below, so every nesting level is inlined exactly once: code size is
 * linear in the depth, there are no out-of-line calls and no scratch, and the
 * child's geometry record stays a scalar load.  Whether the replayed hit needs
 * its normal / u,v is a per-lane flag (`full`), because lanes replay at
 * different steps. */
/* LDS: one hit STACK per wave instead of a fixed 16-entry slab per nesting level.  The list of a
 * CsgOp starts at the per-lane index `base`; while a child is being stepped the child's own lists
 * live above the parent's current top (base + n + k) and are dead when the child returns, so the
 * parent's next entry overwrites them.  Typical trees need 4 entries per level (two hits per
 * primitive child) where the slabs reserved 16: a depth-4 scene runs in 20 KiB per wave instead of
 * 40, i.e. two waves per SIMD instead of one.  A lane that would push beyond csg_cap raises
 * Ctx::overflow and stops collecting; its tile is redone by the full-capacity launch
 * (16 entries x depth, which cannot overflow: every level holds at most 8 + 8). */
template <int LEVEL, int NEED>
__device__ __forceinline__ bool csg_intersect(const Ctx &cx, GeomP G, const ORay &ray, Hit &h, bool full, int base)
{
    static_assert(LEVEL >= 1, "CSG needs a stack");
    double *ldist = reinterpret_cast<double *>(cx.lds) + cx.lane + base * kWave;
    uint16_t *ltag = reinterpret_cast<uint16_t *>(cx.lds + cx.csg_cap * (kWave * 8)) + cx.lane + base * kWave;
    const int room = cx.csg_cap - base; /* entries this list may use */
    const int type = G->type, left = G->left, right = G->right, flags = G->flags;
    const D3 d = ray.d;
    const bool want_full = NEED == kFull || (NEED == kRt && full);

    int nL = 0, n = 0;
    int wside = -1, wk = 0; /* the winning entry: which child, which of its hits */
    Hit t;
    t.dist = 1e99;
    constexpr int kPasses = NEED == kBool ? 2 : 4; /* 0/1: collect left/right, 2/3: replay left/right */
#pragma unroll 1
    for (int pass = 0; pass < kPasses; ++pass) {
        const int side = pass & 1;
        const int child = side ? right : left; /* wave-uniform */
        const bool replay = pass >= 2;
        if (replay && wside != side) continue; /* this lane's winner came from the other child */
        const int limit = replay ? wk + 1 : kMaxCsgHits;
        const bool child_cube = cx.geoms[child].type == C2RT_GEOM_CUBE && (cx.geoms[child].flags & kGeomFinite); /* scalar */
        (void)child_cube; /* see csg_intersect_leaf */
        ORay rr = ray;
        double cur = 0;
        int k = 0;
        while (k < limit) {
            t.dist = 1e99;
            /* the child's lists go above this list's top; a replay no longer needs this list */
            if (!geom_intersect<LEVEL - 1, kRt>(cx, child, rr, t, replay && k == wk && want_full, replay ? base : base + n + k)) break;
            t.dist += cur;
            cur = t.dist;
            rr.o = t.p + d * 1e-6;
            if (!replay) {
                if (n + k >= room) { cx.overflow = true; break; }
                ldist[(n + k) * kWave] = t.dist;
                ltag[(n + k) * kWave] = csg_tag(t.g, side, k);
            }
            ++k;
        }
        if (replay) break; /* `t` is the re-derived winner (data = current, rt/geometry.d:326) */
        if (k == kMaxCsgHits && cx.trunc_counter) atomicAdd(cx.trunc_counter, 1ull);
        if (side == 0) nL = k;
        n += k;
        /* exact shortcuts (GeomFlags): nothing can switch the operator on */
        if (k == 0 && (flags & (side ? kCsgShortB : kCsgShortA))) return false;
        if (side == 0) continue;

        /* both lists are in: sort — util/array.d:95-111 (index rewound by the inner while) */
        for (int inc = n / 2; inc;) {
            for (int i = 0; i < n; ++i) {
                const double ed = ldist[i * kWave];
                const uint16_t et = ltag[i * kWave];
                while (i >= inc && ldist[(i - inc) * kWave] > ed) {
                    ldist[i * kWave] = ldist[(i - inc) * kWave];
                    ltag[i * kWave] = ltag[(i - inc) * kWave];
                    i -= inc;
                }
                ldist[i * kWave] = ed;
                ltag[i * kWave] = et;
            }
            inc = next_gap(inc);
        }
        bool inL = (nL & 1) != 0, inR = ((n - nL) & 1) != 0;
        int win = -1;
        for (int i = 0; i < n; ++i) {
            const uint32_t tag = ltag[i * kWave];
            const bool isL = (int)(tag >> 4) == left;
            inL ^= isL;
            inR ^= !isL;
            const bool in = type == C2RT_GEOM_CSG_UNION ? (inL | inR)
                          : (type == C2RT_GEOM_CSG_INTER ? (inL & inR) : (inL & !inR));
            if (in) { win = i; break; }
        }
        if (win < 0) return false;
        const double wdist = ldist[win * kWave];
        if (wdist > h.dist) return false;
        if (NEED == kBool) { h.dist = wdist; return true; }
        const uint32_t wtag = ltag[win * kWave];
        wside = (wtag >> 3) & 1;
        wk = wtag & 7;
    }
    h = t;

    if (want_full && type == C2RT_GEOM_CSG_DIFF) { /* CsgDiff.intersect — rt/geometry.d:382-397 */
        if (geom_is_inside<LEVEL - 1>(cx, right, h.p - d * 1e-6) != geom_is_inside<LEVEL - 1>(cx, right, h.p + d * 1e-6))
            h.code ^= kCodeFlip; /* normal = -normal */
    }
    return true;
}

/* The same for a CSG whose children are both primitives (the innermost level, by
 * far the most executed one): the three stepping loops are written out, with
 * compile-time NEED for the collect loops — measurably faster than the single
 * call-site form, and the duplicated primitive code is small. */
template <int NEED>
__device__ __forceinline__ bool csg_intersect_leaf(const Ctx &cx, GeomP G, const ORay &ray, Hit &h, bool full, int base)
{
    constexpr int LEVEL = 1;
    double *ldist = reinterpret_cast<double *>(cx.lds) + cx.lane + base * kWave;
    uint16_t *ltag = reinterpret_cast<uint16_t *>(cx.lds + cx.csg_cap * (kWave * 8)) + cx.lane + base * kWave;
    const int room = cx.csg_cap - base;
    const int type = G->type, left = G->left, right = G->right, flags = G->flags;
#if !C2RT_CSG_CERTAIN
    const D3 d = ray.d;
#endif
#if C2RT_TILE_STATS
    if (cx.lane_stats) {
        const unsigned long long act = __ballot(true);
        if (cx.lane == (int)__builtin_ctzll(act)) { atomicAdd(cx.lane_stats + 0, (unsigned long long)__builtin_popcountll(act)); atomicAdd(cx.lane_stats + 1, 64ull); }
    }
#endif

#if C2RT_CSG_CERTAIN /* the frame units only (c2rt_trace_common.inc): the query units compile the parent's text */
    int wside = 0, wk = 0;
    uint32_t wcode = 0;
    (void)wcode; /* (read by the instances that need the hit record) */
    double wdist = 0;
    /* The winner decided from the children's closed-form intervals (csg_certain.h), per lane, where that is certain:
     * such a lane skips both collect loops, the lists and the sort, and takes its record from the literal stepping
     * loop below (for hit 0 that is one literal call on the unmoved ray).  An unsure lane runs the literal evaluation,
     * under divergence.  Not for kRt: the innermost level of a nested tree starts from restarted origins, 1e-6 off a
     * surface, where nothing is certain. */
    bool certain = false;
    if constexpr (NEED != kRt) {
        /* (kBool: `full` is node_intersect's `own` — a wave whose shadow rays all start on this very node asks nothing) */
        if (cx.csg_certain && (flags & kCsgCertain) && !(NEED == kBool && __all(full))) { /* wave-uniform */
            auto child = [&](int c) {
                const double co[3] = {ray.o.x, ray.o.y, ray.o.z}, cd[3] = {ray.d.x, ray.d.y, ray.d.z};
                GeomP C = cx.geoms + c;
                if (C->type == C2RT_GEOM_SPHERE) {
                    const double cc[3] = {C->p[0], C->p[1], C->p[2]};
                    return cc_sphere(co, cd, cc, C->p[3], 1.0);
                }
                const double lo[3] = {C->q[0], C->q[1], C->q[2]}, hi[3] = {C->q[3], C->q[4], C->q[5]};
                if constexpr (kLean) { /* the direction's reciprocals are there (prep_dir): 1 / d.x = -rx */
                    const double ri[3] = {-ray.rx, -ray.ry, -ray.rz};
                    return cc_cube(co, cd, lo, hi, 1.0, ri);
                }
                return cc_cube(co, cd, lo, hi, 1.0);
            };
            const CcResult w = cc_decide_with(type - C2RT_GEOM_CSG_UNION, (flags & kCsgShortA) != 0, (flags & kCsgShortB) != 0,
                                              [&] { return child(left); }, [&] { return child(right); });
#if C2RT_TILE_STATS
            if (cx.lane_stats) {
                const unsigned long long act = __ballot(true), sure = __ballot(w.kind != CC_R_UNSURE);
                if (cx.lane == (int)__builtin_ctzll(act)) {
                    atomicAdd(cx.lane_stats + 4 + 3 * kRegions + 0, (unsigned long long)__builtin_popcountll(sure));
                    atomicAdd(cx.lane_stats + 4 + 3 * kRegions + 1, (unsigned long long)__builtin_popcountll(act & ~sure));
                }
            }
#endif
            if (w.kind == CC_R_NOHIT) return false;
            if (w.kind == CC_R_HIT) {
                if (w.dist - w.del > h.dist) return false; /* the literal `wdist > h.dist`, for every wdist within del */
                if (NEED == kBool) {
                    /* (the callers of kBool — test_visibility — read no distance: h.dist stays) */
                    if (w.dist + w.del < h.dist) return true;
                } else {
                    certain = true;
                    wside = w.side;
                    wk = w.k;
                }
            }
        }
    }

    const D3 d = ray.d;

    if (!certain) {
#endif
    int nL = 0, nR = 0;
    int n = 0;
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
        const int child = side ? right : left;
        /* Unused since the cube early-out went (cube_intersect's comment), and kept: this read is where the compiler
         * places the scalar load of the child's record, which geom_intersect needs anyway — without it the load moves
         * and every instance is scheduled differently from the code all measurements were taken on. */
        const bool child_cube = cx.geoms[child].type == C2RT_GEOM_CUBE && (cx.geoms[child].flags & kGeomFinite); /* scalar */
        (void)child_cube;
        ORay rr = ray;
        double cur = 0;
        int k = 0;
        while (k < kMaxCsgHits) {
            Hit t;
            t.dist = 1e99;
#if C2RT_TILE_STATS
            if (cx.lane_stats) {
                const unsigned long long act = __ballot(true);
                if (cx.lane == (int)__builtin_ctzll(act)) { atomicAdd(cx.lane_stats + 2, (unsigned long long)__builtin_popcountll(act)); atomicAdd(cx.lane_stats + 3, 64ull); }
            }
#endif
            /* (the face code of every collected hit goes into its tag: see the winner below) */
            if (!geom_intersect<0, kFull>(cx, child, rr, t, false, 0)) break;
            t.dist += cur;
            cur = t.dist;
            rr.o = t.p + d * 1e-6;
            if (n + k >= room) { cx.overflow = true; break; }
            ldist[(n + k) * kWave] = t.dist;
            ltag[(n + k) * kWave] = csg_tag(t.code & (kCodeAxis | kCodeSide), side, k); /* the leaf IS the child: `side` names it */
            ++k;
        }
        if (side == 0) nL = k; else nR = k;
        if (k == kMaxCsgHits && cx.trunc_counter) atomicAdd(cx.trunc_counter, 1ull);
        n += k;
        /* exact shortcuts (GeomFlags): nothing can switch the operator on */
        if (k == 0 && (flags & (side ? kCsgShortB : kCsgShortA))) return false;
    }

    /* The regular case — a child contributes no hit or exactly two (a ray through a convex primitive: in, out) and
     * all distances are distinct: the sorted order is then unique, both in/out states start "outside" (even
     * counts) and the walk of rt/geometry.d:303-329 visits L0 < L1 and R0 < R1 merged; its first entry at which
     * the operator is on is decided by comparisons —
     *   Union: the earlier of L0, R0;   Inter: L0 if R0 < L0 < R1, R0 if L0 < R0 < L1;
     *   Diff:  L0 unless R0 < L0 < R1, else R1 if L0 < R1 < L1 —
     * without sorting the lists or walking them (same winner, hence the same bits).  Taken when EVERY active lane
     * is regular; one lane with a tie, a NaN distance, one or three hits on a child (origin inside it, a grazing
     * step) sends the wave through the literal sort and walk below.  `left != right`: the walk tells the lists
     * apart by leaf identity (`current.g is left`), so Op(a, a) is not regular either. */
#if !C2RT_CSG_CERTAIN
    int wside = 0, wk = 0;
    uint32_t wcode = 0;
    (void)wcode; /* (read by the instances that need the hit record) */
    double wdist = 0;
#endif
    bool have = false, regular = false;
    if (left != right) {
        const bool hasL = nL == 2, hasR = nR == 2;
        bool ok = (hasL | (nL == 0)) & (hasR | (nR == 0));
        const double a0 = n >= 2 ? ldist[0] : 0.0, a1 = n >= 2 ? ldist[kWave] : 0.0;
        const double a2 = n >= 4 ? ldist[2 * kWave] : 0.0, a3 = n >= 4 ? ldist[3 * kWave] : 0.0;
        const double L0 = a0, L1 = a1, R0 = hasL ? a2 : a0, R1 = hasL ? a3 : a1;
        ok &= !hasL | (L0 < L1);
        ok &= !hasR | (R0 < R1);
        const bool both = hasL & hasR;
        ok &= !both | (((L0 < R0) | (L0 > R0)) & ((L0 < R1) | (L0 > R1)) & ((L1 < R0) | (L1 > R0)) & ((L1 < R1) | (L1 > R1)));
        if (__all(ok)) {
            regular = true;
            const bool L0inR = hasR & (R0 < L0) & (L0 < R1);
            const bool R0inL = hasL & (L0 < R0) & (R0 < L1);
            const bool R1inL = hasL & (L0 < R1) & (R1 < L1);
            bool candL0, candR0, candR1;
            if (type == C2RT_GEOM_CSG_UNION) { candL0 = hasL & !(hasR & (R0 < L0)); candR0 = hasR & !candL0; candR1 = false; }
            else if (type == C2RT_GEOM_CSG_INTER) { candL0 = hasL & L0inR; candR0 = hasR & R0inL; candR1 = false; }
            else { candL0 = hasL & !L0inR; candR0 = false; candR1 = hasR & R1inL & !candL0; }
            have = candL0 | candR0 | candR1;
            wside = candL0 ? 0 : 1;
            wk = candR1 ? 1 : 0;
            wdist = candL0 ? L0 : (candR0 ? R0 : R1);
            if (have) wcode = ltag[((wside ? nL : 0) + wk) * kWave] >> 4;
        }
    }
    if (!regular) {
        /* sort — util/array.d:95-111 (index rewound by the inner while) */
        for (int inc = n / 2; inc;) {
            for (int i = 0; i < n; ++i) {
                const double ed = ldist[i * kWave];
                const uint16_t et = ltag[i * kWave];
                while (i >= inc && ldist[(i - inc) * kWave] > ed) {
                    ldist[i * kWave] = ldist[(i - inc) * kWave];
                    ltag[i * kWave] = ltag[(i - inc) * kWave];
                    i -= inc;
                }
                ldist[i * kWave] = ed;
                ltag[i * kWave] = et;
            }
            inc = next_gap(inc);
        }

        bool inL = (nL & 1) != 0, inR = (nR & 1) != 0;
        int win = -1;
        for (int i = 0; i < n; ++i) {
            const uint32_t tag = ltag[i * kWave];
            const bool isL = (left == right) | (((tag >> 3) & 1u) == 0); /* `current.g is left`: the leaf is the child itself */
            inL ^= isL;
            inR ^= !isL;
            const bool in = type == C2RT_GEOM_CSG_UNION ? (inL | inR)
                          : (type == C2RT_GEOM_CSG_INTER ? (inL & inR) : (inL & !inR));
            if (in) { win = i; break; }
        }
        have = win >= 0;
        if (have) {
            wdist = ldist[win * kWave];
            const uint32_t wtag = ltag[win * kWave];
            wside = (wtag >> 3) & 1;
            wk = wtag & 7;
            wcode = wtag >> 4;
        }
    }
    if (!have) return false;
    if (wdist > h.dist) return false;
    if (NEED == kBool) { h.dist = wdist; return true; }
#if C2RT_CSG_CERTAIN
    } /* (!certain) */
#endif

    /* re-derive the winning IntersectionData (data = current, rt/geometry.d:326) */
    C2RT_REGION_BEGIN(cx, kRegReplay)
    const int child = wside ? right : left;
    Hit t;
    /* The winner is its child's FIRST hit (a CsgUnion's and a CsgInter's always, a CsgDiff's when the left
     * child's entry point lies outside the right child): its record needs no replay.  The stepping loop met it
     * with the unmoved ray and cur = 0, so its distance is the primitive's own `mult` (mult + 0.0 == mult), its
     * point is that primitive's `o + d * mult` — Plane rt/geometry.d:40, Sphere :107, Cube :213 — its leaf is
     * the child and its face code sits in the tag: the same operands, the same bits. */
#if C2RT_CSG_CERTAIN
    if (wk == 0 && !certain) {
#else
    if (wk == 0) {
#endif
        t.dist = wdist;
        t.p = ray.o + d * wdist;
        t.g = child;
        t.code = (int)wcode;
    } else {
        /* (a certain lane has no list: its record comes from here whatever its k, and for k = 0 the loop below is empty
         * and this is one literal call on the unmoved ray, the very call the collect loop would have begun with) */
        ORay rr = ray;
        double cur = 0;
        for (int i = 0; i < wk; ++i) {
            Hit s;
            s.dist = 1e99;
            geom_intersect<0, kPoint>(cx, child, rr, s, false, 0);
            s.dist += cur;
            cur = s.dist;
            rr.o = s.p + d * 1e-6;
        }
        t.dist = 1e99;
        geom_intersect<0, NEED>(cx, child, rr, t, full, 0);
        t.dist += cur;
#if C2RT_CSG_CERTAIN
        if (certain && t.dist > h.dist) return false; /* the literal rejection, on the literal distance */
#endif
    }
    h = t;

    if (C2RT_WANT_FULL(NEED, full) && type == C2RT_GEOM_CSG_DIFF) { /* CsgDiff.intersect — rt/geometry.d:382-397 */
        if (geom_is_inside<LEVEL - 1>(cx, right, h.p - d * 1e-6) != geom_is_inside<LEVEL - 1>(cx, right, h.p + d * 1e-6))
            h.code ^= kCodeFlip; /* normal = -normal */
    }
    C2RT_REGION_END(cx, kRegReplay)
    return true;
}

/* Geometry.intersect on a given record: `G` is wave-uniform, so this is a scalar branch. */
template <int LEVEL, int NEED>
__device__ __forceinline__ bool geom_intersect_rec(const Ctx &cx, GeomP G, int gid, const ORay &r, Hit &h, bool full, int base)
{
    const int type = G->type;
    if (type == C2RT_GEOM_PLANE) return plane_intersect<NEED>(cx.bad, G, gid, r, h, full);
    if (type == C2RT_GEOM_SPHERE) return sphere_intersect<NEED>(cx.bad, G, gid, r, h, full);
    if (type == C2RT_GEOM_CUBE) return cube_intersect<NEED>(cx.bad, G, gid, r, h, full);
    if constexpr (LEVEL >= 2) {
        return csg_intersect<LEVEL, NEED>(cx, G, r, h, full, base);
    } else if constexpr (LEVEL == 1) {
        return csg_intersect_leaf<NEED>(cx, G, r, h, full, base);
    } else {
        return false;
    }
}

/* `base`: first free entry of this lane's hit stack (CsgOps only) */
template <int LEVEL, int NEED>
__device__ __forceinline__ bool geom_intersect(const Ctx &cx, int gid, const ORay &r, Hit &h, bool full, int base)
{
    return geom_intersect_rec<LEVEL, NEED>(cx, cx.geoms + gid, gid, r, h, full, base);
}

/* ------------------------------------------------------------------ */
/* nodes — rt/node.d:23-49, rt/transform.d:57-86                         */
/* ------------------------------------------------------------------ */

/* The world ray normalised once for every node whose matrix is the identity:
 * undoDirection(dir) == dir there, so `magnitude` and `normalize`
 * (rt/node.d:34-36) give the same bits for all of them. */
struct RayW {
    D3 o, d;
    D3 dn;      /* d * (1/|d|) */
    double len; /* |d| */
    double inv; /* 1 / len, correctly rounded */
    double A;   /* |dn|^2 */
};
DEV RayW make_ray(Oob &bad, D3 o, D3 d)
{
    RayW r;
    r.o = o;
    r.d = d;
    len_inv_unit(bad, sqmag(d), r.len, r.inv); /* every caller hands in a normalised direction */
    const double inv = r.inv;
    r.dn = mk(d.x * inv, d.y * inv, d.z * inv);
    r.A = sqmag(r.dn);
    return r;
}

/* Node.intersect; `best.dist` is data.dist (world units) in and out.  `last` (wave-uniform): no
 * further node will be tested against this ray, so nobody reads the updated best.dist again (it only
 * serves as the next node's limit) and its division is skipped. */
/* `own` (kBool only, per lane): the ray is a shadow ray that starts ON this node — 1e-6 off its surface, where
 * csg_certain.h decides nothing; a wave of such lanes does not ask it (csg_intersect_leaf). */
template <int LEVELS, int NEED, int PO>
#if C2RT_CSG_CERTAIN
DEV bool node_intersect(const Ctx &cx, NodeP N, const RayW &ray, Hit &best, bool last = false, bool own = false)
#else
DEV bool node_intersect(const Ctx &cx, NodeP N, const RayW &ray, Hit &best, bool last = false)
#endif
{
    const uint32_t flags = N->flags;
    ORay rc;
    rc.o = ray.o;
    double len, linv;
    if (!(flags & kNodeZeroOffset)) rc.o = rc.o - ld3(N->off);
    if ((PO & kSpecIdentity) || (flags & kNodeIdentityMatrix)) {
        rc.d = ray.dn;
        rc.A = ray.A;
        len = ray.len;
        linv = ray.inv;
    } else {
        rc.o = mulvm(rc.o, N->inv);
        const D3 dd = mulvm(ray.d, N->inv);
        len_inv(cx.bad, sqmag(dd), len, linv);
        rc.d = mk(dd.x * linv, dd.y * linv, dd.z * linv);
        rc.A = sqmag(rc.d);
    }
    const int gid = N->geom;
    GeomP G = &N->g; /* the node's own copy of its root geometry record */
    Hit h;
    if constexpr (PO & kSpecPlanes) { /* the instance holds Plane.intersect only */
        prep_dir(rc, kPrepY);
        h.dist = best.dist * len;
        if (!plane_intersect<NEED>(cx.bad, G, gid, rc, h, false)) return false;
    } else {
        /* cubes and CSG trees are expensive to miss: bounding-sphere reject first */
        if (G->type >= C2RT_GEOM_CUBE && (G->flags & kGeomBounded) && misses_bound(G, rc)) return false;
        /* the reciprocals this geometry's tests divide by, once per direction (wave-uniform type) */
        prep_dir(rc, G->type == C2RT_GEOM_PLANE ? kPrepY : (G->type == C2RT_GEOM_SPHERE ? kPrepA : (G->type == C2RT_GEOM_CUBE ? (kPrepY | kPrepXZ) : (kPrepY | kPrepXZ | kPrepA))));
        h.dist = best.dist * len;
#if C2RT_TILE_STATS
        if (G->type > C2RT_GEOM_CUBE) { /* (scalar) a CsgOp node: the whole evaluation, all lanes back at END */
            C2RT_REGION_BEGIN(cx, kRegCsg)
            const bool hit_ = geom_intersect_rec<LEVELS, NEED>(cx, G, gid, rc, h, C2RT_OWN(NEED), 0);
            C2RT_REGION_END(cx, kRegCsg)
            if (!hit_) return false;
        } else
#endif
        if (!geom_intersect_rec<LEVELS, NEED>(cx, G, gid, rc, h, C2RT_OWN(NEED), 0)) return false;
    }
    if (NEED == kBool) return true;
    if (!last) best.dist = div_r(cx.bad, h.dist, len, linv);
    /* the hit stays in the node's object space; hit_surface applies the rest of Node.intersect
     * (rt/node.d:41-47) to the one that ends up closest */
    best.g = h.g;
    best.code = h.code;
    best.p = h.p;
    return true;
}

/* The rest of the closest hit's IntersectionData, for the lanes whose closest node is N (wave-uniform):
 * the leaf's normal and u,v from the object-space point — Plane rt/geometry.d:46-53, Sphere :113-122, Cube
 * :217-230 (u, v and the normal of a permuted face pair, un-permuted), CsgDiff's flip :392-396 — then
 * Node.intersect's transform of normal and point, rt/node.d:41-47.  The leaf differs per lane (the cube
 * or the sphere of a CsgDiff), so its record is read per lane. */
/* (the leaf's part: G is the node's own record — scalar loads — when the node's geometry is a primitive, and a
 * per-lane record when it is a CsgOp, whose leaf differs from lane to lane) */
DEV void leaf_surface(const Ctx &cx, GeomP G, int type, const Hit &h, UVWant want_uv, Surf &s, D3 &n, bool &axis_n)
{
    axis_n = true; /* n is an exact signed unit axis: normalize(n) == n */
    s.u = s.v = 0;
    if (type == C2RT_GEOM_PLANE) {
        n = mk(0, 1, 0);
        s.u = h.p.x;
        s.v = h.p.z;
    } else if (type == C2RT_GEOM_CUBE) {
        const D3 c = ld3(G->p);
        const int axis = h.code & kCodeAxis;
        const double side = (h.code & kCodeSide) ? 1.0 : -1.0;
        n = mk(axis == 0 ? side : 0.0, axis == 1 ? side : 0.0, axis == 2 ? side : 0.0);
        /* Y faces: (x, z); X faces, project(1,0,2): (y, z); Z faces, project(0,2,1): (x, y) */
        s.u = axis == 0 ? h.p.y - c.y : h.p.x - c.x;
        s.v = axis == 2 ? h.p.y - c.y : h.p.z - c.z;
    } else {
        const D3 c = ld3(G->p);
        const D3 pc = h.p - c;
        n = normalized(cx.bad, pc);
        axis_n = false;
        /* u,v cost an atan2 and an asin and are read by textured shaders (and the probe) only */
        if (want_uv.kind != kUVNone) {
            C2RT_REGION_BEGIN(cx, kRegSphereUV)
            sphere_uv(pc.x, pc.z, pc.y / G->p[3], want_uv, s.u, s.v);
            C2RT_REGION_END(cx, kRegSphereUV)
        }
    }
}

template <int PO>
DEV void hit_surface(const Ctx &cx, NodeP N, const Hit &h, UVWant want_uv, Surf &s)
{
    D3 n;
    bool axis_n;
    const int root = (PO & kSpecPlanes) ? (int)C2RT_GEOM_PLANE : N->g.type; /* wave-uniform */
    if (root <= C2RT_GEOM_CUBE) {
        leaf_surface(cx, &N->g, root, h, want_uv, s, n, axis_n);
    } else {
        GeomP G = cx.geoms + h.g;
        leaf_surface(cx, G, G->type, h, want_uv, s, n, axis_n);
    }
    if (h.code & kCodeFlip) n = -n;
    const uint32_t flags = N->flags;
    if ((PO & kSpecIdentity) || (flags & kNodeIdentityMatrix)) {
        /* normalize() of an exact unit axis is the identity (sqrt(1) = 1, 1/1 = 1) */
        if (!axis_n) {
            double len, inv;
            len_inv_unit(cx.bad, sqmag(n), len, inv);
            n = n * inv;
        }
        s.n = n;
        s.p = h.p;
    } else {
        /* (a Plane's world normal is the same for every hit: kNodePlaneNormal, c2rt_device.h; a CsgOp's leaf
         * plane may carry the flip, so only a root plane reads it) */
        if (root == C2RT_GEOM_PLANE && (flags & kNodePlaneNormal)) s.n = ld3(N->g.q);
        else s.n = normalized(cx.bad, mulvm(n, N->tinv));
        s.p = mulvm(h.p, N->m);
    }
    if (!(flags & kNodeZeroOffset)) s.p = s.p + ld3(N->off);
}

/* Scene.testVisibility — rt/scene.d:62-78 */
/* `self`: the node the segment starts on (a shadow ray of its closest hit), -1 when the caller does not know */
template <int LEVELS, int PO>
#if C2RT_CSG_CERTAIN
DEV bool test_visibility(const Ctx &cx, D3 from, D3 to, uint32_t node_mask, bool ground_only, int self = -1)
#else
DEV bool test_visibility(const Ctx &cx, D3 from, D3 to, uint32_t node_mask, bool ground_only)
#endif
{
    const D3 raw = to - from;
    if (!(PO & kSpecPlanes) && ground_only) { /* wave-uniform */
        /* plane_points_away for the ground plane (identity matrix, zero offset) */
        const bool sane = (fabs(raw.x) < 1e150) & (fabs(raw.z) < 1e150);
        const bool up = (raw.y > 1e-150) & (raw.y < 1e150), down = (raw.y < -1e-150) & (raw.y > -1e150);
        if (__all(sane & (((from.y > cx.ground_y) & up) | ((from.y < cx.ground_y) & down)))) return true;
    }
    const uint32_t nn = cx.n_nodes;
    uint32_t n = next_node(node_mask, 0);
    if constexpr (PO & kSpecPlanes) { /* every lane's ray provably leaves the leading planes behind: no ray needed yet */
        while (n < nn && __all(plane_points_away(cx.nodes + n, from, raw))) n = next_node(node_mask, n + 1);
        if (n >= nn) return true;
    }
    double rlen, rinv;
    len_inv(cx.bad, sqmag(raw), rlen, rinv);
    const D3 dir = mk(raw.x * rinv, raw.y * rinv, raw.z * rinv); /* normalized(raw) */
    const RayW ray = make_ray(cx.bad, from, dir);
    Hit temp;
    temp.dist = rlen;                                             /* magnitude(raw) */
    for (; n < nn; n = next_node(node_mask, n + 1)) /* scalar loop, file order */
#if C2RT_CSG_CERTAIN
        if (node_intersect<LEVELS, kBool, PO>(cx, cx.nodes + n, ray, temp, false, self == (int)n)) return false;
#else
        if (node_intersect<LEVELS, kBool, PO>(cx, cx.nodes + n, ray, temp)) return false;
#endif
    return true;
}

/* ------------------------------------------------------------------ */
/* shading — rt/shader.d:67-105,197-250                                  */
/* ------------------------------------------------------------------ */

/* MLC ("multi-light"): the instance for scenes with MORE THAN ONE light — the light loop, and the
 * culling masks of lights 1.. derived per sample.  Scenes with at most one light (every scene the
 * reference ships) run the MLC = false instance, in which the one light is straight-line code:
 * nothing of the hit has to stay live for a next light, so the hit point, normal and view direction
 * die before the shadow test (below). */
/* What one visible light adds (rt/shader.d:88-103, 219-243): avgColor / avgSpecular of that light. */
/* lightColor / float(d^2), rt/shader.d:97: three channels over one denominator.  lean::: the refined
 * reciprocal once (fp64_lean.h, fp32 part) when the host has found the light's three numerators in
 * range (DevLight::lit bit 1: each +0 or within 2^+-60); the denominator's own window is tested here */
DEV F3 base_light(Oob &bad, LightP L, double r2)
{
    const float r2f = (float)r2;
    if (kLean && (L->lit & 2u)) {
        oob_note_f32(bad, r2f);
        const float rr = rcp_refined_f32(r2f);
        return mkf(div_with_f32(L->color[0], r2f, rr), div_with_f32(L->color[1], r2f, rr), div_with_f32(L->color[2], r2f, rr));
    }
    return ldf3(L->color) / r2f;
}
DEV void light_terms(Oob &bad, LightP L, D3 lightPos, D3 p, D3 N, D3 rd, bool phong, double &cosTheta, F3 &baseLight, double &cosGamma)
{
    /* squaredMagnitude(p - lightPos) == squaredMagnitude(lightPos - p) bit for bit (IEEE a - b is
     * exactly -(b - a), and the squares drop the sign): one vector, one sum of squares for both
     * normalize(lightPos - p) and the 1/r^2 term */
    const D3 lv = lightPos - p;
    const double r2 = sqmag(lv);
    double rlen, rinv;
    len_inv(bad, r2, rlen, rinv);
    const D3 lightDir = mk(lv.x * rinv, lv.y * rinv, lv.z * rinv);
    cosTheta = dot(lightDir, N);
    baseLight = base_light(bad, L, r2);
    cosGamma = 0;
    if (phong) {
        /* reflect(-lightDir, N) — rt/imported_types.d:62-67 */
        const D3 ml = -lightDir;
        /* (the mirror image of a unit vector in a unit normal is unit up to rounding: the integer form) */
        const D3 rv = ml - N * (2 * dot(ml, N));
        double rl, ri;
        len_inv_unit(bad, sqmag(rv), rl, ri);
        const D3 R = rv * ri;
        cosGamma = dot(R, -rd);
    }
}

template <int LEVELS, bool MLC, int PO>
#if C2RT_CSG_CERTAIN
DEV F3 shade(const RenderParams &P, const Ctx &cx, const Mat &mat, D3 rd, const Surf &h, uint32_t &shadow_rays, int self = -1)
#else
DEV F3 shade(const RenderParams &P, const Ctx &cx, const Mat &mat, D3 rd, const Surf &h, uint32_t &shadow_rays)
#endif
{
    const bool phong = mat.shader_type == C2RT_SHADER_PHONG;
    const D3 N = dot(rd, h.n) < 0 ? h.n : -h.n; /* faceforward — rt/imported_types.d:69-73 */
    C2RT_REGION_BEGIN(cx, kRegTexture)
    const F3 diffuse = mat.tex_type >= 0 ? tex_color(P, mat, h.u, h.v) : mat.color;
    C2RT_REGION_END(cx, kRegTexture)
    F3 lightContrib = mkf(P.ambient[0], P.ambient[1], P.ambient[2]);
    F3 specular = mkf(0, 0, 0);
    if constexpr (!MLC) {
        /* at most one light (every scene the reference ships): straight-line code */
        if (P.n_lights) {
            LightP L = (LightP)P.lights;
            F3 avgColor = mkf(0, 0, 0), avgSpecular = mkf(0, 0, 0);
            if (L->lit & 1u) {
                const D3 lightPos = ld3(L->pos);
                shadow_rays += 1;
                /* Everything the lit branch reads from the hit is evaluated BEFORE the visibility test (same
                 * operations on the same operands, so the same bits; a shadowed sample wastes two
                 * normalisations): across the test — the register peak of the kernel, a CSG walk inside
                 * a node loop — only cosTheta, baseLight and cosGamma stay live instead of p, N and rd. */
                const D3 from = h.p + N * 1e-6;
                double cosTheta, cosGamma;
                F3 baseLight;
                light_terms(cx.bad, L, lightPos, h.p, N, rd, phong, cosTheta, baseLight, cosGamma);
                C2RT_REGION_BEGIN(cx, kRegShadow)
                const bool visible = test_visibility<LEVELS, PO>(cx, from, lightPos, cx.shadow_mask0, cx.shadow_ground_only C2RT_SELF);
                C2RT_REGION_END(cx, kRegShadow)
                if (visible) {
                    C2RT_REGION_BEGIN(cx, kRegLight)
                    if (cosTheta > 0) avgColor = avgColor + baseLight * (float)cosTheta;
                    if (phong & (cosGamma > 0))
                        avgSpecular = avgSpecular + baseLight * c2_pow_f32(cosGamma, mat.exponent) * mat.strength;
                    C2RT_REGION_END(cx, kRegLight)
                }
            }
            /* `/ numSamples` with numSamples == 1 (rt/light.d:56-59) is exact */
            lightContrib = lightContrib + avgColor;
            specular = specular + avgSpecular;
        }
    } else {
        /* Several lights: the visibility of up to 32 lights first (only the hit point and the facing normal
         * are live across the shadow rays — a nested-CSG walk inside a node loop, the register peak of the
         * kernel), then their contributions in the reference's order.  A shadowed light adds exact zeros, as
         * in the reference. */
        const D3 p = h.p;
        const double exponent = mat.exponent;
        const float strength = mat.strength;
        const uint32_t nl = P.n_lights;
        for (uint32_t l0 = 0; l0 < nl; l0 += 32u) {
            const uint32_t l1 = l0 + 32u < nl ? l0 + 32u : nl;
            uint32_t vis = 0;
            for (uint32_t l = l0; l < l1; ++l) {
                LightP L = (LightP)P.lights + l;
                if (L->lit & 1u) {
                    shadow_rays += 1;
                    const D3 from = p + N * 1e-6;
                    if (test_visibility<LEVELS, PO>(cx, from, ld3(L->pos), l == 0 ? cx.shadow_mask0 : light_shadow_mask(P, cx.mask_slot, l), l == 0 && cx.shadow_ground_only C2RT_SELF))
                        vis |= 1u << (l - l0);
                }
            }
            for (uint32_t l = l0; l < l1; ++l) {
                LightP L = (LightP)P.lights + l;
                F3 avgColor = mkf(0, 0, 0), avgSpecular = mkf(0, 0, 0);
                if ((L->lit & 1u) && ((vis >> (l - l0)) & 1u)) {
                    double cosTheta, cosGamma;
                    F3 baseLight;
                    light_terms(cx.bad, L, ld3(L->pos), p, N, rd, phong, cosTheta, baseLight, cosGamma);
                    if (cosTheta > 0) avgColor = avgColor + baseLight * (float)cosTheta;
                    if (phong & (cosGamma > 0))
                        avgSpecular = avgSpecular + baseLight * c2_pow_f32(cosGamma, exponent) * strength;
                }
                lightContrib = lightContrib + avgColor;
                specular = specular + avgSpecular;
            }
        }
    }
    const F3 res = diffuse * lightContrib;
    return phong ? res + specular : res;
}

/* ------------------------------------------------------------------ */
/* camera — rt/camera.d:123-173                                          */
/* ------------------------------------------------------------------ */

template <int DOF>
DEV void screen_ray(Oob &bad, const RenderParams &P, double x, double y, int offset, Rng &rng, D3 &orig, D3 &dir)
{
    const c2rt_camera_frame &cam = P.cam;
    const D3 pos = ld3(cam.pos), upLeft = ld3(cam.up_left);
    /* (upRight - upLeft) and (downLeft - upLeft) are per-frame constants: the host
     * does the same two IEEE subtractions once (c2rt_api.cpp fill_params) */
    /* lean::: the frame's width and height divide every sample; their correctly rounded reciprocals come
     * from the host (fill_params).  No window test: x and y are pixel coordinates, 0 or in [0.3, 2^17) — a
     * numerator of +0 over a positive denominator is +0 in the lean form too */
    double fx, fy;
    if constexpr (kLean) {
        fx = div_with(x, cam.frame_width, P.cam_rw);
        fy = div_with(y, cam.frame_height, P.cam_rh);
    } else {
        fx = x / cam.frame_width;
        fy = y / cam.frame_height;
    }
    const D3 target = upLeft + ld3(P.cam_du) * fx + ld3(P.cam_dv) * fy;
    orig = pos;
    dir = target - pos; /* un-normalised: raytrace() normalises it when a node needs it */
    if constexpr (DOF) {
        const D3 raw0 = dir;
        dir = normalized(bad, raw0);
        const D3 rightDir = ld3(cam.right_dir);
        if (DOF == 2 && offset != 0) orig = orig + rightDir * (offset > 0 ? +cam.stereo_separation : -cam.stereo_separation);
        if (!cam.dof) { dir = raw0; return; }
        const double cosTheta = dot(dir, ld3(cam.front_dir));
        const double M = cam.focal_plane_dist / cosTheta;
        const D3 T = orig + dir * M;
        /* unitDiscSample — rt/camera.d:258-269: (sin, cos)(U1 * 2 pi) * sqrt(U2) */
        const double u1 = rng_next(rng);
        const double rad = sqrt(rng_next(rng));
        double sn, cs;
        lens_sincos2pi(u1, sn, cs);
        double dx = sn * rad, dy = cs * rad;
        dx *= cam.disc_multiplier;
        dy *= cam.disc_multiplier;
        orig = pos + rightDir * dx + ld3(cam.up_dir) * dy;
        if (DOF == 2 && offset != 0) orig = orig + rightDir * (offset > 0 ? +cam.stereo_separation : -cam.stereo_separation);
        dir = T - orig; /* un-normalised */
    }
}

/* ------------------------------------------------------------------ */
/* renderer — rt/renderer.d:223-376                                      */
/* ------------------------------------------------------------------ */

/* trace + raytrace_impl — rt/renderer.d:325-376 (primary rays have depth 0) */
template <int LEVELS, bool MLC, int PO>
DEV F3 raytrace(const RenderParams &P, const Ctx &cx, D3 o, D3 raw, Counters &cnt, c2rt_trace_result *probe)
{
    cnt.primary += 1;
    const uint32_t nn = P.n_nodes;
    uint32_t n = next_node(cx.primary_mask, 0);
    /* planes-only scenes: every lane's ray provably leaves the leading planes behind (sky tiles);
     * `raw` is the screen ray before normalisation (rt/camera.d:144-147) */
    if constexpr (PO & kSpecPlanes) {
        if (!probe) {
            while (n < nn && __all(plane_points_away(cx.nodes + n, o, raw))) n = next_node(cx.primary_mask, n + 1);
            if (n >= nn) return mkf(0, 0, 0); /* Environment.getEnvironment — rt/environment.d:7-10 */
        }
    }
    const D3 d = normalized(cx.bad, raw);
    Hit best;
    best.dist = 1e99;
    best.g = -1;
    best.code = 0;
    Surf surf;
    if (probe) { /* the probe reports the record even without a hit; a frame only reads it after one */
        surf.p = surf.n = mk(0, 0, 0);
        surf.u = surf.v = 0;
    }
    int closest = -1;
    Mat mat;
    if (!probe && cx.primary_ground_only) { /* wave-uniform */
        /* Ground tile (most of a frame that looks at a floor): the node loop collapses to Node.intersect +
         * Plane.intersect on ONE node known to be a Plane under the identity matrix with zero offset
         * (RenderParams::ground_node) — the same operations on the same operands as the general path
         * (node_intersect, plane_intersect), minus the loop, the flag tests, the per-lane record merge and
         * the per-lane shading-input fetch: the node is the same for every lane, so its DevMat stays in
         * scalar registers. */
        NodeP N = cx.nodes + P.ground_node;
        double len, inv;                                 /* make_ray: |d|, d * (1/|d|) */
        len_inv_unit(cx.bad, sqmag(d), len, inv);
        const D3 dn = mk(d.x * inv, d.y * inv, d.z * inv);
        const double y = N->g.p[0], limit = N->g.p[1];
        const bool away = ((o.y > y) & (dn.y > -1e-9)) | ((o.y < y) & (dn.y < 1e-9));
        /* (a lane whose -dn.y is not den_ok is `away`, or has o.y == y: a zero numerator sends the wave
         * to the compiler's division) */
        double rden = 0;
        if constexpr (kLean) rden = rcp_refined(-dn.y);
        const double mult = div_r(cx.bad, o.y - y, -dn.y, rden);
        const D3 p = o + dn * mult;
        const bool miss = away | (mult > 1e99 * len) | (fabs(p.x) > limit) | (fabs(p.z) > limit);
        if (!miss) {
            closest = P.ground_node;
            surf.p = p;
            surf.n = mk(0, 1, 0);
            surf.u = p.x;
            surf.v = p.z;
        }
        load_mat(N, mat);
    } else {
        C2RT_REGION_BEGIN(cx, kRegTrace)
        const RayW ray = make_ray(cx.bad, o, d);
        for (uint32_t nx; n < nn; n = nx) { /* scalar loop, file order */
            nx = next_node(cx.primary_mask, n + 1);
            if (node_intersect<LEVELS, kFull, PO>(cx, cx.nodes + n, ray, best, nx >= nn && !probe)) closest = (int)n;
        }
        C2RT_REGION_END(cx, kRegTrace)
        C2RT_REGION_BEGIN(cx, kRegSurface)
        /* One pass per DISTINCT closest node of the wave (usually one or two): its shading inputs through
         * scalar loads instead of a node -> shader -> texture chain of per-lane loads, and the closest
         * hit's normal, u,v and world-space point (hit_surface).  (Lanes without a hit keep indeterminate
         * records: they return the environment colour before anything reads them.) */
        mat.tex_type = -1;
        bool todo = closest >= 0;
        while (todo) {
            const int cn = __builtin_amdgcn_readfirstlane(closest);
            if (closest == cn) {
                NodeP N = cx.nodes + cn;
                load_mat(N, mat);
                /* (a bitmap texture reads u,v as floats only: the certain-float route, unless the probe reports them) */
                const UVWant want = (!probe && mat.tex_type == C2RT_TEX_BITMAP) ? UVWant{kUVBitmap, (double)__uint_as_float(mat.td[2])}
                                                                                : uv_want(probe || mat.tex_type >= 0);
                hit_surface<PO>(cx, N, best, want, surf);
                todo = false;
            }
        }
        C2RT_REGION_END(cx, kRegSurface)
    }
    if (probe) {
        probe->closest_node = closest;
        probe->leaf_geom = closest >= 0 ? best.g : -1;
        probe->p[0] = surf.p.x; probe->p[1] = surf.p.y; probe->p[2] = surf.p.z;
        probe->normal[0] = surf.n.x; probe->normal[1] = surf.n.y; probe->normal[2] = surf.n.z;
        probe->dist = best.dist; probe->u = surf.u; probe->v = surf.v;
        probe->ray_orig[0] = o.x; probe->ray_orig[1] = o.y; probe->ray_orig[2] = o.z;
        probe->ray_dir[0] = d.x; probe->ray_dir[1] = d.y; probe->ray_dir[2] = d.z;
    }
#if C2RT_TILE_STATS
    {
        C2RT_REGION_BEGIN(cx, kRegShade)
        F3 col_ = mkf(0, 0, 0);
#if C2RT_CSG_CERTAIN
        if (closest >= 0) col_ = shade<LEVELS, MLC, PO>(P, cx, mat, d, surf, cnt.shadow, closest);
#else
        if (closest >= 0) col_ = shade<LEVELS, MLC, PO>(P, cx, mat, d, surf, cnt.shadow);
#endif
        C2RT_REGION_END(cx, kRegShade)
        return col_;
    }
#endif
    if (closest < 0) return mkf(0, 0, 0); /* Environment.getEnvironment — rt/environment.d:7-10 */
#if C2RT_CSG_CERTAIN
    return shade<LEVELS, MLC, PO>(P, cx, mat, d, surf, cnt.shadow, closest);
#else
    return shade<LEVELS, MLC, PO>(P, cx, mat, d, surf, cnt.shadow);
#endif
}

/* The first half of `trace` (rt/renderer.d:325-338) for a CALLER's ray (c2rt_trace_rays; c2rt_rays.hip,
 * trace_rays_kernel): data.dist = 1e99, every node in file order, the last one that returns true is the closest.
 * Unlike raytrace() above, whose argument is the camera's un-normalised screen ray, the direction is used exactly
 * as given — the reference's trace() does not normalise either (Camera.getScreenRay has, by then), and Node.intersect
 * (rt/node.d:34-36) takes the magnitude of whatever it is handed: make_ray's sqrt and reciprocal are that magnitude
 * and the factor of that normalize() for any length in exact::, which is the only namespace this is instantiated
 * in (len_inv_unit's lean shortcut presumes a unit vector).  No culling mask, no ground-tile shortcut, no
 * plane_points_away: caller rays share no eye, so every node is tested.
 * record (wave-uniform): the caller reads best.dist, so the last node's division is not skipped, and the surface
 * carries u, v for untextured nodes too.  Returns the closest node or -1; without a hit `surf` is all zeros and
 * best.dist is 1e99 — the record the probe reports. */
template <int LEVELS>
DEV int trace_closest(const Ctx &cx, D3 o, D3 d, bool record, Hit &best, Surf &surf, Mat &mat)
{
    const uint32_t nn = cx.n_nodes;
    best.dist = 1e99;
    best.g = -1;
    best.code = 0;
    best.p = mk(0, 0, 0);
    surf.p = surf.n = mk(0, 0, 0);
    surf.u = surf.v = 0;
    int closest = -1;
    const RayW ray = make_ray(cx.bad, o, d);
    for (uint32_t n = 0; n < nn; ++n) /* scalar loop, file order */
        if (node_intersect<LEVELS, kFull, 0>(cx, cx.nodes + n, ray, best, n + 1 >= nn && !record)) closest = (int)n;
    /* one pass per distinct closest node of the wave, as in raytrace() */
    mat.tex_type = -1;
    bool todo = closest >= 0;
    while (todo) {
        const int cn = __builtin_amdgcn_readfirstlane(closest);
        if (closest == cn) {
            NodeP N = cx.nodes + cn;
            load_mat(N, mat);
            hit_surface<0>(cx, N, best, uv_want(record || mat.tex_type >= 0), surf);
            todo = false;
        }
    }
    return closest;
}

/* renderSample — rt/renderer.d:254-313 */
template <int LEVELS, int DOF, bool MLC, int PO>
DEV F3 render_sample(const RenderParams &P, const Ctx &cx, double x, double y, int dx, int dy, uint64_t pixel, uint32_t tap,
                     Counters &cnt, c2rt_trace_result *probe)
{
    Rng rng = {DOF ? rng_key(P.seed, pixel, tap) : 0u, 0, 0};
    D3 o, d;
    if constexpr (!DOF) {
        screen_ray<false>(cx.bad, P, x, y, 0, rng, o, d);
        return raytrace<LEVELS, MLC, PO>(P, cx, o, d, cnt, probe);
    } else {
        /* renderSampleDof / renderSampleStereo / renderSampleDefault (rt/renderer.d:270-313)
         * as ONE loop around ONE trace call site (five inlined copies of the tracer made
         * this instance five times the size of the others): lens samples x eyes, in the
         * reference's order, with the random draws in its order. */
        /* DOF = 1: depth of field on a mono camera (what zaphod.sdl asks for): one eye, no offset, no
         * anaglyph merge — all of it compile-time; DOF = 2: a stereo camera, with or without depth of field */
        const bool stereo = DOF == 2 && P.cam.stereo_separation != 0;
        const bool dof = P.cam.dof != 0;
        const uint32_t ns = dof ? P.cam.num_samples : 1u;
        const int eyes = stereo ? 2 : 1;
        F3 average = mkf(0, 0, 0), sample = mkf(0, 0, 0);
        for (uint32_t i = 0; i < ns; ++i) {
            rng.sample = i;
            rng.dim = 0;
            /* as in render_tile's tap loop: what a lens sample reads of the kernel arguments is loaded inside
             * the sample, not ahead of the loop (reading `P` itself was a build switch up to commit f0eed4f) */
            KArgs Ks = cx.kargs;
            asm volatile("" : "+s"(Ks));
            const RenderParams &Ps = *(const RenderParams *)Ks;
            for (int e = 0; e < eyes; ++e) {
                double sx = x, sy = y;
                if (dof) {
                    const double jx = rng_next(rng), jy = rng_next(rng);
                    sx = x + jx * dx;
                    sy = y + jy * dy;
                }
                screen_ray<DOF>(cx.bad, Ps, sx, sy, stereo ? (e == 0 ? -1 : +1) : 0, rng, o, d);
                const F3 c = raytrace<LEVELS, MLC, PO>(Ps, cx, o, d, cnt, e == 0 ? probe : nullptr);
                sample = e == 0 ? c : combine_stereo(sample, c);
            }
            if (!dof) return sample;
            average = average + sample;
        }
        return average / (float)ns;
    }
}

/* AA kernel — rt/renderer.d:235-242 */
__constant__ double k_aa_x[5] = {0.0, 0.3, 0.6, 0.0, 0.6};
__constant__ double k_aa_y[5] = {0.0, 0.3, 0.0, 0.6, 0.6};

/* ------------------------------------------------------------------ */
/* ground-only tiles: a straight-line path of their own (lean:: only)     */
/* ------------------------------------------------------------------ */
/*
 * A tile whose primary rays AND shadow rays towards the one light can reach the ground plane only (bit 1 of the
 * mask table's third word), in a frame the host found eligible (RenderParams::ground_fast: Lambert over a bitmap, a
 * checker or a plain colour, at most one light), rendered whole — tap loop, samples, store — by code that knows all of
 * that.  It performs the IEEE operations of the general path for such a tile, on the same operands, in the same
 * order: screen_ray, normalized, the ground branch of raytrace(), the texture, shade() / light_terms for the one
 * light, the ground_only pre-check of test_visibility, the tap accumulation, the store; and every oob_note of that
 * path, so that a lane outside a lean window sends the tile to exact:: as before.  What it does not carry: a Hit, a
 * Surf, `closest`, the node loop, the surface pass, CSG, LDS, the Phong and Procedure2 code and their libm calls.
 * Nothing joins a general path behind the trace, so the ground node's material, its texture descriptor and the light
 * are wave-uniform values in scalar registers — read once per sample through the re-read kernel-argument pointer,
 * as render_tile's tap loop does —, texture type and light are scalar branches and the texel addresses are built
 * from a scalar width, height and offset.
 *
 * Three folds through the known normal n = (0, 1, 0).  Each holds for every lane whose operands passed the lean
 * windows (any other lane voids the tile; none of this can fault):
 *   d  (the normalised screen ray) and lightDir are FINITE: sqmag(raw) and |lightPos - p|^2 are noted by
 *     normalized() / len_inv and lie in [2^-240, 2^240), so the components are finite and so is the reciprocal length.
 *   dot(d, n) < 0  <=>  d.y < 0:  dot = (d.x * 0 + d.y * 1) + d.z * 0; the outer products are zeros of some sign,
 *     d.y * 1 is d.y, and x + (+-0) is x for x != 0.  For d.y == +-0 the sum is a zero and both sides are false.
 *   N * 1e-6 = (+-0, +-1e-6, +-0):  1 * 1e-6 and -1 * 1e-6 are exact.  `from` enters the pre-check only: from.y as
 *     computed there; from.x, from.z through |lightPos.x - (p.x + (+-0))| < 1e150, and p.x + (+-0) differs from p.x
 *     at most in the sign of a zero, which changes lightPos.x - from.x at most in the sign of a zero: |lv.x| decides.
 *   cosTheta = dot(lightDir, N) is read as `cosTheta > 0` and, when that holds, (float)cosTheta:
 *     dot = (lightDir.x * (+-0) + lightDir.y * (+-1)) + lightDir.z * (+-0) = +-lightDir.y when that is not zero, and
 *     a zero of some sign (not > 0, never converted) when it is.  lightDir.x and lightDir.z are not needed at all.
 *
 * Bail-out: when the pre-check fails for a sample (`__all` over the lanes that hit the plane: the light on the far
 * side of the floor from the eye, a lane with raw.y out of range) the function returns kGroundBail before anything
 * is written and the same wave renders the tile through the code below, as if the path did not exist.
 * Returns per lane; the lanes inside the frame agree (a lane outside it reports kGroundDone: it has nothing to do).
 */
/* dark (wave-uniform, a scalar branch per sample): the tile's third mask word has bit 2 — every shadow ray of the tile
 * towards the one light is provably occluded (csg_void.h, "Dark ground tiles"), so test_visibility is false for every
 * sample, shade() adds avgColor = (0, 0, 0) to the ambient term and nothing else of the light reaches the pixel.  The
 * sample is then ray, normalisation, plane hit, texture and diffuse * (ambient + (0, 0, 0)) — the addition stays, an
 * ambient of -0 becomes +0 as it does in shade() —: no light_terms, no base_light, no pre-check, no bail-out.  The
 * oob_notes of the skipped light arithmetic go with it.  That is sound: a lane outside a lean window only ever sent the
 * tile to exact::, which computes the same bits as lean:: inside the windows, and the values those windows guard are
 * never read here. */
template <int PO>
DEV int ground_tile(const RenderParams &P, KArgs K, const uint32_t trow, const uint32_t bcol, const bool dark)
{
    static_assert(!(PO & kSpecPlanes), "the planes-only instances have no mask table");
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const uint32_t tcol = bcol * kWavesPerBlock + wave; /* (trow, bcol: the tile, trow < P.tiles_y — render_tile) */
    const uint32_t x = tcol * kTileW + (lane % kTileW);
    const uint32_t lr0 = trow * kTileH + (lane / kTileW);
    if (x >= P.width || lr0 >= P.local_rows) return kGroundDone;
    const uint32_t lr = lr0 + P.row_offset;
    const uint32_t y = frame_row(P, lr);
    const uint32_t ntaps = P.taps;

    Oob bad;
    oob_init(bad);
    F3 accum = mkf(0, 0, 0);
#pragma unroll 1
    for (uint32_t s = 0; s < ntaps; ++s) {
        KArgs Kt = K;
        asm volatile("" : "+s"(Kt));
        const RenderParams &Pt = *(const RenderParams *)Kt;
        Rng rng = {0u, 0, 0};
        D3 o, raw;
        screen_ray<0>(bad, Pt, (double)x + k_aa_x[s], (double)y + k_aa_y[s], 0, rng, o, raw);
        const D3 d = normalized(bad, raw);
        /* Node.intersect + Plane.intersect on the ground node: raytrace()'s ground branch */
        NodeP N = (NodeP)Pt.nodes + Pt.ground_node;
        double len, inv;
        len_inv_unit(bad, sqmag(d), len, inv);
        const D3 dn = mk(d.x * inv, d.y * inv, d.z * inv);
        const double gy = N->g.p[0], limit = N->g.p[1];
        const bool away = ((o.y > gy) & (dn.y > -1e-9)) | ((o.y < gy) & (dn.y < 1e-9));
        const double rden = rcp_refined(-dn.y);
        const double mult = div_r(bad, o.y - gy, -dn.y, rden);
        const D3 p = o + dn * mult;
        const bool miss = away | (mult > 1e99 * len) | (fabs(p.x) > limit) | (fabs(p.z) > limit);
        F3 c = mkf(0, 0, 0); /* Environment.getEnvironment — rt/environment.d:7-10 */
        bool bail = false;
        if (!miss) {
            /* shade(): Lambert, u = p.x, v = p.z, N = faceforward((0, 1, 0)) */
            Mat mat;
            load_mat(N, mat);
            const F3 diffuse = mat.tex_type == C2RT_TEX_CHECKER ? checker_color(mat, p.x, p.z)
                             : (mat.tex_type >= 0 ? bitmap_color(Pt, mat, p.x, p.z) : mat.color);
            F3 lightContrib = mkf(Pt.ambient[0], Pt.ambient[1], Pt.ambient[2]);
            if (dark) { /* wave-uniform */
                lightContrib = lightContrib + mkf(0, 0, 0);
            } else if (Pt.n_lights) {
                LightP L = (LightP)Pt.lights;
                F3 avgColor = mkf(0, 0, 0);
                if (L->lit & 1u) {
                    const bool up = d.y < 0; /* N = (0, 1, 0); otherwise (-0, -1, -0) */
                    const D3 lightPos = ld3(L->pos);
                    const double from_y = p.y + (up ? 1e-6 : -1e-6);
                    /* light_terms */
                    const D3 lv = lightPos - p;
                    const double r2 = sqmag(lv);
                    double rlen, rinv;
                    len_inv(bad, r2, rlen, rinv);
                    const double ldy = lv.y * rinv;
                    const double cosTheta = up ? ldy : -ldy;
                    const F3 baseLight = base_light(bad, L, r2);
                    /* test_visibility's ground_only pre-check: plane_points_away for the ground plane */
                    const double raw_y = lightPos.y - from_y, ground_y = Pt.ground_y;
                    const bool sane = (fabs(lv.x) < 1e150) & (fabs(lv.z) < 1e150);
                    const bool rises = (raw_y > 1e-150) & (raw_y < 1e150), falls = (raw_y < -1e-150) & (raw_y > -1e150);
                    bail = !__all(sane & (((from_y > ground_y) & rises) | ((from_y < ground_y) & falls)));
                    if (cosTheta > 0) avgColor = avgColor + baseLight * (float)cosTheta;
                }
                lightContrib = lightContrib + avgColor;
            }
            c = diffuse * lightContrib;
        }
        if (__ballot(bail)) return kGroundBail;
        accum = s == 0 ? c : accum + c;
    }
    if (ntaps > 1) accum = accum / (float)ntaps;
    if (__ballot(oob_any(bad))) return kGroundRedo;
    store_pixel(P, (size_t)(P.frame_rows ? y : lr) * P.width + x, accum);
    return kGroundDone;
}

/*
 * The same tile through the short chain of ground_certain.h, in a frame the host found inside that header's domain
 * (RenderParams::ground_certain_cq: eye and light above the floor, a bitmap or a plain colour, magnitudes in range — so
 * the shadow pre-check holds for the whole frame and d.y < 0 on every lane that hits).  Per sample: the parent's
 * screen ray and its subtraction o.y - gy, bit for bit; one reciprocal, one product and two fma for the hit point; then
 * every float and decision the pixel reads — hit / away / beyond limit, the two texture coordinates, (float)r2,
 * (float)cosTheta — taken from a proven interval around the reference's double, and `unsure` raised where the
 * interval does not decide it.  From those floats on it is ground_tile's arithmetic — the same IEEE operations on the
 * same operands, in the parent's order — in forms of its own where the route knows more: bitmap_filtered_uniform for
 * bitmap_filtered (a wave-uniform bitmap within 32-bit addressing), one light quotient for base_light's three where the
 * channels are the same bits (DevLight::equal), tap_average for the division by the tap count (c2rt_trace_shared.inc).
 * One ballot at the end: a tile with an unsure lane (or one outside a
 * lean window) writes nothing, counts itself (c2rt_get_ground_bails) and returns kGroundBail — the same wave then
 * runs ground_tile as if this function did not exist.
 */
template <int PO>
DEV int ground_tile_certain(const RenderParams &P, KArgs K, const uint32_t trow, const uint32_t bcol, const bool dark)
{
    static_assert(!(PO & kSpecPlanes), "the planes-only instances have no mask table");
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const uint32_t tcol = bcol * kWavesPerBlock + wave;
    const uint32_t x = tcol * kTileW + (lane % kTileW);
    const uint32_t lr0 = trow * kTileH + (lane / kTileW);
    if (x >= P.width || lr0 >= P.local_rows) return kGroundDone;
    const uint32_t lr = lr0 + P.row_offset;
    const uint32_t y = frame_row(P, lr);
    const uint32_t ntaps = P.taps;

    Oob bad;
    oob_init(bad);
    bool unsure = false;
    F3 accum = mkf(0, 0, 0);
#pragma unroll 1
    for (uint32_t s = 0; s < ntaps; ++s) {
        KArgs Kt = K;
        asm volatile("" : "+s"(Kt));
        const RenderParams &Pt = *(const RenderParams *)Kt;
        Rng rng = {0u, 0, 0};
        D3 o, raw;
        screen_ray<0>(bad, Pt, (double)x + k_aa_x[s], (double)y + k_aa_y[s], 0, rng, o, raw);
        NodeP N = (NodeP)Pt.nodes + Pt.ground_node;
        const double gy = N->g.p[0], limit = N->g.p[1];
        double px, pz, bx, bz, q;
        const int state = gc_hit(o.x, o.z, o.y - gy, raw.x, raw.y, raw.z, (double)Pt.ground_certain_cq, limit, &px, &pz, &bx, &bz, &q);
        bool u = state == GC_UNSURE;
        F3 c = mkf(0, 0, 0); /* Environment.getEnvironment — rt/environment.d:7-10 */
        if (state == GC_HIT) {
            Mat mat;
            load_mat(N, mat);
            F3 diffuse = mat.color;
            if (mat.tex_type >= 0) { /* wave-uniform: a bitmap (the host leaves checker floors to ground_tile) */
                const double sc = (double)__uint_as_float(mat.td[2]);
                float fu, fv;
                u |= !gc_tex_float(px, bx, sc, &fu);
                u |= !gc_tex_float(pz, bz, sc, &fv);
                /* bitmap_color from its two floats on */
                const uint32_t w = mat.td[0], hgt = mat.td[1];
                /* (the host keeps a bitmap beyond 2^28 texels of the pool on ground_tile: td[5] is 0 here) */
                diffuse = bitmap_filtered_uniform(Pt.texels, mat.td[4], w, hgt, fu * (float)w, fv * (float)hgt);
            }
            F3 lightContrib = mkf(Pt.ambient[0], Pt.ambient[1], Pt.ambient[2]);
            if (dark) { /* wave-uniform */
                lightContrib = lightContrib + mkf(0, 0, 0);
            } else if (Pt.n_lights) {
                LightP L = (LightP)Pt.lights;
                F3 avgColor = mkf(0, 0, 0);
                if (L->lit & 1u) {
                    const gc_frame f = gc_frame_of(0.0, 1, L->pos[1], gy);
                    float r2f, cosf;
                    double unread[4];
                    u |= !gc_light(px, pz, q, L->pos[0], L->pos[2], &f, &r2f, &cosf, unread);
                    /* (cosTheta > 0 on every lane: the light is above the floor) */
                    if (L->equal) { /* wave-uniform: three equal channels — base_light's quotient, bit for bit, its
                                        * product with cosTheta and its sum with avgColor's +0 once for all three */
                        oob_note_f32(bad, r2f);
                        const float b = div_with_f32(L->color[0], r2f, rcp_refined_f32(r2f));
                        const float a = 0.0f + b * cosf;
                        avgColor = mkf(a, a, a);
                    } else {
                        avgColor = avgColor + base_light(bad, L, (double)r2f) * cosf;
                    }
                }
                lightContrib = lightContrib + avgColor;
            }
            c = diffuse * lightContrib;
        }
        unsure |= u;
        accum = s == 0 ? c : accum + c;
    }
    if (ntaps > 1) tap_average(bad, accum, (float)ntaps);
    if (__ballot(unsure | oob_any(bad))) {
        if (lane == (int)__builtin_ctzll(__ballot(true))) atomicAdd(P.redo_counter + 1, 1ull); /* c2rt_get_ground_bails */
        return kGroundBail;
    }
    store_pixel(P, (size_t)(P.frame_rows ? y : lr) * P.width + x, accum);
    return kGroundDone;
}

/* ------------------------------------------------------------------ */
/* sphere-interior tiles: a straight-line path of their own (lean:: only) */
/* ------------------------------------------------------------------ */
/*
 * A tile of which the mask pre-pass has proven (bit 3 of the mask table's third word; csg_void.h, "Sphere-interior
 * tiles") that every primary ray gets its closest hit on ONE Sphere node under the identity matrix — `node`, the one bit
 * of the primary mask beside the ground's — and that no other node can occlude its shadow rays towards the one light,
 * in a frame and on a node the host found eligible (SphereCull::interior: Lambert or Phong over a plain colour or a
 * bitmap).  Rendered whole — tap loop, samples, store — by code that knows all of that.  It performs the IEEE operations
 * of the general path for such a tile, on the same operands, in the same order: screen_ray, normalized, make_ray,
 * node_intersect's offset subtraction and sphere_intersect<kFull> (against the limit of a ray that has hit nothing: the
 * proof says the ground is farther), the sphere branch of leaf_surface and hit_surface, faceforward, the bitmap's
 * u,v (c2_sphere_uv_bitmap) and texel blend (bitmap_color's arithmetic in front of bitmap_filtered_uniform, which is
 * bitmap_filtered bit for bit), light_terms, test_visibility's arithmetic for that ONE node (len_inv, make_ray, the
 * offset, sphere_intersect<kBool> against the light's distance), the Lambert and Phong terms of shade(), the tap sum,
 * its division by the tap count and the store; and the oob_notes of all of
 * it, so that a lane outside a lean window sends the tile to exact:: as before.  What it does not carry: the node loop
 * with its per-lane best-hit merge, `closest`, the pass over distinct closest nodes, a Mat in vector registers, the
 * ground plane's test, CSG, LDS.  Material, texture descriptor, sphere record and light are wave-uniform: read per
 * sample through the re-read kernel-argument pointer into scalar registers; shader and texture kind are scalar branches.
 *
 * If any lane's sphere test misses, the proof was wrong: the wave writes nothing, counts the tile (redo_counter[2],
 * c2rt_get_sphere_bails) and returns kGroundBail; the general path below then renders it as if this function did not
 * exist.  Returns per lane, like ground_tile. */
template <int PO>
DEV int sphere_tile(const RenderParams &P, KArgs K, const uint32_t trow, const uint32_t bcol, const uint32_t node)
{
    static_assert(!(PO & kSpecPlanes), "the planes-only instances have no mask table");
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const uint32_t tcol = bcol * kWavesPerBlock + wave;
    const uint32_t x = tcol * kTileW + (lane % kTileW);
    const uint32_t lr0 = trow * kTileH + (lane / kTileW);
    if (x >= P.width || lr0 >= P.local_rows) return kGroundDone;
    const uint32_t lr = lr0 + P.row_offset;
    const uint32_t y = frame_row(P, lr);
    const uint32_t ntaps = P.taps;

    Oob bad;
    oob_init(bad);
    bool missed = false;
    F3 accum = mkf(0, 0, 0);
#pragma unroll 1
    for (uint32_t s = 0; s < ntaps; ++s) {
        KArgs Kt = K;
        asm volatile("" : "+s"(Kt));
        const RenderParams &Pt = *(const RenderParams *)Kt;
        Rng rng = {0u, 0, 0};
        D3 o, raw;
        screen_ray<0>(bad, Pt, (double)x + k_aa_x[s], (double)y + k_aa_y[s], 0, rng, o, raw);
        const D3 d = normalized(bad, raw);
        NodeP N = (NodeP)Pt.nodes + node;
        GeomP G = &N->g;
        const bool has_off = !(N->flags & kNodeZeroOffset); /* wave-uniform */
        /* raytrace(): make_ray, then Node.intersect + Sphere.intersect on the one node */
        const RayW ray = make_ray(bad, o, d);
        Hit h;
        {
            ORay rc;
            rc.o = ray.o;
            if (has_off) rc.o = rc.o - ld3(N->off);
            rc.d = ray.dn;
            rc.A = ray.A;
            prep_dir(rc, kPrepA);
            h.dist = 1e99 * ray.len;
            h.p = ray.o; /* (a lane that misses — never, by the proof — reads a defined point below) */
            missed |= !sphere_intersect<kFull>(bad, G, N->geom, rc, h, false);
        }
        /* hit_surface: the sphere branch of leaf_surface, the identity-matrix normal, the offset */
        Mat mat;
        load_mat(N, mat);
        const D3 pc = h.p - ld3(G->p);
        D3 n = normalized(bad, pc);
        F3 diffuse = mat.color;
        if (mat.tex_type >= 0) { /* wave-uniform: a bitmap (the host leaves every other texture to the general path) */
            double u, v;
            const double sc = (double)__uint_as_float(mat.td[2]);
            sphere_uv(pc.x, pc.z, pc.y / G->p[3], UVWant{kUVBitmap, sc}, u, v);
            /* bitmap_color, its texels through the uniform fetch (td[5] is 0 here: the host's limit) */
            u *= sc;
            v *= sc;
            u = u - floor(u);
            v = v - floor(v);
            const uint32_t w = mat.td[0], hgt = mat.td[1];
            diffuse = bitmap_filtered_uniform(Pt.texels, mat.td[4], w, hgt, (float)u * (float)w, (float)v * (float)hgt);
        }
        {
            double len, inv;
            len_inv_unit(bad, sqmag(n), len, inv);
            n = n * inv;
        }
        D3 p = h.p;
        if (has_off) p = p + ld3(N->off);
        /* shade() */
        const bool phong = mat.shader_type == C2RT_SHADER_PHONG; /* wave-uniform */
        const D3 Nf = dot(d, n) < 0 ? n : -n; /* faceforward */
        F3 lightContrib = mkf(Pt.ambient[0], Pt.ambient[1], Pt.ambient[2]);
        F3 specular = mkf(0, 0, 0);
        if (Pt.n_lights) {
            LightP L = (LightP)Pt.lights;
            F3 avgColor = mkf(0, 0, 0), avgSpecular = mkf(0, 0, 0);
            if (L->lit & 1u) {
                const D3 lightPos = ld3(L->pos);
                const D3 from = p + Nf * 1e-6;
                double cosTheta, cosGamma;
                F3 baseLight;
                light_terms(bad, L, lightPos, p, Nf, d, phong, cosTheta, baseLight, cosGamma);
                /* test_visibility for the one node that can occlude: the sphere itself */
                const D3 sraw = lightPos - from;
                double rlen, rinv;
                len_inv(bad, sqmag(sraw), rlen, rinv);
                const RayW sray = make_ray(bad, from, mk(sraw.x * rinv, sraw.y * rinv, sraw.z * rinv));
                ORay rc;
                rc.o = sray.o;
                if (has_off) rc.o = rc.o - ld3(N->off);
                rc.d = sray.dn;
                rc.A = sray.A;
                prep_dir(rc, kPrepA);
                Hit t;
                t.dist = rlen * sray.len;
                const bool visible = !sphere_intersect<kBool>(bad, G, N->geom, rc, t, false);
                if (visible) {
                    if (cosTheta > 0) avgColor = avgColor + baseLight * (float)cosTheta;
                    if (phong & (cosGamma > 0))
                        avgSpecular = avgSpecular + baseLight * c2_pow_f32(cosGamma, mat.exponent) * mat.strength;
                }
            }
            lightContrib = lightContrib + avgColor;
            specular = specular + avgSpecular;
        }
        const F3 res = diffuse * lightContrib;
        const F3 c = phong ? res + specular : res;
        accum = s == 0 ? c : accum + c;
    }
    /* `accum / 5` as render_tile has it, not tap_average: a Phong lobe's far tail (cos^80) leaves channels far below that
     * routine's window, and every such tile would be rendered again */
    if (ntaps > 1) accum = accum / (float)ntaps;
    if (__ballot(missed)) {
        if (lane == (int)__builtin_ctzll(__ballot(true))) atomicAdd(P.redo_counter + 2, 1ull); /* c2rt_get_sphere_bails */
        return kGroundBail;
    }
    if (__ballot(oob_any(bad))) return kGroundRedo;
    store_pixel(P, (size_t)(P.frame_rows ? y : lr) * P.width + x, accum);
    return kGroundDone;
}

#if C2RT_CSG_TILE /* the frame units only (c2rt_trace_common.inc) */
/* ------------------------------------------------------------------ */
/* ground + one leaf CsgOp: a straight-line path of their own (lean:: only) */
/* ------------------------------------------------------------------ */
/*
 * A tile whose live primary mask is exactly {ground node, `node`} and whose live shadow mask towards the one light
 * (`smask`) is a subset of that pair, in a ground_fast frame, where the host marked `node` kNodeCsgTile: a leaf CsgOp
 * that csg_certain.h accepts, under the identity matrix, Lambert or Phong over a plain colour (scene_plan.cpp:
 * plan_csg_tile_nodes).  The condition is read from the two mask words render_tile loads anyway; the pre-pass knows
 * nothing of this path.  Rendered whole — tap loop, samples, store — with the IEEE operations the general path performs
 * for such a tile, on the same operands: screen_ray, normalized, make_ray; the two nodes in FILE order, the running
 * best.dist handed from the first to the second (so the later node wins a tie) and its division skipped behind the
 * second (node_intersect's `last`); the ground through the operations of raytrace()'s ground branch against that limit,
 * the CsgOp through node_intersect<1, kFull> itself; the cube and sphere branches of leaf_surface and hit_surface for
 * the lanes on the CsgOp, (0, 1, 0) and u = p.x, v = p.z for the lanes on the ground; faceforward, light_terms once,
 * with the reflection under the mask of the lanes on a Phong CsgOp; test_visibility's ray, then the nodes `smask`
 * keeps, in file order, a lane leaving at its first occluder — the ground dropped by the wave-uniform test
 * test_visibility has for ground-only tiles (every lane's plane test would return at its first comparison), the CsgOp
 * through node_intersect<1, kBool> with `own` for the lanes that start on it; shade()'s Lambert and Phong terms, the
 * tap sum in the reference's order, `accum / taps`, the store; and the oob_notes of all of it.  One thing it leaves
 * unexecuted: the shadow ray of a lane whose light terms are both off (see `lit_lane` below), whose answer nothing reads.
 *
 * What it does not carry: the loop over a mask, the flag tests and prep_dir selection of the ground node, the pass over
 * distinct closest nodes, the leaf's record and the material read per lane — both children's records and both
 * materials are wave-uniform scalar loads, the lane selects —, a Mat in vector registers (so the floor's texture goes
 * through the uniform fetch, as in ground_tile), u,v of the CsgOp's leaves (the node has no texture).
 *
 * A lane whose CSG hit lists outgrew the wave's stack (Ctx::overflow; never at the capacity a depth-1 launch has) makes
 * the wave write nothing, count the tile (redo_counter[3], c2rt_get_csg_tile_bails) and return kGroundBail: the general
 * path renders it as if this function did not exist.  Returns per lane, like ground_tile.  The lane-statistics build
 * keeps the path and counts the tiles it rendered (redo_counter[4], c2rt_get_csg_tiles).  Not taken for the short
 * chain of ground_certain.h: its texel chain would have to stay live beside the CsgOp's walk, in a kernel that sits at
 * its register budget. */
template <int PO>
DEV int csg_tile(const RenderParams &P, KArgs K, const uint32_t trow, const uint32_t bcol, const uint32_t node, const uint32_t smask)
{
    static_assert(!(PO & kSpecPlanes), "the planes-only instances have no mask table");
    extern __shared__ __align__(16) char lds_all[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const uint32_t tcol = bcol * kWavesPerBlock + wave;
    const uint32_t x = tcol * kTileW + (lane % kTileW);
    const uint32_t lr0 = trow * kTileH + (lane / kTileW);
    if (x >= P.width || lr0 >= P.local_rows) return kGroundDone;
    const uint32_t lr = lr0 + P.row_offset;
    const uint32_t y = frame_row(P, lr);
    const uint32_t ntaps = P.taps;
#if C2RT_TILE_STATS
    const unsigned long long stamp0 = __builtin_amdgcn_s_memtime();
#endif

    Ctx cx;
    query_ctx(cx, P, K, lds_all + (size_t)wave * P.csg_cap * kCsgLdsPerEntry, lane);
    cx.csg_certain = true;
#if C2RT_TILE_STATS
    cx.lane_stats = P.tile_stats ? reinterpret_cast<unsigned long long *>(P.tile_stats + 2 * (size_t)P.tiles_x * P.tiles_y) : nullptr;
#endif
    F3 accum = mkf(0, 0, 0);
#pragma unroll 1
    for (uint32_t s = 0; s < ntaps; ++s) {
        KArgs Kt = K;
        asm volatile("" : "+s"(Kt));
        const RenderParams &Pt = *(const RenderParams *)Kt;
        cx.geoms = (GeomP)Pt.geoms;
        cx.csg_cap = (int)Pt.csg_cap;
        Rng rng = {0u, 0, 0};
        D3 o, raw;
        screen_ray<0>(cx.bad, Pt, (double)x + k_aa_x[s], (double)y + k_aa_y[s], 0, rng, o, raw);
        const D3 d = normalized(cx.bad, raw);
        const uint32_t gnode = (uint32_t)Pt.ground_node;
        NodeP Ng = (NodeP)Pt.nodes + gnode, Nc = (NodeP)Pt.nodes + node;
        const bool ground_first = gnode < node; /* wave-uniform: the scene file's order */
        /* raytrace(): the two nodes in file order */
        const RayW ray = make_ray(cx.bad, o, d);
        Hit best;
        best.dist = 1e99;
        best.g = -1;
        best.code = 0;
        D3 pg = o;
        bool on_g = false, on_c = false;
#pragma unroll 1
        for (int i = 0; i < 2; ++i) {
            const bool last = i == 1;
            if ((i == 0) == ground_first) {
                /* Node.intersect + Plane.intersect on the ground node (identity matrix, zero offset): the operations of
                 * raytrace()'s ground branch, against the limit the node in front of it left */
                const double gy = Ng->g.p[0], limit = Ng->g.p[1];
                const D3 dn = ray.dn;
                const bool away = ((o.y > gy) & (dn.y > -1e-9)) | ((o.y < gy) & (dn.y < 1e-9));
                const double rden = rcp_refined(-dn.y);
                const double mult = div_r(cx.bad, o.y - gy, -dn.y, rden);
                const D3 p = o + dn * mult;
                const bool miss = away | (mult > best.dist * ray.len) | (fabs(p.x) > limit) | (fabs(p.z) > limit);
                if (!miss) {
                    if (!last) best.dist = div_r(cx.bad, mult, ray.len, ray.inv);
                    pg = p;
                    on_g = true;
                    on_c = false;
                }
            } else if (node_intersect<1, kFull, PO>(cx, Nc, ray, best, last)) {
                on_c = true;
                on_g = false;
            }
        }
        F3 c = mkf(0, 0, 0); /* Environment.getEnvironment — rt/environment.d:7-10 */
        if (on_g | on_c) {
            /* hit_surface, with no pass per node: the lanes on the CsgOp take the normal of the child they hit — both
             * children's records are scalar loads —, the lanes on the ground (0, 1, 0) */
            D3 n = mk(0, 1, 0), p = pg;
            if (on_c) {
                GeomP G = &Nc->g;
                const int left = G->left;
                GeomP GL = cx.geoms + left, GR = cx.geoms + G->right;
                const bool is_l = best.g == left;
                const bool sphere = is_l ? GL->type == C2RT_GEOM_SPHERE : GR->type == C2RT_GEOM_SPHERE;
                if (sphere) {
                    const D3 ctr = is_l ? ld3(GL->p) : ld3(GR->p);
                    n = normalized(cx.bad, best.p - ctr);
                    if (best.code & kCodeFlip) n = -n;
                    double len, inv;
                    len_inv_unit(cx.bad, sqmag(n), len, inv);
                    n = n * inv;
                } else {
                    const int axis = best.code & kCodeAxis;
                    const double side = (best.code & kCodeSide) ? 1.0 : -1.0;
                    n = mk(axis == 0 ? side : 0.0, axis == 1 ? side : 0.0, axis == 2 ? side : 0.0);
                    if (best.code & kCodeFlip) n = -n;
                }
                p = best.p;
                if (!(Nc->flags & kNodeZeroOffset)) p = p + ld3(Nc->off);
            }
            /* shade(): the CsgOp's material in scalar registers, the floor's inside its branch */
            MatP Mc = &Nc->mat;
            const bool phong = on_c & (Mc->shader_type == C2RT_SHADER_PHONG); /* (the floor is Lambert: ground_fast) */
            const D3 Nf = dot(d, n) < 0 ? n : -n; /* faceforward */
            F3 diffuse = ldf3(Mc->color);
            if (on_g) {
                Mat mg;
                load_mat(Ng, mg);
                diffuse = mg.tex_type == C2RT_TEX_CHECKER ? checker_color(mg, p.x, p.z)
                        : (mg.tex_type >= 0 ? bitmap_color(Pt, mg, p.x, p.z) : mg.color);
            }
            F3 lightContrib = mkf(Pt.ambient[0], Pt.ambient[1], Pt.ambient[2]);
            F3 specular = mkf(0, 0, 0);
            if (Pt.n_lights) {
                LightP L = (LightP)Pt.lights;
                F3 avgColor = mkf(0, 0, 0), avgSpecular = mkf(0, 0, 0);
                if (L->lit & 1u) {
                    const D3 lightPos = ld3(L->pos);
                    const D3 from = p + Nf * 1e-6;
                    double cosTheta, cosGamma;
                    F3 baseLight;
                    light_terms(cx.bad, L, lightPos, p, Nf, d, phong, cosTheta, baseLight, cosGamma);
                    /* The answer of test_visibility is read by the two additions at the end of this block and by nothing else:
                     * a lane whose surface faces away from the light (cosTheta <= 0, or a NaN) and has no lobe towards the
                     * eye casts no shadow ray — its pixel is the same float either way, and what goes unexecuted is the
                     * most expensive thing such a lane does (a ray that starts on the CsgOp is decided by the literal
                     * lists).  Its oob_notes go with it: a note only ever sends the tile to exact::, which computes the
                     * same bits. */
                    const bool lit_lane = (cosTheta > 0) | (phong & (cosGamma > 0));
                    if (lit_lane) {
                        /* test_visibility over the nodes the shadow mask keeps */
                        const D3 sraw = lightPos - from;
                        bool test_g = (smask >> gnode) & 1u; /* wave-uniform */
                        const bool test_c = (smask >> node) & 1u;
                        if (test_g) {
                            /* every lane above the plane and heading up (or below and heading down): Plane.intersect
                             * returns false at its first comparison for all of them */
                            const double ground_y = Pt.ground_y;
                            const bool sane = (fabs(sraw.x) < 1e150) & (fabs(sraw.z) < 1e150);
                            const bool up = (sraw.y > 1e-150) & (sraw.y < 1e150), down = (sraw.y < -1e-150) & (sraw.y > -1e150);
                            if (__all(sane & (((from.y > ground_y) & up) | ((from.y < ground_y) & down)))) test_g = false;
                        }
                        double rlen, rinv;
                        len_inv(cx.bad, sqmag(sraw), rlen, rinv);
                        const RayW sray = make_ray(cx.bad, from, mk(sraw.x * rinv, sraw.y * rinv, sraw.z * rinv));
                        Hit temp;
                        temp.dist = rlen;
                        bool visible = true;
#pragma unroll 1
                        for (int i = 0; i < 2; ++i) {
                            if ((i == 0) == ground_first) {
                                if (test_g && visible) visible = !node_intersect<1, kBool, PO>(cx, Ng, sray, temp, false, false);
                            } else {
                                if (test_c && visible) visible = !node_intersect<1, kBool, PO>(cx, Nc, sray, temp, false, on_c);
                            }
                        }
                        if (visible) {
                            if (cosTheta > 0) avgColor = avgColor + baseLight * (float)cosTheta;
                            if (phong & (cosGamma > 0))
                                avgSpecular = avgSpecular + baseLight * c2_pow_f32(cosGamma, Mc->exponent) * Mc->strength;
                        }
                    }
                }
                lightContrib = lightContrib + avgColor;
                specular = specular + avgSpecular;
            }
            const F3 res = diffuse * lightContrib;
            c = phong ? res + specular : res;
        }
        accum = s == 0 ? c : accum + c;
    }
    /* `accum / 5` as render_tile has it (not tap_average: a Phong lobe's far tail leaves its window) */
    if (ntaps > 1) accum = accum / (float)ntaps;
    if (__ballot(cx.overflow)) {
        if (lane == (int)__builtin_ctzll(__ballot(true))) atomicAdd(P.redo_counter + 3, 1ull); /* c2rt_get_csg_tile_bails */
        return kGroundBail;
    }
    if (__ballot(oob_any(cx.bad))) return kGroundRedo;
    store_pixel(P, (size_t)(P.frame_rows ? y : lr) * P.width + x, accum);
#if C2RT_TILE_STATS
    if (lane == (int)__builtin_ctzll(__ballot(true))) {
        atomicAdd(P.redo_counter + 4, 1ull); /* c2rt_get_csg_tiles */
        if (P.tile_stats) { /* the stamps render_tile leaves for a tile of the general path */
            const unsigned long long dt = __builtin_amdgcn_s_memtime() - stamp0;
            const uint32_t tile = trow * P.tiles_x + tcol;
            P.tile_stats[2 * tile] = dt > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dt;
            P.tile_stats[2 * tile + 1] = ((1u << P.ground_node) | (1u << node)) << 8;
        }
    }
#endif
    return kGroundDone;
}
#endif /* C2RT_CSG_TILE */

/*
 * Frame kernel: Renderer.renderRT passes 2 and 3b (rt/renderer.d:133-142,
 * 183-186) fused — all taps of a pixel are accumulated in registers in the
 * reference's order and the pixel is written once (12 B of HBM traffic per
 * pixel).  One workgroup = one wavefront = one 8x8 tile.
 */
/* Returns (wave-uniform) true when nothing was written because a lane of lean:: met an operand outside
 * its window: the caller renders the tile again through exact::render_tile, which always returns false. */
template <int LEVELS, int DOF, bool MLC, int PO, bool CNT>
DEV bool render_tile(const RenderParams &P, KArgs K, const uint32_t b)
{
    extern __shared__ __align__(16) char lds_all[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    char *lds = lds_all + (size_t)wave * P.csg_cap * kCsgLdsPerEntry;

    /* XCD-aware block -> tile: blocks b and b+8 share an XCD (round-robin
     * dispatch), so XCD x gets tile rows x, x+8, x+16, ... and walks them
     * left to right.  A block is kWavesPerBlock horizontally adjacent 8x8
     * tiles, one per wavefront. */
    const uint32_t xcd = b & 7u, j = b >> 3;
    /* row groups are walked starting at P.row_group_start (where the boxed nodes begin on screen):
     * the expensive tiles are dispatched first and the launch ends on cheap ones */
    const uint32_t groups = (P.tiles_y + 7u) / 8u;
    uint32_t grp = j / P.blocks_x + P.row_group_start;
    if (grp >= groups) grp -= groups;
    const uint32_t trow = grp * 8u + xcd, bcol = j % P.blocks_x;
    if (trow >= P.tiles_y) return false;
    const uint32_t tcol = bcol * kWavesPerBlock + wave;
#if C2RT_TILE_STATS
    const unsigned long long stamp0 = __builtin_amdgcn_s_memtime();
#endif

    /* Which nodes can this tile's primary rays reach, which can occlude its shadow rays towards the first
     * light, and is the ground plane all that is left?  One scalar load from the table the pre-pass kernel
     * wrote for this frame (tile_mask_entry). */
    uint32_t pmask = 0xFFFFFFFFu, smask0 = 0xFFFFFFFFu, mask_slot = 0;
    bool ground_only = false, primary_ground = false, dark = false, interior = false;
    Oob tile_bad;
    oob_init(tile_bad);
    if constexpr (!DOF) {
        if (P.n_cull) {
            typedef uint32_t __attribute__((ext_vector_type(4))) u4_t;
            mask_slot = (uint32_t)tile_mask_slot(P, trow + (P.row_offset - P.mask_row0) / kTileH, (uint32_t)__builtin_amdgcn_readfirstlane(tcol));
            const u4_t m = ((const u4_t C2RT_K *)P.tile_masks)[mask_slot];
            pmask = m.x;
            smask0 = m.y;
            primary_ground = (m.z & 1u) != 0;
            ground_only = (m.z & 2u) != 0;
            dark = (m.z & 4u) != 0;
            interior = (m.z & 8u) != 0;
        }
    }

    /* Ground-only tile of an eligible frame, or dark tile (bit 2: primary rays reach the ground only and every shadow
     * ray is occluded): ground_tile renders it, unless a sample's shadow pre-check fails (never for a dark tile) — then
     * nothing has been written and the tile goes on below.  The call takes nothing but the kernel-argument pointer and
     * the tile's row and block column, through an empty asm, so that the path shares no value with the code below and
     * nothing of it stays live on its behalf (as render_one does for exact::). */
    if constexpr (kLean && LEVELS <= 1 && !DOF && !MLC && !CNT && !(PO & kSpecPlanes) && !C2RT_TILE_STATS) {
        if (P.ground_fast && (ground_only || dark)) { /* wave-uniform */
            KArgs Kg = K;
            uint32_t trow_g = trow, bcol_g = bcol, dark_g = (uint32_t)__builtin_amdgcn_readfirstlane(dark && !ground_only ? 1 : 0);
            asm volatile("" : "+s"(Kg), "+s"(trow_g), "+s"(bcol_g), "+s"(dark_g));
            /* first the short chain, where the host found the frame inside its domain: it renders the tile, or writes
             * nothing and hands it on (kGroundBail) */
            if (((const RenderParams *)Kg)->ground_certain_cq > 0) { /* wave-uniform */
                const int gc = ground_tile_certain<PO>(*(const RenderParams *)Kg, Kg, trow_g, bcol_g, dark_g != 0);
                if (!__ballot(gc == kGroundBail)) return false;
                asm volatile("" : "+s"(Kg), "+s"(trow_g), "+s"(bcol_g), "+s"(dark_g));
            }
            const int g = ground_tile<PO>(*(const RenderParams *)Kg, Kg, trow_g, bcol_g, dark_g != 0);
            if (!__ballot(g == kGroundBail)) return g == kGroundRedo;
        }
        /* Sphere-interior tile (bit 3: every primary ray's closest hit is on the one Sphere node the primary mask keeps
         * beside the ground, and nothing else can occlude its shadow rays): sphere_tile renders it, or — a lane's sphere
         * test missed, which the proof rules out — writes nothing and the tile goes on below.  The same kind of call. */
        if (__builtin_expect(interior, 0)) { /* wave-uniform; unlikely: the block is laid out behind the general code, where a
                                              * frame that never takes it does not fetch past it */
            uint32_t rest = pmask & (0xFFFFFFFFu >> (32u - P.n_nodes));
            if (P.ground_node >= 0) rest &= ~(1u << P.ground_node);
            KArgs Ks = K;
            uint32_t trow_s = trow, bcol_s = bcol, node_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_ctz(rest | 0x80000000u));
            asm volatile("" : "+s"(Ks), "+s"(trow_s), "+s"(bcol_s), "+s"(node_s));
            const int g = sphere_tile<PO>(*(const RenderParams *)Ks, Ks, trow_s, bcol_s, node_s);
            if (!__ballot(g == kGroundBail)) return g == kGroundRedo;
        }
    }
#if C2RT_CSG_TILE
    /* Tile with the ground and ONE leaf CsgOp node the host marked (kNodeCsgTile) in its primary mask, and nothing beyond
     * those two in its shadow mask: csg_tile renders it, or — a lane's hit lists outgrew the stack — writes nothing and
     * the tile goes on below.  Read from the two words loaded above; the same kind of call as the two before it.  (The
     * lane-statistics build keeps this path: it counts the tiles taken.)  In the identity-matrix instances only, which
     * hold it in 126 VGPRs without scratch: the general depth-1 instance, at 128 VGPRs, went from 48 B to 112 B of scratch
     * with it, so the planner marks no node in a scene that has a matrix (plan_csg_tile_nodes). */
    if constexpr (kLean && LEVELS == 1 && !DOF && !MLC && !CNT && (PO & kSpecIdentity) && !(PO & kSpecPlanes)) {
        if (P.ground_fast && !ground_only && P.n_nodes <= 32u) { /* wave-uniform */
            const uint32_t live = 0xFFFFFFFFu >> (32u - P.n_nodes), gbit = 1u << P.ground_node;
            const uint32_t pm = pmask & live, sm = smask0 & live, rest = pm & ~gbit;
            if (__builtin_expect((pm & gbit) && rest && !(rest & (rest - 1u)) && !(sm & ~pm), 0)) {
                uint32_t node_c = (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_ctz(rest));
                if (((NodeP)P.nodes)[node_c].flags & kNodeCsgTile) {
                    KArgs Kc = K;
                    uint32_t trow_c = trow, bcol_c = bcol, smask_c = (uint32_t)__builtin_amdgcn_readfirstlane((int)sm);
                    asm volatile("" : "+s"(Kc), "+s"(trow_c), "+s"(bcol_c), "+s"(node_c), "+s"(smask_c));
                    const int g = csg_tile<PO>(*(const RenderParams *)Kc, Kc, trow_c, bcol_c, node_c, smask_c);
                    if (!__ballot(g == kGroundBail)) return g == kGroundRedo;
                }
            }
        }
    }
#endif

    /* a scene whose only node is the ground plane (zaphod.sdl, lecture4.sdl): every tile is a ground
     * tile, wherever its rays start (depth of field, stereo) */
    if (P.n_nodes == 1u && P.ground_node == 0) primary_ground = true;

    const uint32_t x = tcol * kTileW + (lane % kTileW);
    const uint32_t lr0 = trow * kTileH + (lane / kTileW); /* row within this launch */
    if (x >= P.width || lr0 >= P.local_rows) return false;
    const uint32_t lr = lr0 + P.row_offset;          /* local row */

    /* local row -> frame row under interleaved strips */
    uint32_t y = lr;
    if (P.strip_world > 1) {
        const uint32_t sh = P.strip_height;
        y = ((lr / sh) * P.strip_world + P.strip_rank) * sh + lr % sh;
    }

    Ctx cx;
    cx.geoms = (GeomP)P.geoms;
    cx.nodes = (NodeP)P.nodes;
    cx.n_nodes = P.n_nodes;
    cx.kargs = K;
    cx.lds = lds;
    cx.lane = lane;
    cx.csg_cap = (int)P.csg_cap;
    cx.overflow = false;
    cx.bad = tile_bad;
    cx.trunc_counter = CNT ? P.ray_counters + 2 : nullptr;
#if C2RT_CSG_CERTAIN
    cx.csg_certain = !CNT;
#endif
#if C2RT_TILE_STATS
    cx.lane_stats = P.tile_stats ? reinterpret_cast<unsigned long long *>(P.tile_stats + 2 * (size_t)P.tiles_x * P.tiles_y) : nullptr;
#endif
    cx.block = b;
    cx.mask_slot = mask_slot;
    cx.primary_mask = pmask;
    cx.shadow_mask0 = smask0;
    cx.shadow_ground_only = ground_only;
    cx.primary_ground_only = primary_ground;
    cx.ground_y = P.ground_y;
    Counters cnt = {0, 0};
    /* prepassOnly (rt/renderer.d:110-130): the pixel shows the sample of the
     * top-left pixel of its 16x16 block inside its bucket */
    uint32_t sx = x, sy = y;
    int jdx = 1, jdy = 1; /* renderPixelNoAA's dx, dy: the extent depth-of-field jitter spans */
    if (P.prepass_bucket) {
        const uint32_t bs = P.prepass_bucket;
        const uint32_t bx = x / bs * bs, by = y / bs * bs;
        sx = bx + ((x - bx) & ~15u);
        sy = by + ((y - by) & ~15u);
        /* the 16x16 block is clipped by its bucket, the bucket by the frame (rt/renderer.d:113-119, 208) */
        const uint32_t bx1 = bx + bs < P.width ? bx + bs : P.width, by1 = by + bs < P.height ? by + bs : P.height;
        jdx = (int)(sx + 16u < bx1 ? 16u : bx1 - sx);
        jdy = (int)(sy + 16u < by1 ? 16u : by1 - sy);
    }
    const uint64_t pixel = (uint64_t)sy * P.width + sx;
    const uint32_t ntaps = P.taps;

    /* renderPixelNoAA — rt/renderer.d:223-228; renderPixelAA — :233-251.
     * Tap 0 has offset (0, 0): x + 0.0 == x, and 0 + c == c for the first
     * sample, so one loop covers both passes. */
    F3 accum = mkf(0, 0, 0);
#pragma unroll 1
    for (uint32_t s = 0; s < ntaps; ++s) {
        /* Every sample reads the kernel arguments through a pointer the optimiser cannot see through: left to
         * itself it loads what a sample needs (camera frame, table pointers, light) once per tile, ahead of
         * this loop, and the values then live in SGPRs across the whole trace — on instances that spill SGPRs
         * to VGPR lanes that is a v_writelane per value and tile and a v_readlane per use.  Loaded where they
         * are used (scalar loads that hit the scalar cache) they die early: render_kernel_idn<1> holds 97
         * spill-lane instructions in its lean half instead of 191; lecture5.sdl 4K x5 0.986 -> 0.944 ms
         * (profiles/r04_variants.md, step 14; reading `P` itself was a build switch up to commit f0eed4f). */
        KArgs Kt = K;
        asm volatile("" : "+s"(Kt));
        const RenderParams &Pt = *(const RenderParams *)Kt;
        /* likewise the table pointers and scalars the tracer keeps in its context — in the instances without
         * nested CsgOps only: lecture5.sdl 1080p +1 %, 4K x5 -0.4 %; csg_stress.sdl (latency-bound, VALU busy
         * 0.64: more scalar loads to wait for) 8.06 -> 8.40 ms with it (step 15) */
        if constexpr (LEVELS <= 1) {
            cx.geoms = (GeomP)Pt.geoms;
            cx.nodes = (NodeP)Pt.nodes;
            cx.n_nodes = Pt.n_nodes;
            cx.kargs = Kt;
            cx.csg_cap = (int)Pt.csg_cap;
            cx.ground_y = Pt.ground_y;
        }
        const F3 c = render_sample<LEVELS, DOF, MLC, PO>(Pt, cx, (double)sx + k_aa_x[s], (double)sy + k_aa_y[s], jdx, jdy, pixel, s, cnt, nullptr);
        accum = s == 0 ? c : accum + c;
    }
    if (ntaps > 1) accum = accum / (float)ntaps; /* `accum / 5`: Color / float */
#if C2RT_TILE_STATS
    if (P.tile_stats && lane == (int)__builtin_ctzll(__ballot(true))) {
        const unsigned long long dt = __builtin_amdgcn_s_memtime() - stamp0;
        const uint32_t tile = trow * P.tiles_x + tcol;
        P.tile_stats[2 * tile] = dt > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dt;
        /* bit 0: primary rays reach the ground only, bit 1: and so do the shadow rays; bits 8..: primary mask */
        P.tile_stats[2 * tile + 1] = (primary_ground ? 1u : 0u) | (ground_only ? 2u : 0u) | (pmask << 8);
    }
#endif

    if constexpr (kLean) {
        if (__ballot(oob_any(cx.bad))) return true;
    }
    if constexpr (LEVELS >= 2) {
        /* some lane's nested hit lists outgrew the stack: nothing of this tile is kept; the
         * full-capacity launch that follows renders the tiles on this list */
        if (__ballot(cx.overflow)) {
            if (lane == (int)__builtin_ctzll(__ballot(true))) {
                const uint32_t slot = atomicAdd(P.retry_list, 1u);
                if (slot < P.retry_max) P.retry_list[1 + slot] = b;
            }
            return false;
        }
    }

    const size_t pixel_index = (size_t)(P.frame_rows ? y : lr) * P.width + x;
    if (P.out_rgb32) { /* wave-uniform */
        /* Color.toRGB32 via convertTo8bit_sRGB_Cached (rt/color.d:154-162,209-214), fused: the display frame
         * needs neither a float frame in HBM nor a second kernel (c2rt_render_frame_rgb32) */
        const float c3[3] = {accum.r, accum.g, accum.b};
        uint32_t ch[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) ch[c] = !(c3[c] > 0) ? 0u : (c3[c] >= 1 ? 255u : (uint32_t)P.srgb_lut[(int)(c3[c] * 4096.0f)]);
        P.out_rgb32[pixel_index] = ch[2] | (ch[1] << 8) | (ch[0] << 16);
    } else {
        /* one 12-byte store per lane (global_store_dwordx3): 8 lanes cover a tile row's 96 contiguous bytes */
        typedef float __attribute__((ext_vector_type(3), aligned(4))) f3_t;
        f3_t v3;
        v3.x = accum.r;
        v3.y = accum.g;
        v3.z = accum.b;
        *reinterpret_cast<f3_t *>(P.out + pixel_index * 3) = v3;
    }

    /* CNT: the instances launched when rays are being counted (opts->count_rays).  The production
     * instances (CNT = false) never read `cnt` nor the truncation counter: the compiler drops the
     * per-lane counters and the whole bookkeeping from them. */
    if constexpr (CNT) {
        atomicAdd(P.ray_counters + 0, (unsigned long long)cnt.primary);
        atomicAdd(P.ray_counters + 1, (unsigned long long)cnt.shadow);
    }
    return false;
}
