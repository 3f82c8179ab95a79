/*
 * ground_certain_check.c — chess2rt_amd/csrc/ground_certain.h against the reference's chain for a ground hit, written
 * out below in IEEE doubles in the reference's operation order (what exact:: computes in c2rt_trace.inc: screen ray,
 * normalize, Node.intersect's second normalize, Plane.intersect, BitmapTexture.getTexColor's two floats, the light
 * vector, its squared length, square root, reciprocal, cosTheta, test_visibility's ground pre-check).  Built with
 * -ffp-contract=off.  Host only (tests/test_ground_certain_host.py).
 *
 *   ground_certain_check grid  W H taps  pos[3] up_left[3] du[3] dv[3] fw fh  gy limit  L[3]  s
 *   ground_certain_check pitch W H taps  pos[3] yaw_x yaw_z pitch_deg half_w  gy limit  L[3]  s
 *   ground_certain_check random N [kp_scale]
 *   ground_certain_check edges N
 *
 * Every section prints one line of key=value figures and the program exits 1 if a bound is exceeded (a) or a
 * "certain" float or decision differs from the reference's (b).  kp_scale (default 1) multiplies every interval the
 * header hands out around the hit point, for the mutation run: with 0 the same operands must show mismatches.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* seeds of the two Newton iterations: off by up to 2^-20 either way, drawn per call */
static _Thread_local double gc_seed_scale = 1.0;
#define GC_SEED_SCALE gc_seed_scale
#include "../chess2rt_amd/csrc/ground_certain.h"

typedef struct { double x, y, z; } v3;

typedef struct {
    int miss, away, up, precheck, cos_pos;
    double px, py, pz, r2, cosv;
    float fu, fv, r2f, cosf;
} ref_t;

/* the reference, operation for operation */
static ref_t reference(v3 o, v3 raw, double gy, double limit, int lit, v3 L, int textured, double s)
{
    ref_t r;
    memset(&r, 0, sizeof r);
    const double s2 = raw.x * raw.x + raw.y * raw.y + raw.z * raw.z;
    const double len = sqrt(s2), inv = 1.0 / len;
    const v3 d = {raw.x * inv, raw.y * inv, raw.z * inv};
    const double s2b = d.x * d.x + d.y * d.y + d.z * d.z;
    const double len2 = sqrt(s2b), inv2 = 1.0 / len2;
    const v3 dn = {d.x * inv2, d.y * inv2, d.z * inv2};
    r.away = ((o.y > gy) & (dn.y > -1e-9)) | ((o.y < gy) & (dn.y < 1e-9));
    const double mult = (o.y - gy) / -dn.y;
    const v3 p = {o.x + dn.x * mult, o.y + dn.y * mult, o.z + dn.z * mult};
    r.miss = r.away | (mult > 1e99 * len2) | (fabs(p.x) > limit) | (fabs(p.z) > limit);
    r.px = p.x; r.py = p.y; r.pz = p.z;
    r.up = d.y < 0;
    if (textured) {
        double a = p.x * s, b = p.z * s;
        a = a - floor(a);
        b = b - floor(b);
        r.fu = (float)a;
        r.fv = (float)b;
    }
    r.precheck = 1;
    if (lit) {
        const double from_y = p.y + (r.up ? 1e-6 : -1e-6);
        const v3 lv = {L.x - p.x, L.y - p.y, L.z - p.z};
        r.r2 = lv.x * lv.x + lv.y * lv.y + lv.z * lv.z;
        const double rlen = sqrt(r.r2), rinv = 1.0 / rlen;
        const double ldy = lv.y * rinv;
        r.cosv = r.up ? ldy : -ldy;
        r.cos_pos = r.cosv > 0;
        r.r2f = (float)r.r2;
        r.cosf = (float)r.cosv;
        const double raw_y = L.y - from_y;
        const int sane = (fabs(lv.x) < 1e150) & (fabs(lv.z) < 1e150);
        const int rises = (raw_y > 1e-150) & (raw_y < 1e150), falls = (raw_y < -1e-150) & (raw_y > -1e150);
        r.precheck = sane & (((from_y > gy) & rises) | ((from_y < gy) & falls));
    }
    return r;
}

typedef struct {
    unsigned long long samples, hits, miss_sure, unsure, tex_unsure, light_unsure, violations, mismatches;
    double max_p, max_py, max_r2, max_cos;
} tally;

static void tally_add(tally *a, const tally *b)
{
    a->samples += b->samples; a->hits += b->hits; a->miss_sure += b->miss_sure; a->unsure += b->unsure;
    a->tex_unsure += b->tex_unsure; a->light_unsure += b->light_unsure; a->violations += b->violations; a->mismatches += b->mismatches;
    if (b->max_p > a->max_p) a->max_p = b->max_p;
    if (b->max_py > a->max_py) a->max_py = b->max_py;
    if (b->max_r2 > a->max_r2) a->max_r2 = b->max_r2;
    if (b->max_cos > a->max_cos) a->max_cos = b->max_cos;
}

static uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static uint64_t rng_next(uint64_t *s)
{
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double rng_unit(uint64_t *s) { return (double)(rng_next(s) >> 11) * 0x1p-53; }
static double rng_log(uint64_t *s, double lo, double hi) { return lo * exp(rng_unit(s) * log(hi / lo)); }

static double g_kp = 1.0; /* mutation: scales every interval */

/* One sample through both chains.  Returns whether the short chain was unsure of anything the pixel reads. */
static int one_sample(v3 o, v3 raw, double gy, double limit, int lit, v3 L, int textured, double s, const gc_frame *f, uint64_t *seed, tally *t)
{
    const ref_t r = reference(o, raw, gy, limit, lit, L, textured, s);
    gc_seed_scale = 1.0 + (rng_unit(seed) * 2 - 1) * 0x1p-20;
    double px, pz, bx, bz, q;
    const int state = gc_hit(o.x, o.z, o.y - gy, raw.x, raw.y, raw.z, f->cq, limit, &px, &pz, &bx, &bz, &q);
    t->samples++;
    /* (a) the hit point's bounds wherever the reference's ray meets the plane and the lane is in the windows */
    const double m1 = fabs(raw.x) + fabs(raw.y) + fabs(raw.z);
    const int in_domain = (m1 >= 0x1p-90) & (m1 < 0x1p90) & (raw.y < 0) & (-raw.y > 1.001e-9 * m1);
    if (in_domain) {
        const long double ex = fabsl((long double)r.px - px), ez = fabsl((long double)r.pz - pz);
        const long double rx_ = ex > 0 ? ex / bx : 0, rz_ = ez > 0 ? ez / bz : 0; /* (an exact hit under a zero bound: the column under the eye) */
        const long double e = rx_ > rz_ ? rx_ : rz_;
        if (bx > GC_KP * GC_U * q * (1 + 0x1p-40) || bz > GC_KP * GC_U * q * (1 + 0x1p-40)) t->violations++; /* BX, BZ <= BQ: gc_light relies on it */
        if (e > t->max_p) t->max_p = (double)e;
        const long double by = 3.1L * GC_U * (o.y - gy) + 1.01L * GC_U * fabs(gy);
        const long double ey = fabsl((long double)r.py - gy) / by;
        if (ey > t->max_py) t->max_py = (double)ey;
        if (e > 1 || ey > 1 || r.away) t->violations++;
    }
    if (state == GC_UNSURE) { t->unsure++; return 1; }
    if (state == GC_MISS) {
        t->miss_sure++;
        if (!r.miss) t->mismatches++;
        return 0;
    }
    t->hits++;
    if (r.miss || !r.up || !r.precheck) t->mismatches++;
    int unsure = 0;
    if (textured) {
        float fu, fv;
        const int cu = gc_tex_float(px, bx * g_kp, s, &fu), cv = gc_tex_float(pz, bz * g_kp, s, &fv);
        if (cu && fbits(fu) != fbits(r.fu)) t->mismatches++;
        if (cv && fbits(fv) != fbits(r.fv)) t->mismatches++;
        if (!cu || !cv) { unsure = 1; t->tex_unsure++; }
    }
    if (lit) {
        float r2f, cosf;
        double dbg[4];
        const gc_frame g = *f;
        gc_seed_scale = 1.0 + (rng_unit(seed) * 2 - 1) * 0x1p-20;
        const int cl = g_kp == 1.0 ? gc_light(px, pz, q, L.x, L.z, &g, &r2f, &cosf, dbg)
                                   : gc_light(px, pz, q * g_kp, L.x, L.z, &g, &r2f, &cosf, dbg);
        if (g_kp == 1.0) {
            const long double e2 = fabsl((long double)r.r2 - dbg[0]) / dbg[1];
            if (e2 > t->max_r2) t->max_r2 = (double)e2;
            if (e2 > 1) t->violations++;
            if (dbg[3] > 0 && dbg[3] < 0x1p-22 * dbg[2]) {
                const long double ec = fabsl((long double)r.cosv - dbg[2]) / dbg[3];
                if (ec > t->max_cos) t->max_cos = (double)ec;
                if (ec > 1) t->violations++;
            }
        }
        if (cl && (fbits(r2f) != fbits(r.r2f) || fbits(cosf) != fbits(r.cosf) || !r.cos_pos)) t->mismatches++;
        if (!cl) { unsure = 1; t->light_unsure++; }
    }
    return unsure;
}

static void report(const char *name, const tally *t, unsigned long long tiles, unsigned long long tiles_unsure)
{
    printf("%s samples=%llu hits=%llu sure_misses=%llu unsure_lanes=%llu tex_unsure=%llu light_unsure=%llu max_p=%.4f max_py=%.4f "
           "max_r2=%.4f max_cos=%.4f violations=%llu mismatches=%llu ground_tiles=%llu unsure_tiles=%llu\n",
           name, t->samples, t->hits, t->miss_sure, t->unsure, t->tex_unsure, t->light_unsure, t->max_p, t->max_py, t->max_r2, t->max_cos,
           t->violations, t->mismatches, tiles, tiles_unsure);
}

/* a whole frame, tile by tile as the kernel walks it: 8x8 lanes, `taps` taps of the AA kernel */
static int run_grid(const char *name, int W, int H, int taps, v3 pos, v3 ul, v3 du, v3 dv, double fw, double fh, double gy, double limit, v3 L, double s)
{
    static const double aax[5] = {0.0, 0.3, 0.6, 0.0, 0.6}, aay[5] = {0.0, 0.3, 0.0, 0.6, 0.6};
    const double o3[3] = {pos.x, pos.y, pos.z}, L3[3] = {L.x, L.y, L.z};
    const float cq = gc_plan(o3, gy, limit, 1, L3, 1, s);
    if (!(cq > 0)) { printf("%s refused\n", name); return 1; }
    const gc_frame f = gc_frame_of((double)cq, 1, L.y, gy);
    tally all;
    memset(&all, 0, sizeof all);
    unsigned long long tiles = 0, tiles_unsure = 0;
    const int ty_n = (H + 7) / 8, tx_n = (W + 7) / 8;
#pragma omp parallel
    {
        tally t;
        memset(&t, 0, sizeof t);
        unsigned long long my_tiles = 0, my_unsure = 0;
#pragma omp for schedule(dynamic, 4)
        for (int ty = 0; ty < ty_n; ++ty) {
            uint64_t seed = 0x1234 + (uint64_t)ty;
            for (int tx = 0; tx < tx_n; ++tx) {
                int any_unsure = 0, all_hit = 1;
                for (int l = 0; l < 64; ++l) {
                    const int x = tx * 8 + l % 8, y = ty * 8 + l / 8;
                    if (x >= W || y >= H) continue;
                    for (int k = 0; k < taps; ++k) {
                        const double fx = ((double)x + aax[k]) / fw, fy = ((double)y + aay[k]) / fh;
                        const v3 target = {ul.x + du.x * fx + dv.x * fy, ul.y + du.y * fx + dv.y * fy, ul.z + du.z * fx + dv.z * fy};
                        const v3 raw = {target.x - pos.x, target.y - pos.y, target.z - pos.z};
                        const unsigned long long m0 = t.miss_sure;
                        any_unsure |= one_sample(pos, raw, gy, limit, 1, L, 1, s, &f, &seed, &t);
                        all_hit &= t.miss_sure == m0; /* a ground tile: no sample certainly misses */
                    }
                }
                if (all_hit) { my_tiles++; my_unsure += any_unsure; }
            }
        }
#pragma omp critical
        { tally_add(&all, &t); tiles += my_tiles; tiles_unsure += my_unsure; }
    }
    report(name, &all, tiles, tiles_unsure);
    return all.violations != 0 || all.mismatches != 0;
}

static v3 cross(v3 a, v3 b) { v3 c = {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; return c; }

/* random rays and floors: every binade of |raw.y| / |raw| down to the away threshold, eye heights 1e-3 .. 1e5,
 * scalings 1e-4 .. 1e3, light heights from 1e-3 up, frames the planner refuses among them (counted, then skipped) */
static int run_random(unsigned long long n)
{
    tally all;
    memset(&all, 0, sizeof all);
    unsigned long long refused = 0;
#pragma omp parallel
    {
        tally t;
        memset(&t, 0, sizeof t);
        unsigned long long my_refused = 0;
#pragma omp for schedule(static)
        for (long long blk = 0; blk < (long long)((n + 63) / 64); ++blk) {
            uint64_t seed = 0xABCDEF + (uint64_t)blk * 7919u;
            /* one frame per block of 64 samples */
            const double eye = rng_log(&seed, 1e-3, 1e5), gy = (rng_unit(&seed) < 0.5) ? 0.0 : (rng_unit(&seed) * 2 - 1) * 100.0;
            const v3 o = {(rng_unit(&seed) * 2 - 1) * 1e3, gy + eye, (rng_unit(&seed) * 2 - 1) * 1e3};
            const v3 L = {(rng_unit(&seed) * 2 - 1) * 1e3, gy + rng_log(&seed, 1e-3, 1e4), (rng_unit(&seed) * 2 - 1) * 1e3};
            const double s = rng_log(&seed, 1e-4, 1e3) * (rng_unit(&seed) < 0.1 ? -1 : 1);
            const double limit = rng_unit(&seed) < 0.3 ? NAN : (rng_unit(&seed) < 0.3 ? 1e99 : rng_log(&seed, 1.0, 1e6));
            const double o3[3] = {o.x, o.y, o.z}, L3[3] = {L.x, L.y, L.z};
            const float cq = gc_plan(o3, gy, limit, 1, L3, 1, s);
            if (!(cq > 0)) { my_refused++; continue; }
            const gc_frame f = gc_frame_of((double)cq, 1, L.y, gy);
            for (int k = 0; k < 64; ++k) {
                /* |raw.y| / |raw| = 2^-e, e uniform over [0, 31] (1e-9 = 2^-29.9), the sign of raw.y mostly down */
                const double ratio = exp2(-rng_unit(&seed) * 31.0), az = rng_unit(&seed) * 6.283185307179586, scale = rng_log(&seed, 1e-3, 1e3);
                const double hz = sqrt(fmax(0.0, 1 - ratio * ratio));
                v3 raw = {hz * cos(az) * scale, -ratio * scale, hz * sin(az) * scale};
                if (rng_unit(&seed) < 0.02) raw.y = -raw.y;
                one_sample(o, raw, gy, limit, 1, L, 1, s, &f, &seed, &t);
            }
        }
#pragma omp critical
        { tally_add(&all, &t); refused += my_refused; }
    }
    report("random", &all, 0, 0);
    printf("random_frames refused=%llu\n", refused);
    return all.violations != 0 || all.mismatches != 0 || all.hits == 0;
}

/* hit points placed on integer p * s, on texel edges (p * s * 256 an integer), on `limit`, and under the light: the eye
 * and the target are chosen first, the ray is their rounded difference, so the reference lands within a few ulps */
static int run_edges(unsigned long long n)
{
    tally all;
    memset(&all, 0, sizeof all);
    unsigned long long placed = 0;
#pragma omp parallel
    {
        tally t;
        memset(&t, 0, sizeof t);
        unsigned long long my_placed = 0;
#pragma omp for schedule(static)
        for (long long i = 0; i < (long long)n; ++i) {
            uint64_t seed = 0x5EED + (uint64_t)i * 104729u;
            const int kind = (int)(i % 4);
            const double s = (i / 4) % 2 ? 0.125 : rng_log(&seed, 1e-2, 1e2);
            const double gy = 0.0, eye = rng_log(&seed, 1e-2, 1e3);
            const v3 o = {floor((rng_unit(&seed) * 2 - 1) * 100), gy + eye, floor((rng_unit(&seed) * 2 - 1) * 100)};
            double tx = (rng_unit(&seed) * 2 - 1) * 500, tz = (rng_unit(&seed) * 2 - 1) * 500, limit = 1e99;
            v3 L = {(rng_unit(&seed) * 2 - 1) * 300, gy + rng_log(&seed, 1e-3, 1e3), (rng_unit(&seed) * 2 - 1) * 300};
            if (kind == 0) { tx = floor(tx * s) / s; tz = floor(tz * s) / s; }                         /* integer p * s */
            if (kind == 1) { tx = floor(tx * s * 256) / (s * 256); tz = floor(tz * s * 256) / (s * 256); } /* texel edges */
            if (kind == 2) limit = fabs(rng_unit(&seed) < 0.5 ? tx : tz);                                /* on limit */
            if (kind == 3) { L.x = tx; L.z = tz; }                                                      /* the light above the hit */
            const v3 raw = {tx - o.x, gy - o.y, tz - o.z};
            const double o3[3] = {o.x, o.y, o.z}, L3[3] = {L.x, L.y, L.z};
            const float cq = gc_plan(o3, gy, limit, 1, L3, 1, s);
            if (!(cq > 0)) continue;
            const gc_frame f = gc_frame_of((double)cq, 1, L.y, gy);
            my_placed++;
            one_sample(o, raw, gy, limit, 1, L, 1, s, &f, &seed, &t);
        }
#pragma omp critical
        { tally_add(&all, &t); placed += my_placed; }
    }
    report("edges", &all, 0, 0);
    printf("edges_placed n=%llu\n", placed);
    return all.violations != 0 || all.mismatches != 0 || all.unsure + all.tex_unsure == 0;
}

/* gc_plan's refusals */
static int run_refusals(void)
{
    const double L[3] = {10, 50, 10}, low[3] = {10, 0.25, 10}, below[3] = {10, -1, 10}, nanv[3] = {NAN, 50, 10};
    const double eye[3] = {0, 5, 0}, eye_below[3] = {0, -5, 0}, eye_on[3] = {0, 0, 0}, eye_far[3] = {0x1p41, 5, 0}, eye_nan[3] = {0, NAN, 0};
    int bad = 0;
    bad += (gc_plan(eye, 0, 1e99, 1, L, 1, 0.1) > 0) != 1;
    bad += (gc_plan(eye, 0, 1e99, 0, L, 0, 0.0) > 0) != 1;      /* no light, no texture: nothing of them is read */
    bad += (gc_plan(eye_below, 0, 1e99, 1, L, 1, 0.1) > 0) != 0;
    bad += (gc_plan(eye_on, 0, 1e99, 1, L, 1, 0.1) > 0) != 0;
    bad += (gc_plan(eye_far, 0, 1e99, 1, L, 1, 0.1) > 0) != 0;
    bad += (gc_plan(eye_nan, 0, 1e99, 1, L, 1, 0.1) > 0) != 0;
    bad += (gc_plan(eye, 0, 1e99, 1, below, 1, 0.1) > 0) != 0;
    bad += (gc_plan(eye, 0, 1e99, 0, below, 1, 0.1) > 0) != 1;  /* a light that does not shine is not read */
    bad += (gc_plan(eye, 0, 1e99, 1, nanv, 1, 0.1) > 0) != 0;
    bad += (gc_plan(eye, 0, 1e99, 1, low, 1, 0.1) > 0) != 0;   /* the eye more than 16 light heights up */
    bad += (gc_plan(eye, 0, 1e99, 1, L, 1, 0.0) > 0) != 0;
    bad += (gc_plan(eye, 0, 1e99, 1, L, 1, INFINITY) > 0) != 0;
    bad += (gc_plan(eye, 0, 1e99, 1, L, 1, NAN) > 0) != 0;
    bad += (gc_plan(eye, 0, NAN, 1, L, 1, 0.1) > 0) != 1;      /* no limit: a plane from a scene file */
    bad += (gc_plan(eye, 0, 0.0, 1, L, 1, 0.1) > 0) != 0;
    bad += (gc_plan(eye, 0, -1.0, 1, L, 1, 0.1) > 0) != 0;
    bad += (gc_plan(eye, NAN, 1e99, 1, L, 1, 0.1) > 0) != 0;
    bad += (gc_plan(eye, 0x1p21, 1e99, 1, L, 1, 0.1) > 0) != 0;
    printf("refusals failures=%d\n", bad);
    return bad != 0;
}

static double num(char **argv, int i) { return strtod(argv[i], NULL); }

int main(int argc, char **argv)
{
    int rc = 1;
    if (argc >= 2 && !strcmp(argv[1], "grid") && argc == 25) {
        const v3 pos = {num(argv, 5), num(argv, 6), num(argv, 7)}, ul = {num(argv, 8), num(argv, 9), num(argv, 10)};
        const v3 du = {num(argv, 11), num(argv, 12), num(argv, 13)}, dv = {num(argv, 14), num(argv, 15), num(argv, 16)};
        const v3 L = {num(argv, 21), num(argv, 22), num(argv, 23)};
        rc = run_grid("grid", atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), pos, ul, du, dv, num(argv, 17), num(argv, 18), num(argv, 19), num(argv, 20), L, num(argv, 24));
    } else if (argc >= 2 && !strcmp(argv[1], "pitch") && argc == 18) {
        /* the camera at pos looking along (yaw_x, ., yaw_z) pitched by pitch_deg, half_w = tan(half the horizontal field) */
        const int W = atoi(argv[2]), H = atoi(argv[3]);
        const v3 pos = {num(argv, 5), num(argv, 6), num(argv, 7)};
        const double yx = num(argv, 8), yz = num(argv, 9), pitch = num(argv, 10) * 3.14159265358979323846 / 180, hw = num(argv, 11);
        const double yl = sqrt(yx * yx + yz * yz);
        const v3 fwd = {cos(pitch) * yx / yl, sin(pitch), cos(pitch) * yz / yl}, world_up = {0, 1, 0};
        v3 right = cross(world_up, fwd);
        const double rl = sqrt(right.x * right.x + right.y * right.y + right.z * right.z);
        right.x /= rl; right.y /= rl; right.z /= rl;
        const v3 up = cross(fwd, right);
        const double hh = hw * H / W;
        const v3 ul = {pos.x + fwd.x - right.x * hw + up.x * hh, pos.y + fwd.y - right.y * hw + up.y * hh, pos.z + fwd.z - right.z * hw + up.z * hh};
        const v3 du = {2 * hw * right.x, 2 * hw * right.y, 2 * hw * right.z}, dv = {-2 * hh * up.x, -2 * hh * up.y, -2 * hh * up.z};
        const v3 L = {num(argv, 14), num(argv, 15), num(argv, 16)};
        rc = run_grid("pitch", W, H, atoi(argv[4]), pos, ul, du, dv, (double)W, (double)H, num(argv, 12), num(argv, 13), L, num(argv, 17));
    } else if (argc >= 3 && !strcmp(argv[1], "random")) {
        if (argc >= 4) g_kp = num(argv, 3);
        rc = run_random(strtoull(argv[2], NULL, 10));
        rc |= run_refusals();
    } else if (argc >= 3 && !strcmp(argv[1], "edges")) {
        if (argc >= 4) g_kp = num(argv, 3);
        rc = run_edges(strtoull(argv[2], NULL, 10));
    } else {
        fprintf(stderr, "usage: see the head of tests/ground_certain_check.c\n");
        return 2;
    }
    printf(rc ? "FAILED\n" : "ALL OK\n");
    return rc;
}
