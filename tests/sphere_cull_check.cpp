/* Host build of the sphere-silhouette test of the mask pre-pass (chess2rt_amd/csrc/csg_void.h: pyramid_cone,
 * cone_misses_ball) for tests/test_sphere_cull_tiles.py and scripts/sphere_cull_tiles.py: the same classifier
 * tile_mask_entry runs, per tile, so that the oracle can check every ray of every tile it drops a sphere node from. */
#include <cmath>
#include <cstddef>

#include "../chess2rt_amd/csrc/csg_void.h"

using c2rt::PyramidCone;

/* One tile, pixel columns [tx0, tx0 + 8) and frame rows [ty0, ty1] (tile_mask_entry's tile bounds): bit 0 = no
 * primary ray passes within rp of c, bit 1 = no shadow ray towards `light` from the tile's ground footprint (plane
 * y = gy) does — only where all four corner rays meet the plane in front of the eye and the footprint stays within
 * `reach`, as tile_mask_entry has it.  flags selects the tests. */
static unsigned char classify_tile(const double pos[3], const double ul[3], const double du[3], const double dv[3], double fw,
                                   double fh, int tx0, int ty0, int ty1, const double c[3], double rp, unsigned flags,
                                   const double light[3], double gy, double reach)
{
    unsigned char r = 0;
    if (flags & 1u) {
        double dir[4][3];
        c2rt::tile_corner_dirs(pos, ul, du, dv, fw, fh, tx0, tx0 + 8, ty0, ty1 + 1, dir);
        if (c2rt::cone_misses_ball(pos, c2rt::pyramid_cone(dir), c, rp)) r |= 1;
    }
    if (flags & 2u) {
        bool ok = true;
        double fx0 = 0, fx1 = 0, fz0 = 0, fz1 = 0;
        for (int k = 0; k < 4; ++k) {
            const double sx = (k & 1) ? (double)(tx0 + 8 + 1) : (double)(tx0 - 1);
            const double sy = (k & 2) ? (double)(ty1 + 2) : (double)(ty0 - 1);
            const double cfx = sx / fw, cfy = sy / fh;
            double d[3];
            for (int i = 0; i < 3; ++i) d[i] = ul[i] + du[i] * cfx + dv[i] * cfy - pos[i];
            const double t = (gy - pos[1]) / d[1];
            ok = ok && t > 0 && t < 1e300;
            const double hx = pos[0] + d[0] * t, hz = pos[2] + d[2] * t;
            fx0 = k ? std::fmin(fx0, hx) : hx;
            fx1 = k ? std::fmax(fx1, hx) : hx;
            fz0 = k ? std::fmin(fz0, hz) : hz;
            fz1 = k ? std::fmax(fz1, hz) : hz;
        }
        ok = ok && fx0 <= fx1 && fz0 <= fz1 && std::fabs(fx0) < 1e300 && std::fabs(fx1) < 1e300 && std::fabs(fz0) < 1e300 &&
             std::fabs(fz1) < 1e300;
        if (ok && std::fmax(std::fabs(fx0), std::fabs(fx1)) + std::fmax(std::fabs(fz0), std::fabs(fz1)) + std::fabs(gy) <= reach) {
            double sdir[4][3];
            c2rt::footprint_dirs(light, gy, fx0, fx1, fz0, fz1, sdir);
            if (c2rt::cone_misses_ball(light, c2rt::pyramid_cone(sdir), c, rp)) r |= 2;
        }
    }
    return r;
}

extern "C" {

/* Explicit tiles: bounds[3 k .. 3 k + 2] = {tx0, ty0, ty1} (first pixel column, first and last frame row); out[k]. */
void c2rt_sphere_classify_tiles(const double pos[3], const double ul[3], const double du[3], const double dv[3], double fw,
                                double fh, size_t n_tiles, const int *bounds, const double c[3], double rp, unsigned flags,
                                const double light[3], double gy, double reach, unsigned char *out)
{
    for (size_t k = 0; k < n_tiles; ++k)
        out[k] = classify_tile(pos, ul, du, dv, fw, fh, bounds[3 * k], bounds[3 * k + 1], bounds[3 * k + 2], c, rp, flags, light, gy, reach);
}

double c2rt_sphere_margin(double scale, double R) { return c2rt::sphere_margin(scale, R); }

/* cone_misses_ball for the pyramid (apex, dir[4][3]); *tan_t and *ok (nullable) report the cone */
int c2rt_cone_misses_ball(const double apex[3], const double *dir, const double c[3], double rp, double *tan_t, int *ok)
{
    double d[4][3];
    for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 3; ++i) d[k][i] = dir[3 * k + i];
    const PyramidCone k = c2rt::pyramid_cone(d);
    if (tan_t) *tan_t = k.tan_t;
    if (ok) *ok = k.ok ? 1 : 0;
    return c2rt::cone_misses_ball(apex, k, c, rp) ? 1 : 0;
}

} /* extern "C" */
