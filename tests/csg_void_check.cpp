/* Host build of the CsgDiff void-tile test (chess2rt_amd/csrc/csg_void.h) for tests/test_csg_void_tiles.py and
 * scripts/csg_void_tiles.py: the same classifier the mask pre-pass runs, per tile of a frame, so that the oracle can
 * check every ray of every tile it calls void. */
#include <algorithm>
#include <cmath>
#include <cstddef>

#include "../chess2rt_amd/csrc/csg_void.h"

using c2rt::VoidNode;

/* One tile, pixel columns [tx0, tx0 + 8) and frame rows [ty0, ty1] (tile_mask_entry's tile bounds): bit 0 = no
 * primary ray can hit the node, bit 1 = no shadow ray towards `light` from the tile's ground footprint (plane
 * y = gy) can hit it (only where all four corner rays meet the plane in front of the eye, as tile_mask_entry has
 * it).  v: box / sphere / r2 as in VoidNode, flags selects the tests. */
static unsigned char classify_tile(const double pos[3], const double ul[3], const double du[3], const double dv[3], double fw,
                                   double fh, int tx0, int ty0, int ty1, const VoidNode &v, const double light[3], double gy)
{
    unsigned char r = 0;
    double dir[4][3];
    c2rt::tile_corner_dirs(pos, ul, du, dv, fw, fh, tx0, tx0 + 8, ty0, ty1 + 1, dir);
    if ((v.flags & 1u) && c2rt::pyramid_void(pos, dir, v)) r |= 1;
    if (v.flags & 2u) {
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
        if (ok && std::fabs(fx0) < 1e300 && std::fabs(fx1) < 1e300 && std::fabs(fz0) < 1e300 && std::fabs(fz1) < 1e300) {
            double sdir[4][3];
            c2rt::footprint_dirs(light, gy, fx0, fx1, fz0, fz1, sdir);
            if (c2rt::pyramid_void(light, sdir, v)) r |= 2;
        }
    }
    return r;
}

static VoidNode void_node(const double lo[3], const double hi[3], const double c[3], double r2, unsigned flags)
{
    VoidNode v{};
    for (int i = 0; i < 3; ++i) { v.lo[i] = lo[i]; v.hi[i] = hi[i]; v.c[i] = c[i]; }
    v.r2 = r2;
    v.flags = flags;
    return v;
}

extern "C" {

/* Per 8x8 tile of a W x H frame (the full-frame tile grid: rows [8 ty, min(8 ty + 7, H - 1)]), out[ty * tw + tx]. */
void c2rt_void_classify(const double pos[3], const double ul[3], const double du[3], const double dv[3], double fw, double fh,
                        int W, int H, const double lo[3], const double hi[3], const double c[3], double r2, unsigned flags,
                        const double light[3], double gy, unsigned char *out)
{
    const VoidNode v = void_node(lo, hi, c, r2, flags);
    const int tw = (W + 7) / 8, th = (H + 7) / 8;
    for (int ty = 0; ty < th; ++ty)
        for (int tx = 0; tx < tw; ++tx)
            out[(size_t)ty * tw + tx] = classify_tile(pos, ul, du, dv, fw, fh, tx * 8, ty * 8, std::min(ty * 8 + 7, H - 1), v, light, gy);
}

/* The same for explicit tiles: bounds[3 k .. 3 k + 2] = {tx0, ty0, ty1} (first pixel column, first and last frame
 * row), e.g. the tiles a strip-sharded or chunked frame's pre-pass evaluates; out[k]. */
void c2rt_void_classify_tiles(const double pos[3], const double ul[3], const double du[3], const double dv[3], double fw,
                              double fh, size_t n_tiles, const int *bounds, const double lo[3], const double hi[3],
                              const double c[3], double r2, unsigned flags, const double light[3], double gy, unsigned char *out)
{
    const VoidNode v = void_node(lo, hi, c, r2, flags);
    for (size_t k = 0; k < n_tiles; ++k)
        out[k] = classify_tile(pos, ul, du, dv, fw, fh, bounds[3 * k], bounds[3 * k + 1], bounds[3 * k + 2], v, light, gy);
}

double c2rt_void_margin(double scale) { return c2rt::void_margin(scale); }

} /* extern "C" */
