/* Host build of the dark-tile test of the mask pre-pass (chess2rt_amd/csrc/csg_void.h: tile_dark_by; the planner's
 * part, chess2rt_amd/csrc/scene_plan.cpp: dark_cull_of) for tests/test_ground_dark_tiles.py, tests/test_gpu_ground_dark.py
 * and scripts/ground_dark_tiles.py: the same classifier tile_mask_entry runs, per tile, so that the oracle can check
 * every shadow ray of every tile it calls dark.  No ROCm on the include path, like tests/scene_plan_check.cpp. */
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>

#include "../chess2rt_amd/csrc/scene_plan.h"

using namespace c2rt;

extern "C" {

struct DarkFrame {
    DarkCull d;
    double light[3];
    double ground_y;
    int32_t ground_node;
    uint32_t n_cull;
};

/* plans `s` and the frame (cam, opts) under C2RT_DEBUG_CULL = debug_cull: the DarkCull its pre-pass is given, with
 * light 0 and the ground beside it; returns sizeof(DarkFrame), 0 when the scene is refused */
size_t c2rt_ground_dark_frame(const c2rt_scene_desc *s, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, int debug_cull,
                              DarkFrame *out)
{
    ScenePlan plan;
    std::string err;
    std::memset(out, 0, sizeof *out);
    if (plan_scene(s, plan, err) != C2RT_OK) return 0;
    DiagKnobs knobs;
    knobs.debug_cull = debug_cull;
    RenderParams p;
    fill_params(plan, DeviceTables(), knobs, cam, opts, p);
    out->d = dark_cull_of(plan, knobs, p);
    for (int j = 0; j < 3 && plan.light_pos.size() >= 3; ++j) out->light[j] = plan.light_pos[j];
    out->ground_y = p.ground_y;
    out->ground_node = p.ground_node;
    out->n_cull = p.n_cull;
    return sizeof *out;
}

/* Explicit tiles: bounds[3 k .. 3 k + 2] = {tx0, ty0, ty1} (first pixel column, first and last frame row); out[k] = 1
 * when every shadow ray towards `light` from the tile's ground footprint (plane y = gy) is occluded by node `k`: the
 * footprint as tile_mask_entry builds it, only where all four corner rays meet the plane in front of the eye. */
void c2rt_ground_dark_classify_tiles(const double pos[3], const double ul[3], const double du[3], const double dv[3], double fw,
                                     double fh, size_t n_tiles, const int *bounds, const DarkNode *k, const double light[3],
                                     double gy, double reach, unsigned char *out)
{
    for (size_t t = 0; t < n_tiles; ++t) {
        const int tx0 = bounds[3 * t], ty0 = bounds[3 * t + 1], ty1 = bounds[3 * t + 2];
        bool ok = true;
        double fx0 = 0, fx1 = 0, fz0 = 0, fz1 = 0;
        for (int c = 0; c < 4; ++c) {
            const double sx = (c & 1) ? (double)(tx0 + 8 + 1) : (double)(tx0 - 1);
            const double sy = (c & 2) ? (double)(ty1 + 2) : (double)(ty0 - 1);
            const double cfx = sx / fw, cfy = sy / fh;
            double d[3];
            for (int i = 0; i < 3; ++i) d[i] = ul[i] + du[i] * cfx + dv[i] * cfy - pos[i];
            const double tt = (gy - pos[1]) / d[1];
            ok = ok && tt > 0 && tt < 1e300;
            const double hx = pos[0] + d[0] * tt, hz = pos[2] + d[2] * tt;
            fx0 = c ? std::fmin(fx0, hx) : hx;
            fx1 = c ? std::fmax(fx1, hx) : hx;
            fz0 = c ? std::fmin(fz0, hz) : hz;
            fz1 = c ? std::fmax(fz1, hz) : hz;
        }
        ok = ok && fx0 <= fx1 && fz0 <= fz1 && std::fabs(fx0) < 1e300 && std::fabs(fx1) < 1e300 && std::fabs(fz0) < 1e300 &&
             std::fabs(fz1) < 1e300;
        out[t] = 0;
        if (!ok) continue;
        double sdir[4][3];
        footprint_dirs(light, gy, fx0, fx1, fz0, fz1, sdir);
        const bool in_reach = std::fmax(std::fabs(fx0), std::fabs(fx1)) + std::fmax(std::fabs(fz0), std::fabs(fz1)) + std::fabs(gy) <= reach;
        out[t] = tile_dark_by(light, sdir, in_reach, *k) ? 1 : 0;
    }
}

} /* extern "C" */
