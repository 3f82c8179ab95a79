/* Host build of the sphere-interior test of the mask pre-pass (chess2rt_amd/csrc/csg_void.h: sphere_interior_tile; the
 * planner's part, chess2rt_amd/csrc/scene_plan.cpp: sphere_cull_of) for tests/test_sphere_interior_tiles.py,
 * tests/test_gpu_sphere_tiles.py and scripts/sphere_interior_tiles.py.  The frame comes from the planner itself
 * (fill_params, void_cull_of, sphere_cull_of); the node loop of tile_mask_entry (c2rt_tile_mask.inc) — rectangle, hull,
 * void and silhouette tests, light-side test — is restated here for tiles that are not primary-ground (the ground
 * refinement never runs on a tile that keeps a sphere), and the claim itself is csg_void.h's own function.  No ROCm on
 * the include path, like tests/scene_plan_check.cpp. */
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>

#include "../chess2rt_amd/csrc/scene_plan.h"

using namespace c2rt;

namespace {

struct Frame {
    ScenePlan plan;
    RenderParams p;
    VoidCull v;
    SphereCull s;
};

} // namespace

extern "C" {

/* plans `s` and the frame (cam, opts) under C2RT_DEBUG_CULL = debug_cull; null when the scene is refused */
void *c2rt_si_new(const c2rt_scene_desc *s, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, int debug_cull)
{
    Frame *f = new Frame;
    std::string err;
    if (plan_scene(s, f->plan, err) != C2RT_OK) {
        delete f;
        return nullptr;
    }
    DiagKnobs knobs;
    knobs.debug_cull = debug_cull;
    fill_params(f->plan, DeviceTables(), knobs, cam, opts, f->p);
    f->v = void_cull_of(f->plan, f->p, ~0u);
    f->s = sphere_cull_of(f->plan, knobs, f->p, ~0u);
    return f;
}

void c2rt_si_free(void *h) { delete (Frame *)h; }

/* info[0] = SphereCull::interior, [1] = SphereCull::n, [2] = n_cull, [3] = ground node (-1: none), [4] = n_lights,
 * [5..8] = the nodes of SphereCull::s; light[3] = light 0 */
void c2rt_si_info(const void *h, int32_t info[9], double light[3])
{
    const Frame &f = *(const Frame *)h;
    info[0] = (int32_t)f.s.interior;
    info[1] = (int32_t)f.s.n;
    info[2] = (int32_t)f.p.n_cull;
    info[3] = f.p.ground_node;
    info[4] = (int32_t)f.p.n_lights;
    for (int j = 0; j < kMaxSphereNodes; ++j) info[5 + j] = j < (int)f.s.n ? (int32_t)f.s.s[j].node : -1;
    for (int j = 0; j < 3; ++j) light[j] = f.v.light0[j];
}

/* Explicit tiles: bounds[3 k .. 3 k + 2] = {tx0, ty0, ty1} (first pixel column, first and last frame row).  Per tile:
 * pmask[k], smask[k] = the first two mask words as tile_mask_entry's node loop leaves them (meaningful where the tile is
 * not primary-ground); node[k] = the claimed sphere's node or -1; claim[k] bit 0 = sphere-interior (the device's bit 3),
 * bit 1 = the same claim with the shadow condition left out.  r_scale != 1: the mutation — obligation (a) is evaluated as if
 * the ball had r_scale times its radius (same margin). */
void c2rt_si_classify(const void *h, size_t n_tiles, const int *bounds, double r_scale, uint32_t *pmask_out, uint32_t *smask_out,
                      int32_t *node_out, unsigned char *claim_out)
{
    const Frame &f = *(const Frame *)h;
    const RenderParams &P = f.p;
    const VoidCull &V = f.v;
    const SphereCull &S = f.s;
    const uint32_t nc = P.n_cull < (uint32_t)kMaxCullNodes ? P.n_cull : (uint32_t)kMaxCullNodes;
    const uint32_t nn = P.n_nodes;
    const int gnode = P.ground_node;
    for (size_t t = 0; t < n_tiles; ++t) {
        const int tx0 = bounds[3 * t], ty0 = bounds[3 * t + 1], ty1 = bounds[3 * t + 2];
        uint32_t pmask = 0xFFFFFFFFu, smask0 = 0xFFFFFFFFu;
        node_out[t] = -1;
        claim_out[t] = 0;
        if (P.n_cull) {
            const float X0 = (float)tx0, X1 = (float)(tx0 + kTileW), Y0 = (float)ty0, Y1 = (float)(ty1 + 1);
            const bool shadow_cull = 0 < P.n_cull_lights;
            const int sx1 = tx0 + kTileW + 1, sy1 = ty1 + 1;
            const int *sd = P.light_side[0];
            const bool in_left = tx0 >= sd[0] && tx0 <= sd[1], in_right = sx1 >= sd[2] && sx1 <= sd[3];
            const bool in_top = ty0 >= sd[4] && ty0 <= sd[5], in_bottom = sy1 >= sd[6] && sy1 <= sd[7];
            double cdir[4][3];
            tile_corner_dirs(P.cam.pos, P.cam.up_left, P.cam_du, P.cam_dv, P.cam.frame_width, P.cam.frame_height, tx0, tx0 + kTileW, ty0,
                             ty1 + 1, cdir);
            const PyramidCone pcone = pyramid_cone(cdir);
            for (uint32_t n = 0; n < nc; ++n) {
                const int r0 = P.cull_rect[n][0], r1 = P.cull_rect[n][1], r2 = P.cull_rect[n][2], r3 = P.cull_rect[n][3];
                const bool rect_misses = r2 <= tx0 || r0 >= tx0 + kTileW || r3 <= ty0 || r1 > ty1;
                bool off_hull = false;
                if (!rect_misses) {
                    for (int e = 0; e < kHullEdges; ++e) {
                        const float a = P.cull_hull[n][e][0], bb = P.cull_hull[n][e][1], c = P.cull_hull[n][e][2];
                        const float ax0 = a * X0, ax1 = a * X1, by0 = bb * Y0, by1 = bb * Y1;
                        const float worst = std::fmax(std::fmax(ax0, ax1) + std::fmax(by0, by1), -3.0e38f) + c;
                        off_hull |= worst < -0.25f;
                    }
                }
                if (rect_misses || off_hull) pmask &= ~(1u << n);
                else {
                    for (uint32_t j = 0; j < V.n; ++j)
                        if (V.v[j].node == n && (V.v[j].flags & 1u) && pyramid_void(P.cam.pos, pcone, V.v[j])) pmask &= ~(1u << n);
                    for (uint32_t j = 0; j < S.n; ++j)
                        if (S.s[j].node == n && (S.s[j].flags & 1u) && cone_misses_ball(P.cam.pos, pcone, S.s[j].c, S.s[j].rp)) pmask &= ~(1u << n);
                }
                if (shadow_cull && ((in_left && r2 <= tx0) || (in_right && r0 >= sx1) || (in_top && r3 <= ty0) || (in_bottom && r1 >= sy1)))
                    smask0 &= ~(1u << n);
            }
            if (S.interior && nn >= 1u && nn <= 32u) {
                const uint32_t live = pmask & (0xFFFFFFFFu >> (32u - nn));
                const uint32_t gbit = gnode >= 0 ? 1u << gnode : 0u;
                const uint32_t rest = live & ~gbit;
                if ((live & gbit) == gbit && rest && !(rest & (rest - 1u)) && (rest & S.interior)) {
                    for (uint32_t j = 0; j < S.n; ++j) {
                        if ((1u << S.s[j].node) != rest) continue;
                        /* (the mutation inflates the INNER ball of obligation (a) alone: the cone test at r_scale R with
                         * the true margin, everything else as it is) */
                        const double R = f.plan.nodes[S.s[j].node].g.p[3], m = S.s[j].rp - R;
                        node_out[t] = (int32_t)S.s[j].node;
                        unsigned char c = 0;
                        double t_lo, t_hi;
                        if (r_scale == 1.0) {
                            if (sphere_interior_tile(P.cam.pos, pcone, S, j, R, V, smask0, nn, gnode, P.ground_y, P.n_lights != 0u)) c |= 1;
                            if (sphere_interior_tile(P.cam.pos, pcone, S, j, R, V, smask0, nn, gnode, P.ground_y, false)) c |= 2;
                        } else if (cone_inside_ball(P.cam.pos, pcone, S.s[j].c, R * r_scale, m, t_lo, t_hi)) {
                            if (sphere_interior_rest(P.cam.pos, pcone, S, j, m, t_lo, t_hi, V, smask0, nn, gnode, P.ground_y, P.n_lights != 0u)) c |= 1;
                            if (sphere_interior_rest(P.cam.pos, pcone, S, j, m, t_lo, t_hi, V, smask0, nn, gnode, P.ground_y, false)) c |= 2;
                        }
                        claim_out[t] = c;
                    }
                }
            }
        }
        pmask_out[t] = pmask;
        smask_out[t] = smask0;
    }
}

} /* extern "C" */
