/* Host build of the planner for tests/test_ground_texel_plan.py: the two decisions behind the short chain's texel fetch
 * and light term (chess2rt_amd/csrc/scene_plan.cpp) — fill_params keeps a frame whose floor bitmap lies outside the
 * 32-bit addressing of bitmap_filtered_uniform on ground_tile, and plan_lights sets DevLight::equal for three bit-equal
 * channels under bit 1 of DevLight::lit.  No ROCm on the include path, like tests/ground_certain_plan_check.cpp. */
#include <cstring>
#include <string>

#include "../chess2rt_amd/csrc/scene_plan.h"

using namespace c2rt;

extern "C" {

/* plans `s` and the frame (cam, opts) with the floor bitmap's description replaced by a fabricated one — `width` x
 * `height` texels from texel `offset` of the pool; nothing is allocated, the planner reads the three numbers only —:
 * RenderParams::ground_certain_cq (0: the frame stays on ground_tile).  width == 0: the scene's own bitmap.  -1 when the
 * scene is refused or its floor has no bitmap. */
double c2rt_ground_texel_cq_of(const c2rt_scene_desc *s, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, uint32_t width,
                               uint32_t height, uint64_t offset)
{
    ScenePlan plan;
    std::string err;
    if (plan_scene(s, plan, err) != C2RT_OK) return -1;
    DiagKnobs knobs;
    RenderParams p;
    fill_params(plan, DeviceTables(), knobs, cam, opts, p);
    if (p.ground_node < 0 || (size_t)p.ground_node >= plan.nodes.size()) return -1;
    DevMat &m = plan.nodes[(size_t)p.ground_node].mat;
    if (m.tex_type != C2RT_TEX_BITMAP) return -1;
    if (width) {
        m.texdata[0] = width;
        m.texdata[1] = height;
        std::memcpy(m.texdata + 4, &offset, sizeof offset);
        fill_params(plan, DeviceTables(), knobs, cam, opts, p);
    }
    return (double)p.ground_certain_cq;
}

/* DevLight::lit + 4 * DevLight::equal of light 0 when its colour is `color` (three floats, taken as bits) and its power
 * `power`; -1 when the scene is refused or has no light */
int c2rt_light_lit_of(const c2rt_scene_desc *s, const float *color, float power)
{
    if (s->n_lights != 1) return -1;
    c2rt_scene_desc d = *s;
    d.light_color = color;
    d.light_power = &power;
    ScenePlan plan;
    std::string err;
    if (plan_scene(&d, plan, err) != C2RT_OK || plan.lights.empty()) return -1;
    if (plan.lights[0].lit > 3u || plan.lights[0].equal > 1u) return -2;
    return (int)(plan.lights[0].lit + 4u * plan.lights[0].equal);
}

} /* extern "C" */
