/* Host build of the planner for tests/test_ground_fast_plan.py: which frames fill_params hands to the ground-tile path
 * (RenderParams::ground_fast, chess2rt_amd/csrc/scene_plan.cpp).  No ROCm on the include path, like
 * tests/scene_plan_check.cpp. */
#include <string>

#include "../chess2rt_amd/csrc/scene_plan.h"

using namespace c2rt;

extern "C" {

/* plans `s` and the frame (cam, opts) under C2RT_DEBUG_CULL = debug_cull: RenderParams::ground_fast, with the frame's
 * ground node and number of culled nodes beside it; -1 when the scene is refused */
int c2rt_ground_fast_of(const c2rt_scene_desc *s, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, int debug_cull,
                        int32_t *ground_node, uint32_t *n_cull)
{
    ScenePlan plan;
    std::string err;
    if (plan_scene(s, plan, err) != C2RT_OK) return -1;
    DiagKnobs knobs;
    knobs.debug_cull = debug_cull;
    RenderParams p;
    fill_params(plan, DeviceTables(), knobs, cam, opts, p);
    *ground_node = p.ground_node;
    *n_cull = p.n_cull;
    return (int)p.ground_fast;
}

} /* extern "C" */
