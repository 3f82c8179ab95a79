/* Host build of the planner for tests/test_ground_certain_plan.py: which frames fill_params hands to the short chain
 * for ground tiles (RenderParams::ground_certain_cq, chess2rt_amd/csrc/scene_plan.cpp; ground_certain.h: gc_plan).  No
 * ROCm on the include path, like tests/ground_fast_check.cpp. */
#include <string>

#include "../chess2rt_amd/csrc/scene_plan.h"

using namespace c2rt;

extern "C" {

/* plans `s` and the frame (cam, opts) under C2RT_DEBUG_CULL = debug_cull: RenderParams::ground_certain_cq (0: the frame
 * stays on ground_tile), with RenderParams::ground_fast beside it; -1 when the scene is refused */
double c2rt_ground_certain_of(const c2rt_scene_desc *s, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, int debug_cull,
                              uint32_t *ground_fast)
{
    ScenePlan plan;
    std::string err;
    if (plan_scene(s, plan, err) != C2RT_OK) return -1;
    DiagKnobs knobs;
    knobs.debug_cull = debug_cull;
    RenderParams p;
    fill_params(plan, DeviceTables(), knobs, cam, opts, p);
    *ground_fast = p.ground_fast;
    return (double)p.ground_certain_cq;
}

} /* extern "C" */
