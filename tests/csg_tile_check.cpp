/* Host build of the planner for tests/test_csg_tile_plan.py, tests/test_gpu_csg_tiles.py and scripts/csg_tile_census.py:
 * which nodes of a frame the frame kernel may render beside the ground through lean::csg_tile — the plan's kNodeCsgTile
 * flags (chess2rt_amd/csrc/scene_plan.cpp: plan_csg_tile_nodes) in a frame fill_params grants RenderParams::ground_fast.
 * No ROCm on the include path, like tests/scene_plan_check.cpp. */
#include <string>

#include "../chess2rt_amd/csrc/scene_plan.h"

using namespace c2rt;

extern "C" {

/* plans `s` and the frame (cam, opts) under C2RT_DEBUG_CULL = debug_cull, as the library does (bit 10: drop_csg_tile on
 * the fresh plan): the mask of the nodes the path may take in this frame — 0 without ground_fast —, with the frame's
 * ground node and the plan's own flags (whatever the frame) beside it; -1 when the scene is refused */
int64_t c2rt_csg_tile_nodes(const c2rt_scene_desc *s, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, int debug_cull,
                            int32_t *ground_node, uint32_t *plan_mask)
{
    ScenePlan plan;
    std::string err;
    if (plan_scene(s, plan, err) != C2RT_OK) return -1;
    if (debug_cull & 512) drop_csg_certain(plan);
    if (debug_cull & 1024) drop_csg_tile(plan);
    DiagKnobs knobs;
    knobs.debug_cull = debug_cull;
    RenderParams p;
    fill_params(plan, DeviceTables(), knobs, cam, opts, p);
    uint32_t mask = 0;
    for (size_t n = 0; n < plan.nodes.size() && n < 32; ++n)
        if (plan.nodes[n].flags & kNodeCsgTile) mask |= 1u << n;
    *ground_node = p.ground_node;
    *plan_mask = mask;
    return p.ground_fast && plan.nodes.size() <= 32 ? (int64_t)mask : 0;
}

} /* extern "C" */
