/*
 * scene_plan_check.cpp — host build of the planner (chess2rt_amd/csrc/scene_plan.cpp) for tests/test_scene_plan.py:
 * plans a c2rt_scene_desc and a frame on the CPU and hands back what the library would upload and launch with.
 * Built without ROCm on the include path (Makefile): the planner must not need it.
 */
#include <cstdio>
#include <cstring>

#include "../chess2rt_amd/csrc/scene_plan.h"

using namespace c2rt;

namespace {

void put(char *msg, size_t len, const std::string &err)
{
    if (msg && len) std::snprintf(msg, len, "%s", err.c_str());
}

template <typename T>
uint64_t fnv(uint64_t h, const std::vector<T> &v)
{
    const unsigned char *b = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return (h ^ v.size()) * 0x100000001b3ull;
}

} // namespace

extern "C" {

struct PlanFacts {
    int32_t ground_node, csg_levels;
    double ground_y;
    uint32_t planes_only, all_identity, n_nodes, n_lights, n_void, n_sphere;
    uint64_t tables_hash;          /* every packed table and host-side vector of the plan, byte for byte */
    VoidNode void_nodes[kMaxVoidNodes];
    SphereNode sphere_nodes[kMaxSphereNodes];
};

struct FramePlan {
    uint32_t n_cull, n_cull_lights;
    int32_t ground_node;
    uint32_t row_group_start, force_exact, pad;
    int32_t cull_rect[kMaxCullNodes][4];
    float cull_hull[kMaxCullNodes][kHullEdges][3];
    int32_t light_side[kMaxCullLights][8];
    VoidCull v;
    SphereCull s;
};

void *c2rt_plan_new(void) { return new ScenePlan(); }
void c2rt_plan_free(void *plan) { delete static_cast<ScenePlan *>(plan); }

int c2rt_plan_scene(void *plan, const c2rt_scene_desc *s, char *msg, size_t msg_len)
{
    std::string err;
    const int st = plan_scene(s, *static_cast<ScenePlan *>(plan), err);
    put(msg, msg_len, err);
    return st;
}

size_t c2rt_plan_facts(const void *plan, PlanFacts *out, uint8_t *node_boxed, size_t n_boxed)
{
    const ScenePlan &p = *static_cast<const ScenePlan *>(plan);
    std::memset(out, 0, sizeof *out);
    out->ground_node = p.ground_node;
    out->csg_levels = p.csg_levels;
    out->ground_y = p.ground_y;
    out->planes_only = p.planes_only;
    out->all_identity = p.all_identity;
    out->n_nodes = p.n_nodes;
    out->n_lights = p.n_lights;
    out->n_void = (uint32_t)p.void_nodes.size();
    out->n_sphere = (uint32_t)p.sphere_nodes.size();
    for (size_t i = 0; i < p.void_nodes.size(); ++i) out->void_nodes[i] = p.void_nodes[i];
    for (size_t i = 0; i < p.sphere_nodes.size(); ++i) out->sphere_nodes[i] = p.sphere_nodes[i];
    uint64_t h = 0xcbf29ce484222325ull;
    h = fnv(h, p.geoms); h = fnv(h, p.nodes); h = fnv(h, p.shaders); h = fnv(h, p.textures); h = fnv(h, p.lights);
    h = fnv(h, p.texels4); h = fnv(h, p.shadow_rects); h = fnv(h, p.node_box); h = fnv(h, p.node_boxed); h = fnv(h, p.light_pos);
    out->tables_hash = h;
    for (size_t n = 0; n < n_boxed && n < p.node_boxed.size(); ++n) node_boxed[n] = p.node_boxed[n];
    return sizeof *out;
}

/* one node of the plan: its DevNode flags (c2rt_device.h), whether plan_world_boxes boxed it and the eight world corners
 * of its padded box; 0 when n is out of range */
int c2rt_plan_node(const void *plan, uint32_t n, uint32_t *flags, uint8_t *boxed, double corners[24])
{
    const ScenePlan &p = *static_cast<const ScenePlan *>(plan);
    if (n >= p.nodes.size()) return 0;
    *flags = p.nodes[n].flags;
    *boxed = p.node_boxed[n];
    std::memcpy(corners, &p.node_box[(size_t)n * 24], 24 * sizeof(double));
    return 1;
}

/* the frame as the library plans it: check_frame, fill_params under C2RT_DEBUG_CULL = debug_cull, and the VoidCull /
 * SphereCull of the pre-pass with every flags word ANDed with void_mask / sphere_mask */
size_t c2rt_plan_frame(const void *plan, const c2rt_camera_frame *cam, const c2rt_render_opts *opts, int debug_cull,
                       uint32_t void_mask, uint32_t sphere_mask, FramePlan *out, int *status, char *msg, size_t msg_len)
{
    const ScenePlan &sp = *static_cast<const ScenePlan *>(plan);
    std::string err;
    std::memset(out, 0, sizeof *out);
    *status = check_frame(cam, opts, err);
    put(msg, msg_len, err);
    if (*status != C2RT_OK) return sizeof *out;
    DiagKnobs knobs;
    knobs.debug_cull = debug_cull;
    RenderParams p;
    fill_params(sp, DeviceTables(), knobs, cam, opts, p);
    out->n_cull = p.n_cull;
    out->n_cull_lights = p.n_cull_lights;
    out->ground_node = p.ground_node;
    out->row_group_start = p.row_group_start;
    out->force_exact = p.force_exact;
    std::memcpy(out->cull_rect, p.cull_rect, sizeof p.cull_rect);
    std::memcpy(out->cull_hull, p.cull_hull, sizeof p.cull_hull);
    std::memcpy(out->light_side, p.light_side, sizeof p.light_side);
    out->v = void_cull_of(sp, p, void_mask);
    out->s = sphere_cull_of(sp, knobs, p, sphere_mask);
    return sizeof *out;
}

} /* extern "C" */
