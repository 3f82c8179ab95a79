/*
 * scene_plan.h — what the kernels are allowed to skip, decided on the host without a device: the validation of a
 * c2rt_scene_desc and its packing into the device tables (plan_scene), and the per-frame parameter block with its
 * culling rectangles, hulls, light sides and pre-pass tests (fill_params, void_cull_of, sphere_cull_of).
 *
 * This unit includes c2rt_device.h and the standard library only: no device runtime, no context, no environment.
 * c2rt_api.cpp uploads what it plans; tests/scene_plan_check.cpp builds it for the CPU tests, which hold it to the
 * Python restatements (scripts/csg_void_tiles.py, scripts/sphere_cull_tiles.py).
 */
#ifndef C2RT_SCENE_PLAN_H
#define C2RT_SCENE_PLAN_H

#include <cstdint>
#include <string>
#include <vector>

#include "c2rt_device.h"

namespace c2rt {

/* Everything derived from a c2rt_scene_desc: the packed tables as they are uploaded, and the host-side facts the
 * frames are planned from. */
struct ScenePlan {
    std::vector<DevGeom> geoms;
    std::vector<DevNode> nodes;
    std::vector<DevShader> shaders;
    std::vector<DevTex> textures;
    std::vector<DevLight> lights;
    std::vector<float> texels4;        /* float4 per texel (rgb, pad) */
    std::vector<double> shadow_rects;  /* [kMaxCullNodes][4]: RenderParams::shadow_rects */

    int csg_levels = 0;
    uint32_t n_nodes = 0, n_lights = 0;
    float ambient[3] = {0, 0, 0};
    uint32_t max_trace_depth = 0;
    uint32_t planes_only = 0;          /* every node is an axis plane (kNodeAxisPlane) */
    uint32_t all_identity = 0;         /* every node has kNodeIdentityMatrix */
    int32_t ground_node = -1;          /* see RenderParams::ground_node */
    double ground_y = 0;
    /* world-space corners of every node's padded bounding box (for the per-frame
     * screen rectangles); node_boxed[n] = 0: unbounded, never culled */
    std::vector<double> node_box;      /* [n_nodes][8][3] */
    std::vector<uint8_t> node_boxed;
    std::vector<double> light_pos;     /* [n_lights][3]: the per-frame shadow-cull thresholds */
    /* CsgDiff(primitive, Sphere) nodes under an identity matrix (translation allowed): the per-tile void test of the
     * mask pre-pass (csg_void.h); VoidNode::r2 holds R here, the frame's margin is applied in void_cull_of */
    std::vector<VoidNode> void_nodes;
    /* Sphere nodes under an identity matrix the pre-pass may drop from tiles outside their silhouette (csg_void.h);
     * SphereNode::rp holds R here, the frame's margin is applied in sphere_cull_of */
    std::vector<SphereNode> sphere_nodes;
    /* the dark-tile test's table (csg_void.h): the nodes whose shadow may make a primary-ground tile dark, margins
     * applied; a scene table like shadow_rects (uploaded, refreshed by c2rt_update_scene); n = 0: none */
    DarkCull dark{};
};

/* The refusals that look at the description's header and table pointers only (null scene, ABI version, GI, a null
 * table with a non-zero count, too many geometries); plan_scene starts with it. */
int check_scene_desc(const c2rt_scene_desc *s, std::string &err);

/* Validates `s` and derives its ScenePlan.  C2RT_OK: `plan` holds the new scene.  Anything else: the status, the
 * reason in `err`, and `plan` untouched. */
int plan_scene(const c2rt_scene_desc *s, ScenePlan &plan, std::string &err);

/* clears kCsgCertain (c2rt_device.h) in every record of `plan`: the diagnostics switch that leaves every CsgOp to the
 * literal evaluation */
void drop_csg_certain(ScenePlan &plan);
/* clears kNodeCsgTile (c2rt_device.h) in every node of `plan`: the diagnostics switch that leaves every tile with the
 * ground and a leaf CsgOp node to the general path */
void drop_csg_tile(ScenePlan &plan);

/* ---- posing an uploaded scene (c2rt_update_scene, c2rt_render_frames_posed) ---- */

/* A deep copy of a planned description without its texels: `desc` points into the vectors (texels null, n_texels
 * kept for the textures' range check).  What a pose patches — node_transform, light_pos, light_color, light_power —
 * is patched here, and the plan is derived from it again by the planner itself. */
struct SceneCopy {
    c2rt_scene_desc desc{};
    std::vector<int32_t> geom_type, geom_child, tex_type, shader_type, shader_texture, light_type, node_geom, node_shader;
    std::vector<double> geom_param, tex_param, shader_exponent, light_pos, node_transform;
    std::vector<float> tex_color, tex_scaling, shader_color, shader_strength, light_color, light_power;
    std::vector<uint32_t> tex_width, tex_height;
    std::vector<uint64_t> tex_offset;

    SceneCopy() = default;
    SceneCopy(const SceneCopy &) = delete;
    SceneCopy &operator=(const SceneCopy &) = delete;
    /* `s` has passed check_scene_desc */
    void assign(const c2rt_scene_desc *s);
};

/* Why `pose` cannot be applied to `scene`, in the documented order (c2rt.h); C2RT_OK otherwise.  Reads the pose's
 * counts, pointers and indices only. */
int check_scene_pose(const SceneCopy &scene, const c2rt_scene_pose *pose, std::string &err);

/* plan_scene(&scene.desc) with the texel conversion skipped: plan.texels4 comes out empty, everything else is what
 * plan_scene derives. */
int replan_scene(const SceneCopy &scene, ScenePlan &plan, std::string &err);

/* What a pose overwrites in a SceneCopy, saved so that it can be put back (pose_scene / unpose_scene: a refused
 * update, a frame of a posed batch). */
struct PoseUndo {
    std::vector<double> node_transform, light_pos;
    std::vector<float> light_color, light_power;
};
/* Applies a checked pose to `scene` in the order its entries are listed, remembering what it overwrote. */
void pose_scene(SceneCopy &scene, const c2rt_scene_pose *pose, PoseUndo &undo);
void unpose_scene(SceneCopy &scene, const c2rt_scene_pose *pose, const PoseUndo &undo);

/* The whole step behind c2rt_update_scene: check, patch, plan again.  C2RT_OK: `scene` is the patched description and
 * `plan` its plan, with the texels4 it had (moved, not converted again).  Anything else: the status, the reason in
 * `err`, `scene` and `plan` as they were. */
int update_scene_plan(SceneCopy &scene, ScenePlan &plan, const c2rt_scene_pose *pose, std::string &err);

/* where the uploaded tables of a ScenePlan live (device pointers; the planner only copies them into RenderParams) */
struct DeviceTables {
    DevGeom *geoms = nullptr;
    DevNode *nodes = nullptr;
    DevShader *shaders = nullptr;
    DevTex *textures = nullptr;
    DevLight *lights = nullptr;
    float *texels = nullptr;
    double *shadow_rects = nullptr;    /* [kMaxCullNodes][4] */
    DarkCull *dark = nullptr;          /* ScenePlan::dark */
    uint32_t *tile_stats = nullptr;    /* diagnostics (c2rt_debug_set_tile_stats): caller-owned device buffer */
};

/* The diagnostics switches (A/B measurement and test knobs), all off in the product library.  Whoever owns an
 * environment fills them; the planner reads none. */
struct DiagKnobs {
    bool exact = false;                /* C2RT_EXACT=1: every tile through exact:: */
    /* C2RT_DEBUG_CULL (frames are unchanged by construction, slower): bit 0: no culling rectangles at all; bit 1: no
     * ground-plane refinement of the shadow mask; bit 2: no view-pyramid culling of shadow rays; bit 3: no
     * sphere-silhouette test in the mask pre-pass; bit 4: no ground-tile path (RenderParams::ground_fast stays 0); bit 5: no
     * dark-tile test in the mask pre-pass (dark_cull_of); bit 6: no short-chain ground tiles (RenderParams::ground_certain_cq
     * stays 0); bit 7: no sphere-interior tiles (SphereCull::interior stays 0); bit 8: sphere-interior
     * tiles whatever the frame's size (sphere_cull_of: kSphereTileMinSamples); bit 9: no CsgOp decided by csg_certain.h
     * (drop_csg_certain on every plan: a switch of the scene's tables, not of a frame); bit 10: no ground-and-CsgOp tiles
     * through lean::csg_tile (drop_csg_tile on every plan, likewise) */
    int debug_cull = 0;
    int csg_first_cap = 0;             /* C2RT_CSG_FIRST_CAP=<entries>: the first pass's hit-stack capacity */
};

uint32_t strip_h(const c2rt_render_opts *o);
uint32_t local_rows_of(const c2rt_render_opts *o, uint32_t rank);
/* why (cam, o), both non-null, cannot be rendered whatever the scene: the reason in `err`; C2RT_OK otherwise */
int check_frame(const c2rt_camera_frame *cam, const c2rt_render_opts *o, std::string &err);

bool hull_half_planes(const double pts[8][2], double pad, double out[kHullEdges][3]);
void cull_rect_of(const c2rt_camera_frame *cam, const double *corners, int32_t out[4], float hull[kHullEdges][3]);
void light_side_of(const c2rt_camera_frame *cam, const double *light, int32_t out[8]);

/* the frame's parameter block up to what a launch adds (output, counters, hit-stack capacity, mask table, retry list) */
void fill_params(const ScenePlan &plan, const DeviceTables &dev, const DiagKnobs &knobs, const c2rt_camera_frame *cam,
                 const c2rt_render_opts *o, RenderParams &p);
VoidCull void_cull_of(const ScenePlan &plan, const RenderParams &p, uint32_t flags_mask);
SphereCull sphere_cull_of(const ScenePlan &plan, const DiagKnobs &knobs, const RenderParams &p, uint32_t flags_mask);
bool dark_frame_ok(const ScenePlan &plan, const DiagKnobs &knobs, const RenderParams &p);
DarkCull dark_cull_of(const ScenePlan &plan, const DiagKnobs &knobs, const RenderParams &p);
KernelVariant variant_of(const ScenePlan &plan, const c2rt_camera_frame *cam);

} // namespace c2rt
#endif
