/*
 * scene_update_check.cpp — host build of the pose-and-replan step behind c2rt_update_scene and c2rt_render_frames_posed
 * (chess2rt_amd/csrc/scene_plan.cpp: SceneCopy, update_scene_plan) for tests/test_scene_update_plan.py: a description is
 * planned and copied as an upload does, poses are applied to it as an update does, and the whole ScenePlan is handed
 * back as bytes — next to the bytes of plan_scene on any description, the yardstick.  Built without ROCm on the include
 * path (Makefile).  Nothing here plans or patches anything itself.
 */
#include <cstdio>
#include <cstring>

#include "../chess2rt_amd/csrc/scene_plan.h"

using namespace c2rt;

namespace {

struct Uploaded {
    SceneCopy scene;
    ScenePlan plan;
};

void put(char *msg, size_t len, const std::string &err)
{
    if (msg && len) std::snprintf(msg, len, "%s", err.c_str());
}

struct Blob {
    std::vector<unsigned char> bytes;
    /* a section: its name (8 bytes, zero padded), its size, its bytes */
    void section(const char *name, const void *data, size_t n)
    {
        char tag[8] = {0};
        std::snprintf(tag, sizeof tag, "%s", name);
        const uint64_t size = n;
        bytes.insert(bytes.end(), tag, tag + 8);
        bytes.insert(bytes.end(), reinterpret_cast<const unsigned char *>(&size), reinterpret_cast<const unsigned char *>(&size) + 8);
        if (n) bytes.insert(bytes.end(), static_cast<const unsigned char *>(data), static_cast<const unsigned char *>(data) + n);
    }
    template <typename T>
    void table(const char *name, const std::vector<T> &v) { section(name, v.data(), v.size() * sizeof(T)); }
    template <typename T>
    void scalar(const char *name, const T &v) { section(name, &v, sizeof v); }
};

/* every table and every scalar fact of a ScenePlan (scene_plan.h), in the order of the struct's members; the records
 * are memset before they are filled (scene_plan.cpp), VoidNode and SphereNode have no padding: the bytes are defined */
void serialise(const ScenePlan &p, Blob &b)
{
    b.table("geoms", p.geoms);
    b.table("nodes", p.nodes);
    b.table("shaders", p.shaders);
    b.table("textur", p.textures);
    b.table("lights", p.lights);
    b.table("texels4", p.texels4);
    b.table("rects", p.shadow_rects);
    b.scalar("levels", p.csg_levels);
    b.scalar("n_nodes", p.n_nodes);
    b.scalar("n_light", p.n_lights);
    b.section("ambient", p.ambient, sizeof p.ambient);
    b.scalar("depth", p.max_trace_depth);
    b.scalar("planes", p.planes_only);
    b.scalar("ident", p.all_identity);
    b.scalar("ground", p.ground_node);
    b.scalar("groundy", p.ground_y);
    b.table("box", p.node_box);
    b.table("boxed", p.node_boxed);
    b.table("lpos", p.light_pos);
    b.table("voids", p.void_nodes);
    b.table("spheres", p.sphere_nodes);
}

size_t hand_over(const Blob &b, unsigned char *out, size_t cap)
{
    if (out && cap >= b.bytes.size()) std::memcpy(out, b.bytes.data(), b.bytes.size());
    return b.bytes.size();
}

} // namespace

extern "C" {

/* what an upload keeps: the plan of `s` and the copy of `s`; null (and the reason in msg) when plan_scene refuses */
void *c2rt_upd_new(const c2rt_scene_desc *s, int *status, char *msg, size_t msg_len)
{
    Uploaded *u = new Uploaded();
    std::string err;
    *status = plan_scene(s, u->plan, err);
    put(msg, msg_len, err);
    if (*status != C2RT_OK) { delete u; return nullptr; }
    u->scene.assign(s);
    return u;
}

void c2rt_upd_free(void *u) { delete static_cast<Uploaded *>(u); }

/* what c2rt_update_scene does on the host */
int c2rt_upd_apply(void *u, const c2rt_scene_pose *pose, char *msg, size_t msg_len)
{
    Uploaded *up = static_cast<Uploaded *>(u);
    std::string err;
    const int st = update_scene_plan(up->scene, up->plan, pose, err);
    put(msg, msg_len, err);
    return st;
}

/* what a frame of c2rt_render_frames_posed does on the host: the pose applied, planned (without texels4) and put back;
 * the frame's plan as bytes */
size_t c2rt_upd_frame_plan_bytes(void *u, const c2rt_scene_pose *pose, int *status, char *msg, size_t msg_len, unsigned char *out, size_t cap)
{
    Uploaded *up = static_cast<Uploaded *>(u);
    std::string err;
    *status = check_scene_pose(up->scene, pose, err);
    ScenePlan frame;
    if (*status == C2RT_OK) {
        PoseUndo undo;
        pose_scene(up->scene, pose, undo);
        *status = replan_scene(up->scene, frame, err);
        unpose_scene(up->scene, pose, undo);
    }
    put(msg, msg_len, err);
    if (*status != C2RT_OK) return 0;
    Blob b;
    serialise(frame, b);
    return hand_over(b, out, cap);
}

/* the plan the handle holds now, as bytes; returns the size (nothing is written when cap is too small) */
size_t c2rt_upd_plan_bytes(const void *u, unsigned char *out, size_t cap)
{
    Blob b;
    serialise(static_cast<const Uploaded *>(u)->plan, b);
    return hand_over(b, out, cap);
}

/* the yardstick: plan_scene(s), as bytes; 0 and the reason in msg when it refuses */
size_t c2rt_upd_fresh_plan_bytes(const c2rt_scene_desc *s, int *status, char *msg, size_t msg_len, unsigned char *out, size_t cap)
{
    ScenePlan plan;
    std::string err;
    *status = plan_scene(s, plan, err);
    put(msg, msg_len, err);
    if (*status != C2RT_OK) return 0;
    Blob b;
    serialise(plan, b);
    return hand_over(b, out, cap);
}

} /* extern "C" */
