// scene_update_replay.cpp — stand-alone replay of the scene-update CPU cases (moves, NaN / infinity, lights, posed frames, every
// refusal) on a lecture5-like description built by hand, for a sanitizer run on the CPU:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/replay \
//       tests/scene_update_replay.cpp tests/scene_update_check.cpp chess2rt_amd/csrc/scene_plan.cpp && /tmp/replay
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../include/c2rt.h"
extern "C" {
void *c2rt_upd_new(const c2rt_scene_desc *, int *, char *, size_t);
void c2rt_upd_free(void *);
int c2rt_upd_apply(void *, const c2rt_scene_pose *, char *, size_t);
size_t c2rt_upd_plan_bytes(const void *, unsigned char *, size_t);
size_t c2rt_upd_fresh_plan_bytes(const c2rt_scene_desc *, int *, char *, size_t, unsigned char *, size_t);
size_t c2rt_upd_frame_plan_bytes(void *, const c2rt_scene_pose *, int *, char *, size_t, unsigned char *, size_t);
}
static void ident(double *t) { std::memset(t, 0, 30 * sizeof(double)); for (int k = 0; k < 3; ++k) t[9 * k] = t[9 * k + 4] = t[9 * k + 8] = 1; }
int main()
{
    const int G = 6, N = 6, L = 3;
    int32_t gt[G] = {0, 1, 2, 1, 5, 1}, gc[2 * G] = {-1, -1, -1, -1, -1, -1, -1, -1, 2, 3, -1, -1};
    double gp[4 * G] = {-0.01, NAN, 0, 0, 100, 50, 320, 50, -100, 60, 200, 100, -100, 60, 200, 70, 0, 0, 0, 0, 0, 0, 0, 15};
    int32_t st[1] = {0}, stex[1] = {-1}; float scol[3] = {.5f, .5f, .5f}, sstr[1] = {1}; double sexp[1] = {16};
    int32_t lt[L] = {0, 0, 0}; double lp[3 * L] = {-90, 700, 350, 200, 400, -50, 0, 300, 500}; float lc[3 * L] = {1, 1, 1, 1, 1, 1, 1, 1, 1}, lw[L] = {8e5f, 3e5f, 2e5f};
    int32_t ng[N] = {0, 1, 4, 5, 5, 5}, ns[N] = {0, 0, 0, 0, 0, 0};
    std::vector<double> xf(30 * N);
    for (int n = 0; n < N; ++n) ident(&xf[30 * n]);
    xf[30 * 3 + 27] = 100; xf[30 * 3 + 28] = 15; xf[30 * 3 + 29] = 256;
    c2rt_scene_desc d; std::memset(&d, 0, sizeof d);
    d.abi_version = C2RT_ABI_VERSION; d.n_geoms = G; d.geom_type = gt; d.geom_param = gp; d.geom_child = gc;
    d.n_shaders = 1; d.shader_type = st; d.shader_color = scol; d.shader_texture = stex; d.shader_exponent = sexp; d.shader_strength = sstr;
    d.n_lights = L; d.light_type = lt; d.light_pos = lp; d.light_color = lc; d.light_power = lw;
    d.n_nodes = N; d.node_geom = ng; d.node_shader = ns; d.node_transform = xf.data();
    d.ambient[0] = d.ambient[1] = d.ambient[2] = .2f; d.max_trace_depth = 4;
    int status; char msg[512];
    void *u = c2rt_upd_new(&d, &status, msg, sizeof msg);
    assert(u && status == 0);
    std::vector<unsigned char> a(1 << 20), b(1 << 20);
    auto same = [&]() { size_t x = c2rt_upd_plan_bytes(u, a.data(), a.size()); size_t y = c2rt_upd_fresh_plan_bytes(&d, &status, msg, sizeof msg, b.data(), b.size()); assert(status == 0 && x == y && x <= a.size() && !std::memcmp(a.data(), b.data(), x)); };
    same();
    // sequences: node moves (translate, scale, NaN, inf, back), light moves / values
    double t[60]; uint32_t idx[2];
    auto node_pose = [&](uint32_t n, const double *tr) { c2rt_scene_pose p; std::memset(&p, 0, sizeof p); idx[0] = n; p.n_nodes = 1; p.node_index = idx; p.node_transform = tr; std::memcpy(&xf[30 * n], tr, 30 * sizeof(double)); int s = c2rt_upd_apply(u, &p, msg, sizeof msg); assert(s == 0); same(); };
    for (uint32_t n : {1u, 0u, 2u, 3u}) {
        ident(t); t[27] = -30; t[28] = 10; t[29] = -40; node_pose(n, t);
        ident(t); t[0] = 1.5; t[9] = 1 / 1.5; t[18] = 1 / 1.5; node_pose(n, t);
        ident(t); t[4] = NAN; node_pose(n, t);
        ident(t); t[28] = INFINITY; node_pose(n, t);
        ident(t); node_pose(n, t);
    }
    auto light_pose = [&](uint32_t l, const double *pos, const float *col, const float *pw) { c2rt_scene_pose p; std::memset(&p, 0, sizeof p); idx[0] = l; p.n_lights = 1; p.light_index = idx; p.light_pos = pos; p.light_color = col; p.light_power = pw;
        if (pos) std::memcpy(&lp[3 * l], pos, 24); if (col) std::memcpy(&lc[3 * l], col, 12); if (pw) lw[l] = *pw;
        // a posed frame plans and puts back: plan unchanged
        size_t x = c2rt_upd_plan_bytes(u, a.data(), a.size()); std::vector<unsigned char> keep(a.begin(), a.begin() + x), f(1 << 20);
        c2rt_upd_frame_plan_bytes(u, &p, &status, msg, sizeof msg, f.data(), f.size()); assert(status == 0);
        size_t y = c2rt_upd_plan_bytes(u, a.data(), a.size()); assert(x == y && !std::memcmp(a.data(), keep.data(), x));
        int s = c2rt_upd_apply(u, &p, msg, sizeof msg); assert(s == 0); same(); };
    const double side[3] = {150, 700, 100}, below[3] = {-90, -50, 350}, on[3] = {-90, -0.01, 350}, two[3] = {-200, 350, 100};
    const float zero = 0, big[3] = {0x1p70f, 1, 1}, one = 1;
    light_pose(0, side, nullptr, nullptr); light_pose(0, below, nullptr, nullptr); light_pose(0, on, nullptr, nullptr);
    light_pose(2, two, nullptr, nullptr); light_pose(0, nullptr, nullptr, &zero); light_pose(0, nullptr, big, &one);
    // refusals: status 1, plan unchanged
    size_t x = c2rt_upd_plan_bytes(u, a.data(), a.size()); std::vector<unsigned char> keep(a.begin(), a.begin() + x);
    auto refused = [&](const c2rt_scene_pose *p) { int s = c2rt_upd_apply(u, p, msg, sizeof msg); assert(s == C2RT_ERR_INVALID_ARG && msg[0]); size_t y = c2rt_upd_plan_bytes(u, a.data(), a.size()); assert(x == y && !std::memcmp(a.data(), keep.data(), x)); };
    c2rt_scene_pose p; ident(t); ident(t + 30);
    refused(nullptr);
    std::memset(&p, 0, sizeof p); p.n_nodes = 1; p.node_transform = t; refused(&p);
    std::memset(&p, 0, sizeof p); p.n_lights = 1; p.light_pos = side; refused(&p);
    std::memset(&p, 0, sizeof p); idx[0] = 0; p.n_nodes = 1; p.node_index = idx; refused(&p);
    std::memset(&p, 0, sizeof p); p.n_lights = 1; p.light_index = idx; refused(&p);
    std::memset(&p, 0, sizeof p); idx[0] = 2; idx[1] = 6; p.n_nodes = 2; p.node_index = idx; p.node_transform = t; refused(&p);
    idx[1] = 2; refused(&p);
    std::memset(&p, 0, sizeof p); idx[0] = 3; p.n_lights = 1; p.light_index = idx; p.light_pos = side; refused(&p);
    std::memset(&p, 0, sizeof p); assert(c2rt_upd_apply(u, &p, msg, sizeof msg) == 0);
    c2rt_upd_free(u);
    std::puts("sanitized replay ok");
    return 0;
}
