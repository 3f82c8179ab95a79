/*
 * scene_plan.cpp — scene validation and packing (plan_scene) and per-frame planning (fill_params and the pre-pass
 * tests) on the host, without a device: see scene_plan.h.  Built without contraction, like everything that restates
 * the reference's arithmetic.
 */
#include "scene_plan.h"
#include "ground_certain.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <utility>

namespace c2rt {
namespace {

int fail(std::string &err, int status, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return status;
}

bool is_csg(int t) { return t == C2RT_GEOM_CSG_UNION || t == C2RT_GEOM_CSG_INTER || t == C2RT_GEOM_CSG_DIFF; }

/* nesting depth of the CsgOp tree under `g` (0 for primitives); -1 on a cycle
 * or an out-of-range child */
int csg_depth(const c2rt_scene_desc *s, int32_t g, std::vector<int> &state, std::vector<int> &memo)
{
    if (g < 0 || (uint32_t)g >= s->n_geoms) return -1;
    if (state[g] == 1) return -1; /* on the current path: cycle */
    if (state[g] == 2) return memo[g];
    int d = 0;
    if (is_csg(s->geom_type[g])) {
        state[g] = 1;
        const int l = csg_depth(s, s->geom_child[2 * g + 0], state, memo);
        const int r = csg_depth(s, s->geom_child[2 * g + 1], state, memo);
        if (l < 0 || r < 0) return -1;
        d = 1 + (l > r ? l : r);
    }
    state[g] = 2;
    memo[g] = d;
    return d;
}

/* ---- conservative bounds and exact CSG shortcuts (see c2rt_device.h) ---- */
struct BoundInfo { bool done = false, bounded = false; double c[3] = {0, 0, 0}, r = 0; };

bool subtree_has_leaf(const c2rt_scene_desc *s, int32_t g, int32_t leaf)
{
    if (!is_csg(s->geom_type[g])) return g == leaf;
    return subtree_has_leaf(s, s->geom_child[2 * g], leaf) || subtree_has_leaf(s, s->geom_child[2 * g + 1], leaf);
}

BoundInfo enclose(const BoundInfo &a, const BoundInfo &b)
{
    BoundInfo o;
    o.done = true;
    if (!a.bounded || !b.bounded) return o;
    const double d = std::sqrt((a.c[0] - b.c[0]) * (a.c[0] - b.c[0]) + (a.c[1] - b.c[1]) * (a.c[1] - b.c[1]) + (a.c[2] - b.c[2]) * (a.c[2] - b.c[2]));
    o.bounded = true;
    for (int i = 0; i < 3; ++i) o.c[i] = a.c[i]; /* keep a's centre: simple and conservative */
    o.r = std::fmax(a.r, d + b.r);
    return o;
}

/* kCsgCertain: the CsgOp over children l and r lies in the domain csg_certain.h's bounds were derived for — two DISTINCT
 * primitives (the walk tells the lists apart by leaf identity: Op(a, a) is another walk), each a Sphere or a Cube with
 * finite parameters, every centre coordinate within 2^20 and the radius / side in [2^-10, 2^20].  A Plane child, a
 * nested child, a non-finite or degenerate primitive or geometry beyond that scale leave the flag off. */
bool csg_certain_ok(const c2rt_scene_desc *s, int32_t l, int32_t r)
{
    if (l == r) return false;
    for (const int32_t c : {l, r}) {
        const int t = s->geom_type[c];
        if (t != C2RT_GEOM_SPHERE && t != C2RT_GEOM_CUBE) return false;
        const double *p = s->geom_param + 4 * (size_t)c;
        for (int i = 0; i < 3; ++i)
            if (!(std::fabs(p[i]) <= 0x1p20)) return false;
        if (!(p[3] >= 0x1p-10 && p[3] <= 0x1p20)) return false;
    }
    return true;
}

/* geometries must already be validated acyclic (csg_depth) */
BoundInfo bound_of(const c2rt_scene_desc *s, int32_t g, std::vector<BoundInfo> &memo, std::vector<DevGeom> &geoms)
{
    if (memo[g].done) return memo[g];
    BoundInfo b;
    b.done = true;
    const int t = s->geom_type[g];
    const double *p = s->geom_param + 4 * (size_t)g;
    if (t == C2RT_GEOM_SPHERE) {
        b.bounded = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(p[3]);
        for (int i = 0; i < 3; ++i) b.c[i] = p[i];
        b.r = std::fabs(p[3]);
    } else if (t == C2RT_GEOM_CUBE) {
        b.bounded = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(p[3]);
        for (int i = 0; i < 3; ++i) b.c[i] = p[i];
        b.r = std::fabs(p[3]) * 0.5 * 1.7320508075688774; /* half diagonal */
    } else if (is_csg(t)) {
        const int32_t l = s->geom_child[2 * g], r = s->geom_child[2 * g + 1];
        const BoundInfo bl = bound_of(s, l, memo, geoms), br = bound_of(s, r, memo, geoms);
        const bool shortA = t != C2RT_GEOM_CSG_UNION && !subtree_has_leaf(s, r, l);
        const bool shortB = t == C2RT_GEOM_CSG_INTER && !is_csg(s->geom_type[l]);
        if (shortA) geoms[g].flags |= kCsgShortA;
        if (shortB) geoms[g].flags |= kCsgShortB;
        if (csg_certain_ok(s, l, r)) geoms[g].flags |= kCsgCertain;
        if (shortA && bl.bounded) b = bl;       /* nothing on the left => false */
        else b = enclose(bl, br);               /* nothing on either side => false */
        b.done = true;
    } /* plane: unbounded */
    if (b.bounded) {
        /* pad: the reject test runs in fp64 on coordinates of this magnitude */
        const double mag = std::fabs(b.c[0]) + std::fabs(b.c[1]) + std::fabs(b.c[2]) + b.r;
        const double rp = b.r * (1 + 1e-6) + 1e-6 * mag + 1e-9;
        if (std::isfinite(rp) && rp * rp < 1e300) {
            geoms[g].flags |= kGeomBounded;
            geoms[g].bound[0] = b.c[0];
            geoms[g].bound[1] = b.c[1];
            geoms[g].bound[2] = b.c[2];
            geoms[g].bound[3] = rp * rp;
        }
    }
    memo[g] = b;
    return b;
}

/* Object-space axis-aligned box with the same contract as the bounding sphere above — a ray
 * (segment) that does not enter it cannot make Geometry.intersect return true — but tight: the
 * sphere's own box, the cube itself, the left child's box for an Inter/Diff with shortcut A
 * (no left hit => false; left hits beyond the segment put the winner beyond it too), the hull of
 * both children otherwise.  It feeds the per-frame screen rectangles and the shadow rectangles,
 * where the bounding sphere of a cube costs a factor 1.7 per axis.  Call after bound_of (flags). */
struct BoxInfo { bool done = false, bounded = false; double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}; };

BoxInfo box_of(const c2rt_scene_desc *s, int32_t g, std::vector<BoxInfo> &memo, const std::vector<DevGeom> &geoms)
{
    if (memo[g].done) return memo[g];
    BoxInfo b;
    b.done = true;
    const int t = s->geom_type[g];
    const double *p = s->geom_param + 4 * (size_t)g;
    if (t == C2RT_GEOM_SPHERE || t == C2RT_GEOM_CUBE) {
        b.bounded = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(p[3]);
        const double e = t == C2RT_GEOM_SPHERE ? std::fabs(p[3]) : std::fabs(p[3]) * 0.5;
        for (int i = 0; i < 3; ++i) { b.lo[i] = p[i] - e; b.hi[i] = p[i] + e; }
    } else if (is_csg(t)) {
        const BoxInfo bl = box_of(s, s->geom_child[2 * g], memo, geoms), br = box_of(s, s->geom_child[2 * g + 1], memo, geoms);
        /* Where can a HIT of this CsgOp lie?  On a leaf's surface of either subtree, in general: the union.  Inside
         * the left child's box only when the walk's `inL` really means "inside the left child": the left child is a
         * PRIMITIVE (its entries carry its own identity, so they and only they toggle inL — kCsgShortA excludes the
         * same leaf inside the right subtree) and the operator needs inL (Inter / Diff).  With a CsgOp as left child
         * no entry ever equals `left` (rt/geometry.d:314-317 compares the LEAF): inL is the parity of the left
         * list for the whole walk, and an Inter / Diff can come out "in" at an entry of the RIGHT child far outside
         * the left child's box — e.g. a shadow ray whose left hits lie beyond the light, occluded by a right-child
         * surface in front of it.  (Found by the offline sweep, seed 108921: three pixels of a 64x48 frame lost a
         * shadow to the view-pyramid culling of shadow rays, which asks where the occluder can BE.) */
        if ((geoms[g].flags & kCsgShortA) && bl.bounded && !is_csg(s->geom_type[s->geom_child[2 * g]])) {
            b = bl;
        } else if (bl.bounded && br.bounded) {
            b.bounded = true;
            for (int i = 0; i < 3; ++i) { b.lo[i] = std::min(bl.lo[i], br.lo[i]); b.hi[i] = std::max(bl.hi[i], br.hi[i]); }
        }
        b.done = true;
    } /* plane: unbounded */
    memo[g] = b;
    return b;
}

/* ---- plan_scene, step by step; each step reads what the steps before it left in `p` ---- */
int plan_geoms(const c2rt_scene_desc *s, ScenePlan &p, std::string &err)
{
    std::vector<DevGeom> &geoms = p.geoms;
    geoms.resize(s->n_geoms);
    for (uint32_t g = 0; g < s->n_geoms; ++g) {
        const int t = s->geom_type[g];
        if (t < C2RT_GEOM_PLANE || t > C2RT_GEOM_CSG_DIFF) return fail(err, C2RT_ERR_UNSUPPORTED, "geometry %u: unknown type %d", g, t);
        DevGeom &d = geoms[g];
        std::memset(&d, 0, sizeof d);
        d.type = t;
        d.left = is_csg(t) ? s->geom_child[2 * g + 0] : -1;
        d.right = is_csg(t) ? s->geom_child[2 * g + 1] : -1;
        for (int i = 0; i < 4; ++i) d.p[i] = s->geom_param[4 * g + i];
        if (t == C2RT_GEOM_CUBE) {
            const double halfSide = d.p[3] * 0.5;
            for (int i = 0; i < 3; ++i) {
                d.q[i] = d.p[i] + -1 * halfSide;     /* center + side * halfSide, side = -1 (== center - halfSide) */
                d.q[3 + i] = d.p[i] + 1 * halfSide;
            }
        } else if (t == C2RT_GEOM_SPHERE) {
            d.q[0] = d.p[3] * d.p[3];
        }
        bool finite = true;
        for (int i = 0; i < 4; ++i) finite = finite && std::isfinite(d.p[i]);
        for (int i = 0; i < 6; ++i) finite = finite && std::isfinite(d.q[i]);
        if (finite && !is_csg(t)) d.flags |= kGeomFinite;
    }
    return C2RT_OK;
}

/* textures: texel pool repacked to float4 (with_texels = false, a replan of a posed scene: the pool is not read and
 * texels4 stays empty) */
int plan_textures(const c2rt_scene_desc *s, ScenePlan &p, std::string &err, bool with_texels)
{
    std::vector<DevTex> &textures = p.textures;
    textures.resize(s->n_textures);
    for (uint32_t t = 0; t < s->n_textures; ++t) {
        const int ty = s->tex_type[t];
        if (ty < C2RT_TEX_CHECKER || ty > C2RT_TEX_BITMAP) return fail(err, C2RT_ERR_UNSUPPORTED, "texture %u: unknown type %d", t, ty);
        DevTex &d = textures[t];
        std::memset(&d, 0, sizeof d);
        d.type = ty;
        d.scaling = s->tex_scaling[t];
        for (int i = 0; i < 18; ++i) d.color[i] = s->tex_color[18 * t + i];
        for (int i = 0; i < 6; ++i) d.param[i] = s->tex_param[6 * t + i];
        if (ty == C2RT_TEX_BITMAP) {
            d.width = s->tex_width[t];
            d.height = s->tex_height[t];
            d.offset = s->tex_offset[t];
            if ((uint64_t)d.width * d.height + d.offset > s->n_texels)
                return fail(err, C2RT_ERR_INVALID_ARG, "texture %u: texels out of the pool", t);
            if (d.width >= (1u << 24) || d.height >= (1u << 24)) return fail(err, C2RT_ERR_LIMIT, "texture %u too large", t);
        }
    }
    if (!with_texels) return C2RT_OK;
    std::vector<float> &texels4 = p.texels4;
    texels4.resize((size_t)s->n_texels * 4);
    for (uint64_t i = 0; i < s->n_texels; ++i) {
        texels4[4 * i + 0] = s->texels[3 * i + 0];
        texels4[4 * i + 1] = s->texels[3 * i + 1];
        texels4[4 * i + 2] = s->texels[3 * i + 2];
        texels4[4 * i + 3] = 0.0f;
    }
    return C2RT_OK;
}

int plan_shaders(const c2rt_scene_desc *s, ScenePlan &p, std::string &err)
{
    std::vector<DevShader> &shaders = p.shaders;
    shaders.resize(s->n_shaders);
    for (uint32_t i = 0; i < s->n_shaders; ++i) {
        const int ty = s->shader_type[i];
        if (ty != C2RT_SHADER_LAMBERT && ty != C2RT_SHADER_PHONG) return fail(err, C2RT_ERR_UNSUPPORTED, "shader %u: unknown type %d", i, ty);
        DevShader &d = shaders[i];
        std::memset(&d, 0, sizeof d);
        d.type = ty;
        d.tex = s->shader_texture[i];
        if (d.tex >= (int32_t)s->n_textures) return fail(err, C2RT_ERR_INVALID_ARG, "shader %u: texture index %d out of range", i, d.tex);
        if (d.tex < 0) d.tex = -1;
        for (int c = 0; c < 3; ++c) d.color[c] = s->shader_color[3 * i + c];
        d.strength = s->shader_strength[i];
        d.exponent = s->shader_exponent[i];
    }
    return C2RT_OK;
}

int plan_lights(const c2rt_scene_desc *s, ScenePlan &p, std::string &err)
{
    std::vector<DevLight> &lights = p.lights;
    lights.resize(s->n_lights);
    for (uint32_t i = 0; i < s->n_lights; ++i) {
        if (s->light_type[i] != C2RT_LIGHT_POINT) return fail(err, C2RT_ERR_UNSUPPORTED, "light %u: unknown type %d", i, s->light_type[i]);
        DevLight &d = lights[i];
        std::memset(&d, 0, sizeof d);
        for (int c = 0; c < 3; ++c) d.pos[c] = s->light_pos[3 * i + c];
        /* Light.color(): lightColor * lightPower — rt/light.d:11-14 */
        for (int c = 0; c < 3; ++c) d.color[c] = s->light_color[3 * i + c] * s->light_power[i];
        /* lightColor.intensity() != 0 — rt/shader.d:88, rt/color.d:141-144 */
        const float intensity = (d.color[0] + d.color[1] + d.color[2]) / 3;
        d.lit = intensity != 0 ? 1u : 0u;
        /* bit 1: every channel is +0 or a finite float within 2^+-60 — the numerators of lean::'s fp32 division
         * by the squared distance need no test on the device (c2rt_trace.inc, shade) */
        bool chan_ok = true;
        for (int c = 0; c < 3; ++c) {
            uint32_t bits;
            std::memcpy(&bits, &d.color[c], 4);
            const float a = std::fabs(d.color[c]);
            chan_ok = chan_ok && (bits == 0u || (a >= 0x1p-60f && a < 0x1p60f));
        }
        if (chan_ok) d.lit |= 2u;
        /* equal: bit 1 holds and the three channels are the same bits (`color 1 1 1`: every scene the reference ships) —
         * lean::ground_tile_certain then takes one quotient by the squared distance for all three */
        d.equal = (chan_ok && !std::memcmp(&d.color[0], &d.color[1], 4) && !std::memcmp(&d.color[0], &d.color[2], 4)) ? 1u : 0u;
    }
    p.light_pos.assign(s->light_pos, s->light_pos + 3 * (size_t)s->n_lights);
    return C2RT_OK;
}

/* a Plane under a non-identity matrix: its world normal, the same for every hit (kNodePlaneNormal) */
void plane_world_normal(DevNode &d)
{
    /* hit_surface: normalized(mulvm((0, 1, 0), tinv)), operation for operation (this file is built
     * without contraction; sqrt and division are IEEE on both sides) */
    const double nx = 0.0, ny = 1.0, nz = 0.0;
    const double *m = d.tinv;
    const double vx = nx * m[0] + ny * m[3] + nz * m[6];
    const double vy = nx * m[1] + ny * m[4] + nz * m[7];
    const double vz = nx * m[2] + ny * m[5] + nz * m[8];
    const double sq = vx * vx + vy * vy + vz * vz;
    const double len = std::sqrt(sq);
    const double inv = 1.0 / len;
    const double wn[3] = {vx * inv, vy * inv, vz * inv};
    if (std::isfinite(wn[0]) && std::isfinite(wn[1]) && std::isfinite(wn[2])) {
        d.g.q[0] = wn[0];
        d.g.q[1] = wn[1];
        d.g.q[2] = wn[2];
        d.flags |= kNodePlaneNormal;
    }
}

/* shading inputs of a node in one record */
void flatten_material(const DevShader &sh, const std::vector<DevTex> &textures, DevMat &m)
{
    m.shader_type = sh.type;
    m.tex = sh.tex;
    m.tex_type = sh.tex >= 0 ? textures[sh.tex].type : -1;
    m.strength = sh.strength;
    std::memcpy(m.color, sh.color, sizeof m.color);
    m.exponent = sh.exponent;
    if (m.tex_type == C2RT_TEX_CHECKER) {
        std::memcpy(m.texdata, textures[sh.tex].color, 6 * sizeof(float));
        std::memcpy(m.texdata + 6, &textures[sh.tex].param[0], sizeof(double));
    } else if (m.tex_type == C2RT_TEX_BITMAP) {
        const DevTex &t = textures[sh.tex];
        m.texdata[0] = t.width;
        m.texdata[1] = t.height;
        std::memcpy(m.texdata + 2, &t.scaling, sizeof(float));
        std::memcpy(m.texdata + 4, &t.offset, sizeof(uint64_t));
    }
}

/* nodes: geometry copy with bounds and shortcuts, transform flags, material; the scene's CSG nesting depth */
int plan_nodes(const c2rt_scene_desc *s, ScenePlan &p, std::string &err)
{
    std::vector<DevGeom> &geoms = p.geoms;
    std::vector<DevNode> &nodes = p.nodes;
    nodes.resize(s->n_nodes);
    std::vector<int> state(s->n_geoms, 0), memo(s->n_geoms, 0);
    std::vector<BoundInfo> bounds(s->n_geoms);
    int levels = 0;
    for (uint32_t n = 0; n < s->n_nodes; ++n) {
        DevNode &d = nodes[n];
        std::memset(&d, 0, sizeof d);
        d.geom = s->node_geom[n];
        d.shader = s->node_shader[n];
        if (d.shader < 0 || (uint32_t)d.shader >= s->n_shaders) return fail(err, C2RT_ERR_INVALID_ARG, "node %u: shader index %d out of range", n, d.shader);
        const int depth = csg_depth(s, d.geom, state, memo);
        if (depth < 0) return fail(err, C2RT_ERR_INVALID_ARG, "node %u: geometry index out of range or cyclic CSG", n);
        if (depth > C2RT_MAX_CSG_DEPTH) return fail(err, C2RT_ERR_LIMIT, "node %u: CSG nesting %d > %d", n, depth, C2RT_MAX_CSG_DEPTH);
        if (depth > levels) levels = depth;
        bound_of(s, d.geom, bounds, geoms);
        d.g = geoms[d.geom]; /* after bound_of: carries the flags and the bound */
        const double *t = s->node_transform + 30 * (size_t)n;
        std::memcpy(d.m, t, 9 * sizeof(double));
        std::memcpy(d.inv, t + 9, 9 * sizeof(double));
        std::memcpy(d.tinv, t + 18, 9 * sizeof(double));
        std::memcpy(d.off, t + 27, 3 * sizeof(double));
        static const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        bool ident = true;
        for (int i = 0; i < 9; ++i) ident = ident && d.m[i] == I[i] && d.inv[i] == I[i] && d.tinv[i] == I[i];
        if (ident) d.flags |= kNodeIdentityMatrix;
        if (d.off[0] == 0 && d.off[1] == 0 && d.off[2] == 0) d.flags |= kNodeZeroOffset;
        if (d.g.type == C2RT_GEOM_PLANE && !ident) plane_world_normal(d);
        flatten_material(p.shaders[d.shader], p.textures, d.mat);
    }
    if (levels > 0 && s->n_geoms > C2RT_MAX_CSG_GEOMS)
        return fail(err, C2RT_ERR_LIMIT, "%u geometries in a scene with CsgOps (limit %d)", s->n_geoms, C2RT_MAX_CSG_GEOMS);
    p.csg_levels = levels;
    return C2RT_OK;
}

/* kNodeAxisPlane per node; planes_only and all_identity for the scene */
void plan_node_flags(const c2rt_scene_desc *s, ScenePlan &p)
{
    std::vector<DevNode> &nodes = p.nodes;
    p.planes_only = s->n_nodes > 0;
    for (uint32_t n = 0; n < s->n_nodes; ++n) {
        DevNode &d = nodes[n];
        bool axis = d.g.type == C2RT_GEOM_PLANE;
        if (axis && !(d.flags & kNodeIdentityMatrix)) {
            for (int i = 0; i < 9; ++i) {
                const double a = std::fabs(d.inv[i]);
                axis = axis && (i % 4 == 0 ? (a >= 1e-100 && a <= 1e100) : d.inv[i] == 0.0);
            }
            axis = axis && d.inv[4] > 0;
        }
        if (axis) d.flags |= kNodeAxisPlane;
        else p.planes_only = 0;
    }
    p.all_identity = s->n_nodes > 0;
    for (uint32_t n = 0; n < s->n_nodes; ++n)
        if (!(nodes[n].flags & kNodeIdentityMatrix)) p.all_identity = 0;
}

/* kNodeCsgTile (c2rt_device.h): the nodes lean::csg_tile may render beside the ground.  A scene fact: the frame's part of
 * the condition (a mask table, no depth of field, no stereo, not counted, an eligible floor) is RenderParams::ground_fast. */
void plan_csg_tile_nodes(const c2rt_scene_desc *s, ScenePlan &p)
{
    /* (every node under the identity matrix: the instances that carry the path, launch_render_level's `idn`) */
    if (s->n_lights > 1 || !p.all_identity) return;
    for (uint32_t n = 0; n < s->n_nodes && n < (uint32_t)kMaxCullNodes; ++n) {
        DevNode &d = p.nodes[n];
        const bool leaf = d.g.type >= C2RT_GEOM_CSG_UNION && (d.g.flags & kCsgCertain);
        const bool shader = d.mat.shader_type == C2RT_SHADER_LAMBERT || d.mat.shader_type == C2RT_SHADER_PHONG;
        if (leaf && (d.flags & kNodeIdentityMatrix) && shader && d.mat.tex_type < 0) d.flags |= kNodeCsgTile;
    }
}

void plan_world_boxes(const c2rt_scene_desc *s, ScenePlan &p)
{
    const std::vector<DevGeom> &geoms = p.geoms;
    const std::vector<DevNode> &nodes = p.nodes;
    /* world-space bounding boxes of the nodes: object-space box (box_of), padded -> the 8
     * corners through Transform.point (affine: hull preserved) */
    p.node_box.assign((size_t)s->n_nodes * 24, 0.0);
    p.node_boxed.assign(s->n_nodes, 0);
    std::vector<BoxInfo> boxes(s->n_geoms);
    for (uint32_t n = 0; n < s->n_nodes; ++n) {
        const DevGeom &g = nodes[n].g;
        if (!(g.flags & kGeomBounded)) continue;
        const BoxInfo bx = box_of(s, nodes[n].geom, boxes, geoms);
        if (!bx.bounded) continue;
        /* a singular / non-finite transform (e.g. `scale 0 0 0`) sends NaN rays into the
         * geometry, whose hits follow no geometric bound: never cull such a node */
        bool sane = true;
        for (int i = 0; i < 9; ++i) sane = sane && std::isfinite(nodes[n].m[i]) && std::isfinite(nodes[n].inv[i]) && std::isfinite(nodes[n].tinv[i]);
        for (int i = 0; i < 3; ++i) sane = sane && std::isfinite(nodes[n].off[i]);
        if (!sane) continue;
        /* pads: the same relative pad as the bounding sphere (the tests run in fp64 on coordinates
         * of this magnitude); shadow rays start 1e-6 (world units) off the surface (rt/shader.d:88):
         * 4e-6 world units = 4e-6 * |M^-1|_F object units (|M^-1|_F >= 1 / smallest scale) */
        double inv_norm = 0;
        for (int i = 0; i < 9; ++i) inv_norm += nodes[n].inv[i] * nodes[n].inv[i];
        inv_norm = std::sqrt(inv_norm);
        double mag = 0, ext = 0;
        for (int i = 0; i < 3; ++i) {
            mag += std::fmax(std::fabs(bx.lo[i]), std::fabs(bx.hi[i]));
            ext = std::fmax(ext, bx.hi[i] - bx.lo[i]);
        }
        const double pad = 1e-6 * ext + 1e-6 * mag + 1e-9 + 4e-6 * (inv_norm > 1 ? inv_norm : 1.0);
        bool finite = std::isfinite(pad);
        for (int k = 0; k < 8 && finite; ++k) {
            const double q[3] = {(k & 1) ? bx.hi[0] + pad : bx.lo[0] - pad, (k & 2) ? bx.hi[1] + pad : bx.lo[1] - pad,
                                 (k & 4) ? bx.hi[2] + pad : bx.lo[2] - pad};
            double *w = &p.node_box[((size_t)n * 8 + k) * 3];
            for (int j = 0; j < 3; ++j) {
                w[j] = q[0] * nodes[n].m[0 + j] + q[1] * nodes[n].m[3 + j] + q[2] * nodes[n].m[6 + j] + nodes[n].off[j];
                finite = finite && std::isfinite(w[j]);
            }
        }
        p.node_boxed[n] = finite ? 1 : 0;
    }
}

/* Ground-plane shadow culling towards light 0 (RenderParams::ground_node): the first Plane node
 * under an identity matrix with zero offset is the ground; every boxed node gets the rectangle
 * (in the plane's x, z) of its padded world box projected from the light onto the plane.
 * Let Q be a point of the box on a shadow segment from P' = P + N*1e-6 (P on the plane) to the
 * light L: L, Q and P' are collinear, so the central projection of Q from L onto the plane is
 * the point where the line L-P' meets it — within 1e-6 * (horizontal / vertical extent of the
 * segment) of P.  Hence P lies in the projected box grown by that much; the rectangle is padded
 * by 1e-5 * (1 + slope) + 1e-9 * scale, far above rounding in P.  Defined only when the light is
 * above the plane and the whole box lies strictly between plane and light (or the mirror image
 * below the plane); otherwise the rectangle is everything. */
void plan_ground_rects(const c2rt_scene_desc *s, ScenePlan &p)
{
    const std::vector<DevNode> &nodes = p.nodes;
    std::vector<double> &rects = p.shadow_rects;
    rects.assign((size_t)kMaxCullNodes * 4, 0.0);
    for (int n = 0; n < kMaxCullNodes; ++n) {
        rects[4 * n + 0] = rects[4 * n + 2] = -HUGE_VAL;
        rects[4 * n + 1] = rects[4 * n + 3] = HUGE_VAL;
    }
    p.ground_node = -1;
    for (uint32_t n = 0; n < s->n_nodes && n < (uint32_t)kMaxCullNodes; ++n) {
        const DevNode &d = nodes[n];
        if (d.g.type == C2RT_GEOM_PLANE && (d.flags & kNodeIdentityMatrix) && (d.flags & kNodeZeroOffset) && std::isfinite(d.g.p[0])) {
            p.ground_node = (int32_t)n;
            p.ground_y = d.g.p[0];
            break;
        }
    }
    if (p.ground_node >= 0 && s->n_lights > 0) {
        const double *L = s->light_pos;
        const double y0 = p.ground_y, h = L[1] - y0; /* light height over the plane (signed) */
        for (uint32_t n = 0; n < s->n_nodes && n < (uint32_t)kMaxCullNodes; ++n) {
            if (!p.node_boxed[n] || !std::isfinite(h) || h == 0) continue;
            /* axis-aligned hull of the node's (possibly sheared) world box */
            double bmin[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, bmax[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
            for (int k = 0; k < 8; ++k)
                for (int j = 0; j < 3; ++j) {
                    const double v = p.node_box[((size_t)n * 8 + k) * 3 + j];
                    bmin[j] = std::min(bmin[j], v);
                    bmax[j] = std::max(bmax[j], v);
                }
            /* heights as t = (y - y0) / h: 0 on the plane, 1 at the light's height.  Shadow segments
             * start within 1e-6 of the plane and end at the light: what the box has beyond the plane
             * (t < 0) is out of their reach, so it is clipped there (with slack) */
            double t_lo = (bmin[1] - y0) / h, t_hi = (bmax[1] - y0) / h;
            if (t_lo > t_hi) std::swap(t_lo, t_hi);
            const double slack = 1e-5 * (1.0 + std::fabs(y0)) / std::fabs(h);
            t_lo = std::max(t_lo, -slack);
            if (!(t_hi < 1 - 1e-9) || !(t_hi >= t_lo)) continue; /* reaches the light's height, or wholly beyond the plane: no rectangle */
            double lo[2] = {HUGE_VAL, HUGE_VAL}, hi[2] = {-HUGE_VAL, -HUGE_VAL};
            double scale = std::fabs(y0) + std::fabs(L[0]) + std::fabs(L[1]) + std::fabs(L[2]);
            bool ok = true;
            for (int k = 0; k < 8 && ok; ++k) {
                const double wx = (k & 1) ? bmax[0] : bmin[0], wz = (k & 2) ? bmax[2] : bmin[2], t = (k & 4) ? t_hi : t_lo;
                const double sfac = 1.0 / (1.0 - t);         /* L + (w - L) * sfac lies on the plane */
                const double px = L[0] + (wx - L[0]) * sfac, pz = L[2] + (wz - L[2]) * sfac;
                ok = std::isfinite(px) && std::isfinite(pz);
                lo[0] = std::min(lo[0], px); hi[0] = std::max(hi[0], px);
                lo[1] = std::min(lo[1], pz); hi[1] = std::max(hi[1], pz);
                scale = std::max(scale, std::fabs(px) + std::fabs(pz));
            }
            if (!ok) continue;
            /* slope of the steepest-sideways shadow segment that can end in the rectangle */
            const double dx = std::max(std::fabs(lo[0] - L[0]), std::fabs(hi[0] - L[0]));
            const double dz = std::max(std::fabs(lo[1] - L[2]), std::fabs(hi[1] - L[2]));
            const double slope = std::sqrt(dx * dx + dz * dz) / std::fabs(h);
            const double pad = 1e-5 * (1.0 + slope) + 1e-9 * scale;
            if (!std::isfinite(pad)) continue;
            rects[4 * n + 0] = lo[0] - pad; rects[4 * n + 1] = hi[0] + pad;
            rects[4 * n + 2] = lo[1] - pad; rects[4 * n + 3] = hi[1] + pad;
        }
    } else {
        p.ground_node = -1;
    }
}

/* CsgDiff(L, Sphere) nodes whose tiles the pre-pass may find void (csg_void.h): L a Cube or a Sphere other than
 * the subtracted one, the node's matrix the identity (its offset moves box and sphere alike), a finite sphere
 * of positive radius.  Shadow test towards light 0 only where the ground refinement runs and the box lies
 * strictly between the ground's side of the light's height and the light (no shadow ray meets it after
 * passing the light). */
void plan_void_nodes(const c2rt_scene_desc *s, ScenePlan &p)
{
    const std::vector<DevGeom> &geoms = p.geoms;
    const std::vector<DevNode> &nodes = p.nodes;
    p.void_nodes.clear();
    for (uint32_t n = 0; n < s->n_nodes && n < (uint32_t)kMaxCullNodes && p.void_nodes.size() < (size_t)kMaxVoidNodes; ++n) {
        const DevNode &d = nodes[n];
        if (!p.node_boxed[n] || !(d.flags & kNodeIdentityMatrix) || d.g.type != C2RT_GEOM_CSG_DIFF) continue;
        const int32_t l = s->geom_child[2 * d.geom], r = s->geom_child[2 * d.geom + 1];
        if (l == r || s->geom_type[r] != C2RT_GEOM_SPHERE) continue;
        if (s->geom_type[l] != C2RT_GEOM_CUBE && s->geom_type[l] != C2RT_GEOM_SPHERE) continue;
        if (!(geoms[l].flags & kGeomFinite) || !(geoms[r].flags & kGeomFinite)) continue;
        const double *sp = s->geom_param + 4 * (size_t)r;
        if (!(sp[3] > 0)) continue;
        VoidNode v{};
        for (int j = 0; j < 3; ++j) { v.lo[j] = HUGE_VAL; v.hi[j] = -HUGE_VAL; }
        for (int k = 0; k < 8; ++k)
            for (int j = 0; j < 3; ++j) {
                const double w = p.node_box[((size_t)n * 8 + k) * 3 + j];
                v.lo[j] = std::min(v.lo[j], w);
                v.hi[j] = std::max(v.hi[j], w);
            }
        bool finite = true;
        for (int j = 0; j < 3; ++j) {
            v.c[j] = sp[j] + d.off[j];
            finite = finite && std::isfinite(v.c[j]) && std::isfinite(v.lo[j]) && std::isfinite(v.hi[j]);
        }
        if (!finite) continue;
        v.r2 = sp[3];
        v.node = n;
        v.flags = 1u;
        if (p.ground_node >= 0 && s->n_lights > 0) {
            const double *L = s->light_pos, gy = p.ground_y, h = L[1] - gy;
            const double tol = 1e-6 + 1e-9 * (std::fabs(L[1]) + std::fabs(v.lo[1]) + std::fabs(v.hi[1]));
            if (std::isfinite(L[0]) && std::isfinite(L[1]) && std::isfinite(L[2]) && std::isfinite(h) &&
                ((h > 0 && v.hi[1] < L[1] - tol) || (h < 0 && v.lo[1] > L[1] + tol)))
                v.flags |= 2u;
        }
        p.void_nodes.push_back(v);
    }
}

/* Sphere nodes the pre-pass may drop from tiles outside their silhouette (csg_void.h): the node's root geometry a
 * finite Sphere of positive radius, its matrix the identity (the offset moves the centre).  The shadow test
 * towards light 0 only where the ground refinement runs; whether the padded ball stays below the light's height
 * depends on the frame's margin (sphere_cull_of). */
void plan_sphere_nodes(const c2rt_scene_desc *s, ScenePlan &p)
{
    const std::vector<DevGeom> &geoms = p.geoms;
    const std::vector<DevNode> &nodes = p.nodes;
    p.sphere_nodes.clear();
    for (uint32_t n = 0; n < s->n_nodes && n < (uint32_t)kMaxCullNodes && p.sphere_nodes.size() < (size_t)kMaxSphereNodes; ++n) {
        const DevNode &d = nodes[n];
        if (!p.node_boxed[n] || !(d.flags & kNodeIdentityMatrix) || d.g.type != C2RT_GEOM_SPHERE) continue;
        if (!(geoms[d.geom].flags & kGeomFinite)) continue;
        const double *sp = s->geom_param + 4 * (size_t)d.geom;
        if (!(sp[3] > 0)) continue;
        SphereNode v{};
        bool finite = true;
        for (int j = 0; j < 3; ++j) {
            v.c[j] = sp[j] + d.off[j];
            finite = finite && std::isfinite(v.c[j]);
        }
        if (!finite) continue;
        v.rp = sp[3];
        v.node = n;
        v.flags = 1u;
        if (p.ground_node >= 0 && s->n_lights > 0 && std::isfinite(s->light_pos[0]) && std::isfinite(s->light_pos[1]) &&
            std::isfinite(s->light_pos[2]))
            v.flags |= 2u;
        p.sphere_nodes.push_back(v);
    }
}

/* The dark-tile test's table (csg_void.h, "Dark ground tiles"): the Sphere nodes above and the CsgDiff nodes above
 * whose left child is a Cube, with their convex sets eroded by the margins.  The table belongs to the scene — it is
 * uploaded with it and refreshed by c2rt_update_scene like the shadow rectangles —, so the margins are derived for
 * every eye within DarkCull::eye_max of the origin (max-norm; four times the scene's own scale, at least 1000), and
 * a frame whose eye lies farther out goes without the test (dark_cull_of).  Only where the scene has a ground, light 0
 * is finite and lit, and the node's convex set lies strictly between the ground and the light's height by more than
 * its margin. */
void plan_dark_nodes(const c2rt_scene_desc *s, ScenePlan &p)
{
    p.dark = DarkCull{};
    if (p.ground_node < 0 || s->n_lights == 0 || p.lights.empty() || !(p.lights[0].lit & 1u)) return;
    const double *L = s->light_pos, gy = p.ground_y, h = L[1] - gy;
    if (!(std::isfinite(L[0]) && std::isfinite(L[1]) && std::isfinite(L[2]) && std::isfinite(h)) || h == 0) return;
    const double light_mag = std::max(std::fabs(L[0]), std::max(std::fabs(L[1]), std::fabs(L[2])));
    double base = 0; /* the largest R + |c| of the tested balls */
    for (const SphereNode &b : p.sphere_nodes)
        base = std::max(base, b.rp + std::max(std::fabs(b.c[0]), std::max(std::fabs(b.c[1]), std::fabs(b.c[2]))));
    for (const VoidNode &v : p.void_nodes)
        base = std::max(base, v.r2 + std::max(std::fabs(v.c[0]), std::max(std::fabs(v.c[1]), std::fabs(v.c[2]))));
    const double eye_max = std::max(1000.0, 4 * (base + light_mag));
    const double scale = base + light_mag + eye_max; /* at least every scale void_cull_of / sphere_cull_of derive */
    if (!std::isfinite(scale)) return;
    DarkCull dc{};
    dc.eye_max = eye_max;
    dc.reach = scale;
    const auto between = [&](double klo, double khi) { /* the set's extent in y, already grown by the margin */
        const double tol = 1e-6 + 1e-9 * (std::fabs(L[1]) + std::fabs(gy) + std::fabs(klo) + std::fabs(khi));
        return std::isfinite(klo) && std::isfinite(khi) &&
               ((h > 0 && klo > gy + tol && khi < L[1] - tol) || (h < 0 && khi < gy - tol && klo > L[1] + tol));
    };
    for (const SphereNode &b : p.sphere_nodes) {
        if (dc.n >= (uint32_t)kMaxDarkNodes) break;
        const double R = b.rp, m = sphere_margin(scale, R); /* (R: plan_sphere_nodes) */
        DarkNode k{};
        for (int j = 0; j < 3; ++j) k.c[j] = b.c[j];
        k.r = R - 2 * m;
        k.node = b.node;
        k.kind = 0u;
        if (!(k.r > 0) || !std::isfinite(k.r) || !between(k.c[1] - R - m, k.c[1] + R + m)) continue;
        dc.d[dc.n++] = k;
    }
    for (const VoidNode &v : p.void_nodes) {
        if (dc.n >= (uint32_t)kMaxDarkNodes) break;
        const DevNode &d = p.nodes[v.node];
        const int32_t l = s->geom_child[2 * d.geom];
        if (s->geom_type[l] != C2RT_GEOM_CUBE) continue;
        const double *cp = s->geom_param + 4 * (size_t)l;
        const double half = std::fabs(cp[3]) * 0.5, R = v.r2, m = void_margin(scale); /* (R: plan_void_nodes) */
        DarkNode k{};
        bool ok = half > 0;
        for (int j = 0; j < 3; ++j) {
            /* the cube's own faces moved inwards by the node box's padding (a bound of every rounding the box
             * carries), then by 2 m */
            const double clo = cp[j] - half + d.off[j], chi = cp[j] + half + d.off[j];
            const double pad = std::max(std::fabs(clo - v.lo[j]), std::fabs(v.hi[j] - chi));
            k.lo[j] = clo + pad + 2 * m;
            k.hi[j] = chi - pad - 2 * m;
            k.c[j] = v.c[j];
            ok = ok && std::isfinite(k.lo[j]) && std::isfinite(k.hi[j]) && k.lo[j] < k.hi[j];
        }
        k.r = R + 2 * m;
        k.node = v.node;
        k.kind = 1u;
        if (!ok || !(k.r > 0) || !std::isfinite(k.r) || !between(v.lo[1] - m, v.hi[1] + m)) continue;
        dc.d[dc.n++] = k;
    }
    if (dc.n) p.dark = dc;
}

} // namespace

int check_scene_desc(const c2rt_scene_desc *s, std::string &err)
{
    if (!s) return fail(err, C2RT_ERR_INVALID_ARG, "null scene");
    if (s->abi_version != C2RT_ABI_VERSION)
        return fail(err, C2RT_ERR_INVALID_ARG, "scene abi_version %u != %u", s->abi_version, C2RT_ABI_VERSION);
    if (s->gi_enabled) return fail(err, C2RT_ERR_UNSUPPORTED, "GIEnabled scenes (path tracing) are outside the hot path");
    if ((s->n_geoms && (!s->geom_type || !s->geom_param || !s->geom_child)) ||
        (s->n_textures && (!s->tex_type || !s->tex_color || !s->tex_param || !s->tex_scaling || !s->tex_width ||
                           !s->tex_height || !s->tex_offset)) ||
        (s->n_shaders && (!s->shader_type || !s->shader_color || !s->shader_texture || !s->shader_exponent ||
                          !s->shader_strength)) ||
        (s->n_lights && (!s->light_type || !s->light_pos || !s->light_color || !s->light_power)) ||
        (s->n_nodes && (!s->node_geom || !s->node_shader || !s->node_transform)) || (s->n_texels && !s->texels))
        return fail(err, C2RT_ERR_INVALID_ARG, "null table with non-zero count");
    if (s->n_geoms >= (1u << 23)) return fail(err, C2RT_ERR_LIMIT, "too many geometries");
    return C2RT_OK;
}

namespace {

/* plan_scene behind its header check; with_texels = false: replan_scene */
int plan_checked_scene(const c2rt_scene_desc *s, ScenePlan &plan, std::string &err, bool with_texels)
{
    int st;
    ScenePlan p;
    if ((st = plan_geoms(s, p, err)) != C2RT_OK) return st;
    if ((st = plan_textures(s, p, err, with_texels)) != C2RT_OK) return st;
    if ((st = plan_shaders(s, p, err)) != C2RT_OK) return st;
    if ((st = plan_lights(s, p, err)) != C2RT_OK) return st;
    if ((st = plan_nodes(s, p, err)) != C2RT_OK) return st;
    plan_node_flags(s, p);
    plan_csg_tile_nodes(s, p);
    plan_world_boxes(s, p);
    plan_ground_rects(s, p);
    plan_void_nodes(s, p);
    plan_sphere_nodes(s, p);
    plan_dark_nodes(s, p);
    p.n_nodes = s->n_nodes;
    p.n_lights = s->n_lights;
    std::memcpy(p.ambient, s->ambient, sizeof p.ambient);
    p.max_trace_depth = s->max_trace_depth;
    plan = std::move(p);
    return C2RT_OK;
}

template <typename T>
const T *copy_table(std::vector<T> &dst, const T *src, size_t n)
{
    if (src && n) dst.assign(src, src + n);
    else dst.clear();
    return dst.empty() ? nullptr : dst.data();
}

} // namespace

int plan_scene(const c2rt_scene_desc *s, ScenePlan &plan, std::string &err)
{
    if (const int st = check_scene_desc(s, err)) return st;
    return plan_checked_scene(s, plan, err, true);
}

/* ---- posing an uploaded scene ---- */
void SceneCopy::assign(const c2rt_scene_desc *s)
{
    desc = *s;
    const size_t g = s->n_geoms, t = s->n_textures, sh = s->n_shaders, l = s->n_lights, n = s->n_nodes;
    desc.geom_type = copy_table(geom_type, s->geom_type, g);
    desc.geom_param = copy_table(geom_param, s->geom_param, 4 * g);
    desc.geom_child = copy_table(geom_child, s->geom_child, 2 * g);
    desc.tex_type = copy_table(tex_type, s->tex_type, t);
    desc.tex_color = copy_table(tex_color, s->tex_color, 18 * t);
    desc.tex_param = copy_table(tex_param, s->tex_param, 6 * t);
    desc.tex_scaling = copy_table(tex_scaling, s->tex_scaling, t);
    desc.tex_width = copy_table(tex_width, s->tex_width, t);
    desc.tex_height = copy_table(tex_height, s->tex_height, t);
    desc.tex_offset = copy_table(tex_offset, s->tex_offset, t);
    desc.texels = nullptr; /* n_texels stays: plan_textures checks every bitmap's range against it */
    desc.shader_type = copy_table(shader_type, s->shader_type, sh);
    desc.shader_color = copy_table(shader_color, s->shader_color, 3 * sh);
    desc.shader_texture = copy_table(shader_texture, s->shader_texture, sh);
    desc.shader_exponent = copy_table(shader_exponent, s->shader_exponent, sh);
    desc.shader_strength = copy_table(shader_strength, s->shader_strength, sh);
    desc.light_type = copy_table(light_type, s->light_type, l);
    desc.light_pos = copy_table(light_pos, s->light_pos, 3 * l);
    desc.light_color = copy_table(light_color, s->light_color, 3 * l);
    desc.light_power = copy_table(light_power, s->light_power, l);
    desc.node_geom = copy_table(node_geom, s->node_geom, n);
    desc.node_shader = copy_table(node_shader, s->node_shader, n);
    desc.node_bump = nullptr; /* the planner does not read it (base modifyNormal is a no-op) */
    desc.node_transform = copy_table(node_transform, s->node_transform, 30 * n);
}

int check_scene_pose(const SceneCopy &scene, const c2rt_scene_pose *pose, std::string &err)
{
    if (!pose) return fail(err, C2RT_ERR_INVALID_ARG, "null pose");
    if (pose->n_nodes && !pose->node_index) return fail(err, C2RT_ERR_INVALID_ARG, "pose: %u nodes with a null node_index", pose->n_nodes);
    if (pose->n_lights && !pose->light_index) return fail(err, C2RT_ERR_INVALID_ARG, "pose: %u lights with a null light_index", pose->n_lights);
    if (pose->n_nodes && !pose->node_transform) return fail(err, C2RT_ERR_INVALID_ARG, "pose: %u nodes with a null node_transform", pose->n_nodes);
    if (pose->n_lights && !pose->light_pos && !pose->light_color && !pose->light_power)
        return fail(err, C2RT_ERR_INVALID_ARG, "pose: %u lights with null light_pos, light_color and light_power", pose->n_lights);
    const uint32_t have[2] = {scene.desc.n_nodes, scene.desc.n_lights}, n[2] = {pose->n_nodes, pose->n_lights};
    const uint32_t *index[2] = {pose->node_index, pose->light_index};
    static const char *const what[2] = {"node", "light"};
    for (int k = 0; k < 2; ++k)
        for (uint32_t i = 0; i < n[k]; ++i)
            if (index[k][i] >= have[k])
                return fail(err, C2RT_ERR_INVALID_ARG, "pose: %s_index[%u] = %u out of range (the scene has %u %ss)", what[k], i, index[k][i], have[k], what[k]);
    for (int k = 0; k < 2; ++k) {
        std::vector<uint8_t> seen(have[k], 0);
        for (uint32_t i = 0; i < n[k]; ++i) {
            if (seen[index[k][i]]) return fail(err, C2RT_ERR_INVALID_ARG, "pose: %s_index[%u] = %u is listed twice", what[k], i, index[k][i]);
            seen[index[k][i]] = 1;
        }
    }
    return C2RT_OK;
}

void drop_csg_certain(ScenePlan &plan)
{
    for (DevGeom &g : plan.geoms) g.flags &= ~kCsgCertain;
    for (DevNode &n : plan.nodes) n.g.flags &= ~kCsgCertain;
}

void drop_csg_tile(ScenePlan &plan)
{
    for (DevNode &n : plan.nodes) n.flags &= ~kNodeCsgTile;
}

int replan_scene(const SceneCopy &scene, ScenePlan &plan, std::string &err)
{
    return plan_checked_scene(&scene.desc, plan, err, false);
}

void pose_scene(SceneCopy &scene, const c2rt_scene_pose *pose, PoseUndo &undo)
{
    undo.node_transform.resize(30 * (size_t)pose->n_nodes);
    undo.light_pos.resize(3 * (size_t)pose->n_lights);
    undo.light_color.resize(3 * (size_t)pose->n_lights);
    undo.light_power.resize(pose->n_lights);
    for (uint32_t i = 0; i < pose->n_nodes; ++i) {
        double *t = &scene.node_transform[30 * (size_t)pose->node_index[i]];
        std::memcpy(&undo.node_transform[30 * (size_t)i], t, 30 * sizeof(double));
        std::memcpy(t, pose->node_transform + 30 * (size_t)i, 30 * sizeof(double));
    }
    for (uint32_t i = 0; i < pose->n_lights; ++i) {
        const size_t l = pose->light_index[i];
        std::memcpy(&undo.light_pos[3 * (size_t)i], &scene.light_pos[3 * l], 3 * sizeof(double));
        std::memcpy(&undo.light_color[3 * (size_t)i], &scene.light_color[3 * l], 3 * sizeof(float));
        undo.light_power[i] = scene.light_power[l];
        if (pose->light_pos) std::memcpy(&scene.light_pos[3 * l], pose->light_pos + 3 * (size_t)i, 3 * sizeof(double));
        if (pose->light_color) std::memcpy(&scene.light_color[3 * l], pose->light_color + 3 * (size_t)i, 3 * sizeof(float));
        if (pose->light_power) scene.light_power[l] = pose->light_power[i];
    }
}

void unpose_scene(SceneCopy &scene, const c2rt_scene_pose *pose, const PoseUndo &undo)
{
    for (uint32_t i = 0; i < pose->n_nodes; ++i)
        std::memcpy(&scene.node_transform[30 * (size_t)pose->node_index[i]], &undo.node_transform[30 * (size_t)i], 30 * sizeof(double));
    for (uint32_t i = 0; i < pose->n_lights; ++i) {
        const size_t l = pose->light_index[i];
        std::memcpy(&scene.light_pos[3 * l], &undo.light_pos[3 * (size_t)i], 3 * sizeof(double));
        std::memcpy(&scene.light_color[3 * l], &undo.light_color[3 * (size_t)i], 3 * sizeof(float));
        scene.light_power[l] = undo.light_power[i];
    }
}

int update_scene_plan(SceneCopy &scene, ScenePlan &plan, const c2rt_scene_pose *pose, std::string &err)
{
    if (const int st = check_scene_pose(scene, pose, err)) return st;
    if (pose->n_nodes == 0 && pose->n_lights == 0) return C2RT_OK;
    PoseUndo undo;
    pose_scene(scene, pose, undo);
    ScenePlan next;
    if (const int st = replan_scene(scene, next, err)) {
        unpose_scene(scene, pose, undo);
        return st;
    }
    next.texels4 = std::move(plan.texels4);
    plan = std::move(next);
    return C2RT_OK;
}

/* ---- the per-frame half ---- */
uint32_t strip_h(const c2rt_render_opts *o) { return o->strip_height ? o->strip_height : 1u; }

uint32_t local_rows_of(const c2rt_render_opts *o, uint32_t rank)
{
    if (o->strip_world <= 1) return o->height;
    const uint32_t sh = strip_h(o);
    const uint32_t n_strips = (o->height + sh - 1) / sh;
    uint32_t rows = 0;
    for (uint32_t s = rank; s < n_strips; s += o->strip_world) {
        const uint32_t y0 = s * sh;
        rows += (y0 + sh <= o->height) ? sh : (o->height - y0);
    }
    return rows;
}

int check_frame(const c2rt_camera_frame *cam, const c2rt_render_opts *o, std::string &err)
{
    if (o->width == 0 || o->height == 0 || o->width > (1u << 16) || o->height > (1u << 16))
        return fail(err, C2RT_ERR_INVALID_ARG, "bad frame size %ux%u", o->width, o->height);
    if (o->taps != C2RT_TAPS_1 && o->taps != C2RT_TAPS_REF5 && o->taps != C2RT_TAPS_4)
        return fail(err, C2RT_ERR_INVALID_ARG, "bad tap mode %u", o->taps);
    if (o->strip_world > 1 && o->strip_rank >= o->strip_world)
        return fail(err, C2RT_ERR_INVALID_ARG, "strip_rank %u >= strip_world %u", o->strip_rank, o->strip_world);
    if (cam->dof && (cam->num_samples == 0 || cam->num_samples > 4096))
        return fail(err, C2RT_ERR_LIMIT, "dof numSamples %u outside 1..4096", cam->num_samples);
    if (o->prepass_bucket > 65536) return fail(err, C2RT_ERR_UNSUPPORTED, "prepass bucket size %u > 65536", o->prepass_bucket);
    if (!(cam->frame_width > 0) || !(cam->frame_height > 0))
        return fail(err, C2RT_ERR_INVALID_ARG, "camera frame size must be positive");
    return C2RT_OK;
}

/* Convex hull of eight 2-D points (Andrew's monotone chain) as up to kHullEdges half planes
 * a*x + b*y + c >= 0 ((a, b) of unit length), each pushed outward by `pad`.  The central projection of a
 * box is at most a hexagon; false (nothing written) for a degenerate hull or one with more edges. */
bool hull_half_planes(const double pts[8][2], double pad, double out[kHullEdges][3])
{
    int order[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    std::sort(order, order + 8, [&](int i, int j) { return pts[i][0] < pts[j][0] || (pts[i][0] == pts[j][0] && pts[i][1] < pts[j][1]); });
    auto cross = [&](int o, int a, int b) {
        return (pts[a][0] - pts[o][0]) * (pts[b][1] - pts[o][1]) - (pts[a][1] - pts[o][1]) * (pts[b][0] - pts[o][0]);
    };
    int hv[17], m = 0;
    for (int i = 0; i < 8; ++i) { /* lower chain */
        while (m >= 2 && cross(hv[m - 2], hv[m - 1], order[i]) <= 0) --m;
        hv[m++] = order[i];
    }
    for (int i = 6, t = m + 1; i >= 0; --i) { /* upper chain */
        while (m >= t && cross(hv[m - 2], hv[m - 1], order[i]) <= 0) --m;
        hv[m++] = order[i];
    }
    --m; /* the last point repeats the first; hv[0..m) is the hull, counter-clockwise */
    if (m < 3 || m > kHullEdges) return false;
    /* Two projected corners that nearly coincide (the eye almost on the line of a box edge) pass the turn
     * tests on noise-dominated cross products and would contribute an "edge" whose half plane is not a
     * supporting line of the true hull — it could cull tiles the box covers.  Such a hull is refused (the
     * caller keeps the rectangle, which has no such failure mode): every edge must be longer than 1e-6 of
     * the hull's extent. */
    double ext = 0;
    for (int i = 0; i < m; ++i)
        for (int j = i + 1; j < m; ++j)
            ext = std::fmax(ext, std::fmax(std::fabs(pts[hv[i]][0] - pts[hv[j]][0]), std::fabs(pts[hv[i]][1] - pts[hv[j]][1])));
    double tmp[kHullEdges][3];
    for (int e = 0; e < kHullEdges; ++e) { tmp[e][0] = tmp[e][1] = 0; tmp[e][2] = 1; }
    for (int e = 0; e < m; ++e) {
        const double *p0 = pts[hv[e]], *p1 = pts[hv[(e + 1) % m]];
        double a = -(p1[1] - p0[1]), b = p1[0] - p0[0]; /* interior to the left of p0 -> p1: inward normal */
        const double len = std::sqrt(a * a + b * b);
        if (!(len > 1e-6 * ext) || !std::isfinite(len)) return false;
        a /= len; b /= len;
        const double c = -(a * p0[0] + b * p0[1]) + pad;
        if (!std::isfinite(c)) return false;
        tmp[e][0] = a; tmp[e][1] = b; tmp[e][2] = c;
    }
    std::memcpy(out, tmp, sizeof tmp);
    return true;
}

void fill_params(const ScenePlan &plan, const DeviceTables &dev, const DiagKnobs &knobs, const c2rt_camera_frame *cam,
                 const c2rt_render_opts *o, RenderParams &p)
{
    std::memset(&p, 0, sizeof p);
    p.geoms = dev.geoms;
    p.nodes = dev.nodes;
    p.shaders = dev.shaders;
    p.textures = dev.textures;
    p.lights = dev.lights;
    p.texels = dev.texels;
    p.n_nodes = plan.n_nodes;
    p.n_lights = plan.n_lights;
    std::memcpy(p.ambient, plan.ambient, sizeof p.ambient);
    p.max_trace_depth = plan.max_trace_depth;
    p.cam = *cam;
    for (int i = 0; i < 3; ++i) {
        p.cam_du[i] = cam->up_right[i] - cam->up_left[i];
        p.cam_dv[i] = cam->down_left[i] - cam->up_left[i];
    }
    /* lean:: divides sample coordinates by the camera's frame size through these (c2rt_trace.inc, screen_ray);
     * a frame size that is not a sane denominator (the ABI accepts any positive double) — or, in the diagnostics
     * build, C2RT_EXACT=1 (A/B runs: the compiler's IEEE divide / sqrt everywhere, as in rounds 1-2) — sends
     * every tile down the exact:: path */
    p.cam_rw = 1.0 / cam->frame_width;
    p.cam_rh = 1.0 / cam->frame_height;
    const auto sane = [](double v) { return v >= 0x1p-100 && v < 0x1p100; };
    p.force_exact = (knobs.exact || !sane(cam->frame_width) || !sane(cam->frame_height)) ? 1u : 0u;
    p.width = o->width;
    p.height = o->height;
    p.taps = o->prepass_bucket ? 1u : o->taps;
    p.prepass_bucket = o->prepass_bucket;
    p.strip_height = strip_h(o);
    p.strip_rank = o->strip_world > 1 ? o->strip_rank : 0;
    p.strip_world = o->strip_world > 1 ? o->strip_world : 1;
    p.local_rows = local_rows_of(o, p.strip_rank);
    p.tiles_x = (o->width + kTileW - 1) / kTileW;
    p.tiles_y = (p.local_rows + kTileH - 1) / kTileH;
    p.blocks_x = (p.tiles_x + kWavesPerBlock - 1) / kWavesPerBlock;
    p.seed = o->seed;
    p.tile_stats = dev.tile_stats;
    p.row_group_start = 0;
    p.planes_only = plan.planes_only;
    p.all_identity = plan.all_identity;
    p.ground_node = plan.ground_node;
    p.ground_y = plan.ground_y;
    p.shadow_rects = dev.shadow_rects;
    p.n_cull = 0;
    if (!cam->dof && cam->stereo_separation == 0 && !o->prepass_bucket) {
        /* up to the last bounded node; nothing bounded => no per-wave work at all */
        const uint32_t lim = plan.n_nodes < (uint32_t)kMaxCullNodes ? plan.n_nodes : (uint32_t)kMaxCullNodes;
        for (uint32_t n = 0; n < lim; ++n)
            if (plan.node_boxed[n]) p.n_cull = n + 1;
        for (uint32_t n = 0; n < p.n_cull; ++n) {
            for (int e = 0; e < kHullEdges; ++e) { p.cull_hull[n][e][0] = p.cull_hull[n][e][1] = 0.0f; p.cull_hull[n][e][2] = 1.0f; }
            if (plan.node_boxed[n]) cull_rect_of(cam, &plan.node_box[(size_t)n * 24], p.cull_rect[n], p.cull_hull[n]);
            else { p.cull_rect[n][0] = p.cull_rect[n][1] = INT32_MIN; p.cull_rect[n][2] = p.cull_rect[n][3] = INT32_MAX; }
        }
        /* dispatch order: start at the tile rows where the boxed nodes begin (their tiles are the
         * expensive ones), wrap around to the rows above them (mostly sky) at the end */
        int32_t top = INT32_MAX;
        for (uint32_t n = 0; n < p.n_cull; ++n)
            if (plan.node_boxed[n] && p.cull_rect[n][1] < top) top = p.cull_rect[n][1];
        if (top != INT32_MAX && top > 0 && (uint32_t)top < o->height) {
            /* frame row -> local row of this launch (strips: rows are dealt round-robin) */
            const uint32_t local = (uint32_t)top / p.strip_world;
            const uint32_t groups = (p.tiles_y + 7u) / 8u;
            const uint32_t g = local / (kTileH * 8u);
            p.row_group_start = g < groups ? g : 0;
        }
        if (p.n_cull) {
            p.n_cull_lights = plan.n_lights < (uint32_t)kMaxCullLights ? plan.n_lights : (uint32_t)kMaxCullLights;
            for (uint32_t l = 0; l < p.n_cull_lights; ++l) light_side_of(cam, &plan.light_pos[3 * (size_t)l], p.light_side[l]);
        }
    }
    /* diagnostics build only (like C2RT_CSG_FIRST_CAP; frames are unchanged by construction, slower): C2RT_DEBUG_CULL bit 0:
     * no culling rectangles at all; bit 1: no ground-plane refinement of the shadow mask; bit 2: no view-pyramid
     * culling of shadow rays; bit 3: no sphere-silhouette test in the mask pre-pass (sphere_cull_of) */
    const int debug_cull = knobs.debug_cull;
    if (debug_cull & 1) p.n_cull = 0;
    if (debug_cull & 2) p.ground_node = -1;
    if (debug_cull & 4) p.n_cull_lights = 0;
    /* Ground-only tiles through lean::ground_tile (c2rt_trace.inc): only where the frame has a mask table (which rules
     * out depth of field, stereo and the prepass preview) and a ground node, at most one light (the instances that
     * carry the path), no counted rays (those frames run exact:: throughout), and a floor the path is specialised
     * for — Lambert over a bitmap, a checker or a plain colour: no libm call (Phong's pow, Procedure2's sin) enters
     * it.  Diagnostics build: C2RT_DEBUG_CULL bit 4 leaves every tile to the general path (A/B runs, tests). */
    p.ground_fast = 0;
    if (p.n_cull && p.ground_node >= 0 && (uint32_t)p.ground_node < plan.nodes.size() && plan.n_lights <= 1 && !o->count_rays &&
        !cam->dof && cam->stereo_separation == 0 && !(debug_cull & 16)) {
        const DevMat &m = plan.nodes[(size_t)p.ground_node].mat;
        const bool tex_ok = m.tex_type < 0 || m.tex_type == C2RT_TEX_CHECKER || m.tex_type == C2RT_TEX_BITMAP;
        p.ground_fast = (m.shader_type == C2RT_SHADER_LAMBERT && tex_ok) ? 1u : 0u;
    }
    /* Of those frames, the ones inside the domain of ground_certain.h take lean::ground_tile_certain first: a bitmap or
     * a plain colour (a checker floor stays on ground_tile: its parity test has no certainty form yet), the eye above the
     * floor, the light — if it shines — above it too, magnitudes in that header's windows (gc_plan).  The light and the
     * plane are read from the tables the kernel reads, so a posed frame is judged by its own pose.  Diagnostics build:
     * C2RT_DEBUG_CULL bit 6 leaves every tile to ground_tile. */
    p.ground_certain_cq = 0;
    if (p.ground_fast && !(debug_cull & 64)) {
        const DevNode &g = plan.nodes[(size_t)p.ground_node];
        const bool bitmap = g.mat.tex_type == C2RT_TEX_BITMAP;
        float scaling;
        std::memcpy(&scaling, &g.mat.texdata[2], sizeof scaling);
        const bool lit = plan.n_lights == 1 && !plan.lights.empty() && (plan.lights[0].lit & 1u);
        const double none[3] = {0, 0, 0};
        /* bitmap_filtered_uniform (c2rt_trace_shared.inc) addresses the floor's texels with 32-bit byte offsets and a
         * 24-bit row product: the bitmap ends within the pool's first 2^28 texels and neither side reaches 2^24 */
        bool tex_fits = true;
        if (bitmap) {
            const uint64_t w = g.mat.texdata[0], h = g.mat.texdata[1];
            const uint64_t offset = (uint64_t)g.mat.texdata[4] | ((uint64_t)g.mat.texdata[5] << 32);
            tex_fits = w < (1ull << 24) && h < (1ull << 24) && offset <= (1ull << 28) && w * h <= (1ull << 28) - offset;
        }
        if ((g.mat.tex_type < 0 || bitmap) && tex_fits && g.g.p[0] == p.ground_y)
            p.ground_certain_cq = gc_plan(cam->pos, g.g.p[0], g.g.p[1], lit, lit ? plan.lights[0].pos : none, bitmap, (double)scaling);
    }
}

/* Screen rectangle of a node for this frame: the projection of the 8 world-space
 * box corners through the camera (a projective map, convex on the half space in
 * front of the eye), widened by 2 pixels (the AA taps reach 0.6 px, rounding is
 * ~1e-13 px).  Any corner at or behind the eye plane => the whole frame. */
void cull_rect_of(const c2rt_camera_frame *cam, const double *corners, int32_t out[4], float hull[kHullEdges][3])
{
    const int32_t kAll[4] = {INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX};
    std::memcpy(out, kAll, sizeof kAll);
    double du[3], dv[3], ul[3];
    for (int i = 0; i < 3; ++i) {
        du[i] = cam->up_right[i] - cam->up_left[i];
        dv[i] = cam->down_left[i] - cam->up_left[i];
        ul[i] = cam->up_left[i] - cam->pos[i];
    }
    /* solve a*du + b*dv + l*ul = w by Cramer's rule */
    auto det3 = [](const double *a, const double *b, const double *c) {
        return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
    };
    const double det = det3(du, dv, ul);
    if (!std::isfinite(det) || det == 0) return;
    double xmin = 1e300, xmax = -1e300, ymin = 1e300, ymax = -1e300;
    double pts[8][2];
    for (int k = 0; k < 8; ++k) {
        double w[3];
        for (int i = 0; i < 3; ++i) w[i] = corners[3 * k + i] - cam->pos[i];
        const double a = det3(w, dv, ul) / det, b = det3(du, w, ul) / det, l = det3(du, dv, w) / det;
        if (!(l > 1e-9) || !std::isfinite(a) || !std::isfinite(b)) return; /* at / behind the eye: no culling */
        const double px = a / l * cam->frame_width, py = b / l * cam->frame_height;
        if (!std::isfinite(px) || !std::isfinite(py)) return;
        pts[k][0] = px; pts[k][1] = py;
        xmin = std::fmin(xmin, px); xmax = std::fmax(xmax, px);
        ymin = std::fmin(ymin, py); ymax = std::fmax(ymax, py);
    }
    const double lim = 1e9;
    if (xmin < -lim || ymin < -lim || xmax > lim || ymax > lim) return;
    out[0] = (int32_t)std::floor(xmin) - 2;
    out[1] = (int32_t)std::floor(ymin) - 2;
    out[2] = (int32_t)std::ceil(xmax) + 3;
    out[3] = (int32_t)std::ceil(ymax) + 3;

    /* the hull of the eight projected corners, one outward-padded half plane per edge.  Only for rectangles
     * of sane size (float coefficients: |c| < 1e6 keeps the evaluation error at a tile corner below
     * 0.25 px, and the pad is 2.5 px where the rectangle's is 2). */
    if (!hull || xmin < -3e5 || ymin < -3e5 || xmax > 3e5 || ymax > 3e5) return;
    double hp[kHullEdges][3];
    if (!hull_half_planes(pts, 2.5, hp)) return;
    for (int e = 0; e < kHullEdges; ++e)
        if (std::fabs(hp[e][2]) > 1e6) return;
    for (int e = 0; e < kHullEdges; ++e)
        for (int k = 0; k < 3; ++k) hull[e][k] = (float)hp[e][k];
}

/* For one light: the integer boundary coordinates x (pixels) for which the light is
 * certainly in the closed half space a - l*x/W >= 0 (">= x" side of the vertical
 * boundary plane through the eye) resp. <= 0, and the same for y.  (a, b, l) are
 * the light's coordinates in the (du, dv, ul) basis; the half spaces are linear in
 * them, so this is valid for lights behind the eye too.  One pixel of slack. */
void light_side_of(const c2rt_camera_frame *cam, const double *light, int32_t out[8])
{
    for (int i = 0; i < 4; ++i) { out[2 * i] = 1; out[2 * i + 1] = 0; } /* empty intervals */
    double du[3], dv[3], ul[3], w[3];
    for (int i = 0; i < 3; ++i) {
        du[i] = cam->up_right[i] - cam->up_left[i];
        dv[i] = cam->down_left[i] - cam->up_left[i];
        ul[i] = cam->up_left[i] - cam->pos[i];
        w[i] = light[i] - cam->pos[i];
    }
    auto det3 = [](const double *a, const double *b, const double *c) {
        return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
    };
    const double det = det3(du, dv, ul);
    if (!std::isfinite(det) || det == 0) return;
    const double a = det3(w, dv, ul) / det, b = det3(du, w, ul) / det, l = det3(du, dv, w) / det;
    if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(l)) return;
    const double lim = 1e9;
    auto axis = [&](double c, double size, int32_t *ge, int32_t *le) {
        /* phi(x) = c*size - l*x: ">= x side" <=> phi(x) >= 0, "<= x side" <=> phi(x) <= 0 */
        const double eps = 1e-12 * (std::fabs(c) + std::fabs(l));
        if (std::fabs(l) <= eps) {
            if (c > eps) { ge[0] = INT32_MIN; ge[1] = INT32_MAX; }
            if (c < -eps) { le[0] = INT32_MIN; le[1] = INT32_MAX; }
            return;
        }
        const double xs = c * size / l;
        if (!(std::fabs(xs) < lim)) return;
        if (l > 0) { /* phi decreasing: >= 0 for x <= xs */
            ge[0] = INT32_MIN; ge[1] = (int32_t)std::floor(xs) - 1;
            le[0] = (int32_t)std::ceil(xs) + 1; le[1] = INT32_MAX;
        } else {     /* phi increasing: >= 0 for x >= xs */
            ge[0] = (int32_t)std::ceil(xs) + 1; ge[1] = INT32_MAX;
            le[0] = INT32_MIN; le[1] = (int32_t)std::floor(xs) - 1;
        }
    };
    axis(a, cam->frame_width, out + 0, out + 2);
    axis(b, cam->frame_height, out + 4, out + 6);
}

KernelVariant variant_of(const ScenePlan &plan, const c2rt_camera_frame *cam)
{
    KernelVariant v;
    v.csg_levels = plan.csg_levels;
    v.dof_or_stereo = cam->dof != 0 || cam->stereo_separation != 0;
    return v;
}

/* the void test's per-frame part (csg_void.h): the ball's margin at this frame's scale (void_margin), the nodes the
 * frame culls, the shadow test only where the frame runs the ground refinement towards light 0.  flags_mask: every
 * VoidNode::flags is ANDed with it (~0u for frames; the diagnostics readback c2rt_debug_tile_masks varies it). */
VoidCull void_cull_of(const ScenePlan &plan, const RenderParams &p, uint32_t flags_mask)
{
    VoidCull vc{};
    for (const VoidNode &seed : plan.void_nodes) {
        if (seed.node >= p.n_cull) continue;
        VoidNode v = seed;
        const double R = seed.r2;
        double scale = R;
        scale += std::max(std::fabs(v.c[0]), std::max(std::fabs(v.c[1]), std::fabs(v.c[2])));
        scale += std::max(std::fabs(p.cam.pos[0]), std::max(std::fabs(p.cam.pos[1]), std::fabs(p.cam.pos[2])));
        if (!plan.light_pos.empty())
            scale += std::max(std::fabs(plan.light_pos[0]), std::max(std::fabs(plan.light_pos[1]), std::fabs(plan.light_pos[2])));
        const double rm = R - void_margin(scale);
        if (!(rm > 0) || !std::isfinite(scale)) continue;
        v.r2 = rm * rm;
        if (p.n_cull_lights == 0 || p.ground_node < 0) v.flags &= ~2u;
        v.flags &= flags_mask;
        vc.v[vc.n++] = v;
    }
    if (!plan.light_pos.empty())
        for (int j = 0; j < 3; ++j) vc.light0[j] = plan.light_pos[j];
    return vc;
}

/* the sphere test's per-frame part (csg_void.h): one scale for the frame (the largest R + |c| of its balls, the eye,
 * light 0), which is also the reach of the shadow test; R + sphere_margin per ball; the shadow test only where the
 * frame runs the ground refinement towards light 0 and the PADDED ball stays on the ground's side of the light's
 * height.  flags_mask: every SphereNode::flags is ANDed with it (~0u for frames). */
SphereCull sphere_cull_of(const ScenePlan &plan, const DiagKnobs &knobs, const RenderParams &p, uint32_t flags_mask)
{
    SphereCull sc{};
    /* diagnostics build only: C2RT_DEBUG_CULL bit 3: no sphere-silhouette test (frames are unchanged, slower) */
    if (knobs.debug_cull & 8) flags_mask = 0;
    double scale = 0;
    for (const SphereNode &seed : plan.sphere_nodes)
        scale = std::max(scale, seed.rp + std::max(std::fabs(seed.c[0]), std::max(std::fabs(seed.c[1]), std::fabs(seed.c[2]))));
    scale += std::max(std::fabs(p.cam.pos[0]), std::max(std::fabs(p.cam.pos[1]), std::fabs(p.cam.pos[2])));
    if (!plan.light_pos.empty())
        scale += std::max(std::fabs(plan.light_pos[0]), std::max(std::fabs(plan.light_pos[1]), std::fabs(plan.light_pos[2])));
    if (!std::isfinite(scale) || !(flags_mask & 3u)) return sc;
    sc.reach = scale;
    for (const SphereNode &seed : plan.sphere_nodes) {
        if (seed.node >= p.n_cull) continue;
        SphereNode s = seed;
        s.rp = seed.rp + sphere_margin(scale, seed.rp);
        if (!std::isfinite(s.rp)) continue;
        if (p.n_cull_lights == 0 || p.ground_node < 0 || plan.light_pos.empty()) s.flags &= ~2u;
        if (s.flags & 2u) {
            const double Ly = plan.light_pos[1], h = Ly - p.ground_y;
            const double tol = 1e-6 + 1e-9 * (std::fabs(Ly) + std::fabs(s.c[1]) + s.rp);
            if (!((h > 0 && s.c[1] + s.rp < Ly - tol) || (h < 0 && s.c[1] - s.rp > Ly + tol))) s.flags &= ~2u;
        }
        s.flags &= flags_mask;
        if (s.flags) sc.s[sc.n++] = s;
    }
    /* Sphere-interior tiles through lean::sphere_tile (c2rt_trace.inc; csg_void.h): the frame conditions of the ground-tile
     * path — a mask table, at most one light, no depth of field, no stereo, no nested CsgOp (the instances that carry the
     * path), not a counted frame (RenderParams::ray_counters is set by then: those run exact:: throughout) — and per node a material the path carries:
     * Lambert or Phong over a plain colour or a bitmap that bitmap_filtered_uniform can address (within the pool's first
     * 2^28 texels, sides below 2^24).  Checker and Procedure2 spheres stay on the general path.
     * And only a frame large enough to pay for the test: in the pre-pass — one lane per tile, a chain of latencies in
     * front of the frame kernel — the claim costs about 3 us per frame whatever the frame's size, and a claimed tile
     * saves about 0.7 ns per tap (profiles/r12_variants.md: lecture5 at 1080p with one tap lost 1.9 us with the path, at
     * 4K with five it gains 21 us).  With some 6 % of the tiles claimed the two meet near five million samples per launch;
     * kSphereTileMinSamples is a little above.  Diagnostics build: C2RT_DEBUG_CULL bit 7 leaves every tile to the general
     * path, bit 8 drops the size condition (the tests' small frames). */
    constexpr uint64_t kSphereTileMinSamples = 6000000;
    const uint64_t samples = (uint64_t)p.width * p.height * p.taps / (p.strip_world > 1 ? p.strip_world : 1u);
    if (p.n_cull && plan.n_lights <= 1 && plan.csg_levels <= 1 && !p.cam.dof && p.cam.stereo_separation == 0 && !p.ray_counters &&
        !(knobs.debug_cull & 128) &&
        (samples >= kSphereTileMinSamples || (knobs.debug_cull & 256))) {
        for (uint32_t j = 0; j < sc.n; ++j) {
            const uint32_t n = sc.s[j].node;
            if (n >= plan.nodes.size() || n >= 32u) continue;
            const DevMat &m = plan.nodes[n].mat;
            if (m.shader_type != C2RT_SHADER_LAMBERT && m.shader_type != C2RT_SHADER_PHONG) continue;
            bool tex_ok = m.tex_type < 0;
            if (m.tex_type == C2RT_TEX_BITMAP) {
                const uint64_t w = m.texdata[0], h = m.texdata[1];
                const uint64_t offset = (uint64_t)m.texdata[4] | ((uint64_t)m.texdata[5] << 32);
                tex_ok = w < (1ull << 24) && h < (1ull << 24) && offset <= (1ull << 28) && w * h <= (1ull << 28) - offset;
            }
            if (tex_ok) sc.interior |= 1u << n;
        }
    }
    return sc;
}

/* the dark-tile test's per-frame part (csg_void.h): the scene's table (plan_dark_nodes), or none — where the frame
 * runs no ground refinement, where the eye is not on the light's side of the ground, or lies beyond the distance the
 * table's margins were derived for.  Independent of the void and silhouette tests' switches.  Diagnostics build only:
 * C2RT_DEBUG_CULL bit 5: no dark-tile test (frames are unchanged, slower). */
bool dark_frame_ok(const ScenePlan &plan, const DiagKnobs &knobs, const RenderParams &p)
{
    if ((knobs.debug_cull & 32) || !plan.dark.n || p.ground_node < 0 || !p.n_cull || plan.light_pos.size() < 3) return false;
    const double h = plan.light_pos[1] - p.ground_y, eye = p.cam.pos[1] - p.ground_y;
    if (!((h > 0 && eye > 0) || (h < 0 && eye < 0))) return false;
    const double cam_mag = std::max(std::fabs(p.cam.pos[0]), std::max(std::fabs(p.cam.pos[1]), std::fabs(p.cam.pos[2])));
    return cam_mag <= plan.dark.eye_max;
}

DarkCull dark_cull_of(const ScenePlan &plan, const DiagKnobs &knobs, const RenderParams &p)
{
    return dark_frame_ok(plan, knobs, p) ? plan.dark : DarkCull{};
}

} // namespace c2rt
