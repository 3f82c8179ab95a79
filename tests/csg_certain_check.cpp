/* Host build of csg_certain.h (tests/test_csg_certain_host.py, scripts/csg_certain_census.py): the decision the frame
 * kernels take per lane in csg_intersect_leaf, for arrays of object-space rays against one leaf CsgOp. */
#include <stdint.h>

#include <string>

#include "../chess2rt_amd/csrc/csg_certain.h"
#include "../chess2rt_amd/csrc/scene_plan.h"

using namespace c2rt;

/* a primitive's tables as the planner packs them (scene_plan.cpp: plan_geoms): p = {centre, R | side}, q = {lo, hi} */
static void pack(const double *p, double *q)
{
    const double halfSide = p[3] * 0.5;
    for (int i = 0; i < 3; ++i) {
        q[i] = p[i] + -1 * halfSide;
        q[3 + i] = p[i] + 1 * halfSide;
    }
}

/* op: 0 Union, 1 Inter, 2 Diff; l_sphere / r_sphere: the child is a Sphere (else a Cube); lp / rp: its four parameters;
 * o, d: n rays (3 doubles each); ms: the margins' scale (1: as shipped).  Out, per ray: kind (CC_R_*), side, k, dist, del. */
extern "C" void csg_certain_decide(int op, int short_a, int short_b, int l_sphere, const double *lp, int r_sphere, const double *rp,
                                   const double *o, const double *d, int64_t n, double ms, int32_t *kind, int32_t *side, int32_t *k,
                                   double *dist, double *del)
{
    double lq[6], rq[6];
    pack(lp, lq);
    pack(rp, rq);
    for (int64_t i = 0; i < n; ++i) {
        const CcResult w = cc_decide(op, short_a != 0, short_b != 0, l_sphere != 0, lp, lq, r_sphere != 0, rp, rq, o + 3 * i, d + 3 * i, ms);
        kind[i] = w.kind;
        side[i] = w.side;
        k[i] = w.k;
        dist[i] = w.dist;
        del[i] = w.del;
    }
}

/* one child alone: st (CC_EMPTY / ONE / TWO / UNSURE), a0, a1, del */
extern "C" void csg_certain_child(int is_sphere, const double *p, const double *o, const double *d, int64_t n, double ms, int32_t *st,
                                  double *a0, double *a1, double *del)
{
    double q[6];
    pack(p, q);
    for (int64_t i = 0; i < n; ++i) {
        const CcChild c = cc_child(is_sphere != 0, o + 3 * i, d + 3 * i, p, q, ms);
        st[i] = c.st;
        a0[i] = c.a0;
        a1[i] = c.a1;
        del[i] = c.del;
    }
}

/* the planner's GeomFlags of every geometry of `s` (kCsgCertain = 16 among them), as plan_scene leaves them; with
 * drop != 0 after drop_csg_certain (the diagnostics switch).  Returns plan_scene's status. */
extern "C" int csg_certain_plan_flags(const c2rt_scene_desc *s, int drop, int32_t *flags, uint32_t n)
{
    ScenePlan plan;
    std::string err;
    const int st = plan_scene(s, plan, err);
    if (st != C2RT_OK) return st;
    if (drop) drop_csg_certain(plan);
    for (uint32_t g = 0; g < n && g < plan.geoms.size(); ++g) flags[g] = plan.geoms[g].flags;
    /* a node's own copy of its root record must agree */
    for (const DevNode &nd : plan.nodes)
        if (nd.g.flags != plan.geoms[nd.geom].flags) return -1000;
    return st;
}
