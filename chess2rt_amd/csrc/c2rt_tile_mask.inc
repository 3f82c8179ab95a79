/*
 * c2rt_tile_mask.inc — the per-frame culling masks (host-computed rectangles, RenderParams): the classifier the
 * pre-pass kernel runs per tile (tile_mask_entry), where a tile's words live (tile_mask_slot) and the reader of the
 * further lights' masks (light_shadow_mask).  No lean / exact distinction: included ONCE by c2rt_trace_common.inc,
 * at c2rt::{anonymous} scope, behind c2rt_trace_shared.inc and in front of the two copies of c2rt_trace.inc.
 */

/* The culling masks of ONE tile, evaluated by ONE lane (the pre-pass kernel, c2rt_kernels.hip: tile_masks_kernel):
 * which nodes the tile's primary rays can reach, which can occlude its shadow rays towards light 0, and whether
 * only the ground plane is left in either.  Until round 3 every wave of the frame kernel derived this for its own
 * tile before its first sample — lane n testing node n, ballots, four corner rays read back across lanes — which
 * was 13 % of the resident wave-cycles of the headline frame and 42 % of a single-tap 1080p frame's (a chain of
 * dependent kernel-argument, rectangle, hull and shadow-rectangle loads in front of every tile).  Here a lane owns
 * a tile and loops over the nodes (their rectangles and hulls are scalar loads), 64 tiles per wave; the frame
 * kernel reads the four words with one scalar load.  out: {primary mask, shadow mask for light 0,
 * bit 0 = primary rays reach the ground plane only | bit 1 = and so do the shadow rays | bit 2 = primary-ground and every
 * shadow ray occluded (dark) | bit 3 = every primary ray's closest hit is on the one Sphere node left in the primary mask
 * beside the ground and no other node can occlude its shadow rays (sphere-interior), 0}. */
/* Where the tile in tile row `trow` of the table (row 0 = local row RenderParams::mask_row0), tile column `tcol`
 * keeps its four words: tile rows r, r + 8, r + 16, ... of a launch run on the same XCD (round-robin dispatch,
 * render_tile), so the table is laid out in eight row classes — each L2 fetches its own eighth once instead of
 * sharing every 128-byte line with a neighbour. */
DEV size_t tile_mask_slot(const RenderParams &P, uint32_t trow, uint32_t tcol)
{
    const uint32_t per_class = ((P.mask_rows + kTileH - 1) / kTileH + 7u) / 8u; /* tile rows per class */
    return ((size_t)(trow & 7u) * per_class + (trow >> 3)) * (P.blocks_x * kWavesPerBlock) + tcol;
}

/* Nodes that may occlude this tile's shadow rays towards light l >= 1 (light 0: Ctx::shadow_mask0): every hit point
 * lies in the tile's view pyramid; a node whose box is entirely beyond one side plane of the pyramid while the light
 * is on the inner side of that plane is in a half space none of those segments enters.  From the second table the
 * pre-pass wrote for frames with several culled lights (tile_mask_entry: out[4..6]) — until round 4 every sample
 * derived it again with lane n standing for node n and a ballot. */
static_assert(kMaxCullLights <= 4, "one table word per culled light beyond the first");
DEV uint32_t light_shadow_mask(const RenderParams &P, uint32_t mask_slot, uint32_t l)
{
    if (!P.n_cull || l >= P.n_cull_lights) return 0xFFFFFFFFu;
    return ((const uint32_t C2RT_K *)P.tile_masks)[((size_t)P.mask_entries + mask_slot) * 4u + (l - 1u)];
}

DEV void tile_mask_entry(const RenderParams &P, KArgs K, const VoidCull &V, const SphereCull &S, const DarkCull *Dp, uint32_t trow, uint32_t tcol, uint32_t out[8])
{
    typedef const int C2RT_K *KInt;
    typedef const char C2RT_K *KChar;
    /* frame-space bounds of the tile, as render_tile has them for the launch that renders it */
    int tx0 = (int)(tcol * kTileW), ty0, ty1;
    {
        const uint32_t lr_first = trow * kTileH + P.mask_row0;
        uint32_t lr_last = trow * kTileH + kTileH - 1;
        if (lr_last >= P.mask_rows) lr_last = P.mask_rows - 1;
        lr_last += P.mask_row0;
        ty0 = (int)lr_first;
        ty1 = (int)lr_last;
        if (P.strip_world > 1) {
            const uint32_t sh = P.strip_height;
            ty0 = (int)(((lr_first / sh) * P.strip_world + P.strip_rank) * sh + lr_first % sh);
            ty1 = (int)(((lr_last / sh) * P.strip_world + P.strip_rank) * sh + lr_last % sh);
        }
    }
    const uint32_t nc = P.n_cull < (uint32_t)kMaxCullNodes ? P.n_cull : (uint32_t)kMaxCullNodes;
    KInt rects = (KInt)((KChar)K + __builtin_offsetof(RenderParams, cull_rect));
    KFlt hulls = (KFlt)((KChar)K + __builtin_offsetof(RenderParams, cull_hull));
    const float X0 = (float)tx0, X1 = (float)(tx0 + kTileW), Y0 = (float)ty0, Y1 = (float)(ty1 + 1);
    /* shadow rays towards light 0: the tile's view pyramid against the node rectangles (shadow_cull_mask) */
    const bool shadow_cull = 0 < P.n_cull_lights;
    const int sx1 = tx0 + kTileW + 1, sy1 = ty1 + 1;
    const int *sd = P.light_side[0];
    const bool in_left = tx0 >= sd[0] && tx0 <= sd[1], in_right = sx1 >= sd[2] && sx1 <= sd[3];
    const bool in_top = ty0 >= sd[4] && ty0 <= sd[5], in_bottom = sy1 >= sd[6] && sy1 <= sd[7];
    uint32_t pmask = 0xFFFFFFFFu, smask0 = 0xFFFFFFFFu;
    PyramidCone pcone;
    bool have_pcone = false;
    const auto primary_cone = [&]() {
        double cdir[4][3];
        tile_corner_dirs(P.cam.pos, P.cam.up_left, P.cam_du, P.cam_dv, P.cam.frame_width, P.cam.frame_height,
                         tx0, tx0 + kTileW, ty0, ty1 + 1, cdir);
        return pyramid_cone(cdir);
    };
    for (uint32_t n = 0; n < nc; ++n) {
        const int r0 = rects[4 * n + 0], r1 = rects[4 * n + 1], r2 = rects[4 * n + 2], r3 = rects[4 * n + 3];
        /* the node's rectangle, then its hull (RenderParams::cull_hull): outside one padded edge with all four
         * tile corners */
        const bool rect_misses = r2 <= tx0 || r0 >= tx0 + kTileW || r3 <= ty0 || r1 > ty1;
        bool off_hull = false;
        if (!rect_misses) {
            KFlt hl = hulls + n * (kHullEdges * 3);
#pragma unroll
            for (int e = 0; e < kHullEdges; ++e) {
                const float a = hl[3 * e], bb = hl[3 * e + 1], c = hl[3 * e + 2];
                const float ax0 = a * X0, ax1 = a * X1, by0 = bb * Y0, by1 = bb * Y1;
                const float worst = fmaxf(fmaxf(ax0, ax1) + fmaxf(by0, by1), -3.0e38f) + c; /* the corner deepest inside */
                off_hull |= worst < -0.25f; /* (0.25 px: float evaluation error at |coordinates| < 1e6) */
            }
        }
        if (rect_misses || off_hull) pmask &= ~(1u << n);
        else if (V.n | S.n) {
            /* a CsgDiff(L, Sphere) node, or a Sphere node, that no primary ray of the tile can hit (csg_void.h): only
             * for tiles whose rectangle and hull keep it; the tile's cone is derived once, by the first node to ask */
            for (uint32_t j = 0; j < V.n; ++j) {
                const VoidNode &vn = V.v[j];
                if (vn.node != n || !(vn.flags & 1u)) continue;
                if (!have_pcone) { pcone = primary_cone(); have_pcone = true; }
                if (pyramid_void(P.cam.pos, pcone, vn)) pmask &= ~(1u << n);
            }
            for (uint32_t j = 0; j < S.n; ++j) {
                const SphereNode &sn = S.s[j];
                if (sn.node != n || !(sn.flags & 1u)) continue;
                if (!have_pcone) { pcone = primary_cone(); have_pcone = true; }
                if (cone_misses_ball(P.cam.pos, pcone, sn.c, sn.rp)) pmask &= ~(1u << n);
            }
        }
        if (shadow_cull && ((in_left && r2 <= tx0) || (in_right && r0 >= sx1) || (in_top && r3 <= ty0) || (in_bottom && r1 >= sy1)))
            smask0 &= ~(1u << n);
    }
    /* Ground-plane refinement (RenderParams::ground_node): if this tile's primary rays can only
     * reach the ground plane, all its hit points lie inside the tile's footprint on that plane
     * — the convex image of the pixel rectangle (+1 px all round; the AA taps reach 0.6 px),
     * provided all four corner rays meet the plane in front of the eye — and a node whose
     * shadow rectangle misses the footprint's bounding rectangle cannot occlude any of them. */
    bool primary_ground = false, ground_only = false, dark = false;
    const int gnode = P.ground_node;
    const uint32_t nn = P.n_nodes;
    if (gnode >= 0 && nn <= 32u && (pmask & (0xFFFFFFFFu >> (32u - nn))) == (1u << gnode)) {
        primary_ground = true;
        const D3 pos = ld3(P.cam.pos), ul = ld3(P.cam.up_left), du = ld3(P.cam_du), dv = ld3(P.cam_dv);
        const double gy = P.ground_y;
        bool ok = true;
        double fx0 = 0, fx1 = 0, fz0 = 0, fz1 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double sx = (k & 1) ? (double)(tx0 + kTileW + 1) : (double)(tx0 - 1);
            const double sy = (k & 2) ? (double)(ty1 + 2) : (double)(ty0 - 1);
            const double cfx = sx / P.cam.frame_width, cfy = sy / P.cam.frame_height;
            const D3 dir = ul + du * cfx + dv * cfy - pos;
            const double t = (gy - pos.y) / dir.y;
            ok = ok & (t > 0) & (t < 1e300);
            const double hx = pos.x + dir.x * t, hz = pos.z + dir.z * t;
            fx0 = k ? fmin(fx0, hx) : hx;
            fx1 = k ? fmax(fx1, hx) : hx;
            fz0 = k ? fmin(fz0, hz) : hz;
            fz1 = k ? fmax(fz1, hz) : hz;
        }
        const double padx = 1e-9 * (fabs(fx0) + fabs(fx1)), padz = 1e-9 * (fabs(fz0) + fabs(fz1));
        ok = ok & (fx0 <= fx1) & (fz0 <= fz1) & (fabs(fx0) < 1e300) & (fabs(fx1) < 1e300) & (fabs(fz0) < 1e300) & (fabs(fz1) < 1e300);
        if (ok) {
            KDbl rects_s = (KDbl)P.shadow_rects;
            for (uint32_t n = 0; n < nc; ++n) {
                KDbl sr = rects_s + 4 * n;
                if ((sr[1] < fx0 - padx) | (sr[0] > fx1 + padx) | (sr[3] < fz0 - padz) | (sr[2] > fz1 + padz)) smask0 &= ~(1u << n);
            }
            /* a CsgDiff(L, Sphere) node, or a Sphere node, that no shadow ray towards light 0 from the footprint can
             * hit (csg_void.h); the sphere test only for footprints within the reach its margin was derived for */
            PyramidCone scone;
            bool have_scone = false;
            const auto shadow_cone = [&]() {
                double sdir[4][3];
                footprint_dirs(V.light0, gy, fx0, fx1, fz0, fz1, sdir);
                return pyramid_cone(sdir);
            };
            for (uint32_t j = 0; j < V.n; ++j) {
                const VoidNode &vn = V.v[j];
                if (!((smask0 >> vn.node) & 1u) || !(vn.flags & 2u)) continue;
                if (!have_scone) { scone = shadow_cone(); have_scone = true; }
                if (pyramid_void(V.light0, scone, vn)) smask0 &= ~(1u << vn.node);
            }
            const bool in_reach = fmax(fabs(fx0), fabs(fx1)) + fmax(fabs(fz0), fabs(fz1)) + fabs(gy) <= S.reach;
            for (uint32_t j = 0; j < S.n; ++j) {
                const SphereNode &sn = S.s[j];
                if (!in_reach || !((smask0 >> sn.node) & 1u) || !(sn.flags & 2u)) continue;
                if (!have_scone) { scone = shadow_cone(); have_scone = true; }
                if (cone_misses_ball(V.light0, scone, sn.c, sn.rp)) smask0 &= ~(1u << sn.node);
            }
            /* dark tile: one node occludes every shadow ray from the footprint (csg_void.h, "Dark ground tiles"); asked
             * of the nodes whose shadow rectangle meets the footprint, whatever the tests above were allowed to do */
            if (Dp && Dp->n) { /* (a null table: the frame runs no dark test) */
                const DarkCull &D = *Dp;
                double sdir[4][3];
                footprint_dirs(V.light0, gy, fx0, fx1, fz0, fz1, sdir);
                const bool dark_reach = fmax(fabs(fx0), fabs(fx1)) + fmax(fabs(fz0), fabs(fz1)) + fabs(gy) <= D.reach;
                for (uint32_t j = 0; j < D.n; ++j) {
                    const DarkNode &dn = D.d[j];
                    if (dn.node >= nc) continue;
                    KDbl sr = rects_s + 4 * dn.node;
                    if ((sr[1] < fx0 - padx) | (sr[0] > fx1 + padx) | (sr[3] < fz0 - padz) | (sr[2] > fz1 + padz)) continue;
                    if (tile_dark_by(V.light0, sdir, dark_reach, dn)) dark = true;
                }
            }
        }
        ground_only = (smask0 & (0xFFFFFFFFu >> (32u - nn))) == (1u << gnode);
    }
    /* Sphere-interior tile (csg_void.h, "Sphere-interior tiles"): after every test above the primary mask holds ONE Sphere
     * node the host marked (SphereCull::interior), the ground plane and nothing else, every primary ray hits that sphere in
     * front of the ground, and nothing else can occlude the shadow rays.  Only tiles that keep such a sphere get here; its
     * radius comes from the node's own record (a scalar load). */
    bool interior = false;
    if (__builtin_expect(S.interior != 0u, 0) && nn >= 1u && nn <= 32u) { /* (unlikely: laid out behind the rest, which a frame
                                                                          * without the claim then runs as it did before) */
        const uint32_t live = pmask & (0xFFFFFFFFu >> (32u - nn));
        const uint32_t gbit = gnode >= 0 ? 1u << gnode : 0u;
        const uint32_t rest = live & ~gbit;
        if ((live & gbit) == gbit && rest && !(rest & (rest - 1u)) && (rest & S.interior)) {
            for (uint32_t j = 0; j < S.n; ++j) {
                const SphereNode &sn = S.s[j];
                if ((1u << sn.node) != rest) continue;
                if (!have_pcone) { pcone = primary_cone(); have_pcone = true; }
                const double R = ((NodeP)P.nodes)[sn.node].g.p[3];
                interior = sphere_interior_tile(P.cam.pos, pcone, S, j, R, V, smask0, nn, gnode, P.ground_y, P.n_lights != 0u);
            }
        }
    }
    out[0] = pmask;
    out[1] = smask0;
    out[2] = (primary_ground ? 1u : 0u) | (ground_only ? 2u : 0u) | (dark ? 4u : 0u) | (interior ? 8u : 0u);
    /* shadow masks of the further culled lights (second table): the same predicate as light 0's view-pyramid part */
    out[3] = 0;
    out[4] = out[5] = out[6] = 0xFFFFFFFFu;
    out[7] = 0;
    for (uint32_t l = 1; l < P.n_cull_lights; ++l) {
        const int *sl = P.light_side[l];
        const bool l_left = tx0 >= sl[0] && tx0 <= sl[1], l_right = sx1 >= sl[2] && sx1 <= sl[3];
        const bool l_top = ty0 >= sl[4] && ty0 <= sl[5], l_bottom = sy1 >= sl[6] && sy1 <= sl[7];
        uint32_t sm = 0xFFFFFFFFu;
        for (uint32_t n = 0; n < nc; ++n) {
            const int r0 = rects[4 * n + 0], r1 = rects[4 * n + 1], r2 = rects[4 * n + 2], r3 = rects[4 * n + 3];
            if ((l_left && r2 <= tx0) || (l_right && r0 >= sx1) || (l_top && r3 <= ty0) || (l_bottom && r1 >= sy1)) sm &= ~(1u << n);
        }
        out[3 + l] = sm;
    }
}
