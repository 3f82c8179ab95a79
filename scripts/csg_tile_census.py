"""Ground-and-CsgOp tiles on the host: which 8x8 tiles of a frame the frame kernel hands to lean::csg_tile
(chess2rt_amd/csrc/c2rt_trace.inc) — the live primary mask is exactly {ground node, n}, the live shadow mask towards
light 0 a subset of that pair, in a frame with RenderParams::ground_fast, n a node the planner marked kNodeCsgTile
(scene_plan.cpp: plan_csg_tile_nodes, through its host build tests/libcsg_tile_check.so).  The mask words are the
planner's own classifier's (scripts/sphere_interior_tiles.py: Frame.classify_tiles, which restates the node loop of
tile_mask_entry); the pre-pass knows nothing of this path.

    python scripts/csg_tile_census.py [--scene tests/golden/scenes/lecture5.sdl] [--size 3840x2160 ...] [--check N]

prints, per frame size, the tiles the path takes per node and the other tiles left to the general path; with --check N
verifies in the oracle, for every pixel and all 5 taps of N claimed tiles per node (0 = all), that the primary ray's
closest node is the ground, n or nothing, and that the shadow ray from p + N * 1e-6 towards light 0 is hit by no node
other than those two before the light: the host's eligibility says nothing false.
"""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import csg_void_tiles as cv  # noqa: E402
import sphere_interior_tiles as si  # noqa: E402

NO_PATH = 1024  # C2RT_DEBUG_CULL bit 10: every tile to the general path

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(ROOT, "tests", "libcsg_tile_check.so")
        if not os.path.exists(path):
            raise RuntimeError("not built: run `make tests/libcsg_tile_check.so`")
        L = C.CDLL(path)
        L.c2rt_csg_tile_nodes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
        L.c2rt_csg_tile_nodes.restype = C.c_int64
        _lib = L
    return _lib


def eligible_nodes(desc, cam, opts, debug_cull=0):
    """(mask of the nodes csg_tile may take in this frame, the frame's ground node, the plan's kNodeCsgTile mask whatever
    the frame)"""
    ground, plan_mask = C.c_int32(-1), C.c_uint32(0)
    m = lib().c2rt_csg_tile_nodes(C.cast(desc, C.c_void_p), C.cast(C.pointer(cam), C.c_void_p), C.cast(C.pointer(opts), C.c_void_p),
                                  int(debug_cull), C.byref(ground), C.byref(plan_mask))
    if m < 0:
        raise RuntimeError("c2rt_csg_tile_nodes: the planner refused the scene")
    return int(m), int(ground.value), int(plan_mask.value)


def claim_from_masks(pm, sm, n_nodes, ground, eligible):
    """render_tile's condition on the first two mask words (arrays): -> the node csg_tile takes per tile, -1 for none"""
    pm, sm = np.asarray(pm, dtype=np.uint32), np.asarray(sm, dtype=np.uint32)
    node = np.full(pm.shape, -1, dtype=np.int32)
    if not eligible or ground < 0 or n_nodes > 32:
        return node
    live = np.uint32(0xFFFFFFFF >> (32 - n_nodes))
    gbit = np.uint32(1 << ground)
    p, s = pm & live, sm & live
    rest = p & ~gbit
    one = (rest != 0) & ((rest & (rest - np.uint32(1))) == 0)
    ok = ((p & gbit) != 0) & one & ((s & ~p) == 0) & ((rest & np.uint32(eligible)) != 0)
    # (a tile whose shadow mask is the ground alone is a ground-only tile only when its primary mask is too: not here)
    idx = np.zeros(pm.shape, dtype=np.int32)
    for n in range(n_nodes):
        idx[rest == np.uint32(1 << n)] = n
    node[ok] = idx[ok]
    return node


def claimed_tiles(desc, cam, opts, bounds, debug_cull=0):
    """-> (node per tile of `bounds`, -1 for none; pmask; smask0) as the frame kernel decides it"""
    eligible, ground, _ = eligible_nodes(desc, cam, opts, debug_cull)
    frame = si.Frame(desc, cam, opts, debug_cull)
    pm, sm, _, _ = frame.classify_tiles(bounds)
    if not frame.n_cull:
        return np.full(len(bounds), -1, dtype=np.int32), pm, sm
    return claim_from_masks(pm, sm, cv._fields(desc).n_nodes, ground, eligible), pm, sm


def check_tile(desc, cam, W, H, node, ground, bounds, light, n_lights):
    """Oracle, every sample of one claimed tile: the closest node is the ground, `node` or nothing, and no other node
    occludes the shadow ray.  -> (samples, samples on the CsgOp, samples on the ground); raises on a violation."""
    import oracle_lib
    from oracle_lib import OrcHit

    L = oracle_lib.lib()
    D = cv._fields(desc)
    o, d = (C.c_double * 3)(), (C.c_double * 3)()
    n_samples = n_csg = n_ground = 0
    tx0, ty0, ty1 = bounds
    for y in range(ty0, min(ty1 + 1, H)):
        for x in range(tx0, min(tx0 + 8, W)):
            for ox, oy in cv.TAPS:
                L.orc_screen_ray(C.byref(cam), x + ox, y + oy, o, d)
                best, closest = OrcHit(), -1
                best.dist = 1e99
                for n in range(D.n_nodes):
                    h = OrcHit()
                    h.dist = best.dist
                    if L.orc_node_intersect(desc, n, o, d, C.byref(h)):
                        best, closest = h, n
                if closest not in (-1, ground, node):
                    raise AssertionError("primary ray (%g, %g) of a claimed tile: closest node %d, not %d or %d" % (x + ox, y + oy, closest, ground, node))
                n_samples += 1
                n_csg += closest == node
                n_ground += closest == ground
                if closest < 0 or not n_lights:
                    continue
                N = list(best.normal)
                if N[0] * d[0] + N[1] * d[1] + N[2] * d[2] > 0:
                    N = [-v for v in N]
                frm = [best.p[i] + N[i] * 1e-6 for i in range(3)]
                v = [light[i] - frm[i] for i in range(3)]
                dist = math.sqrt(sum(t * t for t in v))
                sdir = cv._a3([t / dist for t in v])
                for n in range(D.n_nodes):
                    sh = OrcHit()
                    sh.dist = dist
                    if n not in (ground, node) and L.orc_node_intersect(desc, n, cv._a3(frm), sdir, C.byref(sh)):
                        raise AssertionError("shadow ray from (%g, %g) of a claimed tile is occluded by node %d" % (x + ox, y + oy, n))
    return n_samples, n_csg, n_ground


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl"))
    ap.add_argument("--size", nargs="*", default=["3840x2160", "1920x1080"])
    ap.add_argument("--check", type=int, default=-1, help="oracle-check N claimed tiles per node (0: all; default: none)")
    args = ap.parse_args()
    import chess2rt_amd as c2

    for size in args.size:
        W, H = (int(v) for v in size.split("x"))
        scene = c2.parseSceneFromFile(args.scene)
        scene.setFrameSize(W, H)
        cam = scene.beginFrame()
        opts = scene.renderOpts(taps=5)
        tw, th = (W + 7) // 8, (H + 7) // 8
        bounds = [cv.tile_bounds(r, c, 0, H) for r in range(th) for c in range(tw)]
        eligible, ground, plan_mask = eligible_nodes(scene.desc, cam, opts)
        node, pm, sm = claimed_tiles(scene.desc, cam, opts, bounds)
        frame = si.Frame(scene.desc, cam, opts)
        _, _, _, claim = frame.classify_tiles(bounds)
        gbit = np.uint32(1 << ground) if ground >= 0 else np.uint32(0)
        n_nodes = cv._fields(scene.desc).n_nodes
        live = np.uint32(0xFFFFFFFF >> (32 - n_nodes)) if 0 < n_nodes <= 32 else np.uint32(0xFFFFFFFF)
        ground_tiles = (pm & live & ~gbit) == 0
        interior = (claim & 1) != 0
        rest = ~ground_tiles & ~interior & (node < 0)
        print("%s %dx%d: %d tiles; eligible nodes 0x%x (the plan's 0x%x), ground node %d; %d tiles take csg_tile (%.2f %%), "
              "%d other tiles stay on the general path" % (os.path.basename(args.scene), W, H, node.size, eligible, plan_mask, ground,
                                                          int((node >= 0).sum()), 100.0 * (node >= 0).sum() / node.size, int(rest.sum())))
        for n in sorted(set(int(v) for v in node[node >= 0])):
            mine = np.nonzero(node == n)[0]
            print("  node %d: %d tiles" % (n, len(mine)))
            if args.check >= 0:
                todo = mine
                if args.check and len(todo) > args.check:
                    todo = np.random.default_rng(0).choice(todo, size=args.check, replace=False)
                tot = [0, 0, 0]
                for t in todo:
                    r = check_tile(scene.desc, cam, W, H, n, ground, bounds[int(t)], frame.light, frame.n_lights)
                    tot = [a + b for a, b in zip(tot, r)]
                print("    oracle: %d tiles, %d samples: %d on node %d, %d on the ground, %d on nothing; no shadow ray meets another node"
                      % (len(todo), tot[0], tot[1], n, tot[2], tot[0] - tot[1] - tot[2]))


if __name__ == "__main__":
    main()
