"""Sphere-interior tiles on the host: which 8x8 tiles of a frame the mask pre-pass may hand to lean::sphere_tile — every
primary ray's closest hit lies on ONE Sphere node and no other node can occlude the shadow rays towards light 0
(chess2rt_amd/csrc/csg_void.h, "Sphere-interior tiles", through its host build tests/libsphere_interior_check.so, which
also runs the planner's fill_params / void_cull_of / sphere_cull_of and restates the node loop of tile_mask_entry) — and
a per-sample check of that claim against the CPU oracle (tests/oracle_lib.py).

    python scripts/sphere_interior_tiles.py [--scene tests/golden/scenes/lecture5.sdl] [--size 3840x2160 ...] [--check N]

prints, per frame size, the tiles claimed per node, their share of the frame and how many tiles the shadow condition
alone refused; with --check N verifies in the oracle, for every pixel and all 5 taps of N claimed tiles per node (0 =
all), that the primary ray's closest node is the claimed one and that the shadow ray from p + N * 1e-6 towards light 0 is
hit by no other node before the light.
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

ANY_SIZE = 256  # C2RT_DEBUG_CULL bit 8: the claim whatever the frame's size

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(ROOT, "tests", "libsphere_interior_check.so")
        if not os.path.exists(path):
            raise RuntimeError("not built: run `make tests/libsphere_interior_check.so`")
        L = C.CDLL(path)
        L.c2rt_si_new.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.c2rt_si_new.restype = C.c_void_p
        L.c2rt_si_free.argtypes = [C.c_void_p]
        L.c2rt_si_free.restype = None
        L.c2rt_si_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
        L.c2rt_si_info.restype = None
        L.c2rt_si_classify.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.c2rt_si_classify.restype = None
        _lib = L
    return _lib


class Frame:
    """The planner's view of one frame (scene_plan.cpp: fill_params, void_cull_of, sphere_cull_of) under C2RT_DEBUG_CULL =
    debug_cull: interior (SphereCull::interior), nodes (SphereCull::s[].node), n_cull, ground_node, n_lights, light."""

    def __init__(self, desc, cam, opts, debug_cull=0):
        self.h = lib().c2rt_si_new(C.cast(desc, C.c_void_p), C.cast(C.pointer(cam), C.c_void_p), C.cast(C.pointer(opts), C.c_void_p),
                                   debug_cull)
        if not self.h:
            raise RuntimeError("c2rt_si_new: the planner refused the scene")
        info, light = (C.c_int32 * 9)(), (C.c_double * 3)()
        lib().c2rt_si_info(self.h, info, light)
        self.interior = info[0] & 0xFFFFFFFF
        self.nodes = [info[5 + j] for j in range(info[1])]
        self.n_cull, self.ground_node, self.n_lights = info[2], info[3], info[4]
        self.light = list(light)

    def __del__(self):
        if getattr(self, "h", None):
            lib().c2rt_si_free(self.h)
            self.h = None

    def classify_tiles(self, bounds, r_scale=1.0):
        """(pmask, smask0, node, claim) arrays over bounds = [(tx0, ty0, ty1)] (csg_void_tiles.tile_bounds): the first two
        mask words as tile_mask_entry's node loop leaves them, the claimed sphere's node (-1: none), and claim bit 0 =
        sphere-interior (the device's bit 3 of the third word), bit 1 = the claim without its shadow condition.
        r_scale: the mutation test's inflated ball."""
        n = len(bounds)
        pm, sm = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        node, claim = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.uint8)
        if n:
            b = np.ascontiguousarray(np.asarray(bounds, dtype=np.int32).reshape(-1, 3))
            lib().c2rt_si_classify(self.h, n, b.ctypes.data_as(C.c_void_p), float(r_scale), pm.ctypes.data_as(C.c_void_p),
                                   sm.ctypes.data_as(C.c_void_p), node.ctypes.data_as(C.c_void_p), claim.ctypes.data_as(C.c_void_p))
        return pm, sm, node, claim

    def classify(self, W, H, r_scale=1.0):
        """(node, claim) as (tiles_y, tiles_x) grids over the full frame"""
        tw, th = (W + 7) // 8, (H + 7) // 8
        bounds = [cv.tile_bounds(r, c, 0, H) for r in range(th) for c in range(tw)]
        _, _, node, claim = self.classify_tiles(bounds, r_scale)
        return node.reshape(th, tw), claim.reshape(th, tw)


def check_tile_bounds(desc, cam, W, H, node, bounds, light, n_lights):
    """Oracle, every sample of one claimed tile, bounds = (tx0, ty0, ty1): the primary ray (5 taps) hits `node` and no
    other node at or before that distance in the reference's order (a later node wins a tie: `dist <= best`), and — with a
    light — the shadow ray from p + N * 1e-6 towards light 0 (rt/shader.d:88) is hit by no OTHER node before the light.
    Returns (samples, self-shadowed samples); raises on a violation."""
    import oracle_lib
    from oracle_lib import OrcHit

    L = oracle_lib.lib()
    D = cv._fields(desc)
    o, d = (C.c_double * 3)(), (C.c_double * 3)()
    n_samples = n_self = 0
    tx0, ty0, ty1 = bounds
    for y in range(ty0, min(ty1 + 1, H)):
        for x in range(tx0, min(tx0 + 8, W)):
            for ox, oy in cv.TAPS:
                L.orc_screen_ray(C.byref(cam), x + ox, y + oy, o, d)
                # Scene.intersect: every node in file order against the running distance
                best, closest = OrcHit(), -1
                best.dist = 1e99
                for n in range(D.n_nodes):
                    h = OrcHit()
                    h.dist = best.dist
                    if L.orc_node_intersect(desc, n, o, d, C.byref(h)):
                        best, closest = h, n
                if closest != node:
                    raise AssertionError("primary ray (%g, %g) of a claimed tile: closest node %d, claimed %d" % (x + ox, y + oy, closest, node))
                n_samples += 1
                if not n_lights:
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
                    if L.orc_node_intersect(desc, n, cv._a3(frm), sdir, C.byref(sh)):
                        if n != node:
                            raise AssertionError("shadow ray from (%g, %g) of a claimed tile is occluded by node %d" % (x + ox, y + oy, n))
                        n_self += 1
    return n_samples, n_self


def check_tiles(desc, cam, W, H, frame, node_grid, claim_grid, node, sample=0, seed=0):
    """oracle-checks the claimed tiles of one node, a seeded sample of them if sample > 0; -> (tiles, samples, self-shadowed)"""
    todo = list(zip(*np.nonzero(((claim_grid & 1) != 0) & (node_grid == node))))
    if sample and len(todo) > sample:
        rng = np.random.default_rng(seed)
        todo = [todo[i] for i in rng.choice(len(todo), size=sample, replace=False)]
    samples = selfs = 0
    for ty, tx in todo:
        a, b = check_tile_bounds(desc, cam, W, H, node, cv.tile_bounds(int(ty), int(tx), 0, H), frame.light, frame.n_lights)
        samples += a
        selfs += b
    return len(todo), samples, selfs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl"))
    ap.add_argument("--size", nargs="*", default=["3840x2160", "1920x1080", "640x480"])
    ap.add_argument("--check", type=int, default=-1, help="oracle-check N claimed tiles per node (0: all; default: none)")
    args = ap.parse_args()
    import chess2rt_amd as c2

    for size in args.size:
        W, H = (int(v) for v in size.split("x"))
        scene = c2.parseSceneFromFile(args.scene)
        scene.setFrameSize(W, H)
        cam = scene.beginFrame()
        opts = scene.renderOpts(taps=5)
        shipped = Frame(scene.desc, cam, opts).interior != 0  # frames below six million samples go without (sphere_cull_of)
        frame = Frame(scene.desc, cam, opts, ANY_SIZE)
        node, claim = frame.classify(W, H)
        total = node.size
        claimed = (claim & 1) != 0
        shadow_refused = ((claim & 2) != 0) & ~claimed
        print("%s %dx%d: %d tiles, %d sphere-interior (%.2f %% of the frame); the shadow condition alone refused %d; eligible "
              "nodes 0x%x; a 5-tap frame of this size %s" % (os.path.basename(args.scene), W, H, total, int(claimed.sum()),
                                                            100.0 * claimed.sum() / total, int(shadow_refused.sum()), frame.interior,
                                                            "takes the path" if shipped else "is too small to take the path"))
        for n in frame.nodes:
            if not (frame.interior >> n) & 1:
                continue
            mine = claimed & (node == n)
            print("  node %d: %d tiles (%.2f %%), %d more refused by the shadow condition" %
                  (n, int(mine.sum()), 100.0 * mine.sum() / total, int((shadow_refused & (node == n)).sum())))
            if args.check >= 0:
                t, s, selfs = check_tiles(scene.desc, cam, W, H, frame, node, claim, n, args.check)
                print("    oracle: %d tiles, %d samples: closest node %d on every one; %d shadow rays hit the sphere itself, none "
                      "another node" % (t, s, n, selfs))


if __name__ == "__main__":
    main()
