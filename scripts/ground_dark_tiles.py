"""Dark ground tiles on the host: which 8x8 tiles of a frame the mask pre-pass may call dark — their primary rays reach
the ground plane only and every shadow ray towards light 0 is occluded by one node (chess2rt_amd/csrc/csg_void.h, "Dark
ground tiles", through its host build tests/libground_dark_check.so, which also runs the planner's dark_cull_of) — and a
per-ray check of that claim against the CPU oracle (tests/oracle_lib.py).

    python scripts/ground_dark_tiles.py [--scene tests/golden/scenes/lecture5.sdl] [--size 3840x2160 ...] [--check N]

prints the dark-tile counts per node and frame size; with --check N verifies in the oracle, for every pixel and all 5
taps of N dark tiles per node (0 = all), that the primary ray hits the ground before anything else and that the shadow
ray from p + N * 1e-6 towards light 0 gets a hit on the claimed node before the light.

"Primary-ground" is restated here from the nodes' screen rectangles less the tiles the silhouette and void tests drop
(scripts/sphere_cull_tiles.py, scripts/csg_void_tiles.py); the device also applies the hulls, so its count is a little
higher (tests/test_gpu_ground_dark.py compares the device's bits under the device's own primary-ground bit).
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
import sphere_cull_tiles as sc  # noqa: E402

MAX_DARK_NODES = 8  # csg_void.h: kMaxDarkNodes
KIND_SPHERE, KIND_CSG_DIFF = 0, 1


class DarkNodeC(C.Structure):  # csg_void.h: DarkNode
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3), ("c", C.c_double * 3), ("r", C.c_double),
                ("node", C.c_uint32), ("kind", C.c_uint32)]


class DarkCullC(C.Structure):  # csg_void.h: DarkCull
    _fields_ = [("n", C.c_uint32), ("pad", C.c_uint32), ("reach", C.c_double), ("eye_max", C.c_double),
                ("d", DarkNodeC * MAX_DARK_NODES)]


class DarkFrameC(C.Structure):  # tests/ground_dark_check.cpp: DarkFrame
    _fields_ = [("d", DarkCullC), ("light", C.c_double * 3), ("ground_y", C.c_double), ("ground_node", C.c_int32),
                ("n_cull", C.c_uint32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(ROOT, "tests", "libground_dark_check.so")
        if not os.path.exists(path):
            raise RuntimeError("not built: run `make tests/libground_dark_check.so`")
        L = C.CDLL(path)
        d3 = C.POINTER(C.c_double)
        L.c2rt_ground_dark_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(DarkFrameC)]
        L.c2rt_ground_dark_frame.restype = C.c_size_t
        L.c2rt_ground_dark_classify_tiles.argtypes = [d3, d3, d3, d3, C.c_double, C.c_double, C.c_size_t, C.c_void_p,
                                                      C.POINTER(DarkNodeC), d3, C.c_double, C.c_double, C.c_void_p]
        L.c2rt_ground_dark_classify_tiles.restype = None
        _lib = L
    return _lib


def dark_frame(desc, cam, opts, debug_cull=0):
    """DarkFrameC: the DarkCull the library hands the mask pre-pass for this frame (scene_plan.cpp: dark_cull_of, run
    by the planner itself), with light 0 and the ground."""
    out = DarkFrameC()
    got = lib().c2rt_ground_dark_frame(C.cast(desc, C.c_void_p), C.cast(C.pointer(cam), C.c_void_p),
                                       C.cast(C.pointer(opts), C.c_void_p), debug_cull, C.byref(out))
    if got != C.sizeof(DarkFrameC):
        raise RuntimeError("c2rt_ground_dark_frame: %d bytes, expected %d" % (got, C.sizeof(DarkFrameC)))
    return out


def with_radius(node, R_scale):
    """a copy of a CsgDiff DarkNode whose corner cut is placed as if the subtracted ball were R_scale times its size
    (the mutation test: below 1 the convex set reaches into the ball)"""
    k = DarkNodeC.from_buffer_copy(node)
    k.r = node.r * R_scale
    return k


def classify_tiles(cam, bounds, node, frame):
    """uint8 [len(bounds)]: 1 = every shadow ray of the tile's ground footprint is occluded by `node` (a DarkNodeC of
    frame.d); bounds = [(tx0, ty0, ty1)] (csg_void_tiles.tile_bounds)."""
    out = np.zeros(len(bounds), dtype=np.uint8)
    if not len(bounds):
        return out
    du = [cam.up_right[i] - cam.up_left[i] for i in range(3)]
    dv = [cam.down_left[i] - cam.up_left[i] for i in range(3)]
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.int32).reshape(-1, 3))
    lib().c2rt_ground_dark_classify_tiles(cv._a3(cam.pos), cv._a3(cam.up_left), cv._a3(du), cv._a3(dv), cam.frame_width,
                                          cam.frame_height, len(bounds), b.ctypes.data_as(C.c_void_p), C.byref(node),
                                          cv._a3(frame.light), frame.ground_y, frame.d.reach, out.ctypes.data_as(C.c_void_p))
    return out


def classify(cam, W, H, node, frame):
    """uint8 (tiles_y, tiles_x) over the full-frame tile grid"""
    tw, th = (W + 7) // 8, (H + 7) // 8
    bounds = [cv.tile_bounds(r, c, 0, H) for r in range(th) for c in range(tw)]
    return classify_tiles(cam, bounds, node, frame).reshape(th, tw)


def primary_ground_tiles(desc, cam, W, H):
    """bool (tiles_y, tiles_x): tiles no boxed node's screen rectangle keeps once the silhouette and void tests have
    dropped what they can — a subset of the device's primary-ground tiles (module docstring)."""
    keep_any = np.zeros(((H + 7) // 8, (W + 7) // 8), dtype=bool)
    rects = sc.boxed_rect_tiles(desc, cam, W, H)
    drops = {}
    reach, entries = sc.frame_sphere_cull(desc, cam) or (0.0, [])
    for e in entries:
        drops[e["node"]] = (sc.classify(desc, cam, W, H, e, reach) & 1) != 0
    for cand in cv.void_candidates(desc):
        drops[cand.node] = (cv.classify(desc, cam, W, H, cand) & 1) != 0
    for n, keep in rects.items():
        keep_any |= keep & ~drops[n] if n in drops else keep
    return ~keep_any


def dark_tiles(desc, cam, opts, W, H, debug_cull=0, mutate=None):
    """[(DarkNodeC, bool (tiles_y, tiles_x))]: per node of the frame's DarkCull, the primary-ground tiles it makes dark.
    mutate: DarkNodeC -> DarkNodeC applied before classifying (the mutation test)."""
    frame = dark_frame(desc, cam, opts, debug_cull)
    if not frame.d.n:
        return frame, []
    pg = primary_ground_tiles(desc, cam, W, H)
    out = []
    for j in range(frame.d.n):
        k = frame.d.d[j]
        k = mutate(k) if mutate else k
        out.append((k, (classify(cam, W, H, k, frame) != 0) & pg))
    return frame, out


def check_tile_bounds(desc, cam, W, H, node, bounds, light, ground):
    """Oracle, every ray of one dark tile, bounds = (tx0, ty0, ty1) as csg_void_tiles.tile_bounds has them: each
    primary ray (5 taps) hits the ground and no other node before it, and the shadow ray from p + N * 1e-6 towards
    light 0 (rt/shader.d:88) gets a hit on `node` before the light.  Returns the number of shadow rays checked;
    raises on a violation."""
    import oracle_lib
    from oracle_lib import OrcHit

    L = oracle_lib.lib()
    D = cv._fields(desc)
    o, d = (C.c_double * 3)(), (C.c_double * 3)()
    n_rays = 0
    tx0, ty0, ty1 = bounds
    for y in range(ty0, min(ty1 + 1, H)):
        for x in range(tx0, min(tx0 + 8, W)):
            for ox, oy in cv.TAPS:
                L.orc_screen_ray(C.byref(cam), x + ox, y + oy, o, d)
                gh = OrcHit()
                gh.dist = 1e99
                if not L.orc_node_intersect(desc, ground, o, d, C.byref(gh)):
                    raise AssertionError("primary ray (%g, %g) of a dark tile misses the ground" % (x + ox, y + oy))
                for n in range(D.n_nodes):
                    if n == ground:
                        continue
                    oh = OrcHit()
                    oh.dist = gh.dist
                    if L.orc_node_intersect(desc, n, o, d, C.byref(oh)):
                        raise AssertionError("primary ray (%g, %g) of a dark tile hits node %d" % (x + ox, y + oy, n))
                N = list(gh.normal)
                if N[0] * d[0] + N[1] * d[1] + N[2] * d[2] > 0:
                    N = [-v for v in N]
                frm = [gh.p[i] + N[i] * 1e-6 for i in range(3)]
                v = [light[i] - frm[i] for i in range(3)]
                dist = math.sqrt(sum(t * t for t in v))
                sh = OrcHit()
                sh.dist = dist
                if not L.orc_node_intersect(desc, node, cv._a3(frm), cv._a3([t / dist for t in v]), C.byref(sh)):
                    raise AssertionError("shadow ray from (%g, %g) is not occluded by node %d of a dark tile" % (x + ox, y + oy, node))
                if not sh.dist <= dist:
                    raise AssertionError("shadow ray from (%g, %g): node %d is hit behind the light" % (x + ox, y + oy, node))
                n_rays += 1
    return n_rays


def check_tiles(desc, cam, W, H, frame, node, tiles, sample=0, seed=0):
    """oracle-checks the dark tiles (bool grid) of one node, a seeded sample of them if sample > 0; -> (tiles, rays)"""
    todo = list(zip(*np.nonzero(tiles)))
    if sample and len(todo) > sample:
        rng = np.random.default_rng(seed)
        todo = [todo[i] for i in rng.choice(len(todo), size=sample, replace=False)]
    light = [frame.light[i] for i in range(3)]
    rays = sum(check_tile_bounds(desc, cam, W, H, node, cv.tile_bounds(int(ty), int(tx), 0, H), light, frame.ground_node)
               for ty, tx in todo)
    return len(todo), rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl"))
    ap.add_argument("--size", nargs="*", default=["3840x2160", "1920x1080", "640x480", "320x240"])
    ap.add_argument("--check", type=int, default=-1, help="oracle-check N dark tiles per node (0: all; default: none)")
    args = ap.parse_args()
    import chess2rt_amd as c2

    for size in args.size:
        W, H = (int(v) for v in size.split("x"))
        scene = c2.parseSceneFromFile(args.scene)
        scene.setFrameSize(W, H)
        cam = scene.beginFrame()
        opts = scene.renderOpts(taps=5)
        frame, per_node = dark_tiles(scene.desc, cam, opts, W, H)
        total = ((W + 7) // 8) * ((H + 7) // 8)
        union = np.zeros(((H + 7) // 8, (W + 7) // 8), dtype=bool)
        for _, t in per_node:
            union |= t
        print("%s %dx%d: %d tiles, %d dark (%.2f %%), %d nodes tested" % (os.path.basename(args.scene), W, H, total,
                                                                        int(union.sum()), 100.0 * union.sum() / total, len(per_node)))
        for k, t in per_node:
            print("  node %d (%s): %d dark tiles" % (k.node, "Sphere" if k.kind == KIND_SPHERE else "CsgDiff(Cube, Sphere)", int(t.sum())))
            if args.check >= 0:
                n, rays = check_tiles(scene.desc, cam, W, H, frame, k.node, t, args.check)
                print("    oracle: %d tiles, %d shadow rays, every one occluded by node %d before the light" % (n, rays, k.node))


if __name__ == "__main__":
    main()
