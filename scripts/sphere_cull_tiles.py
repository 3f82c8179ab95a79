"""Sphere-silhouette culling on the host: which 8x8 tiles of a frame the mask pre-pass may drop a Sphere node from
(chess2rt_amd/csrc/csg_void.h: cone_misses_ball, through its host build tests/libsphere_cull_check.so), and a per-ray
check of that claim against the CPU oracle (scripts/csg_void_tiles.py: check_tile_bounds).

    python scripts/sphere_cull_tiles.py [--scene tests/golden/scenes/lecture5.sdl] [--size 3840x2160 ...] [--check N]

prints, per sphere node and frame size, the tiles its screen rectangle keeps (the projected box + 2 px, as
cull_rect_of; the hull is not restated on the host), those of them the cone test drops from the primary mask, the
tiles that thereby keep no boxed node's rectangle but the ground (an upper bound of "become primary-ground": the hull
and the CsgDiff void test drop more), and the tiles whose ground footprint the shadow cone clears.  The device's own
class counts (hull and void test included) come from tests/sphere_cull_device.py on the GPU.
"""
import argparse
import ctypes as C
import math
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import csg_void_tiles as cv  # noqa: E402

MAX_SPHERE_NODES = 4  # csg_void.h: kMaxSphereNodes

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(ROOT, "tests", "libsphere_cull_check.so")
        if not os.path.exists(path):
            raise RuntimeError("not built: run `make tests/libsphere_cull_check.so`")
        L = C.CDLL(path)
        d3 = C.POINTER(C.c_double)
        L.c2rt_sphere_classify_tiles.argtypes = [d3, d3, d3, d3, C.c_double, C.c_double, C.c_size_t, C.c_void_p, d3, C.c_double,
                                                 C.c_uint, d3, C.c_double, C.c_double, C.c_void_p]
        L.c2rt_sphere_classify_tiles.restype = None
        L.c2rt_sphere_margin.argtypes = [C.c_double, C.c_double]
        L.c2rt_sphere_margin.restype = C.c_double
        L.c2rt_cone_misses_ball.argtypes = [d3, d3, d3, C.c_double, d3, C.POINTER(C.c_int)]
        L.c2rt_cone_misses_ball.restype = C.c_int
        _lib = L
    return _lib


class Ball(namedtuple("Ball", "node c R flags")):
    """A Sphere node the library tests (scene_plan.cpp, plan_sphere_nodes): world centre, radius, and the flags it may get
    (bit 0 primary, bit 1 shadow towards light 0 where the scene has a ground and a finite light 0)."""


def sphere_candidates(desc):
    """[Ball], restated from scene_plan.cpp (plan_sphere_nodes): the first kMaxSphereNodes nodes below kMaxCullNodes whose
    root geometry is a finite Sphere of positive radius under an identity matrix (offset allowed) and that are boxed
    (bound and padded box finite, as for every node: csg_void_tiles.void_candidates)."""
    desc = cv._fields(desc)
    gn, _ = cv.ground_of(desc)
    light = [desc.light_pos[i] for i in range(3)] if desc.n_lights else None
    out = []
    for n in range(min(desc.n_nodes, cv.MAX_CULL_NODES)):
        if len(out) >= MAX_SPHERE_NODES:
            break
        g = desc.node_geom[n]
        m, inv, tinv, off = cv._node_tr(desc, n)
        if desc.geom_type[g] != cv.GEOM_SPHERE or not (m == inv == tinv == cv._IDENTITY):
            continue
        if not cv._geom_finite(desc, g):
            continue
        p = [desc.geom_param[4 * g + i] for i in range(4)]
        if not p[3] > 0:
            continue
        br = abs(p[3])
        bmag = abs(p[0]) + abs(p[1]) + abs(p[2]) + br
        rp = br * (1 + 1e-6) + 1e-6 * bmag + 1e-9
        if not (math.isfinite(rp) and rp * rp < 1e300) or not cv._finite(*off):
            continue
        lo = [p[i] - br for i in range(3)]
        hi = [p[i] + br for i in range(3)]
        mag = sum(max(abs(lo[i]), abs(hi[i])) for i in range(3))
        pad = 1e-6 * (2 * br) + 1e-6 * mag + 1e-9 + 4e-6 * math.sqrt(3.0)
        c = [p[j] + off[j] for j in range(3)]
        if not cv._finite(pad, *c, *[lo[j] - pad + off[j] for j in range(3)], *[hi[j] + pad + off[j] for j in range(3)]):
            continue
        flags = 1
        if gn is not None and light is not None and cv._finite(*light):
            flags |= 2
        out.append(Ball(n, c, p[3], flags))
    return out


def frame_sphere_cull(desc, cam, debug_cull=0, flags_mask=3):
    """(reach, [dict(node, c, rp, flags)]): the SphereCull the library hands the mask pre-pass for this camera
    (scene_plan.cpp, sphere_cull_of), operation for operation.  None: the frame culls nothing."""
    desc = cv._fields(desc)
    if debug_cull & 1:
        return None
    if debug_cull & 8:
        flags_mask = 0
    gn, gy = cv.ground_of(desc)
    if debug_cull & 2:
        gn = None
    n_cull_lights = 0 if debug_cull & 4 else min(desc.n_lights, cv.MAX_CULL_LIGHTS)
    balls = sphere_candidates(desc)
    scale = 0.0
    for b in balls:
        scale = max(scale, b.R + max(abs(b.c[0]), abs(b.c[1]), abs(b.c[2])))
    scale += max(abs(cam.pos[0]), abs(cam.pos[1]), abs(cam.pos[2]))
    if desc.n_lights:
        scale += max(abs(desc.light_pos[0]), abs(desc.light_pos[1]), abs(desc.light_pos[2]))
    if not math.isfinite(scale) or not flags_mask & 3:
        return 0.0, []
    out = []
    for b in balls:
        rp = b.R + lib().c2rt_sphere_margin(scale, b.R)
        if not math.isfinite(rp):
            continue
        flags = b.flags
        if n_cull_lights == 0 or gn is None or not desc.n_lights:
            flags &= ~2
        if flags & 2:
            Ly = desc.light_pos[1]
            h = Ly - gy
            tol = 1e-6 + 1e-9 * (abs(Ly) + abs(b.c[1]) + rp)
            if not ((h > 0 and b.c[1] + rp < Ly - tol) or (h < 0 and b.c[1] - rp > Ly + tol)):
                flags &= ~2
        flags &= flags_mask
        if flags:
            out.append(dict(node=b.node, c=list(b.c), rp=rp, flags=flags))
    return scale, out


def classify_tiles(desc, cam, bounds, entry, reach):
    """uint8 [len(bounds)]: bit 0 = the primary cone misses the padded ball, bit 1 = the shadow cone of the tile's
    ground footprint does; bounds = [(tx0, ty0, ty1)] (csg_void_tiles.tile_bounds), entry from frame_sphere_cull."""
    desc = cv._fields(desc)
    out = np.zeros(len(bounds), dtype=np.uint8)
    if not len(bounds):
        return out
    _, gy = cv.ground_of(desc)
    light = [desc.light_pos[i] for i in range(3)] if desc.n_lights else [0.0, 0.0, 0.0]
    du = [cam.up_right[i] - cam.up_left[i] for i in range(3)]
    dv = [cam.down_left[i] - cam.up_left[i] for i in range(3)]
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.int32).reshape(-1, 3))
    lib().c2rt_sphere_classify_tiles(cv._a3(cam.pos), cv._a3(cam.up_left), cv._a3(du), cv._a3(dv), cam.frame_width,
                                     cam.frame_height, len(bounds), b.ctypes.data_as(C.c_void_p), cv._a3(entry["c"]),
                                     entry["rp"], entry["flags"], cv._a3(light), gy if gy is not None else 0.0, reach,
                                     out.ctypes.data_as(C.c_void_p))
    return out


def classify(desc, cam, W, H, entry, reach):
    """uint8 (tiles_y, tiles_x) over the full-frame tile grid"""
    tw, th = (W + 7) // 8, (H + 7) // 8
    bounds = [cv.tile_bounds(r, c, 0, H) for r in range(th) for c in range(tw)]
    return classify_tiles(desc, cam, bounds, entry, reach).reshape(th, tw)


def boxed_rect_tiles(desc, cam, W, H):
    """{node: bool (tiles_y, tiles_x)} for the Sphere / Cube / CsgDiff nodes of the scene: the tiles their screen
    rectangles meet (boxes without the library's padding, which is a fraction of a pixel)."""
    D = cv._fields(desc)
    out = {}
    cands = {c.node: (c.lo, c.hi) for c in cv.void_candidates(desc)}
    for b in sphere_candidates(desc):
        cands[b.node] = ([b.c[i] - b.R for i in range(3)], [b.c[i] + b.R for i in range(3)])
    for n in range(min(D.n_nodes, cv.MAX_CULL_NODES)):
        if n in cands:
            out[n] = cv.node_rect_tiles(cam, W, H, *cands[n])
    return out


def table(desc, cam, W, H):
    """rows of step 0's table: per sphere node (node, rectangle tiles, cone-dropped, thereby ground-only rectangle,
    shadow-cleared among the frame's tiles), and the frame's totals"""
    reach, entries = frame_sphere_cull(desc, cam)
    rects = boxed_rect_tiles(desc, cam, W, H)
    rows = []
    any_before = np.zeros(((H + 7) // 8, (W + 7) // 8), dtype=bool)
    any_after = any_before.copy()
    drops = {}
    for e in entries:
        cls = classify(desc, cam, W, H, e, reach)
        drops[e["node"]] = cls
    for n, keep in rects.items():
        any_before |= keep
        any_after |= keep & ~((drops[n] & 1) != 0) if n in drops else keep
    for e in entries:
        n = e["node"]
        keep = rects[n]
        dropped = keep & ((drops[n] & 1) != 0)
        others = np.zeros_like(keep)
        for k, r in rects.items():
            if k != n:
                others |= r & ~((drops[k] & 1) != 0) if k in drops else r
        rows.append((n, int(keep.sum()), int(dropped.sum()), int((dropped & ~others).sum()), int(((drops[n] & 2) != 0).sum())))
    return rows, int(any_before.sum()), int(any_after.sum()), any_before.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl"))
    ap.add_argument("--size", nargs="*", default=["3840x2160", "1920x1080", "640x480"])
    ap.add_argument("--check", type=int, default=-1, help="oracle-check N dropped tiles per node (0: all; default: none)")
    args = ap.parse_args()
    import chess2rt_amd as c2

    for size in args.size:
        W, H = (int(v) for v in size.split("x"))
        scene = c2.parseSceneFromFile(args.scene)
        scene.setFrameSize(W, H)
        cam = scene.beginFrame()
        desc = scene.desc
        rows, before, after, total = table(desc, cam, W, H)
        print("%s %dx%d: %d tiles; tiles with an object rectangle %d (%.2f %%) -> %d (%.2f %%) after the cone test: "
              "%d tiles (%.2f %% of the frame) change class" % (os.path.basename(args.scene), W, H, total, before,
                                                              100.0 * before / total, after, 100.0 * after / total,
                                                              before - after, 100.0 * (before - after) / total))
        for n, keep, dropped, alone, shadow in rows:
            print("  node %d: rectangle %d tiles, cone drops %d (%.1f %%), %d of them left to the ground; shadow cone clear on "
                  "%d tiles of the frame" % (n, keep, dropped, 100.0 * dropped / max(keep, 1), alone, shadow))
        if args.check >= 0:
            gn, _ = cv.ground_of(desc)
            light = [cv._fields(desc).light_pos[i] for i in range(3)]
            reach, entries = frame_sphere_cull(desc, cam)
            for e in entries:
                cls = classify(desc, cam, W, H, e, reach)
                tiles = list(zip(*np.nonzero(cls)))
                if args.check:
                    rng = np.random.default_rng(0)
                    tiles = [tiles[i] for i in rng.choice(len(tiles), size=min(args.check, len(tiles)), replace=False)]
                rays = sum(cv.check_tile(desc, cam, W, H, e["node"], int(ty), int(tx), int(cls[ty, tx]), light, gn) for ty, tx in tiles)
                print("  oracle: node %d, %d dropped tiles, %d rays checked, none hits it" % (e["node"], len(tiles), rays))


if __name__ == "__main__":
    main()
