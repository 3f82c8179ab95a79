"""CsgDiff void tiles on the host: which 8x8 tiles of a frame the mask pre-pass may drop a CsgDiff(L, Sphere) node
from (chess2rt_amd/csrc/csg_void.h, through its host build tests/libcsg_void_check.so), and a per-ray check of that
claim against the CPU oracle (tests/oracle_lib.py).

    python scripts/csg_void_tiles.py [--scene tests/golden/scenes/lecture5.sdl] [--size 3840x2160] [--check N]

prints, per candidate node, the share of the tiles whose rectangle keeps the node (its pixel bounding box
of the projected box, as cull_rect_of) that come out primary-void / shadow-void, and with --check N verifies
every primary ray (5 taps) and every ground shadow ray of N void tiles (0 = all) in the oracle.
"""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GEOM_PLANE, GEOM_SPHERE, GEOM_CUBE, GEOM_DIFF = 0, 1, 2, 5
TAPS = ((0.0, 0.0), (0.3, 0.3), (0.6, 0.0), (0.0, 0.6), (0.6, 0.6))  # rt/renderer.d:235-242

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(ROOT, "tests", "libcsg_void_check.so")
        if not os.path.exists(path):
            raise RuntimeError("not built: run `make tests/libcsg_void_check.so`")
        L = C.CDLL(path)
        d3 = C.POINTER(C.c_double)
        L.c2rt_void_classify.argtypes = [d3, d3, d3, d3, C.c_double, C.c_double, C.c_int, C.c_int, d3, d3, d3,
                                         C.c_double, C.c_uint, d3, C.c_double, C.c_void_p]
        L.c2rt_void_classify.restype = None
        L.c2rt_void_margin.argtypes = [C.c_double]
        L.c2rt_void_margin.restype = C.c_double
        _lib = L
    return _lib


def _a3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def _fields(desc):
    return desc.contents if hasattr(desc, "contents") else desc


def void_candidates(desc):
    """[(node, lo, hi, centre, R)] for the nodes the library tests: CsgDiff(Cube | Sphere, Sphere) under an identity
    matrix (offset allowed), box = the left child's box plus the library's pad (c2rt_api.cpp, node boxes)."""
    desc = _fields(desc)
    out = []
    for n in range(desc.n_nodes):
        g = desc.node_geom[n]
        if desc.geom_type[g] != GEOM_DIFF:
            continue
        tr = [desc.node_transform[30 * n + i] for i in range(30)]
        if tr[0:9] != [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0] or tr[9:18] != tr[0:9]:
            continue
        off = tr[27:30]
        l, r = desc.geom_child[2 * g], desc.geom_child[2 * g + 1]
        if l == r or desc.geom_type[r] != GEOM_SPHERE or desc.geom_type[l] not in (GEOM_SPHERE, GEOM_CUBE):
            continue
        pl = [desc.geom_param[4 * l + i] for i in range(4)]
        pr = [desc.geom_param[4 * r + i] for i in range(4)]
        if not pr[3] > 0:
            continue
        e = abs(pl[3]) if desc.geom_type[l] == GEOM_SPHERE else abs(pl[3]) * 0.5
        lo = [pl[i] - e for i in range(3)]
        hi = [pl[i] + e for i in range(3)]
        mag = sum(max(abs(lo[i]), abs(hi[i])) for i in range(3))
        pad = 1e-6 * (2 * e) + 1e-6 * mag + 1e-9 + 4e-6
        out.append((n, [lo[i] - pad + off[i] for i in range(3)], [hi[i] + pad + off[i] for i in range(3)],
                    [pr[i] + off[i] for i in range(3)], pr[3]))
    return out


def ground_of(desc):
    """(node, y) of the first Plane node under an identity matrix with zero offset, or (None, None)."""
    desc = _fields(desc)
    for n in range(desc.n_nodes):
        g = desc.node_geom[n]
        tr = [desc.node_transform[30 * n + i] for i in range(30)]
        if desc.geom_type[g] == GEOM_PLANE and tr[0:9] == [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0] and tr[27:30] == [0, 0, 0]:
            return n, desc.geom_param[4 * g]
    return None, None


def classify(desc, cam, W, H, cand, r_override=None):
    """uint8 (tiles_y, tiles_x): bit 0 primary-void, bit 1 shadow-void (towards light 0 from the ground footprint)."""
    n, lo, hi, c, R = cand
    desc = _fields(desc)
    light = [desc.light_pos[i] for i in range(3)] if desc.n_lights else [0.0, 0.0, 0.0]
    scale = R + max(abs(x) for x in c) + max(abs(x) for x in cam.pos) + (max(abs(x) for x in light) if desc.n_lights else 0)
    rm = (R if r_override is None else r_override) - lib().c2rt_void_margin(scale)
    flags = 1
    gn, gy = ground_of(desc)
    if gn is not None and desc.n_lights:
        h = light[1] - gy
        tol = 1e-6 + 1e-9 * (abs(light[1]) + abs(lo[1]) + abs(hi[1]))
        if (h > 0 and hi[1] < light[1] - tol) or (h < 0 and lo[1] > light[1] + tol):
            flags |= 2
    tw, th = (W + 7) // 8, (H + 7) // 8
    out = np.zeros((th, tw), dtype=np.uint8)
    if not rm > 0:
        return out
    du = [cam.up_right[i] - cam.up_left[i] for i in range(3)]
    dv = [cam.down_left[i] - cam.up_left[i] for i in range(3)]
    lib().c2rt_void_classify(_a3(cam.pos), _a3(cam.up_left), _a3(du), _a3(dv), cam.frame_width, cam.frame_height, W, H,
                             _a3(lo), _a3(hi), _a3(c), rm * rm, flags, _a3(light), gy if gy is not None else 0.0,
                             out.ctypes.data_as(C.c_void_p))
    return out


def node_rect_tiles(cam, W, H, lo, hi):
    """bool (tiles_y, tiles_x): tiles that the node's screen rectangle (projected box + 2 px) meets; all if a corner
    is at or behind the eye."""
    tw, th = (W + 7) // 8, (H + 7) // 8
    pos = np.array(cam.pos)
    du = np.array(cam.up_right) - np.array(cam.up_left)
    dv = np.array(cam.down_left) - np.array(cam.up_left)
    ul = np.array(cam.up_left) - pos
    M = np.stack([du, dv, ul], axis=1)
    xs, ys = [], []
    for k in range(8):
        w = np.array([hi[0] if k & 1 else lo[0], hi[1] if k & 2 else lo[1], hi[2] if k & 4 else lo[2]]) - pos
        a, b, l = np.linalg.solve(M, w)
        if not l > 1e-9:
            return np.ones((th, tw), dtype=bool)
        xs.append(a / l * cam.frame_width)
        ys.append(b / l * cam.frame_height)
    x0, x1 = math.floor(min(xs)) - 2, math.ceil(max(xs)) + 3
    y0, y1 = math.floor(min(ys)) - 2, math.ceil(max(ys)) + 3
    tx = np.arange(tw) * 8
    ty = np.arange(th) * 8
    cx = (tx + 8 > x0) & (tx < x1)
    cy = (ty + 8 > y0) & (ty < y1)
    return cy[:, None] & cx[None, :]


def check_tile(desc, cam, W, H, node, ty, tx, bits, light, ground):
    """Oracle, every ray of one void tile: primary rays (5 taps) miss the node; with bit 1, for primary rays that hit
    the ground, the shadow ray towards light 0 (from p + N*1e-6, rt/shader.d:88) gets no hit on the node before the
    light.  Returns the number of rays checked; raises on a violation."""
    import oracle_lib
    from oracle_lib import OrcHit

    L = oracle_lib.lib()
    o, d = (C.c_double * 3)(), (C.c_double * 3)()
    n_rays = 0
    for y in range(ty * 8, min(ty * 8 + 8, H)):
        for x in range(tx * 8, min(tx * 8 + 8, W)):
            for ox, oy in TAPS:
                L.orc_screen_ray(C.byref(cam), x + ox, y + oy, o, d)
                if bits & 1:
                    hit = OrcHit()
                    hit.dist = 1e99
                    if L.orc_node_intersect(desc, node, o, d, C.byref(hit)):
                        raise AssertionError("primary ray (%g, %g) hits node %d of a void tile" % (x + ox, y + oy, node))
                    n_rays += 1
                if bits & 2 and ground is not None:
                    gh = OrcHit()
                    gh.dist = 1e99
                    if not L.orc_node_intersect(desc, ground, o, d, C.byref(gh)):
                        continue
                    N = list(gh.normal)
                    if N[0] * d[0] + N[1] * d[1] + N[2] * d[2] > 0:
                        N = [-v for v in N]
                    frm = [gh.p[i] + N[i] * 1e-6 for i in range(3)]
                    v = [light[i] - frm[i] for i in range(3)]
                    dist = math.sqrt(sum(t * t for t in v))
                    sh = OrcHit()
                    sh.dist = dist
                    if L.orc_node_intersect(desc, node, _a3(frm), _a3([t / dist for t in v]), C.byref(sh)):
                        raise AssertionError("shadow ray from (%g, %g) hits node %d of a shadow-void tile" % (x + ox, y + oy, node))
                    n_rays += 1
    return n_rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl"))
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--check", type=int, default=-1, help="oracle-check N void tiles (0: all; default: none)")
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    import chess2rt_amd as c2

    scene = c2.parseSceneFromFile(args.scene)
    scene.setFrameSize(W, H)
    cam = scene.beginFrame()
    desc = scene.desc
    gn, _ = ground_of(desc)
    light = [_fields(desc).light_pos[i] for i in range(3)]
    for cand in void_candidates(desc):
        node, lo, hi = cand[0], cand[1], cand[2]
        cls = classify(desc, cam, W, H, cand)
        keep = node_rect_tiles(cam, W, H, lo, hi)
        nk = int(keep.sum())
        pv = int(((cls & 1) != 0)[keep].sum())
        sv = int(((cls & 3) == 3)[keep].sum())
        print("%s %dx%d node %d: %d of %d tiles (%.1f %%) keep it by rectangle; primary-void %d (%.1f %% of them), "
              "primary- and shadow-void %d (%.1f %%)" % (os.path.basename(args.scene), W, H, node, nk, keep.size,
                                                        100.0 * nk / keep.size, pv, 100.0 * pv / max(nk, 1), sv,
                                                        100.0 * sv / max(nk, 1)))
        if args.check >= 0:
            tiles = list(zip(*np.nonzero(cls)))
            if args.check:
                rng = np.random.default_rng(0)
                tiles = [tiles[i] for i in rng.choice(len(tiles), size=min(args.check, len(tiles)), replace=False)]
            rays = sum(check_tile(desc, cam, W, H, node, int(ty), int(tx), int(cls[ty, tx]), light, gn) for ty, tx in tiles)
            print("  oracle: %d void tiles, %d rays checked, none hits node %d" % (len(tiles), rays, node))


if __name__ == "__main__":
    main()
