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
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GEOM_PLANE, GEOM_SPHERE, GEOM_CUBE, GEOM_DIFF = 0, 1, 2, 5
TAPS = ((0.0, 0.0), (0.3, 0.3), (0.6, 0.0), (0.0, 0.6), (0.6, 0.6))  # rt/renderer.d:235-242
MAX_VOID_NODES = 4   # csg_void.h: kMaxVoidNodes
MAX_CULL_NODES = 32  # c2rt_device.h: kMaxCullNodes
MAX_CULL_LIGHTS = 4  # c2rt_device.h: kMaxCullLights
TILE = 8

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


class Cand(namedtuple("Cand", "node lo hi c R flags")):
    """A CsgDiff(L, Sphere) node the library tests (scene_plan.cpp, plan_void_nodes): its padded world box, the subtracted
    sphere's world centre and radius, and its VoidNode::flags (bit 0 primary, bit 1 shadow towards light 0)."""


_IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def _node_tr(desc, n):
    tr = [desc.node_transform[30 * n + i] for i in range(30)]
    return tr[0:9], tr[9:18], tr[18:27], tr[27:30]


def _finite(*xs):
    return all(math.isfinite(x) for x in xs)


def ground_of(desc):
    """(node, y) of the ground as the library picks it (scene_plan.cpp, plan_ground_rects; RenderParams::ground_node): the first Plane node
    below kMaxCullNodes under an identity matrix with zero offset and a finite height, or (None, None)."""
    desc = _fields(desc)
    for n in range(min(desc.n_nodes, MAX_CULL_NODES)):
        g = desc.node_geom[n]
        m, inv, tinv, off = _node_tr(desc, n)
        if desc.geom_type[g] == GEOM_PLANE and m == inv == tinv == _IDENTITY and off == [0, 0, 0] \
                and math.isfinite(desc.geom_param[4 * g]):
            return n, desc.geom_param[4 * g]
    return None, None


def _geom_finite(desc, g):
    """DevGeom kGeomFinite of a Sphere / Cube: its parameters and derived values are finite"""
    p = [desc.geom_param[4 * g + i] for i in range(4)]
    if desc.geom_type[g] == GEOM_CUBE:
        h = p[3] * 0.5
        q = [p[i] + -1 * h for i in range(3)] + [p[i] + 1 * h for i in range(3)]
    else:
        q = [p[3] * p[3]]
    return _finite(*p) and _finite(*q)


def void_candidates(desc):
    """[Cand] for the nodes the library tests, restated from scene_plan.cpp (plan_world_boxes, plan_void_nodes) operation for operation: the
    first kMaxVoidNodes nodes below kMaxCullNodes that are CsgDiff(Cube | Sphere, Sphere) under an identity matrix
    (offset allowed) with finite children and R > 0.  The box is the left child's (box_of: shortcut A) padded as for
    every node (1e-6 ext + 1e-6 mag + 1e-9 + 4e-6 max(|M^-1|_F, 1)) and moved by the offset; the shadow flag needs
    the ground and the box strictly on the ground's side of light 0's height."""
    desc = _fields(desc)
    gn, gy = ground_of(desc)
    light = [desc.light_pos[i] for i in range(3)] if desc.n_lights else None
    out = []
    for n in range(min(desc.n_nodes, MAX_CULL_NODES)):
        if len(out) >= MAX_VOID_NODES:
            break
        g = desc.node_geom[n]
        m, inv, tinv, off = _node_tr(desc, n)
        if desc.geom_type[g] != GEOM_DIFF or not (m == inv == tinv == _IDENTITY):
            continue
        l, r = desc.geom_child[2 * g], desc.geom_child[2 * g + 1]
        if l == r or desc.geom_type[r] != GEOM_SPHERE or desc.geom_type[l] not in (GEOM_SPHERE, GEOM_CUBE):
            continue
        if not (_geom_finite(desc, l) and _geom_finite(desc, r)):
            continue
        pl = [desc.geom_param[4 * l + i] for i in range(4)]
        pr = [desc.geom_param[4 * r + i] for i in range(4)]
        if not pr[3] > 0:
            continue
        # node_boxed: the Diff's bound (bound_of, the left child's) is finite and small enough, the offset finite
        br = abs(pl[3]) if desc.geom_type[l] == GEOM_SPHERE else abs(pl[3]) * 0.5 * 1.7320508075688774
        bmag = abs(pl[0]) + abs(pl[1]) + abs(pl[2]) + br
        rp = br * (1 + 1e-6) + 1e-6 * bmag + 1e-9
        if not (math.isfinite(rp) and rp * rp < 1e300) or not _finite(*off):
            continue
        e = abs(pl[3]) if desc.geom_type[l] == GEOM_SPHERE else abs(pl[3]) * 0.5
        lo = [pl[i] - e for i in range(3)]
        hi = [pl[i] + e for i in range(3)]
        inv_norm = 0.0
        for x in inv:
            inv_norm += x * x
        inv_norm = math.sqrt(inv_norm)
        mag = ext = 0.0
        for i in range(3):
            mag += max(abs(lo[i]), abs(hi[i]))
            ext = max(ext, hi[i] - lo[i])
        pad = 1e-6 * ext + 1e-6 * mag + 1e-9 + 4e-6 * (inv_norm if inv_norm > 1 else 1.0)
        if not math.isfinite(pad):
            continue
        corners = []
        for k in range(8):
            q = [hi[0] + pad if k & 1 else lo[0] - pad, hi[1] + pad if k & 2 else lo[1] - pad, hi[2] + pad if k & 4 else lo[2] - pad]
            corners.append([q[0] * m[0 + j] + q[1] * m[3 + j] + q[2] * m[6 + j] + off[j] for j in range(3)])
        if not _finite(*[w for cw in corners for w in cw]):
            continue
        wlo = [min(cw[j] for cw in corners) for j in range(3)]
        whi = [max(cw[j] for cw in corners) for j in range(3)]
        c = [pr[j] + off[j] for j in range(3)]
        if not _finite(*c, *wlo, *whi):
            continue
        flags = 1
        if gn is not None and light is not None:
            h = light[1] - gy
            tol = 1e-6 + 1e-9 * (abs(light[1]) + abs(wlo[1]) + abs(whi[1]))
            if _finite(*light, h) and ((h > 0 and whi[1] < light[1] - tol) or (h < 0 and wlo[1] > light[1] + tol)):
                flags |= 2
        out.append(Cand(n, wlo, whi, c, pr[3], flags))
    return out


def frame_void_nodes(desc, cam, debug_cull=0):
    """The VoidCull the library hands the mask pre-pass for this camera (scene_plan.cpp, void_cull_of): per candidate
    (node, lo, hi, c, r2 = (R - void_margin(scale))^2, flags), without bit 1 where the frame runs no shadow culling
    or no ground refinement (the diagnostics build's C2RT_DEBUG_CULL bits 2 and 4).  None: the frame culls nothing
    (C2RT_DEBUG_CULL bit 1)."""
    desc = _fields(desc)
    if debug_cull & 1:
        return None
    gn, _ = ground_of(desc)
    n_cull_lights = 0 if debug_cull & 4 else min(desc.n_lights, MAX_CULL_LIGHTS)
    if debug_cull & 2:
        gn = None
    out = []
    for cand in void_candidates(desc):
        scale = cand.R
        scale += max(abs(cand.c[0]), abs(cand.c[1]), abs(cand.c[2]))
        scale += max(abs(cam.pos[0]), abs(cam.pos[1]), abs(cam.pos[2]))
        if desc.n_lights:
            scale += max(abs(desc.light_pos[0]), abs(desc.light_pos[1]), abs(desc.light_pos[2]))
        rm = cand.R - lib().c2rt_void_margin(scale)
        if not (rm > 0) or not math.isfinite(scale):
            continue
        flags = cand.flags
        if n_cull_lights == 0 or gn is None:
            flags &= ~2
        out.append(dict(node=cand.node, lo=cand.lo, hi=cand.hi, c=cand.c, r2=rm * rm, flags=flags))
    return out


def _scale_and_light(desc, cam, cand):
    light = [desc.light_pos[i] for i in range(3)] if desc.n_lights else [0.0, 0.0, 0.0]
    scale = cand.R + max(abs(x) for x in cand.c) + max(abs(x) for x in cam.pos) + (max(abs(x) for x in light) if desc.n_lights else 0)
    return scale, light


def _classify_args(desc, cam, cand, r_override):
    desc = _fields(desc)
    scale, light = _scale_and_light(desc, cam, cand)
    rm = (cand.R if r_override is None else r_override) - lib().c2rt_void_margin(scale)
    _, gy = ground_of(desc)
    du = [cam.up_right[i] - cam.up_left[i] for i in range(3)]
    dv = [cam.down_left[i] - cam.up_left[i] for i in range(3)]
    head = (_a3(cam.pos), _a3(cam.up_left), _a3(du), _a3(dv), cam.frame_width, cam.frame_height)
    tail = (_a3(cand.lo), _a3(cand.hi), _a3(cand.c), rm * rm, cand.flags, _a3(light), gy if gy is not None else 0.0)
    return rm, head, tail


def classify(desc, cam, W, H, cand, r_override=None):
    """uint8 (tiles_y, tiles_x) over the full-frame tile grid: bit 0 primary-void, bit 1 shadow-void (towards light 0
    from the ground footprint; only for candidates with flag bit 1).  r_override: classify with this radius instead
    of the sphere's (the mutation test)."""
    tw, th = (W + 7) // 8, (H + 7) // 8
    out = np.zeros((th, tw), dtype=np.uint8)
    rm, head, tail = _classify_args(desc, cam, cand, r_override)
    if not rm > 0:
        return out
    lib().c2rt_void_classify(*head, W, H, *tail, out.ctypes.data_as(C.c_void_p))
    return out


def tile_bounds(trow, tcol, mask_row0, mask_rows, strip_height=1, strip_rank=0, strip_world=1):
    """(tx0, ty0, ty1): the first pixel column and the first and last FRAME row of the tile in row `trow` (row 0 =
    local row mask_row0) and column `tcol` of a mask table, restated from tile_mask_entry (c2rt_tile_mask.inc): the
    last tile row may be ragged; under strips (local rows dealt round-robin in strips of strip_height) the local rows
    map to frame rows and a tile may span two strips, whose frame rows [ty0, ty1] then also hold other ranks' rows."""
    lr_first = trow * TILE + mask_row0
    lr_last = min(trow * TILE + TILE - 1, mask_rows - 1) + mask_row0
    ty0, ty1 = lr_first, lr_last
    if strip_world > 1:
        sh = strip_height
        ty0 = ((lr_first // sh) * strip_world + strip_rank) * sh + lr_first % sh
        ty1 = ((lr_last // sh) * strip_world + strip_rank) * sh + lr_last % sh
    return tcol * TILE, ty0, ty1


def _classify_tiles_fn():
    """c2rt_void_classify_tiles, bound on first use: lib() itself needs only the entry points every caller uses"""
    fn = lib().c2rt_void_classify_tiles
    if fn.restype is not None:
        d3 = C.POINTER(C.c_double)
        fn.argtypes = [d3, d3, d3, d3, C.c_double, C.c_double, C.c_size_t, C.c_void_p, d3, d3, d3, C.c_double, C.c_uint,
                       d3, C.c_double, C.c_void_p]
        fn.restype = None
    return fn


def classify_tiles(desc, cam, bounds, cand, r_override=None):
    """uint8 [len(bounds)]: classify explicit tiles, bounds = [(tx0, ty0, ty1)] (tile_bounds)."""
    out = np.zeros(len(bounds), dtype=np.uint8)
    rm, head, tail = _classify_args(desc, cam, cand, r_override)
    if not rm > 0 or not len(bounds):
        return out
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.int32).reshape(-1, 3))
    _classify_tiles_fn()(*head, len(bounds), b.ctypes.data_as(C.c_void_p), *tail, out.ctypes.data_as(C.c_void_p))
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
    """Oracle, every ray of one void tile of the full-frame grid (check_tile_bounds)."""
    return check_tile_bounds(desc, cam, W, H, node, (tx * 8, ty * 8, min(ty * 8 + 7, H - 1)), bits, light, ground)


def check_tile_bounds(desc, cam, W, H, node, bounds, bits, light, ground):
    """Oracle, every ray of one void tile, bounds = (tx0, ty0, ty1) as tile_bounds has them (every frame row of
    [ty0, ty1]): primary rays (5 taps) miss the node; with bit 1, for primary rays that hit the ground, the shadow
    ray towards light 0 (from p + N*1e-6, rt/shader.d:88) gets no hit on the node before the light.  Returns the
    number of rays checked; raises on a violation."""
    import oracle_lib
    from oracle_lib import OrcHit

    L = oracle_lib.lib()
    o, d = (C.c_double * 3)(), (C.c_double * 3)()
    n_rays = 0
    tx0, ty0, ty1 = bounds
    for y in range(ty0, min(ty1 + 1, H)):
        for x in range(tx0, min(tx0 + 8, W)):
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
