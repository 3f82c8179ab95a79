"""What csg_certain.h decides on lecture5.sdl, per frame size (CPU only: tests/libcsg_certain_check.so, `make all`):
    python scripts/csg_certain_census.py [WIDTHxHEIGHT ...]          (default: 3840x2160 1920x1080 640x480, five taps)
Per frame: the evaluations of the CsgDiff node by outcome — primary rays inside the node's bound: empty (the left child
certainly missed), void (a certain "no hit" behind a hit left child), L0 (the cube's first hit), R1 (the sphere's second
hit), other certain hits, unsure; the floor's shadow segments towards the light likewise —, the unsure share, and the 8x8
tiles that contain an unsure lane.  The rays are the camera's through the five taps of every pixel, as
tests/test_csg_certain_host.py builds them; shadow rays that start on the CsgOp's own surface are not part of it (the
kernels do not ask for them)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import chess2rt_amd as c2  # noqa: E402
from chess2rt_amd import _abi  # noqa: E402
import test_csg_certain_host as H  # noqa: E402

lib = C.CDLL(H.LIBPATH)
EMPTY = 0


def child_state(param, is_sphere, o, v):
    n = len(o)
    st, a0, a1, dl = np.zeros(n, np.int32), np.zeros(n), np.zeros(n), np.zeros(n)
    lib.csg_certain_child(int(is_sphere), (C.c_double * 4)(*param), np.ascontiguousarray(o).ctypes.data_as(H._DP),
                          np.ascontiguousarray(v).ctypes.data_as(H._DP), C.c_int64(n), C.c_double(1.0), st.ctypes.data_as(H._IP),
                          a0.ctypes.data_as(H._DP), a1.ctypes.data_as(H._DP), dl.ctypes.data_as(H._DP))
    return st


def outcomes(o, v):
    kind, side, k, _, _ = H.decide(lib, _abi.GEOM_CSG_DIFF, (False, H.CUBE), (True, H.SPHERE), o, v)
    left = child_state(H.CUBE, False, o, v)
    nohit, hit = kind == H.NOHIT, kind == H.HIT
    out = dict(empty=int((nohit & (left == EMPTY)).sum()), void=int((nohit & (left != EMPTY)).sum()),
               L0=int((hit & (side == 0) & (k == 0)).sum()), R1=int((hit & (side == 1) & (k == 1)).sum()))
    out["other"] = int(hit.sum()) - out["L0"] - out["R1"]
    out["unsure"] = int((kind == H.UNSURE).sum())
    return out, kind == H.UNSURE


for size in sys.argv[1:] or ["3840x2160", "1920x1080", "640x480"]:
    W, Hh = (int(x) for x in size.split("x"))
    s = c2.parseSceneFromFile(os.path.join(H.SCENES, "lecture5.sdl"))
    s.setFrameSize(W, Hh)
    cam = s.beginFrame()
    d = s.desc.contents
    pos, dirs = H.screen_dirs(cam, W, Hh, 5)
    c, rad = np.array(H.CUBE[:3]), H.CUBE[3] * 0.5 * np.sqrt(3.0) * 1.001
    Hv = pos - c
    b = dirs @ Hv
    inside = b * b - (Hv @ Hv - rad * rad) > 0
    pixel = np.tile(np.arange(W * Hh), 5)
    tiles_x = (W + 7) // 8
    tile_of = (pixel // W // 8) * tiles_x + (pixel % W) // 8
    prim, pu = outcomes(np.broadcast_to(pos, dirs.shape)[inside], dirs[inside])
    light = np.array([d.light_pos[i] for i in range(3)])
    down = dirs[:, 1] < -1e-9
    sf, sd = H.floor_shadow(pos, dirs, d.geom_param[0], light)
    shad, su = outcomes(sf, sd)
    total = sum(prim.values()) + sum(shad.values())
    unsure_tiles = len(set(tile_of[inside][pu].tolist()) | set(tile_of[down][su].tolist()))
    print("%s x5: %d samples" % (size, len(dirs)))
    print("  primary rays inside the bound: %d  %s" % (sum(prim.values()), "  ".join("%s %d" % kv for kv in prim.items())))
    print("  floor shadow segments:         %d  %s" % (sum(shad.values()), "  ".join("%s %d" % kv for kv in shad.items())))
    print("  unsure share %.3e of %d evaluations; tiles with an unsure lane: %d of %d" % (
        (prim["unsure"] + shad["unsure"]) / total, total, unsure_tiles, tiles_x * ((Hh + 7) // 8)))
