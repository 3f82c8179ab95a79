"""Shared by tests/test_temporal_motion_abi.py (CPU) and tests/test_gpu_temporal_motion.py (GPU): the synthetic anchor of
the motion accumulation — a tilted plane patch on a node that moves rigidly under a still camera — and the posed
three-frame sequence of lecture5_like both files run."""
import ctypes as C
import functools

import numpy as np

import scene_update_util as su
import temporal_cases as tc
import temporal_reference as tr
from chess2rt_amd import _abi

ANCHOR_NODE = 5
ANCHOR_OPTS = dict(max_age=8, min_normal_dot=0.9, max_plane_dist=0.1)
# two rigid poses of the node, far apart: the node turns by tens of degrees and travels hundreds of units
ANCHOR_PREV = (("rotate", 20, 10, 5), ("translate", 10, -5, 3))
ANCHOR_CUR = (("rotate", -15, 30, 40), ("translate", -200, 80, 150))


def camera_struct(pos, up_left, up_right, down_left):
    cam = _abi.CameraFrame()
    for name, v in (("pos", pos), ("up_left", up_left), ("up_right", up_right), ("down_left", down_left)):
        setattr(cam, name, (C.c_double * 3)(*[float(x) for x in v]))
    return cam


def parts(t):
    """(transform, inverseTransform, transposedInverse, offset) of 30 doubles"""
    t = np.asarray(t, dtype=np.float64).reshape(30)
    return t[0:9].reshape(3, 3), t[9:18].reshape(3, 3), t[18:27].reshape(3, 3), t[27:30]


def moved_point(p, frm, to, dtype=np.float64):
    """Transform.point of `to` after Transform.undoPoint of `frm`, literally (row vectors), in `dtype`"""
    _, If, _, of = (x.astype(dtype) for x in parts(frm))
    Tt, _, _, ot = (x.astype(dtype) for x in parts(to))
    return ((np.asarray(p).astype(dtype) - of) @ If) @ Tt + ot


def moved_normal(n, frm, to, dtype=np.float64):
    """the normal of a RIGID pose `frm` as `to` turns it: back through frm's rotation, forth through to's"""
    _, If, _, _ = (x.astype(dtype) for x in parts(frm))
    _, _, TIt, _ = (x.astype(dtype) for x in parts(to))
    return (np.asarray(n).astype(dtype) @ If) @ TIt


@functools.lru_cache(maxsize=None)
def anchor(w, h, channels=3):
    """(cam, frame 0 guides, history 0, c0, frame 1 guides, in 1, prev pose, cur pose, patch): the camera looks from the
    origin through (i, j, 1) at pixel (i, j) and stands still; frame 0 sees the plane z = 4 + a x + b y as node 5 on a patch
    (the whole frame where it is small), with history colour c0 and age 1; frame 1 sees the same patch, pixel for pixel,
    carried from the pose ANCHOR_PREV to the pose ANCHOR_CUR."""
    cam = camera_struct((0, 0, 0), (0, 0, 1), (w, 0, 1), (0, h, 1))
    prev, cur = su.xf(*ANCHOR_PREV), su.xf(*ANCHOR_CUR)
    ys, xs = np.mgrid[0:h, 0:w]
    a, b = 0.1 / w, 0.15 / h
    t = 4.0 / (1.0 - a * xs - b * ys)
    p0 = np.stack([t * xs, t * ys, t], axis=-1)
    n0 = np.array([a, b, -1.0]) / np.sqrt(a * a + b * b + 1.0)
    normal0 = np.broadcast_to(n0, (h, w, 3)).copy()
    node = np.full((h, w), -1, dtype=np.int32)
    patch = np.zeros((h, w), dtype=bool)
    if w >= 16 and h >= 16:
        patch[4:h - 4, 5:w - 5] = True
    else:
        patch[:] = True
    node[patch] = ANCHOR_NODE
    rng = np.random.RandomState(7 * w + h)
    c0 = rng.uniform(0.5, 1.5, (h, w, channels)).astype(np.float32)
    in1 = rng.uniform(0.5, 1.5, (h, w, channels)).astype(np.float32)
    first = tr.accumulate(node, normal0, p0, c0, ANCHOR_OPTS["max_age"], ANCHOR_OPTS["min_normal_dot"], ANCHOR_OPTS["max_plane_dist"])
    g0 = dict(node=node, normal=normal0, p=p0)
    g1 = dict(node=node, normal=moved_normal(normal0, prev, cur), p=moved_point(p0, prev, cur))
    for g in (g0, g1):
        for v in g.values():
            v.setflags(write=False)
    return cam, g0, first["history"], c0, g1, in1, prev, cur, patch


def anchor_motion(prev, cur, n_listed, where):
    """a motion list of `n_listed` entries with the anchor's node `where`: "first", "last" or "absent"; the other entries
    are nodes no pixel lies on, each with a pose pair of its own"""
    others = [100 + k for k in range(n_listed)]
    poses = {k: (su.xf(("rotate", k, 2 * k, 3), ("translate", k, 1, 2)), su.xf(("scale", 1 + 0.01 * k, 1, 1))) for k in others}
    order = others[:n_listed - 1] if where != "absent" else others
    if where == "first":
        order = [ANCHOR_NODE] + order
    elif where == "last":
        order = order + [ANCHOR_NODE]
    return {k: ((prev, cur) if k == ANCHOR_NODE else poses[k]) for k in order}


# ---- the posed sequence of lecture5_like ----
W, H = 96, 64
SEQ_OPTS = dict(max_age=8, min_normal_dot=0.9, max_plane_dist=0.1)
N_FRAMES = 3


def posed_sequence(tmp_path):
    """(scene, cameras, render options, poses, base transforms): lecture5_like at 96 x 64 under the camera step of
    tests/temporal_cases.py; frame 0 is the scene as it is, frame 1 translates node 3 and turns node 2 (the CsgDiff), frame
    2 turns node 2 further, scales node 1 and names node 3 no longer (it is back where it was).  Each pose is relative to
    the base, as the posed calls take them: {node: transform30}."""
    scene = su.load_text(tmp_path, su.lecture5_like(1), "l5_motion.sdl", size=(W, H))
    scene.setDof(False)
    cams = [scene.beginFrame()]
    for _ in range(N_FRAMES - 1):
        scene.moveCamera(*tc.MOVE)
        scene.rotateCamera(*tc.ROTATE)
        cams.append(scene.beginFrame())
    base = su.Desc(scene.desc)
    poses = [{},
             {3: su.xf(("translate", 80, 15, 236)), 2: su.xf(("rotate", 12, 0, 0), ("translate", 10, 0, -15))},
             {2: su.xf(("rotate", 30, 6, 0), ("translate", 25, 0, -30)), 1: su.xf(("scale", 1.2, 0.8, 1.1), ("translate", -15, 0, 10))}]
    return scene, cams, scene.renderOpts(taps=_abi.TAPS_1), poses, {n: base.transform(n) for n in (1, 2, 3)}


def frame_motion(poses, base, i):
    """frame i's motion list as the posed sequence calls build it: {node: (prev, cur)}, ascending, unchanged nodes dropped"""
    out = {}
    for n in sorted(set(poses[i - 1]) | set(poses[i])):
        prev, cur = poses[i - 1].get(n, base[n]), poses[i].get(n, base[n])
        if np.asarray(prev).tobytes() != np.asarray(cur).tobytes():
            out[n] = (prev, cur)
    return out


def full_pose(poses, base, i):
    """the base patched by poses[i] as ONE pose over every posable node of the sequence: what c2rt_update_scene takes to
    put the context into frame i's scene whatever it held before"""
    return {n: poses[i].get(n, base[n]) for n in base}
