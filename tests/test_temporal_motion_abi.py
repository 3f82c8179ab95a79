"""CPU half of the motion-accumulation tests (c2rt_temporal_accumulate_motion): the ABI's struct, the one refusal that needs
no device, properties of the numpy restatement (tests/temporal_motion_reference.py), independent anchors for the composed
matrices and for the accumulation itself, and the precondition of the GPU comparison — that the posed sequence it runs
puts pixels into every class, counted from the oracle alone.

The refusals that need a context (reserved, the limit, null arrays, an index listed twice) are in
tests/test_gpu_temporal_motion.py: a context exists only on a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scene_update_util as su
import temporal_motion_cases as mc
import temporal_motion_reference as tm
import temporal_reference as tr
from chess2rt_amd import _abi, makeMotion
from ray_query_util import oracle_trace, screen_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_struct_layout_matches_c(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "c2rt.h"
int main(void) {
  printf("TemporalMotion %zu\\n", sizeof(c2rt_temporal_motion));
  printf("reserved %zu\\n", offsetof(c2rt_temporal_motion, reserved));
  printf("node_index %zu\\n", offsetof(c2rt_temporal_motion, node_index));
  printf("prev_transform %zu\\n", offsetof(c2rt_temporal_motion, prev_transform));
  printf("cur_transform %zu\\n", offsetof(c2rt_temporal_motion, cur_transform));
  printf("max_nodes %d\\n", C2RT_MAX_MOTION_NODES);
  printf("abi %u\\n", C2RT_ABI_VERSION);
  return 0;
}
""")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())}
    M = _abi.TemporalMotion
    assert got == {"TemporalMotion": C.sizeof(M), "reserved": M.reserved.offset, "node_index": M.node_index.offset,
                   "prev_transform": M.prev_transform.offset, "cur_transform": M.cur_transform.offset, "max_nodes": _abi.MAX_MOTION_NODES,
                   "abi": _abi.ABI_VERSION}
    assert C.sizeof(M) == 32 and _abi.MAX_MOTION_NODES == tm.MAX_MOTION_NODES == 16 and _abi.ABI_VERSION == 1


def test_symbols_and_the_null_context():
    """the four new symbols are exported; a null context is refused before anything else is read, whatever the motion"""
    L = _abi.load_library()
    for name in ("c2rt_temporal_accumulate_motion", "c2rt_temporal_accumulate_motion_device", "c2rt_render_paths_sequence_posed",
                 "c2rt_render_paths_sequence_posed_variance"):
        assert hasattr(L, name), name
    m = makeMotion({3: (su.xf(), su.xf(("translate", 1, 2, 3)))})
    assert m.n_nodes == 1 and m.reserved == 0
    assert L.c2rt_temporal_accumulate_motion(None, None, None, None, C.byref(m), None, None, None, None) == _abi.ERR_INVALID_ARG
    assert L.c2rt_temporal_accumulate_motion_device(None, None, None, None, C.byref(m), None, None, None, None, None) == _abi.ERR_INVALID_ARG


# ---- properties of the restatement ----


def small_case(seed=3, w=24, h=18):
    """a second frame over a first: nodes 0..2 in patches, misses among them, a camera one small step on"""
    prev = mc.camera_struct((0, 0, 0), (-1.0, -0.8, 1.0), (1.0, -0.8, 1.0), (-1.0, 0.8, 1.0))
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    node = (((xs // 5) + 2 * (ys // 4)) % 3).astype(np.int32)
    node[rng.uniform(size=(h, w)) < 0.08] = -1
    normal = rng.uniform(-0.1, 0.1, (h, w, 3))
    normal[..., 2] = -1.0
    sx, sy = (xs + 0.3)[..., None], (ys - 0.2)[..., None]
    p = 5.0 * (np.array([-1.0, -0.8, 1.0]) + np.array([2.0, 0, 0]) * (sx / w) + np.array([0, 1.6, 0]) * (sy / h))
    p0 = 5.0 * (np.array([-1.0, -0.8, 1.0]) + np.array([2.0, 0, 0]) * (xs[..., None] / w) + np.array([0, 1.6, 0]) * (ys[..., None] / h))
    a, b = (rng.uniform(0, 2, (h, w, 3)).astype(np.float32) for _ in range(2))
    first = tr.accumulate(node, normal, p0, a, 8, 0.8, 0.3)
    return prev, node, normal, p, b, first["history"]


def same_result(x, y, h, w, ch=3):
    return (tr.count_differing(x["colour"], y["colour"]) == 0 and tr.count_differing(x["variance"], y["variance"]) == 0
            and np.array_equal(x["age"], y["age"]) and tr.history_differing(x["history"], y["history"], h, w, ch) == 0)


def test_empty_and_null_motion_are_the_static_call_to_the_bit():
    prev, node, normal, p, img, hist = small_case()
    h, w = node.shape
    want = tr.accumulate(node, normal, p, img, 8, 0.8, 0.3, prev_cam=prev, history=hist)
    assert (want["age"] == 2).sum() > 100
    for motion in (None, {}, {7: (su.xf(), su.xf(("translate", 1, 2, 3)))}):          # node 7: no pixel lies on it
        got = tm.accumulate(node, normal, p, img, 8, 0.8, 0.3, prev_cam=prev, history=hist, motion=motion)
        assert same_result(got, want, h, w), motion
    first = tm.accumulate(node, normal, p, img, 8, 0.8, 0.3, motion={1: (su.xf(), su.xf(("translate", 1, 2, 3)))})      # no history: ignored
    assert same_result(first, tr.accumulate(node, normal, p, img, 8, 0.8, 0.3), h, w)


def test_unlisted_pixels_do_not_see_what_is_listed():
    prev, node, normal, p, img, hist = small_case(seed=4)
    h, w = node.shape
    want = tr.accumulate(node, normal, p, img, 8, 0.8, 0.3, prev_cam=prev, history=hist)
    a = tm.accumulate(node, normal, p, img, 8, 0.8, 0.3, prev_cam=prev, history=hist, motion={1: (su.xf(), su.xf(("translate", 0.4, 0, 0)))}, counts=(ca := {}))
    b = tm.accumulate(node, normal, p, img, 8, 0.8, 0.3, prev_cam=prev, history=hist,
                      motion={1: (su.xf(("rotate", 40, 0, 0)), su.xf(("scale", 2, 1, 1))), 9: (su.xf(), su.xf())})
    off = node != 1
    for got in (a, b):
        for k in ("colour", "variance", "age"):
            assert tr.count_differing(got[k][off].astype(np.float32), want[k][off].astype(np.float32)) == 0, k
        hs, ws = tr.split_history(got["history"], h, w, 3), tr.split_history(want["history"], h, w, 3)
        assert tr.count_differing(hs["m"][off], ws["m"][off]) == 0 and tr.count_differing(hs["c"][off], ws["c"][off]) == 0
        # the history out holds the CURRENT guides of every pixel, moved or not
        assert tr.count_differing(hs["nf"], ws["nf"]) == 0 and tr.count_differing(hs["pf"], ws["pf"]) == 0 and np.array_equal(hs["node"], ws["node"])
    on = node == 1
    assert tr.count_differing(a["colour"][on], want["colour"][on]) > 0                      # and the listed ones do move
    assert ca["moved_kept"] + ca["moved_rejected"] + ca["moved_lost"] == on.sum() and ca["moved_kept"] > 20
    assert ca["unlisted_history"] + ca["unlisted_restart"] == (off & (node >= 0)).sum()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("slot", [0, 4, 13, 22, 28])                                          # a part of each of the four, prev or cur
@pytest.mark.parametrize("which", ["prev", "cur"])
def test_a_non_finite_transform_restarts_its_node_and_nothing_else(bad, slot, which):
    prev, node, normal, p, img, hist = small_case(seed=5)
    want = tr.accumulate(node, normal, p, img, 8, 0.8, 0.3, prev_cam=prev, history=hist)
    pose = (su.xf_with(slot, bad), su.xf()) if which == "prev" else (su.xf(), su.xf_with(slot, bad))
    # (prev.inverseTransform and cur.transposedInverse are not read by the contract: a bad value there changes nothing)
    unread = (which == "prev" and 9 <= slot < 18) or (which == "cur" and 18 <= slot < 27)
    got = tm.accumulate(node, normal, p, img, 8, 0.8, 0.3, prev_cam=prev, history=hist, motion={2: pose})
    on = node == 2
    assert on.sum() > 50 and (want["age"][on] == 2).sum() > 50
    if not unread:
        assert (got["age"][on] == 1).all()
        assert got["colour"][on].tobytes() == img[on].tobytes() and not got["variance"][on].any()
    else:
        assert np.array_equal(got["age"][on], want["age"][on])
    assert np.array_equal(got["age"][~on], want["age"][~on]) and tr.count_differing(got["colour"][~on], want["colour"][~on]) == 0
    assert np.isfinite(got["colour"]).all()


# ---- an independent anchor for the composed matrices ----

POSE_PAIRS = {
    "translation": ((("translate", 100, 15, 256),), (("translate", 80, 25, 236),)),
    "rotation": ((("rotate", 10, 20, 30),), (("rotate", -40, 5, 60),)),
    "scale": ((("scale", 1.5, 0.75, 1.25),), (("scale", 0.8, 2.0, 1.1),)),
    "combined": ((("scale", 1.2, 0.8, 1.1), ("rotate", 15, -25, 35), ("translate", -30, 10, 40)),
                 (("scale", 0.9, 1.3, 0.7), ("rotate", -50, 10, 5), ("translate", 120, -60, 300))),
}


@pytest.mark.parametrize("name", list(POSE_PAIRS))
def test_composed_record_against_the_literal_transforms(name):
    """p' of the restatement against Transform.point of the previous pose after Transform.undoPoint of the current one,
    written out in np.longdouble.  Bound 1e-9 x the largest magnitude among p and the offsets: a gross-error guard, fp64
    rounding of the ~30 operations is some three orders below it.  For the rigid pairs n' against the turned normal too,
    and its squared length within 1e-6 of 1."""
    prev, cur = (su.xf(*steps) for steps in POSE_PAIRS[name])
    rng = np.random.RandomState(11)
    p = rng.uniform(-300, 300, (200, 3))
    n = rng.normal(size=(200, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    pp, nn = tm.carry(p, n, tm.compose(prev, cur))
    lit = mc.moved_point(p, cur, prev, np.longdouble)
    scale = max(np.abs(p).max(), np.abs(prev[27:]).max(), np.abs(cur[27:]).max())
    err = float(np.abs(pp.astype(np.longdouble) - lit).max())
    print(name, "largest |p' - literal| = %.3g, bound %.3g" % (err, 1e-9 * scale))
    assert err <= 1e-9 * scale
    assert float(np.abs(lit - p).max()) > 1.0                                                  # the pair does move the points
    if name in ("translation", "rotation"):
        want = mc.moved_normal(n, cur, prev, np.longdouble)
        assert float(np.abs(nn.astype(np.longdouble) - want).max()) <= 1e-9
        nf = nn.astype(np.float32)
        l2 = (nf[:, 0] * nf[:, 0] + nf[:, 1] * nf[:, 1]) + nf[:, 2] * nf[:, 2]
        assert np.abs(l2.astype(np.float64) - 1.0).max() <= 1e-6
    else:
        # a normal stays a normal: perpendicular to every tangent carried the same way
        t = np.cross(n, rng.normal(size=(200, 3)))
        tt = mc.moved_point(p + t, cur, prev, np.longdouble) - lit
        dots = np.abs((tt * nn.astype(np.longdouble)).sum(axis=1))
        assert float(dots.max()) <= 1e-9 * float(np.abs(tt).max()) * float(np.abs(nn).max())


# ---- a reference-free anchor of the accumulation ----


def test_a_rigidly_moved_patch_finds_its_history_and_the_static_call_does_not():
    """61 x 47, the camera still: frame 1's patch is frame 0's carried from one rigid pose to another.  Through the motion
    call every pixel of the patch finds itself: age 2 and colour = c0 + (in - c0) / 2 to 1e-5 relative (the weight that
    leaks to a neighbour is of the order of the reprojection's 1e-13).  Through the static call the same guides restart on
    every pixel of the node: the behaviour there was before."""
    cam, g0, hist0, c0, g1, in1, prev, cur, patch = mc.anchor(61, 47)
    o = mc.ANCHOR_OPTS
    assert patch.sum() == (47 - 8) * (61 - 10)
    assert np.abs(g1["p"] - g0["p"])[patch].max(axis=-1).min() > 100 * o["max_plane_dist"]     # displaced far beyond the plane test
    static = tr.accumulate(g1["node"], g1["normal"], g1["p"], in1, o["max_age"], o["min_normal_dot"], o["max_plane_dist"], prev_cam=cam, history=hist0)
    assert (static["age"][patch] == 1).all() and static["colour"][patch].tobytes() == in1[patch].tobytes()
    counts = {}
    got = tm.accumulate(g1["node"], g1["normal"], g1["p"], in1, o["max_age"], o["min_normal_dot"], o["max_plane_dist"], prev_cam=cam, history=hist0,
                        motion={mc.ANCHOR_NODE: (prev, cur)}, counts=counts)
    assert (got["age"][patch] == 2).all() and (got["age"][~patch] == 0).all()
    assert counts["moved_kept"] == patch.sum() and counts["moved_rejected"] == 0 and counts["moved_lost"] == 0
    want = c0.astype(np.float64) + (in1.astype(np.float64) - c0.astype(np.float64)) / 2
    rel = np.abs(got["colour"].astype(np.float64) - want)[patch] / np.abs(want)[patch]
    print("moved patch: largest relative error %.3g" % rel.max())
    assert rel.max() <= 1e-5
    hs = tr.split_history(got["history"], 47, 61, 3)
    assert np.array_equal(hs["pf"], g1["p"].astype(np.float32)) and np.array_equal(hs["nf"], g1["normal"].astype(np.float32))


# ---- the precondition of the GPU scene cases, from the oracle alone ----


def test_posed_sequence_fills_every_class(tmp_path):
    """lecture5_like at 96 x 64, three frames under the camera step of tests/temporal_cases.py, node 3 translated, node 2
    (the CsgDiff) turned, node 1 scaled unevenly (tests/temporal_motion_cases.py): the oracle's own planes put at least 50
    pixels into each of: on a moved node with its history kept; on a moved node, reprojected into the frame, every tap
    dropped; on no listed node with its history.  As measured, frames 1 and 2 together: see the assertion."""
    scene, cams, _, poses, base = mc.posed_sequence(tmp_path)
    desc = su.Desc(scene.desc)
    zero = np.zeros((mc.H, mc.W, 3), dtype=np.float32)
    hist, counts, per_frame = None, {}, []
    for i, cam in enumerate(cams):
        rec = oracle_trace(desc.patched(nodes=mc.full_pose(poses, base, i)).d, screen_rays(cam, mc.W, mc.H))
        g = (rec["closest_node"].reshape(mc.H, mc.W), rec["normal"].reshape(mc.H, mc.W, 3), rec["p"].reshape(mc.H, mc.W, 3))
        c = {}
        out = tm.accumulate(*g, zero, SEQ["max_age"], SEQ["min_normal_dot"], SEQ["max_plane_dist"], prev_cam=cams[i - 1] if i else None, history=hist,
                            motion=mc.frame_motion(poses, base, i) if i else None, counts=c)
        hist = out["history"]
        per_frame.append(c)
        for k, v in c.items():
            counts[k] = counts.get(k, 0) + v
    print({k: counts[k] for k in tm.MOTION_CLASSES}, [{k: c.get(k, 0) for k in tm.MOTION_CLASSES} for c in per_frame])
    assert sorted(mc.frame_motion(poses, base, 1)) == [2, 3] and sorted(mc.frame_motion(poses, base, 2)) == [1, 2, 3]
    for k in ("moved_kept", "moved_rejected", "unlisted_history"):
        assert counts[k] >= 50, (k, counts)
        assert per_frame[2][k] >= 50, (k, per_frame[2])                                       # the frame whose list holds all three kinds


SEQ = mc.SEQ_OPTS
