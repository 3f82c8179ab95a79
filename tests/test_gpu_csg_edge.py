"""GPU: the CsgOp code where ties, odd hit counts and leaf identity decide (c2rt_trace.inc: the wave-wide regular case
decided by comparisons, first-hit winners rebuilt without a replay, face codes in the hit tags, the kCsgShortA/B early
returns, lists told apart by the leaf id in the tag, the literal shell sort and walk for irregular waves), against
tests/geom_reference.py on tests/csg_edge_scenes.py: children that share face planes bit for bit, shared leaves,
Op(a, a), Plane operands, depth 4 and a tree that reaches the cap of 8 hits per child.
tests/test_csg_edge_reference.py holds the reference against the oracle on the CPU and states what the ray sets contain (its coverage conditions, among them the 64-aligned groups of 64 regular rays
and of 63 regular rays and one tied or odd one: the two sides of the device's `__all`).

Tolerances as in tests/test_gpu_geom.py: node and leaf equal, dist and p bit for bit, normal within 1e-15, u, v within
1e-12; visibility byte for byte; frames under shade_reference.compare / camera_reference.compare."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import camera_reference as cr
import camera_scenes as cs
import csg_edge_scenes as es
import geom_reference as gr
import oracle_lib as orc
import shade_reference as sr
from chess2rt_amd import _abi
from parity_util import TOL, maxdiff
from ray_query_util import assert_records_match_oracle

pytestmark = pytest.mark.gpu

MIN_REACH = 30
AMBIGUOUS_CAP = 0.001


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def reference(scene, name):
    """the reference's records, shadow segments, visibility, occluders and (screen set) colours — once, read-only"""
    r = Ref()
    case = es.load(scene)
    T, r.Ts = gr.Tables(case.desc), sr.Tables(case.desc)
    r.rays = es.ray_set(scene, name)
    t0 = time.time()
    r.recs, _ = gr.trace(T, r.rays)
    r.segs = sr.shadow_segments(r.Ts, r.rays[:, 3:], r.recs)
    vis, occ, _ = gr.test_visibility(T, r.segs)
    r.vis, r.occluder = vis.reshape(len(r.rays), -1), occ.reshape(len(r.rays), -1)
    r.shaded = sr.shade(r.Ts, r.rays[:, 3:], r.recs, r.vis) if name == "screen" else None
    print("reference of %s %s: %.2f s on the CPU" % (scene, name, time.time() - t0))
    return r


@functools.lru_cache(maxsize=None)
def five_tap_reference(scene):
    case = es.load(scene)
    return cr.render_frame((gr.Tables(case.desc), sr.Tables(case.desc)), cs.from_abi(case.cam), cr.Opts(es.W, es.H, taps=cr.TAPS_REF5))


_gpu_cases = {}


def gpu_case(gpu_ctx, scene):
    """uploads the scene; the queries run once per scene and are shared by the tests below (read-only)"""
    case = es.load(scene)
    gpu_ctx.uploadScene(case.desc)
    if scene not in _gpu_cases:
        out = {}
        for name in es.RAY_SETS:
            r = reference(scene, name)
            rec, rgb = gpu_ctx.traceRays(r.rays)
            out[name] = (rec, rgb, gpu_ctx.testVisibility(r.segs))
        _gpu_cases[scene] = out
    return _gpu_cases[scene]


def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("scene", es.SCENE_NAMES)
def test_queries_equal_the_reference(gpu_ctx, scene):
    for name, (rec, rgb, vis) in gpu_case(gpu_ctx, scene).items():
        r = reference(scene, name)
        wrong = np.nonzero((rec["closest_node"] != r.recs["closest_node"]) | (rec["leaf_geom"] != r.recs["leaf_geom"]) | (rec["dist"] != r.recs["dist"]))[0]
        print("%s %s: %d rays; node, leaf or dist differ on %d (first: %s); visibility differs on %d of %d"
              % (scene, name, len(r.rays), len(wrong), wrong[:8].tolist(), int((vis != r.vis.ravel()).sum()), vis.size))
        assert_records_match_oracle(rec, r.recs, "%s %s" % (scene, name))
        assert vis.dtype == np.uint8 and np.array_equal(vis, r.vis.ravel()), (scene, name)


@pytest.mark.parametrize("scene", es.SCENE_NAMES)
def test_hit_planes_equal_the_query_of_the_screen_rays(gpu_ctx, scene):
    case = es.load(scene)
    rec, rgb, _ = gpu_case(gpu_ctx, scene)["screen"]
    planes = gpu_ctx.renderHits(case.cam, case.opts)
    n = es.W * es.H
    assert np.array_equal(planes["node"].ravel(), rec["closest_node"]) and np.array_equal(planes["leaf"].ravel(), rec["leaf_geom"])
    for plane, want in (("dist", rec["dist"]), ("p", rec["p"]), ("normal", rec["normal"]), ("uv", np.stack([rec["u"], rec["v"]], axis=1))):
        assert np.array_equal(np.ascontiguousarray(planes[plane]).reshape(n, -1).view(np.uint64),
                              np.ascontiguousarray(want).reshape(n, -1).view(np.uint64)), (scene, plane)
    assert np.array_equal(_bits32(planes["rgb"]).reshape(n, 3), _bits32(rgb)), scene


@pytest.mark.parametrize("scene", es.SCENE_NAMES)
def test_frame_equals_the_frame_computed_without_the_oracle(gpu_ctx, scene):
    """renderFrame, one tap, against shade_reference.shade of the REFERENCE's records and visibility; on "identity" no
    tile is handed to the exact instance.  Five taps against camera_reference.render_frame under its interval rule, and
    against the oracle under the suite's TOL."""
    case = es.load(scene)
    gpu_case(gpu_ctx, scene)
    r = reference(scene, "screen")
    assert r.shaded.ambiguous.mean() <= AMBIGUOUS_CAP
    before = gpu_ctx.exactRedos()
    frame = gpu_ctx.renderFrame(case.cam, case.opts)
    redone = gpu_ctx.exactRedos() - before
    plain, outside = sr.compare(frame, r.shaded)
    print("%s frame: %d tiles redone exactly, %d ambiguous samples, %d floats differ outside them, %d outside their bounds"
          % (scene, redone, int(r.shaded.ambiguous.sum()), plain, outside))
    assert plain == 0 and outside == 0, (scene, plain, outside)
    if scene == "identity":
        assert redone == 0, "the lean instance handed tiles to the exact one"
    opts5 = case.scene.renderOpts(taps=_abi.TAPS_REF5)
    frame5 = gpu_ctx.renderFrame(case.cam, opts5)
    five = five_tap_reference(scene)
    held = float((five.ambiguous | five.wide).mean())
    plain5, outside5 = cr.compare(frame5, five)
    print("%s five taps against the reference: %d pixels held to an interval, %d floats differ, %d outside their bounds"
          % (scene, int((five.ambiguous | five.wide).sum()), plain5, outside5))
    assert held <= 5 * AMBIGUOUS_CAP
    assert plain5 == 0 and outside5 == 0, (scene, plain5, outside5)
    md, nbad, nne = maxdiff(frame5, orc.render_frame(case.desc, case.cam, opts5, 0))
    print("%s five taps against the oracle: max|d|=%.3g, differing floats: %d" % (scene, md, nne))
    assert md <= TOL and nbad == 0


@pytest.mark.parametrize("tree", es.CARVED)
def test_carved_parts_and_their_shadows(gpu_ctx, tree):
    """pixels the reference finds seen THROUGH the subtracted cube of Diff(a, e) / Diff(a, b), and ground pixels it finds
    cut off from a light by that node: what a wrong cull or shadow-rectangle decision at a shared face would lose (no
    tree of these scenes is a CsgDiff(., Sphere), so the void-tile test itself registers none of them)"""
    case = es.load("identity")
    rec, _, vis = gpu_case(gpu_ctx, "identity")["screen"]
    r = reference("identity", "screen")
    node = es.node_index("identity", tree)
    through = es.seen_through(r.rays, r.recs, *es.carved_box("identity", tree))
    shaded = (r.recs["closest_node"] == es.GROUND) & (r.occluder == node).any(axis=1)
    print("%s: %d pixels seen through the carved part, %d ground pixels shaded by the node" % (tree, int(through.sum()), int(shaded.sum())))
    assert through.sum() >= MIN_REACH and shaded.sum() >= MIN_REACH
    assert np.array_equal(vis.reshape(r.vis.shape)[shaded], r.vis[shaded])
    assert np.array_equal(rec["closest_node"][through], r.recs["closest_node"][through])
    frame = gpu_ctx.renderFrame(case.cam, case.opts).reshape(-1, 3)
    for pick in (through, shaded):
        sub = sr.Shaded()
        for f in ("rgb", "lo", "hi", "ambiguous"):
            setattr(sub, f, getattr(r.shaded, f)[pick])
        assert sr.compare(frame[pick], sub) == (0, 0)


def test_counted_frame_of_the_placed_scene_reports_the_oracles_truncations(gpu_ctx):
    """a counted frame of "placed": the ray of one pixel is the cap tree's axis, so csgTruncations() is non-zero, and it
    equals the oracle's count for that frame; frame and ray counts equal the oracle's"""
    case = es.load("placed")
    gpu_ctx.uploadScene(case.desc)
    opts = case.scene.renderOpts(taps=_abi.TAPS_1, count_rays=1)
    a = gpu_ctx.renderFrame(case.cam, opts)
    got, rays = gpu_ctx.csgTruncations(), gpu_ctx.rayStats()
    L = orc.lib()
    L.orc_take_csg_truncations()
    st = {}
    ref = orc.render_frame(case.desc, case.cam, opts, 1, st)
    want = int(L.orc_take_csg_truncations())
    print("placed, counted: %d truncated lists on the device, %d in the oracle" % (got, want))
    assert got > 0 and got == want
    assert np.array_equal(_bits32(a), _bits32(ref)) and rays == (st["primary"], st["shadow"])


def test_reduced_hit_stack_renders_the_placed_scene_unchanged():
    """One run of "placed" with the LDS hit stack reduced to 3 entries, through the diagnostics library in a fresh
    process, as test_gpu_parity.py::test_csg_hit_stack_overflow_is_redone_at_full_capacity does it: the frame bits and
    the ray counts are the oracle's."""
    code = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import chess2rt_amd as c2, oracle_lib as orc, csg_edge_scenes as es
from chess2rt_amd import _abi
case = es.load("placed")
ctx = c2.Context(0)
ctx.uploadScene(case.desc)
for taps in (_abi.TAPS_1, _abi.TAPS_REF5):
    opts = case.scene.renderOpts(taps=taps, count_rays=1)
    a = ctx.renderFrame(case.cam, opts)
    rays = ctx.rayStats()
    st = {}
    ref = orc.render_frame(case.desc, case.cam, opts, 0, st)
    assert np.array_equal(a.view(np.uint32), ref.view(np.uint32)), taps
    assert rays == (st["primary"], st["shadow"]), taps
print("ok")
'''
    env = dict(os.environ, C2RT_CSG_FIRST_CAP="3", C2RT_LIB_VARIANT="diag")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr
