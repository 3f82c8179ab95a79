"""GPU: the general branch of the node transform (rotations, shears with M != M^T, rotation + non-uniform scale), the
precomputed world normal of a rotated Plane, a finite Plane limit and Union / Inter / Diff / nested CSG under rotated
matrices, against tests/geom_reference.py — a typed numpy restatement of the reference's geometry stage written from the
D source, which tests/test_geom_reference.py holds against the oracle on the CPU.  With tests/shade_reference.py behind
it the frames below are compared with a frame that has no oracle anywhere in it: rays -> records -> visibility ->
colour; and with tests/camera_reference.py in front of it the five-tap frame is computed from the camera's frame alone:
sub-pixel rays -> records -> visibility -> colour -> the fp32 sum / 5.  Scene and rays: tests/geom_scenes.py (61x47:
partial 8x8 tiles on both edges; 2000 eyeless rays).

Tolerances are the ones the project already holds the device to (ray_query_util.assert_records_match_oracle): node and
leaf equal, dist and p bit for bit, normal within 1e-15, u, v within 1e-12; visibility byte for byte; frames under
shade_reference.compare (bit for bit outside the samples whose pow lies at a float32 rounding midpoint)."""
import functools

import numpy as np
import pytest

import camera_reference as cr
import camera_scenes as cs
import chess2rt_amd as c2
import geom_reference as gr
import geom_scenes as gs
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
def reference(variant, name):
    """the reference's records, shadow segments, visibility, occluders and (screen set) colours — once, read-only"""
    r = Ref()
    scene = gs.load(variant)
    T, r.Ts = gr.Tables(scene.desc), sr.Tables(scene.desc)
    r.rays = gs.ray_set(name)
    r.recs, _ = gr.trace(T, r.rays)
    r.segs = sr.shadow_segments(r.Ts, r.rays[:, 3:], r.recs)
    vis, occ, _ = gr.test_visibility(T, r.segs)
    r.vis, r.occluder = vis.reshape(len(r.rays), -1), occ.reshape(len(r.rays), -1)
    r.shaded = sr.shade(r.Ts, r.rays[:, 3:], r.recs, r.vis) if name == "screen" else None
    return r


@functools.lru_cache(maxsize=None)
def five_tap_reference(variant):
    """camera_reference.render_frame of the variant's camera frame at five taps — once, read-only"""
    scene = gs.load(variant)
    return cr.render_frame((gr.Tables(scene.desc), sr.Tables(scene.desc)), cs.from_abi(scene.cam), cr.Opts(gs.W, gs.H, taps=cr.TAPS_REF5))


_gpu_cases = {}


def gpu_case(gpu_ctx, variant):
    """uploads the variant; the queries run once per variant and are shared by the tests below (read-only)"""
    scene = gs.load(variant)
    gpu_ctx.uploadScene(scene.desc)
    if variant not in _gpu_cases:
        out = {}
        for name in gs.RAY_SETS:
            r = reference(variant, name)
            rec, rgb = gpu_ctx.traceRays(r.rays)
            out[name] = (rec, rgb, gpu_ctx.testVisibility(r.segs))
        _gpu_cases[variant] = out
    return _gpu_cases[variant]


def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("variant", gs.VARIANTS)
def test_queries_equal_the_reference(gpu_ctx, variant):
    for name, (rec, rgb, vis) in gpu_case(gpu_ctx, variant).items():
        r = reference(variant, name)
        with np.errstate(invalid="ignore"):
            hit = r.recs["closest_node"] >= 0
            print("%s %s: %d rays; max |normal - ref| %.3g, max |u - ref| %.3g, max |v - ref| %.3g, visibility differs on %d of %d"
                  % (variant, name, len(r.rays), np.abs(rec["normal"][hit] - r.recs["normal"][hit]).max(),
                     np.nanmax(np.abs(rec["u"][hit] - r.recs["u"][hit])), np.nanmax(np.abs(rec["v"][hit] - r.recs["v"][hit])),
                     int((vis != r.vis.ravel()).sum()), vis.size))
        assert_records_match_oracle(rec, r.recs, "%s %s" % (variant, name))
        assert vis.dtype == np.uint8 and np.array_equal(vis, r.vis.ravel()), (variant, name)


@pytest.mark.parametrize("variant", gs.VARIANTS)
def test_hit_planes_equal_the_query_of_the_screen_rays(gpu_ctx, variant):
    scene = gs.load(variant)
    rec, rgb, _ = gpu_case(gpu_ctx, variant)["screen"]
    planes = gpu_ctx.renderHits(scene.cam, scene.opts)
    n = gs.W * gs.H
    assert np.array_equal(planes["node"].ravel(), rec["closest_node"]) and np.array_equal(planes["leaf"].ravel(), rec["leaf_geom"])
    for plane, want in (("dist", rec["dist"]), ("p", rec["p"]), ("normal", rec["normal"]), ("uv", np.stack([rec["u"], rec["v"]], axis=1))):
        assert np.array_equal(np.ascontiguousarray(planes[plane]).reshape(n, -1).view(np.uint64),
                              np.ascontiguousarray(want).reshape(n, -1).view(np.uint64)), (variant, plane)
    assert np.array_equal(_bits32(planes["rgb"]).reshape(n, 3), _bits32(rgb)), variant


@pytest.mark.parametrize("variant", gs.VARIANTS)
def test_frame_equals_the_frame_computed_without_the_oracle(gpu_ctx, variant):
    """renderFrame, one tap: the lean instance with every cull active (screen rectangles and hulls of the sheared world
    boxes, ground shadow rectangles, void tiles of DIFF_ID, the silhouette of SPHERE_ID), against shade_reference.shade
    of the REFERENCE's records and visibility.  Five taps are compared with camera_reference.render_frame, which makes
    the sub-pixel rays itself, under its interval rule (both counts 0), and with the oracle under the suite's TOL."""
    scene = gs.load(variant)
    gpu_case(gpu_ctx, variant)
    r = reference(variant, "screen")
    assert r.shaded.ambiguous.mean() <= AMBIGUOUS_CAP
    before = gpu_ctx.exactRedos()
    frame = gpu_ctx.renderFrame(scene.cam, scene.opts)
    redone = gpu_ctx.exactRedos() - before
    plain, outside = sr.compare(frame, r.shaded)
    print("%s frame: %d tiles redone exactly, %d ambiguous samples, %d floats differ outside them, %d outside their bounds"
          % (variant, redone, int(r.shaded.ambiguous.sum()), plain, outside))
    assert plain == 0 and outside == 0, (variant, plain, outside)
    assert redone == 0, "the lean instance handed tiles to the exact one"
    batch = gpu_ctx.renderFrames(scene.cams, scene.opts)
    for i, cam in enumerate(scene.cams):
        single = frame if i == 0 else gpu_ctx.renderFrame(cam, scene.opts)
        assert np.array_equal(_bits32(batch[i]), _bits32(single)), (variant, i)
    opts5 = scene.scene.renderOpts(taps=_abi.TAPS_REF5)
    frame5 = gpu_ctx.renderFrame(scene.cam, opts5)
    five = five_tap_reference(variant)
    held = float((five.ambiguous | five.wide).mean())
    plain5, outside5 = cr.compare(frame5, five)
    print("%s five taps against the reference: %d pixels held to an interval, %d floats differ, %d outside their bounds"
          % (variant, int((five.ambiguous | five.wide).sum()), plain5, outside5))
    assert held <= 5 * AMBIGUOUS_CAP
    assert plain5 == 0 and outside5 == 0, (variant, plain5, outside5)
    md, nbad, nne = maxdiff(frame5, orc.render_frame(scene.desc, scene.cam, opts5, 0))
    print("%s five taps against the oracle: max|d|=%.3g, differing floats: %d" % (variant, md, nne))
    assert md <= TOL and nbad == 0


def test_two_slot_context_renders_the_same_frame_bits(gpu_ctx):
    """the multi-light instance dealt in strips to two slots of one device (ids repeated)"""
    scene = gs.load("L2")
    gpu_case(gpu_ctx, "L2")
    frame = gpu_ctx.renderFrame(scene.cam, scene.opts)
    multi = c2.Context(devices=[0, 0])
    try:
        assert multi.deviceCount == 2
        multi.uploadScene(scene.desc)
        assert np.array_equal(_bits32(multi.renderFrame(scene.cam, scene.opts)), _bits32(frame))
    finally:
        multi.close()


@pytest.mark.parametrize("node", [gs.ROT_CUBE, gs.SHEAR_SPHERE])
def test_shadow_of_a_general_node_on_the_ground(gpu_ctx, node):
    """the ground's shadow rectangle of a node is cut from its (rotated, sheared) world box: a wrong box loses these
    pixels — ground pixels that the reference finds cut off from light 0 by this node"""
    scene = gs.load("L1")
    _, _, vis = gpu_case(gpu_ctx, "L1")["screen"]
    r = reference("L1", "screen")
    shaded = (r.recs["closest_node"] == gs.GROUND) & (r.vis[:, 0] == 0) & (r.occluder[:, 0] == node)
    print("node %d shades %d ground pixels from light 0" % (node, int(shaded.sum())))
    assert shaded.sum() >= MIN_REACH
    assert not vis.reshape(r.vis.shape)[shaded, 0].any()
    frame = gpu_ctx.renderFrame(scene.cam, scene.opts).reshape(-1, 3)[shaded]
    sub = sr.Shaded()
    for f in ("rgb", "lo", "hi", "ambiguous"):
        setattr(sub, f, getattr(r.shaded, f)[shaded])
    assert sr.compare(frame, sub) == (0, 0)
