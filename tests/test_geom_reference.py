"""CPU: tests/geom_reference.py (a typed numpy restatement of the reference's geometry stage, written from the D source)
against the oracle on the one scene of the suite whose node matrices have off-diagonal entries (tests/geom_scenes.py:
rotations, rotation + non-uniform scale, shears with M != M^T, a finite Plane limit, Union / Inter / Diff and a nested
tree under rotations) — the oracle's first independent check of Node.intersect's general branch, of Cube, Sphere and
Plane as a whole and of the CsgOp walk — plus the conditions that make the comparison mean something (reach counts,
branches taken, no hit-list cap, no sort ties), a mutation check, a frame computed with no oracle in it, and the scene
plan's flags and world boxes for these matrices.

"Bit for bit": closest_node, leaf_geom, dist, p, normal and the u, v of plane and cube leaves have the oracle's bits;
u, v of sphere leaves (libm and the reference's 80-bit PI on the oracle's side, mpmath rounded once on the reference's)
agree within the project's 1e-12."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import geom_reference as gr
import geom_scenes as gs
import oracle_lib as orc
import shade_reference as sr
from ray_query_util import assert_records_match_oracle, oracle_trace, oracle_visibility

AMBIGUOUS_CAP = 0.001       # tests/test_shade_reference.py
MIN_REACH = 30              # tests/test_shade_reference.py
MIN_MUTATION_RECORDS = 30
K_NODE_AXIS_PLANE, K_NODE_PLANE_NORMAL = 4, 8      # chess2rt_amd/csrc/c2rt_device.h


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(variant, name):
    """oracle and reference records and visibility of one ray set — computed once, shared, read-only"""
    c = Case()
    c.scene = gs.load(variant)
    c.T, c.Ts = gr.Tables(c.scene.desc), sr.Tables(c.scene.desc)
    c.rays = gs.ray_set(name)
    t0 = time.time()
    c.orc = oracle_trace(c.scene.desc, c.rays)
    t1 = time.time()
    c.ref, c.trace = gr.trace(c.T, c.rays)
    t2 = time.time()
    c.segs = sr.shadow_segments(c.Ts, c.rays[:, 3:], c.ref)
    c.orc_vis = oracle_visibility(c.scene.desc, c.segs).reshape(len(c.rays), -1)
    vis, occ, c.vis_trace = gr.test_visibility(c.T, c.segs)
    c.vis, c.occluder = vis.reshape(len(c.rays), -1), occ.reshape(len(c.rays), -1)
    c.hit = c.ref["closest_node"] >= 0
    c.seconds = (t1 - t0, t2 - t1, time.time() - t2)
    return c


def bits_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    d = a.view(np.uint64) != b.view(np.uint64)
    return d.reshape(len(a), -1).any(axis=1)


# ---- (a) comparison ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", gs.RAY_SETS)
@pytest.mark.parametrize("variant", gs.VARIANTS)
def test_reference_records_and_visibility_equal_the_oracles(variant, name):
    c = case(variant, name)
    print("%s %s: %d rays, oracle %.2f s, reference %.2f s, visibility %.2f s" % ((variant, name, len(c.rays)) + c.seconds))
    assert np.array_equal(c.ref["closest_node"], c.orc["closest_node"])
    assert np.array_equal(c.ref["leaf_geom"], c.orc["leaf_geom"])
    for f in ("dist", "p", "normal"):
        assert not bits_differ(c.ref[f], c.orc[f]).any(), (f, np.nonzero(bits_differ(c.ref[f], c.orc[f]))[0][:10])
    sphere = c.hit & (c.T.geom_type[np.where(c.hit, c.ref["leaf_geom"], 0)] == gr.GEOM_SPHERE)
    for f in ("u", "v"):
        d = bits_differ(c.ref[f], c.orc[f])
        assert not (d & ~sphere).any(), (f, np.nonzero(d & ~sphere)[0][:10])
    assert sphere.sum() >= MIN_REACH and (c.hit & ~sphere).sum() >= MIN_REACH
    assert_records_match_oracle(c.ref, c.orc, "%s %s" % (variant, name))          # sphere u, v within 1e-12
    assert c.vis.dtype == c.orc_vis.dtype == np.uint8 and np.array_equal(c.vis, c.orc_vis)


# ---- (b) conditions ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", gs.RAY_SETS)
@pytest.mark.parametrize("variant", gs.VARIANTS)
def test_coverage_conditions(variant, name):
    """Each ray set on its own: at least MIN_REACH hits on EACH node (the oracle's records); each cube face pair and
    each sphere root as the statement that made a surviving record; a flipped and an unflipped CsgDiff normal; a hit on
    the nested tree decided by an entry of the right child's list; a ray that passed the Plane's distance test and was
    turned away by the finite limit; no hit list at the cap; no equal distances in a sorted
    list.  The branch flags come from the reference, whose records the comparison above holds equal to the oracle's."""
    c = case(variant, name)
    reach = [int((c.orc["closest_node"] == n).sum()) for n in range(gs.N_NODES)]
    print("%s %s reach per node: %s, misses %d" % (variant, name, reach, int((~c.hit).sum())))
    assert min(reach) >= MIN_REACH, reach
    tag = c.trace.hits.tag[c.hit]
    counts = np.bincount(tag[tag >= 0], minlength=9)
    print("  cube faces -y +y -x +x -z +z: %s, sphere roots near, far: %s" % (counts[:6].tolist(), counts[6:8].tolist()))
    for pair in range(3):
        assert counts[2 * pair] + counts[2 * pair + 1] >= 1, ("cube face pair", pair)
    assert counts[gr.TAG_SPHERE_NEAR] >= 1 and counts[gr.TAG_SPHERE_FAR] >= 1
    for node in gs.DIFF_NODES:
        m = c.ref["closest_node"] == node
        flipped, plain = int(c.trace.hits.flip[m].sum()), int((~c.trace.hits.flip[m]).sum())
        print("  CsgDiff node %d: %d flipped, %d unflipped" % (node, flipped, plain))
        assert flipped >= 1 and plain >= 1, node
    by_right = int(c.trace.hits.right[c.ref["closest_node"] == gs.NESTED].sum())
    limit = int(c.trace.flags["plane_limit_rejects"].sum())
    print("  nested tree decided by a right-child entry: %d; turned away by the limit: %d" % (by_right, limit))
    assert by_right >= 1 and limit >= 1
    assert c.trace.truncations == 0 and c.vis_trace.truncations == 0
    assert c.trace.ties == 0 and c.vis_trace.ties == 0
    L = orc.lib()
    L.orc_take_csg_truncations()
    oracle_trace(c.scene.desc, c.rays[:: 7])
    assert L.orc_take_csg_truncations() == 0


@pytest.mark.parametrize("variant", gs.VARIANTS)
def test_each_general_node_gives_both_visibility_answers(variant):
    """over the two ray sets together (no camera ray ends behind the SLOPE, so only eyeless rays find it between a
    point and a light): each general node is the occluder of a shadow segment, and a segment that STARTS on it is
    visible (the node does not shade itself from a light it faces)"""
    for node in gs.GENERAL:
        blocked = seen = 0
        for name in gs.RAY_SETS:
            c = case(variant, name)
            blocked += int((c.hit[:, None] & (c.occluder == node)).sum())
            seen += int((c.hit[:, None] & (c.vis == 1) & (c.ref["closest_node"] == node)[:, None]).sum())
        print("%s node %d: occluder of %d segments, origin of %d visible ones" % (variant, node, blocked, seen))
        assert blocked >= 1 and seen >= 1, node


def test_shadows_of_the_rotated_cube_and_the_sheared_sphere_fall_on_the_ground():
    """what tests/test_gpu_geom.py's shadow case rests on: light 0 is cut off from at least 30 screen pixels of the
    ground by each of the two nodes"""
    c = case("L1", "screen")
    ground = c.ref["closest_node"] == gs.GROUND
    for node in (gs.ROT_CUBE, gs.SHEAR_SPHERE):
        n = int((ground & (c.occluder[:, 0] == node)).sum())
        print("ground pixels shaded from light 0 by node %d: %d" % (node, n))
        assert n >= MIN_REACH


# ---- (c) mutations -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mutation", gr.GEOM_MUTATIONS)
def test_the_ray_sets_see_each_named_misreading(mutation):
    """a record counts when any of its bits changes, or the visibility of its shadow segments does (the segments are
    those of the UNMUTATED records, so that a changed answer is the visibility statement's own)"""
    changed = 0
    for name in gs.RAY_SETS:
        c = case("L2", name)
        wrong, _ = gr.trace(c.T, c.rays, mutation)
        rec = np.zeros(len(c.rays), dtype=bool)
        for f in ("closest_node", "leaf_geom"):
            rec |= wrong[f] != c.ref[f]
        for f in ("dist", "u", "v", "p", "normal"):
            rec |= bits_differ(wrong[f], c.ref[f])
        vis, _, _ = gr.test_visibility(c.T, c.segs, mutation)
        rec |= c.hit & (vis.reshape(c.vis.shape) != c.vis).any(axis=1)
        print("%s on %s: %d of %d records change" % (mutation, name, rec.sum(), len(rec)))
        changed += int(rec.sum())
    assert changed >= MIN_MUTATION_RECORDS


# ---- (d) a frame with no oracle in it, against the oracle's -----------------------------------------------------------------


@pytest.mark.parametrize("variant", gs.VARIANTS)
def test_reference_frame_equals_the_oracles_one_tap_frame(variant):
    c = case(variant, "screen")
    shaded = sr.shade(c.Ts, c.rays[:, 3:], c.ref, c.vis)
    frame = orc.render_frame(c.scene.desc, c.scene.cam, c.scene.opts, 1).reshape(-1, 3)
    plain, outside = sr.compare(frame, shaded)
    share = float(shaded.ambiguous.mean())
    print("%s: %d samples, ambiguous share %.5f, %d floats differ outside them, %d outside their bounds" % (variant, len(c.rays), share, plain, outside))
    assert share <= AMBIGUOUS_CAP
    assert plain == 0 and outside == 0


# ---- (e) the scene plan ----------------------------------------------------------------------------------------------------------


def _plan_nodes(desc):
    import test_scene_plan as tsp

    L = tsp.lib()
    L.c2rt_plan_node.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)]
    plan = tsp.Plan()
    st, msg = plan.plan(C.pointer(desc))
    assert st == 0, msg
    facts, boxed = plan.facts()
    nodes = []
    for n in range(facts.n_nodes):
        flags, b, corners = C.c_uint32(), C.c_uint8(), (C.c_double * 24)()
        assert L.c2rt_plan_node(plan.h, n, C.byref(flags), C.byref(b), corners) == 1
        assert b.value == boxed[n]
        nodes.append((flags.value, b.value, np.array(list(corners)).reshape(8, 3)))
    return facts, nodes


def test_scene_plan_flags_and_world_boxes():
    """The rotated plane keeps its precomputed world normal but is no axis plane; no shortcut instance is picked;
    every general node with a bounded geometry is boxed (a Plane has no box), and every reference hit point on a boxed
    node lies inside the hull of that node's eight world corners — the parallelepiped they span, so a box built from
    the wrong matrix loses points."""
    scene = gs.load("L1")
    facts, nodes = _plan_nodes(scene.desc)
    flags = nodes[gs.SLOPE][0]
    assert flags & K_NODE_PLANE_NORMAL and not flags & K_NODE_AXIS_PLANE
    assert facts.planes_only == 0 and facts.all_identity == 0 and facts.ground_node == gs.GROUND
    for node in gs.GENERAL:
        assert nodes[node][1] == (node != gs.SLOPE), node
    checked = 0
    for name in gs.RAY_SETS:
        c = case("L1", name)
        for node, (_, boxed, corners) in enumerate(nodes):
            p = c.ref["p"][c.ref["closest_node"] == node]
            if not boxed or not len(p):
                continue
            # corner k = (k & 1, k & 2, k & 4) of the object box: c0 and its three edges span the hull
            basis = np.stack([corners[1] - corners[0], corners[2] - corners[0], corners[4] - corners[0]])
            coeff = np.linalg.solve(basis.T, (p - corners[0]).T).T
            assert (coeff >= -1e-9).all() and (coeff <= 1 + 1e-9).all(), (name, node, coeff.min(), coeff.max())
            checked += len(p)
    assert checked >= 10 * MIN_REACH
