"""CPU: tests/geom_reference.py against the oracle where the CsgOp walk of rt/geometry.d:292-337 is decided by ties, odd
hit counts and leaf identity — tests/csg_edge_scenes.py: children that share face planes bit for bit (a cube minus an
adjacent cube), a leaf on both sides of an operator, Op(a, a), a Plane as an operand (isInside always false, one hit, so
the parity starts "inside"), depth 4, and the build-defined cap of 8 hits per child.  tests/test_geom_reference.py
stays clear of all of these (it requires zero ties and zero truncations on its scene); here the reference sorts tied
lists with the reference's own shell sort restated literally, so it is DEFINED on them, and the conditions below require
that the ray sets are full of them.

What the comparison rests on, and what it does not.  On the same trees a CPU trial found (and the counts printed below
repeat): exact ties are plentiful — the k-th hits of two children on a shared plane are the same double, whereas a first
and a second hit on it land within rounding of each other (the second is a restart's 1e-6 short) and the last bits
decide; the order of chain(leftData, rightData) decides hundreds of records; a STABLE sort in place of the shell sort
changes none (the two differ from length 4 up, on key patterns that need a first hit equal to a second hit), so
`stable_sort` is printed, not required; and the `ref i` rewind of the sort's `foreach` changes the work only.

Reach.  Every tree is hit by at least MIN_REACH rays of each ray set, with two exceptions that no camera can lift, on
the SCREEN set of scene "identity": Inter(a, b) of two adjacent cubes is hit only by rays that lie IN a shared plane
(every one of its hits exists through an exact tie L0 == R0; a ray that crosses the shared face meets a's exit a
restart's 1e-6 before b's entry), and Inter(a, a) only from inside a (from outside inR never leaves false).  Both are
held to MIN_REACH on the eyeless set, whose rays are aimed that way, and their screen counts are printed.

"Bit for bit" as in tests/test_geom_reference.py: node, leaf, dist, p, normal and non-sphere u, v have the oracle's bits,
sphere u, v agree within 1e-12, visibility byte for byte."""
import functools
import time

import numpy as np
import pytest

import csg_edge_scenes as es
import geom_reference as gr
import oracle_lib as orc
import shade_reference as sr
from ray_query_util import assert_records_match_oracle, oracle_trace, oracle_visibility

AMBIGUOUS_CAP = 0.001       # tests/test_shade_reference.py
MIN_REACH = 30              # tests/test_shade_reference.py
MIN_MUTATION_RECORDS = 30   # tests/test_geom_reference.py
MIN_TIED_AB = 10            # Inter(a, b): a trial of 1500 random rays had 26 hits, all through ties
FLAGS = ("tied_list", "odd_list", "capped_list", "right_entry_toggles_left", "left_entry_toggles_right")
AE_TREES = {"identity": ("diff_ae", "union_ae", "inter_ae", "union_ea", "inter_ea", "diff_ea"), "placed": ("diff_ae", "inter_ae")}
UNREACHABLE_FROM_A_CAMERA = {("identity", "screen"): ("inter_ab", "inter_aa")}      # the docstring's two exceptions
CASES = [(s, n) for s in es.SCENE_NAMES for n in es.RAY_SETS]


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(scene, name):
    """oracle and reference records and visibility of one ray set — computed once, shared, read-only"""
    c = Case()
    c.scene = es.load(scene)
    c.T, c.Ts = gr.Tables(c.scene.desc), sr.Tables(c.scene.desc)
    c.rays = es.ray_set(scene, name)
    L = orc.lib()
    L.orc_take_csg_truncations()
    t0 = time.time()
    c.orc = oracle_trace(c.scene.desc, c.rays)
    c.orc_truncations = int(L.orc_take_csg_truncations())
    t1 = time.time()
    c.ref, c.trace = gr.trace(c.T, c.rays)
    t2 = time.time()
    c.segs = sr.shadow_segments(c.Ts, c.rays[:, 3:], c.ref)
    c.orc_vis = oracle_visibility(c.scene.desc, c.segs).reshape(len(c.rays), -1)
    L.orc_take_csg_truncations()
    vis, occ, c.vis_trace = gr.test_visibility(c.T, c.segs)
    c.vis, c.occluder = vis.reshape(len(c.rays), -1), occ.reshape(len(c.rays), -1)
    c.hit = c.ref["closest_node"] >= 0
    c.seconds = (t1 - t0, t2 - t1, time.time() - t2)
    return c


def bits_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    d = a.view(np.uint64) != b.view(np.uint64)
    return d.reshape(len(a), -1).any(axis=1)


def changed_records(c, mutation):
    """records of `c` that a misreading changes: any bit of the record, or the visibility of its shadow segments (those of
    the UNMUTATED records) — as tests/test_geom_reference.py counts"""
    wrong, _ = gr.trace(c.T, c.rays, mutation)
    rec = np.zeros(len(c.rays), dtype=bool)
    for f in ("closest_node", "leaf_geom"):
        rec |= wrong[f] != c.ref[f]
    for f in ("dist", "u", "v", "p", "normal"):
        rec |= bits_differ(wrong[f], c.ref[f])
    vis, _, _ = gr.test_visibility(c.T, c.segs, mutation)
    rec |= c.hit & (vis.reshape(c.vis.shape) != c.vis).any(axis=1)
    return rec


# ---- (a) comparison ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("scene,name", CASES)
def test_reference_records_and_visibility_equal_the_oracles(scene, name):
    c = case(scene, name)
    print("%s %s: %d rays, oracle %.2f s, reference %.2f s, visibility %.2f s; ties %d + %d, truncations %d + %d"
          % ((scene, name, len(c.rays)) + c.seconds + (c.trace.ties, c.vis_trace.ties, c.trace.truncations, c.vis_trace.truncations)))
    assert np.array_equal(c.ref["closest_node"], c.orc["closest_node"]), np.nonzero(c.ref["closest_node"] != c.orc["closest_node"])[0][:10]
    assert np.array_equal(c.ref["leaf_geom"], c.orc["leaf_geom"])
    for f in ("dist", "p", "normal"):
        assert not bits_differ(c.ref[f], c.orc[f]).any(), (f, np.nonzero(bits_differ(c.ref[f], c.orc[f]))[0][:10])
    sphere = c.hit & (c.T.geom_type[np.where(c.hit, c.ref["leaf_geom"], 0)] == gr.GEOM_SPHERE)
    for f in ("u", "v"):
        d = bits_differ(c.ref[f], c.orc[f])
        assert not (d & ~sphere).any(), (f, np.nonzero(d & ~sphere)[0][:10])
    assert_records_match_oracle(c.ref, c.orc, "%s %s" % (scene, name))            # sphere u, v within 1e-12
    assert c.vis.dtype == c.orc_vis.dtype == np.uint8 and np.array_equal(c.vis, c.orc_vis)


# ---- (b) conditions ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("scene,name", CASES)
def test_every_tree_is_reached_and_only_the_cap_tree_is_capped(scene, name):
    """at least MIN_REACH hits on each tree (the docstring's two exceptions are printed); hit lists reach the cap under
    the cap tree of "placed" (on the screen set: the pixel whose ray is the tree's axis) and under no other tree, and
    the oracle counts as many capped lists for the same rays as the reference"""
    c = case(scene, name)
    names = [t[0] for t in es.TREES[scene]]
    reach = {t: int((c.orc["closest_node"] == es.node_index(scene, t)).sum()) for t in names}
    print("%s %s reach per tree: %s, ground %d, misses %d" % (scene, name, reach, int((c.orc["closest_node"] == es.GROUND).sum()), int((~c.hit).sum())))
    excused = UNREACHABLE_FROM_A_CAMERA.get((scene, name), ())
    for t in names:
        assert reach[t] >= MIN_REACH or t in excused, (t, reach[t])
    trunc = c.trace.node_truncations + c.vis_trace.node_truncations
    print("  lists at the cap per node (records + visibility): %s; the oracle's count for the records: %d" % (trunc.tolist(), c.orc_truncations))
    for t in names:
        if t != "cap":
            assert trunc[es.node_index(scene, t)] == 0, t
    assert trunc[es.GROUND] == 0
    assert c.orc_truncations == c.trace.truncations
    if "cap" in names:
        assert c.trace.node_truncations[es.node_index(scene, "cap")] > 0 and c.orc_truncations > 0
    else:
        assert c.orc_truncations == 0


@pytest.mark.parametrize("scene", es.SCENE_NAMES)
def test_ties_shared_leaves_planes_and_depth_four_decide_records(scene):
    """Over the scene's two ray sets, from the reference's flags: at least 30 rays with a tied list on each (a, e)-type
    tree and at least 10 on Inter(a, b); at least 30 hits on an Op(a, a) tree and 30 whose leaf is a Plane operand
    (scene "identity"); hits on the depth-4 tree decided by an entry of the right list (scene "placed")."""
    cs = [case(scene, n) for n in es.RAY_SETS]

    def count(flag, tree):
        return sum(int(c.trace.flag(flag, es.node_index(scene, tree)).sum()) for c in cs)

    def hits(tree):
        return sum(int((c.ref["closest_node"] == es.node_index(scene, tree)).sum()) for c in cs)
    print("%s: equal neighbours met in sorted lists, per node: %s" % (scene, sum(c.trace.node_ties for c in cs).tolist()))
    for t in AE_TREES[scene]:
        print("  %s: %d rays with a tied list" % (t, count("tied_list", t)))
        assert count("tied_list", t) >= MIN_REACH, t
    if scene == "identity":
        print("  inter_ab: %d rays with a tied list, %d hits" % (count("tied_list", "inter_ab"), hits("inter_ab")))
        assert count("tied_list", "inter_ab") >= MIN_TIED_AB
        aa = {t: hits(t) for t in ("union_aa", "inter_aa", "diff_aa")}
        plane = sum(int((c.hit & (c.T.geom_type[np.where(c.hit, c.ref["leaf_geom"], 0)] == gr.GEOM_PLANE) & (c.ref["closest_node"] != es.GROUND)).sum()) for c in cs)
        print("  hits on Op(a, a): %s; hits whose leaf is a Plane operand: %d" % (aa, plane))
        assert max(aa.values()) >= MIN_REACH and plane >= MIN_REACH
    else:
        node = es.node_index(scene, "depth4")
        by_right = sum(int(c.trace.hits.right[c.ref["closest_node"] == node].sum()) for c in cs)
        print("  depth-4 tree: %d hits, %d decided by an entry of the right list" % (hits("depth4"), by_right))
        assert by_right >= 1


def test_each_flag_of_the_walk_is_set_on_thirty_rays():
    total = {f: 0 for f in FLAGS}
    for scene, name in CASES:
        c = case(scene, name)
        row = {f: int(c.trace.flag(f).sum()) for f in FLAGS}
        print("%s %s: %s" % (scene, name, row))
        for f in FLAGS:
            total[f] += row[f]
    print("over the ray sets: %s" % total)
    for f in FLAGS:
        assert total[f] >= MIN_REACH, f


@pytest.mark.parametrize("scene", es.SCENE_NAMES)
def test_wave_sized_groups_of_regular_rays_and_of_all_but_one(scene):
    """The device decides a CsgOp of two leaves by comparisons when EVERY lane of a wave has 0 or 2 hits per child and
    distinct distances, and sorts and walks otherwise.  For two depth-1 tie trees the eyeless set opens with a
    64-aligned group of 64 rays with no tied, odd, long or capped list under that tree, then a 64-aligned group with
    exactly one tied or odd ray among 63 such — by the reference's flags."""
    c = case(scene, "eyeless")
    for k, tree in enumerate(es.GROUP_TREES[scene]):
        node = es.node_index(scene, tree)
        odd = c.trace.flag("tied_list", node) | c.trace.flag("odd_list", node)
        irregular = odd | c.trace.flag("long_list", node) | c.trace.flag("capped_list", node)
        a, b = slice(128 * k, 128 * k + 64), slice(128 * k + 64, 128 * k + 128)
        print("%s %s: group of 64 regular rays with %d hits on the tree; group of 63 + 1 with %d" %
              (scene, tree, int((c.ref["closest_node"][a] == node).sum()), int((c.ref["closest_node"][b] == node).sum())))
        assert irregular[a].sum() == 0
        assert irregular[b].sum() == 1 and odd[b].sum() == 1
        assert (c.ref["closest_node"][a] == node).sum() >= 16 and (c.ref["closest_node"][b] == node).sum() >= 16


def test_carved_parts_on_the_screen():
    """what tests/test_gpu_csg_edge.py's carved-tile case rests on (scene "identity"): for Diff(a, e) and Diff(a, b), at
    least 30 pixels seen through the carved part (csg_edge_scenes.carved_box), at least 30 ground pixels cut off from a light by the
    node, an 8x8 tile wholly seen through it and one that its boundary cuts"""
    c = case("identity", "screen")
    for tree in es.CARVED:
        node = es.node_index("identity", tree)
        through = es.seen_through(c.rays, c.ref, *es.carved_box("identity", tree))
        shaded = (c.ref["closest_node"] == es.GROUND) & (c.occluder == node).any(axis=1)
        whole, cut = es.tiles(through)
        print("%s: %d pixels seen through the carved part (%d tiles wholly, %d cut), %d ground pixels shaded by it"
              % (tree, int(through.sum()), whole, cut, int(shaded.sum())))
        assert through.sum() >= MIN_REACH and shaded.sum() >= MIN_REACH
        assert whole >= 1 and cut >= 1


# ---- (c) mutations -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mutation", gr.CSG_EDGE_MUTATIONS)
def test_the_ray_sets_see_each_named_misreading(mutation):
    changed = 0
    for scene, name in CASES:
        rec = changed_records(case(scene, name), mutation)
        print("%s on %s %s: %d of %d records change" % (mutation, scene, name, rec.sum(), len(rec)))
        changed += int(rec.sum())
    assert changed >= MIN_MUTATION_RECORDS


def test_a_stable_sort_is_reported_not_required():
    """the count is printed: a stable sort in place of the shell sort is not observable on these inputs (docstring)"""
    for scene, name in CASES:
        c = case(scene, name)
        rec = changed_records(c, "stable_sort")
        print("stable_sort on %s %s: %d of %d records change (%d rays walked a tied list)" % (scene, name, rec.sum(), len(rec), int(c.trace.flag("tied_list").sum())))


def test_the_literal_sort_sorts_and_differs_from_a_stable_one_only_in_the_order_of_equal_keys():
    """gr.shell_sort on seeded lists up to length 16 with repeated keys: the keys come out sorted; [2, 3, 1, 2] is a
    list on which the order of the equal keys differs from a stable sort's"""
    rng = np.random.RandomState(5)
    for n in range(0, 17):
        for _ in range(200):
            keys = rng.randint(0, 4, size=n).astype(float).tolist()
            perm = gr.shell_sort(keys)
            assert sorted(perm) == list(range(n)) and [keys[i] for i in perm] == sorted(keys)
    assert gr.shell_sort([2.0, 3.0, 1.0, 2.0]) == [2, 3, 0, 1]
    assert list(np.argsort([2.0, 3.0, 1.0, 2.0], kind="stable")) == [2, 0, 3, 1]


# ---- (d) a frame with no oracle in it, against the oracle's -----------------------------------------------------------------


@pytest.mark.parametrize("scene", es.SCENE_NAMES)
def test_reference_frame_equals_the_oracles_one_tap_frame(scene):
    c = case(scene, "screen")
    shaded = sr.shade(c.Ts, c.rays[:, 3:], c.ref, c.vis)
    frame = orc.render_frame(c.scene.desc, c.scene.cam, c.scene.opts, 1).reshape(-1, 3)
    plain, outside = sr.compare(frame, shaded)
    share = float(shaded.ambiguous.mean())
    print("%s: %d samples, ambiguous share %.5f, %d floats differ outside them, %d outside their bounds" % (scene, len(c.rays), share, plain, outside))
    assert share <= AMBIGUOUS_CAP
    assert plain == 0 and outside == 0
