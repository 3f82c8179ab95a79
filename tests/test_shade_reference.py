"""CPU: tests/shade_reference.py (a typed numpy restatement of the reference's shading stage, written from the D source)
against the oracle — the oracle's first independent check of Procedure2, Phong's strength != 1, many lights in list
order, dark lights and the bitmap / checker edge coordinates — plus the conditions that make the comparison mean
something (coverage counts, the cap on ambiguous samples) and a mutation check of the inputs.

"Bit for bit" below: every float of every sample that is not AMBIGUOUS (shade_reference: a pow / sin value within 4 fp64
ulp of a float32 rounding midpoint) has the oracle's bits; an ambiguous sample lies within the bounds obtained by moving
each such cast to its neighbour.  Samples whose only flag is a sine below 2^-100 (u or v of 0 or +-tiny on the
Procedure2 plane, a fixed handful of the crafted set) have no neighbour to move to and are compared bit for bit as
well; they are counted apart from the cap, which is about samples whose comparison is loosened."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import oracle_lib as orc
import shade_reference as sr
import shade_scenes as ss
from ray_query_util import oracle_trace, oracle_visibility

AMBIGUOUS_CAP = 0.001
MIN_REACH = 30
MIN_MUTATION_CHANGE = 0.01


@functools.lru_cache(maxsize=None)
def oracle_case(variant, name):
    """(tables, rays, oracle records, oracle visibility (n, n_lights), reference Shaded, seconds) — shared, read-only"""
    scene, _, _ = ss.load(variant)
    T = sr.Tables(scene.desc)
    rays = ss.ray_set(variant, name)
    t0 = time.time()
    recs = oracle_trace(scene.desc, rays)
    vis = oracle_visibility(scene.desc, sr.shadow_segments(T, rays[:, 3:], recs)).reshape(len(rays), -1)
    vis[recs["closest_node"] < 0] = 0
    ref = sr.shade(T, rays[:, 3:], recs, vis)
    return T, rays, recs, vis, ref, time.time() - t0


def changed(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=1)


# ---- (a) textures ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("node", [ss.GROUND, ss.CEILING, ss.PROC_PLANE])
def test_tex_color_matches_the_oracle_on_crafted_coordinates(node):
    scene, _, _ = ss.load("L2")
    T = sr.Tables(scene.desc)
    t = int(T.shader_texture[T.node_shader[node]])
    u, v = ss.CRAFTED[node]()
    got, ambiguous = sr.tex_color(T, t, u, v)
    want = np.zeros((len(u), 3), dtype=np.float32)
    L = orc.lib()
    for i in range(len(u)):
        L.orc_tex_color(scene.desc, t, float(u[i]), float(v[i]), want[i].ctypes.data_as(C.POINTER(C.c_float)))
    diff = changed(got, want)
    print("texture %d: %d samples, %d flagged, %d differ outside the flagged, %d inside" % (t, len(u), ambiguous.sum(), (diff & ~ambiguous).sum(), (diff & ambiguous).sum()))
    assert not (diff & ~ambiguous).any(), np.nonzero(diff & ~ambiguous)[0][:10]
    libm = sr.Libm(len(u))
    sr.tex_color(T, t, u, v, libm)
    assert not (diff & (libm.ambiguous == 0)).any()          # a tiny sine has no neighbour: bit-equal too
    assert (libm.ambiguous > 0).sum() <= max(1, AMBIGUOUS_CAP * len(u))


# ---- (b) frames ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("variant", ss.VARIANTS)
def test_reference_colours_equal_the_oracles_one_tap_frame(variant):
    scene, cam, opts = ss.load(variant)
    T, rays, recs, vis, ref, secs = oracle_case(variant, "screen")
    frame = orc.render_frame(scene.desc, cam, opts, 1).reshape(-1, 3)
    plain, outside = sr.compare(frame, ref)
    print("%s screen: %d samples, %d ambiguous, %d floats differ outside them, %d outside their bounds, %.1f s"
          % (variant, len(rays), ref.ambiguous.sum(), plain, outside, secs))
    assert plain == 0 and outside == 0


@pytest.mark.parametrize("variant", ["L1", "L5"])
def test_libm_free_variant_has_no_libm_on_its_path(variant):
    """what test_gpu_shade's outright bit identity rests on: without the Phong / Procedure2 nodes the reference meets
    no pow and no sin, and equals the oracle with no exception at all"""
    scene, cam, opts = ss.load(variant, True)
    T = sr.Tables(scene.desc)
    rays = ss.ray_set(variant, "screen")
    recs = oracle_trace(scene.desc, rays)
    vis = oracle_visibility(scene.desc, sr.shadow_segments(T, rays[:, 3:], recs)).reshape(len(rays), -1)
    ref = sr.shade(T, rays[:, 3:], recs, vis)
    assert ref.libm_calls == 0 and not ref.ambiguous.any()
    frame = orc.render_frame(scene.desc, cam, opts, 1).reshape(-1, 3)
    assert np.array_equal(frame.view(np.uint32), ref.rgb.view(np.uint32))


# ---- (c) conditions ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("variant", ss.VARIANTS)
def test_conditions_hold_on_reference_and_oracle_alone(variant):
    """Counted over the variant's three ray sets together (the planes are unbounded and horizontal: no camera sees all
    three, so node 2 is reached by the crafted and the random rays only); the cap holds for each set on its own."""
    reach = {}
    lit = None
    for name in ss.RAY_SETS:
        T, rays, recs, vis, ref, _ = oracle_case(variant, name)
        lit = T.lit()
        n = len(rays)
        print("%s %s: %d samples, %d near a midpoint, %d with a tiny sine" % (variant, name, n, ref.midpoint.sum(), ref.tiny.sum()))
        assert ref.midpoint.sum() <= AMBIGUOUS_CAP * n, (variant, name)
        assert ref.tiny.sum() <= (16 if name == "crafted" else 0), (variant, name)      # u or v in {0, +-tiny} only
        hit = recs["closest_node"] >= 0
        for node in range(T.n_nodes):
            reach["node %d" % node] = reach.get("node %d" % node, 0) + int((recs["closest_node"] == node).sum())
        for k, f in ref.flags.items():
            reach[k] = reach.get(k, 0) + int(f.sum())
        for l in (0, 1, 31, 32):
            if l < T.n_lights:
                reach["shadowed by light %d" % l] = reach.get("shadowed by light %d" % l, 0) + int((hit & (vis[:, l] == 0)).sum())
        if T.n_lights > 32:
            only = hit & (vis[:, :32][:, lit[:32]].sum(axis=1) == 0) & (vis[:, 32:].sum(axis=1) > 0)
            reach["lit only by a light >= 32"] = reach.get("lit only by a light >= 32", 0) + int(only.sum())
    print(variant, reach)
    wanted = ["node %d" % n for n in range(8)] + ["checker_color1", "checker_color2", "bitmap_red", "bitmap_wrapped_column",
                                                   "bitmap_wrapped_row", "costheta_le0_visible", "cosgamma_gt0", "cosgamma_le0",
                                                   "shadowed by light 0"]
    if len(lit) > 1:
        wanted.append("shadowed by light 1")
    if len(lit) > 32:
        wanted += ["shadowed by light 31", "shadowed by light 32", "lit only by a light >= 32"]
    for k in wanted:
        assert reach.get(k, 0) >= MIN_REACH, (variant, k, reach.get(k, 0))
    assert all(lit[l] for l in (0, 1, 31, 32) if l < len(lit))


# ---- (d) mutations -------------------------------------------------------------------------------------------------------------

# misreading -> (variant, ray set) that targets it
MUTATION_TARGETS = {
    "strength_ignored": ("L2", "screen"), "strength_on_lambert": ("L2", "screen"), "specular_times_diffuse": ("L2", "screen"),
    "lightdir_in_float": ("L2", "screen"), "weights_transposed": ("L5", "crafted"), "no_column_wrap": ("L5", "crafted"),
    "scaling_in_float": ("L5", "crafted"), "sin_in_float": ("L5", "crafted"), "uv_colors_swapped": ("L5", "crafted"),
    "dark_light_shifts_visibility": ("L4", "screen"), "light_32_dropped": ("L33", "screen"),
}


def test_every_named_misreading_has_a_target():
    assert sorted(MUTATION_TARGETS) == sorted(sr.MUTATIONS)


@pytest.mark.parametrize("mutation", sr.MUTATIONS)
def test_the_ray_sets_see_each_named_misreading(mutation):
    variant, name = MUTATION_TARGETS[mutation]
    T, rays, recs, vis, ref, _ = oracle_case(variant, name)
    wrong = sr.shade(T, rays[:, 3:], recs, vis, mutation)
    # a sample counts only if it leaves the bounds of the unmutated reference (so ambiguity cannot hide it)
    with np.errstate(invalid="ignore"):
        moved = (~((wrong.rgb >= ref.lo) & (wrong.rgb <= ref.hi))).any(axis=1) | (changed(wrong.rgb, ref.rgb) & ~ref.ambiguous)
    print("%s on %s %s: %d of %d samples change (%.1f %%)" % (mutation, variant, name, moved.sum(), len(rays), 100.0 * moved.mean()))
    assert moved.mean() >= MIN_MUTATION_CHANGE
