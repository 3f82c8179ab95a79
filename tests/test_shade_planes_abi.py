"""Shading planes, CPU side: the ABI (a C program against the headers, the five entry points refusing a null context),
the entitlement of the GPU tests' yardstick — the three parts of tests/shade_parts_reference.py recombine bit for bit to
shade_reference's colour on the oracle's records and visibility — and the preconditions of the GPU tests, asserted on
the oracle alone.  No GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import shade_parts_reference as sp
import shade_reference as sr
import shade_scenes as ss
from chess2rt_amd import _abi
from golden_configs import SCENES
from ray_query_util import oracle_trace, oracle_visibility, screen_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_REACH = 30

C_PROGRAM = r"""
#include <stddef.h>
#include <stdint.h>
#include "c2rt.h"
#include "c2rt_host.h"
_Static_assert(sizeof(c2rt_shade_planes) == 48, "c2rt_shade_planes");
_Static_assert(offsetof(c2rt_shade_planes, node) == 0 && offsetof(c2rt_shade_planes, albedo) == 8 && offsetof(c2rt_shade_planes, light) == 16 &&
               offsetof(c2rt_shade_planes, specular) == 24 && offsetof(c2rt_shade_planes, visible) == 32 && offsetof(c2rt_shade_planes, rgb) == 40,
               "c2rt_shade_planes members");
_Static_assert(C2RT_ABI_VERSION == 1, "the shading planes are additive");
/* the prototypes, as the issue states them */
static int (*const p_frame_dev)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, const c2rt_shade_planes *, void *) = c2rt_render_shading_device;
static int (*const p_frame)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, const c2rt_shade_planes *) = c2rt_render_shading;
static int (*const p_rays_dev)(c2rt_ctx *, const c2rt_ray *, uint64_t, const c2rt_shade_planes *, void *) = c2rt_trace_rays_shading_device;
static int (*const p_rays)(c2rt_ctx *, const c2rt_ray *, uint64_t, const c2rt_shade_planes *) = c2rt_trace_rays_shading;
static int (*const p_host)(c2rt_ctx *, c2rt_host_scene *, const c2rt_shade_planes *) = c2rt_host_render_shading;
/* the members' types */
static int32_t *node_of(c2rt_shade_planes *p) { return p->node; }
static float *albedo_of(c2rt_shade_planes *p) { return p->albedo; }
static float *light_of(c2rt_shade_planes *p) { return p->light; }
static float *specular_of(c2rt_shade_planes *p) { return p->specular; }
static uint32_t *visible_of(c2rt_shade_planes *p) { return p->visible; }
static float *rgb_of(c2rt_shade_planes *p) { return p->rgb; }
int planes_size(void)
{
    c2rt_shade_planes pl = {0};
    return (int)sizeof pl + (node_of(&pl) || albedo_of(&pl) || light_of(&pl) || specular_of(&pl) || visible_of(&pl) || rgb_of(&pl));
}
void null_context(int *st)
{
    c2rt_ray ray = {{0, 0, 0}, {0, 0, 1}};
    int32_t node;
    c2rt_camera_frame cam = {{0}};
    c2rt_render_opts opts = {0};
    c2rt_shade_planes planes = {0};
    planes.node = &node;
    st[0] = p_frame_dev(NULL, &cam, &opts, &planes, NULL);
    st[1] = p_frame(NULL, &cam, &opts, &planes);
    st[2] = p_rays_dev(NULL, &ray, 1, &planes, NULL);
    st[3] = p_rays(NULL, &ray, 1, &planes);
    st[4] = p_host(NULL, NULL, &planes);
}
"""


def test_header_layout_and_null_context(tmp_path):
    src = tmp_path / "shading.c"
    src.write_text(C_PROGRAM)
    so = tmp_path / "libshading_probe.so"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)])
    _abi.load_library()                      # RTLD_GLOBAL: the probe's undefined symbols resolve to libc2rt.so's
    probe = C.CDLL(str(so))
    assert probe.planes_size() == 48 == C.sizeof(_abi.ShadePlanes)
    assert [f[0] for f in _abi.ShadePlanes._fields_] == ["node", "albedo", "light", "specular", "visible", "rgb"]
    st = (C.c_int * 5)(*([-1] * 5))
    probe.null_context(st)
    assert list(st) == [_abi.ERR_INVALID_ARG] * 5
    for name in ("c2rt_render_shading_device", "c2rt_render_shading", "c2rt_trace_rays_shading_device", "c2rt_trace_rays_shading"):
        assert name in _abi.C2RT_SYMBOLS
    assert "c2rt_host_render_shading" in _abi.C2RT_HOST_SYMBOLS
    from chess2rt_amd.api import SHADE_PLANES
    assert list(SHADE_PLANES) == [f[0] for f in _abi.ShadePlanes._fields_]
    assert sum(np.dtype(d).itemsize * c for d, c in SHADE_PLANES.values()) == 56


# ---- entitlement and preconditions, on the oracle alone ----------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def oracle_parts(variant, name):
    """(tables, rays, oracle records, oracle visibility, whole reference Shaded, Parts) — shared, read-only"""
    from test_shade_reference import oracle_case            # its cache: the whole colour is evaluated once per session

    T, rays, recs, vis, ref, _ = oracle_case(variant, name)
    return T, rays, recs, vis, ref, sp.parts(T, rays[:, 3:], recs, vis)


@pytest.mark.parametrize("name", ss.RAY_SETS)
@pytest.mark.parametrize("variant", ss.VARIANTS)
def test_the_reference_parts_recombine_to_the_reference_colour(variant, name):
    T, rays, recs, vis, ref, P = oracle_parts(variant, name)
    got = sp.recombine(P.albedo.rgb, P.light.rgb, P.specular.rgb, P.phong)
    differ = int((~sp.same_bits(got, ref.rgb)).sum())
    finite = all(np.isfinite(x.rgb).all() for x in (P.albedo, P.light, P.specular))
    print("%s %s: %d samples, %d floats of the recombination differ from the colour, parts finite: %s" % (variant, name, len(rays), differ, finite))
    assert differ == 0 and finite
    lambert = P.hit & ~P.phong
    assert not P.specular.rgb[lambert | ~P.hit].view(np.uint32).any()           # +0 bits on Lambert nodes and on misses
    for part in (P.albedo, P.light, P.specular):
        assert not part.rgb[~P.hit].view(np.uint32).any()
    # an ambiguous sample of the whole is ambiguous in a part, and the other way round: the parts see the same libm calls
    assert np.array_equal(P.albedo.ambiguous | P.specular.ambiguous, ref.ambiguous)


@pytest.mark.parametrize("variant", ss.VARIANTS)
def test_preconditions_of_the_gpu_tests(variant):
    counts = {"phong, specular != 0": 0, "phong, specular == 0": 0, "lambert": 0}
    lit_by_32_alone = 0
    for name in ss.RAY_SETS:
        T, rays, recs, vis, ref, P = oracle_parts(variant, name)
        spec = P.specular.rgb.view(np.uint32).any(axis=1)
        counts["phong, specular != 0"] += int((P.phong & spec).sum())
        counts["phong, specular == 0"] += int((P.phong & ~spec).sum())
        counts["lambert"] += int((P.hit & ~P.phong).sum())
        word = sp.pack_visible(T, vis)
        assert not word[~P.hit].any()
        # every set on its own shades Phong and Lambert nodes
        assert int(P.phong.sum()) >= MIN_REACH and int((P.hit & ~P.phong).sum()) >= MIN_REACH, (variant, name)
        if name == "random":
            print("%s random: %d misses" % (variant, int((~P.hit).sum())))
            assert int((~P.hit).sum()) >= MIN_REACH
        if variant in ("L2", "L4", "L5"):
            two = np.bincount(word[P.hit] & 3, minlength=4)
            print("%s %s: visible & 3 -> %s" % (variant, name, two.tolist()))
            assert (two >= MIN_REACH).all(), (variant, name, two.tolist())
        if variant == "L33":
            masks = len(np.unique(word[P.hit]))
            print("%s %s: %d distinct masks" % (variant, name, masks))
            assert masks >= 14, (name, masks)
            # lights 31 and 32 behave differently: one has a bit, the other none and still lights samples
            assert T.lit()[31] and T.lit()[32]
            assert int((P.hit & (vis[:, 31] != 0)).sum()) >= MIN_REACH and int((P.hit & (vis[:, 32] != 0) & (vis[:, 31] == 0)).sum()) >= MIN_REACH
            # no bit set, and light 32 alone raises `light` above the ambient term
            lit_by_32_alone += int((P.hit & (word == 0) & (vis[:, 32] != 0) & (P.light.rgb != T.ambient[None, :]).any(axis=1)).sum())
    print(variant, counts, "lit by light 32 alone:", lit_by_32_alone)
    assert variant != "L33" or lit_by_32_alone >= MIN_REACH
    for k, v in counts.items():
        assert v >= MIN_REACH, (variant, k, v)


@functools.lru_cache(maxsize=None)
def lecture5_case():
    """(scene, camera, options, screen rays, oracle records, oracle visibility (n, n_lights)) of lecture5.sdl at 61x47, AA off"""
    import chess2rt_amd as c2

    scene = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    scene.setFrameSize(ss.W, ss.H)
    scene.setAA(False)
    scene.setDof(False)
    cam, opts = scene.beginFrame(), scene.renderOpts(taps=_abi.TAPS_1)
    rays = screen_rays(cam, ss.W, ss.H)
    recs = oracle_trace(scene.desc, rays)
    T = sr.Tables(scene.desc)
    vis = oracle_visibility(scene.desc, sr.shadow_segments(T, rays[:, 3:], recs)).reshape(len(rays), -1)
    vis[recs["closest_node"] < 0] = 0
    return scene, cam, opts, rays, recs, vis


def test_preconditions_of_the_frame_tests():
    scene, cam, opts, rays, recs, vis = lecture5_case()
    T = sr.Tables(scene.desc)
    hit = recs["closest_node"] >= 0
    shadowed = hit & (sp.pack_visible(T, vis) == 0)
    reach = np.bincount(recs["closest_node"][hit], minlength=T.n_nodes)
    print("lecture5 61x47: %d misses, %d shadowed hits, nodes reached %s" % (int((~hit).sum()), int(shadowed.sum()), reach.tolist()))
    assert T.n_nodes == 6 and T.n_lights == 1 and T.lit()[0]
    assert int((~hit).sum()) >= MIN_REACH and int(shadowed.sum()) >= MIN_REACH and (reach >= 14).all()
