"""Hit layers, CPU side: the ABI (a C program against the header, the four entry points refusing a null context), the
entitlement of the GPU tests' yardstick — the definition (hit_layers_util.walk_layers) over the oracle's trace against
the same definition over the independent typed reference (tests/geom_reference.py) — and the preconditions of the GPU
tests, asserted on the oracle alone.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import geom_reference as gr
import geom_scenes as gs
from chess2rt_amd import _abi
from hit_layers_util import (EYELESS_RICH, FRAME_SCENES, LAYERS, check_layer_preconditions, eyeless_layers, frame_layers, walk_layers,
                             written)
from ray_query_util import oracle_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_PROGRAM = r"""
#include <stddef.h>
#include <stdint.h>
#include "c2rt.h"
#include "c2rt_host.h"
_Static_assert(C2RT_MAX_HIT_LAYERS == 16, "C2RT_MAX_HIT_LAYERS");
_Static_assert(C2RT_ABI_VERSION == 1, "the layers are additive");
/* the prototypes, as the issue states them */
static int (*const p_rays_dev)(c2rt_ctx *, const c2rt_ray *, uint64_t, uint32_t, c2rt_ray_hit *, float *, uint8_t *, void *) = c2rt_trace_rays_layers_device;
static int (*const p_rays)(c2rt_ctx *, const c2rt_ray *, uint64_t, uint32_t, c2rt_ray_hit *, float *, uint8_t *) = c2rt_trace_rays_layers;
static int (*const p_frame_dev)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, uint32_t, const c2rt_hit_planes *, uint8_t *, void *) = c2rt_render_hit_layers_device;
static int (*const p_frame)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, uint32_t, const c2rt_hit_planes *, uint8_t *) = c2rt_render_hit_layers;
static int (*const p_host)(c2rt_ctx *, c2rt_host_scene *, uint32_t, const c2rt_hit_planes *, uint8_t *) = c2rt_host_render_hit_layers;
int max_hit_layers(void) { return C2RT_MAX_HIT_LAYERS; }
void null_context(int *st)
{
    c2rt_ray ray = {{0, 0, 0}, {0, 0, 1}};
    c2rt_ray_hit hit;
    float rgb[3];
    uint8_t count;
    c2rt_camera_frame cam = {{0}};
    c2rt_render_opts opts = {0};
    c2rt_hit_planes planes = {0};
    st[0] = p_rays_dev(NULL, &ray, 1, 1, &hit, rgb, &count, NULL);
    st[1] = p_rays(NULL, &ray, 1, 1, &hit, rgb, &count);
    st[2] = p_frame_dev(NULL, &cam, &opts, 1, &planes, &count, NULL);
    st[3] = p_frame(NULL, &cam, &opts, 1, &planes, &count);
    st[4] = p_host(NULL, NULL, 1, &planes, &count);
}
"""


def test_header_constant_and_null_context(tmp_path):
    src = tmp_path / "layers.c"
    src.write_text(C_PROGRAM)
    so = tmp_path / "liblayers_probe.so"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)])
    _abi.load_library()                      # RTLD_GLOBAL: the probe's undefined symbols resolve to libc2rt.so's
    probe = C.CDLL(str(so))
    assert probe.max_hit_layers() == 16 == _abi.MAX_HIT_LAYERS
    st = (C.c_int * 5)(*([-1] * 5))
    probe.null_context(st)
    assert list(st) == [_abi.ERR_INVALID_ARG] * 5
    for name in ("c2rt_trace_rays_layers_device", "c2rt_trace_rays_layers", "c2rt_render_hit_layers_device", "c2rt_render_hit_layers"):
        assert name in _abi.C2RT_SYMBOLS
    assert "c2rt_host_render_hit_layers" in _abi.C2RT_HOST_SYMBOLS


def test_walk_layers_is_the_definition():
    """three surfaces at distances 1, 2, 3 along +z, by a trace that is a table: dist accumulates without the steps,
    the final miss is stored, nothing behind it, and K truncates"""
    from chess2rt_amd.api import RAY_HIT_DTYPE

    def trace(rays):
        out = np.zeros(len(rays), dtype=RAY_HIT_DTYPE)
        for i, r in enumerate(rays):
            nxt = np.floor(r[2]) + 1.0            # the surfaces are the planes z = 1, 2, 3
            if r[0] == 0.0 and nxt <= 3.0:
                out[i] = (int(nxt), int(nxt) + 10, nxt - r[2], 0.25, 0.5, (0.0, 0.0, nxt), (0.0, 0.0, -1.0))
            else:
                out[i] = (-1, -1, 1e99, 0.0, 0.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
        return out

    rays = np.array([[0, 0, 0, 0, 0, 1], [5, 0, 0, 0, 0, 1]], dtype=np.float64)
    recs, count = walk_layers(trace, rays, 6)
    assert list(count) == [3, 0]
    assert list(recs["closest_node"][:, 0]) == [1, 2, 3, -1, 0, 0] and list(recs["closest_node"][:, 1]) == [-1, 0, 0, 0, 0, 0]
    d1 = 1.0
    d2 = (2.0 - (1.0 + 1e-6)) + d1
    d3 = (3.0 - (2.0 + 1e-6)) + d2
    assert list(recs["dist"][:4, 0]) == [d1, d2, d3, 1e99] and d3 < 3.0       # short by the steps
    assert written(count, 6).sum(axis=0).tolist() == [4, 1]
    recs2, count2 = walk_layers(trace, rays, 2)
    assert list(count2) == [2, 0] and np.array_equal(recs2[:, 0], recs[:2, 0]) and written(count2, 2).sum(axis=0).tolist() == [2, 1]


@pytest.mark.parametrize("name", gs.RAY_SETS)
@pytest.mark.parametrize("variant", gs.VARIANTS)
def test_oracle_layers_equal_the_typed_references(variant, name):
    """K = 16: two of the 2 000 eyeless rays reach 8 layers"""
    K = 16
    scene = gs.load(variant)
    T = gr.Tables(scene.desc)
    rays = gs.ray_set(name)
    o_recs, o_count = walk_layers(lambda r: oracle_trace(scene.desc, r), rays, K)
    r_recs, r_count = walk_layers(lambda r: gr.trace(T, r)[0], rays, K)
    print("%s %s: count histogram %s" % (variant, name, np.bincount(o_count, minlength=K + 1).tolist()))
    assert np.array_equal(o_count, r_count)
    assert int(o_count.max()) < K and int((o_count >= 3).sum()) >= 100
    m = written(o_count, K)
    assert np.array_equal(o_recs["closest_node"][m], r_recs["closest_node"][m])
    assert np.array_equal(o_recs["leaf_geom"][m], r_recs["leaf_geom"][m])
    for f in ("dist", "p", "normal"):
        a, b = np.ascontiguousarray(o_recs[f][m]), np.ascontiguousarray(r_recs[f][m])
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f
    hit = o_recs["closest_node"][m] >= 0
    sphere = hit & (T.geom_type[np.where(hit, o_recs["leaf_geom"][m], 0)] == gr.GEOM_SPHERE)
    for f in ("u", "v"):
        a, b = np.ascontiguousarray(o_recs[f][m]), np.ascontiguousarray(r_recs[f][m])
        differ = a.view(np.uint64) != b.view(np.uint64)
        assert not (differ & ~sphere).any(), f                                  # plane and cube leaves: the oracle's bits
        with np.errstate(invalid="ignore"):
            assert bool(np.all((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= 1e-12))), f     # sphere leaves: 1e-12


@pytest.mark.parametrize("name", EYELESS_RICH)
def test_preconditions_of_the_gpu_tests_eyeless(name):
    _, _, _, count = eyeless_layers(name)
    deep, most = check_layer_preconditions(name, count)
    print("%s: %d rays with three or more layers, at most %d; histogram %s" % (name, deep, most, np.bincount(count, minlength=LAYERS + 1).tolist()))


@pytest.mark.parametrize("name", ("many_nodes_31", "many_nodes_41"))
def test_the_many_node_scenes_are_deep_and_truncate(name):
    """rows of spheres: some rays cross eight surfaces and more, so here max_layers = 8 cuts walks short — the contract
    and oracle tests see the cap at work on these two, and no truncation on the others"""
    _, _, _, count = eyeless_layers(name)
    assert int((count >= 3).sum()) >= 100 and int((count == LAYERS).sum()) >= 1, (name, np.bincount(count).tolist())


@pytest.mark.parametrize("scene_file", FRAME_SCENES)
def test_preconditions_of_the_gpu_tests_frames(scene_file):
    _, _, _, _, _, count = frame_layers(scene_file)
    deep, most = check_layer_preconditions(scene_file, count)
    print("%s: %d pixels with three or more layers, at most %d; histogram %s" % (scene_file, deep, most, np.bincount(count, minlength=LAYERS + 1).tolist()))
