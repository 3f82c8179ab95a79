"""Gather planes, CPU side: the ABI (a C program against the headers, the five entry points refusing a null context), the
Python layer's argument checks, the reduction of tests/gather_reference.py on hand-made inputs, and the precondition of
the GPU tests, asserted on the oracle alone.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gather_reference as gr
import occlusion_cases as oc
from chess2rt_amd import _abi, api
from ray_query_util import oracle_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_PROGRAM = r"""
#include <stddef.h>
#include <stdint.h>
#include "c2rt.h"
#include "c2rt_host.h"
_Static_assert(sizeof(c2rt_gather_opts) == 16, "c2rt_gather_opts");
_Static_assert(offsetof(c2rt_gather_opts, seed) == 0 && offsetof(c2rt_gather_opts, samples) == 8 &&
               offsetof(c2rt_gather_opts, reserved) == 12, "c2rt_gather_opts members");
_Static_assert(sizeof(c2rt_gather_planes) == 32, "c2rt_gather_planes");
_Static_assert(offsetof(c2rt_gather_planes, node) == 0 && offsetof(c2rt_gather_planes, hits) == 8 &&
               offsetof(c2rt_gather_planes, indirect) == 16 && offsetof(c2rt_gather_planes, bounce) == 24, "c2rt_gather_planes members");
_Static_assert(C2RT_MAX_GATHER_SAMPLES == 64, "one 64-bit mask");
_Static_assert(C2RT_ABI_VERSION == 1, "the gather planes are additive");
/* the prototypes, as the issue states them */
static int (*const p_frame_dev)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, const c2rt_gather_opts *,
                                const c2rt_gather_planes *, void *) = c2rt_render_gather_device;
static int (*const p_frame)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, const c2rt_gather_opts *,
                            const c2rt_gather_planes *) = c2rt_render_gather;
static int (*const p_rays_dev)(c2rt_ctx *, const c2rt_ray *, uint64_t, const c2rt_gather_opts *, const c2rt_gather_planes *,
                               void *) = c2rt_trace_rays_gather_device;
static int (*const p_rays)(c2rt_ctx *, const c2rt_ray *, uint64_t, const c2rt_gather_opts *, const c2rt_gather_planes *) = c2rt_trace_rays_gather;
static int (*const p_host)(c2rt_ctx *, c2rt_host_scene *, const c2rt_gather_opts *, const c2rt_gather_planes *) = c2rt_host_render_gather;
/* the members' types */
static uint64_t *seed_of(c2rt_gather_opts *o) { return &o->seed; }
static uint32_t *samples_of(c2rt_gather_opts *o) { return &o->samples; }
static uint32_t *reserved_of(c2rt_gather_opts *o) { return &o->reserved; }
static int32_t *node_of(c2rt_gather_planes *p) { return p->node; }
static uint64_t *hits_of(c2rt_gather_planes *p) { return p->hits; }
static float *indirect_of(c2rt_gather_planes *p) { return p->indirect; }
static float *bounce_of(c2rt_gather_planes *p) { return p->bounce; }
int opts_size(void)
{
    c2rt_gather_opts o = {0};
    return (int)sizeof o + (*seed_of(&o) || *samples_of(&o) || *reserved_of(&o));
}
int planes_size(void)
{
    c2rt_gather_planes pl = {0};
    return (int)sizeof pl + (node_of(&pl) || hits_of(&pl) || indirect_of(&pl) || bounce_of(&pl));
}
void null_context(int *st)
{
    c2rt_ray ray = {{0, 0, 0}, {0, 0, 1}};
    int32_t node;
    c2rt_camera_frame cam = {{0}};
    c2rt_render_opts opts = {0};
    c2rt_gather_opts g = {0, 1, 0};
    c2rt_gather_planes planes = {0};
    planes.node = &node;
    st[0] = p_frame_dev(NULL, &cam, &opts, &g, &planes, NULL);
    st[1] = p_frame(NULL, &cam, &opts, &g, &planes);
    st[2] = p_rays_dev(NULL, &ray, 1, &g, &planes, NULL);
    st[3] = p_rays(NULL, &ray, 1, &g, &planes);
    st[4] = p_host(NULL, NULL, &g, &planes);
}
"""


def test_header_layout_and_null_context(tmp_path):
    src = tmp_path / "gather.c"
    src.write_text(C_PROGRAM)
    so = tmp_path / "libgather_probe.so"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)])
    lib = _abi.load_library()                # RTLD_GLOBAL: the probe's undefined symbols resolve to libc2rt.so's
    probe = C.CDLL(str(so))
    assert probe.opts_size() == 16 == C.sizeof(_abi.GatherOpts)
    assert probe.planes_size() == 32 == C.sizeof(_abi.GatherPlanes)
    assert [(f[0], getattr(_abi.GatherOpts, f[0]).offset) for f in _abi.GatherOpts._fields_] == [("seed", 0), ("samples", 8), ("reserved", 12)]
    assert [f[0] for f in _abi.GatherPlanes._fields_] == ["node", "hits", "indirect", "bounce"]
    st = (C.c_int * 5)(*([-1] * 5))
    probe.null_context(st)
    assert list(st) == [_abi.ERR_INVALID_ARG] * 5
    for name in ("c2rt_render_gather_device", "c2rt_render_gather", "c2rt_trace_rays_gather_device", "c2rt_trace_rays_gather"):
        assert name in _abi.C2RT_SYMBOLS and hasattr(lib, name)
    assert "c2rt_host_render_gather" in _abi.C2RT_HOST_SYMBOLS and hasattr(lib, "c2rt_host_render_gather")
    assert list(api.GATHER_PLANES) == [f[0] for f in _abi.GatherPlanes._fields_]
    assert sum(np.dtype(d).itemsize * c for d, c in api.GATHER_PLANES.values()) == 36
    assert _abi.ABI_VERSION == 1


def test_python_layer_checks_its_arguments_before_the_library():
    """an unknown plane name and a wrong ray shape are refused by the Python layer: no context is touched"""
    with pytest.raises(ValueError):
        api._GATHER.new(("node", "depth"), (4,))
    with pytest.raises(ValueError):
        api._GATHER.device({"open": 1})
    pl, out = api._GATHER.new(("hits", "bounce"), (3, 5))
    assert list(out) == ["hits", "bounce"] and out["hits"].shape == (3, 5) and out["bounce"].shape == (3, 5, 3)
    assert out["hits"].dtype == np.uint64 and out["bounce"].dtype == np.float32
    assert pl.node is None and pl.indirect is None and pl.hits == out["hits"].ctypes.data and pl.bounce == out["bounce"].ctypes.data
    dev = api._GATHER.device({"node": 64, "indirect": 0})
    assert dev.node == 64 and dev.indirect is None and dev.hits is None and dev.bounce is None
    g = api._gather_opts(16, (1 << 40) + 5)
    assert (g.samples, g.seed, g.reserved) == (16, (1 << 40) + 5, 0)

    class NoContext:
        _lib = _h = None
    with pytest.raises(ValueError):
        api.Context.traceRaysGather(NoContext(), np.zeros((4, 5)), 16)


def test_reference_planes_of_hand_made_inputs():
    """the reduction: bits, the float32 product and sum in sample order, the division, the albedo, the miss and depth 0"""
    rec = np.zeros(3, dtype=api.RAY_HIT_DTYPE)
    rec["closest_node"] = [2, -1, 0]
    rec["normal"] = [[0, 1, 0], [0, 0, 0], [0, -1, 0]]
    rec["p"] = [[1, 0, 2], [0, 0, 0], [3, 0, 4]]
    dirs = np.array([[0, -1, 0], [0, 0, 1], [0, -1, 0.0]])
    K = 3
    hit, N, rays = gr.spawned(rec, dirs, np.arange(3), K, 1)
    assert hit.tolist() == [True, False, True] and not rays[1].any()
    assert np.array_equal(N, [[0, 1, 0], [0, 0, 0], [0, 1, 0]])            # faceforward turned the third normal to +y
    assert np.array_equal(rays[0, :, :3], np.broadcast_to([1, 1e-6, 2], (K, 3)))
    assert (rays[0, :, 4] >= 0).all() and (rays[2, :, 4] >= 0).all()
    w = gr.weights(rays[:, :, 3:], N)
    assert w.dtype == np.float32 and np.array_equal(w[0], (2.0 * rays[0, :, 4]).astype(np.float32))
    node = np.array([[1, -1, 4], [5, 5, 5], [-1, -1, -1]])
    rgb = np.zeros((3, K, 3), dtype=np.float32)
    rgb[0] = [[0.5, 0.25, 1.0], [0, 0, 0], [0.125, 2.0, 0.75]]
    rgb[1] = 9.0                                                        # a miss reads nothing
    albedo = np.array([[0.5, 0.25, 2.0], [1, 1, 1], [1, 1, 1]], dtype=np.float32)
    pl = gr.planes(rec, N, rays, node, rgb, albedo, K)
    assert pl["hits"].tolist() == [5, 0, 0] and pl["node"].tolist() == [2, -1, 0]
    f = np.float32
    want = ((f(0) + rgb[0, 0] * w[0, 0]) + rgb[0, 1] * w[0, 1]) + rgb[0, 2] * w[0, 2]
    assert pl["indirect"][0].tobytes() == (want / f(K)).astype(f).tobytes()
    assert pl["bounce"][0].tobytes() == (albedo[0] * pl["indirect"][0]).tobytes()
    assert not pl["indirect"][1:].view(np.uint32).any() and not pl["bounce"][1:].view(np.uint32).any()
    zero = gr.planes(rec, N, rays, node, rgb, albedo, K, depth0=True)
    assert zero["node"].tolist() == [2, -1, 0] and not zero["hits"].any()
    assert not zero["indirect"].view(np.uint32).any() and not zero["bounce"].view(np.uint32).any()


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_the_screen_rays_spawned_rays_see_floor_and_sky(name):
    """the inputs are worth testing: among the hits of the screen set, at least 100 `hits` masks are mixed (oracle only)"""
    scene, _, _ = oc.load(name)
    rays = oc.ray_set(name, "screen")
    recs = oracle_trace(scene.desc, rays)
    hit, N, sp = gr.spawned(recs, rays[:, 3:], np.arange(len(rays)), oc.K, oc.SEED)
    node = np.full((len(rays), oc.K), -1, dtype=np.int64)
    node[hit] = oracle_trace(scene.desc, sp[hit].reshape(-1, 6))["closest_node"].reshape(-1, oc.K)
    zeros = np.zeros((len(rays), oc.K, 3), dtype=np.float32)
    pl = gr.planes(recs, N, sp, node, zeros, np.zeros((len(rays), 3), dtype=np.float32), oc.K)
    mixed, full, empty = gr.mask_kinds(pl["hits"], hit, oc.K)
    print("%s screen %dx%d, K = %d, seed %d: %d hits, %d mixed, %d full, %d empty masks" % (name, oc.W, oc.H, oc.K, oc.SEED, int(hit.sum()), mixed, full, empty))
    assert mixed >= 100
    assert not (pl["hits"] >> np.uint64(oc.K)).any() and not pl["hits"][~hit].any()
