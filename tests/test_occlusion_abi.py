"""Occlusion planes, CPU side: the ABI (a C program against the headers, the five entry points refusing a null context),
the entitlement of the GPU tests' yardstick — the libm-free direction generator of tests/occlusion_reference.py against
the reference's own formula (rt/shader.d:158-173) evaluated through numpy's libm — and the preconditions of the GPU
tests, asserted on the oracle alone.  No GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import occlusion_cases as oc
import occlusion_reference as ocr
from chess2rt_amd import _abi
from ray_query_util import oracle_trace, oracle_visibility

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_PROGRAM = r"""
#include <stddef.h>
#include <stdint.h>
#include "c2rt.h"
#include "c2rt_host.h"
_Static_assert(sizeof(c2rt_occlusion_opts) == 24, "c2rt_occlusion_opts");
_Static_assert(offsetof(c2rt_occlusion_opts, radius) == 0 && offsetof(c2rt_occlusion_opts, seed) == 8 &&
               offsetof(c2rt_occlusion_opts, samples) == 16 && offsetof(c2rt_occlusion_opts, reserved) == 20, "c2rt_occlusion_opts members");
_Static_assert(sizeof(c2rt_occlusion_planes) == 32, "c2rt_occlusion_planes");
_Static_assert(offsetof(c2rt_occlusion_planes, node) == 0 && offsetof(c2rt_occlusion_planes, open) == 8 &&
               offsetof(c2rt_occlusion_planes, ao) == 16 && offsetof(c2rt_occlusion_planes, bent) == 24, "c2rt_occlusion_planes members");
_Static_assert(C2RT_MAX_OCCLUSION_SAMPLES == 64, "one 64-bit mask");
_Static_assert(C2RT_ABI_VERSION == 1, "the occlusion planes are additive");
/* the prototypes, as the issue states them */
static int (*const p_frame_dev)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, const c2rt_occlusion_opts *,
                                const c2rt_occlusion_planes *, void *) = c2rt_render_occlusion_device;
static int (*const p_frame)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, const c2rt_occlusion_opts *,
                            const c2rt_occlusion_planes *) = c2rt_render_occlusion;
static int (*const p_rays_dev)(c2rt_ctx *, const c2rt_ray *, uint64_t, const c2rt_occlusion_opts *, const c2rt_occlusion_planes *,
                               void *) = c2rt_trace_rays_occlusion_device;
static int (*const p_rays)(c2rt_ctx *, const c2rt_ray *, uint64_t, const c2rt_occlusion_opts *, const c2rt_occlusion_planes *) = c2rt_trace_rays_occlusion;
static int (*const p_host)(c2rt_ctx *, c2rt_host_scene *, const c2rt_occlusion_opts *, const c2rt_occlusion_planes *) = c2rt_host_render_occlusion;
/* the members' types */
static double *radius_of(c2rt_occlusion_opts *o) { return &o->radius; }
static uint64_t *seed_of(c2rt_occlusion_opts *o) { return &o->seed; }
static uint32_t *samples_of(c2rt_occlusion_opts *o) { return &o->samples; }
static uint32_t *reserved_of(c2rt_occlusion_opts *o) { return &o->reserved; }
static int32_t *node_of(c2rt_occlusion_planes *p) { return p->node; }
static uint64_t *open_of(c2rt_occlusion_planes *p) { return p->open; }
static float *ao_of(c2rt_occlusion_planes *p) { return p->ao; }
static double *bent_of(c2rt_occlusion_planes *p) { return p->bent; }
int opts_size(void)
{
    c2rt_occlusion_opts o = {0};
    return (int)sizeof o + (*radius_of(&o) != 0 || *seed_of(&o) || *samples_of(&o) || *reserved_of(&o));
}
int planes_size(void)
{
    c2rt_occlusion_planes pl = {0};
    return (int)sizeof pl + (node_of(&pl) || open_of(&pl) || ao_of(&pl) || bent_of(&pl));
}
void null_context(int *st)
{
    c2rt_ray ray = {{0, 0, 0}, {0, 0, 1}};
    int32_t node;
    c2rt_camera_frame cam = {{0}};
    c2rt_render_opts opts = {0};
    c2rt_occlusion_opts occ = {1.0, 0, 1, 0};
    c2rt_occlusion_planes planes = {0};
    planes.node = &node;
    st[0] = p_frame_dev(NULL, &cam, &opts, &occ, &planes, NULL);
    st[1] = p_frame(NULL, &cam, &opts, &occ, &planes);
    st[2] = p_rays_dev(NULL, &ray, 1, &occ, &planes, NULL);
    st[3] = p_rays(NULL, &ray, 1, &occ, &planes);
    st[4] = p_host(NULL, NULL, &occ, &planes);
}
"""


def test_header_layout_and_null_context(tmp_path):
    src = tmp_path / "occlusion.c"
    src.write_text(C_PROGRAM)
    so = tmp_path / "libocclusion_probe.so"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)])
    lib = _abi.load_library()                # RTLD_GLOBAL: the probe's undefined symbols resolve to libc2rt.so's
    probe = C.CDLL(str(so))
    assert probe.opts_size() == 24 == C.sizeof(_abi.OcclusionOpts)
    assert probe.planes_size() == 32 == C.sizeof(_abi.OcclusionPlanes)
    assert [(f[0], getattr(_abi.OcclusionOpts, f[0]).offset) for f in _abi.OcclusionOpts._fields_] == [("radius", 0), ("seed", 8), ("samples", 16), ("reserved", 20)]
    assert [f[0] for f in _abi.OcclusionPlanes._fields_] == ["node", "open", "ao", "bent"]
    st = (C.c_int * 5)(*([-1] * 5))
    probe.null_context(st)
    assert list(st) == [_abi.ERR_INVALID_ARG] * 5
    for name in ("c2rt_render_occlusion_device", "c2rt_render_occlusion", "c2rt_trace_rays_occlusion_device", "c2rt_trace_rays_occlusion"):
        assert name in _abi.C2RT_SYMBOLS and hasattr(lib, name)
    assert "c2rt_host_render_occlusion" in _abi.C2RT_HOST_SYMBOLS and hasattr(lib, "c2rt_host_render_occlusion")
    from chess2rt_amd.api import OCCLUSION_PLANES
    assert list(OCCLUSION_PLANES) == [f[0] for f in _abi.OcclusionPlanes._fields_]
    assert sum(np.dtype(d).itemsize * c for d, c in OCCLUSION_PLANES.values()) == 40


# ---- the direction generator against the reference's formula -----------------------------------------------------------


def test_directions_against_the_reference_formula_through_libm():
    """200 000 draws of the generator's own (u, v): each component within 1e-14 of cos(theta) cos(phi), sin(phi),
    sin(theta) cos(phi) with theta = 2 pi u, phi = acos(2 v - 1) - pi / 2 (rt/shader.d:158-173), unit length within
    1e-15, and dot(res, N) >= 0 after the flip for random normals."""
    n, K = 12500, 16
    u, v = ocr.uniforms(oc.SEED, np.arange(n), K)
    assert u.shape == v.shape == (n, K) and (u >= 0).all() and (u < 1).all() and (v >= 0).all() and (v < 1).all()
    got = ocr.unflipped(u, v)
    theta = 2 * np.pi * u
    phi = np.arccos(2 * v - 1) - np.pi / 2
    want = np.stack([np.cos(theta) * np.cos(phi), np.sin(phi), np.sin(theta) * np.cos(phi)], axis=-1)
    err = float(np.abs(got - want).max())
    length = float(np.abs(np.sqrt((got * got).sum(axis=-1)) - 1.0).max())
    print("%d draws: max component error %.3g, max |length - 1| %.3g" % (n * K, err, length))
    assert err <= 1e-14
    assert length <= 1e-15
    rng = np.random.RandomState(5)
    N = rng.normal(size=(n, 1, 3))
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    res, flip = ocr.flipped(got, N)
    assert (ocr.dot3(res, N) >= 0).all()
    assert 0.4 < flip.mean() < 0.6                                       # a hemisphere: half of the sphere's draws turn round
    assert np.array_equal(res[flip], -got[flip]) and np.array_equal(res[~flip], got[~flip])
    # the two draws of a sample are independent of the other samples' and of K
    u4, v4 = ocr.uniforms(oc.SEED, np.arange(n), 4)
    assert np.array_equal(u4, u[:, :4]) and np.array_equal(v4, v[:, :4])
    assert not np.array_equal(ocr.uniforms(oc.SEED + 1, np.arange(n), 4)[0], u4)


def test_reference_planes_of_hand_made_answers():
    """the reduction: bits, popcount / K in float32, the sum in sample order, and the miss"""
    from chess2rt_amd.api import RAY_HIT_DTYPE
    rec = np.zeros(3, dtype=RAY_HIT_DTYPE)
    rec["closest_node"] = [2, -1, 0]
    rec["normal"] = [[0, 1, 0], [0, 0, 0], [0, -1, 0]]
    dirs = np.array([[0, -1, 0], [0, 0, 1], [0, -1, 0.0]])
    hit, res, seg, flip = ocr.samples(rec, dirs, np.arange(3), 3, 2.0, 1)
    assert hit.tolist() == [True, False, True] and not res[1].any() and not seg[1].any()
    assert (res[0, :, 1] >= 0).all() and (res[2, :, 1] >= 0).all()      # faceforward turned the third normal to +y
    assert np.array_equal(seg[0, :, :3], np.broadcast_to([0, 1e-6, 0], (3, 3)))
    assert np.array_equal(seg[0, :, 3:], seg[0, :, :3] + res[0] * 2.0)
    pl = ocr.planes(rec, res, np.array([[1, 0, 1], [1, 1, 1], [0, 0, 0]]), 3)
    assert pl["open"].tolist() == [5, 7, 0] and pl["node"].tolist() == [2, -1, 0]
    assert pl["ao"].tobytes() == (np.array([2, 3, 0], dtype=np.float32) / np.float32(3)).tobytes()
    assert np.array_equal(pl["bent"][0], (np.zeros(3) + res[0, 0]) + res[0, 2]) and not pl["bent"][1:].view(np.uint64).any()


# ---- the preconditions of the GPU tests, on the oracle alone -------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def oracle_case(name, which):
    """(rays, oracle records, hit, directions, flips, oracle visibility (n, K), reference planes) — shared, read-only"""
    scene, _, _ = oc.load(name)
    rays = oc.ray_set(name, which)
    recs = oracle_trace(scene.desc, rays)
    hit, res, seg, flip = ocr.samples(recs, rays[:, 3:], np.arange(len(rays)), oc.K, oc.RADIUS[name], oc.SEED)
    vis = np.zeros((len(rays), oc.K), dtype=np.uint8)
    vis[hit] = oracle_visibility(scene.desc, seg[hit].reshape(-1, 6)).reshape(-1, oc.K)
    return rays, recs, hit, res, flip, vis, ocr.planes(recs, res, vis, oc.K)


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_preconditions_of_the_screen_ray_tests(name):
    scene, _, _ = oc.load(name)
    rays, recs, hit, res, flip, vis, pl = oracle_case(name, "screen")
    mixed, full, empty = ocr.mask_kinds(pl["open"], hit, oc.K)
    reach = np.bincount(recs["closest_node"][hit], minlength=scene.desc.contents.n_nodes)
    print("%s screen %dx%d, K = %d, radius %g: %d hits, %d mixed, %d full, %d empty masks, nodes reached %s, %d of %d draws flipped"
          % (name, oc.W, oc.H, oc.K, oc.RADIUS[name], int(hit.sum()), mixed, full, empty, reach.tolist(), int(flip[hit].sum()), int(hit.sum()) * oc.K))
    assert len(rays) == oc.W * oc.H
    assert mixed >= 200 and full >= 200
    assert (reach > 0).all()                                             # hits on every node
    assert flip[hit].any() and not flip[hit].all()                       # both outcomes of the flip
    v = vis[hit] != 0
    assert v.any(axis=0).all() and (~v).any(axis=0).all()                # every sample index open somewhere, closed somewhere
    # ao and bent follow the masks
    assert np.array_equal(pl["ao"], np.array([bin(int(x)).count("1") for x in pl["open"]], dtype=np.float32) / np.float32(oc.K))


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_preconditions_of_the_eyeless_tests(name):
    rays, recs, hit, res, flip, vis, pl = oracle_case(name, "eyeless")
    mixed, full, empty = ocr.mask_kinds(pl["open"], hit, oc.K)
    print("%s eyeless n = %d: %d hits, %d mixed, %d full, %d empty masks" % (name, len(rays), int(hit.sum()), mixed, full, empty))
    assert len(rays) == oc.N_EYELESS and len(rays) % 64 != 0             # the last wave is partial
    assert empty >= 1                                                    # origins inside solids
    assert mixed >= 100
    assert (~hit).any() and (pl["open"][~hit] == np.uint64((1 << oc.K) - 1)).all()
