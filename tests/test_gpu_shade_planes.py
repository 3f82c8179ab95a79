"""Shading planes on the GPU (c2rt_render_shading*, c2rt_trace_rays_shading*): rgb and node against the hit calls, the
recombination identity on the GPU's own planes, `visible` against the context's own visibility queries and the oracle's,
and albedo / light / specular against the parts of the independent typed reference (tests/shade_parts_reference.py over
tests/shade_reference.py) fed with the GPU's own records and visibility, as tests/test_gpu_shade.py feeds the whole
colour.  Bits everywhere; an ambiguous sample (a pow / sin value within 4 fp64 ulp of a float32 rounding midpoint) must
lie within the bounds of its re-evaluations.  No tolerance anywhere."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

import chess2rt_amd as c2
import query_test_util as Q
import shade_parts_reference as sp
import shade_reference as sr
import shade_scenes as ss
from chess2rt_amd import _abi
from chess2rt_amd.api import SHADE_PLANES
from golden_configs import SCENES
from query_test_util import SHADING, check_device_against_host, check_filled, device_planes, guarded, last_error, lib, raw_call, struct_of, untouched
from ray_query_util import bits, oracle_visibility, screen_rays

pytestmark = pytest.mark.gpu

W, H = ss.W, ss.H
PLANES = tuple(SHADE_PLANES)
FLOATS = ("albedo", "light", "specular", "rgb")
MIN_REACH = 30
_gpu_cases = {}


same_planes = functools.partial(Q.same_planes, names=PLANES)


def phong_of(T, node):
    node = np.asarray(node).reshape(-1)
    hit = node >= 0
    phong = np.zeros(len(node), dtype=bool)
    phong[hit] = T.shader_type[T.node_shader[node[hit]]] == sr.SHADER_PHONG
    return hit, phong


def check_identity(T, pl, what):
    """test 2: on the planes' own values, in numpy float32, no exclusion, NaN equal to NaN"""
    hit, phong = phong_of(T, pl["node"])
    rgb = pl["rgb"].reshape(-1, 3)
    want = sp.recombine(pl["albedo"], pl["light"], pl["specular"], phong)
    bad = ~sp.same_bits(rgb, want)[hit]
    assert not bad.any(), "%s: rgb != albedo * light (+ specular) on %d floats" % (what, int(bad.sum()))
    spec = pl["specular"].reshape(-1, 3)
    assert not spec[~phong].view(np.uint32).any(), "%s: specular is not +0 on a Lambert node or a miss" % what
    miss = ~hit
    assert (pl["node"].reshape(-1)[miss] == -1).all() and not pl["visible"].reshape(-1)[miss].any(), what
    for name in FLOATS:
        assert not pl[name].reshape(-1, 3)[miss].view(np.uint32).any(), "%s: %s of a miss is not +0" % (what, name)
    return hit, phong


def gpu_case(gpu_ctx, variant):
    """uploads the variant and returns {ray set: (rays, GPU records, GPU rgb, shading planes, GPU visibility (n, n_lights),
    segments asked, their answers)} — the queries run once per variant and are shared by the tests below (read-only)"""
    scene, _, _ = ss.load(variant)
    gpu_ctx.uploadScene(scene.desc)
    if variant not in _gpu_cases:
        T = sr.Tables(scene.desc)
        lit = T.lit()
        out = {}
        for name in ss.RAY_SETS:
            rays = ss.ray_set(variant, name)
            rec, rgb = gpu_ctx.traceRays(rays)
            pl = gpu_ctx.traceRaysShading(rays)
            segs = sr.shadow_segments(T, rays[:, 3:], rec).reshape(len(rays), T.n_lights, 6)
            hit = rec["closest_node"] >= 0
            ask = np.ascontiguousarray(segs[hit][:, lit].reshape(-1, 6))        # every lit light of every hit
            vis = np.zeros((len(rays), T.n_lights), dtype=np.uint8)
            got = gpu_ctx.testVisibility(ask)
            sub = np.zeros((int(hit.sum()), T.n_lights), dtype=np.uint8)
            sub[:, lit] = got.reshape(-1, int(lit.sum()))
            vis[hit] = sub
            out[name] = (rays, rec, rgb, pl, vis, ask, got)
        _gpu_cases[variant] = out
    return _gpu_cases[variant]


@functools.lru_cache(maxsize=None)
def reference_parts(variant, name):
    """the reference's parts of the GPU's own records and visibility — evaluated once, after gpu_case has run"""
    scene, _, _ = ss.load(variant)
    rays, rec, _, _, vis, _, _ = _gpu_cases[variant][name]
    return sp.parts(sr.Tables(scene.desc), rays[:, 3:], rec, vis)


# ---- 1, 2: rgb and node are the hit calls'; the identity ---------------------------------------------------------------


@pytest.mark.parametrize("variant", ss.VARIANTS)
def test_rgb_and_node_are_the_hit_calls_and_the_parts_recombine(gpu_ctx, variant):
    scene, cam, opts = ss.load(variant)
    T = sr.Tables(scene.desc)
    for name, (rays, rec, rgb, pl, vis, _, _) in gpu_case(gpu_ctx, variant).items():
        what = "%s %s" % (variant, name)
        assert set(pl) == set(PLANES)
        for p in PLANES:
            assert pl[p].dtype == SHADE_PLANES[p][0] and pl[p].shape == ((len(rays),) if SHADE_PLANES[p][1] == 1 else (len(rays), 3)), (what, p)
        assert bits(pl["rgb"]).tobytes() == bits(rgb).tobytes(), "%s: rgb differs from traceRays" % what
        assert np.array_equal(pl["node"], rec["closest_node"]), "%s: node differs from traceRays" % what
        hit, phong = check_identity(T, pl, what)
        assert hit.sum() >= MIN_REACH and phong.sum() >= MIN_REACH and (hit & ~phong).sum() >= MIN_REACH, what
    frame = gpu_ctx.renderShading(cam, opts)
    hits = gpu_ctx.renderHits(cam, opts, planes=("node", "rgb"))
    same_planes(frame, hits, "%s frame against renderHits" % variant, names=("node", "rgb"))
    check_identity(T, frame, "%s frame" % variant)
    # the frame's planes are the planes of its own screen rays
    screen = gpu_case(gpu_ctx, variant)["screen"][3]
    for p in PLANES:
        assert bits(frame[p]).tobytes() == bits(screen[p]).tobytes(), "%s: frame plane %s differs from its screen rays'" % (variant, p)


# ---- 3: visible ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("variant", ss.VARIANTS)
def test_visible_is_the_contexts_and_the_oracles_visibility(gpu_ctx, variant):
    scene, _, _ = ss.load(variant)
    T = sr.Tables(scene.desc)
    lit = T.lit()
    lit_by_32_alone = with_bit_31 = 0
    for name, (rays, rec, rgb, pl, vis, ask, got) in gpu_case(gpu_ctx, variant).items():
        what = "%s %s" % (variant, name)
        assert np.array_equal(pl["visible"], sp.pack_visible(T, vis)), "%s: visible differs from testVisibility's answers" % what
        want = oracle_visibility(scene.desc, ask)
        assert np.array_equal(got, want), "%s: visibility differs from the oracle" % what
        hit = rec["closest_node"] >= 0
        ovis = np.zeros_like(vis)
        sub = np.zeros((int(hit.sum()), T.n_lights), dtype=np.uint8)
        sub[:, lit] = want.reshape(-1, int(lit.sum()))
        ovis[hit] = sub
        assert np.array_equal(pl["visible"], sp.pack_visible(T, ovis)), "%s: visible differs from the oracle's answers" % what
        for l in np.nonzero(~lit[:32])[0]:
            assert not (pl["visible"] & np.uint32(1 << int(l))).any(), "%s: dark light %d has a bit" % (what, l)
        if T.n_lights > 32:
            with_bit_31 += int(((pl["visible"] >> np.uint32(31)) & 1).sum())
            # light 32 has no bit and still lights the sample: nothing below 32 is visible, light 32 is, cosTheta > 0
            alone = hit & (pl["visible"] == 0) & (vis[:, 32] != 0)
            above_ambient = (pl["light"].reshape(-1, 3) != T.ambient[None, :]).any(axis=1)
            lit_by_32_alone += int((alone & above_ambient).sum())
            assert not (hit & (pl["visible"] == 0) & (vis[:, 32] == 0) & above_ambient).any(), what
    if variant in ("L4", "L5"):
        assert not lit[2]
    if T.n_lights > 32:
        print("L33: %d samples with bit 31, %d lit by light 32 alone" % (with_bit_31, lit_by_32_alone))
        assert with_bit_31 >= MIN_REACH and lit_by_32_alone >= MIN_REACH


# ---- 4: the parts against the reference's ------------------------------------------------------------------------------


@pytest.mark.parametrize("variant", ss.VARIANTS)
def test_parts_equal_the_reference_of_the_gpus_own_records(gpu_ctx, variant):
    for name, (rays, rec, rgb, pl, vis, _, _) in gpu_case(gpu_ctx, variant).items():
        P = reference_parts(variant, name)
        what = "%s %s" % (variant, name)
        assert not P.light.ambiguous.any()
        for part, ref in (("light", P.light), ("specular", P.specular), ("albedo", P.albedo)):
            plain, outside = sr.compare(pl[part], ref)
            print("%s %s: %d samples, %d ambiguous, %d floats differ outside them, %d outside their bounds"
                  % (what, part, len(rays), int(ref.ambiguous.sum()), plain, outside))
            assert plain == 0 and outside == 0, (what, part, plain, outside)


# ---- 5: plane subsets --------------------------------------------------------------------------------------------------


SUBSETS = [(p,) for p in PLANES] + list(itertools.combinations(PLANES, 2))


@pytest.mark.parametrize("variant", ["L1", "L5"])
def test_plane_subsets(gpu_ctx, variant):
    """L1: the one-light instance; L5: the light loop"""
    scene, cam, opts = ss.load(variant)
    case = gpu_case(gpu_ctx, variant)
    rays, full_rays = case["random"][0], case["random"][3]
    full = gpu_ctx.renderShading(cam, opts)
    Q.check_plane_subsets(SHADING, gpu_ctx, cam, opts, rays, None, SUBSETS, full, full_rays, W * H, variant)
    got = gpu_ctx.renderShading(cam, opts, planes=("visible", "albedo"))
    assert set(got) == {"visible", "albedo"}
    same_planes(got, full, variant, names=("visible", "albedo"))
    with pytest.raises(ValueError):
        gpu_ctx.renderShading(cam, opts, planes=("depth",))


# ---- 6: strips -------------------------------------------------------------------------------------------------------


def test_strips(gpu_ctx):
    scene, cam, opts = ss.load("L5")
    gpu_ctx.uploadScene(scene.desc)
    full = gpu_ctx.renderShading(cam, opts)
    Q.check_strips(gpu_ctx, scene, lambda o: gpu_ctx.renderShading(cam, o), full, H, 3, 8, PLANES, "L5")


# ---- 7: host chunking ------------------------------------------------------------------------------------------------


def lecture5(width, height, pitch_up=0.0):
    scene = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    scene.setFrameSize(width, height)
    scene.setAA(False)
    scene.setDof(False)
    hc = scene.camera
    hc.pitch += pitch_up
    scene.camera = hc
    return scene, scene.beginFrame(), scene.renderOpts(taps=_abi.TAPS_1)


def test_host_chunks_of_a_frame_equal_the_device_call(gpu_ctx):
    import torch

    w, h = 640, 480                          # 307 200 pixels: two chunks of whole rows
    scene, cam, opts = lecture5(w, h)
    gpu_ctx.uploadScene(scene.desc)
    host = gpu_ctx.renderShading(cam, opts)
    dev = torch.device("cuda:0")
    s1 = torch.cuda.Stream(dev)
    t = device_planes(SHADE_PLANES, w * h, dev, guard_bytes=64)
    torch.cuda.synchronize()
    gpu_ctx.renderShadingDevice(cam, opts, {k: v.data_ptr() for k, v in t.items()}, s1.cuda_stream)
    s1.synchronize()
    check_device_against_host(SHADE_PLANES, t, host, w * h, "640x480")
    assert 0 < int((host["node"] >= 0).sum()) < w * h


def test_host_chunks_of_rays_equal_the_device_call(gpu_ctx):
    import torch

    base = gpu_case(gpu_ctx, "L5")["random"]
    n = (1 << 18) + 5
    rays = np.ascontiguousarray(np.tile(base[0], (n // len(base[0]) + 1, 1))[:n])
    host = gpu_ctx.traceRaysShading(rays)
    reps = np.arange(n) % len(base[0])
    for name in PLANES:
        assert bits(host[name]).tobytes() == bits(base[3][name][reps]).tobytes(), name
    dev = torch.device("cuda:0")
    s1 = torch.cuda.Stream(dev)
    t = device_planes(SHADE_PLANES, n, dev, guard_bytes=64)
    rays_t = torch.from_numpy(rays).to(dev)
    torch.cuda.synchronize()
    gpu_ctx.traceRaysShadingDevice(rays_t.data_ptr(), n, {k: v.data_ptr() for k, v in t.items()}, s1.cuda_stream)
    s1.synchronize()
    check_device_against_host(SHADE_PLANES, t, host, n, "2^18 + 5 rays")


# ---- 8: rays of garbage ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("variant", ["L1", "L33"])
def test_garbage_rays_terminate_and_change_no_other_ray(gpu_ctx, variant):
    rays0, _, _, want, _, _, _ = gpu_case(gpu_ctx, variant)["random"]
    rays = rays0.copy()
    where = {3: np.nan, 64 + 17: 0.0, 1400: 1e300}       # in three different waves
    for i, v in where.items():
        rays[i] = v
    got = gpu_ctx.traceRaysShading(rays)
    keep = np.ones(len(rays), dtype=bool)
    keep[list(where)] = False
    for name in PLANES:
        assert bits(got[name][keep]).tobytes() == bits(want[name][keep]).tobytes(), (variant, name)


# ---- 9: statuses, before anything is touched -----------------------------------------------------------------------------


def test_frame_statuses_leave_the_outputs_untouched(gpu_ctx):
    scene, cam, opts = ss.load("L2")
    gpu_ctx.uploadScene(scene.desc)
    n = W * H

    def copy_cam(**kw):
        return Q.with_fields(cam, **kw)

    def copy_opts(**kw):
        return Q.with_fields(opts, **kw)

    bufs = guarded(SHADE_PLANES, PLANES, n)
    L = lib()
    pl = struct_of(_abi.ShadePlanes, bufs)
    assert L.c2rt_render_shading(gpu_ctx.handle, None, C.byref(opts), C.byref(pl)) == _abi.ERR_INVALID_ARG          # a frame call's own
    assert L.c2rt_render_shading(gpu_ctx.handle, C.byref(cam), C.byref(copy_opts(width=0)), C.byref(pl)) == L.c2rt_render_hits(
        gpu_ctx.handle, C.byref(cam), C.byref(copy_opts(width=0)), C.byref(_abi.HitPlanes(node=bufs["node"].ctypes.data)))
    assert raw_call(SHADING, gpu_ctx, bufs, cam, opts, null_struct=True) == _abi.ERR_INVALID_ARG
    assert last_error(gpu_ctx) == "null planes"
    assert raw_call(SHADING, gpu_ctx, {}, cam, opts) == _abi.ERR_INVALID_ARG
    assert last_error(gpu_ctx) == "no plane asked for: all six pointers of c2rt_shade_planes are null"
    # the planes are judged before the modes: a depth-of-field camera with no plane is an invalid argument
    assert raw_call(SHADING, gpu_ctx, {}, copy_cam(dof=1, num_samples=4), opts) == _abi.ERR_INVALID_ARG
    cases = [(copy_cam(dof=1, num_samples=4), opts, "depth of field: a pixel's terms are one ray's, a lens has many per pixel"),
             (copy_cam(stereo_separation=0.5), opts, "stereo: a pixel's terms are one ray's, a stereo camera has two per pixel"),
             (cam, copy_opts(count_rays=1), "count_rays: the shading planes do not count rays"),
             (cam, copy_opts(prepass_bucket=48), "prepass_bucket: a preview's pixels share the sample of their block")]
    for c, o, cause in cases:
        assert raw_call(SHADING, gpu_ctx, bufs, c, o) == _abi.ERR_UNSUPPORTED, cause
        assert last_error(gpu_ctx) == cause, (cause, last_error(gpu_ctx))
        # the device variant decides the same before it enqueues anything (the pointers are never used)
        assert L.c2rt_render_shading_device(gpu_ctx.handle, C.byref(c), C.byref(o), C.byref(pl), None) == _abi.ERR_UNSUPPORTED, cause
        assert last_error(gpu_ctx) == cause
    fresh = c2.Context(0)
    try:
        assert raw_call(SHADING, fresh, bufs, cam, opts) == _abi.ERR_NO_SCENE
        assert "no scene" in last_error(fresh)
        assert raw_call(SHADING, fresh, {}, cam, opts) == _abi.ERR_NO_SCENE                  # the frame checks come first
    finally:
        fresh.close()
    assert untouched(bufs)
    # afterwards the same context renders a correct plane set
    want = gpu_ctx.renderShading(cam, opts)
    assert raw_call(SHADING, gpu_ctx, bufs, cam, opts) == _abi.OK
    check_filled(SHADE_PLANES, bufs, want, n, "after the refusals")


def test_ray_statuses_leave_the_outputs_untouched(gpu_ctx):
    rays, _, _, want, _, _, _ = gpu_case(gpu_ctx, "L2")["random"]
    n = len(rays)
    bufs = guarded(SHADE_PLANES, PLANES, n)
    L = lib()
    pl = struct_of(_abi.ShadePlanes, bufs)
    rp = rays.ctypes.data_as(C.c_void_p)
    for fn, tail in ((L.c2rt_trace_rays_shading, ()), (L.c2rt_trace_rays_shading_device, (None,))):
        assert fn(None, rp, n, C.byref(pl), *tail) == _abi.ERR_INVALID_ARG                        # null context
        assert fn(gpu_ctx.handle, None, 0, None, *tail) == _abi.OK                                # n == 0, whatever else
        assert fn(gpu_ctx.handle, None, n, None, *tail) == _abi.ERR_INVALID_ARG                   # null rays before null planes
        assert "null input array" in last_error(gpu_ctx)
        assert fn(gpu_ctx.handle, rp, _abi.MAX_RAYS + 1, None, *tail) == _abi.ERR_LIMIT           # the limit before the planes
        assert "rays in one call" in last_error(gpu_ctx)
        assert fn(gpu_ctx.handle, rp, n, None, *tail) == _abi.ERR_INVALID_ARG
        assert last_error(gpu_ctx) == "null planes"
        empty = _abi.ShadePlanes()
        assert fn(gpu_ctx.handle, rp, n, C.byref(empty), *tail) == _abi.ERR_INVALID_ARG
        assert last_error(gpu_ctx) == "no plane asked for: all six pointers of c2rt_shade_planes are null"
    fresh = c2.Context(0)
    try:
        assert raw_call(SHADING, fresh, bufs, rays=rays, n=n) == _abi.ERR_NO_SCENE
        assert "no scene" in last_error(fresh)
        assert raw_call(SHADING, fresh, bufs, rays=rays, n=n, null_struct=True) == _abi.ERR_NO_SCENE   # no scene before the planes
        assert raw_call(SHADING, fresh, bufs, rays=rays, n=_abi.MAX_RAYS + 1) == _abi.ERR_LIMIT        # the limit before the scene
        assert raw_call(SHADING, fresh, {}, n=0, null_struct=True) == _abi.OK
    finally:
        fresh.close()
    assert untouched(bufs)
    assert raw_call(SHADING, gpu_ctx, bufs, rays=rays, n=n) == _abi.OK
    check_filled(SHADE_PLANES, bufs, want, n, "after the refusals")


# ---- 10: host mirror ---------------------------------------------------------------------------------------------------


def test_renderer_equals_context_for_the_scenes_camera(gpu_ctx):
    scene, cam, opts = lecture5(32, 24)
    gpu_ctx.uploadScene(scene.desc)
    want = gpu_ctx.renderShading(cam, opts)
    assert 0 < int((want["node"] >= 0).sum()) < 32 * 24
    got = c2.Renderer(scene, gpu_ctx).renderShading()
    assert set(got) == set(PLANES)
    for name in PLANES:
        assert got[name].shape == want[name].shape == ((24, 32) if SHADE_PLANES[name][1] == 1 else (24, 32, 3)) and got[name].dtype == want[name].dtype, name
    same_planes(got, want, "Renderer.renderShading")
    sub = c2.Renderer(scene, gpu_ctx).renderShading(planes=("light",))
    assert list(sub) == ["light"] and bits(sub["light"]).tobytes() == bits(want["light"]).tobytes()
    dof = c2.parseSceneFromFile(os.path.join(SCENES, "zaphod.sdl"))      # as shipped: depth of field
    dof.setFrameSize(32, 24)
    assert dof.camera.dof
    with pytest.raises(c2.C2rtError) as e:
        c2.Renderer(dof, gpu_ctx).renderShading()
    assert e.value.status == _abi.ERR_UNSUPPORTED and "depth of field" in str(e.value)


# ---- 11: CSG depths ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("scene_file", ["lecture5.sdl", "csg_stress.sdl"])
def test_csg_scenes_hit_calls_and_identity(gpu_ctx, scene_file):
    """lecture5: a CsgOp of leaves (the depth-1 instance); csg_stress: nested CsgOps (a nested instance, LDS-bound)"""
    scene = c2.parseSceneFromFile(os.path.join(SCENES, scene_file))
    scene.setFrameSize(W, H)
    scene.setAA(False)
    scene.setDof(False)
    hc = scene.camera
    hc.pitch += 5.0          # some rays leave the scene
    scene.camera = hc
    cam, opts = scene.beginFrame(), scene.renderOpts(taps=_abi.TAPS_1)
    gpu_ctx.uploadScene(scene.desc)
    T = sr.Tables(scene.desc)
    pl = gpu_ctx.renderShading(cam, opts)
    hits = gpu_ctx.renderHits(cam, opts, planes=("node", "rgb"))
    same_planes(pl, hits, scene_file, names=("node", "rgb"))
    hit, _ = check_identity(T, pl, scene_file)
    assert 0 < hit.sum() < W * H
    rays = screen_rays(cam, W, H)
    rec, rgb = gpu_ctx.traceRays(rays)
    rpl = gpu_ctx.traceRaysShading(rays)
    assert bits(rpl["rgb"]).tobytes() == bits(rgb).tobytes() and np.array_equal(rpl["node"], rec["closest_node"]), scene_file
    check_identity(T, rpl, scene_file + " rays")
    for p in PLANES:
        assert bits(pl[p]).tobytes() == bits(rpl[p]).tobytes(), (scene_file, p)
