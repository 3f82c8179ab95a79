"""Hit planes on the GPU (c2rt_render_hits*): every plane against the ray queries over the frame's own screen rays
(the query kernel), the context's 1-tap frame (the frame kernel), its pixel probe and the CPU oracle.  All comparisons
are exact except where ray_query_util.assert_records_match_oracle allows the project's probe tolerances against the
oracle."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import chess2rt_amd as c2
from chess2rt_amd import _abi
from chess2rt_amd.api import HIT_PLANES, RAY_HIT_DTYPE
from golden_configs import SCENES
from query_test_util import HITS, check_device_against_host, check_filled, check_strips, device_planes, guarded, last_error, raw_call, untouched, with_fields
from ray_query_util import assert_records_match_oracle, bits, oracle_trace, record_from_trace_result, screen_rays

pytestmark = pytest.mark.gpu

W, H = 61, 47
PLANES = tuple(HIT_PLANES)
# the set-up of test_gpu_ray_queries.test_a_frames_own_rays_reproduce_the_frame: the file's camera with its pitch raised
# so that at least a tenth of the rays leave the scene while every node is still some ray's closest
PITCH_UP = {"lecture5.sdl": 5.0, "csg_stress.sdl": 5.0, "zaphod.sdl": 40.0, "lecture4-proc-texture.sdl": 5.0}


def make_scene(scene_file, width, height, pitch_up=0.0):
    scene = c2.parseSceneFromFile(os.path.join(SCENES, scene_file))
    scene.setFrameSize(width, height)
    scene.setAA(False)
    scene.setDof(False)
    hc = scene.camera
    hc.pitch += pitch_up
    scene.camera = hc
    return scene, scene.beginFrame(), scene.renderOpts(taps=_abi.TAPS_1)


@functools.lru_cache(maxsize=None)
def frame_case(scene_file):
    """(scene, camera, options, screen rays, oracle records) at 61x47, computed once and shared (read-only)"""
    scene, cam, opts = make_scene(scene_file, W, H, PITCH_UP[scene_file])
    rays = screen_rays(cam, W, H)
    return scene, cam, opts, rays, oracle_trace(scene.desc, rays)


def field_of(name, rec, rgb):
    """the plane `name` as the ray queries report it for the same rays, flat"""
    if name == "node":
        return np.ascontiguousarray(rec["closest_node"])
    if name == "leaf":
        return np.ascontiguousarray(rec["leaf_geom"])
    if name == "dist":
        return np.ascontiguousarray(rec["dist"])
    if name == "uv":
        return np.ascontiguousarray(np.stack([rec["u"], rec["v"]], axis=1))
    if name == "p":
        return np.ascontiguousarray(rec["p"])
    if name == "normal":
        return np.ascontiguousarray(rec["normal"])
    return np.ascontiguousarray(rgb)


def records_of(pl):
    n = pl["node"].size
    rec = np.zeros(n, dtype=RAY_HIT_DTYPE)
    rec["closest_node"] = pl["node"].ravel()
    rec["leaf_geom"] = pl["leaf"].ravel()
    rec["dist"] = pl["dist"].ravel()
    rec["u"], rec["v"] = pl["uv"].reshape(n, 2)[:, 0], pl["uv"].reshape(n, 2)[:, 1]
    rec["p"] = pl["p"].reshape(n, 3)
    rec["normal"] = pl["normal"].reshape(n, 3)
    return rec


# ---- 1: the planes are the frame's own rays ------------------------------------------------------------------------


@pytest.mark.parametrize("scene_file", sorted(PITCH_UP))
def test_the_planes_are_the_frames_own_rays(gpu_ctx, scene_file):
    scene, cam, opts, rays, want = frame_case(scene_file)
    n = W * H
    hit = want["closest_node"] >= 0
    assert hit.sum() >= 0.1 * n and (~hit).sum() >= 0.1 * n, (scene_file, int(hit.sum()))
    assert set(int(v) for v in want["closest_node"][hit]) == set(range(scene.desc.contents.n_nodes)), scene_file
    gpu_ctx.uploadScene(scene.desc)
    pl = gpu_ctx.renderHits(cam, opts)
    assert set(pl) == set(PLANES)
    rec, rgb = gpu_ctx.traceRays(rays)
    for name in PLANES:
        assert bits(pl[name]).tobytes() == bits(field_of(name, rec, rgb)).tobytes(), "%s: plane %s differs from the ray query's field" % (scene_file, name)
    frame = gpu_ctx.renderFrame(cam, opts)
    assert bits(pl["rgb"]).tobytes() == bits(frame).tobytes(), "%s: rgb differs from the 1-tap frame" % scene_file
    got = records_of(pl)
    assert_records_match_oracle(got, want, scene_file)
    rng = np.random.RandomState(5)
    pts = [(int(rng.randint(0, W)), int(rng.randint(0, H))) for _ in range(100)] + [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    for (x, y) in pts:
        g = record_from_trace_result(gpu_ctx.renderPixel(cam, opts, x, y))
        i = y * W + x
        assert bits(np.array([g], dtype=RAY_HIT_DTYPE)).tobytes() == bits(got[i:i + 1]).tobytes(), (scene_file, x, y)


# ---- 2: edges --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("height", [1, 9])
def test_edges(gpu_ctx, height):
    for width in (1, 7, 8, 9, 63, 64, 65):
        scene, cam, opts = make_scene("lecture5.sdl", width, height, PITCH_UP["lecture5.sdl"])
        gpu_ctx.uploadScene(scene.desc)
        rec, rgb = gpu_ctx.traceRays(screen_rays(cam, width, height))
        n = width * height
        bufs = guarded(HIT_PLANES, PLANES, n)
        assert raw_call(HITS, gpu_ctx, bufs, cam, opts) == _abi.OK, last_error(gpu_ctx)
        check_filled(HIT_PLANES, bufs, {name: field_of(name, rec, rgb) for name in PLANES}, n, (width, height))


# ---- 3: plane subsets --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("subset", [(p,) for p in PLANES] + [("node", "dist")], ids=lambda s: "+".join(s))
def test_plane_subsets(gpu_ctx, subset):
    scene, cam, opts, _, _ = frame_case("lecture5.sdl")
    gpu_ctx.uploadScene(scene.desc)
    full = gpu_ctx.renderHits(cam, opts)
    n = W * H
    bufs = guarded(HIT_PLANES, subset, n)
    # what is not asked for is null in the struct; the buffers passed sit in one allocation each with their guards
    assert raw_call(HITS, gpu_ctx, bufs, cam, opts) == _abi.OK, last_error(gpu_ctx)
    check_filled(HIT_PLANES, bufs, full, n, subset, subset)
    got = gpu_ctx.renderHits(cam, opts, planes=subset)
    assert set(got) == set(subset)
    for name in subset:
        assert bits(got[name]).tobytes() == bits(full[name]).tobytes(), (subset, name)


# ---- 4: strips -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("world", [2, 3])
def test_strips(gpu_ctx, world):
    sw, sh, strip = 40, 50, 8
    scene, cam, opts = make_scene("lecture5.sdl", sw, sh, PITCH_UP["lecture5.sdl"])
    gpu_ctx.uploadScene(scene.desc)
    names = ("node", "dist", "normal", "rgb")
    full = gpu_ctx.renderHits(cam, opts, planes=names)
    assert 0 < int((full["node"] >= 0).sum()) < sw * sh
    check_strips(gpu_ctx, scene, lambda o: gpu_ctx.renderHits(cam, o, planes=names), full, sh, world, strip, names, world)


# ---- 5: no hit -------------------------------------------------------------------------------------------------------


def test_no_hit(gpu_ctx):
    scene, cam, opts = make_scene("lecture5.sdl", 33, 17, 0.0)
    hc = scene.camera
    hc.pitch = 80.0      # at the sky
    scene.camera = hc
    cam = scene.beginFrame()
    want = oracle_trace(scene.desc, screen_rays(cam, 33, 17))
    assert (want["closest_node"] == -1).all()
    gpu_ctx.uploadScene(scene.desc)
    pl = gpu_ctx.renderHits(cam, opts)
    assert (pl["node"] == -1).all() and (pl["leaf"] == -1).all()
    assert bits(pl["dist"]).tobytes() == bits(np.full((17, 33), 1e99)).tobytes()
    for name in ("uv", "p", "normal", "rgb"):
        assert not bits(pl[name]).any(), name


# ---- 6: statuses, before anything is touched -----------------------------------------------------------------------------


def test_statuses_leave_the_outputs_untouched(gpu_ctx):
    scene, cam, opts, rays, _ = frame_case("lecture5.sdl")
    gpu_ctx.uploadScene(scene.desc)
    n = W * H

    def copy_cam(**kw):
        return with_fields(cam, **kw)

    def copy_opts(**kw):
        return with_fields(opts, **kw)

    bufs = guarded(HIT_PLANES, PLANES, n)
    assert raw_call(HITS, gpu_ctx, bufs, cam, opts, null_struct=True) == _abi.ERR_INVALID_ARG
    assert last_error(gpu_ctx) == "null planes"
    assert raw_call(HITS, gpu_ctx, {}, cam, opts) == _abi.ERR_INVALID_ARG
    assert last_error(gpu_ctx) == "no plane asked for: all seven pointers of c2rt_hit_planes are null"
    cases = [(copy_cam(dof=1, num_samples=4), opts, "depth of field: a pixel's record is one ray's, a lens has many per pixel"),
             (copy_cam(stereo_separation=0.5), opts, "stereo: a pixel's record is one ray's, a stereo camera has two per pixel"),
             (cam, copy_opts(count_rays=1), "count_rays: the hit planes do not count rays"),
             (cam, copy_opts(prepass_bucket=48), "prepass_bucket: a preview's pixels share the sample of their block")]
    lib = _abi.load_library()
    for c, o, cause in cases:
        assert raw_call(HITS, gpu_ctx, bufs, c, o) == _abi.ERR_UNSUPPORTED, cause
        assert last_error(gpu_ctx) == cause, (cause, last_error(gpu_ctx))
        assert untouched(bufs), cause
        # the device variant decides the same before it enqueues anything (the pointers are never used)
        pl = _abi.HitPlanes()
        pl.node = bufs["node"].ctypes.data
        assert lib.c2rt_render_hits_device(gpu_ctx.handle, C.byref(c), C.byref(o), C.byref(pl), None) == _abi.ERR_UNSUPPORTED, cause
        assert last_error(gpu_ctx) == cause
    fresh = c2.Context(0)
    try:
        assert raw_call(HITS, fresh, bufs, cam, opts) == _abi.ERR_NO_SCENE
        assert "no scene" in last_error(fresh)
    finally:
        fresh.close()
    assert untouched(bufs)
    # afterwards the same context renders a correct plane set
    rec, rgb = gpu_ctx.traceRays(rays)
    assert raw_call(HITS, gpu_ctx, bufs, cam, opts) == _abi.OK
    check_filled(HIT_PLANES, bufs, {name: field_of(name, rec, rgb) for name in PLANES}, n, "after the refusals")


# ---- 7: streams and slots -------------------------------------------------------------------------------------------


def test_streams_and_slots(gpu_ctx):
    import torch

    scene, cam, opts, rays, _ = frame_case("csg_stress.sdl")
    gpu_ctx.uploadScene(scene.desc)
    n = W * H
    want = gpu_ctx.renderHits(cam, opts)
    want_frame = gpu_ctx.renderFrame(cam, opts)
    dev = torch.device("cuda:0")
    s1 = torch.cuda.Stream(dev)
    t = device_planes(HIT_PLANES, n, dev, guard_bytes=64)
    frame_t = torch.full((H, W, 3), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    gpu_ctx.renderHitsDevice(cam, opts, {k: v.data_ptr() for k, v in t.items()}, s1.cuda_stream)
    gpu_ctx.renderFrameDevice(cam, opts, frame_t.data_ptr(), s1.cuda_stream)
    s1.synchronize()
    check_device_against_host(HIT_PLANES, t, want, n, "own stream")
    assert bits(frame_t.cpu().numpy()).tobytes() == bits(want_frame).tobytes()
    two = c2.Context(devices=[0, 0])
    try:
        two.uploadScene(scene.desc)
        t2 = device_planes(HIT_PLANES, n, dev, guard_bytes=64)
        torch.cuda.synchronize()
        two.renderHitsDevice(cam, opts, {k: v.data_ptr() for k, v in t2.items()}, s1.cuda_stream)
        s1.synchronize()
        for name in PLANES:
            assert t2[name].cpu().numpy().tobytes() == t[name].cpu().numpy().tobytes(), name
        host = two.renderHits(cam, opts)
        for name in PLANES:
            assert bits(host[name]).tobytes() == bits(want[name]).tobytes(), name
    finally:
        two.close()


# ---- 8: host mirror and Python face -----------------------------------------------------------------------------------


def test_host_mirror_and_python_face(gpu_ctx):
    scene, cam, opts = make_scene("lecture5.sdl", 32, 24)
    gpu_ctx.uploadScene(scene.desc)
    want = gpu_ctx.renderHits(cam, opts)
    shapes = {"node": (24, 32), "leaf": (24, 32), "dist": (24, 32), "uv": (24, 32, 2), "p": (24, 32, 3), "normal": (24, 32, 3), "rgb": (24, 32, 3)}
    for name in PLANES:
        assert want[name].shape == shapes[name] and want[name].dtype == HIT_PLANES[name][0], name
    assert 0 < int((want["node"] >= 0).sum())
    got = c2.Renderer(scene, gpu_ctx).renderHits()
    assert set(got) == set(PLANES)
    for name in PLANES:
        assert got[name].shape == shapes[name] and got[name].dtype == want[name].dtype, name
        assert bits(got[name]).tobytes() == bits(want[name]).tobytes(), name
    sub = c2.Renderer(scene, gpu_ctx).renderHits(planes=("dist",))
    assert list(sub) == ["dist"] and bits(sub["dist"]).tobytes() == bits(want["dist"]).tobytes()
    with pytest.raises(ValueError):
        gpu_ctx.renderHits(cam, opts, planes=("depth",))
    dof = c2.parseSceneFromFile(os.path.join(SCENES, "zaphod.sdl"))      # as shipped: depth of field
    dof.setFrameSize(32, 24)
    assert dof.camera.dof
    with pytest.raises(c2.C2rtError) as e:
        c2.Renderer(dof, gpu_ctx).renderHits()
    assert e.value.status == _abi.ERR_UNSUPPORTED and "depth of field" in str(e.value)


# ---- 9: host chunking ---------------------------------------------------------------------------------------------------


def test_host_chunks_of_a_frame_equal_the_device_call(gpu_ctx):
    import torch

    w, h = 640, 480                          # 307 200 pixels: chunks of 409 and 71 whole rows
    scene, cam, opts = make_scene("lecture5.sdl", w, h)
    gpu_ctx.uploadScene(scene.desc)
    host = gpu_ctx.renderHits(cam, opts)
    dev = torch.device("cuda:0")
    s1 = torch.cuda.Stream(dev)
    t = device_planes(HIT_PLANES, w * h, dev, guard_bytes=64)
    torch.cuda.synchronize()
    gpu_ctx.renderHitsDevice(cam, opts, {k: v.data_ptr() for k, v in t.items()}, s1.cuda_stream)
    s1.synchronize()
    check_device_against_host(HIT_PLANES, t, host, w * h, "640x480")
    assert 0 < int((host["node"][409:] >= 0).sum())                    # hits behind the chunk boundary
