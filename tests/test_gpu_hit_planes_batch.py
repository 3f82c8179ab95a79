"""Hit planes for batches on the GPU (c2rt_render_frames_hits*, c2rt_render_frames_posed_hits*).  Every comparison is of
bytes, and every yardstick comes from an entry point that shares none of the batch's new code:

  single frame  renderHits(cams[i]) — for a posed frame on a scratch context after uploadScene + updateScene(poses[i]);
  frame kernel  the rgb slices against renderFrames(cams, taps = 1).

Every buffer handed to a raw entry point is pre-filled with a sentinel and has guard elements behind every plane.
Frames are 61x47 unless stated otherwise: neither side is a multiple of the 8x8 tile, so a frame's last tiles overhang
and the next frame's slice starts in the middle of a tile row."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import chess2rt_amd as c2
import query_test_util as Q
import scene_update_util as U
from chess2rt_amd import _abi
from chess2rt_amd.api import HIT_PLANES
from query_test_util import SENTINEL, device_planes, fetch, free_all, last_error, lib, plane_bytes, same, scratch_ctx, struct_of, untouched, with_fields
from ray_query_util import bits

pytestmark = pytest.mark.gpu

W, H = 61, 47
PLANES = tuple(HIT_PLANES)
# the cameras of tests/test_gpu_hit_planes.py: the file's camera with its pitch raised so that part of the rays leave
# the scene while every node is still some ray's closest
PITCH_UP = {"lecture5.sdl": 5.0, "csg_stress.sdl": 5.0, "zaphod.sdl": 40.0, "lecture4-proc-texture.sdl": 5.0}


def make_scene(scene_file, width=W, height=H):
    scene = c2.parseSceneFromFile(os.path.join(U.SCENES, scene_file))
    scene.setFrameSize(width, height)
    scene.setAA(False)
    scene.setDof(False)
    hc = scene.camera
    hc.pitch += PITCH_UP[scene_file]
    scene.camera = hc
    return scene


def orbit(scene, n, yaw):
    cams = [scene.beginFrame()]
    for _ in range(n - 1):
        scene.rotateCamera(yaw, 0, 0)
        cams.append(scene.beginFrame())
    return cams


@functools.lru_cache(maxsize=None)
def orbit_case(scene_file):
    """(scene, five cameras 8 degrees apart, one-tap options) at 61x47, made once and shared (read-only)"""
    scene = make_scene(scene_file)
    return scene, orbit(scene, 5, 8.0), scene.renderOpts(taps=_abi.TAPS_1)


_SINGLES = {}


def singles(ctx, scene_file):
    """[renderHits(cams[i]) for the orbit of `scene_file`], all seven planes: the yardstick, computed once"""
    if scene_file not in _SINGLES:
        scene, cams, opts = orbit_case(scene_file)
        ctx.uploadScene(scene.desc)
        _SINGLES[scene_file] = [ctx.renderHits(cam, opts) for cam in cams]
    return _SINGLES[scene_file]


guarded = functools.partial(Q.guarded, HIT_PLANES)                  # 64 elements behind every plane, host and device
guarded_dev = functools.partial(Q.guarded_device, HIT_PLANES)


def raw(ctx, cams, n, opts, bufs, poses=None, posed=False, device=False, stream=None, null_struct=False, handle=True):
    """one of the four entry points: cams / poses ctypes arrays or None; the planes not in `bufs` ({name: host buffer,
    DeviceBytes or address}) are passed as null"""
    pl = struct_of(_abi.HitPlanes, bufs)
    fn = getattr(lib(), "c2rt_render_frames%s_hits%s" % ("_posed" if posed else "", "_device" if device else ""))
    args = [ctx.handle if handle else None, cams] + ([poses] if posed else []) + [n, C.byref(opts) if opts is not None else None,
                                                                                 None if null_struct else C.byref(pl)]
    return fn(*(args + ([stream] if device else [])))


def assert_slices(bufs, names, n, pixels, want, what):
    """bufs[name] holds want[i][name] at slice i for i < n, then sentinel"""
    for name in names:
        nb = plane_bytes(HIT_PLANES, name, pixels)
        for i in range(n):
            assert bufs[name][i * nb:(i + 1) * nb].tobytes() == bits(want[i][name]).tobytes(), "%s: frame %d, plane %s" % (what, i, name)
        assert (bufs[name][n * nb:] == SENTINEL).all(), "%s: plane %s: written behind frame %d" % (what, name, n - 1)


def assert_batch(got, want, what, names=PLANES):
    """{name: [n, ...]} against [{name: [...]}]"""
    assert set(got) == set(names), what
    for name in names:
        assert got[name].shape[0] == len(want) and got[name].dtype == HIT_PLANES[name][0], (what, name)
        for i, w in enumerate(want):
            assert same(got[name][i], w[name]), "%s: frame %d, plane %s differs from the single-frame call" % (what, i, name)


# ---- 1: composition, plain --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("scene_file", sorted(PITCH_UP))
def test_composition(gpu_ctx, scene_file):
    scene, cams, opts = orbit_case(scene_file)
    want = singles(gpu_ctx, scene_file)
    gpu_ctx.uploadScene(scene.desc)
    hit = np.stack([w["node"] for w in want]) >= 0
    assert hit.any() and not hit.all(), scene_file                                 # hits and misses in the batch
    assert len({w["p"].tobytes() + w["rgb"].tobytes() for w in want}) == 5         # the cameras see different frames
    got = gpu_ctx.renderFramesHits(cams, opts)
    shapes = {"node": (5, H, W), "leaf": (5, H, W), "dist": (5, H, W), "uv": (5, H, W, 2), "p": (5, H, W, 3), "normal": (5, H, W, 3),
              "rgb": (5, H, W, 3)}
    for name in PLANES:
        assert got[name].shape == shapes[name], (scene_file, name)
    assert_batch(got, want, scene_file)
    # the frame kernel's batch: an entry point that shares none of the new code
    frames = gpu_ctx.renderFrames(cams, opts)
    assert same(got["rgb"], frames), "%s: the rgb slices differ from the one-tap frames" % scene_file
    one = gpu_ctx.renderFramesHits(cams[3:4], opts)
    assert_batch(one, want[3:4], scene_file + ", one frame")
    # the device variant, every plane guarded
    dev = guarded_dev(PLANES, 5 * W * H)
    gpu_ctx.renderFramesHitsDevice(cams, opts, {k: v.ptr.value for k, v in dev.items()})
    assert_slices(fetch(dev), PLANES, 5, W * H, want, scene_file + ", device")
    free_all(dev)


# ---- 2: plane subsets -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("subset", [("node", "dist"), ("rgb",), ("uv", "normal")], ids=lambda s: "+".join(s))
def test_plane_subsets(gpu_ctx, subset):
    scene, cams, opts = orbit_case("lecture5.sdl")
    want = singles(gpu_ctx, "lecture5.sdl")
    gpu_ctx.uploadScene(scene.desc)
    n, px = 3, W * H
    arr = (_abi.CameraFrame * n)(*cams[:n])
    host, dev = guarded(PLANES, n * px), guarded_dev(PLANES, n * px)
    # what is not asked for is null in the struct; its buffer is kept to show that nothing strays into it
    assert raw(gpu_ctx, arr, n, opts, {k: host[k] for k in subset}) == _abi.OK, last_error(gpu_ctx)
    assert raw(gpu_ctx, arr, n, opts, {k: dev[k] for k in subset}, device=True) == _abi.OK, last_error(gpu_ctx)
    for where, bufs in (("host", host), ("device", fetch(dev))):
        assert_slices(bufs, subset, n, px, want, "%s %s" % (where, "+".join(subset)))
        assert untouched({k: v for k, v in bufs.items() if k not in subset}), (where, subset)
    free_all(dev)
    got = gpu_ctx.renderFramesHits(cams[:n], opts, planes=subset)
    assert_batch(got, want[:n], "+".join(subset), subset)


# ---- 3: strips --------------------------------------------------------------------------------------------------------------


def test_strips(gpu_ctx):
    scene, cams, opts = orbit_case("lecture5.sdl")
    want = singles(gpu_ctx, "lecture5.sdl")
    gpu_ctx.uploadScene(scene.desc)
    n, strip, world = 3, 4, 3
    full = gpu_ctx.renderFramesHits(cams[:n], opts)
    assert_batch(full, want[:n], "unstriped")
    seen = np.zeros(H, dtype=int)
    for rank in range(world):
        o = scene.renderOpts(taps=_abi.TAPS_1, strip_height=strip, strip_rank=rank, strip_world=world)
        rows = [y for y in range(H) if (y // strip) % world == rank]
        assert gpu_ctx.localRows(o) == len(rows)
        got = gpu_ctx.renderFramesHits(cams[:n], o)
        for i in range(n):
            single = gpu_ctx.renderHits(cams[i], o)
            for name in PLANES:
                assert got[name].shape[:3] == (n, len(rows), W), (rank, name)     # compact: local_rows * width per slice
                assert same(got[name][i], single[name]), (rank, i, name)
                assert same(got[name][i], np.ascontiguousarray(full[name][i][rows])), (rank, i, name)
        # the raw entry point: the slices are local_rows * width apart and nothing lands behind the last
        host = guarded(PLANES, n * len(rows) * W)
        assert raw(gpu_ctx, (_abi.CameraFrame * n)(*cams[:n]), n, o, host) == _abi.OK, last_error(gpu_ctx)
        assert_slices(host, PLANES, n, len(rows) * W, [{k: got[k][i] for k in PLANES} for i in range(n)], "rank %d" % rank)
        seen[rows] += 1
    assert (seen == 1).all()


# ---- 4: posed ---------------------------------------------------------------------------------------------------------------


def check_posed(ctx, scratch, scene_file, cams, poses, what):
    """slice i against uploadScene + updateScene(poses[i]) + renderHits(cams[i]) on the scratch context; the batch's
    context keeps its scene; a frame with a pose differs from the same camera's frame without it, in some plane"""
    scene, _, opts = orbit_case(scene_file)
    base = U.Desc(scene.desc)
    ctx.uploadScene(base.d)
    before = ctx.renderHits(cams[0], opts)
    got = ctx.renderFramesPosedHits(cams, poses, opts)
    want = []
    for cam, (nodes, lights) in zip(cams, poses):
        scratch.uploadScene(base.d)          # poses are relative to the scene as it is
        scratch.updateScene(nodes, lights)
        want.append(scratch.renderHits(cam, opts))
    assert_batch(got, want, what)
    after = ctx.renderHits(cams[0], opts)
    for name in PLANES:
        assert same(after[name], before[name]), "%s: the call changed the context's scene (plane %s)" % (what, name)
    plain = ctx.renderFramesHits(cams, opts)
    for i, (nodes, lights) in enumerate(poses):
        differs = [name for name in PLANES if not same(got[name][i], plain[name][i])]
        if nodes or lights:
            assert differs, "%s: frame %d ignores its pose" % (what, i)
        else:
            assert not differs, (what, i, differs)
    # frames whose poses differ, differ: under ONE camera, so that only the pose can tell them apart
    one_cam = ctx.renderFramesPosedHits([cams[0]] * len(poses), poses, opts)
    keys = [b"".join(one_cam[name][i].tobytes() for name in PLANES) for i in range(len(poses))]
    assert len(set(keys)) == len(poses), what
    dev = guarded_dev(PLANES, len(cams) * W * H)
    ctx.renderFramesPosedHitsDevice(cams, poses, opts, {k: v.ptr.value for k, v in dev.items()})
    assert_slices(fetch(dev), PLANES, len(cams), W * H, want, what + ", device")
    free_all(dev)
    return got


def test_posed_lecture5(gpu_ctx, scratch_ctx):
    """no pose; the three balls translated (every matrix stays the identity); one ball scaled (a general matrix); the light
    moved"""
    _, cams, _ = orbit_case("lecture5.sdl")
    poses = [({}, None),
             ({3: U.xf(("translate", 60, 15, 220)), 4: U.xf(("translate", 10, 45, 180)), 5: U.xf(("translate", -40, 15, 140))}, None),
             ({4: U.xf(("scale", 1.5, 2, 1.5), ("rotate", 20, 10, 0), ("translate", 50, 30, 206))}, None),
             (None, {0: dict(pos=(150, 500, 100), power=500000.0)})]
    got = check_posed(gpu_ctx, scratch_ctx, "lecture5.sdl", cams[:4], poses, "lecture5")
    # a moved light changes colours only
    plain = gpu_ctx.renderFramesHits(cams[:4], orbit_case("lecture5.sdl")[2])
    assert same(got["dist"][3], plain["dist"][3]) and not same(got["rgb"][3], plain["rgb"][3])


def test_posed_zaphod(gpu_ctx, scratch_ctx):
    """planes only, one light: a pose that rotates the plane node out of its axis beside an empty pose — the frame path
    runs two instance groups here, the hit planes one launch"""
    scene, cams, _ = orbit_case("zaphod.sdl")
    assert scene.desc.contents.n_nodes == 1 and scene.desc.contents.n_lights == 1
    check_posed(gpu_ctx, scratch_ctx, "zaphod.sdl", cams[:2], [({0: U.xf(("rotate", 10, 5, 0))}, None), ({}, None)], "zaphod")


def test_posed_csg_stress(gpu_ctx, scratch_ctx):
    """depth 4, three lights: two poses"""
    _, cams, _ = orbit_case("csg_stress.sdl")
    poses = [({1: U.xf(("translate", 15, 0, 10))}, None), ({2: U.xf(("scale", 1.2, 1.2, 1.2), ("translate", -10, 5, 0))}, {0: dict(pos=(100, 300, -150))})]
    check_posed(gpu_ctx, scratch_ctx, "csg_stress.sdl", cams[:2], poses, "csg_stress")


# ---- 5: stream order --------------------------------------------------------------------------------------------------------


def test_stream_order(gpu_ctx):
    """frame batch, hit batch, posed hit batch, a larger frame batch (the slot's table grows) on one stream of the
    caller's with no sync in between: each call rewrites the slot's table as soon as its own copy is ordered"""
    import torch

    scene, cams, opts = orbit_case("lecture5.sdl")
    want = singles(gpu_ctx, "lecture5.sdl")
    gpu_ctx.uploadScene(scene.desc)
    more = orbit(make_scene("lecture5.sdl"), 7, 5.0)
    poses = [({3: U.xf(("translate", 60, 15, 220))}, None), ({}, None), (None, {0: dict(pos=(150, 500, 100))})]
    want_frames = gpu_ctx.renderFrames(cams[:3], opts)
    want_posed = gpu_ctx.renderFramesPosedHits(cams[:3], poses, opts)
    want_more = gpu_ctx.renderFrames(more, opts)
    px = W * H
    dev = torch.device("cuda:0")

    def planes(n):
        return device_planes(HIT_PLANES, n * px, dev, guard_elems=64)

    def check(t, n, wanted, what):
        assert_slices({k: v.cpu().numpy() for k, v in t.items()}, PLANES, n, px, wanted, what)

    for stream in (torch.cuda.Stream(dev), None):
        handle = stream.cuda_stream if stream is not None else 0
        f1 = torch.full((3, H, W, 3), -1.0, dtype=torch.float32, device=dev)
        f2 = torch.full((7, H, W, 3), -1.0, dtype=torch.float32, device=dev)
        t1, t2 = planes(5), planes(3)
        torch.cuda.synchronize()
        gpu_ctx.renderFramesDevice(cams[:3], opts, f1.data_ptr(), handle)
        gpu_ctx.renderFramesHitsDevice(cams, opts, {k: v.data_ptr() for k, v in t1.items()}, handle)
        gpu_ctx.renderFramesPosedHitsDevice(cams[:3], poses, opts, {k: v.data_ptr() for k, v in t2.items()}, handle)
        if stream is not None:
            gpu_ctx.renderFramesDevice(more, opts, f2.data_ptr(), handle)
        (stream.synchronize if stream is not None else torch.cuda.synchronize)()
        what = "own stream" if stream is not None else "default stream"
        assert same(f1.cpu().numpy(), want_frames), what
        check(t1, 5, want, what)
        check(t2, 3, [{k: want_posed[k][i] for k in PLANES} for i in range(3)], what + ", posed")
        if stream is not None:
            assert same(f2.cpu().numpy(), want_more), what


# ---- 6: host chunking -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("scene_file,width,height,n,names", [("lecture4-proc-texture.sdl", 256, 256, 9, ("node", "dist", "rgb")),
                                                              ("lecture5.sdl", 640, 480, 2, ("node", "dist"))],
                         ids=["whole-frames-4-4-1", "row-chunks"])
def test_host_chunking(gpu_ctx, scene_file, width, height, n, names):
    """65536 pixels per frame: chunks of 4, 4 and 1 whole frames of the 2^18-pixel staging chunk; 307200 pixels per frame:
    more than 2^18, each frame in chunks of whole rows"""
    scene = make_scene(scene_file, width, height)
    cams = orbit(scene, n, 8.0)
    opts = scene.renderOpts(taps=_abi.TAPS_1)
    gpu_ctx.uploadScene(scene.desc)
    px = width * height
    assert (px <= 1 << 18) == (scene_file != "lecture5.sdl")
    host, dev = guarded(names, n * px), guarded_dev(names, n * px)
    arr = (_abi.CameraFrame * n)(*cams)
    assert raw(gpu_ctx, arr, n, opts, dev, device=True) == _abi.OK, last_error(gpu_ctx)
    assert raw(gpu_ctx, arr, n, opts, host) == _abi.OK, last_error(gpu_ctx)
    back = fetch(dev)
    for name in names:
        assert host[name].tobytes() == back[name].tobytes(), (scene_file, name)
        assert (host[name][plane_bytes(HIT_PLANES, name, n * px):] == SENTINEL).all(), (scene_file, name)
    free_all(dev)
    # and both are the single-frame call's: the last frame, which the last chunk holds
    last = gpu_ctx.renderHits(cams[-1], opts, planes=names)
    for name in names:
        nb = plane_bytes(HIT_PLANES, name, px)
        assert host[name][(n - 1) * nb:n * nb].tobytes() == bits(last[name]).tobytes(), (scene_file, name)
    assert len({host["dist"][i * px * 8:(i + 1) * px * 8].tobytes() for i in range(n)}) == n


# ---- 7: limits and refusals -------------------------------------------------------------------------------------------------


def test_256_frames_and_one_too_many(gpu_ctx):
    """C2RT_MAX_BATCH_FRAMES frames of 8x8 (one tile each), 1.4 degrees apart: a full turn"""
    scene = make_scene("lecture5.sdl", 8, 8)
    cams = orbit(scene, 256, 1.4)
    opts = scene.renderOpts(taps=_abi.TAPS_1)
    gpu_ctx.uploadScene(scene.desc)
    host = guarded(PLANES, 256 * 64)
    assert raw(gpu_ctx, (_abi.CameraFrame * 256)(*cams), 256, opts, host) == _abi.OK, last_error(gpu_ctx)
    for i in (0, 127, 255):
        single = gpu_ctx.renderHits(cams[i], opts)
        for name in PLANES:
            nb = plane_bytes(HIT_PLANES, name, 64)
            assert host[name][i * nb:(i + 1) * nb].tobytes() == bits(single[name]).tobytes(), (i, name)
    for name in PLANES:
        assert (host[name][plane_bytes(HIT_PLANES, name, 256 * 64):] == SENTINEL).all(), name
    assert len({host["rgb"][i * 768:(i + 1) * 768].tobytes() for i in range(256)}) > 128
    arr = (_abi.CameraFrame * 257)(*(cams + cams[:1]))
    parr = (_abi.ScenePose * 257)()          # both counts 0: frames of the scene as it is
    fresh, dev = guarded(PLANES, 64), guarded_dev(PLANES, 64)
    for posed in (False, True):
        for device in (False, True):
            assert raw(gpu_ctx, arr, 257, opts, dev if device else fresh, parr, posed, device) == _abi.ERR_LIMIT
            assert "257 frames" in last_error(gpu_ctx)
    assert untouched(fresh) and untouched(fetch(dev))
    free_all(dev)


def test_statuses_in_order_leave_the_outputs_untouched(gpu_ctx):
    width, height, n = 40, 24, 3
    scene = make_scene("lecture5.sdl", width, height)
    cams = orbit(scene, n, 8.0)
    opts = scene.renderOpts(taps=_abi.TAPS_1)
    gpu_ctx.uploadScene(scene.desc)
    arr = (_abi.CameraFrame * n)(*cams)
    big = (_abi.CameraFrame * 257)(*([cams[0]] * 257))
    t = U.xf(("translate", 0, 90, 200))
    # (a ScenePose owns its arrays: the lists keep them alive behind the ctypes arrays' copies)
    good_poses = [c2.makePose({3: t}), c2.makePose(), c2.makePose(None, {0: dict(power=1.0)})]
    bad_pose = c2.makePose({9: t})
    good = (_abi.ScenePose * n)(*good_poses)
    bad = (_abi.ScenePose * n)(good_poses[0], good_poses[1], bad_pose)
    big_poses = (_abi.ScenePose * 257)()
    px = n * width * height
    host, dev = guarded(PLANES, px), guarded_dev(PLANES, px)

    def cams_with(**kw):
        return (_abi.CameraFrame * n)(cams[0], with_fields(cams[1], **kw), cams[2])

    def opts_with(**kw):
        return with_fields(opts, **kw)

    def refused(status, cause, ctx=gpu_ctx, cc=arr, count=n, oo=opts, poses=good, null_struct=False, no_plane=False, plain=True):
        for posed in ((False, True) if plain else (True,)):
            for device in (False, True):
                bufs = {} if no_plane else (dev if device else host)
                got = raw(ctx, cc, count, oo, bufs, poses, posed, device, null_struct=null_struct)
                assert got == status, (cause, posed, device, got, last_error(ctx))
                assert cause in last_error(ctx), (cause, posed, device, last_error(ctx))
        assert untouched(host) and untouched(fetch(dev)), cause

    # 1, 2: the null context, then no frame at all — whatever the other pointers are
    garbage = {name: 0x10 for name in PLANES}
    for posed in (False, True):
        for device in (False, True):
            assert raw(gpu_ctx, None, 0, None, {}, None, posed, device, handle=False) == _abi.ERR_INVALID_ARG
            assert raw(gpu_ctx, arr, n, opts, dev if device else host, good, posed, device, handle=False) == _abi.ERR_INVALID_ARG
            assert raw(gpu_ctx, None, 0, None, {}, None, posed, device, null_struct=True) == _abi.OK
            assert raw(gpu_ctx, C.cast(0x10, C.POINTER(_abi.CameraFrame)), 0, C.cast(0x10, C.POINTER(_abi.RenderOpts)).contents, garbage,
                       C.cast(0x10, C.POINTER(_abi.ScenePose)), posed, device, stream=0x10) == _abi.OK
            assert raw(gpu_ctx, big, 0, opts_with(count_rays=1), dev if device else host, bad, posed, device) == _abi.OK
    assert untouched(host) and untouched(fetch(dev))
    # 3: a batch call's
    refused(_abi.ERR_INVALID_ARG, "null cameras", cc=None)
    refused(_abi.ERR_INVALID_ARG, "null cameras", oo=None)
    refused(_abi.ERR_LIMIT, "257 frames", cc=big, count=257, poses=big_poses)
    refused(_abi.ERR_UNSUPPORTED, "count_rays", oo=opts_with(count_rays=1))
    refused(_abi.ERR_UNSUPPORTED, "prepass_bucket", oo=opts_with(prepass_bucket=48))
    refused(_abi.ERR_UNSUPPORTED, "camera 1 has depth of field", cc=cams_with(dof=1, num_samples=4))
    refused(_abi.ERR_UNSUPPORTED, "camera 1 is a stereo camera", cc=cams_with(stereo_separation=0.5))
    refused(_abi.ERR_INVALID_ARG, "bad frame size", oo=opts_with(width=0))                     # a frame call's argument checks
    refused(_abi.ERR_INVALID_ARG, "strip_rank", oo=opts_with(strip_height=8, strip_rank=2, strip_world=2))
    fresh = c2.Context(0)
    try:
        refused(_abi.ERR_NO_SCENE, "no scene", ctx=fresh)
        refused(_abi.ERR_NO_SCENE, "no scene", ctx=fresh, null_struct=True)                    # before the planes
    finally:
        fresh.close()
    two = c2.Context(devices=[0, 0])
    try:
        two.uploadScene(scene.desc)
        refused(_abi.ERR_UNSUPPORTED, "multi-device", ctx=two)
        refused(_abi.ERR_LIMIT, "257 frames", ctx=two, cc=big, count=257, poses=big_poses)     # the limit comes first
        refused(_abi.ERR_UNSUPPORTED, "multi-device", ctx=two, oo=opts_with(count_rays=1))     # then the context
    finally:
        two.close()
    # 4: the planes
    refused(_abi.ERR_INVALID_ARG, "null planes", null_struct=True)
    refused(_abi.ERR_INVALID_ARG, "all seven", no_plane=True)
    # 5: the poses
    refused(_abi.ERR_INVALID_ARG, "null poses", poses=None, plain=False)
    refused(_abi.ERR_INVALID_ARG, "frame 2: pose: node_index[0] = 9 out of range", poses=bad, plain=False)
    assert last_error(gpu_ctx).startswith("frame 2: ")
    # the order: where two causes are present the earlier one wins
    refused(_abi.ERR_INVALID_ARG, "null cameras", cc=None, count=257)
    refused(_abi.ERR_LIMIT, "257 frames", cc=big, count=257, oo=opts_with(count_rays=1), poses=big_poses)
    refused(_abi.ERR_UNSUPPORTED, "count_rays", oo=opts_with(count_rays=1, prepass_bucket=48), cc=cams_with(dof=1, num_samples=4))
    refused(_abi.ERR_UNSUPPORTED, "prepass_bucket", oo=opts_with(prepass_bucket=48), cc=cams_with(dof=1, num_samples=4))
    refused(_abi.ERR_UNSUPPORTED, "count_rays", oo=opts_with(count_rays=1), null_struct=True)
    refused(_abi.ERR_UNSUPPORTED, "depth of field", cc=cams_with(dof=1, num_samples=4), null_struct=True)
    refused(_abi.ERR_UNSUPPORTED, "stereo", cc=cams_with(stereo_separation=0.5), no_plane=True, poses=bad)
    refused(_abi.ERR_INVALID_ARG, "bad frame size", oo=opts_with(width=0), null_struct=True, poses=None)
    refused(_abi.ERR_INVALID_ARG, "null planes", null_struct=True, poses=None)
    refused(_abi.ERR_INVALID_ARG, "all seven", no_plane=True, poses=bad)
    refused(_abi.ERR_INVALID_ARG, "null poses", poses=None, plain=False)
    # afterwards the same context renders the batch, plain and posed, host and device
    want = [gpu_ctx.renderHits(cam, opts) for cam in cams]
    assert raw(gpu_ctx, arr, n, opts, host) == _abi.OK, last_error(gpu_ctx)
    assert_slices(host, PLANES, n, width * height, want, "after the refusals")
    assert raw(gpu_ctx, arr, n, opts, dev, device=True) == _abi.OK, last_error(gpu_ctx)
    back = fetch(dev)
    for name in PLANES:
        assert back[name].tobytes() == host[name].tobytes(), name
    posed_host = guarded(PLANES, px)
    assert raw(gpu_ctx, arr, n, opts, posed_host, good, True) == _abi.OK, last_error(gpu_ctx)
    assert posed_host["rgb"].tobytes() != host["rgb"].tobytes()
    assert raw(gpu_ctx, arr, n, opts, dev, good, True, True) == _abi.OK, last_error(gpu_ctx)
    back = fetch(dev)
    for name in PLANES:
        assert back[name].tobytes() == posed_host[name].tobytes(), name
    free_all(dev)


# ---- 8: the Python face -----------------------------------------------------------------------------------------------------


def test_python_face(gpu_ctx):
    scene, cams, opts = orbit_case("lecture5.sdl")
    want = singles(gpu_ctx, "lecture5.sdl")
    gpu_ctx.uploadScene(scene.desc)
    none = [({}, None)] * 3
    got = gpu_ctx.renderFramesPosedHits((_abi.CameraFrame * 3)(*cams[:3]), none, opts)
    assert_batch(got, want[:3], "ctypes cameras, empty poses")
    got = gpu_ctx.renderFramesPosedHits(cams[:3], [c2.makePose()] * 3, opts, planes=("dist",))
    assert list(got) == ["dist"] and same(got["dist"][2], want[2]["dist"])
    empty = gpu_ctx.renderFramesHits([], opts)
    assert empty["node"].shape == (0, H, W) and empty["uv"].shape == (0, H, W, 2)
    with pytest.raises(ValueError):
        gpu_ctx.renderFramesHits(cams, opts, planes=("depth",))
    with pytest.raises(ValueError):
        gpu_ctx.renderFramesHitsDevice(cams, opts, {"depth": 1})
    with pytest.raises(ValueError):
        gpu_ctx.renderFramesPosedHits(cams[:3], none[:2], opts)
    with pytest.raises(ValueError):
        gpu_ctx.renderFramesPosedHitsDevice(cams[:3], none[:2], opts, {"node": 1})
    for call, status in ((lambda: gpu_ctx.renderFramesHits(cams * 52, opts), _abi.ERR_LIMIT),
                         (lambda: gpu_ctx.renderFramesHits(cams, opts, planes=()), _abi.ERR_INVALID_ARG),
                         (lambda: gpu_ctx.renderFramesHitsDevice(cams, opts, {"node": 0}), _abi.ERR_INVALID_ARG),
                         (lambda: gpu_ctx.renderFramesPosedHits(cams[:3], [({9: U.xf()}, None)] * 3, opts), _abi.ERR_INVALID_ARG),
                         (lambda: gpu_ctx.renderFramesPosedHitsDevice(cams[:3], none, opts, {}), _abi.ERR_INVALID_ARG)):
        with pytest.raises(c2.C2rtError) as e:
            call()
        assert e.value.status == status, str(e.value)
