"""Adaptive anti-aliasing for batches on the GPU (c2rt_render_frames_adaptive*, c2rt_render_frames_posed_adaptive*).
Every comparison is of bits, and every yardstick is built from entry points that do not share the batch's new code:

  composition   the one-tap and the five-tap batch (renderFrames / renderFramesPosed) and the typed numpy edge test
                (tests/aa_reference.py) applied to the one-tap frames: mask i is the numpy mask of one-tap frame i, a
                flagged pixel holds the five-tap bits, an unflagged one the one-tap bits;
  single frame  renderFrameAdaptive(cams[i]) — for a posed frame on a scratch context after updateScene(poses[i]).

The flagged shares in the comments were computed on the CPU oracle's one-tap frames at threshold 0.1; each test prints
the shares of the GPU's own one-tap frames and asserts its bounds on them.  Where the case gives no bound of its own the
bound is the orbit's, 0.02 <= share <= 0.90: some but not all tiles have work."""
import ctypes as C
import os

import numpy as np
import pytest

import chess2rt_amd as c2
import scene_update_util as U
from aa_reference import needs_aa, tile_counts
from chess2rt_amd import _abi
from query_test_util import DeviceBytes, frame_and_mask, hip_runtime, holds, last_error, lib, same, scratch_ctx, untouched, with_fields
from query_test_util import float_bits as bits

pytestmark = pytest.mark.gpu

GUARD = 64               # extra bytes behind both outputs
THR = _abi.AA_THRESHOLD_REF


def file_scene(name, size):
    scene = c2.parseSceneFromFile(os.path.join(U.SCENES, name))
    scene.setFrameSize(*size)
    scene.setAA(False)
    scene.setDof(False)
    return scene


def orbit(scene, n, yaw):
    cams = [scene.beginFrame()]
    for _ in range(n - 1):
        scene.rotateCamera(yaw, 0, 0)
        cams.append(scene.beginFrame())
    return cams


def opts_of(scene):
    return scene.renderOpts(taps=_abi.TAPS_1), scene.renderOpts(taps=_abi.TAPS_REF5)


def classes(mask):
    """tiles with 1..16 flags (one round of the packed refinement), 17..63 (several rounds), 64 (a full tile)"""
    k = tile_counts(mask)
    return int(((k >= 1) & (k <= 16)).sum()), int(((k >= 17) & (k <= 63)).sum()), int((k == 64).sum())


def shares(what, one, thr=THR):
    """the numpy masks of the one-tap frames, their shares printed"""
    want = [needs_aa(f, thr) for f in one]
    print("%s: flagged shares %s, tiles with 1..16 / 17..63 / 64 flags %s" % (
        what, " / ".join("%.1f %%" % (100 * float(m.mean())) for m in want), " ".join("%d/%d/%d" % classes(m) for m in want)))
    return want


def assert_composition(frames, masks, one, five, want, what):
    assert frames.dtype == np.float32 and frames.shape == one.shape, what
    assert masks.dtype == np.uint8 and masks.shape == one.shape[:3], what
    for i in range(len(one)):
        assert masks[i].tobytes() == want[i].tobytes(), "%s: frame %d: %d mask bytes differ from the numpy detection" % (what, i, int((masks[i] != want[i]).sum()))
        m = want[i] == 1
        assert bits(frames[i])[m].tobytes() == bits(five[i])[m].tobytes(), "%s: frame %d: flagged pixels differ from the five-tap frame" % (what, i)
        assert bits(frames[i])[~m].tobytes() == bits(one[i])[~m].tobytes(), "%s: frame %d: unflagged pixels differ from the one-tap frame" % (what, i)


def assert_single_frames(ctx, cams, five_opts, frames, masks, what, thr=THR):
    for i, cam in enumerate(cams):
        f, m = ctx.renderFrameAdaptive(cam, five_opts, thr)
        assert same(masks[i], m) and same(frames[i], f), "%s: frame %d differs from the single-frame call" % (what, i)


def assert_posed_single_frames(scratch, base, cams, poses, five_opts, frames, masks, what):
    for i, (cam, (nodes, lights)) in enumerate(zip(cams, poses)):
        scratch.uploadScene(base.d)        # poses are relative to the scene as it is
        scratch.updateScene(nodes, lights)
        f, m = scratch.renderFrameAdaptive(cam, five_opts, THR)
        assert same(masks[i], m) and same(frames[i], f), "%s: frame %d differs from update + single-frame call" % (what, i)


def check_plain(ctx, scene, cams, what, lo=0.02, hi=0.90):
    """uploads, renders yardsticks and batch, compares; returns (frames, masks, one, five, numpy masks)"""
    o1, o5 = opts_of(scene)
    ctx.uploadScene(scene.desc)
    one, five = ctx.renderFrames(cams, o1), ctx.renderFrames(cams, o5)
    want = shares(what, one)
    for m in want:
        assert lo <= float(m.mean()) <= hi, (what, float(m.mean()))
    frames, masks = ctx.renderFramesAdaptive(cams, o5)
    assert_composition(frames, masks, one, five, want, what)
    assert_single_frames(ctx, cams, o5, frames, masks, what)
    return frames, masks, one, five, want


def check_posed(ctx, scratch, scene, cams, poses, what):
    """the same for a posed batch, bounds left to the caller; returns (frames, masks, numpy masks)"""
    o1, o5 = opts_of(scene)
    base = U.Desc(scene.desc)
    ctx.uploadScene(base.d)
    before = ctx.renderFrame(cams[0], o5)
    one, five = ctx.renderFramesPosed(cams, poses, o1), ctx.renderFramesPosed(cams, poses, o5)
    want = shares(what, one)
    frames, masks = ctx.renderFramesPosedAdaptive(cams, poses, o5)
    assert_composition(frames, masks, one, five, want, what)
    # the context's scene is unchanged
    assert same(ctx.renderFrame(cams[0], o5), before), what
    assert_posed_single_frames(scratch, base, cams, poses, o5, frames, masks, what)
    return frames, masks, want


# ---- 1: an orbit ------------------------------------------------------------------------------------------------------------


def test_orbit(gpu_ctx):
    """lecture5 67x45, four cameras 8 degrees apart: oracle shares 14.1 / 14.8 / 14.0 / 11.4 %"""
    scene = file_scene("lecture5.sdl", (67, 45))
    cams = orbit(scene, 4, 8.0)
    frames, masks, one, five, want = check_plain(gpu_ctx, scene, cams, "orbit")
    for i, m in enumerate(want):
        few, several, full = classes(m)
        assert few > 0 and several > 0, (i, few, several, full)
    assert len({m.tobytes() for m in masks}) == 4 and len({f.tobytes() for f in frames}) == 4
    # the refinement did something in every frame
    for i in range(4):
        m = want[i] == 1
        assert (bits(five[i])[m] != bits(one[i])[m]).any(), i


# ---- 2: poses ---------------------------------------------------------------------------------------------------------------


def five_poses():
    """tests/test_gpu_frames_posed.py::_five_poses: none; the three balls translated; one ball scaled (the general
    instance); the light moved; CSG object, globe and light moved"""
    return [
        ({}, None),
        ({3: U.xf(("translate", 60, 15, 220)), 4: U.xf(("translate", 10, 45, 180)), 5: U.xf(("translate", -40, 15, 140))}, None),
        ({4: U.xf(("scale", 1.5, 2, 1.5), ("translate", 50, 30, 206))}, None),
        (None, {0: dict(pos=(150, 500, 100), power=500000.0)}),
        ({2: U.xf(("translate", 30, 0, 40)), 1: U.xf(("translate", -20, 10, -60))}, {0: dict(pos=(-200, 400, 300))}),
    ]


def test_posed(gpu_ctx, scratch_ctx):
    """lecture5 100x52, five cameras and five poses: oracle shares 13.9 / 13.2 / 15.0 / 14.7 / 46.2 %"""
    scene = file_scene("lecture5.sdl", (100, 52))
    cams = orbit(scene, 5, 8.0)
    frames, masks, want = check_posed(gpu_ctx, scratch_ctx, scene, cams, five_poses(), "posed")
    for m in want:
        assert 0.02 <= float(m.mean()) <= 0.90, float(m.mean())
    assert len({m.tobytes() for m in masks}) == 5


# ---- 3: two instance groups; frames without flags among frames with flags -------------------------------------------


def test_two_instance_groups_keep_every_frame_at_its_index(gpu_ctx, scratch_ctx, tmp_path):
    """planes only, 100x52: frames 0, 2 and 4 keep the plane instance, frames 1 and 3 rotate a plane out of it, so the
    one-tap table is ordered 0 2 4 1 3 while frames, masks and refinement blocks go by frame.  Oracle shares 2.7 / 0 / 0
    / 3.9 / 3.0 %"""
    scene = U.load_text(tmp_path, U.planes_only(), "planes.sdl", (100, 52))
    cams = orbit(scene, 5, 5.0)
    poses = [({}, None), ({1: U.xf(("rotate", 0, 20, 0))}, None), ({1: U.xf(("translate", 0, -20, 0))}, None),
             ({0: U.xf(("rotate", 10, 5, 0))}, None), ({0: U.xf(("scale", 2, 3, 2))}, None)]
    frames, masks, want = check_posed(gpu_ctx, scratch_ctx, scene, cams, poses, "planes")
    for i in (1, 2):
        assert int(want[i].sum()) == 0 and int(masks[i].sum()) == 0, i
    for i in (0, 3, 4):
        assert int(want[i].sum()) > 0 and int(masks[i].sum()) > 0, i
    assert len({f.tobytes() for f in frames}) == 5


# ---- 4: several lights ------------------------------------------------------------------------------------------------------


def test_several_lights(gpu_ctx, tmp_path):
    """lecture5_like(3) 96x64, three cameras: the MLC instance.  Oracle shares 37.2 / 39.0 / 39.5 %"""
    scene = U.load_text(tmp_path, U.lecture5_like(3), "l5x3.sdl", (96, 64))
    assert scene.desc.contents.n_lights == 3
    cams = orbit(scene, 3, 8.0)
    frames, masks, one, five, want = check_plain(gpu_ctx, scene, cams, "three lights")
    for i, m in enumerate(want):
        assert classes(m)[2] > 0, (i, classes(m))


# ---- 5: nested CSG ----------------------------------------------------------------------------------------------------------


def test_nested_csg_posed(gpu_ctx, scratch_ctx, tmp_path):
    """nested_csg() 96x64 (depth 2), three cameras, frame 1 posed.  Oracle shares 7.8 / 7.4 / 7.8 %"""
    scene = U.load_text(tmp_path, U.nested_csg(), "nested.sdl", (96, 64))
    cams = orbit(scene, 3, 8.0)
    poses = [({}, None), ({1: U.xf(("translate", 20, 0, 10))}, None), ({}, None)]
    frames, masks, want = check_posed(gpu_ctx, scratch_ctx, scene, cams, poses, "nested csg")
    for m in want:
        assert 0.02 <= float(m.mean()) <= 0.90, float(m.mean())


def test_csg_stress(gpu_ctx):
    """csg_stress.sdl 96x72 (depth 4: 40 KiB of hit stack per wave), three cameras.  Oracle shares 54.9 / 54.6 / 53.5 %;
    every frame has at least 79 multi-round tiles and 4 to 6 full tiles"""
    scene = file_scene("csg_stress.sdl", (96, 72))
    cams = orbit(scene, 3, 8.0)
    frames, masks, one, five, want = check_plain(gpu_ctx, scene, cams, "csg_stress")
    for i, m in enumerate(want):
        few, several, full = classes(m)
        assert several >= 79 and 4 <= full <= 6, (i, few, several, full)


# ---- 6: nothing flagged -----------------------------------------------------------------------------------------------------


def test_nothing_flagged(gpu_ctx):
    """zaphod.sdl without depth of field 129x86, two cameras: oracle share 0 in both"""
    scene = file_scene("zaphod.sdl", (129, 86))
    cams = orbit(scene, 2, 8.0)
    frames, masks, one, five, want = check_plain(gpu_ctx, scene, cams, "zaphod", lo=0.0, hi=0.0)
    assert not masks.any() and same(frames, one)
    assert not same(one[0], one[1])


def test_a_threshold_nothing_reaches(gpu_ctx):
    scene = file_scene("lecture5.sdl", (67, 45))
    cams = orbit(scene, 4, 8.0)
    o1, o5 = opts_of(scene)
    gpu_ctx.uploadScene(scene.desc)
    one = gpu_ctx.renderFrames(cams, o1)
    frames, masks = gpu_ctx.renderFramesAdaptive(cams, o5, threshold=3e38)
    assert not masks.any() and same(frames, one)


# ---- the raw entry points ---------------------------------------------------------------------------------------------------


def host_bufs(n, width, height):
    return frame_and_mask(n * width * height, guard_bytes=GUARD)


# The messages every adaptive call shares (the library builds them in one place), whole: a cause listed here is compared
# with the whole message, any other cause as a part of it
WHOLE = {
    "threshold -1": "threshold -1: neither negative nor NaN",
    "threshold nan": "threshold nan: neither negative nor NaN",
    "null output": "null output",
    "null needs_aa": "null needs_aa: the device variant keeps the flags in the caller's buffer",
    "strip_world": "strip_world > 1: the rows above and below a strip belong to other ranks",
}


def addr(buf):
    if buf is None:
        return None
    return buf.ctypes.data if isinstance(buf, np.ndarray) else buf


def raw(ctx, cams, n, opts, thr, out, mask, poses=None, posed=False, device=False, tail=None):
    """one of the four entry points: cams / poses ctypes arrays or None, out / mask numpy arrays, device pointers or None;
    tail: the stop flag (host) or the stream (device)"""
    name = "c2rt_render_frames%s_adaptive%s" % ("_posed" if posed else "", "_device" if device else "")
    args = [ctx.handle, cams] + ([poses] if posed else []) + [n, C.byref(opts) if opts is not None else None, thr, addr(out), addr(mask), addr(tail)]
    return getattr(lib(), name)(*args)


def unpack(fbuf, mbuf, n, width, height):
    px = n * width * height
    return fbuf[:px * 12].view(np.float32).reshape(n, height, width, 3), mbuf[:px].reshape(n, height, width)


# ---- 7: counts and sizes ----------------------------------------------------------------------------------------------------


def test_one_frame_is_the_single_frame_call(gpu_ctx):
    scene = file_scene("lecture5.sdl", (67, 45))
    cams = orbit(scene, 2, 8.0)
    o1, o5 = opts_of(scene)
    gpu_ctx.uploadScene(scene.desc)
    f, m = gpu_ctx.renderFrameAdaptive(cams[1], o5)
    frames, masks = gpu_ctx.renderFramesAdaptive(cams[1:], o5)
    assert frames.shape == (1, 45, 67, 3) and same(frames[0], f) and same(masks[0], m) and m.any()


def test_no_frame_and_one_frame_too_many(gpu_ctx):
    scene = file_scene("lecture5.sdl", (24, 16))
    o1, o5 = opts_of(scene)
    gpu_ctx.uploadScene(scene.desc)
    cam = scene.beginFrame()
    arr = (_abi.CameraFrame * 257)(*([cam] * 257))
    parr = (_abi.ScenePose * 257)()          # both counts 0: frames of the scene as it is
    fbuf, mbuf = host_bufs(1, 24, 16)
    fdev, mdev = DeviceBytes(fbuf.nbytes), DeviceBytes(mbuf.nbytes)
    for posed in (False, True):
        for device in (False, True):
            out, mask = (fdev.ptr, mdev.ptr) if device else (fbuf, mbuf)
            assert raw(gpu_ctx, arr, 0, o5, THR, out, mask, parr, posed, device) == _abi.OK
            assert raw(gpu_ctx, None, 0, None, THR, None, None, None, posed, device) == _abi.OK      # nothing is read
            assert raw(gpu_ctx, arr, 257, o5, THR, out, mask, parr, posed, device) == _abi.ERR_LIMIT
            assert "257 frames" in last_error(gpu_ctx)
    assert hip_runtime().hipDeviceSynchronize() == 0
    assert untouched((fbuf, mbuf, fdev.get(), mdev.get()))
    fdev.free()
    mdev.free()
    frames, masks = gpu_ctx.renderFramesAdaptive([], o5)
    assert frames.shape == (0, 16, 24, 3) and masks.shape == (0, 16, 24)


def test_256_frames(gpu_ctx):
    """C2RT_MAX_BATCH_FRAMES frames of 24x16, lecture5, 1.4 degrees apart: a full turn"""
    scene = file_scene("lecture5.sdl", (24, 16))
    cams = orbit(scene, 256, 1.4)
    o1, o5 = opts_of(scene)
    gpu_ctx.uploadScene(scene.desc)
    one, five = gpu_ctx.renderFrames(cams, o1), gpu_ctx.renderFrames(cams, o5)
    want = [needs_aa(f, THR) for f in one]
    flagged = np.array([int(m.sum()) for m in want])
    print("256 frames: %d to %d flagged pixels of 384 per frame, %d frames without any" % (flagged.min(), flagged.max(), int((flagged == 0).sum())))
    assert flagged[0] > 0 and len({m.tobytes() for m in want}) > 128
    fbuf, mbuf = host_bufs(256, 24, 16)
    arr = (_abi.CameraFrame * 256)(*cams)
    assert raw(gpu_ctx, arr, 256, o5, THR, fbuf, mbuf) == _abi.OK, last_error(gpu_ctx)
    frames, masks = unpack(fbuf, mbuf, 256, 24, 16)
    assert_composition(frames, masks, one, five, want, "256 frames")
    assert untouched((fbuf[256 * 384 * 12:], mbuf[256 * 384:]))
    assert_single_frames(gpu_ctx, cams, o5, frames, masks, "256 frames")


@pytest.mark.parametrize("width,height", [(1, 1), (9, 1), (1, 9), (61, 47)])
def test_frame_sizes(gpu_ctx, width, height):
    """two cameras each; 9x1 and 1x9 have no flags at the reference's threshold, so two smaller ones as well: a
    neighbour that reached into the other frame would show in the first and last pixels' flags"""
    scene = file_scene("lecture5.sdl", (width, height))
    cams = orbit(scene, 2, 30.0)
    o1, o5 = opts_of(scene)
    gpu_ctx.uploadScene(scene.desc)
    one, five = gpu_ctx.renderFrames(cams, o1), gpu_ctx.renderFrames(cams, o5)
    arr = (_abi.CameraFrame * 2)(*cams)
    px = 2 * width * height
    for thr in (THR, 0.02, 0.0):
        want = [needs_aa(f, thr) for f in one]
        fbuf, mbuf = host_bufs(2, width, height)
        assert raw(gpu_ctx, arr, 2, o5, thr, fbuf, mbuf) == _abi.OK, last_error(gpu_ctx)
        frames, masks = unpack(fbuf, mbuf, 2, width, height)
        assert ((masks == 0) | (masks == 1)).all(), (width, height, thr)
        assert_composition(frames, masks, one, five, want, "%dx%d at %g" % (width, height, thr))
        assert untouched((fbuf[px * 12:], mbuf[px:])), (width, height, thr)
        assert_single_frames(gpu_ctx, cams, o5, frames, masks, "%dx%d at %g" % (width, height, thr), thr)
    if (width, height) != (1, 1):
        assert needs_aa(one[0], 0.0).any(), (width, height)


# ---- 8: statuses, before anything is touched --------------------------------------------------------------------------------


def test_statuses_leave_the_outputs_untouched(gpu_ctx):
    width, height, n = 40, 24, 3
    scene = file_scene("lecture5.sdl", (width, height))
    cams = orbit(scene, n, 8.0)
    o1, o5 = opts_of(scene)
    gpu_ctx.uploadScene(scene.desc)
    arr = (_abi.CameraFrame * n)(*cams)
    t = U.xf(("translate", 0, 90, 200))
    # (a ScenePose owns its arrays: the lists keep them alive behind the ctypes arrays' copies)
    good_poses = [c2.makePose({3: t}), c2.makePose(), c2.makePose(None, {0: dict(power=1.0)})]
    bad_pose = c2.makePose({9: t})
    good = (_abi.ScenePose * n)(*good_poses)
    fbuf, mbuf = host_bufs(n, width, height)
    fdev, mdev = DeviceBytes(fbuf.nbytes), DeviceBytes(mbuf.nbytes)

    def cams_with(**kw):
        return (_abi.CameraFrame * n)(cams[0], with_fields(cams[1], **kw), cams[2])

    def opts_with(**kw):
        return with_fields(o5, **kw)

    def refused(status, cause, cc=arr, oo=o5, thr=THR, poses=good, null_out=False, null_mask=False, host=True, plain=True):
        for posed in ((False, True) if plain else (True,)):
            for device in ((False, True) if host else (True,)):
                out, mask = (fdev.ptr, mdev.ptr) if device else (fbuf, mbuf)
                got = raw(gpu_ctx, cc, n, oo, thr, None if null_out else out, None if null_mask else mask, poses, posed, device)
                assert got == status, (cause, posed, device, got, last_error(gpu_ctx))
                assert last_error(gpu_ctx) == WHOLE[cause] if cause in WHOLE else cause in last_error(gpu_ctx), (cause, posed, device, last_error(gpu_ctx))
        assert hip_runtime().hipDeviceSynchronize() == 0
        assert untouched((fbuf, mbuf, fdev.get(), mdev.get())), cause

    refused(_abi.ERR_INVALID_ARG, "null cameras", cc=None)
    refused(_abi.ERR_INVALID_ARG, "null cameras", oo=None)
    refused(_abi.ERR_INVALID_ARG, "C2RT_TAPS_REF5", oo=opts_with(taps=_abi.TAPS_1))
    refused(_abi.ERR_INVALID_ARG, "threshold -1", thr=-1.0)
    refused(_abi.ERR_INVALID_ARG, "threshold nan", thr=float("nan"))
    refused(_abi.ERR_INVALID_ARG, "null output", null_out=True)
    refused(_abi.ERR_INVALID_ARG, "null needs_aa", null_mask=True, host=False)       # required in the device variants only
    refused(_abi.ERR_UNSUPPORTED, "camera 1 has depth of field", cc=cams_with(dof=1, num_samples=4))
    refused(_abi.ERR_UNSUPPORTED, "camera 1 is a stereo camera", cc=cams_with(stereo_separation=0.5))
    refused(_abi.ERR_UNSUPPORTED, "count_rays", oo=opts_with(count_rays=1))
    refused(_abi.ERR_UNSUPPORTED, "prepass_bucket", oo=opts_with(prepass_bucket=48))
    refused(_abi.ERR_UNSUPPORTED, "strip_world", oo=opts_with(strip_height=8, strip_rank=1, strip_world=2))
    # the order: a batch call's refusals, then this call's arguments, then strips, then the poses
    refused(_abi.ERR_UNSUPPORTED, "count_rays", oo=opts_with(count_rays=1, taps=_abi.TAPS_1), thr=-1.0)
    refused(_abi.ERR_INVALID_ARG, "threshold -1", oo=opts_with(strip_height=8, strip_rank=1, strip_world=2), thr=-1.0)
    bad = (_abi.ScenePose * n)(good_poses[0], good_poses[1], bad_pose)
    refused(_abi.ERR_UNSUPPORTED, "strip_world", oo=opts_with(strip_height=8, strip_rank=1, strip_world=2), poses=bad)
    refused(_abi.ERR_INVALID_ARG, "frame 2: pose: node_index[0] = 9 out of range", poses=bad, plain=False)
    assert last_error(gpu_ctx).startswith("frame 2: ")
    refused(_abi.ERR_INVALID_ARG, "null poses", poses=None, plain=False)
    # a stop request before the launches
    stop = np.ones(1, dtype=np.uint8)
    for posed in (False, True):
        assert raw(gpu_ctx, arr, n, o5, THR, fbuf, mbuf, good, posed, False, stop) == _abi.ERR_CANCELLED
        assert "stop requested" in last_error(gpu_ctx) and untouched((fbuf, mbuf))
    stop[0] = 0
    # afterwards the same context renders the batch, and nothing lands behind frame n - 1 or mask n - 1
    px = n * width * height
    one, five = gpu_ctx.renderFrames(cams, o1), gpu_ctx.renderFrames(cams, o5)
    want = [needs_aa(f, THR) for f in one]
    assert raw(gpu_ctx, arr, n, o5, THR, fbuf, mbuf, tail=stop) == _abi.OK, last_error(gpu_ctx)
    frames, masks = unpack(fbuf, mbuf, n, width, height)
    assert_composition(frames, masks, one, five, want, "after the refusals")
    assert untouched((fbuf[px * 12:], mbuf[px:]))
    assert raw(gpu_ctx, arr, n, o5, THR, fdev.ptr, mdev.ptr, device=True) == _abi.OK, last_error(gpu_ctx)
    assert hip_runtime().hipDeviceSynchronize() == 0
    assert fdev.get().tobytes() == fbuf.tobytes() and mdev.get().tobytes() == mbuf.tobytes()
    # the host variants without a mask
    for posed in (False, True):
        fbuf2, mbuf2 = host_bufs(n, width, height)
        none = (_abi.ScenePose * n)()        # both counts 0: frames of the scene as it is
        assert raw(gpu_ctx, arr, n, o5, THR, fbuf2, None, none, posed) == _abi.OK, last_error(gpu_ctx)
        assert fbuf2.tobytes() == fbuf.tobytes() and untouched((mbuf2,))
    # the posed variants into guarded buffers
    posed_one, posed_five = gpu_ctx.renderFramesPosed(cams, good, o1), gpu_ctx.renderFramesPosed(cams, good, o5)
    posed_want = [needs_aa(f, THR) for f in posed_one]
    fbuf3, mbuf3 = host_bufs(n, width, height)
    fdev3, mdev3 = DeviceBytes(fbuf3.nbytes), DeviceBytes(mbuf3.nbytes)
    assert raw(gpu_ctx, arr, n, o5, THR, fbuf3, mbuf3, good, True) == _abi.OK, last_error(gpu_ctx)
    frames, masks = unpack(fbuf3, mbuf3, n, width, height)
    assert_composition(frames, masks, posed_one, posed_five, posed_want, "posed, after the refusals")
    assert untouched((fbuf3[px * 12:], mbuf3[px:]))
    assert raw(gpu_ctx, arr, n, o5, THR, fdev3.ptr, mdev3.ptr, good, True, True) == _abi.OK, last_error(gpu_ctx)
    assert hip_runtime().hipDeviceSynchronize() == 0
    assert fdev3.get().tobytes() == fbuf3.tobytes() and mdev3.get().tobytes() == mbuf3.tobytes()
    for b in (fdev, mdev, fdev3, mdev3):
        b.free()


# ---- 9: streams -------------------------------------------------------------------------------------------------------------


def test_streams(gpu_ctx):
    """two batches behind one another on a stream of the caller's, no sync in between (the second overwrites the stream's
    tables as soon as the first's copy is ordered), a third on a second stream; one synchronise at the end"""
    width, height, n = 67, 45, 4
    scene = file_scene("lecture5.sdl", (width, height))
    cams = orbit(scene, n, 8.0)
    o1, o5 = opts_of(scene)
    gpu_ctx.uploadScene(scene.desc)
    poses = five_poses()[1:]
    want_a = gpu_ctx.renderFramesAdaptive(cams, o5)
    want_b = gpu_ctx.renderFramesAdaptive(cams[::-1], o5, threshold=0.02)
    want_c = gpu_ctx.renderFramesPosedAdaptive(cams, poses, o5)
    assert not same(want_a[1], want_b[1][::-1])
    hip = hip_runtime()
    s1, s2 = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s1)) == 0 and hip.hipStreamCreate(C.byref(s2)) == 0
    px = n * width * height
    bufs = [(DeviceBytes(px * 12 + GUARD), DeviceBytes(px + GUARD)) for _ in range(3)]
    gpu_ctx.renderFramesAdaptiveDevice(cams, o5, bufs[0][0].ptr.value, bufs[0][1].ptr.value, stream=s1.value)
    gpu_ctx.renderFramesAdaptiveDevice(cams[::-1], o5, bufs[1][0].ptr.value, bufs[1][1].ptr.value, threshold=0.02, stream=s1.value)
    gpu_ctx.renderFramesPosedAdaptiveDevice(cams, poses, o5, bufs[2][0].ptr.value, bufs[2][1].ptr.value, stream=s2.value)
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipStreamDestroy(s1) == 0 and hip.hipStreamDestroy(s2) == 0      # the library keeps no reference to them
    for (f, m), (wf, wm) in zip(bufs, (want_a, want_b, want_c)):
        assert holds(m.get(), wm) and holds(f.get(), wf)
        f.free()
        m.free()
    again = gpu_ctx.renderFramesAdaptive(cams, o5)
    assert same(again[0], want_a[0]) and same(again[1], want_a[1])


# ---- 10: the Python face ----------------------------------------------------------------------------------------------------


def test_python_face(gpu_ctx):
    scene = file_scene("lecture5.sdl", (32, 24))
    cams = orbit(scene, 3, 8.0)
    o1, o5 = opts_of(scene)
    gpu_ctx.uploadScene(scene.desc)
    frames, masks = gpu_ctx.renderFramesAdaptive(cams, o5)
    assert frames.shape == (3, 24, 32, 3) and frames.dtype == np.float32
    assert masks.shape == (3, 24, 32) and masks.dtype == np.uint8 and 0 < int(masks.sum()) < masks.size
    # a ctypes array of cameras, poses as ScenePose or as (nodes, lights) pairs
    none = [({}, None)] * 3
    pf, pm = gpu_ctx.renderFramesPosedAdaptive((_abi.CameraFrame * 3)(*cams), none, o5)
    assert same(pf, frames) and same(pm, masks)
    pf, pm = gpu_ctx.renderFramesPosedAdaptive(cams, [c2.makePose()] * 3, o5, threshold=THR, stop_flag=np.zeros(1, dtype=np.uint8))
    assert same(pf, frames) and same(pm, masks)
    with pytest.raises(ValueError):
        gpu_ctx.renderFramesPosedAdaptive(cams, none[:2], o5)
    with pytest.raises(ValueError):
        gpu_ctx.renderFramesPosedAdaptiveDevice(cams, none[:2], o5, 1, 1)
    for call, status in ((lambda: gpu_ctx.renderFramesAdaptive(cams, o1), _abi.ERR_INVALID_ARG),
                         (lambda: gpu_ctx.renderFramesAdaptive(cams, o5, threshold=-1.0), _abi.ERR_INVALID_ARG),
                         (lambda: gpu_ctx.renderFramesAdaptive(cams * 86, o5), _abi.ERR_LIMIT),
                         (lambda: gpu_ctx.renderFramesAdaptive(cams, o5, stop_flag=np.ones(1, dtype=np.uint8)), _abi.ERR_CANCELLED),
                         (lambda: gpu_ctx.renderFramesPosedAdaptive(cams, [({9: U.xf()}, None)] * 3, o5), _abi.ERR_INVALID_ARG),
                         (lambda: gpu_ctx.renderFramesAdaptiveDevice(cams, o5, 0, 0), _abi.ERR_INVALID_ARG),
                         (lambda: gpu_ctx.renderFramesPosedAdaptiveDevice(cams, none, o5, 0, 0), _abi.ERR_INVALID_ARG)):
        with pytest.raises(c2.C2rtError) as e:
            call()
        assert e.value.status == status, str(e.value)
    px = 3 * 24 * 32
    fdev, mdev = DeviceBytes(px * 12), DeviceBytes(px)
    gpu_ctx.renderFramesAdaptiveDevice(cams, o5, fdev.ptr.value, mdev.ptr.value)
    assert hip_runtime().hipDeviceSynchronize() == 0
    assert fdev.get().tobytes() == bits(frames).tobytes() and mdev.get().tobytes() == masks.tobytes()
    gpu_ctx.renderFramesPosedAdaptiveDevice(cams, five_poses()[:3], o5, fdev.ptr.value, mdev.ptr.value)
    assert hip_runtime().hipDeviceSynchronize() == 0
    pf, pm = gpu_ctx.renderFramesPosedAdaptive(cams, five_poses()[:3], o5)
    assert fdev.get().tobytes() == bits(pf).tobytes() and mdev.get().tobytes() == pm.tobytes()
    fdev.free()
    mdev.free()
