"""Adaptive anti-aliasing on the GPU (c2rt_render_frame_adaptive*): the mask against the typed numpy restatement of the
edge test (tests/aa_reference.py) applied to the context's own one-tap frame, flagged pixels against the context's
five-tap frame and unflagged pixels against its one-tap frame.  Every comparison is of bits.

No reference output pins the detection (the reference computes the flag and never reads it), so the mask's yardstick is
the numpy restatement; the pixels' yardsticks are the library's own frames.

Frame sizes: the issue's.  Checked on the CPU oracle's one-tap frames before the first GPU run: flagged shares 14 %,
14 %, 55 %, 63 % and 67 % for the five composition cases, and across them tiles with 1..16, with 17..63 and with 64
flagged pixels (lecture5 67x45: 23 / 10 / 0 tiles, csg_stress 96x72: 9 / 79 / 6, lecture4 160x120: 8 / 66 / 134), so no
size had to be changed.  The test asserts both on the GPU's own frames."""
import ctypes as C
import os

import numpy as np
import pytest

import chess2rt_amd as c2
from aa_reference import needs_aa, tile_counts
from chess2rt_amd import _abi
from golden_configs import SCENES
from query_test_util import DeviceBytes, frame_and_mask, hip_runtime, holds, last_error, lib, untouched, with_fields
from query_test_util import float_bits as bits

pytestmark = pytest.mark.gpu

GUARD = 64               # extra bytes behind the device outputs, extra elements behind the host outputs
COMPOSITION = [("lecture5.sdl", 67, 45), ("csg_corner.sdl", 96, 72), ("csg_stress.sdl", 96, 72), ("lecture4.sdl", 160, 120),
               ("lecture4-proc-texture.sdl", 61, 47)]
_cases = {}
_tile_classes = {}


def make_scene(scene_file, width, height):
    scene = c2.parseSceneFromFile(os.path.join(SCENES, scene_file))
    scene.setFrameSize(width, height)
    scene.setAA(False)
    scene.setDof(False)
    return scene, scene.beginFrame(), scene.renderOpts(taps=_abi.TAPS_REF5)


def frame_case(ctx, scene_file, width, height):
    """(scene, camera, five-tap options, one-tap frame, five-tap frame) of the file's camera, rendered once and shared
    (read-only); the scene is uploaded on return"""
    key = (scene_file, width, height)
    if key not in _cases:
        scene, cam, opts = make_scene(scene_file, width, height)
        ctx.uploadScene(scene.desc)
        one = ctx.renderFrame(cam, scene.renderOpts(taps=_abi.TAPS_1))
        five = ctx.renderFrame(cam, opts)
        one.setflags(write=False)
        five.setflags(write=False)
        _cases[key] = (scene, cam, opts, one, five)
    scene = _cases[key][0]
    ctx.uploadScene(scene.desc)
    return _cases[key]


def assert_composition(frame, mask, one, five, want_mask, what):
    assert mask.dtype == np.uint8 and mask.shape == want_mask.shape, what
    assert mask.tobytes() == want_mask.tobytes(), "%s: %d mask bytes differ from the numpy detection" % (what, int((mask != want_mask).sum()))
    m = want_mask == 1
    assert bits(frame)[m].tobytes() == bits(five)[m].tobytes(), "%s: flagged pixels differ from the five-tap frame" % (what,)
    assert bits(frame)[~m].tobytes() == bits(one)[~m].tobytes(), "%s: unflagged pixels differ from the one-tap frame" % (what,)


def raw_call(ctx, cam, opts, threshold, frame_buf, mask_buf, stop=None):
    return lib().c2rt_render_frame_adaptive(ctx.handle, C.byref(cam) if cam is not None else None, C.byref(opts) if opts is not None else None,
                                          threshold, frame_buf.ctypes.data if frame_buf is not None else None,
                                          mask_buf.ctypes.data if mask_buf is not None else None,
                                          stop.ctypes.data if stop is not None else None)


def raw_device_call(ctx, cam, opts, threshold, out_ptr, mask_ptr, stream=None):
    return lib().c2rt_render_frame_adaptive_device(ctx.handle, C.byref(cam), C.byref(opts), threshold, out_ptr, mask_ptr, stream)


# The messages every adaptive call shares (the library builds them in one place), whole: a cause listed here is compared
# with the whole message, any other cause as a part of it
WHOLE = {
    "threshold -1": "threshold -1: neither negative nor NaN",
    "threshold nan": "threshold nan: neither negative nor NaN",
    "null output": "null output",
    "null needs_aa": "null needs_aa: the device variant keeps the flags in the caller's buffer",
    "depth of field": "depth of field: the flags compare one ray per pixel, a lens has many",
    "stereo": "stereo: the flags compare one ray per pixel, a stereo camera has two",
    "count_rays": "count_rays: the refinement does not count rays",
    "prepass_bucket": "prepass_bucket: a preview's pixels share the sample of their block",
    "strip_world": "strip_world > 1: the rows above and below a strip belong to other ranks",
    "multi-device": "multi-device context: the rows above and below a strip are on other devices",
}


# ---- 1: composition ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("scene_file,width,height", COMPOSITION, ids=["%s-%dx%d" % (s[:-4], w, h) for s, w, h in COMPOSITION])
def test_composition(gpu_ctx, scene_file, width, height):
    scene, cam, opts, one, five = frame_case(gpu_ctx, scene_file, width, height)
    want_mask = needs_aa(one, _abi.AA_THRESHOLD_REF)
    share = float(want_mask.mean())
    k = tile_counts(want_mask)
    classes = (int(((k >= 1) & (k <= 16)).sum()), int(((k >= 17) & (k <= 63)).sum()), int((k == 64).sum()))
    _tile_classes[(scene_file, width, height)] = classes
    print("%s %dx%d: flagged share %.4f, tiles with 1..16 / 17..63 / 64 flags: %d / %d / %d" % ((scene_file, width, height, share) + classes))
    assert 0.02 <= share <= 0.90, (scene_file, share)
    assert bits(one).tobytes() != bits(five).tobytes()
    frame, mask = gpu_ctx.renderFrameAdaptive(cam, opts)
    assert frame.shape == (height, width, 3) and frame.dtype == np.float32
    assert_composition(frame, mask, one, five, want_mask, scene_file)
    # the refinement did something: some flagged pixel's five-tap value differs from its one-tap value
    m = want_mask == 1
    assert (bits(five)[m] != bits(one)[m]).any(), scene_file


def test_the_composition_cases_cover_one_round_several_rounds_and_a_full_tile(gpu_ctx):
    """1 <= k <= 16 flagged pixels is one round of the packed refinement, 17 <= k <= 63 several, k = 64 a full tile"""
    total = [0, 0, 0]
    for scene_file, width, height in COMPOSITION:
        key = (scene_file, width, height)
        if key not in _tile_classes:        # run on its own: the masks of the shared one-tap frames
            one = frame_case(gpu_ctx, scene_file, width, height)[3]
            k = tile_counts(needs_aa(one, _abi.AA_THRESHOLD_REF))
            _tile_classes[key] = (int(((k >= 1) & (k <= 16)).sum()), int(((k >= 17) & (k <= 63)).sum()), int((k == 64).sum()))
        total = [a + b for a, b in zip(total, _tile_classes[key])]
    assert all(t > 0 for t in total), total


# ---- 2: nothing flagged --------------------------------------------------------------------------------------------------


def test_nothing_flagged(gpu_ctx):
    scene, cam, opts, one, five = frame_case(gpu_ctx, "zaphod.sdl", 129, 86)
    assert not needs_aa(one, _abi.AA_THRESHOLD_REF).any()
    frame, mask = gpu_ctx.renderFrameAdaptive(cam, opts)
    assert not mask.any()
    assert bits(frame).tobytes() == bits(one).tobytes()


# ---- 3: threshold ----------------------------------------------------------------------------------------------------------


def test_threshold(gpu_ctx):
    scene, cam, opts, one, five = frame_case(gpu_ctx, "lecture5.sdl", 67, 45)
    frame, none = gpu_ctx.renderFrameAdaptive(cam, opts, threshold=3e38)
    assert not none.any() and bits(frame).tobytes() == bits(one).tobytes()
    masks = {}
    for thr in (0.0, 0.02, _abi.AA_THRESHOLD_REF):
        frame, masks[thr] = gpu_ctx.renderFrameAdaptive(cam, opts, threshold=thr)
        assert_composition(frame, masks[thr], one, five, needs_aa(one, thr), "threshold %g" % thr)
    # nested: a larger threshold flags a subset
    assert (masks[0.02] <= masks[0.0]).all() and (none <= masks[0.02]).all()
    assert (masks[_abi.AA_THRESHOLD_REF] <= masks[0.02]).all()
    assert 0 < int(masks[0.02].sum()) < int(masks[0.0].sum())
    fbuf, mbuf = frame_and_mask(67 * 45, guard_elems=GUARD)
    for bad in (-1.0, float("nan")):
        assert raw_call(gpu_ctx, cam, opts, bad, fbuf, mbuf) == _abi.ERR_INVALID_ARG, bad
        assert "threshold" in last_error(gpu_ctx)
        assert untouched((fbuf, mbuf)), bad


# ---- 4: edges ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("width,height", [(1, 1), (9, 1), (1, 9), (61, 47)])
def test_edges(gpu_ctx, width, height):
    scene, cam, opts, one, five = frame_case(gpu_ctx, "lecture5.sdl", width, height)
    n = width * height
    # the reference's threshold, and two at which the small frames have flags as well (9x1 and 1x9 have none at 0.1)
    for thr in (_abi.AA_THRESHOLD_REF, 0.02, 0.0):
        want_mask = needs_aa(one, thr)
        fbuf, mbuf = frame_and_mask(width * height, guard_elems=GUARD)
        assert raw_call(gpu_ctx, cam, opts, thr, fbuf, mbuf) == _abi.OK, last_error(gpu_ctx)
        mask = mbuf[:n].reshape(height, width)
        assert ((mask == 0) | (mask == 1)).all(), (width, height, thr)
        frame = fbuf[:n * 12].view(np.float32).reshape(height, width, 3)
        assert_composition(frame, mask, one, five, want_mask, "%dx%d at %g" % (width, height, thr))
        assert untouched((fbuf[n * 12:], mbuf[n:])), (width, height, thr)
    if (width, height) != (1, 1):
        assert needs_aa(one, 0.0).any(), (width, height)


# ---- 5: statuses, before anything is touched ------------------------------------------------------------------------------


def test_statuses_leave_the_outputs_untouched(gpu_ctx):
    width, height = 61, 47
    scene, cam, opts, one, five = frame_case(gpu_ctx, "lecture5.sdl", width, height)
    n = width * height

    def copy_cam(**kw):
        return with_fields(cam, **kw)

    def copy_opts(**kw):
        return with_fields(opts, **kw)

    fdev, mdev = DeviceBytes(n * 12 + GUARD), DeviceBytes(n + GUARD)
    fbuf, mbuf = frame_and_mask(width * height, guard_elems=GUARD)
    thr = _abi.AA_THRESHOLD_REF

    def refused(ctx, c, o, t, status, cause, host_frame=fbuf, dev_frame=fdev.ptr, dev_mask=mdev.ptr, host=True):
        if host:
            assert raw_call(ctx, c, o, t, host_frame, mbuf) == status, cause
            assert last_error(ctx) == WHOLE[cause] if cause in WHOLE else cause in last_error(ctx), (cause, last_error(ctx))
        assert raw_device_call(ctx, c, o, t, dev_frame, dev_mask) == status, cause
        assert last_error(ctx) == WHOLE[cause] if cause in WHOLE else cause in last_error(ctx), (cause, last_error(ctx))
        assert hip_runtime().hipDeviceSynchronize() == 0
        assert untouched((fbuf, mbuf, fdev.get(), mdev.get())), cause

    # a frame call's own statuses come first: a bad size wins over a bad tap mode for this call
    refused(gpu_ctx, cam, copy_opts(width=0, taps=_abi.TAPS_1), thr, _abi.ERR_INVALID_ARG, "")
    for taps in (_abi.TAPS_1, _abi.TAPS_4):
        refused(gpu_ctx, cam, copy_opts(taps=taps), thr, _abi.ERR_INVALID_ARG, "C2RT_TAPS_REF5")
    refused(gpu_ctx, cam, opts, -1.0, _abi.ERR_INVALID_ARG, "threshold -1")
    refused(gpu_ctx, cam, opts, float("nan"), _abi.ERR_INVALID_ARG, "threshold nan")
    refused(gpu_ctx, cam, opts, thr, _abi.ERR_INVALID_ARG, "null output", host_frame=None, dev_frame=None)
    # the mask is required in the device variant only
    refused(gpu_ctx, cam, opts, thr, _abi.ERR_INVALID_ARG, "null needs_aa", dev_mask=None, host=False)
    # an invalid argument is reported before an unsupported mode
    refused(gpu_ctx, copy_cam(dof=1, num_samples=4), opts, -1.0, _abi.ERR_INVALID_ARG, "threshold -1")
    for c, o, cause in [(copy_cam(dof=1, num_samples=4), opts, "depth of field"),
                        (copy_cam(stereo_separation=0.5), opts, "stereo"),
                        (cam, copy_opts(count_rays=1), "count_rays"),
                        (cam, copy_opts(prepass_bucket=48), "prepass_bucket"),
                        (cam, copy_opts(strip_height=8, strip_rank=1, strip_world=2), "strip_world")]:
        refused(gpu_ctx, c, o, thr, _abi.ERR_UNSUPPORTED, cause)
    two = c2.Context(devices=[0, 0])
    try:
        two.uploadScene(scene.desc)
        refused(two, cam, opts, thr, _abi.ERR_UNSUPPORTED, "multi-device")
    finally:
        two.close()
    fresh = c2.Context(0)
    try:
        refused(fresh, cam, opts, thr, _abi.ERR_NO_SCENE, "no scene")
    finally:
        fresh.close()
    # a stop request before the launches
    stop = np.ones(1, dtype=np.uint8)
    assert raw_call(gpu_ctx, cam, opts, thr, fbuf, mbuf, stop) == _abi.ERR_CANCELLED
    assert untouched((fbuf, mbuf))
    # afterwards the same context renders a correct adaptive frame, with and without the (nullable) host mask
    stop[0] = 0
    assert raw_call(gpu_ctx, cam, opts, thr, fbuf, mbuf, stop) == _abi.OK, last_error(gpu_ctx)
    want_mask = needs_aa(one, thr)
    frame = fbuf[:n * 12].view(np.float32).reshape(height, width, 3)
    assert_composition(frame, mbuf[:n].reshape(height, width), one, five, want_mask, "after the refusals")
    fbuf2, mbuf2 = frame_and_mask(width * height, guard_elems=GUARD)
    assert raw_call(gpu_ctx, cam, opts, thr, fbuf2, None) == _abi.OK, last_error(gpu_ctx)
    assert fbuf2.tobytes() == fbuf.tobytes() and untouched((mbuf2,))
    fdev.free()
    mdev.free()


# ---- 6: streams ---------------------------------------------------------------------------------------------------------------


def test_streams(gpu_ctx):
    width, height = 96, 72
    scene, cam, opts, one, five = frame_case(gpu_ctx, "csg_stress.sdl", width, height)
    n = width * height
    want_frame, want_mask = gpu_ctx.renderFrameAdaptive(cam, opts)
    want_frame2, want_mask2 = gpu_ctx.renderFrameAdaptive(cam, opts, threshold=0.02)
    assert want_mask.tobytes() != want_mask2.tobytes()
    # a stream of the caller's own
    hip = hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    f1, m1, f2, m2 = DeviceBytes(n * 12 + GUARD), DeviceBytes(n + GUARD), DeviceBytes(n * 12 + GUARD), DeviceBytes(n + GUARD)
    plain = DeviceBytes(n * 12 + GUARD)
    # three calls behind one another on that stream, no sync in between
    gpu_ctx.renderFrameAdaptiveDevice(cam, opts, f1.ptr.value, m1.ptr.value, stream=stream.value)
    gpu_ctx.renderFrameAdaptiveDevice(cam, opts, f2.ptr.value, m2.ptr.value, threshold=0.02, stream=stream.value)
    gpu_ctx.renderFrameDevice(cam, opts, plain.ptr.value, stream.value)
    assert hip.hipStreamSynchronize(stream) == 0
    assert hip.hipStreamDestroy(stream) == 0          # the library keeps no reference to it
    for f, m, wf, wm in ((f1, m1, want_frame, want_mask), (f2, m2, want_frame2, want_mask2)):
        assert holds(m.get(), wm) and holds(f.get(), wf)
    assert holds(plain.get(), five)
    for b in (f1, m1, f2, m2, plain):
        b.free()
    frame, mask = gpu_ctx.renderFrameAdaptive(cam, opts)
    assert mask.tobytes() == want_mask.tobytes() and bits(frame).tobytes() == bits(want_frame).tobytes()


# ---- 7: host mirror and Python face --------------------------------------------------------------------------------------------


def test_host_mirror_and_python_face(gpu_ctx):
    scene, cam, opts = make_scene("lecture5.sdl", 32, 24)
    gpu_ctx.uploadScene(scene.desc)
    want_frame, want_mask = gpu_ctx.renderFrameAdaptive(cam, opts)
    assert want_frame.shape == (24, 32, 3) and want_frame.dtype == np.float32
    assert want_mask.shape == (24, 32) and want_mask.dtype == np.uint8 and 0 < int(want_mask.sum()) < 24 * 32
    # the scene's AA setting does not matter to the mirror: it always refines to five taps
    for aa in (False, True):
        scene.setAA(aa)
        frame, mask = c2.Renderer(scene, gpu_ctx).renderRTAdaptive()
        assert mask.tobytes() == want_mask.tobytes() and mask.shape == (24, 32)
        assert bits(frame).tobytes() == bits(want_frame).tobytes() and frame.shape == (24, 32, 3)
    dof = c2.parseSceneFromFile(os.path.join(SCENES, "zaphod.sdl"))      # as shipped: depth of field
    dof.setFrameSize(32, 24)
    assert dof.camera.dof
    with pytest.raises(c2.C2rtError) as e:
        c2.Renderer(dof, gpu_ctx).renderRTAdaptive()
    assert e.value.status == _abi.ERR_UNSUPPORTED and "depth of field" in str(e.value)
