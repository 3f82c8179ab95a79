"""Sample tables on the GPU (c2rt_render_frame_taps*, c2rt_render_frame_adaptive_taps*).  Every comparison is of bits and every
expected value comes from an entry point the suite already holds to the oracle — the context's own frames, hit planes, ray
query and adaptive frames — or from fp32 additions and one division in numpy.

Tables (tests/sample_taps_cases.py): REF5 the reference's five taps, GRID16 = tap_grid(4), ODD7 seven taps of which three
leave the pixel, SHIFT2 two taps neither of which is the corner.  The adaptive cases' flagged shares and tile classes are
asserted on the oracle in tests/test_sample_taps_abi.py."""
import ctypes as C
import os

import numpy as np
import pytest

import camera_reference as cr
import camera_scenes as cs
import chess2rt_amd as c2
import sample_taps_cases as tc
import scene_update_util as U
from aa_reference import needs_aa, tile_counts
from chess2rt_amd import _abi
from chess2rt_amd.api import _tap_table
from golden_configs import SCENES
from query_test_util import DeviceBytes, frame_and_mask, hip_runtime, holds, last_error, lib, same, untouched, with_fields
from query_test_util import float_bits as bits

pytestmark = pytest.mark.gpu
needs_x87 = pytest.mark.skipif(not cr.x87_available(), reason="np.longdouble is not the x87 80-bit format: radians cannot be restated")

GUARD = 64               # extra bytes behind the device outputs, extra elements behind the host outputs
F = np.float32
_cases = {}


# The messages every adaptive call shares, c2rt_render_frame_adaptive_taps* among them (the library builds them in one place), whole: a cause listed here is compared
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


def golden_case(ctx, scene_file, width, height):
    """(scene, camera, one-tap options, one-tap frame) of the file's camera, rendered once and shared (read-only); the scene
    is uploaded on return"""
    key = (scene_file, width, height)
    if key not in _cases:
        scene, cam, opts = tc.make_scene(scene_file, width, height)
        ctx.uploadScene(scene.desc)
        one = ctx.renderFrame(cam, opts)
        one.setflags(write=False)
        _cases[key] = (scene, cam, opts, one)
    ctx.uploadScene(_cases[key][0].desc)
    return _cases[key]


def composed(ctx, cam, width, height, table, rows=None):
    """The header's definition through the context's own ray query: for every tap the reference's screen ray through
    (x + dx, y + dy) of every pixel, traced by traceRays; the sum in tap order and the division in fp32."""
    frame = cs.from_abi(cam)
    ys = np.arange(height) if rows is None else np.asarray(rows)
    yy, xx = np.meshgrid(ys.astype(np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    accum = None
    for dx, dy in table:
        o, d = cr.screen_ray(frame, xx.ravel() + np.float64(dx), yy.ravel() + np.float64(dy))
        _, c = ctx.traceRays(np.ascontiguousarray(np.hstack([o, d])), hits=False)
        assert c.dtype == np.float32
        accum = c if accum is None else accum + c
        assert accum.dtype == np.float32
    if len(table) > 1:
        accum = accum / F(len(table))
    assert accum.dtype == np.float32
    return accum.reshape(len(ys), width, 3)


# ---- 1: equalities with the existing frames -------------------------------------------------------------------------------

REF5_GOLDEN = [("lecture5.sdl", 67, 45), ("csg_corner.sdl", 96, 72), ("csg_stress.sdl", 96, 72), ("lecture4-proc-texture.sdl", 61, 47)]


@pytest.mark.parametrize("scene_file,width,height", REF5_GOLDEN, ids=["%s-%dx%d" % (s[:-4], w, h) for s, w, h in REF5_GOLDEN])
def test_the_references_taps_give_the_five_tap_frame(gpu_ctx, scene_file, width, height):
    scene, cam, opts, one = golden_case(gpu_ctx, scene_file, width, height)
    five = gpu_ctx.renderFrame(cam, scene.renderOpts(taps=_abi.TAPS_REF5))
    got = gpu_ctx.renderFrameTaps(cam, opts, tc.REF5)
    assert got.shape == (height, width, 3) and got.dtype == np.float32
    assert same(got, five), "%d floats differ" % int((bits(got) != bits(five)).sum())
    assert not same(five, one)
    # opts.taps is ignored, a TapTable is taken as it is
    assert same(gpu_ctx.renderFrameTaps(cam, scene.renderOpts(taps=_abi.TAPS_4), _tap_table(tc.REF5)), five)


@needs_x87
@pytest.mark.parametrize("name,mode,table", [("rolled_textured", "taps5", tc.REF5), ("tall", "taps5", tc.REF5), ("rolled", "taps4", tc.REF5[:4])],
                         ids=["rolled_textured-ref5", "tall-ref5", "rolled-first4"])
def test_rolled_cameras_ground_path_and_the_four_tap_mode(gpu_ctx, name, mode, table):
    """rolled_textured: the frame kernel takes its ground path there; tall: 19x53; rolled: REF5[:4] is C2RT_TAPS_4"""
    c = cs.case(name)
    m = c.modes[mode]
    gpu_ctx.uploadScene(c.desc)
    want = gpu_ctx.renderFrame(m.cam, m.opts)
    got = gpu_ctx.renderFrameTaps(m.cam, m.opts, table)
    assert same(got, want), (name, int((bits(got) != bits(want)).sum()))


@pytest.mark.parametrize("width,height", [(1, 1), (9, 1), (1, 9), (61, 47)])
def test_the_corner_alone_is_the_one_tap_frame_and_the_hit_planes_rgb(gpu_ctx, width, height):
    scene, cam, opts, one = golden_case(gpu_ctx, "lecture5.sdl", width, height)
    got = gpu_ctx.renderFrameTaps(cam, opts, [(0.0, 0.0)])
    assert same(got, one)
    assert same(got, gpu_ctx.renderHits(cam, opts, planes=("rgb",))["rgb"])


# ---- 2: composition, for tables no frame kernel has -----------------------------------------------------------------------


@pytest.mark.parametrize("scene_file,width,height", tc.ADAPTIVE, ids=tc.ADAPTIVE_IDS)
@pytest.mark.parametrize("table", [tc.ODD7, tc.SHIFT2, tc.GRID16], ids=["odd7", "shift2", "grid16"])
def test_a_frame_is_the_composition_of_ray_queries(gpu_ctx, scene_file, width, height, table):
    scene, cam, opts, one = golden_case(gpu_ctx, scene_file, width, height)
    want = composed(gpu_ctx, cam, width, height, table)
    got = gpu_ctx.renderFrameTaps(cam, opts, table)
    assert same(got, want), "%d floats differ" % int((bits(got) != bits(want)).sum())
    assert not same(got, one)


@needs_x87
def test_composition_on_a_width_whose_reciprocal_is_inexact(gpu_ctx):
    c = cs.case("wide")
    m = c.modes["taps1"]
    gpu_ctx.uploadScene(c.desc)
    want = composed(gpu_ctx, m.cam, c.W, c.H, tc.SHIFT2)
    got = gpu_ctx.renderFrameTaps(m.cam, m.opts, tc.SHIFT2)
    assert got.shape == (cs.WIDE_H, cs.WIDE_W, 3)
    assert same(got, want), int((bits(got) != bits(want)).sum())


# ---- 3: strips -------------------------------------------------------------------------------------------------------------


def test_strips_give_the_rows_of_the_whole_frame(gpu_ctx):
    width, height, sh, world = 24, 23, 5, 3
    scene, cam, opts, one = golden_case(gpu_ctx, "lecture5.sdl", width, height)
    whole = gpu_ctx.renderFrameTaps(cam, opts, tc.ODD7)
    seen = []
    for rank in range(world):
        o = scene.renderOpts(taps=_abi.TAPS_1, strip_height=sh, strip_world=world, strip_rank=rank)
        rows = [y for y in range(height) if (y // sh) % world == rank]
        assert gpu_ctx.localRows(o) == len(rows)
        got = gpu_ctx.renderFrameTaps(cam, o, tc.ODD7)
        assert got.shape == (len(rows), width, 3)
        assert same(got, np.ascontiguousarray(whole[rows])), rank
        seen += rows
    assert sorted(seen) == list(range(height))


# ---- 4, 5: host chunks, the device variant on a stream of its own ---------------------------------------------------------------


def test_host_chunks_equal_one_device_launch(gpu_ctx):
    width, height = 4099, 65
    n = width * height
    assert n > 1 << 18                                       # more than one chunk of whole rows
    scene, cam, opts = tc.make_scene("lecture5.sdl", width, height)
    gpu_ctx.uploadScene(scene.desc)
    host = gpu_ctx.renderFrameTaps(cam, opts, tc.SHIFT2)
    dev = DeviceBytes(n * 12 + GUARD)
    try:
        gpu_ctx.renderFrameTapsDevice(cam, opts, tc.SHIFT2, dev.ptr.value)
        assert dev.hip.hipDeviceSynchronize() == 0
        got = dev.get()
    finally:
        dev.free()
    assert holds(got, host)
    # the last rows, which the second chunk holds, are not the first rows again
    assert not same(host[-1], host[0])


def test_device_variant_on_a_stream_of_its_own(gpu_ctx):
    width, height = 96, 72
    n = width * height
    scene, cam, opts, one = golden_case(gpu_ctx, "csg_stress.sdl", width, height)
    want = gpu_ctx.renderFrameTaps(cam, opts, tc.GRID16)
    hip = hip_runtime()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    plain, out = DeviceBytes(n * 12 + GUARD), DeviceBytes(n * 12 + GUARD)
    try:
        # behind a frame on the same stream, no sync in between
        gpu_ctx.renderFrameDevice(cam, opts, plain.ptr.value, stream.value)
        gpu_ctx.renderFrameTapsDevice(cam, opts, tc.GRID16, out.ptr.value, stream=stream.value)
        assert hip.hipStreamSynchronize(stream) == 0
        assert hip.hipStreamDestroy(stream) == 0             # the library keeps no reference to it
        got, first = out.get(), plain.get()
    finally:
        plain.free()
        out.free()
    assert holds(got, want)
    assert holds(first, one)
    assert same(gpu_ctx.renderFrameTaps(cam, opts, tc.GRID16), want)


# ---- 6: adaptive -----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("scene_file,width,height", tc.ADAPTIVE, ids=tc.ADAPTIVE_IDS)
def test_adaptive_with_the_references_taps_is_the_adaptive_frame(gpu_ctx, scene_file, width, height):
    scene, cam, opts, one = golden_case(gpu_ctx, scene_file, width, height)
    want_frame, want_mask = gpu_ctx.renderFrameAdaptive(cam, scene.renderOpts(taps=_abi.TAPS_REF5))
    frame, mask = gpu_ctx.renderFrameAdaptiveTaps(cam, opts, tc.REF5)
    assert mask.dtype == np.uint8 and mask.tobytes() == want_mask.tobytes()
    assert same(frame, want_frame), int((bits(frame) != bits(want_frame)).sum())
    assert 0 < int(mask.sum()) < mask.size


@pytest.mark.parametrize("scene_file,width,height", tc.ADAPTIVE, ids=tc.ADAPTIVE_IDS)
@pytest.mark.parametrize("table", [tc.ODD7, tc.GRID16], ids=["odd7", "grid16"])
def test_adaptive_refines_the_flagged_pixels_to_the_whole_frames_bits(gpu_ctx, scene_file, width, height, table):
    scene, cam, opts, one = golden_case(gpu_ctx, scene_file, width, height)
    want_mask = needs_aa(one, _abi.AA_THRESHOLD_REF)
    k = tile_counts(want_mask)
    share = float(want_mask.mean())
    print("%s %dx%d: flagged share %.4f, tiles with 1..4 / 5.. flags: %d / %d" % (scene_file, width, height, share, int(((k >= 1) & (k <= 4)).sum()), int((k >= 5).sum())))
    assert 0.02 <= share <= 0.90
    full = gpu_ctx.renderFrameTaps(cam, opts, table)
    frame, mask = gpu_ctx.renderFrameAdaptiveTaps(cam, opts, table)
    assert frame.shape == (height, width, 3) and frame.dtype == np.float32 and mask.shape == (height, width) and mask.dtype == np.uint8
    assert mask.tobytes() == want_mask.tobytes(), "%d mask bytes differ from the numpy detection" % int((mask != want_mask).sum())
    m = want_mask == 1
    assert bits(frame)[m].tobytes() == bits(full)[m].tobytes(), "%d flagged floats differ from the whole frame's" % int((bits(frame)[m] != bits(full)[m]).sum())
    assert bits(frame)[~m].tobytes() == bits(one)[~m].tobytes(), "unflagged pixels differ from the one-tap frame"
    assert (bits(full)[m] != bits(one)[m]).any()


@pytest.mark.parametrize("table", [tc.PAIR2, tc.GRID9, tc.TEN], ids=["pair2", "grid9", "ten"])
def test_adaptive_around_the_pass_size(gpu_ctx, table):
    """1, 8 and 9 extra taps: the refinement kernel holds at most 8 samples per pixel and goes in passes beyond"""
    scene_file, width, height = tc.ADAPTIVE[0]
    scene, cam, opts, one = golden_case(gpu_ctx, scene_file, width, height)
    want_mask = needs_aa(one, _abi.AA_THRESHOLD_REF)
    full = gpu_ctx.renderFrameTaps(cam, opts, table)
    assert same(full, composed(gpu_ctx, cam, width, height, table))
    frame, mask = gpu_ctx.renderFrameAdaptiveTaps(cam, opts, table)
    assert mask.tobytes() == want_mask.tobytes()
    m = want_mask == 1
    assert bits(frame)[m].tobytes() == bits(full)[m].tobytes(), "%d flagged floats differ from the whole frame's" % int((bits(frame)[m] != bits(full)[m]).sum())
    assert bits(frame)[~m].tobytes() == bits(one)[~m].tobytes()
    assert (bits(full)[m] != bits(one)[m]).any()


def test_adaptive_thresholds_everything_in_a_tile_and_nothing(gpu_ctx):
    scene_file, width, height = tc.FULL_TILES
    scene, cam, opts, one = golden_case(gpu_ctx, scene_file, width, height)
    full = gpu_ctx.renderFrameTaps(cam, opts, tc.GRID16)
    # threshold 0: tiles flag in full — 960 items, 15 full rounds of the packed refinement per full tile (8 + 7, by pass)
    want_mask = needs_aa(one, 0.0)
    assert (tile_counts(want_mask) == 64).any()
    frame, mask = gpu_ctx.renderFrameAdaptiveTaps(cam, opts, tc.GRID16, threshold=0.0)
    assert mask.tobytes() == want_mask.tobytes()
    m = want_mask == 1
    assert bits(frame)[m].tobytes() == bits(full)[m].tobytes() and bits(frame)[~m].tobytes() == bits(one)[~m].tobytes()
    # threshold 3e38: nothing is flagged
    frame, mask = gpu_ctx.renderFrameAdaptiveTaps(cam, opts, tc.GRID16, threshold=3e38)
    assert not mask.any() and same(frame, one)


# ---- 7: after updateScene ---------------------------------------------------------------------------------------------------------


def test_both_calls_see_the_posed_scene(gpu_ctx):
    scene, cam, opts, one = golden_case(gpu_ctx, "lecture5.sdl", 67, 45)
    before = gpu_ctx.renderFrameTaps(cam, opts, tc.ODD7)
    move = {3: U.xf(("translate", 60, 15, 200))}
    try:
        gpu_ctx.updateScene(move)
        posed = gpu_ctx.renderFrameTaps(cam, opts, tc.ODD7)
        posed_frame, posed_mask = gpu_ctx.renderFrameAdaptiveTaps(cam, opts, tc.ODD7)
        fresh = U.Desc(scene.desc).patched(nodes=move)
        gpu_ctx.uploadScene(fresh.d)
        assert same(posed, gpu_ctx.renderFrameTaps(cam, opts, tc.ODD7))
        want_frame, want_mask = gpu_ctx.renderFrameAdaptiveTaps(cam, opts, tc.ODD7)
        assert posed_mask.tobytes() == want_mask.tobytes() and same(posed_frame, want_frame)
        assert not same(posed, before)
    finally:
        gpu_ctx.uploadScene(scene.desc)


# ---- 8: statuses, before anything is touched ----------------------------------------------------------------------------------------


def table_of(taps, **kw):
    t = _abi.TapTable.from_buffer_copy(_tap_table(taps))
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def with_offset(taps, s, axis, value):
    t = table_of(taps)
    t.offset[s][axis] = value
    return t


def test_statuses_leave_the_outputs_untouched(gpu_ctx):
    width, height = 61, 47
    n = width * height
    scene, cam, opts, one = golden_case(gpu_ctx, "lecture5.sdl", width, height)
    L = lib()
    thr = _abi.AA_THRESHOLD_REF
    good = table_of(tc.ODD7)

    def copy_cam(**kw):
        return with_fields(cam, **kw)

    def copy_opts(**kw):
        return with_fields(opts, **kw)

    def ref(x):
        return C.byref(x) if x is not None else None

    fdev, mdev = DeviceBytes(n * 12 + GUARD), DeviceBytes(n + GUARD)
    fbuf, mbuf = frame_and_mask(n, guard_elems=GUARD)

    def whole_refused(ctx, c, o, t, status, cause, out=True):
        for st in (L.c2rt_render_frame_taps(ctx.handle, ref(c), ref(o), ref(t), fbuf.ctypes.data if out else None),
                   L.c2rt_render_frame_taps_device(ctx.handle, ref(c), ref(o), ref(t), fdev.ptr if out else None, None)):
            assert st == status, (cause, st, last_error(ctx))
            assert cause in last_error(ctx), (cause, last_error(ctx))
        assert hip_runtime().hipDeviceSynchronize() == 0
        assert untouched((fbuf, fdev.get())), cause

    def adaptive_refused(ctx, c, o, t, threshold, status, cause, out=True, dev_mask=True, host=True):
        calls = []
        if host:
            calls.append(L.c2rt_render_frame_adaptive_taps(ctx.handle, ref(c), ref(o), ref(t), threshold, fbuf.ctypes.data if out else None, mbuf.ctypes.data, None))
        calls.append(L.c2rt_render_frame_adaptive_taps_device(ctx.handle, ref(c), ref(o), ref(t), threshold, fdev.ptr if out else None,
                                                              mdev.ptr if dev_mask else None, None))
        for st in calls:
            assert st == status, (cause, st, last_error(ctx))
            assert last_error(ctx) == WHOLE[cause] if cause in WHOLE else cause in last_error(ctx), (cause, last_error(ctx))
        assert hip_runtime().hipDeviceSynchronize() == 0
        assert untouched((fbuf, mbuf, fdev.get(), mdev.get())), cause

    def both_refused(ctx, c, o, t, status, cause):
        whole_refused(ctx, c, o, t, status, cause)
        adaptive_refused(ctx, c, o, t, thr, status, cause)

    lens, stereo = copy_cam(dof=1, num_samples=4), copy_cam(stereo_separation=0.5)
    try:
        # a frame call's own statuses come first, in c2rt_render_hits' order
        both_refused(gpu_ctx, None, opts, good, _abi.ERR_INVALID_ARG, "null camera or options")
        both_refused(gpu_ctx, cam, None, good, _abi.ERR_INVALID_ARG, "null camera or options")
        both_refused(gpu_ctx, cam, copy_opts(width=0), None, _abi.ERR_INVALID_ARG, "bad frame size")
        both_refused(gpu_ctx, cam, copy_opts(taps=3), None, _abi.ERR_INVALID_ARG, "bad tap mode")   # opts.taps: ignored, but a mode
        both_refused(gpu_ctx, cam, copy_opts(strip_rank=2, strip_world=2), None, _abi.ERR_INVALID_ARG, "strip_rank")
        fresh = c2.Context(0)
        try:
            both_refused(fresh, cam, opts, None, _abi.ERR_NO_SCENE, "no scene")
        finally:
            fresh.close()
        # then the table's, in this order
        both_refused(gpu_ctx, cam, opts, None, _abi.ERR_INVALID_ARG, "null taps")
        both_refused(gpu_ctx, cam, opts, table_of(tc.ODD7, n=0, reserved=1), _abi.ERR_INVALID_ARG, "n is 0")
        both_refused(gpu_ctx, cam, opts, table_of(tc.GRID16, n=17, reserved=1), _abi.ERR_LIMIT, "at most 16")
        both_refused(gpu_ctx, cam, opts, _tap_table([(0.0, 0.0)] * 17), _abi.ERR_LIMIT, "at most 16")
        both_refused(gpu_ctx, cam, opts, with_offset(table_of(tc.ODD7, reserved=1), 3, 0, float("nan")), _abi.ERR_INVALID_ARG, "reserved")
        both_refused(gpu_ctx, cam, opts, with_offset(tc.ODD7, 3, 0, float("nan")), _abi.ERR_INVALID_ARG, "tap 3")
        both_refused(gpu_ctx, cam, opts, with_offset(tc.ODD7, 6, 1, float("-inf")), _abi.ERR_INVALID_ARG, "tap 6")
        # then a null output, then the unsupported modes: an unsupported camera AND n = 0 reports n
        whole_refused(gpu_ctx, lens, opts, with_offset(tc.ODD7, 2, 1, float("inf")), _abi.ERR_INVALID_ARG, "tap 2", out=False)
        whole_refused(gpu_ctx, lens, opts, good, _abi.ERR_INVALID_ARG, "null output", out=False)
        both_refused(gpu_ctx, lens, opts, table_of(tc.ODD7, n=0), _abi.ERR_INVALID_ARG, "n is 0")
        for c, o, cause in [(lens, opts, "depth of field"), (stereo, opts, "stereo"), (cam, copy_opts(count_rays=1), "count_rays"),
                            (cam, copy_opts(prepass_bucket=48), "prepass_bucket")]:
            both_refused(gpu_ctx, c, o, good, _abi.ERR_UNSUPPORTED, cause)
        whole_refused(gpu_ctx, lens, copy_opts(count_rays=1), good, _abi.ERR_UNSUPPORTED, "depth of field")
        # the adaptive call's own arguments, behind the table's
        adaptive_refused(gpu_ctx, cam, opts, with_offset([(0.5, 0.5)], 0, 0, float("nan")), -1.0, _abi.ERR_INVALID_ARG, "tap 0")
        adaptive_refused(gpu_ctx, cam, opts, table_of([(0.0, 0.0)]), -1.0, _abi.ERR_INVALID_ARG, "at least 2")
        adaptive_refused(gpu_ctx, cam, opts, table_of(tc.SHIFT2), -1.0, _abi.ERR_INVALID_ARG, "tap 0 is")
        adaptive_refused(gpu_ctx, cam, opts, with_offset(tc.ODD7, 0, 1, 0.25), thr, _abi.ERR_INVALID_ARG, "tap 0 is")
        adaptive_refused(gpu_ctx, cam, opts, good, -1.0, _abi.ERR_INVALID_ARG, "threshold -1", out=False)
        adaptive_refused(gpu_ctx, cam, opts, good, float("nan"), _abi.ERR_INVALID_ARG, "threshold nan")
        adaptive_refused(gpu_ctx, lens, opts, good, thr, _abi.ERR_INVALID_ARG, "null output", out=False)
        adaptive_refused(gpu_ctx, lens, opts, good, thr, _abi.ERR_INVALID_ARG, "null needs_aa", dev_mask=False, host=False)
        adaptive_refused(gpu_ctx, lens, opts, table_of([(0.0, 0.0)]), thr, _abi.ERR_INVALID_ARG, "at least 2")
        strips = copy_opts(strip_height=8, strip_rank=1, strip_world=2)
        adaptive_refused(gpu_ctx, cam, strips, good, thr, _abi.ERR_UNSUPPORTED, "strip_world")
        adaptive_refused(gpu_ctx, cam, copy_opts(prepass_bucket=48, strip_height=8, strip_rank=1, strip_world=2), good, thr, _abi.ERR_UNSUPPORTED, "prepass_bucket")
        want = gpu_ctx.renderFrameTaps(cam, opts, tc.ODD7)
        two = c2.Context(devices=[0, 0])
        try:
            two.uploadScene(scene.desc)
            adaptive_refused(two, cam, opts, good, thr, _abi.ERR_UNSUPPORTED, "multi-device")
            assert same(two.renderFrameTaps(cam, opts, tc.ODD7), want)       # the whole-frame call runs on the lead device
        finally:
            two.close()
        # a stop request before the launches
        stop = np.ones(1, dtype=np.uint8)
        assert L.c2rt_render_frame_adaptive_taps(gpu_ctx.handle, ref(cam), ref(opts), ref(good), thr, fbuf.ctypes.data, mbuf.ctypes.data,
                                                 stop.ctypes.data) == _abi.ERR_CANCELLED
        assert untouched((fbuf, mbuf))
        # an offset the table does not count is not read; afterwards the context renders correct frames, behind sentinels,
        # with and without the (nullable) host mask
        t = with_offset(tc.ODD7, 7, 0, float("nan"))
        assert L.c2rt_render_frame_taps(gpu_ctx.handle, ref(cam), ref(opts), ref(t), fbuf.ctypes.data) == _abi.OK, last_error(gpu_ctx)
        assert holds(fbuf, want)
        want_frame, want_mask = gpu_ctx.renderFrameAdaptiveTaps(cam, opts, tc.ODD7)
        fbuf2, mbuf2 = frame_and_mask(n, guard_elems=GUARD)
        stop[0] = 0
        assert L.c2rt_render_frame_adaptive_taps(gpu_ctx.handle, ref(cam), ref(opts), ref(t), thr, fbuf2.ctypes.data, mbuf2.ctypes.data,
                                                 stop.ctypes.data) == _abi.OK, last_error(gpu_ctx)
        assert holds(fbuf2, want_frame) and holds(mbuf2, want_mask)
        fbuf3, mbuf3 = frame_and_mask(n, guard_elems=GUARD)
        assert L.c2rt_render_frame_adaptive_taps(gpu_ctx.handle, ref(cam), ref(opts), ref(t), thr, fbuf3.ctypes.data, None, None) == _abi.OK
        assert fbuf3.tobytes() == fbuf2.tobytes() and untouched((mbuf3,))
        assert L.c2rt_render_frame_adaptive_taps_device(gpu_ctx.handle, ref(cam), ref(opts), ref(t), thr, fdev.ptr, mdev.ptr, None) == _abi.OK
        assert hip_runtime().hipDeviceSynchronize() == 0
        got_f, got_m = fdev.get(), mdev.get()
        assert holds(got_f, want_frame) and holds(got_m, want_mask)
    finally:
        fdev.free()
        mdev.free()


# ---- 9: host mirror and Python face ----------------------------------------------------------------------------------------------------


def test_host_mirror_and_python_face(gpu_ctx):
    scene, cam, opts = tc.make_scene("lecture5.sdl", 32, 24)
    gpu_ctx.uploadScene(scene.desc)
    want = gpu_ctx.renderFrameTaps(cam, opts, tc.GRID16)
    want_frame, want_mask = gpu_ctx.renderFrameAdaptiveTaps(cam, opts, tc.GRID16)
    assert 0 < int(want_mask.sum()) < 24 * 32
    r = c2.Renderer(scene, gpu_ctx)
    # the scene's AA setting does not matter to the mirror: the table is the pattern
    for aa in (False, True):
        scene.setAA(aa)
        got = r.renderRTTaps(tc.GRID16)
        assert got.shape == (24, 32, 3) and same(got, want)
        frame, mask = r.renderRTAdaptiveTaps(tc.GRID16)
        assert mask.shape == (24, 32) and mask.tobytes() == want_mask.tobytes() and same(frame, want_frame)
    scene.setAA(False)
    assert same(r.renderRTTaps(c2.TAPS_REF5_TABLE), gpu_ctx.renderFrame(cam, scene.renderOpts(taps=_abi.TAPS_REF5)))
    assert same(r.renderRTTaps(c2.tap_grid(1)), gpu_ctx.renderFrame(cam, opts))
    with pytest.raises(c2.C2rtError) as e:
        r.renderRTAdaptiveTaps(tc.SHIFT2)
    assert e.value.status == _abi.ERR_INVALID_ARG and "tap 0" in str(e.value)
    dof = c2.parseSceneFromFile(os.path.join(SCENES, "zaphod.sdl"))      # as shipped: depth of field
    dof.setFrameSize(32, 24)
    assert dof.camera.dof
    for call in (c2.Renderer(dof, gpu_ctx).renderRTTaps, c2.Renderer(dof, gpu_ctx).renderRTAdaptiveTaps):
        with pytest.raises(c2.C2rtError) as e:
            call(tc.GRID16)
        assert e.value.status == _abi.ERR_UNSUPPORTED and "depth of field" in str(e.value)
