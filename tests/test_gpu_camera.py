"""GPU: camera -> rays -> taps -> pixel against tests/camera_reference.py, a typed numpy restatement of the reference's
camera and sampling stages written from the D source, chained with tests/geom_reference.py and tests/shade_reference.py:
every frame below is compared with a frame that has no oracle and no host mirror anywhere in it (the camera frames are
camera_reference.begin_frame's; tests/test_camera_reference.py holds the host's beginFrame to them on the CPU).
Cases: tests/camera_scenes.py — yaw, pitch and roll, 61x47, 19x53 and 4099x9 frames, 1, 5 and 4 taps, stereo, depth of
field under two seeds, the pre-pass preview, interleaved strips.

Frames are held to camera_reference.compare: bit for bit where a pixel's interval is one float, inside [lo, hi] where a
sample's pow or sin lies at a float32 rounding midpoint; both counts must be 0.  Records under
ray_query_util.assert_records_match_oracle's tolerances."""
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_reference as cr
import camera_scenes as cs
import chess2rt_amd as c2
from chess2rt_amd.api import RAY_HIT_DTYPE
from ray_query_util import assert_records_match_oracle

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not cr.x87_available(), reason="np.longdouble is not the x87 80-bit format: radians cannot be restated")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_GROUND_TILES = 4        # of the 48 tiles of 61x47: the path must have something to render


def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def upload(gpu_ctx, name):
    c = cs.case(name)
    gpu_ctx.uploadScene(c.desc)
    return c


_frames = {}


def gpu_frame(gpu_ctx, name, mode):
    """renderFrame of a case and mode, once (read-only), and the exact redos it caused"""
    if (name, mode) not in _frames:
        c = upload(gpu_ctx, name)
        m = c.modes[mode]
        before = gpu_ctx.exactRedos()
        frame = gpu_ctx.renderFrame(m.cam, m.opts)
        _frames[name, mode] = (frame, gpu_ctx.exactRedos() - before)
    return _frames[name, mode]


# ---- rays ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,mode", [("rolled", "taps1"), ("tall", "taps5"), ("stereo", "taps1"), ("dof", "taps1_seedA"),
                                       ("dof_stereo", "taps1")])
def test_probed_rays_have_the_references_bits(gpu_ctx, name, mode):
    """renderPixel(x, y) at the corners, the edges' midpoints, the centre and seeded random pixels: ray_orig and ray_dir
    are screen_ray's, bit for bit; with a lens the last sample's (lens origin, focal point), the left eye's under stereo"""
    c = upload(gpu_ctx, name)
    m = c.modes[mode]
    for x, y in cs.probe_pixels(c.W, c.H, 64):
        t = gpu_ctx.renderPixel(m.cam, m.opts, x, y)
        assert np.array_equal(_bits64(list(t.ray_orig) + list(t.ray_dir)), _bits64(cs.probed_ray(name, mode, x, y))), (name, x, y)


# ---- hit planes ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,mode", [("rolled", "taps1"), ("tall", "taps5"), ("wide", "taps1")])
def test_hit_planes_equal_the_trace_of_the_references_rays(gpu_ctx, name, mode):
    c = upload(gpu_ctx, name)
    m = c.modes[mode]
    n = c.W * c.H
    ref = cs.reference(name, mode)
    rays, want = ref.rays[:n], ref.recs[:n]                       # tap (0, 0) of every pixel, row-major
    planes = gpu_ctx.renderHits(m.cam, m.opts)
    got = np.zeros(n, dtype=RAY_HIT_DTYPE)
    got["closest_node"], got["leaf_geom"], got["dist"] = planes["node"].ravel(), planes["leaf"].ravel(), planes["dist"].ravel()
    uv = np.ascontiguousarray(planes["uv"]).reshape(n, 2)
    got["u"], got["v"] = uv[:, 0], uv[:, 1]
    got["p"], got["normal"] = np.ascontiguousarray(planes["p"]).reshape(n, 3), np.ascontiguousarray(planes["normal"]).reshape(n, 3)
    assert_records_match_oracle(got, want, "%s planes" % name)
    rec, _ = gpu_ctx.traceRays(np.ascontiguousarray(rays))
    assert np.array_equal(rec["closest_node"], got["closest_node"]) and np.array_equal(rec["leaf_geom"], got["leaf_geom"])
    for f in ("dist", "u", "v", "p", "normal"):
        assert np.array_equal(_bits64(rec[f]), _bits64(got[f])), (name, f)


# ---- frames --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,mode", cs.ALL, ids=cs.IDS)
def test_frame_equals_the_frame_computed_without_the_oracle(gpu_ctx, name, mode):
    c = cs.case(name)
    m = c.modes[mode]
    ref = cs.reference(name, mode)
    frame, redone = gpu_frame(gpu_ctx, name, mode)
    plain, outside = cr.compare(frame, ref)
    print("%s %s: %d pixels, %d held to an interval, %d floats differ, %d outside their bounds, %d tiles redone exactly"
          % (name, mode, ref.ambiguous.size, int((ref.ambiguous | ref.wide).sum()), plain, outside, redone))
    assert frame.shape == ref.rgb.shape
    assert plain == 0 and outside == 0, (name, mode, plain, outside)
    if (name, mode) in cs.NO_LENS:
        assert redone == 0, "the lean instance handed tiles to the exact one"
    fr = m.frame
    if not fr.dof and fr.stereo_separation == 0 and not m.opts.prepass_bucket:      # what a batch accepts
        upload(gpu_ctx, name)
        batch = gpu_ctx.renderFrames([m.cam], m.opts)
        assert np.array_equal(_bits32(batch[0]), _bits32(frame)), (name, mode)


# ---- the ground path -----------------------------------------------------------------------------------------------------------

_CHILD = r'''
import os, sys
sys.path[:0] = [os.getcwd(), os.path.join(os.getcwd(), "tests"), os.path.join(os.getcwd(), "scripts")]
import numpy as np
import chess2rt_amd as c2, csg_void_device as vdev, camera_scenes as cs
out, name, mode = sys.argv[1:4]
c = cs.case(name)
m = c.modes[mode]
ctx = c2.Context(0)
ctx.uploadScene(c.desc)
t = vdev.read_tile_masks(ctx, m.cam, m.opts, 3)
ground_only = -1 if t is None else int(((t[0][..., 2] & 2) != 0).sum())
np.savez(out, frame=ctx.renderFrame(m.cam, m.opts), ground_only=ground_only)
ctx.close()
print("ok")
'''


def _child(out, env_extra):
    env = dict(os.environ, C2RT_LIB_VARIANT="diag", **env_extra)
    p = subprocess.run([sys.executable, "-c", _CHILD, out, "rolled_textured", "taps5"], capture_output=True, text=True, timeout=300,
                       env=env, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout[-4000:] + p.stderr[-4000:]
    return np.load(out), p.stderr


def test_ground_tiles_of_rolled_textured_take_the_ground_path(gpu_ctx, tmp_path):
    """five taps of the bitmap floor under a rolled camera: the mask table marks ground-only tiles (the counter
    tests/test_gpu_ground_tiles.py reads), the ground path renders them, and the frame is the reference's and, bit for
    bit, the one rendered with C2RT_DEBUG_CULL bit 4 set, which leaves every tile to the general path — each in a fresh
    child process on the diagnostics library"""
    on, _ = _child(str(tmp_path / "on.npz"), {})
    off, err = _child(str(tmp_path / "off.npz"), dict(C2RT_DEBUG_CULL="16"))
    assert "C2RT_DEBUG_CULL=16" in err
    print("rolled_textured taps5: %d ground-only tiles" % int(on["ground_only"]))
    assert int(on["ground_only"]) == int(off["ground_only"]) >= MIN_GROUND_TILES
    assert np.array_equal(_bits32(on["frame"]), _bits32(off["frame"]))
    ref = cs.reference("rolled_textured", "taps5")
    assert cr.compare(on["frame"], ref) == (0, 0)
    assert np.array_equal(_bits32(on["frame"]), _bits32(gpu_frame(gpu_ctx, "rolled_textured", "taps5")[0]))


# ---- strips --------------------------------------------------------------------------------------------------------------------


def test_strips_reinterleave_to_the_whole_frame(gpu_ctx):
    c = cs.case("strips")
    whole, _ = gpu_frame(gpu_ctx, "strips", "whole")
    ref = cs.reference("strips", "whole")
    built = np.full_like(whole, np.nan)
    ref_built = np.full_like(whole, np.nan)
    for r in range(3):
        mode = "rank%d" % r
        rows = cr.local_frame_rows(c.modes[mode].ropts)
        part, _ = gpu_frame(gpu_ctx, "strips", mode)
        assert part.shape[0] == len(rows) == gpu_ctx.localRows(c.modes[mode].opts)
        built[rows] = part
        ref_built[rows] = cs.reference("strips", mode).rgb
    assert np.array_equal(_bits32(built), _bits32(whole))
    assert np.array_equal(_bits32(ref_built), _bits32(ref.rgb))          # the reference's ranks make its whole frame too
    assert cr.compare(built, ref) == (0, 0)


def test_two_slot_context_renders_tall_to_the_same_bits(gpu_ctx):
    c = cs.case("tall")
    m = c.modes["taps5"]
    frame, _ = gpu_frame(gpu_ctx, "tall", "taps5")
    multi = c2.Context(devices=[0, 0])
    try:
        assert multi.deviceCount == 2
        multi.uploadScene(c.desc)
        assert np.array_equal(_bits32(multi.renderFrame(m.cam, m.opts)), _bits32(frame))
    finally:
        multi.close()


# ---- the display frame ---------------------------------------------------------------------------------------------------------


def test_rgb32_frame_is_the_encoding_of_the_reference_frame(gpu_ctx):
    """renderFrameRGB32 of rolled at five taps against the host's Color.toRGB32 of the reference frame, but for the
    pixels whose interval straddles a byte boundary (tests/test_camera_reference.py: at most 3)"""
    c = upload(gpu_ctx, "rolled")
    m = c.modes["taps5"]
    ref = cs.reference("rolled", "taps5")
    lo, hi = cs.encode_rgb32(ref.lo), cs.encode_rgb32(ref.hi)
    straddle = lo != hi
    packed = gpu_ctx.renderFrameRGB32(m.cam, m.opts)
    print("rolled taps5 rgb32: %d pixels straddle a byte boundary" % int(straddle.sum()))
    assert packed.shape == lo.shape and packed.dtype == np.uint32
    assert np.array_equal(packed[~straddle], cs.encode_rgb32(ref.rgb)[~straddle])
    for shift in (0, 8, 16):
        ch, a, b = (packed >> shift) & 255, (lo >> shift) & 255, (hi >> shift) & 255
        assert ((ch >= a) & (ch <= b))[straddle].all()
