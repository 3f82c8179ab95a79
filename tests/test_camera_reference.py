"""CPU: tests/camera_reference.py (a typed numpy restatement of the reference's camera and sampling stages, written from
the D source) against the host mirror's beginFrame, the oracle's rays, RNG, lens sample and frames, on the cases of
tests/camera_scenes.py — plus the conditions that make the comparison mean something (what the frames show, the
ambiguity cap, no hit-list cap, no sort ties), a mutation check and the accuracy of the build-defined lens sample.

A frame comparison uses camera_reference.compare's two counts (floats that differ in pixels held to their bits, floats
outside [lo, hi] in the others); both must be 0.  A shared misreading of the D source between the new reference and the
oracle's author would not show here; a private one in either does."""
import ctypes as C
import os
import re

import mpmath
import numpy as np
import pytest

import camera_reference as cr
import camera_scenes as cs
import chess2rt_amd as c2
import oracle_lib as orc
from golden_configs import SCENES
from unit_inputs import RNG_INPUTS

pytestmark = pytest.mark.skipif(not cr.x87_available(), reason="np.longdouble is not the x87 80-bit format: radians cannot be restated")

MIN_REACH = 30              # tests/test_shade_reference.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured here over the cases' draws and 10^5 random u, in units of 2^-52 (an ulp of 1): the largest distance of the
# restated (sin, cos)(2 pi u) from mpmath's was 0.7802 ulp (1.73e-16); the bound asserted is twice that
LENS_MEASURED_ULPS = 0.7802
LENS_BOUND_ULPS = 2 * LENS_MEASURED_ULPS
RGB32_STRADDLE_CAP = 3


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- (a) the host mirror ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,mode", cs.ALL, ids=cs.IDS)
def test_host_begin_frame_equals_the_reference_on_the_cases(name, mode):
    m = cs.case(name).modes[mode]
    assert cs.frame_bits(m.host_cam) == cs.frame_bits(m.frame) == cs.frame_bits(m.cam), m.params


@pytest.mark.parametrize("scene_file", ["zaphod.sdl", "csg_stress.sdl", "lecture5.sdl"])
def test_host_begin_frame_equals_the_reference_on_the_scene_files(scene_file):
    """the file's own camera, then the state after rotateCamera(10, 5, -100) (the pitch clamp) and moveCamera"""
    scene = c2.parseSceneFromFile(os.path.join(SCENES, scene_file))
    hc = scene.camera
    W, H = int(hc.frame_width), int(hc.frame_height)
    args, cam = cs.host_camera(scene, W, H)
    frame = cr.begin_frame(**args)
    assert cs.frame_bits(cam) == cs.frame_bits(frame), args
    scene.rotateCamera(10.0, 5.0, -100.0)
    yaw, pitch, roll = cr.rotate(args["yaw"], args["pitch"], args["roll"], 10.0, 5.0, -100.0)
    assert pitch == -90.0
    turned = cr.begin_frame(**dict(args, yaw=yaw, pitch=pitch, roll=roll))
    assert cs.frame_bits(scene.beginFrame()) == cs.frame_bits(turned)
    scene.moveCamera(3.5, -1.25, 40.0)
    pos = cr.move(turned, 3.5, -1.25, 40.0)
    moved = cr.begin_frame(**dict(args, yaw=yaw, pitch=pitch, roll=roll, pos=tuple(pos)))
    assert cs.frame_bits(scene.beginFrame()) == cs.frame_bits(moved)
    hc = scene.camera
    assert (hc.yaw, hc.pitch, hc.roll) == (yaw, pitch, roll) and np.array_equal(_bits(list(hc.pos)), _bits(pos))


# ---- (b) rays, RNG, the lens sample ----------------------------------------------------------------------------------------


def test_screen_rays_equal_the_oracles_on_every_pixel_and_tap_of_rolled():
    c = cs.case("rolled")
    m = c.modes["taps1"]
    L = orc.lib()
    yy, xx = np.meshgrid(np.arange(c.H, dtype=np.float64), np.arange(c.W, dtype=np.float64), indexing="ij")
    o3, d3 = (C.c_double * 3)(), (C.c_double * 3)()
    for ox, oy in cr.AA_KERNEL:
        x, y = xx.ravel() + ox, yy.ravel() + oy
        orig, dirn = cr.screen_ray(m.frame, x, y)
        want = np.empty((len(x), 6))
        for i in range(len(x)):
            L.orc_screen_ray(C.byref(m.cam), x[i], y[i], o3, d3)
            want[i, :3], want[i, 3:] = list(o3), list(d3)
        assert np.array_equal(_bits(np.hstack([orig, dirn])), _bits(want)), (ox, oy)
    first = cr.screen_ray(m.frame, xx.ravel(), yy.ravel())
    assert np.array_equal(_bits(cs.pixel_rays("rolled")), _bits(np.hstack(first)))


@pytest.mark.parametrize("name,mode", [("rolled", "taps1"), ("stereo", "taps1"), ("dof", "taps1_seedA"), ("dof_stereo", "taps1")])
def test_probed_rays_equal_the_oracles(name, mode):
    """what renderPixel reports as the ray: the last lens sample's, the left eye's — lens origin and focal point to the bit"""
    c = cs.case(name)
    m = c.modes[mode]
    for x, y in cs.probe_pixels(c.W, c.H, 16):
        t = orc.render_pixel(c.desc, m.cam, m.opts, x, y)
        assert np.array_equal(_bits(list(t.ray_orig) + list(t.ray_dir)), _bits(cs.probed_ray(name, mode, x, y))), (x, y)


def _case_draws():
    """every uniform the cases with a lens drew"""
    return np.unique(np.concatenate([cs.reference(n, m).draws for n, m in cs.ALL if len(cs.reference(n, m).draws)]))


def test_rng_equals_the_oracles():
    L = orc.lib()
    for seed, pixel, tap, sample, dim in RNG_INPUTS:
        got = cr.rng_uniform(cr.rng_key(seed, pixel, tap), sample, dim)
        assert float(got) == L.orc_rng_uniform(seed, pixel, tap, sample, dim), (seed, pixel, tap, sample, dim)
    # the cases' own draws: every pixel, some (lens sample, dimension) pairs; a second eye draws dimensions 4..7
    for name, mode, seed, taps, dims in (("dof", "taps5_seedA", cs.SEED_A, (0, 4), ((0, 0), (0, 3), (2, 1), (2, 2))),
                                         ("dof", "taps5_seedB", cs.SEED_B, (0, 4), ((0, 0), (0, 3), (2, 1), (2, 2))),
                                         ("dof_stereo", "taps1", cs.SEED_A, (0,), ((0, 5), (1, 0), (1, 7)))):
        c = cs.case(name)
        drawn = cs.reference(name, mode).draws
        pixel = np.arange(c.W * c.H, dtype=np.uint64)
        for tap in taps:
            key = cr.rng_key(seed, pixel, np.full(len(pixel), tap, dtype=np.uint32))
            for sample, dim in dims:
                got = cr.rng_uniform(key, np.full(len(pixel), sample), np.full(len(pixel), dim))
                want = [L.orc_rng_uniform(seed, int(p), tap, sample, dim) for p in pixel]
                assert np.array_equal(_bits(got), _bits(want)), (name, seed, tap, sample, dim)
                assert np.isin(got, drawn).all(), (name, tap, sample, dim)


def test_lens_coefficients_are_the_correctly_rounded_reciprocal_factorials():
    """each +-1/k! computed here (fractions, rounded once) equals the device's hex constant, and so does pi / 2"""
    text = open(os.path.join(ROOT, "chess2rt_amd", "csrc", "c2rt_trace_shared.inc")).read()
    body = text[text.index("DEV void lens_sincos2pi"):]
    body = body[:body.index("\n}\n")]
    consts = [float.fromhex(h) for h in re.findall(r"-?0x1\.[0-9a-f]+p[+-]\d+", body)]
    assert len(consts) == 1 + 8 + 7, consts
    assert consts[0] == cr.HALF_PI
    assert tuple(consts[1:9]) == cr.SIN_COEFFS
    assert tuple(consts[9:]) == cr.COS_COEFFS[:7] and cr.COS_COEFFS[7] == -0.5 and "-0.5 + z * pc" in body


def test_lens_sincos_equals_the_oracles_and_is_close_to_the_exact_values():
    rng = np.random.RandomState(2026)
    u = np.concatenate([_case_draws(), rng.randint(0, 2 ** 32, size=100000).astype(np.float64) * 2.0 ** -32,
                        [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1 - 2.0 ** -32, 2.0 ** -32]])
    sn, cs_ = cr.lens_sincos2pi(u)
    L = orc.lib()
    a, b = (C.c_double * 1)(), (C.c_double * 1)()
    want = np.empty((len(u), 2))
    for i, ui in enumerate(u):
        L.orc_lens_sincos2pi(ui, a, b)
        want[i] = a[0], b[0]
    assert np.array_equal(_bits(np.stack([sn, cs_], axis=1)), _bits(want))
    worst = mpmath.mpf(0)
    for ui, s, c in zip(u, sn, cs_):
        es, ec = cr.exact_sincos2pi(ui)
        worst = max(worst, abs(es - mpmath.mpf(float(s))), abs(ec - mpmath.mpf(float(c))))
    ulps = float(worst * 2 ** 52)
    print("lens_sincos2pi: largest distance from mpmath over %d draws: %.4f ulp of 1 (%.3g); measured when written: %.4f, bound %.4f"
          % (len(u), ulps, float(worst), LENS_MEASURED_ULPS, LENS_BOUND_ULPS))
    assert ulps <= LENS_BOUND_ULPS


# ---- (c) frames ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,mode", cs.ALL, ids=cs.IDS)
def test_reference_frame_equals_the_oracles(name, mode):
    c = cs.case(name)
    m = c.modes[mode]
    r = cs.reference(name, mode)
    frame = orc.render_frame(c.desc, m.cam, m.opts, 1)
    plain, outside = cr.compare(frame, r)
    held = int((r.ambiguous | r.wide).sum())
    print("%s %s: %d pixels, %d rays, %.2f s; %d pixels with a non-degenerate interval, %d held to an interval; %d floats differ, %d outside"
          % (name, mode, r.ambiguous.size, len(r.rays), r.seconds, int(r.wide.sum()), held, plain, outside))
    assert frame.shape == r.rgb.shape
    assert plain == 0 and outside == 0


@pytest.mark.parametrize("name,mode", cs.ALL, ids=cs.IDS)
def test_conditions_on_the_cases(name, mode):
    """the ambiguity cap (pixels held to an interval <= samples per pixel x 0.001), no hit list at the cap, no equal
    distances in a sorted list, and something to see: at least two nodes reached by MIN_REACH rays each
    (the preview has a dozen samples: two distinct block colours)"""
    r = cs.reference(name, mode)
    held = float((r.ambiguous | r.wide).mean())
    assert held <= cs.ambiguity_cap(r), (held, cs.ambiguity_cap(r))
    assert r.trace.truncations == 0 and r.vis_trace.truncations == 0 and r.trace.ties == 0 and r.vis_trace.ties == 0
    nodes, counts = np.unique(r.recs["closest_node"], return_counts=True)
    print("%s %s: closest node -> rays %s" % (name, mode, dict(zip(nodes.tolist(), counts.tolist()))))
    if name == "preview":
        assert len(np.unique(r.rgb.reshape(-1, 3).view(np.uint32), axis=0)) >= 2
        return
    assert (counts[nodes >= 0] >= MIN_REACH).sum() >= 2
    assert np.isfinite(r.rgb).all() and (r.rgb > 0).any()


def test_wide_reaches_the_sphere_across_columns_beyond_4096():
    r = cs.reference("wide", "taps1")
    node = r.recs["closest_node"].reshape(cs.WIDE_H, cs.WIDE_W)
    cols = np.nonzero((node == cs.WIDE_SPHERE).any(axis=0))[0]
    print("wide: the sphere spans columns %d..%d; the last column shows node %s" % (cols.min(), cols.max(), node[:, -1].tolist()))
    assert len(cols) >= MIN_REACH and (node[:, 4097:] >= 0).all()


def test_accumulation_is_monotone():
    """what carrying [lo, hi] through combineStereo and both sums rests on: lo <= x <= hi per channel going in gives the
    same coming out — random colours, every mode's shape"""
    rng = np.random.RandomState(5)
    for ntaps, ns, ne, dof in ((1, 1, 1, False), (5, 1, 1, False), (4, 1, 2, False), (5, 3, 1, True), (1, 2, 2, True)):
        fr = cr.Frame()
        fr.dof, fr.num_samples = dof, ns
        x = rng.uniform(0, 2, size=(ntaps * ns * ne * 500, 3)).astype(np.float32)
        lo = np.nextafter(x, np.float32(-np.inf)) - (rng.rand(*x.shape) < 0.3).astype(np.float32) * np.float32(1e-3)
        hi = np.nextafter(x, np.float32(np.inf)) + (rng.rand(*x.shape) < 0.3).astype(np.float32) * np.float32(1e-3)
        a, b, c = (cr.accumulate(v, ntaps, ns, ne, fr) for v in (lo, x, hi))
        assert (a <= b).all() and (b <= c).all() and (a < c).any()


def test_rgb32_of_rolled_straddles_few_byte_boundaries():
    """what tests/test_gpu_camera.py's display-frame case rests on: the encodings of lo and hi differ on few pixels"""
    r = cs.reference("rolled", "taps5")
    n = int((cs.encode_rgb32(r.lo) != cs.encode_rgb32(r.hi)).sum())
    print("rolled taps5: %d pixels whose interval straddles a byte boundary" % n)
    assert n <= RGB32_STRADDLE_CAP


# ---- (d) mutations ------------------------------------------------------------------------------------------------------------

# misreading -> the (case, mode) that sees it
MUTATION_TARGETS = {
    "pixel_centre": ("rolled", "taps1"), "aspect_inverted": ("rolled", "taps1"), "rotation_order_reversed": ("rolled", "taps1"),
    "column_vector_product": ("rolled", "taps1"), "fov_not_halved": ("rolled", "taps1"),
    "second_stereo_offset_dropped": ("dof_stereo", "taps1"), "stereo_sign_swapped": ("stereo", "taps1"),
    "lens_sin_cos_swapped": ("dof", "taps1_seedA"), "disc_multiplier_is_fnumber": ("dof", "taps1_seedA"),
    "focal_distance_along_ray": ("dof", "taps1_seedA"), "cos_from_unnormalised_dir": ("dof", "taps1_seedA"),
    "lens_up_before_right": ("dof", "taps1_seedA"), "taps_two_and_three_swapped": ("rolled", "taps5"),
    "tap_divide_by_reciprocal": ("rolled", "taps5"), "eyes_share_one_jitter": ("dof_stereo", "taps1"),
    "draws_lens_before_jitter": ("dof", "taps1_seedA"), "rng_pixel_from_local_row": ("strips", "rank1"),
    "prepass_block_not_clipped": ("preview", "lens"), "prepass_pixel_from_own_xy": ("preview", "lens"),
    "saturation_after_channel_mask": ("stereo", "taps1"),
}
MIN_MUTATION_PIXELS = 30
# (pos + dx * rightDir) + dy * upDir against (pos + dy * upDir) + dx * rightDir is the last bit of the origin: no colour of
# frames this small moves, the rays do — so this one is counted on the rays, and tests/test_gpu_camera.py holds the
# device's probe to the reference's lens origin bit for bit
COUNTED_ON_RAYS = ("lens_up_before_right",)


def test_every_named_misreading_has_a_target():
    assert sorted(MUTATION_TARGETS) == sorted(cr.MUTATIONS)


@pytest.mark.parametrize("mutation", cr.MUTATIONS)
def test_the_cases_see_each_named_misreading(mutation):
    """a pixel counts only if it leaves the bounds of the unmutated reference (so ambiguity cannot hide it); for
    COUNTED_ON_RAYS a pixel counts when the bits of one of its rays change"""
    name, mode = MUTATION_TARGETS[mutation]
    c = cs.case(name)
    m = c.modes[mode]
    ref = cs.reference(name, mode)
    wrong = cr.render_frame(c.tables, cr.begin_frame(mut=mutation, **m.params), m.ropts, mut=mutation)
    with np.errstate(invalid="ignore"):
        moved = (~((wrong.rgb >= ref.lo) & (wrong.rgb <= ref.hi))).any(axis=-1)
    if mutation in COUNTED_ON_RAYS:
        assert not moved.any()          # (if it ever does, count it on the pixels like the others)
        moved = (wrong.rays.view(np.uint64) != ref.rays.view(np.uint64)).any(axis=1).reshape(ref.samples_per_pixel, -1).any(axis=0)
    print("%s is caught by %s %s: %d of %d pixels change%s" % (mutation, name, mode, int(moved.sum()), moved.size,
                                                               " (their rays)" if mutation in COUNTED_ON_RAYS else ""))
    assert moved.sum() >= MIN_MUTATION_PIXELS


# ---- (e) C2RT_TAPS_4 ----------------------------------------------------------------------------------------------------------


def test_taps_4_is_the_first_four_entries_of_the_table():
    """"taps 1-4 of that table averaged /4.0f" counts the table's five taps from 1, and a pixel's
    own sample at (0, 0) is the one the AA pass starts from — entries 0..3.  The ABI comment says so, the reference
    computes so, and the oracle's frame (hence the device's, tests/test_gpu_camera.py) equals it."""
    header = open(os.path.join(ROOT, "include", "c2rt.h")).read()
    line = [l for l in header.splitlines() if "C2RT_TAPS_4 = 4" in l][0]
    assert "first four entries" in line and "1..4" not in line
    c = cs.case("rolled")
    four, five = cs.reference("rolled", "taps4"), cs.reference("rolled", "taps5")
    n = c.W * c.H
    assert np.array_equal(four.rays, five.rays[:4 * n])           # the rays of table entries 0..3, in order
    assert np.array_equal(four.rays[:n], cs.reference("rolled", "taps1").rays)
