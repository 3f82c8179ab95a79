"""CPU half of the variance-guided filter's tests: the numpy restatement itself (tests/denoise_variance_reference.py) tied
to c2rt_denoise's and on cases worked out by hand, the ABI's struct and the one entry point that needs no device, the
property the feature exists for — the same relative residue at every noise level — and the precondition of the GPU
comparison: that the frames it compares put pixels and taps into every class of both stages."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import denoise_reference as dr
import denoise_variance_cases as vc
import denoise_variance_reference as vr
import occlusion_cases as oc
import temporal_cases as tc
import temporal_reference as tr
from chess2rt_amd import _abi, denoise_variance_scratch_bytes
from ray_query_util import oracle_trace, screen_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
LUM = (F(0.2126), F(0.7152), F(0.0722))


def flat_guides(h, w, node=0):
    """every pixel on one node, facing +z, on the plane z = 0: every normal and plane term is exactly 1"""
    ys, xs = np.mgrid[0:h, 0:w]
    normal = np.zeros((h, w, 3))
    normal[..., 2] = 1.0
    p = np.stack([xs, ys, np.zeros_like(xs)], axis=-1).astype(np.float64)
    return np.full((h, w), node, dtype=np.int32), normal, p


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the ABI ------------------------------------------------------------------------------------------------------------------


def test_struct_layouts_match_c(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "c2rt.h"
int main(void) {
  printf("DenoiseVarianceOpts %zu\\n", sizeof(c2rt_denoise_variance_opts));
  printf("opts.levels %zu\\n", offsetof(c2rt_denoise_variance_opts, levels));
  printf("opts.sigma_plane %zu\\n", offsetof(c2rt_denoise_variance_opts, sigma_plane));
  printf("opts.sigma_lum %zu\\n", offsetof(c2rt_denoise_variance_opts, sigma_lum));
  printf("opts.var_floor %zu\\n", offsetof(c2rt_denoise_variance_opts, var_floor));
  printf("opts.min_age %zu\\n", offsetof(c2rt_denoise_variance_opts, min_age));
  printf("opts.reserved %zu\\n", offsetof(c2rt_denoise_variance_opts, reserved));
  printf("min_age %d\\n", C2RT_MAX_VARIANCE_MIN_AGE);
  printf("abi %u\\n", C2RT_ABI_VERSION);
  return 0;
}
""")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    O = _abi.DenoiseVarianceOpts
    assert {k: int(v) for k, v in got.items()} == {
        "DenoiseVarianceOpts": C.sizeof(O), "opts.levels": O.levels.offset, "opts.sigma_plane": O.sigma_plane.offset, "opts.sigma_lum": O.sigma_lum.offset,
        "opts.var_floor": O.var_floor.offset, "opts.min_age": O.min_age.offset, "opts.reserved": O.reserved.offset,
        "min_age": _abi.MAX_VARIANCE_MIN_AGE, "abi": _abi.ABI_VERSION}
    assert C.sizeof(O) == 40 and _abi.ABI_VERSION == 1 and _abi.MAX_VARIANCE_MIN_AGE == vr.MAX_MIN_AGE == 64


def test_scratch_bytes_is_host_arithmetic():
    """no context, no device: the header's formula, never more than 56 B per pixel, and zero for every refused option"""
    for w, h in ((1, 1), (61, 47), (1920, 1080), (65536, 3)):
        for ch in (1, 3):
            for levels in range(0, 9):
                for min_age in (0, 4):
                    n = denoise_variance_scratch_bytes(w, h, ch, levels, min_age=min_age)
                    want = (32 if levels > 0 or min_age > 0 else 0) + (4 * ch if levels > 1 else 0) + (8 if levels > 0 else 0) + (4 if levels > 1 else 0)
                    assert n == w * h * want and n <= 56 * w * h
    assert denoise_variance_scratch_bytes(8, 8, 3, 0, min_age=0) == 0 and denoise_variance_scratch_bytes(8, 8, 3, 5) == 64 * 56
    ok = dict(width=8, height=8, channels=3, levels=5, normal_power_log2=5, sigma_plane=1.0, sigma_lum=4.0, var_floor=1e-8, min_age=4)
    assert denoise_variance_scratch_bytes(**ok) > 0
    assert denoise_variance_scratch_bytes(**dict(ok, sigma_lum=0.0, min_age=64, var_floor=1e-45)) > 0
    for bad in (dict(width=0), dict(height=0), dict(channels=2), dict(channels=4), dict(channels=0), dict(sigma_plane=0.0), dict(sigma_plane=-1.0),
                dict(sigma_plane=float("nan")), dict(sigma_plane=float("inf")), dict(sigma_lum=-0.5), dict(sigma_lum=float("nan")),
                dict(sigma_lum=float("inf")), dict(var_floor=0.0), dict(var_floor=-1e-8), dict(var_floor=float("nan")), dict(var_floor=float("inf")),
                dict(levels=9), dict(normal_power_log2=8), dict(min_age=65)):
        assert denoise_variance_scratch_bytes(**dict(ok, **bad)) == 0, bad
    lib = _abi.load_library()
    o = _abi.DenoiseVarianceOpts(width=8, height=8, levels=5, channels=3, normal_power_log2=5, sigma_plane=1.0, sigma_lum=4.0, var_floor=1e-8, min_age=4,
                                 reserved=1)
    assert lib.c2rt_denoise_variance_scratch_bytes(C.byref(o)) == 0
    assert lib.c2rt_denoise_variance_scratch_bytes(None) == 0


# ---- 2. the tie to c2rt_denoise ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("levels", [0, 1, 3, 8])
def test_no_luminance_term_is_the_plain_filter_without_a_colour_term(levels):
    for (h, w), ch in (((9, 13), 3), ((47, 61), 3), ((20, 33), 1)):
        g, img, variance, age = vc.synthetic(h, w, 100 * w + h, ch)
        img = img if ch == 3 else img[..., 0]
        for power, kw in ((1, {}), (5, dict(albedo=img[::-1].copy(), base=img[:, ::-1].copy()))):
            want = dr.denoise(g["node"], g["normal"], g["p"], img, levels, power, 0.5, sigma_colour=0.0, **kw)
            for a in (None, age):
                got, _ = vr.denoise_variance(g["node"], g["normal"], g["p"], img, variance, a, levels, power, 0.5, sigma_lum=0.0, min_age=vc.MIN_AGE, **kw)
                assert got.shape == img.shape and bits(got).tobytes() == bits(want).tobytes(), (h, w, ch, power, levels)


# ---- 3. cases worked out by hand --------------------------------------------------------------------------------------------------


def test_one_pixel_frame_and_a_lone_hit_among_misses():
    """only the centre counts: D = (w C) / w and V' = (w w V) / (w w) with w = K[2] K[2] = 9/64 at every level, whatever the
    luminance term; a young lone pixel has l alone in its window: m2 - m1 m1 = l l - l l = 0, V0 = +0f"""
    w9 = dr.K[2] * dr.K[2]
    c = np.array([[[0.3, 1.7, 0.9]]], dtype=np.float32)
    v = np.array([[0.37]], dtype=np.float32)
    node, normal, p = flat_guides(1, 1)
    out, vout = vr.denoise_variance(node, normal, p, c, v, None, 2, 5, 1.0)
    want, wantv = c, v
    for _ in range(2):
        want, wantv = (w9 * want) / w9, ((w9 * w9) * wantv) / (w9 * w9)
    assert bits(out).tobytes() == bits(want).tobytes() and bits(vout).tobytes() == bits(wantv).tobytes()
    out, vout = vr.denoise_variance(node, normal, p, c, v, np.array([[1]], dtype=np.uint32), 0, 5, 1.0, min_age=4)
    assert bits(out).tobytes() == bits(c).tobytes() and bits(vout)[0, 0] == 0

    node, normal, p = flat_guides(7, 9)
    node[:] = -1
    node[3, 4] = 2
    rng = np.random.RandomState(2)
    img = rng.uniform(0, 2, (7, 9, 3)).astype(np.float32)
    var = rng.uniform(0, 1, (7, 9)).astype(np.float32)
    out, vout = vr.denoise_variance(node, normal, p, img, var, None, 1, 5, 1.0)
    miss = node < 0
    assert bits(out[miss]).tobytes() == bits(img[miss]).tobytes() and not bits(vout[miss]).any()        # a miss: C's bits, V0 = +0f
    assert bits(out[3, 4]).tobytes() == bits((w9 * img[3, 4]) / w9).tobytes()
    assert bits(vout[3, 4]) == bits(((w9 * w9) * var[3, 4]) / (w9 * w9))


def test_constant_plane_with_constant_variance():
    """Flat guides, power 0, a constant colour c and variance V, one level.  dl = 0 exactly, so the luminance factor is 1f /
    (1f + 0f * inv_l) = 1 and w = K[i] K[j] = k / 256: every product with c = 2995/4096 (12 bits) and every partial sum fits 24
    bits, sumw = 1 at an interior pixel, the quotient is correctly rounded: the colour stays within half an ulp (asserted to
    one, over the whole frame, as c2rt_denoise's test does).  The variance at an interior pixel is V * sum (K[i] K[j])^2 / 1^2
    = V * (35/128)^2 = V * 1225/16384 — exactly, for V a power of two (every (K[i] K[j])^2 is a multiple of 2^-16)."""
    c, V = F(2995.0 / 4096.0), F(0.25)
    node, normal, p = flat_guides(12, 17)
    img = np.full((12, 17, 3), c, dtype=np.float32)
    out, vout = vr.denoise_variance(node, normal, p, img, np.full((12, 17), V, dtype=np.float32), None, 1, 0, 1.0, sigma_lum=4.0)
    assert np.abs(out.astype(np.float64) - np.float64(c)).max() <= np.spacing(c)
    k = [Fraction(1, 16), Fraction(1, 4), Fraction(3, 8), Fraction(1, 4), Fraction(1, 16)]
    ratio = sum((a * b) ** 2 for a in k for b in k)
    assert ratio == Fraction(1225, 16384)
    assert (vout[2:-2, 2:-2] == F(0.25 * 1225 / 16384)).all() and float(F(0.25 * 1225 / 16384)) == 0.25 * 1225 / 16384
    assert (vout[0, 0] > vout[2, 2])                              # fewer taps at a corner: less averaging


def test_young_pixel_with_two_known_luminances():
    """A 7x7 flat frame, one channel, every pixel 1 except the left three columns at 3; the centre (3, 3) is young with age
    2, min_age 4.  Its window is the whole frame, every w = 1 (power 0, flat): sumw = 49, s1 = 21*3 + 28*1 = 91, s2 = 21*9 +
    28 = 217, all exact; m1 = fl(91/49), m2 = fl(217/49), v = m2 - m1*m1 in fp32 (about 48/49), times the boost 4/2 = 2.
    Its neighbour (3, 2) has age 0: the boost divides by max(0, 1) = 1 and is 4; its window is the columns 0 .. 5 (x = -1 is
    outside), 21 threes and 21 ones: m1 = 84/42 = 2, m2 = 210/42 = 5, v = 1, V0 = 4 exactly.  (3, 4) is old enough: its
    temporal bits."""
    node, normal, p = flat_guides(7, 7)
    img = np.ones((7, 7), dtype=np.float32)
    img[:, :3] = 3.0
    var = np.full((7, 7), 0.125, dtype=np.float32)
    age = np.full((7, 7), 9, dtype=np.uint32)
    age[3, 3], age[3, 2] = 2, 0
    counts = {}
    _, v0 = vr.denoise_variance(node, normal, p, img, var, age, 0, 0, 1.0, min_age=4, counts=counts)
    m1, m2 = F(91.0) / F(49.0), F(217.0) / F(49.0)
    v = m2 - m1 * m1
    assert abs(float(v) - 48.0 / 49.0) < 1e-5 and v > 0
    assert bits(v0[3, 3]) == bits(v * (F(4.0) / F(2.0)))
    assert bits(v0[3, 2]) == bits(F(4.0))
    assert bits(v0[3, 4]) == bits(F(0.125))
    assert counts["young"] == 2 and counts["temporal"] == 47
    # three channels: the luminance of a grey pixel is (0.2126f g + 0.7152f g) + 0.0722f g, not g
    rgb = np.repeat(img[..., None], 3, axis=2)
    _, v3 = vr.denoise_variance(node, normal, p, rgb, var, age, 0, 0, 1.0, min_age=4)
    l1, l3 = (LUM[0] * F(1) + LUM[1] * F(1)) + LUM[2] * F(1), (LUM[0] * F(3) + LUM[1] * F(3)) + LUM[2] * F(3)
    s1 = s2 = sw = F(0)
    for j in range(7):
        for i in range(7):
            l = l3 if i < 3 else l1
            s1, s2, sw = s1 + F(1) * l, s2 + F(1) * (l * l), sw + F(1)
    m1, m2 = s1 / sw, s2 / sw
    v = m2 - m1 * m1
    assert bits(v3[3, 3]) == bits((v if v > 0 else F(0)) * (F(4.0) / F(2.0)))


def test_age_null_or_min_age_zero_keep_the_temporal_variance():
    g, img, variance, age = vc.synthetic(9, 11, 3)
    hit = g["node"] >= 0
    for a, m in ((None, 4), (age, 0), (np.full_like(age, 4), 4)):
        _, v0 = vr.denoise_variance(g["node"], g["normal"], g["p"], img, variance, a, 0, 5, 1.0, min_age=m)
        assert bits(v0[hit]).tobytes() == bits(variance[hit]).tobytes() and not bits(v0[~hit]).any()


# ---- 4. what the feature is for -------------------------------------------------------------------------------------------------


def step_scene(sd):
    """64x48, one flat node (p = (0.1 x, 0.1 y, 0), normal +z), luminance 0.2 left of x = 32 and 1.0 from there on, normal
    noise of standard deviation sd in all three channels; the luminance's variance is sd^2 (0.2126^2 + 0.7152^2 + 0.0722^2)"""
    h, w = 48, 64
    ys, xs = np.mgrid[0:h, 0:w]
    normal = np.zeros((h, w, 3))
    normal[..., 2] = 1.0
    p = np.stack([0.1 * xs, 0.1 * ys, 0.0 * xs], axis=-1)
    clean = np.where(xs >= 32, 1.0, 0.2)[..., None].repeat(3, axis=2)
    noisy = (clean + sd * np.random.RandomState(11).normal(size=(h, w, 3))).astype(np.float32)
    variance = np.full((h, w), sd * sd * (0.2126 ** 2 + 0.7152 ** 2 + 0.0722 ** 2), dtype=np.float32)
    return np.zeros((h, w), dtype=np.int32), normal, p, clean, noisy, variance, np.abs(xs - 31.5)


def residue(out, clean, where, sd):
    d = (out.astype(np.float64) - clean)[where]
    return float(np.sqrt((d * d).mean())) / sd


def test_noise_adaptivity_of_the_contract():
    """One sigma_lum serves every noise level: the flat region's residue relative to sd agrees across sd = 0.02, 0.1, 0.3
    within a factor 1.25 and is below 0.06, the edge region's stays below 0.25 — while c2rt_denoise with ONE sigma_colour
    (0.5) varies by more than a factor 2 across the same three."""
    flat_v, edge_v, flat_c = [], [], []
    for sd in (0.02, 0.1, 0.3):
        node, normal, p, clean, noisy, variance, dist = step_scene(sd)
        age = np.full(node.shape, 100, dtype=np.uint32)
        out, _ = vr.denoise_variance(node, normal, p, noisy, variance, age, 4, 5, 1.0, sigma_lum=4.0, var_floor=1e-8)
        plain = dr.denoise(node, normal, p, noisy, 4, 5, 1.0, sigma_colour=0.5)
        flat_v.append(residue(out, clean, dist >= 20, sd))
        edge_v.append(residue(out, clean, dist < 8, sd))
        flat_c.append(residue(plain, clean, dist >= 20, sd))
    print("variance-guided, flat / sd:", flat_v, "edge / sd:", edge_v, "; plain filter, flat / sd:", flat_c)
    assert max(flat_v) / min(flat_v) <= 1.25
    assert max(flat_v) < 0.06
    assert max(edge_v) < 0.25
    assert max(flat_c) / min(flat_c) > 2.0


# ---- 5. the GPU comparison is not vacuous ----------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def oracle_sequence(name):
    """frame 3 of the sequence of tests/temporal_cases.py from the oracle alone: oracle_trace over the screen rays of the
    four cameras, a seeded heavy-tailed noise plane as `indirect` (denoise_variance_cases.noise_indirect), accumulated by the temporal reference"""
    scene, cams, _ = tc.sequence(name)
    hist, g, acc = None, None, None
    for i, cam in enumerate(cams):
        rec = oracle_trace(scene.desc, screen_rays(cam, tc.W, tc.H))
        g = (rec["closest_node"].reshape(tc.H, tc.W), rec["normal"].reshape(tc.H, tc.W, 3), rec["p"].reshape(tc.H, tc.W, 3))
        indirect = vc.noise_indirect(oc.SEED + i, tc.H, tc.W)
        acc = tr.accumulate(*g, indirect, vc.MAX_AGE, tc.MIN_NORMAL_DOT, tc.MAX_PLANE_DIST, prev_cam=cams[i - 1] if i else None, history=hist)
        hist = acc["history"]
    return g, acc


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_gpu_comparison_is_not_vacuous(name):
    """Frame 3 of the sequences tests/test_gpu_denoise_variance.py filters, with min_age 3, holds at least 50 young hit
    pixels and at least 50 with a temporal variance; at sigma_lum 4 EACH of the levels 0, 1 and 2 halves at least 20 taps;
    and with the NaN, infinite, negative and zero variances of denoise_variance_cases.inject under TINY_FLOOR at least 20
    taps are dropped by the luminance term alone.  As measured, young / temporal, soft-lum taps of level 0 / 1 / 2, dropped:
      lecture5:   633 / 1685, 51 / 146 / 266, 21860
      csg_stress: 585 / 1637, 117 / 114 / 366, 16257"""
    g, acc = oracle_sequence(name)
    counts = {}
    vr.denoise_variance(*g, acc["colour"], acc["variance"], acc["age"], 3, 5, 1.0, sigma_lum=vc.SIGMA_LUM, var_floor=vc.VAR_FLOOR, min_age=vc.MIN_AGE,
                        counts=counts)
    print(name, counts)
    assert counts["young"] >= 50 and counts["temporal"] >= 50
    assert counts["young"] + counts["temporal"] == int((g[0] >= 0).sum())
    assert len(counts["levels"]) == 3 and sum(l["soft_lum"] for l in counts["levels"]) == counts["soft_lum"]
    for l in range(3):
        assert counts["levels"][l]["soft_lum"] >= 20, (l, counts)
    injected = {}
    vr.denoise_variance(*g, acc["colour"], vc.inject(acc["variance"], g[0]), acc["age"], 3, 5, 1.0, sigma_lum=vc.SIGMA_LUM, var_floor=vc.TINY_FLOOR,
                        min_age=vc.MIN_AGE, counts=injected)
    print(name, "injected", injected)
    assert injected["dropped_lum"] >= 20
