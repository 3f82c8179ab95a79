"""CPU half of the temporal tests: the numpy restatement itself (tests/temporal_reference.py) on cases worked out by hand,
the ABI's structs and the one entry point that needs no device, and the precondition of the GPU comparison — that the
camera pairs it compares put pixels and taps into every class of the reprojection."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import occlusion_cases as oc
import temporal_cases as tc
import temporal_reference as tr
from chess2rt_amd import _abi, temporal_history_bytes
from ray_query_util import oracle_trace, screen_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 8, 4                   # powers of two: every quotient of the reprojection below is exact
F = np.float32


def camera(x=0.0, y=0.0, z=0.0):
    """a camera at (x, y, z) looking along +z whose pixel (i, j) looks through (x + i, y + j, z + 1): over the plane at unit
    distance a pixel is one world unit wide, and every constant of the reprojection is a small integer — A = (0, 0, 1),
    U = (W, 0, 0), V = (0, H, 0), na = (0, 0, WH), nb = (H, 0, 0), nc = (0, W, 0), det = WH"""
    return dict(pos=(x, y, z), up_left=(x, y, z + 1.0), up_right=(x + W, y, z + 1.0), down_left=(x, y + H, z + 1.0))


def plane_guides(cam, node=0):
    """what that camera sees of the plane z = 1, facing it: p = (x + i, y + j, 1)"""
    js, is_ = np.mgrid[0:H, 0:W]
    p = np.stack([cam["pos"][0] + is_, cam["pos"][1] + js, np.ones_like(is_)], axis=-1).astype(np.float64)
    normal = np.zeros((H, W, 3))
    normal[..., 2] = -1.0
    return np.full((H, W), node, dtype=np.int32), normal, p


def images(n, channels=3, seed=1):
    rng = np.random.RandomState(seed)
    return [rng.uniform(0.0, 2.0, (H, W, channels)).astype(np.float32) for _ in range(n)]


def lum(img):
    return (F(0.2126) * img[..., 0] + F(0.7152) * img[..., 1]) + F(0.0722) * img[..., 2]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_constants_of_the_hand_camera():
    pos, na, nb, nc, det, Wd, Hd = tr.camera_constants(camera(), W, H)
    assert list(na) == [0, 0, W * H] and list(nb) == [H, 0, 0] and list(nc) == [0, W, 0] and det == W * H and (Wd, Hd) == (W, H)


@pytest.mark.parametrize("channels", [1, 3])
def test_same_camera_flat_plane_is_the_running_mean(channels):
    """every pixel finds itself (sx = x exactly: one tap of weight 1, h = (1 * c) / 1 = c), ages count 1, 2, 3 and stay at
    max_age = 3, and colour and moments are the running mean written out by hand, one fp32 operation at a time"""
    cam, ins = camera(), images(6, channels, seed=2)
    node, normal, p = plane_guides(cam)
    hist, c, m1, m2 = None, None, None, None
    for k, img in enumerate(ins):
        counts = {}
        got = tr.accumulate(node, normal, p, img, 3, 0.5, 0.25, prev_cam=cam if k else None, history=hist, counts=counts)
        l = lum(img) if channels == 3 else img[..., 0]
        if k == 0:
            c, m1, m2, age = img, l, l * l, 1
            assert counts["first"] == W * H
        else:
            age = min(k + 1, 3)
            a = F(1.0) / F(age)
            c = c + (img - c) * a
            m1 = m1 + (l - m1) * a
            m2 = m2 + (l * l - m2) * a
            assert counts["partial"] == W * H and counts["tap_kept"] == W * H and counts["tap_zero"] + counts["tap_outside"] == 3 * W * H
        v = m2 - m1 * m1
        assert (got["age"] == age).all()
        assert bits(got["colour"]).tobytes() == bits(c).tobytes(), k
        assert bits(got["variance"]).tobytes() == bits(np.where((k > 0) & (v > 0), v, F(0))).tobytes(), k
        hs = tr.split_history(got["history"], H, W, channels)
        assert bits(hs["c"]).tobytes() == bits(c).tobytes() and (hs["age"] == age).all() and (hs["node"] == 0).all()
        assert bits(hs["m"][..., 0]).tobytes() == bits(m1).tobytes() and bits(hs["m"][..., 1]).tobytes() == bits(m2).tobytes()
        assert np.array_equal(hs["pf"], p.astype(np.float32)) and np.array_equal(hs["nf"], normal.astype(np.float32))
        hist = got["history"]
    assert got["variance"].max() > 0
    with np.errstate(all="ignore"):
        two = tr.accumulate(node, normal, p, ins[1], 3, 0.5, 0.25, prev_cam=cam, history=tr.accumulate(node, normal, p, ins[0], 3, 0.5, 0.25)["history"])
    assert np.array_equal(two["colour"], ins[0] + (ins[1] - ins[0]) * F(0.5))             # the mean of two, exactly the formula


def first_history(cam, img, age=1, node=0):
    """the history a first frame leaves for `cam` over the plane, with every age set to `age`"""
    n, normal, p = plane_guides(cam, node)
    hs = tr.split_history(tr.accumulate(n, normal, p, img, tr.MAX_AGE, 0.5, 0.25)["history"], H, W, img.shape[2])
    return {k: v.copy() for k, v in hs.items()}, dict(age=np.full((H, W), age, dtype=np.uint32))


def join(hs, **kw):
    hs = dict(hs, **kw)
    return tr.join_history(hs["nf"], hs["node"], hs["pf"], hs["age"], hs["c"], hs["m"])


def test_camera_shifted_by_one_pixel_moves_the_history_by_one_pixel():
    """the camera moves one pixel's width along its right direction: pixel x now sees what pixel x + 1 saw, sx = x + 1; the
    last column has sx = W exactly, which is outside: it restarts at age 1"""
    prev, cur = camera(), camera(x=1.0)
    a, b = images(2, seed=3)
    hs, _ = first_history(prev, a)
    node, normal, p = plane_guides(cur)
    counts = {}
    got = tr.accumulate(node, normal, p, b, 8, 0.5, 0.25, prev_cam=prev, history=join(hs), counts=counts)
    assert counts["outside"] == H and counts["partial"] == (W - 1) * H
    assert (got["age"][:, :-1] == 2).all() and (got["age"][:, -1] == 1).all()
    want = a[:, 1:] + (b[:, :-1] - a[:, 1:]) * F(0.5)
    assert bits(got["colour"][:, :-1]).tobytes() == bits(want).tobytes()
    assert bits(got["colour"][:, -1]).tobytes() == bits(b[:, -1]).tobytes()
    assert (got["variance"][:, -1] == 0).all()


def test_half_pixel_shift_takes_two_taps_of_one_half():
    """sx = x + 0.5: taps x and x + 1 weigh 0.5 each, sumw = 1; in the last column the second tap is outside the frame and
    the first is renormalised: (0.5 c) / 0.5 = c.  The age is the smaller of the two taps' plus one."""
    prev, cur = camera(), camera(x=0.5)
    a, b = images(2, seed=4)
    hs, _ = first_history(prev, a)
    age = np.full((H, W), 5, dtype=np.uint32)
    age[:, 3] = 2
    node, normal, p = plane_guides(cur)
    counts = {}
    got = tr.accumulate(node, normal, p, b, 100, 0.5, 0.25, prev_cam=prev, history=join(hs, age=age), counts=counts)
    assert counts["partial"] == W * H and counts["tap_kept"] == 2 * W * H - H and counts["tap_zero"] + counts["tap_outside"] == 2 * W * H + H
    h = np.empty_like(a)
    h[:, :-1] = (F(0.5) * a[:, :-1] + F(0.5) * a[:, 1:]) / F(1.0)
    h[:, -1] = (F(0.5) * a[:, -1]) / F(0.5)
    n = np.full((H, W), 6, dtype=np.uint32)
    n[:, 2:4] = 3
    assert np.array_equal(got["age"], n)
    want = h + (b - h) * (F(1.0) / n.astype(np.float32))[..., None]
    assert bits(got["colour"]).tobytes() == bits(want).tobytes()


def test_rejected_taps_are_left_out_and_the_rest_renormalised():
    """half a pixel in x and y: four taps of 0.25.  Pixel (2, 1) fetches (2, 1), (3, 1), (2, 2), (3, 2): the second lies on
    another node, the third faces away, the fourth is off the plane — only the first counts, (0.25 c) / 0.25 = c, in the
    contract's order of tests"""
    prev, cur = camera(), camera(x=0.5, y=0.5)
    a, b = images(2, seed=5)
    hs, _ = first_history(prev, a)
    hs["node"][1, 3] = 7
    hs["nf"][2, 2] = (0.0, 0.0, 1.0)
    hs["pf"][2, 3] = (3.0, 2.0, 1.5)
    node, normal, p = plane_guides(cur)
    counts = {}
    got = tr.accumulate(node, normal, p, b, 8, 0.5, 0.25, prev_cam=prev, history=join(hs), counts=counts)
    h = (F(0.25) * a[1, 2]) / F(0.25)
    assert bits(got["colour"][1, 2]).tobytes() == bits(h + (b[1, 2] - h) * F(0.5)).tobytes()
    assert got["age"][1, 2] == 2
    untouched = (0, 0)                                   # taps (0, 0), (1, 0), (0, 1), (1, 1): all four kept
    q = ((F(0.25) * a[0, 0] + F(0.25) * a[0, 1]) + F(0.25) * a[1, 0]) + F(0.25) * a[1, 1]
    assert bits(got["colour"][untouched]).tobytes() == bits(q / F(1.0) + (b[untouched] - q / F(1.0)) * F(0.5)).tobytes()
    # (3, 1), (2, 2) and (3, 2) are each fetched by four pixels (all inside this frame)
    assert counts["tap_other"] == 4 and counts["tap_normal"] == 4 and counts["tap_plane"] == 4
    assert counts["full"] > 0 and counts["disoccluded"] == 0
    far = tr.accumulate(node, normal, p, b, 8, 0.5, 0.25, prev_cam=prev, history=join(hs, node=np.full((H, W), 9, dtype=np.int32)), counts=(c2 := {}))
    assert c2["disoccluded"] == W * H and (far["age"] == 1).all() and bits(far["colour"]).tobytes() == bits(b).tobytes()


def test_points_behind_the_previous_camera_and_at_its_eye_have_no_history():
    prev = camera()
    a, b = images(2, seed=6)
    hs, _ = first_history(prev, a)
    node, normal, p = plane_guides(prev)
    p[0, 0] = (0.0, 0.0, -1.0)                           # behind: ka = -WH
    p[0, 1] = (0.0, 0.0, 0.0)                            # the eye: ka = 0, and 0 / 0 behind it
    p[0, 2] = (np.nan, 0.0, 1.0)
    counts = {}
    got = tr.accumulate(node, normal, p, b, 8, 0.5, 0.25, prev_cam=prev, history=join(hs), counts=counts)
    assert counts["behind"] == 3
    assert list(got["age"][0, :4]) == [1, 1, 1, 2]
    assert bits(got["colour"][0, :3]).tobytes() == bits(b[0, :3]).tobytes()
    mirrored = dict(prev, up_right=prev["up_left"], up_left=prev["up_right"])          # det < 0: the sign of ka turns with it
    assert tr.camera_constants(mirrored, W, H)[4] < 0
    got = tr.accumulate(node, normal, p, b, 8, 0.5, 0.25, prev_cam=mirrored, history=join(hs), counts=(c2 := {}))
    assert c2["behind"] == 3 and got["age"][0, 3] == 2


def test_frame_edges_minus_one_and_width_are_outside():
    """sx exactly -1 and exactly W: NO HISTORY; just inside (-0.5, W - 0.5) one tap is in the frame and counts"""
    prev = camera()
    a, b = images(2, seed=7)
    hs, _ = first_history(prev, a)
    node, normal, p = plane_guides(prev)
    p[1, 0] = (-1.0, 1.0, 1.0)
    p[1, 1] = (float(W), 1.0, 1.0)
    p[1, 2] = (-0.5, 1.0, 1.0)
    p[1, 3] = (W - 0.5, 1.0, 1.0)
    p[2, 0] = (2.0, -1.0, 1.0)
    p[2, 1] = (2.0, float(H), 1.0)
    counts = {}
    got = tr.accumulate(node, normal, p, b, 8, 0.5, 0.25, prev_cam=prev, history=join(hs), counts=counts)
    assert counts["outside"] == 4
    assert list(got["age"][1, :4]) == [1, 1, 2, 2] and list(got["age"][2, :2]) == [1, 1]
    h = (F(0.5) * a[1, 0]) / F(0.5)
    assert bits(got["colour"][1, 2]).tobytes() == bits(h + (b[1, 2] - h) * F(0.5)).tobytes()
    h = (F(0.5) * a[1, W - 1]) / F(0.5)
    assert bits(got["colour"][1, 3]).tobytes() == bits(h + (b[1, 3] - h) * F(0.5)).tobytes()


def test_misses_pass_through_with_age_zero():
    prev = camera()
    a, b = images(2, seed=8)
    hs, _ = first_history(prev, a)
    node, normal, p = plane_guides(prev)
    node[1, 1:4] = -1
    b[1, 1] = (np.nan, np.inf, -0.0)
    for hist in (None, join(hs)):
        got = tr.accumulate(node, normal, p, b, 8, 0.5, 0.25, prev_cam=prev, history=hist)
        assert bits(got["colour"][1, 1:4]).tobytes() == bits(b[1, 1:4]).tobytes()
        assert (got["age"][1, 1:4] == 0).all() and (got["variance"][1, 1:4] == 0).all()
        out = tr.split_history(got["history"], H, W, 3)
        assert (out["node"][1, 1:4] == -1).all() and (bits(out["m"][1, 1:4]) == 0).all() and (out["age"][1, 1:4] == 0).all()
        assert np.isfinite(got["colour"][node >= 0]).all()              # a miss in the history is another node: its NaN reaches no hit


def test_age_saturates_without_wrapping():
    prev = camera()
    a, b = images(2, seed=9)
    hs, _ = first_history(prev, a)
    age = np.full((H, W), 65534, dtype=np.uint32)
    age[0, 0], age[0, 1], age[0, 2] = 65535, 0xFFFFFFFF, 0
    node, normal, p = plane_guides(prev)
    got = tr.accumulate(node, normal, p, b, tr.MAX_AGE, 0.5, 0.25, prev_cam=prev, history=join(hs, age=age))
    assert list(got["age"][0, :4]) == [65535, 65535, 1, 65535]
    assert bits(got["colour"][0, 2]).tobytes() == bits(a[0, 2] + (b[0, 2] - a[0, 2]) * F(1.0)).tobytes()
    assert bits(got["colour"][0, 3]).tobytes() == bits(a[0, 3] + (b[0, 3] - a[0, 3]) * (F(1.0) / F(65535.0))).tobytes()


def test_struct_layouts_match_c(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "c2rt.h"
int main(void) {
  printf("TemporalOpts %zu\\n", sizeof(c2rt_temporal_opts));
  printf("TemporalGuides %zu\\n", sizeof(c2rt_temporal_guides));
  printf("TemporalPlanes %zu\\n", sizeof(c2rt_temporal_planes));
  printf("opts.max_age %zu\\n", offsetof(c2rt_temporal_opts, max_age));
  printf("opts.max_plane_dist %zu\\n", offsetof(c2rt_temporal_opts, max_plane_dist));
  printf("opts.reserved %zu\\n", offsetof(c2rt_temporal_opts, reserved));
  printf("guides.p %zu\\n", offsetof(c2rt_temporal_guides, p));
  printf("planes.age %zu\\n", offsetof(c2rt_temporal_planes, age));
  printf("max_age %d\\n", C2RT_MAX_TEMPORAL_AGE);
  printf("abi %u\\n", C2RT_ABI_VERSION);
  return 0;
}
""")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert {k: int(v) for k, v in got.items()} == {
        "TemporalOpts": C.sizeof(_abi.TemporalOpts), "TemporalGuides": C.sizeof(_abi.TemporalGuides), "TemporalPlanes": C.sizeof(_abi.TemporalPlanes),
        "opts.max_age": _abi.TemporalOpts.max_age.offset, "opts.max_plane_dist": _abi.TemporalOpts.max_plane_dist.offset,
        "opts.reserved": _abi.TemporalOpts.reserved.offset, "guides.p": _abi.TemporalGuides.p.offset, "planes.age": _abi.TemporalPlanes.age.offset,
        "max_age": _abi.MAX_TEMPORAL_AGE, "abi": _abi.ABI_VERSION}
    assert C.sizeof(_abi.TemporalOpts) == 32 and C.sizeof(_abi.TemporalGuides) == 24 and C.sizeof(_abi.TemporalPlanes) == 24 and _abi.ABI_VERSION == 1
    assert _abi.MAX_TEMPORAL_AGE == tr.MAX_AGE == 65535


def test_history_bytes_is_host_arithmetic():
    """no context, no device: px * (32 + 4 * channels + 8), and zero for every refused option"""
    for w, h in ((1, 1), (61, 47), (1920, 1080), (65536, 3)):
        for ch in (1, 3):
            assert temporal_history_bytes(w, h, ch) == w * h * (32 + 4 * ch + 8) == tr.history_bytes(w, h, ch)
    ok = dict(width=8, height=8, channels=3, max_age=32, min_normal_dot=0.9, max_plane_dist=0.1)
    assert temporal_history_bytes(**ok) == 64 * 52
    assert temporal_history_bytes(**dict(ok, max_age=1)) > 0 and temporal_history_bytes(**dict(ok, max_age=65535, min_normal_dot=0.0)) > 0
    for bad in (dict(width=0), dict(height=0), dict(channels=0), dict(channels=2), dict(channels=4), dict(min_normal_dot=float("nan")),
                dict(min_normal_dot=float("inf")), dict(min_normal_dot=-0.1), dict(min_normal_dot=1.0), dict(max_plane_dist=float("nan")),
                dict(max_plane_dist=float("inf")), dict(max_plane_dist=0.0), dict(max_plane_dist=-1.0), dict(max_age=0), dict(max_age=65536)):
        assert temporal_history_bytes(**dict(ok, **bad)) == 0, bad
    lib = _abi.load_library()
    for reserved in ((1, 0), (0, 1)):
        o = _abi.TemporalOpts(width=8, height=8, channels=3, max_age=32, min_normal_dot=0.9, max_plane_dist=0.1, reserved=reserved)
        assert lib.c2rt_temporal_history_bytes(C.byref(o)) == 0
    assert lib.c2rt_temporal_history_bytes(None) == 0


@functools.lru_cache(maxsize=None)
def oracle_counts(name):
    """the classes of the first camera pair of tests/temporal_cases.py, from the oracle alone: oracle_trace over the screen
    rays of both cameras, frame 0's history from the reference, frame 1 against it"""
    scene, cams, _ = tc.sequence(name)
    g = []
    for cam in cams[:2]:
        rec = oracle_trace(scene.desc, screen_rays(cam, tc.W, tc.H))
        g.append((rec["closest_node"].reshape(tc.H, tc.W), rec["normal"].reshape(tc.H, tc.W, 3), rec["p"].reshape(tc.H, tc.W, 3)))
    zero = np.zeros((tc.H, tc.W, 3), dtype=np.float32)
    first = tr.accumulate(*g[0], zero, 8, tc.MIN_NORMAL_DOT, tc.MAX_PLANE_DIST)
    counts = {}
    tr.accumulate(*g[1], zero, 8, tc.MIN_NORMAL_DOT, tc.MAX_PLANE_DIST, prev_cam=cams[0], history=first["history"], counts=counts)
    return counts


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_gpu_comparison_is_not_vacuous(name):
    """The first camera pair of the sequences tests/test_gpu_temporal.py compares (the shipped camera, then moveCamera(10,
    2, 5) and rotateCamera(8, 0, 3); min_normal_dot 0.9, max_plane_dist 0.1) puts at least 50 of the 2867 pixels into each
    of: all four taps kept, one to three kept, disoccluded, reprojected outside the frame, miss — and at least 20 taps
    into each of the three rejections.  ONE pair fills every class on both scenes.  Recomputed here from the oracle alone;
    as measured, full / partial / disoccluded / outside / miss and other node / normal / plane:
      lecture5:   1795 / 448 / 168 / 212 / 244 and 693 / 156 / 692
      csg_stress: 1761 / 470 / 94 / 254 / 288 and 480 / 150 / 738"""
    counts = oracle_counts(name)
    print(name, counts)
    for k in ("full", "partial", "disoccluded", "outside", "miss"):
        assert counts[k] >= 50, (k, counts)
    for k in ("tap_other", "tap_normal", "tap_plane"):
        assert counts[k] >= 20, (k, counts)
    want = {"lecture5": (1795, 448, 168, 212, 244, 693, 156, 692), "csg_stress": (1761, 470, 94, 254, 288, 480, 150, 738)}[name]
    assert tuple(counts[k] for k in ("full", "partial", "disoccluded", "outside", "miss", "tap_other", "tap_normal", "tap_plane")) == want
    assert sum(counts[k] for k in tr.PIXEL_CLASSES) == tc.W * tc.H
    assert sum(counts[k] for k in tr.TAP_CLASSES) == 4 * (counts["full"] + counts["partial"] + counts["disoccluded"])
