"""CPU half of the counted path planes and the path counts: the new symbols and struct sizes, the one entry point that
needs no device, every refusal a null context reaches, the count rule of tests/path_counts_reference.py on histories made
by hand, and its tie to tests/temporal_reference.py — the two restate the same reprojection and must agree on the age."""
import ctypes as C
import os
import subprocess

import numpy as np

import path_counts_reference as cr
import temporal_reference as tr
from chess2rt_amd import _abi, paths_counted_scratch_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 8, 4                   # powers of two: every quotient of the reprojection below is exact
F = np.float32
NEW = ("c2rt_paths_counted_scratch_bytes", "c2rt_render_paths_counted_device", "c2rt_render_paths_counted", "c2rt_trace_rays_paths_counted_device",
       "c2rt_trace_rays_paths_counted", "c2rt_path_counts_device", "c2rt_path_counts", "c2rt_render_paths_sequence_adaptive")


def test_symbols_and_struct_sizes(tmp_path):
    lib = _abi.load_library()
    for name in NEW:
        assert name in _abi.C2RT_SYMBOLS and getattr(lib, name) is not None, name
    src = tmp_path / "sizes.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "c2rt.h"
int main(void) {
  printf("PathCountOpts %zu\\n", sizeof(c2rt_path_count_opts));
  printf("young_paths %zu\\n", offsetof(c2rt_path_count_opts, young_paths));
  printf("paths_per_variance %zu\\n", offsetof(c2rt_path_count_opts, paths_per_variance));
  printf("prev_paths %zu\\n", offsetof(c2rt_path_count_opts, prev_paths));
  printf("reserved %zu\\n", offsetof(c2rt_path_count_opts, reserved));
  printf("PathOpts %zu\\n", sizeof(c2rt_path_opts));
  printf("PathPlanes %zu\\n", sizeof(c2rt_path_planes));
  return 0;
}
""")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())}
    o = _abi.PathCountOpts
    assert got == {"PathCountOpts": C.sizeof(o), "young_paths": o.young_paths.offset, "paths_per_variance": o.paths_per_variance.offset,
                   "prev_paths": o.prev_paths.offset, "reserved": o.reserved.offset, "PathOpts": C.sizeof(_abi.PathOpts),
                   "PathPlanes": C.sizeof(_abi.PathPlanes)}
    assert C.sizeof(o) == 32 and got["PathOpts"] == 16 and got["PathPlanes"] == 40


def test_scratch_bytes_is_host_arithmetic():
    """no context, no device: a head of 512 bytes, then one index of 32 bits per sample, rounded up to 16"""
    for n, want in ((0, 512), (1, 528), (4, 528), (5, 544), (61 * 47, 512 + 11472), (2000, 8512), (1920 * 1080, 512 + 4 * 1920 * 1080),
                    ((1 << 28), 512 + (1 << 30)), ((1 << 32) + 3, 512 + (1 << 34) + 16)):
        assert paths_counted_scratch_bytes(n) == want == 512 + -(-4 * n // 16) * 16, n


def test_a_null_context_is_refused_by_every_call():
    L = _abi.load_library()
    cam, opts, g, pl = _abi.CameraFrame(), _abi.RenderOpts(), _abi.PathOpts(seed=1, paths=4, bounces=2), _abi.PathPlanes()
    counts = np.zeros(64, dtype=np.uint8)
    rays = np.zeros((64, 6))
    cp, rp = counts.ctypes.data_as(C.c_void_p), rays.ctypes.data_as(C.c_void_p)
    E = _abi.ERR_INVALID_ARG
    assert L.c2rt_render_paths_counted(None, C.byref(cam), C.byref(opts), C.byref(g), cp, C.byref(pl)) == E
    assert L.c2rt_render_paths_counted_device(None, C.byref(cam), C.byref(opts), C.byref(g), cp, C.byref(pl), None, None) == E
    assert L.c2rt_trace_rays_paths_counted(None, rp, 64, C.byref(g), cp, C.byref(pl)) == E
    assert L.c2rt_trace_rays_paths_counted_device(None, rp, 64, C.byref(g), cp, C.byref(pl), None, None) == E
    assert L.c2rt_trace_rays_paths_counted(None, rp, 0, C.byref(g), cp, C.byref(pl)) == E               # before n == 0
    tg, t, pc = _abi.TemporalGuides(), _abi.TemporalOpts(), _abi.PathCountOpts()
    assert L.c2rt_path_counts(None, None, C.byref(tg), C.byref(t), C.byref(pc), None, None, cp, None, None) == E
    assert L.c2rt_path_counts_device(None, None, C.byref(tg), C.byref(t), C.byref(pc), None, None, cp, None, None, None) == E
    dv = _abi.DenoiseVarianceOpts()
    assert L.c2rt_render_paths_sequence_adaptive(None, C.byref(cam), 1, C.byref(opts), C.byref(g), C.byref(t), C.byref(dv), C.byref(pc), cp) == E


# ---- the count rule on histories made by hand ------------------------------------------------------------------------------


def camera(x=0.0, y=0.0, z=0.0):
    """tests/test_temporal_abi.py's camera: at (x, y, z) looking along +z, pixel (i, j) through (x + i, y + j, z + 1)"""
    return dict(pos=(x, y, z), up_left=(x, y, z + 1.0), up_right=(x + W, y, z + 1.0), down_left=(x, y + H, z + 1.0))


def plane_guides(cam, node=0):
    """what that camera sees of the plane z = 1, facing it: p = (x + i, y + j, 1)"""
    js, is_ = np.mgrid[0:H, 0:W]
    p = np.stack([cam["pos"][0] + is_, cam["pos"][1] + js, np.ones_like(is_)], axis=-1).astype(np.float64)
    normal = np.zeros((H, W, 3))
    normal[..., 2] = -1.0
    return np.full((H, W), node, dtype=np.int32), normal, p


def history(cam, m1, m2, age, node=0):
    """the history of the plane seen by `cam` whose moments and ages are the (H, W) arrays given (colour: zeros)"""
    n, normal, p = plane_guides(cam, node)
    return tr.join_history(normal.astype(F), n, p.astype(F), np.broadcast_to(np.asarray(age, dtype=np.uint32), (H, W)),
                           np.zeros((H, W, 3), dtype=F), np.stack([np.broadcast_to(F(m1), (H, W)), np.broadcast_to(F(m2), (H, W))], axis=-1))


RULE = dict(min_paths=2, max_paths=32, young_paths=16, min_age=3, paths_per_variance=2.0, prev_paths=4)


def counts_of(guides, cam, hist, prev_counts=None, classes=None, **kw):
    return cr.path_counts(*guides, 3, 0.5, 0.25, prev_cam=cam, history=hist, prev_counts=prev_counts, classes=classes, **dict(RULE, **kw))


def test_count_rule_on_hand_made_histories():
    """the same camera over the flat plane: every pixel finds itself through one tap of weight 1, so m1 = M1, m2 = M2
    and v = M2 - M1 * M1 exactly; with M1 = 0, cprev = 4 and paths_per_variance = 2: t = 8 * M2"""
    cam = camera()
    g = plane_guides(cam)
    m1, m2, age = np.zeros((H, W), dtype=F), np.zeros((H, W), dtype=F), np.full((H, W), 5, dtype=np.uint32)
    g[0][0, 0] = -1                                       # a miss
    age[0, 1] = 2                                         # young: below min_age 3
    m1[0, 2], m2[0, 2] = 1.0, 1.0                         # v = 0: min_paths
    m2[0, 3] = 0.5                                        # t = 4 exactly: no round-up
    m2[0, 4] = np.nextafter(F(0.5), F(1.0))               # t just above 4: 5
    m2[0, 5] = 4.0                                        # t = 32 = max_paths: !(t < max)
    m2[0, 6] = 1000.0                                     # far above
    m2[0, 7] = np.nan                                     # a NaN moment: max_paths
    m2[1, 0] = np.inf
    m1[1, 1] = np.nan
    m2[1, 2] = 0.125                                      # t = 1: below min_paths
    m1[1, 3], m2[1, 3] = 2.0, 3.0                         # v = -1: clamped to +0, min_paths
    m2[1, 4] = 3.9                                        # t = 31.2: 32 by the round-up, below max all the same
    age[1, 5] = 3                                         # exactly min_age: old enough
    m2[1, 5] = 1.0
    hist = history(cam, m1, m2, age)
    classes = {}
    got = counts_of(g, cam, hist, classes=classes)
    c, v, a = got["counts"], got["variance"], got["age"]
    assert c.dtype == np.uint8 and v.dtype == F and a.dtype == np.uint32
    assert (c[0, 0], a[0, 0]) == (0, 0) and v[0, 0].view(np.uint32) == 0
    assert (c[0, 1], a[0, 1]) == (16, 2) and v[0, 1].view(np.uint32) == 0
    assert list(c[0, 2:8]) == [2, 4, 5, 32, 32, 32] and list(c[1, 0:6]) == [32, 32, 2, 2, 32, 8]
    assert (a.reshape(-1)[2:] == age.reshape(-1)[2:]).all()
    assert v[0, 3] == F(0.5) and v[0, 2].view(np.uint32) == 0 and v[1, 3].view(np.uint32) == 0 and np.isnan(v[0, 7]) and np.isnan(v[1, 1]) and np.isinf(v[1, 0])
    assert (c[2:] == 2).all() and (v[2:].view(np.uint32) == 0).all()                   # everything else: v = 0
    assert classes["miss"] == 1 and classes["young"] == 1 and classes["at_max"] == 6 and classes["between"] == 3 and classes["no_history"] == 0
    assert sum(classes.values()) == W * H
    # no history at all, and a history on another node: young_paths, age 0
    for hist_, cam_ in ((None, None), (history(cam, m1, m2, age, node=7), cam)):
        got = counts_of(g, cam_, hist_, classes=(cl := {}))
        assert (got["counts"].reshape(-1)[1:] == 16).all() and got["counts"][0, 0] == 0 and not got["age"].any() and not got["variance"].view(np.uint32).any()
        assert cl["no_history"] == W * H - 1 and cl["miss"] == 1
    # min_age 0: a tap of age 0 is old enough
    assert counts_of(g, cam, history(cam, m1, m2, 0), min_age=0)["counts"][0, 3] == 4


def test_cprev_is_the_largest_count_among_the_kept_taps():
    """half a pixel to the right: pixel x gathers taps x and x + 1, half each.  With M1 = 0 and M2 = 0.5 everywhere
    v = 0.5 and t = 0.5 * cprev * 2 = cprev"""
    prev, cur = camera(), camera(x=0.5)
    g = plane_guides(cur)
    hs = history(prev, 0.0, 0.5, 5)
    given = np.full((H, W), 3, dtype=np.uint8)
    given[0, 2] = 9                                       # seen by pixels (1, 0) and (2, 0)
    given[1, 4] = 0                                       # a zero beside a 3: the 3
    given[2, :] = 0                                       # zeros alone: cprev = 1, t = 1, min_paths
    given[3, 7] = 200                                     # beyond any count: t = 200, max_paths
    got = counts_of(g, prev, hs, prev_counts=given)["counts"]
    assert list(got[0]) == [3, 9, 9, 3, 3, 3, 3, 3] and list(got[1]) == [3] * 8 and list(got[2]) == [2] * 8 and list(got[3]) == [3] * 6 + [32, 32]
    # one of the two taps dropped (another node): its count no longer reaches the pixel
    hs2 = tr.split_history(hs.copy(), H, W, 3)
    hs2["node"][0, 2] = 7
    got = counts_of(g, prev, tr.join_history(hs2["nf"], hs2["node"], hs2["pf"], hs2["age"], hs2["c"], hs2["m"]), prev_counts=given)["counts"]
    assert list(got[0][:4]) == [3, 3, 3, 3]
    # prev_counts null: prev_paths behind every tap
    assert (counts_of(g, prev, hs)["counts"] == 4).all() and (counts_of(g, prev, hs, prev_paths=7)["counts"] == 7).all()


def test_age_is_the_accumulations_age_minus_one():
    """the tie to tests/temporal_reference.py on a moving pair: the camera moves half a pixel right and down over a
    history of mixed ages, nodes and normals, so that pixels keep four, some and no taps.  Wherever the accumulation reports
    an age strictly between 1 and max_age the rule's age is that minus one, and it is 0 exactly where the accumulation
    restarts (age 1) or misses (age 0)"""
    prev, cur = camera(), camera(x=0.5, y=0.5)
    rng = np.random.RandomState(5)
    img = rng.uniform(0.0, 2.0, (H, W, 3)).astype(F)
    n0, normal0, p0 = plane_guides(prev)
    hs = tr.split_history(tr.accumulate(n0, normal0, p0, img, tr.MAX_AGE, 0.5, 0.25)["history"].copy(), H, W, 3)
    hs["age"][...] = rng.randint(1, 9, (H, W))
    hs["age"][0:2, 0:3] = 7                               # pixels (0, 0) and (1, 0) gather nothing younger: saturated
    hs["node"][1, 3] = 7
    hs["node"][2, 5:] = 7
    hs["node"][3, 5:] = 7
    hs["nf"][2, 2] = (0.0, 0.0, 1.0)
    hist = tr.join_history(hs["nf"], hs["node"], hs["pf"], hs["age"], hs["c"], hs["m"])
    node, normal, p = plane_guides(cur)
    node[0, 7] = -1
    max_age = 6
    acc = tr.accumulate(node, normal, p, img, max_age, 0.5, 0.25, prev_cam=prev, history=hist)["age"]
    got = counts_of((node, normal, p), prev, hist, classes=(cl := {}))["age"]
    mid = (acc > 1) & (acc < max_age)
    assert mid.sum() >= 8 and (acc == 1).sum() >= 2 and (acc == max_age).sum() >= 2 and (acc == 0).sum() == 1
    assert (got[mid] == acc[mid] - 1).all()
    assert np.array_equal(got == 0, acc <= 1)
    assert (got[acc == max_age] >= max_age - 1).all()
    assert cl["no_history"] == (acc == 1).sum() and cl["miss"] == 1
