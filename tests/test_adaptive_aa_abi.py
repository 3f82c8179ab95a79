"""Adaptive anti-aliasing, CPU side: the entry points and their ctypes tables, the threshold constant as a C compiler
sees it, and the typed numpy restatement of the edge test (tests/aa_reference.py) on hand-made images.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

from aa_reference import needs_aa, tile_counts
from chess2rt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_the_entry_points_are_exported_and_in_the_tables():
    lib = _abi.load_library()
    for name in ("c2rt_render_frame_adaptive", "c2rt_render_frame_adaptive_device"):
        assert getattr(lib, name) is not None
        assert name in _abi.C2RT_SYMBOLS
        restype, argtypes = _abi.C2RT_SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == 7 and argtypes[3] is C.c_float
    assert getattr(lib, "c2rt_host_render_rt_adaptive") is not None
    assert _abi.C2RT_HOST_SYMBOLS["c2rt_host_render_rt_adaptive"] == (C.c_int, [C.c_void_p] * 4)


def test_the_threshold_constant_as_gcc_prints_it(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "c2rt.h"\nint main(void) {\n'
                   'float t = C2RT_AA_THRESHOLD_REF;\nprintf("%a %zu %u\\n", (double)t, sizeof(C2RT_AA_THRESHOLD_REF), (unsigned)C2RT_ABI_VERSION);\nreturn 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    value, size, abi = subprocess.check_output([str(exe)], text=True).split()
    assert float.fromhex(value) == float(F(0.1))
    assert int(size) == 4                                  # a float constant, not a double
    assert F(_abi.AA_THRESHOLD_REF) == F(0.1)
    assert int(abi) == _abi.ABI_VERSION == 1               # only entry points were added


def grey(values):
    """(H, W, 3) float32 image with the same value in every channel"""
    v = np.asarray(values, dtype=np.float32)
    return np.ascontiguousarray(np.repeat(v[..., None], 3, axis=2))


def test_one_pixel_never_differs_from_itself():
    for v in (0.0, 0.25, 1.0, 1e30):
        assert needs_aa(grey([[v]])).tolist() == [[0]]
    assert needs_aa(grey([[0.7]]), 0.0).shape == (1, 1)


def test_a_single_bright_pixel_flags_the_cross_not_the_diagonals():
    img = np.zeros((3, 3), dtype=np.float32)
    img[1, 1] = 1.0
    assert needs_aa(grey(img)).tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    # one channel is enough
    one = np.zeros((3, 3, 3), dtype=np.float32)
    one[1, 1, 2] = 1.0
    assert needs_aa(one).tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    assert tile_counts(needs_aa(one)).tolist() == [5]


def test_borders_clamp_to_the_pixel_itself():
    # a bright corner: its missing neighbours are the corner itself, neighs of (0, 0) = {1, 1, 0, 1, 0}, average 0.6
    img = np.zeros((3, 3), dtype=np.float32)
    img[0, 0] = 1.0
    assert needs_aa(grey(img)).tolist() == [[1, 1, 0], [1, 0, 0], [0, 0, 0]]
    # clamped, the corner's largest difference is |0 - 0.6|; with black outside the frame the average would be 0.2 and
    # the largest difference |1 - 0.2| = 0.8: a threshold of 0.7 tells the two apart
    assert needs_aa(grey(img), 0.5)[0, 0] == 1
    assert needs_aa(grey(img), 0.7)[0, 0] == 0
    # the same along an edge, (0, 1) of a bright top row: neighs = {1, 1, 1, 1 (clamped), 0}, average 0.8
    img = np.zeros((3, 3), dtype=np.float32)
    img[0, :] = 1.0
    assert needs_aa(grey(img), 0.7)[0, 1] == 1            # |0 - 0.8|
    assert needs_aa(grey(img), 0.85)[0, 1] == 0           # ... is the largest difference
    # a uniform frame one pixel high or wide never flags
    assert not needs_aa(grey(np.full((1, 9), 0.8))).any()
    assert not needs_aa(grey(np.full((9, 1), 0.8))).any()


def test_the_comparison_is_greater_than():
    # pixel (0, 0) of a 3x3 image, neighs = {0, 0, a, 0, 0}: average = a / 5, largest difference fl(a - fl(a / 5)).
    # a = 0.125: that difference is exactly 0.1f, which does not flag; the next float above a does.
    a = F(0.125)
    diff = F(a - F(a / F(5.0)))
    assert diff == F(0.1), float(diff)
    img = np.zeros((3, 3), dtype=np.float32)
    img[0, 1] = a
    assert needs_aa(grey(img))[0, 0] == 0
    b = np.nextafter(a, F(1.0))
    assert F(b - F(b / F(5.0))) > F(0.1)
    img[0, 1] = b
    assert needs_aa(grey(img))[0, 0] == 1
    # the threshold is compared as fp32: 0.1 (a double) and 0.1f are the same threshold
    img[0, 1] = a
    assert needs_aa(grey(img), float(F(0.1)))[0, 0] == 0 and needs_aa(grey(img), 0.1)[0, 0] == 0


def test_nan_does_not_flag():
    img = np.zeros((3, 3), dtype=np.float32)
    img[1, 1] = np.nan
    # every pixel of the cross has a NaN average: every comparison is false
    assert not needs_aa(grey(img)).any()
    # infinities: the cross has an infinite average; |inf - inf| is NaN (no flag from the pixel itself), |0 - inf| flags
    img[1, 1] = np.inf
    got = needs_aa(grey(img))
    assert got.tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    # a NaN elsewhere in the image does not leak past the cross
    img = np.zeros((5, 5), dtype=np.float32)
    img[0, 0] = np.nan
    img[4, 4] = 1.0
    got = needs_aa(grey(img))
    assert got[:3, :3].sum() == 0 and got[4, 4] == 1 and got[3, 4] == 1 and got[4, 3] == 1 and got[3, 3] == 0


def test_the_sum_order_is_the_references():
    # ((((0 + n0) + n1) + n2) + n3) + n4 in fp32, n0 the pixel itself: with n0 = 2^24 and four ones every one is absorbed
    # (2^24 + 1 ties to even), so the sum is 2^24; summing the ones first, or in a wider type, gives 2^24 + 4.  The
    # pixel's own difference is 13421773 with the reference's average and 13421772 with the other: a threshold of
    # 13421772 tells them apart.
    big = F(2.0 ** 24)
    img = np.ones((3, 3), dtype=np.float32)
    img[1, 1] = big
    ref_sum = F(F(F(F(F(F(0.0) + big) + F(1.0)) + F(1.0)) + F(1.0)) + F(1.0))
    assert ref_sum == big
    ref_diff = F(big - F(ref_sum / F(5.0)))
    other_diff = F(big - F(F(big + F(4.0)) / F(5.0)))
    assert float(ref_diff) == 13421773.0 and float(other_diff) == 13421772.0
    assert needs_aa(grey(img), 13421772.0)[1, 1] == 1
    assert needs_aa(grey(img), 13421773.0)[1, 1] == 0
