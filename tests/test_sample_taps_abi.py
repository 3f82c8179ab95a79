"""Sample tables, CPU side: the ABI (a C program against the headers, the six entry points refusing a null context), the
ctypes mirror, the two table helpers of the Python face, and the preconditions of the GPU tests' adaptive cases, asserted
on the oracle alone.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_reference as cr
import chess2rt_amd as c2
import oracle_lib as orc
import sample_taps_cases as tc
from aa_reference import needs_aa, tile_counts
from chess2rt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_PROGRAM = r"""
#include <stddef.h>
#include <stdint.h>
#include "c2rt.h"
#include "c2rt_host.h"
_Static_assert(sizeof(c2rt_tap_table) == 264, "c2rt_tap_table");
_Static_assert(offsetof(c2rt_tap_table, n) == 0 && offsetof(c2rt_tap_table, reserved) == 4 && offsetof(c2rt_tap_table, offset) == 8,
               "c2rt_tap_table members");
_Static_assert(C2RT_MAX_SAMPLE_TAPS == 16, "a 4x4 grid");
_Static_assert(sizeof(((c2rt_tap_table *)0)->offset) == 16 * 2 * sizeof(double), "offset[C2RT_MAX_SAMPLE_TAPS][2]");
_Static_assert(C2RT_ABI_VERSION == 1, "the sample tables are additive");
/* the prototypes, as the issue states them */
static int (*const p_frame_dev)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, const c2rt_tap_table *, float *,
                                void *) = c2rt_render_frame_taps_device;
static int (*const p_frame)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, const c2rt_tap_table *, float *) = c2rt_render_frame_taps;
static int (*const p_adaptive_dev)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, const c2rt_tap_table *, float, float *,
                                   uint8_t *, void *) = c2rt_render_frame_adaptive_taps_device;
static int (*const p_adaptive)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_render_opts *, const c2rt_tap_table *, float, float *,
                               uint8_t *, const volatile uint8_t *) = c2rt_render_frame_adaptive_taps;
static int (*const p_host)(c2rt_ctx *, c2rt_host_scene *, const c2rt_tap_table *, float *) = c2rt_host_render_rt_taps;
static int (*const p_host_adaptive)(c2rt_ctx *, c2rt_host_scene *, const c2rt_tap_table *, float *, uint8_t *) = c2rt_host_render_rt_adaptive_taps;
/* the members' types */
static uint32_t *n_of(c2rt_tap_table *t) { return &t->n; }
static uint32_t *reserved_of(c2rt_tap_table *t) { return &t->reserved; }
static double (*offset_of(c2rt_tap_table *t))[2] { return t->offset; }
int table_size(void)
{
    c2rt_tap_table t = {0};
    return (int)sizeof t + (*n_of(&t) || *reserved_of(&t) || offset_of(&t)[15][1] != 0);
}
void null_context(int *st)
{
    c2rt_camera_frame cam = {{0}};
    c2rt_render_opts opts = {0};
    c2rt_tap_table taps = {2, 0, {{0, 0}, {0.5, 0.5}}};
    float rgb[3];
    uint8_t flag;
    st[0] = p_frame_dev(NULL, &cam, &opts, &taps, rgb, NULL);
    st[1] = p_frame(NULL, &cam, &opts, &taps, rgb);
    st[2] = p_adaptive_dev(NULL, &cam, &opts, &taps, C2RT_AA_THRESHOLD_REF, rgb, &flag, NULL);
    st[3] = p_adaptive(NULL, &cam, &opts, &taps, C2RT_AA_THRESHOLD_REF, rgb, &flag, NULL);
    st[4] = p_host(NULL, NULL, &taps, rgb);
    st[5] = p_host_adaptive(NULL, NULL, &taps, rgb, &flag);
}
"""


def test_header_layout_and_null_context(tmp_path):
    src = tmp_path / "sample_taps.c"
    src.write_text(C_PROGRAM)
    so = tmp_path / "libsample_taps_probe.so"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)])
    lib = _abi.load_library()                # RTLD_GLOBAL: the probe's undefined symbols resolve to libc2rt.so's
    probe = C.CDLL(str(so))
    assert probe.table_size() == 264
    st = (C.c_int * 6)(*([-1] * 6))
    probe.null_context(st)
    assert list(st) == [_abi.ERR_INVALID_ARG] * 6
    for name in ("c2rt_render_frame_taps_device", "c2rt_render_frame_taps", "c2rt_render_frame_adaptive_taps_device", "c2rt_render_frame_adaptive_taps"):
        assert name in _abi.C2RT_SYMBOLS and hasattr(lib, name)
    for name in ("c2rt_host_render_rt_taps", "c2rt_host_render_rt_adaptive_taps"):
        assert name in _abi.C2RT_HOST_SYMBOLS and hasattr(lib, name)
    assert _abi.C2RT_SYMBOLS["c2rt_render_frame_adaptive_taps"][1][4] is C.c_float
    assert _abi.C2RT_SYMBOLS["c2rt_render_frame_adaptive_taps_device"][1][4] is C.c_float
    assert _abi.ABI_VERSION == 1


def test_tap_table_has_the_c_layout():
    assert C.sizeof(_abi.TapTable) == 264
    assert [(f[0], getattr(_abi.TapTable, f[0]).offset) for f in _abi.TapTable._fields_] == [("n", 0), ("reserved", 4), ("offset", 8)]
    assert _abi.MAX_SAMPLE_TAPS == 16
    t = _abi.TapTable()
    assert len(t.offset) == 16 and len(t.offset[0]) == 2
    t.offset[3][1] = 0.75                    # [tap][axis], row-major: tap 3's y is double number 7 behind the header
    raw = np.frombuffer(bytes(t), dtype=np.float64)
    assert raw[1 + 2 * 3 + 1] == 0.75 and np.count_nonzero(raw) == 1
    assert c2.TapTable is _abi.TapTable


def test_tap_grid():
    for k in (1, 2, 3, 4):
        g = c2.tap_grid(k)
        assert len(g) == k * k and g[0] == (0.0, 0.0)
        for s, (dx, dy) in enumerate(g):
            assert isinstance(dx, float) and isinstance(dy, float)
            assert dx == float(s % k) / float(k) and dy == float(s // k) / float(k), (k, s)
    assert c2.tap_grid(4)[5] == (0.25, 0.25) and c2.tap_grid(4)[15] == (0.75, 0.75) and c2.tap_grid(3)[5] == (2.0 / 3.0, 1.0 / 3.0)
    for bad in (0, 5):
        with pytest.raises(ValueError):
            c2.tap_grid(bad)
    assert tc.GRID16 == c2.tap_grid(4) and len(tc.GRID16) == _abi.MAX_SAMPLE_TAPS


def test_the_references_table():
    assert tuple(c2.TAPS_REF5_TABLE) == tuple(cr.AA_KERNEL)
    assert len(c2.TAPS_REF5_TABLE) == _abi.TAPS_REF5


def test_tables_reach_the_struct_as_given():
    from chess2rt_amd.api import _tap_table

    t = _tap_table(tc.ODD7)
    assert t.n == 7 and t.reserved == 0
    assert [(t.offset[s][0], t.offset[s][1]) for s in range(7)] == list(tc.ODD7)
    assert all(t.offset[s][0] == 0 and t.offset[s][1] == 0 for s in range(7, 16))
    assert _tap_table(t) is t
    # a sequence the struct cannot hold keeps its count: the library refuses it, not Python
    assert _tap_table([(0.0, 0.0)] * 17).n == 17
    assert tc.ODD7[0] == (0.0, 0.0) and tc.GRID16[0] == (0.0, 0.0) and tc.REF5[0] == (0.0, 0.0) and tc.SHIFT2[0] != (0.0, 0.0)


# ---- the preconditions of the GPU tests' adaptive cases, on the oracle alone ----------------------------------------------


@pytest.mark.parametrize("scene_file,width,height", tc.ADAPTIVE, ids=tc.ADAPTIVE_IDS)
def test_the_adaptive_cases_flag_a_share_and_tiles_of_both_kinds(scene_file, width, height):
    """the oracle's one-tap frame under the reference's edge test: 2 .. 90 % flagged (what the adaptive suite asserts of the
    device's frames), a tile with 1 .. 4 flags (15 k items at 16 taps fit one round of 64 lanes) and a tile with 5 or
    more (several rounds); the refinement kernel goes in passes of at most 8 taps, so also a tile with 9 or more, whose
    8 k items of one pass take several rounds"""
    scene, cam, opts = tc.make_scene(scene_file, width, height)
    one = orc.render_frame(scene.desc, cam, opts)
    mask = needs_aa(one, _abi.AA_THRESHOLD_REF)
    share = float(mask.mean())
    k = tile_counts(mask)
    one_round, several, per_pass = int(((k >= 1) & (k <= 4)).sum()), int((k >= 5).sum()), int((k >= 9).sum())
    print("%s %dx%d: flagged share %.4f, tiles with 1..4 / 5.. / 9.. flags: %d / %d / %d" % (scene_file, width, height, share, one_round, several, per_pass))
    assert 0.02 <= share <= 0.90, share
    assert one_round >= 1 and several >= 1 and per_pass >= 1, (one_round, several, per_pass)
    assert 15 * 4 <= 64 < 15 * 5 and 8 * 8 <= 64 < 8 * 9


def test_the_threshold_zero_case_has_full_tiles():
    """lecture5 at 24x17 under threshold 0: tiles with all 64 pixels flagged — 960 items, 15 rounds, at 16 taps (a pass of 8
    taps and one of 7: 8 + 7 full rounds)"""
    scene, cam, opts = tc.make_scene(*tc.FULL_TILES)
    k = tile_counts(needs_aa(orc.render_frame(scene.desc, cam, opts), 0.0))
    assert int((k == 64).sum()) >= 1, k.tolist()
    assert 15 * 64 == 960 and 960 // 64 == 15
