"""Adaptive anti-aliasing for batches, CPU side: the four entry points (c2rt_render_frames_adaptive[_device],
c2rt_render_frames_posed_adaptive[_device]) are exported by both libraries, declared in include/c2rt.h as a C compiler
reads it, in the ctypes tables, and have their Context methods.  No compute calls (runs without a GPU)."""
import ctypes as C
import inspect
import os
import subprocess

import chess2rt_amd as c2
from chess2rt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ("c2rt_render_frames_adaptive", "c2rt_render_frames_adaptive_device")
POSED = ("c2rt_render_frames_posed_adaptive", "c2rt_render_frames_posed_adaptive_device")


def exported(library):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "chess2rt_amd", library)],
                         capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.split()}


def test_both_libraries_export_the_four_symbols():
    for library in ("libc2rt.so", "libc2rt_diag.so"):
        assert set(PLAIN + POSED) <= exported(library), library
    lib = _abi.load_library()
    for name in PLAIN + POSED:
        assert getattr(lib, name) is not None


def test_the_header_declares_them_as_a_c_compiler_reads_it(tmp_path):
    """assigning each entry point to a pointer of the documented type compiles without a warning only if the header's
    prototype is that type"""
    src = tmp_path / "t.c"
    src.write_text('''#include <stdio.h>
#include "c2rt.h"
typedef int (*dev_fn)(c2rt_ctx *, const c2rt_camera_frame *, uint32_t, const c2rt_render_opts *, float, float *, uint8_t *, void *);
typedef int (*host_fn)(c2rt_ctx *, const c2rt_camera_frame *, uint32_t, const c2rt_render_opts *, float, float *, uint8_t *, const volatile uint8_t *);
typedef int (*posed_dev_fn)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_scene_pose *, uint32_t, const c2rt_render_opts *, float, float *, uint8_t *, void *);
typedef int (*posed_host_fn)(c2rt_ctx *, const c2rt_camera_frame *, const c2rt_scene_pose *, uint32_t, const c2rt_render_opts *, float, float *, uint8_t *, const volatile uint8_t *);
int main(void) {
    dev_fn a = c2rt_render_frames_adaptive_device;
    host_fn b = c2rt_render_frames_adaptive;
    posed_dev_fn c = c2rt_render_frames_posed_adaptive_device;
    posed_host_fn d = c2rt_render_frames_posed_adaptive;
    /* n_frames = 0 is C2RT_OK before anything is read; a null context is refused */
    printf("%d %d %d %d %u\\n", a(NULL, NULL, 0, NULL, 0.1f, NULL, NULL, NULL), b(NULL, NULL, 0, NULL, 0.1f, NULL, NULL, NULL),
           c(NULL, NULL, NULL, 0, NULL, 0.1f, NULL, NULL, NULL), d(NULL, NULL, NULL, 0, NULL, 0.1f, NULL, NULL, NULL), (unsigned)C2RT_ABI_VERSION);
    return 0;
}
''')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", os.path.join(ROOT, "chess2rt_amd"), "-lc2rt", "-Wl,-rpath," + os.path.join(ROOT, "chess2rt_amd"), "-o", str(exe)])
    got = subprocess.check_output([str(exe)], text=True).split()
    assert [int(v) for v in got[:4]] == [_abi.ERR_INVALID_ARG] * 4      # the null context
    assert int(got[4]) == _abi.ABI_VERSION == 1                        # only entry points were added


def test_the_ctypes_tables_hold_them():
    for name in PLAIN:
        restype, argtypes = _abi.C2RT_SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == 8 and argtypes[2] is C.c_uint32 and argtypes[4] is C.c_float, name
    for name in POSED:
        restype, argtypes = _abi.C2RT_SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == 9 and argtypes[3] is C.c_uint32 and argtypes[5] is C.c_float, name
        assert argtypes[2] is _abi.C2RT_SYMBOLS["c2rt_render_frames_posed"][1][2]


def test_the_context_has_the_four_methods():
    for name, leading in (("renderFramesAdaptive", ["self", "cams", "opts"]), ("renderFramesAdaptiveDevice", ["self", "cams", "opts", "out_ptr", "mask_ptr"]),
                          ("renderFramesPosedAdaptive", ["self", "cams", "poses", "opts"]),
                          ("renderFramesPosedAdaptiveDevice", ["self", "cams", "poses", "opts", "out_ptr", "mask_ptr"])):
        method = getattr(c2.Context, name)
        params = inspect.signature(method).parameters
        assert list(params)[:len(leading)] == leading, name
        assert params["threshold"].default == _abi.AA_THRESHOLD_REF, name
        assert ("stream" in params) == name.endswith("Device") and ("stop_flag" in params) != name.endswith("Device"), name
