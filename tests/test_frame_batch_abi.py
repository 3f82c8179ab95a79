"""The batch entry points (c2rt_render_frames, c2rt_render_frames_device) at the boundary: the plain-C example
compiles against include/c2rt.h and links libc2rt.so, the Python face has the methods, the diagnostics library
exports the symbols.  No compute calls (runs without a GPU)."""
import ctypes as C
import os
import subprocess

import chess2rt_amd as c2
from chess2rt_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_c_batch_caller_links_and_fails_loudly_without_gpu(tmp_path):
    import torch

    exe = str(tmp_path / "c_batch_demo")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_batch_demo.c"),
                           "-L", os.path.join(ROOT, "chess2rt_amd"), "-lc2rt", "-Wl,-rpath," + os.path.join(ROOT, "chess2rt_amd"),
                           "-lm", "-o", exe])
    p = subprocess.run([exe, "40", "24", "3"], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert p.returncode == 0, p.stdout + p.stderr
        assert p.stdout.count("equals the single frame") == 3 and "depth of field" in p.stdout
    else:
        assert p.returncode != 0 and "no usable GPU" in p.stderr


def test_python_face_has_the_batch_methods():
    assert callable(c2.Context.renderFrames) and callable(c2.Context.renderFramesDevice)
    for name in ("c2rt_render_frames", "c2rt_render_frames_device"):
        restype, argtypes = _abi.C2RT_SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == 6 and argtypes[2] is C.c_uint32


def test_diagnostics_library_exports_the_batch_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "chess2rt_amd", "libc2rt_diag.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert {"c2rt_render_frames", "c2rt_render_frames_device"} <= exported
