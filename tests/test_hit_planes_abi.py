"""Hit planes, CPU side: the ABI layout of c2rt_hit_planes as a C compiler sees it against the ctypes mirror, and the
Python face's table of planes.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

from chess2rt_amd import _abi
from chess2rt_amd.api import HIT_PLANES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["node", "leaf", "dist", "uv", "p", "normal", "rgb"]


def test_hit_planes_layout_matches_c(tmp_path):
    src = tmp_path / "h.c"
    lines = ['printf("size %zu\\n", sizeof(c2rt_hit_planes));']
    lines += ['printf("%s %%zu\\n", offsetof(c2rt_hit_planes, %s));' % (f, f) for f in FIELDS]
    lines.append('printf("abi %u\\n", (unsigned)C2RT_ABI_VERSION);')
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "c2rt.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    exe = tmp_path / "h"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_abi.HitPlanes) == 7 * C.sizeof(C.c_void_p)
    for f in FIELDS:
        assert int(got[f]) == getattr(_abi.HitPlanes, f).offset, f
    assert int(got["dist"]) == _abi.HitPlanes.dist.offset == 2 * C.sizeof(C.c_void_p)
    assert int(got["rgb"]) == _abi.HitPlanes.rgb.offset == 6 * C.sizeof(C.c_void_p)
    assert [name for name, _ in _abi.HitPlanes._fields_] == FIELDS
    assert int(got["abi"]) == _abi.ABI_VERSION == 1      # only entry points were added


def test_the_python_table_of_planes():
    assert list(HIT_PLANES) == FIELDS
    want = {"node": (np.int32, 1), "leaf": (np.int32, 1), "dist": (np.float64, 1), "uv": (np.float64, 2),
            "p": (np.float64, 3), "normal": (np.float64, 3), "rgb": (np.float32, 3)}
    assert HIT_PLANES == want
    # 92 bytes per pixel with every plane: what include/c2rt.h states for the host variant's staging
    assert sum(np.dtype(t).itemsize * c for t, c in HIT_PLANES.values()) == 92


def test_the_entry_points_are_exported():
    lib = _abi.load_library()
    for name in ("c2rt_render_hits", "c2rt_render_hits_device", "c2rt_host_render_hits"):
        assert getattr(lib, name) is not None
