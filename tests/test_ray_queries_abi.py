"""Ray queries, CPU side: the ABI layout of the three records, and the entitlement of the GPU tests' reference — the
reference's trace() loop restated over orc_node_intersect reproduces orc_render_pixel's record.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as orc
from chess2rt_amd import _abi
from chess2rt_amd.api import RAY_HIT_DTYPE
from golden_configs import load_config
from ray_query_util import assert_records_match_oracle, oracle_trace, record_from_trace_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_struct_layouts_match_c(tmp_path):
    src = tmp_path / "q.c"
    fields = {"c2rt_ray": ["orig", "dir"], "c2rt_segment": ["from", "to"],
              "c2rt_ray_hit": ["closest_node", "leaf_geom", "dist", "u", "v", "p", "normal"]}
    lines = ['printf("%s %%zu\\n", sizeof(%s));' % (s, s) for s in fields]
    lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f) for s in fields for f in fields[s]]
    lines.append('printf("MAX_RAYS %llu\\n", (unsigned long long)C2RT_MAX_RAYS);')
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "c2rt.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    exe = tmp_path / "q"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    mirrors = {"c2rt_ray": _abi.Ray, "c2rt_segment": _abi.Segment, "c2rt_ray_hit": _abi.RayHit}
    for s, cls in mirrors.items():
        assert int(got[s]) == C.sizeof(cls), s
        for f in fields[s]:
            assert int(got["%s.%s" % (s, f)]) == getattr(cls, "from_" if f == "from" else f).offset, (s, f)
    assert (int(got["c2rt_ray"]), int(got["c2rt_segment"]), int(got["c2rt_ray_hit"])) == (48, 48, 80)
    assert int(got["MAX_RAYS"]) == _abi.MAX_RAYS == 1 << 28
    # the numpy face of c2rt_ray_hit
    assert RAY_HIT_DTYPE.itemsize == 80
    for f in fields["c2rt_ray_hit"]:
        assert RAY_HIT_DTYPE.fields[f][1] == int(got["c2rt_ray_hit.%s" % f]), f


def test_the_ray_oracle_is_the_references_trace_loop():
    """for node: orc_node_intersect over one OrcHit that starts at 1e99, fed orc_screen_ray rays, is
    orc_render_pixel's record: node, leaf, dist and p exactly, normal within 1e-15, u, v within 1e-12."""
    L = orc.lib()
    for name in ("lecture5_640x480_t1", "csg_stress_320x240_t1", "zaphod_645x430_t1"):
        scene, cam, opts = load_config(name)
        rng = np.random.RandomState(11)
        pts = [(int(rng.randint(0, opts.width)), int(rng.randint(0, opts.height))) for _ in range(300)]
        pts += [(0, 0), (opts.width - 1, 0), (0, opts.height - 1), (opts.width - 1, opts.height - 1)]
        rays = np.empty((len(pts), 6))
        want = np.zeros(len(pts), dtype=RAY_HIT_DTYPE)
        o, v = (C.c_double * 3)(), (C.c_double * 3)()
        for i, (x, y) in enumerate(pts):
            L.orc_screen_ray(C.byref(cam), float(x), float(y), o, v)
            rays[i] = list(o) + list(v)
            t = orc.render_pixel(scene.desc, cam, opts, x, y)
            assert list(t.ray_orig) == list(o) and list(t.ray_dir) == list(v)
            want[i] = record_from_trace_result(t)
        got = oracle_trace(scene.desc, rays)
        assert_records_match_oracle(got, want, name)
        hits = int((want["closest_node"] >= 0).sum())
        assert 0 < hits, name
