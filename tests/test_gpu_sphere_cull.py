"""The sphere-silhouette test of the mask pre-pass on the device (chess2rt_amd/csrc/csg_void.h: cone_misses_ball,
c2rt_tile_mask.inc: tile_mask_entry).

Through the diagnostics hooks (tests/sphere_cull_device.py) the device's drops equal the host classifier's claims
tile for tile — the classifier tests/test_sphere_cull_tiles.py checks ray by ray in the oracle —, the table with the
switch off passes the CsgDiff void test's own device comparison (tests/csg_void_device.py: the pre-pass as it was
before the sphere test), and full frames of lecture5 are bit-equal with the switch on and off."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# Runs in a child process on the diagnostics library; one JSON line per frame configuration.
_CHILD = r'''
import json, os, sys, tempfile
sys.path[:0] = [os.path.join(os.getcwd(), "tests"), os.path.join(os.getcwd(), "scripts")]
import numpy as np
import chess2rt_amd as c2, csg_void_device as vdev, sphere_cull_device as dev, sphere_cull_scenes as S
mode, cases = sys.argv[1], json.loads(sys.argv[2])
debug_cull = int(os.environ.get("C2RT_DEBUG_CULL", "0"))
ctx = c2.Context(0)
tmp = tempfile.mkdtemp()
for name, sdl, W, H, taps, sh, world in cases:
    path = S.LECTURE5
    if sdl is not None:
        path = os.path.join(tmp, name + ".sdl")
        open(path, "w").write(sdl)
    scene = c2.parseSceneFromFile(path)
    scene.setFrameSize(W, H)
    cam = scene.beginFrame()
    ctx.uploadScene(scene.desc)
    for rank in range(world):
        opts = scene.renderOpts(taps=taps, strip_height=sh, strip_rank=rank, strip_world=world)
        if mode == "tables":
            r = dev.compare(ctx, scene.desc, cam, opts, debug_cull)
            dev.set_sphere_mask(ctx, 0)
            vdev.compare(ctx, scene.desc, cam, opts, debug_cull)  # switch off: the void test's pre-pass, unchanged
            dev.set_sphere_mask(ctx, 3)
            print(json.dumps(dict(name=name, rank=rank, world=world, drops=r and {str(k): v for k, v in r["drops"].items()},
                                  classes_off=r and r["classes_off"], classes_on=r and r["classes_on"])), flush=True)
        else:
            frames = []
            for mask in (3, 0):
                dev.set_sphere_mask(ctx, mask)
                frames.append(ctx.renderFrame(cam, opts))
            dev.set_sphere_mask(ctx, 3)
            equal = bool(np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32)))
            print(json.dumps(dict(name=name, taps=taps, equal=equal, nonzero=bool(np.any(frames[0])))), flush=True)
print("ok")
'''


def _run_child(mode, cases, env_extra=None, timeout=900):
    env = dict(os.environ, C2RT_LIB_VARIANT="diag", **(env_extra or {}))
    p = subprocess.run([sys.executable, "-c", _CHILD, mode, json.dumps(cases)], capture_output=True, text=True, timeout=timeout,
                       env=env, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout[-4000:] + p.stderr[-4000:]
    rows = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    for r in rows:
        print(r)
    return rows


def _cases():
    sys.path[:0] = [os.path.join(ROOT, "tests")]
    import sphere_cull_scenes as S

    c = [("lecture5_640", None, 640, 480, 5, 0, 1), ("lecture5_1080p", None, 1920, 1080, 5, 0, 1),
         ("lecture5_4k", None, 3840, 2160, 5, 0, 1), ("lecture5_333x217", None, 333, 217, 1, 0, 1)]
    c += [("lecture5_strips_%d_%d" % (world, sh), None, 640, 480, 5, sh, world) for world, sh in ((2, 8), (3, 4))]
    c += [("fuzz%d" % s, S.fuzz_scene(s), 320, 240, 5, 0, 1) for s in range(8)]
    c += [(name, sdl, 160, 120, 5, 0, 1) for name, sdl in S.adversarial()]
    return c


def test_device_drops_equal_host_claims():
    rows = _run_child("tables", _cases())
    by = {}
    for r in rows:
        by.setdefault(r["name"], []).append(r)
    assert set(by) == {c[0] for c in _cases()}

    def total(name, k):
        return sum(v[k] for r in by[name] for v in (r["drops"] or {}).values())

    # not vacuous: primary and shadow drops on lecture5 at every size and under strips, and on the fuzzed scenes
    for name in ("lecture5_640", "lecture5_1080p", "lecture5_4k", "lecture5_strips_2_8", "lecture5_strips_3_4"):
        assert total(name, 0) >= 20 and total(name, 1) >= 1, name
    assert sum(total("fuzz%d" % s, 0) for s in range(8)) >= 20
    # the headline frame: more ground-only tiles, fewer tiles with objects in view
    off, on = by["lecture5_4k"][0]["classes_off"], by["lecture5_4k"][0]["classes_on"]
    print("lecture5 4K tile classes (ground-only, ground-primary, objects, none): off %s, on %s" % (off, on))
    assert on[0] > off[0] and on[2] < off[2]


def test_switch_off_by_environment():
    """C2RT_DEBUG_CULL=8 (diagnostics build): no sphere test, whatever the hook asks for — the device drops nothing"""
    rows = _run_child("tables", [("lecture5_640", None, 640, 480, 5, 0, 1)], env_extra=dict(C2RT_DEBUG_CULL="8"))
    assert rows[0]["drops"] == {} and rows[0]["classes_off"] == rows[0]["classes_on"]


def test_lecture5_frames_bit_equal_with_the_switch_on_and_off():
    rows = _run_child("frames", [("lecture5_640", None, 640, 480, 1, 0, 1), ("lecture5_640", None, 640, 480, 5, 0, 1),
                                 ("lecture5_4k", None, 3840, 2160, 5, 0, 1)])
    assert len(rows) == 3 and all(r["equal"] and r["nonzero"] for r in rows), rows
