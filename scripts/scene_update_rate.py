#!/usr/bin/env python3
"""What it costs to move one sphere of lecture5 between frames, three ways, in one process:

  (a) c2rt_upload_scene of the patched description + c2rt_render_frame_device   (the route the library had: the baseline)
  (b) c2rt_update_scene + c2rt_render_frame_device on one stream                (no sync, no re-upload)
  (c) one c2rt_render_frames_posed_device call per 16 frames                    (a pose per frame, one launch pair)

and, from the same run, so that the cost of posing itself is visible:

  (f) c2rt_render_frame_device alone, the scene standing still
  (g) one c2rt_render_frames_device call per 16 frames, the scene standing still

at 1920x1080 and 640x360, one tap, 64 positions of ball S1 on a circle.  The legs are interleaved `--rounds` times;
every timed window holds at least `--window-ms` of frames behind a settling phase and ends in a device sync.  The
frames of (a), (b) and (c) are compared bit for bit before any time is printed.

  python scripts/scene_update_rate.py [--rounds 5] [--json out.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import chess2rt_amd as c2
from chess2rt_amd import _abi

SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl")
POINTS = [(1920, 1080), (640, 360)]
N_POS, BATCH = 64, 16
LEGS = "abcfg"


def translated(x, y, z):
    lib = _abi.load_library()
    t = np.empty(30, dtype=np.float64)
    lib.c2rt_host_transform_reset(t.ctypes.data_as(_abi._f64p))
    lib.c2rt_host_transform_translate(t.ctypes.data_as(_abi._f64p), (C.c_double * 3)(x, y, z))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--json")
    args = ap.parse_args()
    assert args.rounds >= 1
    ctx = c2.Context(0)
    lib = _abi.load_library()
    s0 = torch.cuda.Stream()
    stream = C.c_void_p(s0.cuda_stream)
    results = []
    for w, h in POINTS:
        scene = c2.parseSceneFromFile(SCENE)
        scene.setFrameSize(w, h)
        scene.setAA(False)
        cam, opts = scene.beginFrame(), scene.renderOpts(taps=1)
        ball = scene.nodeIndex("S1")
        p0 = scene.nodeTransform("S1")[27:30]
        xfs = [translated(p0[0] + 40 * math.cos(2 * math.pi * k / N_POS), p0[1], p0[2] + 40 * math.sin(2 * math.pi * k / N_POS)) for k in range(N_POS)]
        poses = [c2.makePose({ball: t}) for t in xfs]
        pose_arr = (_abi.ScenePose * N_POS)(*poses)
        cam_arr = (_abi.CameraFrame * BATCH)(*([cam] * BATCH))
        # (a): the patched descriptions, made once — the upload is what is timed, not the patching
        descs = []
        for t in xfs:
            scene.setNodeTransform("S1", t)
            d = _abi.SceneDesc.from_buffer_copy(scene.desc.contents)
            xf_all = np.ctypeslib.as_array(d.node_transform, shape=(30 * d.n_nodes,)).copy()
            d.node_transform = xf_all.ctypes.data_as(_abi._f64p)
            descs.append((d, xf_all))
        scene.setNodeTransform("S1", translated(*p0))
        bufs = {k: torch.full((N_POS, h, w, 3), -1.0, dtype=torch.float32, device="cuda:0") for k in "abc"}
        frame_bytes = h * w * 3 * 4
        ptr = {k: bufs[k].data_ptr() for k in "abc"}
        h0, o = ctx.handle, C.byref(opts)

        def leg_a():
            for i in range(N_POS):
                assert lib.c2rt_upload_scene(h0, C.byref(descs[i][0])) == _abi.OK
                lib.c2rt_render_frame_device(h0, C.byref(cam), o, C.c_void_p(ptr["a"] + i * frame_bytes), stream)

        def leg_b():
            for i in range(N_POS):
                lib.c2rt_update_scene(h0, C.byref(pose_arr[i]), stream)
                lib.c2rt_render_frame_device(h0, C.byref(cam), o, C.c_void_p(ptr["b"] + i * frame_bytes), stream)

        def leg_c():
            for i in range(0, N_POS, BATCH):
                st = lib.c2rt_render_frames_posed_device(h0, cam_arr, C.byref(pose_arr[i]), BATCH, o, C.c_void_p(ptr["c"] + i * frame_bytes), stream)
                assert st == _abi.OK, lib.c2rt_last_error(h0)

        def leg_f():
            for i in range(N_POS):
                lib.c2rt_render_frame_device(h0, C.byref(cam), o, C.c_void_p(ptr["b"] + i * frame_bytes), stream)

        def leg_g():
            for i in range(0, N_POS, BATCH):
                lib.c2rt_render_frames_device(h0, cam_arr, BATCH, o, C.c_void_p(ptr["c"] + i * frame_bytes), stream)

        legs = {"a": leg_a, "b": leg_b, "c": leg_c, "f": leg_f, "g": leg_g}
        ctx.uploadScene(scene.desc)
        for k in "abc":
            legs[k]()
            torch.cuda.synchronize()
            ctx.uploadScene(scene.desc)
        ref = bufs["a"].cpu().numpy().view(np.uint32)
        assert (ref != np.float32(-1.0).view(np.uint32)).any() and not np.array_equal(ref[0], ref[N_POS // 2])
        for k in "bc":
            assert np.array_equal(ref, bufs[k].cpu().numpy().view(np.uint32)), "leg %s differs from leg a (%dx%d)" % (k, w, h)

        times = {k: [] for k in LEGS}
        passes = {}
        for k in LEGS:   # passes of 64 frames per timed window, from one timed pass of the leg itself
            torch.cuda.synchronize()
            t = time.perf_counter()
            legs[k]()
            torch.cuda.synchronize()
            passes[k] = max(1, int(math.ceil(args.window_ms * 1e-3 / (time.perf_counter() - t) * 1.25)))
        for _ in range(args.rounds):
            for k in LEGS:
                ctx.uploadScene(scene.desc)
                for _ in range(max(1, passes[k] // 4)):   # settling phase
                    legs[k]()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(passes[k]):
                    legs[k]()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t) / (passes[k] * N_POS) * 1e6)
        row = {"scene": "lecture5.sdl", "width": w, "height": h, "taps": 1, "positions": N_POS, "batch": BATCH, "passes_per_window": passes}
        for k in LEGS:
            row[k] = {"us_per_frame_median": round(statistics.median(times[k]), 3), "min": round(min(times[k]), 3),
                      "max": round(max(times[k]), 3), "all": [round(x, 3) for x in times[k]]}
        results.append(row)
        print("lecture5 %4dx%-4d us/frame:  " % (w, h) + "  ".join("%s %9.2f [%.2f..%.2f]" % (k, row[k]["us_per_frame_median"], row[k]["min"], row[k]["max"]) for k in LEGS), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
