#!/usr/bin/env python3
"""Frames per second of SMALL frames, three ways, in one process:

  (a) 16 c2rt_render_frame_device calls on one stream           (the yardstick: code the library had before batches)
  (b) the same 16 calls alternating over two streams            (what a caller could do to overlap frames)
  (c) one c2rt_render_frames_device call for the 16 cameras     (one mask pre-pass launch + one frame launch)

for lecture5.sdl and lecture4.sdl at 1920x1080 and 640x360, one tap, 16 cameras on an orbit.  The legs are
interleaved a/b/c `--rounds` times; every timed window holds at least `--window-ms` of frames behind a settling phase
and ends in a device sync.  The frames of the three legs are compared bit for bit before any time is printed.

  python scripts/frame_batch_rate.py [--rounds 5] [--json out.json]
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/frame_batch_rate.py --only lecture5.sdl:1920x1080 --rounds 1
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

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
POINTS = [("lecture5.sdl", 1920, 1080), ("lecture5.sdl", 640, 360), ("lecture4.sdl", 1920, 1080), ("lecture4.sdl", 640, 360)]
N_CAMS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--only", help="scene:WxH, e.g. lecture5.sdl:1920x1080")
    ap.add_argument("--json")
    args = ap.parse_args()
    assert args.rounds >= 1
    points = POINTS
    if args.only:
        f, size = args.only.split(":")
        w, h = size.split("x")
        points = [(f, int(w), int(h))]

    ctx = c2.Context(0)
    lib = _abi.load_library()
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    results = []
    for scene_file, w, h in points:
        scene = c2.parseSceneFromFile(os.path.join(SCENES, scene_file))
        scene.setFrameSize(w, h)
        scene.setAA(False)
        scene.setDof(False)
        cams = []
        for _ in range(N_CAMS):
            cams.append(scene.beginFrame())
            scene.rotateCamera(360.0 / N_CAMS, 0, 0)
        opts = scene.renderOpts(taps=1)
        ctx.uploadScene(scene.desc)
        cam_arr = (_abi.CameraFrame * N_CAMS)(*cams)
        bufs = {k: torch.full((N_CAMS, h, w, 3), -1.0, dtype=torch.float32, device="cuda:0") for k in "abc"}
        frame_bytes = h * w * 3 * 4
        ptr = {k: bufs[k].data_ptr() for k in "abc"}
        h0, h1, o = ctx.handle, C.byref(opts), None

        def leg_a():
            for i in range(N_CAMS):
                lib.c2rt_render_frame_device(h0, C.byref(cam_arr[i]), h1, C.c_void_p(ptr["a"] + i * frame_bytes), C.c_void_p(s0.cuda_stream))

        def leg_b():
            for i in range(N_CAMS):
                lib.c2rt_render_frame_device(h0, C.byref(cam_arr[i]), h1, C.c_void_p(ptr["b"] + i * frame_bytes),
                                             C.c_void_p((s0 if i % 2 == 0 else s1).cuda_stream))

        def leg_c():
            st = lib.c2rt_render_frames_device(h0, cam_arr, N_CAMS, h1, C.c_void_p(ptr["c"]), C.c_void_p(s0.cuda_stream))
            assert st == _abi.OK, lib.c2rt_last_error(h0)

        legs = {"a": leg_a, "b": leg_b, "c": leg_c}
        for k in "abc":
            legs[k]()
        torch.cuda.synchronize()
        ref = bufs["a"].cpu().numpy().view(np.uint32)
        assert (ref != np.float32(-1.0).view(np.uint32)).any()
        for k in "bc":
            assert np.array_equal(ref, bufs[k].cpu().numpy().view(np.uint32)), "leg %s differs from leg a (%s %dx%d)" % (k, scene_file, w, h)

        # passes of 16 frames per timed window: from one timed pass of leg (a), the slowest per launch
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(4):
            leg_a()
        torch.cuda.synchronize()
        per_pass = (time.perf_counter() - t) / 4
        passes = max(4, int(math.ceil(args.window_ms * 1e-3 / per_pass * 1.25)))

        times = {k: [] for k in "abc"}
        for _ in range(args.rounds):
            for k in "abc":
                for _ in range(max(2, passes // 4)):   # settling phase
                    legs[k]()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(passes):
                    legs[k]()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                times[k].append(dt / (passes * N_CAMS) * 1e6)
        row = {"scene": scene_file, "width": w, "height": h, "taps": 1, "cameras": N_CAMS, "passes_per_window": passes,
               "window_ms": {k: round(statistics.median(times[k]) * passes * N_CAMS * 1e-3, 2) for k in "abc"}}
        for k in "abc":
            row[k] = {"us_per_frame_median": round(statistics.median(times[k]), 3), "min": round(min(times[k]), 3),
                      "max": round(max(times[k]), 3), "all": [round(x, 3) for x in times[k]]}
        results.append(row)
        print("%-13s %4dx%-4d  a %8.2f [%.2f..%.2f]  b %8.2f [%.2f..%.2f]  c %8.2f [%.2f..%.2f] us/frame  (c/a %.3f, c/b %.3f; %d passes/window)" % (
            scene_file, w, h, row["a"]["us_per_frame_median"], row["a"]["min"], row["a"]["max"],
            row["b"]["us_per_frame_median"], row["b"]["min"], row["b"]["max"],
            row["c"]["us_per_frame_median"], row["c"]["min"], row["c"]["max"],
            row["c"]["us_per_frame_median"] / row["a"]["us_per_frame_median"], row["c"]["us_per_frame_median"] / row["b"]["us_per_frame_median"], passes), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
