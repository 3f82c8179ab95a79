#!/usr/bin/env python3
"""Anti-aliased frames of an orbit, four ways, in one process: 16 cameras into device buffers,

  (a) 16 c2rt_render_frame_adaptive_device calls on one stream      (the yardstick: code the library had before)
  (b) the same 16 calls alternating over two streams                (what a caller could do to overlap frames)
  (c) one c2rt_render_frames_adaptive_device call                   (one-tap batch, ONE detection and ONE refinement launch)
  (d) one five-tap c2rt_render_frames_device call                   (the batch a caller had to take for anti-aliased frames)

for lecture5.sdl at 640x360 and 1920x1080 and lecture4.sdl at 1920x1080 (the adverse case: 18.8 % of the pixels flag).
The legs are interleaved a/b/c/d `--rounds` times; every timed window holds at least `--window-ms` of frames behind a
settling phase and ends in a device sync; median, minimum and maximum are printed, and with them how much of a window
had passed when its calls had returned (the host's share: a leg whose share is the whole window is bound by the host's
enqueueing, not by the device).  Before any time is taken the frames
and masks of (a), (b) and (c) are compared bit for bit, and (c)'s flagged pixels with (d)'s.

  python scripts/adaptive_batch_rate.py [--rounds 5] [--json out.json]
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/adaptive_batch_rate.py --only lecture5.sdl:640x360 --once
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
import torch

import chess2rt_amd as c2
from chess2rt_amd import _abi

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
POINTS = [("lecture5.sdl", 640, 360), ("lecture5.sdl", 1920, 1080), ("lecture4.sdl", 1920, 1080)]
N_CAMS = 16
LEGS = "abcd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--only", help="scene:WxH, e.g. lecture5.sdl:640x360")
    ap.add_argument("--once", action="store_true", help="each leg once after the comparison and nothing else (under rocprofv3)")
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
    thr = C.c_float(_abi.AA_THRESHOLD_REF)
    results = []
    for scene_file, w, h in points:
        scene = c2.parseSceneFromFile(os.path.join(SCENES, scene_file))
        scene.setFrameSize(w, h)
        scene.setAA(True)
        scene.setDof(False)
        cams = []
        for _ in range(N_CAMS):
            cams.append(scene.beginFrame())
            scene.rotateCamera(360.0 / N_CAMS, 0, 0)
        opts = scene.renderOpts(taps=_abi.TAPS_REF5)
        ctx.uploadScene(scene.desc)
        cam_arr = (_abi.CameraFrame * N_CAMS)(*cams)
        frames = {k: torch.full((N_CAMS, h, w, 3), -1.0, dtype=torch.float32, device="cuda:0") for k in LEGS}
        masks = {k: torch.full((N_CAMS, h, w), 7, dtype=torch.uint8, device="cuda:0") for k in "abc"}
        frame_bytes, mask_bytes = h * w * 3 * 4, h * w
        fp = {k: frames[k].data_ptr() for k in LEGS}
        mp = {k: masks[k].data_ptr() for k in "abc"}
        h0, o = ctx.handle, C.byref(opts)

        def single(k, i, stream):
            st = lib.c2rt_render_frame_adaptive_device(h0, C.byref(cam_arr[i]), o, thr, C.c_void_p(fp[k] + i * frame_bytes),
                                                       C.c_void_p(mp[k] + i * mask_bytes), C.c_void_p(stream.cuda_stream))
            assert st == _abi.OK, lib.c2rt_last_error(h0)

        def leg_a():
            for i in range(N_CAMS):
                single("a", i, s0)

        def leg_b():
            for i in range(N_CAMS):
                single("b", i, s0 if i % 2 == 0 else s1)

        def leg_c():
            st = lib.c2rt_render_frames_adaptive_device(h0, cam_arr, N_CAMS, o, thr, C.c_void_p(fp["c"]), C.c_void_p(mp["c"]), C.c_void_p(s0.cuda_stream))
            assert st == _abi.OK, lib.c2rt_last_error(h0)

        def leg_d():
            st = lib.c2rt_render_frames_device(h0, cam_arr, N_CAMS, o, C.c_void_p(fp["d"]), C.c_void_p(s0.cuda_stream))
            assert st == _abi.OK, lib.c2rt_last_error(h0)

        legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d}
        for k in LEGS:
            legs[k]()
        torch.cuda.synchronize()
        name = "%s %dx%d" % (scene_file, w, h)
        as_bits = lambda t: t.view(torch.int32)
        assert bool(((masks["a"] == 0) | (masks["a"] == 1)).all()) and bool((frames["a"] != -1.0).any())
        for k in "bc":
            assert torch.equal(masks[k], masks["a"]), "leg %s: masks differ from leg a (%s)" % (k, name)
            assert torch.equal(as_bits(frames[k]), as_bits(frames["a"])), "leg %s: frames differ from leg a (%s)" % (k, name)
        flagged = masks["c"] == 1
        assert torch.equal(as_bits(frames["c"])[flagged], as_bits(frames["d"])[flagged]), "leg c: flagged pixels differ from the five-tap batch (%s)" % name
        share = [float(m.to(torch.float32).mean().item()) for m in masks["c"]]
        print("%-26s flagged share %.4f over the orbit (%.4f..%.4f per frame); legs a, b, c agree bit for bit, c's flagged pixels with d's" % (
            name, sum(share) / N_CAMS, min(share), max(share)), flush=True)
        if args.once:
            continue

        # passes of 16 frames per timed window, per leg: from three timed passes of it
        passes = {}
        for k in LEGS:
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(3):
                legs[k]()
            torch.cuda.synchronize()
            passes[k] = max(4, int(math.ceil(args.window_ms * 1e-3 / ((time.perf_counter() - t) / 3) * 1.25)))

        times, host = {k: [] for k in LEGS}, {k: [] for k in LEGS}
        for _ in range(args.rounds):
            for k in LEGS:
                for _ in range(max(2, passes[k] // 4)):   # settling phase
                    legs[k]()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(passes[k]):
                    legs[k]()
                enqueued = time.perf_counter() - t      # the calls have returned; the device may still be busy
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                times[k].append(dt / (passes[k] * N_CAMS) * 1e6)
                host[k].append(enqueued / (passes[k] * N_CAMS) * 1e6)
        row = {"scene": scene_file, "width": w, "height": h, "cameras": N_CAMS, "threshold": _abi.AA_THRESHOLD_REF,
               "flagged_share": round(sum(share) / N_CAMS, 5), "passes_per_window": passes,
               "window_ms": {k: round(min(times[k]) * passes[k] * N_CAMS * 1e-3, 2) for k in LEGS}}
        for k in LEGS:
            row[k] = {"us_per_frame_median": round(statistics.median(times[k]), 3), "min": round(min(times[k]), 3),
                      "max": round(max(times[k]), 3), "all": [round(x, 3) for x in times[k]],
                      "host_us_per_frame_median": round(statistics.median(host[k]), 3)}
        med = {k: row[k]["us_per_frame_median"] for k in LEGS}
        spread = {k: row[k]["max"] - row[k]["min"] for k in LEGS}
        row["a_minus_c"] = round(med["a"] - med["c"], 3)
        row["spread_a_plus_c"] = round(spread["a"] + spread["c"], 3)
        results.append(row)
        print("%-26s %s us/frame" % (name, "  ".join("%s %8.2f [%.2f..%.2f]" % (k, med[k], row[k]["min"], row[k]["max"]) for k in LEGS)), flush=True)
        print("%-26s of which on the host, until the calls have returned: %s us/frame" % (
            "", "  ".join("%s %.2f" % (k, row[k]["host_us_per_frame_median"]) for k in LEGS)), flush=True)
        print("%-26s c/a %.3f  c/b %.3f  c/d %.3f;  a - c = %.2f us against spreads (max - min) of a and c together %.2f us;  passes/window %s" % (
            "", med["c"] / med["a"], med["c"] / med["b"], med["c"] / med["d"], row["a_minus_c"], row["spread_a_plus_c"],
            " ".join("%s %d" % (k, passes[k]) for k in LEGS)), flush=True)
    if args.json and results:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
