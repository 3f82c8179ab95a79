#!/usr/bin/env python3
"""Pixels per second of the hit planes (c2rt_render_hits_device) on lecture5.sdl at 1920x1080, everything resident
in HBM, next to the route the ray queries offer for the same pixels:

  planes   all seven, node + dist only, everything but rgb
  rays     c2rt_trace_rays_device over the same camera's screen rays, already in HBM: hits only, hits + colour
  frame    the context's own 1-tap frame of that camera, for context (culled, lean arithmetic, 12 B per pixel)

Every timed window holds at least --window-ms of work behind a settling phase and ends in a device sync; the legs are
interleaved --rounds times and the median, minimum and maximum are printed.  The library variant under test is the
one C2RT_LIB_VARIANT names (A/B builds of the pixel-to-lane mapping and of the row stores: profiles/hit_planes.md).

  python scripts/hit_plane_rate.py [--rounds 5] [--json out.json]
"""
import argparse
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
from chess2rt_amd.api import HIT_PLANES

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--planes-only", action="store_true", help="skip the ray-query and frame legs (variant builds)")
    ap.add_argument("--json")
    args = ap.parse_args()
    w, h = args.size
    n = w * h
    scene = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    scene.setFrameSize(w, h)
    scene.setAA(False)
    scene.setDof(False)
    cam = scene.beginFrame()
    opts = scene.renderOpts(taps=1)
    ctx = c2.Context(0)
    ctx.uploadScene(scene.desc)
    dev = torch.device("cuda:0")
    planes_t = {k: torch.empty(n * comps, dtype=torch.from_numpy(np.empty(0, dtype=t)).dtype, device=dev) for k, (t, comps) in HIT_PLANES.items()}
    ptrs = {k: v.data_ptr() for k, v in planes_t.items()}
    st = torch.cuda.Stream(dev)
    s = st.cuda_stream
    legs = {}
    legs["planes all seven"] = lambda: ctx.renderHitsDevice(cam, opts, ptrs, s)
    legs["planes node + dist"] = lambda: ctx.renderHitsDevice(cam, opts, {"node": ptrs["node"], "dist": ptrs["dist"]}, s)
    no_rgb = {k: v for k, v in ptrs.items() if k != "rgb"}
    legs["planes all but rgb"] = lambda: ctx.renderHitsDevice(cam, opts, no_rgb, s)
    if not args.planes_only:
        # Camera.getScreenRay (rt/camera.d:123-154), vectorised: the exact bits do not matter to a rate
        ul, ur, dl, pos = (np.array(list(v)) for v in (cam.up_left, cam.up_right, cam.down_left, cam.pos))
        xs, ys = np.meshgrid(np.arange(w) / cam.frame_width, np.arange(h) / cam.frame_height)
        d = ul + (ur - ul) * xs[..., None] + (dl - ul) * ys[..., None] - pos
        d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(n, 3)
        rays_t = torch.from_numpy(np.ascontiguousarray(np.hstack([np.broadcast_to(pos, d.shape), d]))).to(dev)
        hits_t = torch.empty(n * 80, dtype=torch.uint8, device=dev)
        rgb_t = torch.empty((n, 3), dtype=torch.float32, device=dev)
        frame_t = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        legs["rays hits only"] = lambda: ctx.traceRaysDevice(rays_t.data_ptr(), n, hits_t.data_ptr(), 0, s)
        legs["rays hits + colour"] = lambda: ctx.traceRaysDevice(rays_t.data_ptr(), n, hits_t.data_ptr(), rgb_t.data_ptr(), s)
        legs["frame 1 tap (context)"] = lambda: ctx.renderFrameDevice(cam, opts, frame_t.data_ptr(), s)
    passes = {}
    for k, leg in legs.items():
        leg()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(3):
            leg()
        torch.cuda.synchronize()
        passes[k] = max(3, int(math.ceil(args.window_ms * 1e-3 / ((time.perf_counter() - t) / 3) * 1.25)))
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, leg in legs.items():
            for _ in range(max(2, passes[k] // 4)):   # settling phase
                leg()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(passes[k]):
                leg()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t) / passes[k])
    variant = os.environ.get("C2RT_LIB_VARIANT", "") or "default"
    rows = []
    for k in legs:
        med = statistics.median(times[k])
        rows.append({"variant": variant, "leg": k, "pixels": n, "us_median": round(med * 1e6, 2), "us_min": round(min(times[k]) * 1e6, 2),
                     "us_max": round(max(times[k]) * 1e6, 2), "gpixels_per_s": round(n / med * 1e-9, 3), "passes_per_window": passes[k]})
        print("%-10s %-24s %9.1f us [%.1f..%.1f]  %7.3f Gpx/s  (%d passes/window)" % (variant, k, med * 1e6, min(times[k]) * 1e6, max(times[k]) * 1e6, n / med * 1e-9, passes[k]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
