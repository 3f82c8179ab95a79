#!/usr/bin/env python3
"""Rays per second of the ray and visibility queries (c2rt_trace_rays_device, c2rt_test_visibility_device) on
lecture5.sdl, everything resident in HBM:

  coherent   the 1920x1080 screen rays of the scene's camera, in pixel order — hits + colour, hits only, colour only
  shuffled   the same rays in random order (divergent closest-node passes and texel fetches)
  visibility segments from each coherent ray's hit point (or a point along a miss) to the light, in order and shuffled
  frame      the context's own 1-tap 1080p frame of that camera, for context (culled, lean arithmetic, 12 B per ray)

Every timed window holds at least --window-ms of work behind a settling phase and ends in a device sync; the legs are
interleaved --rounds times and the median, minimum and maximum are printed.

  python scripts/ray_query_rate.py [--rounds 5] [--json out.json]
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

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
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
    # Camera.getScreenRay (rt/camera.d:123-154), vectorised: the exact bits do not matter to a rate
    ul, ur, dl, pos = (np.array(list(v)) for v in (cam.up_left, cam.up_right, cam.down_left, cam.pos))
    xs, ys = np.meshgrid(np.arange(w) / cam.frame_width, np.arange(h) / cam.frame_height)
    d = ul + (ur - ul) * xs[..., None] + (dl - ul) * ys[..., None] - pos
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(n, 3)
    rays = np.ascontiguousarray(np.hstack([np.broadcast_to(pos, d.shape), d]))
    perm = np.random.RandomState(1).permutation(n)
    dev = torch.device("cuda:0")
    rays_t = {"coherent": torch.from_numpy(rays).to(dev), "shuffled": torch.from_numpy(np.ascontiguousarray(rays[perm])).to(dev)}
    hits_t = torch.empty(n * 80, dtype=torch.uint8, device=dev)
    rgb_t = torch.empty((n, 3), dtype=torch.float32, device=dev)
    vis_t = torch.empty(n, dtype=torch.uint8, device=dev)
    frame_t = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    rec, _ = ctx.traceRays(rays, colors=False)
    light = np.array([scene.desc.contents.light_pos[k] for k in range(3)])
    frm = np.where((rec["closest_node"] >= 0)[:, None], rec["p"] + rec["normal"] * 1e-6, rays[:, :3] + rays[:, 3:] * 100.0)
    segs = np.ascontiguousarray(np.hstack([frm, np.broadcast_to(light, frm.shape)]))
    segs_t = {"coherent": torch.from_numpy(segs).to(dev), "shuffled": torch.from_numpy(np.ascontiguousarray(segs[perm])).to(dev)}
    st = torch.cuda.Stream(dev)
    s = st.cuda_stream
    legs = {}
    for order in ("coherent", "shuffled"):
        rp, sp = rays_t[order].data_ptr(), segs_t[order].data_ptr()
        legs["rays %s hits+colour" % order] = lambda rp=rp: ctx.traceRaysDevice(rp, n, hits_t.data_ptr(), rgb_t.data_ptr(), s)
        legs["rays %s hits only" % order] = lambda rp=rp: ctx.traceRaysDevice(rp, n, hits_t.data_ptr(), 0, s)
        legs["rays %s colour only" % order] = lambda rp=rp: ctx.traceRaysDevice(rp, n, 0, rgb_t.data_ptr(), s)
        legs["visibility %s" % order] = lambda sp=sp: ctx.testVisibilityDevice(sp, n, vis_t.data_ptr(), s)
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
    rows = []
    for k in legs:
        med = statistics.median(times[k])
        rows.append({"leg": k, "rays": n, "us_median": round(med * 1e6, 2), "us_min": round(min(times[k]) * 1e6, 2), "us_max": round(max(times[k]) * 1e6, 2),
                     "grays_per_s": round(n / med * 1e-9, 3), "passes_per_window": passes[k]})
        print("%-32s %9.1f us [%.1f..%.1f]  %7.3f G/s  (%d passes/window)" % (k, med * 1e6, min(times[k]) * 1e6, max(times[k]) * 1e6, n / med * 1e-9, passes[k]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
