#!/usr/bin/env python3
"""Time of the counted path planes (c2rt_render_paths_counted_device, `indirect` alone) on lecture5.sdl, 4 bounces, a cap of
64 paths, everything resident in HBM, in BOTH launch orders, over three count planes:

  (a)  the counts c2rt_path_counts makes for frame 3 of the moving sequence scripts/denoise_variance_rate.py uses (the
       shipped camera, then three times moveCamera(10, 2, 5) and rotateCamera(8, 0, 3); frames 0 .. 2 traced at 16 paths
       and accumulated by c2rt_temporal_accumulate): min 2 / max 64 / young 16, min_age 2, and a paths_per_variance
       bisected so that the mean count of the hit pixels is near --mean (printed: the value used)
  (b)  synthetic, scattered: 5 % of the pixels at 64, chosen by a fixed hash, the rest at 4
  (c)  synthetic, clustered: the same share as whole 32x32 blocks, chosen by the same hash

For each plane, per call: the counted call in natural order and in count order (the sort's memset and three kernels
included), and — the YARDSTICK, out of --yardstick NAME, libc2rt_NAME.so built from the PARENT commit's source (make
VARIANT=NAME in a checkout of it), never the new code against itself — c2rt_render_paths_device at P = 64 and at
P = ceil(mean count): the bound no per-pixel scheme beats by much.  Then the counted call with every count 16 against the
yardstick's P = 16 (what reading the plane costs), c2rt_path_counts_device against the yardstick's
c2rt_temporal_accumulate_device on the same frame, and one quality figure: the RMSE of `indirect` on plane (a)'s frame
against a 64-path reference of another seed, for the counted call and for the uniform call at the same total number of
paths.  The two orders and the all-16 plane are compared bit for bit on the way.

Every window holds --calls calls behind a warm-up call and lies between two device events; the legs are interleaved
--rounds times in one process; median [min..max] per call.  The spread of the uniform call is its [min..max].

  python scripts/paths_counted_rate.py --yardstick parent [--width 1920 --height 1080] [--json out.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import chess2rt_amd as c2
from chess2rt_amd import _abi

MOVE, ROTATE, FRAMES = (10.0, 2.0, 5.0), (8.0, 0.0, 3.0), 4
CAP, BOUNCES, SEED = 64, 4, 7
RULE = dict(min_paths=2, max_paths=64, young_paths=16, min_age=2, prev_paths=16)
NAMES = ("c2rt_init", "c2rt_destroy", "c2rt_last_error", "c2rt_upload_scene", "c2rt_render_paths_device", "c2rt_temporal_accumulate_device")


def med(v):
    return "%9.1f us [%.1f..%.1f]" % (statistics.median(v), min(v), max(v))


def mix(i):
    x = np.asarray(i, dtype=np.uint64) * np.uint64(0x9E3779B1) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = x * np.uint64(0x85EBCA77) & np.uint64(0xFFFFFFFF)
    return x ^ (x >> np.uint64(13))


class Yardstick:
    """a build of the library from another commit and a context of its own on device 0, with the scene uploaded"""

    def __init__(self, variant, desc):
        self.name = variant
        self.lib = C.CDLL(os.path.join(ROOT, "chess2rt_amd", "libc2rt_%s.so" % variant), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)   # DEEPBIND: its own launchers
        for name in NAMES:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _abi.C2RT_SYMBOLS[name]
        self.h = C.c_void_p()
        assert self.lib.c2rt_init(0, C.byref(self.h)) == 0
        self.check(self.lib.c2rt_upload_scene(self.h, desc))

    def check(self, st):
        assert st == 0, self.lib.c2rt_last_error(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--mean", type=float, default=8.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--yardstick", required=True)
    ap.add_argument("--json")
    a = ap.parse_args()
    W, H, px = a.width, a.height, a.width * a.height
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    scene = c2.parseSceneFromFile(os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl"))
    scene.setFrameSize(W, H)
    scene.setAA(False)
    scene.setDof(False)
    opts = scene.renderOpts(taps=_abi.TAPS_1)
    ctx = c2.Context(0)
    ctx.uploadScene(scene.desc)
    yard = Yardstick(a.yardstick, scene.desc)

    # ---- the three count planes ----
    prev, hist = None, None
    for i in range(FRAMES):                                      # the sequence, through the host calls: once, untimed
        cam = scene.beginFrame()
        hits = ctx.renderHits(cam, opts, planes=("node", "normal", "p"))
        if i + 1 < FRAMES:
            indirect = ctx.renderPaths(cam, opts, 16, BOUNCES, seed=SEED + i, planes=("indirect",))["indirect"]
            _, hist = ctx.temporalAccumulate(hits, indirect, prev_cam=prev, history=hist, planes=())
            prev = cam
            scene.moveCamera(*MOVE)
            scene.rotateCamera(*ROTATE)
    hit = hits["node"] >= 0
    n_hit = int(hit.sum())

    def counts_at(ppv):
        return ctx.pathCounts(hits, prev_cam=prev, history=hist, paths_per_variance=ppv, planes=(), **RULE)["counts"]

    lo, hi = 1.0, 1e7                                            # the mean count grows with paths_per_variance
    for _ in range(24):
        ppv = math.sqrt(lo * hi)
        if counts_at(ppv)[hit].mean() < a.mean:
            lo = ppv
        else:
            hi = ppv
    ppv = float(np.float32(math.sqrt(lo * hi)))
    plane_a = counts_at(ppv)
    ys, xs = np.mgrid[0:H, 0:W]
    heavy = mix(ys * W + xs) % np.uint64(1000) < np.uint64(50)
    plane_b = np.where(heavy, 64, 4).astype(np.uint8)
    heavy = mix((ys // 32) * ((W + 31) // 32) + xs // 32 + 12345) % np.uint64(1000) < np.uint64(50)
    plane_c = np.where(heavy, 64, 4).astype(np.uint8)
    planes = {"a": plane_a, "b": plane_b, "c": plane_c, "16": np.full((H, W), 16, dtype=np.uint8)}
    print("lecture5 %dx%d, %d bounces, cap %d; frame %d of the sequence: %d of %d pixels hit" % (W, H, BOUNCES, CAP, FRAMES - 1, n_hit, px))
    print("(a) paths_per_variance %.9g (min %d / max %d / young %d, min_age %d): counts of the hit pixels: mean %.3f, %s"
          % (ppv, RULE["min_paths"], RULE["max_paths"], RULE["young_paths"], RULE["min_age"], plane_a[hit].mean(),
             ", ".join("%d: %.1f %%" % (k, 100.0 * (plane_a[hit] == k).sum() / n_hit) for k in (2, 16, 64))))
    means = {}
    for k, p in planes.items():
        means[k] = float(np.minimum(p, CAP)[hit].mean())
        print("plane (%s): mean count of the hit pixels %.3f, of all pixels %.3f" % (k, means[k], float(p.mean())))

    # ---- device state ----
    t_counts = {k: torch.from_numpy(np.ascontiguousarray(p)).to(dev) for k, p in planes.items()}
    out = {k: torch.empty((H, W, 3), dtype=torch.float32, device=dev) for k in ("natural", "count", "yard")}
    scratch = torch.empty(c2.paths_counted_scratch_bytes(px), dtype=torch.uint8, device=dev)
    g = _abi.PathOpts(seed=SEED + FRAMES - 1, paths=CAP, bounces=BOUNCES)

    def counted(k, order):
        ctx.renderPathsCountedDevice(cam, opts, t_counts[k].data_ptr(), CAP, BOUNCES, {"indirect": out[order].data_ptr()}, seed=g.seed,
                                     scratch_ptr=scratch.data_ptr() if order == "count" else 0, stream=stream)

    def uniform(paths):
        gp = _abi.PathOpts(seed=g.seed, paths=paths, bounces=BOUNCES)
        pl = _abi.PathPlanes(indirect=out["yard"].data_ptr())
        yard.check(yard.lib.c2rt_render_paths_device(yard.h, C.byref(cam), C.byref(opts), C.byref(gp), C.byref(pl), stream))

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / calls

    # warm-up of every shape, and the bits: the two orders against each other, the all-16 plane against the yardstick's P = 16
    for k in planes:
        counted(k, "natural")
        counted(k, "count")
        torch.cuda.synchronize()
        d = int((out["natural"].view(torch.int32) != out["count"].view(torch.int32)).sum())
        print("plane (%s): natural order against count order: %d of %d values differ" % (k, d, px * 3))
    uniform(16)
    torch.cuda.synchronize()
    print("plane (16) against %s at P = 16: %d of %d values differ" % (yard.name, int((out["count"].view(torch.int32) != out["yard"].view(torch.int32)).sum()), px * 3))

    legs = {}
    for k in ("a", "b", "c"):
        legs["(%s) counted, natural order" % k] = lambda k=k: counted(k, "natural")
        legs["(%s) counted, count order" % k] = lambda k=k: counted(k, "count")
        legs["(%s) %s uniform P = %d = ceil(mean)" % (k, yard.name, math.ceil(means[k]))] = lambda k=k: uniform(math.ceil(means[k]))
    legs["%s uniform P = 64" % yard.name] = lambda: uniform(64)
    legs["(16) counted, natural order"] = lambda: counted("16", "natural")
    legs["(16) counted, count order"] = lambda: counted("16", "count")
    legs["%s uniform P = 16" % yard.name] = lambda: uniform(16)

    # c2rt_path_counts_device against the yardstick's accumulation, the same frame and history
    th = {k: torch.from_numpy(np.ascontiguousarray(hits[k])).to(dev) for k in ("node", "normal", "p")}
    t_hist, t_hist_out = torch.from_numpy(hist).to(dev), torch.empty(len(hist), dtype=torch.uint8, device=dev)
    t_in = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    t_cnt = torch.empty((H, W), dtype=torch.uint8, device=dev)
    t_var, t_age = torch.empty((H, W), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.int32, device=dev)
    ptrs = {k: v.data_ptr() for k, v in th.items()}
    tg = _abi.TemporalGuides(node=ptrs["node"], normal=ptrs["normal"], p=ptrs["p"])
    to = _abi.TemporalOpts(width=W, height=H, channels=3, max_age=32, min_normal_dot=0.9, max_plane_dist=0.1)
    tp = _abi.TemporalPlanes(variance=t_var.data_ptr(), age=t_age.data_ptr())
    legs["c2rt_path_counts_device, counts alone"] = lambda: ctx.pathCountsDevice(ptrs, W, H, t_hist.data_ptr(), t_counts["16"].data_ptr(), t_cnt.data_ptr(),
                                                                                prev_cam=prev, paths_per_variance=ppv, stream=stream, **RULE)
    legs["c2rt_path_counts_device, counts + variance + age"] = lambda: ctx.pathCountsDevice(ptrs, W, H, t_hist.data_ptr(), t_counts["16"].data_ptr(), t_cnt.data_ptr(),
                                                                                           t_var.data_ptr(), t_age.data_ptr(), prev_cam=prev,
                                                                                           paths_per_variance=ppv, stream=stream, **RULE)
    legs["%s c2rt_temporal_accumulate_device, history + variance + age" % yard.name] = lambda: yard.check(yard.lib.c2rt_temporal_accumulate_device(
        yard.h, C.byref(prev), C.byref(tg), C.byref(to), t_in.data_ptr(), t_hist.data_ptr(), t_hist_out.data_ptr(), C.byref(tp), stream))
    small = {k for k in legs if "path_counts" in k or "temporal" in k}

    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    T = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            T[k].append(window(fn, a.calls * 20 if k in small else a.calls))
    for k in legs:
        print("%-66s %s" % (k, med(T[k])))
    m = {k: statistics.median(v) for k, v in T.items()}
    for k in ("a", "b", "c"):
        nat, cnt = m["(%s) counted, natural order" % k], m["(%s) counted, count order" % k]
        bound = m["(%s) %s uniform P = %d = ceil(mean)" % (k, yard.name, math.ceil(means[k]))]
        print("plane (%s): count order / natural order %.3f; natural / uniform 64: %.3f; count / uniform 64: %.3f; natural / bound: %.2f; count / bound: %.2f"
              % (k, cnt / nat, nat / m["%s uniform P = 64" % yard.name], cnt / m["%s uniform P = 64" % yard.name], nat / bound, cnt / bound))
    u16 = T["%s uniform P = 16" % yard.name]
    print("all counts 16, natural order, over the uniform call at 16: %.4f (the uniform call's own spread: %.4f .. %.4f of its median)"
          % (m["(16) counted, natural order"] / statistics.median(u16), min(u16) / statistics.median(u16), max(u16) / statistics.median(u16)))

    # ---- quality on plane (a)'s frame ----
    ref = ctx.renderPaths(cam, opts, 64, BOUNCES, seed=1000, planes=("indirect",))["indirect"]
    total = int(np.minimum(plane_a, CAP)[hit].astype(np.int64).sum())
    p_same = max(1, int(round(total / n_hit)))
    adaptive = ctx.renderPathsCounted(cam, opts, plane_a, CAP, BOUNCES, seed=g.seed, planes=("indirect",))["indirect"]
    flat = ctx.renderPaths(cam, opts, p_same, BOUNCES, seed=g.seed, planes=("indirect",))["indirect"]

    def rmse(x):
        return float(np.sqrt(((x[hit].astype(np.float64) - ref[hit]) ** 2).mean()))

    print("quality, `indirect` against a 64-path reference of another seed, RMSE over the %d hit pixels:" % n_hit)
    print("  counted, plane (a): %d paths in all                  %.6f" % (total, rmse(adaptive)))
    print("  uniform at P = %d: %d paths in all                   %.6f" % (p_same, p_same * n_hit, rmse(flat)))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"size": [W, H], "paths_per_variance": ppv, "means": means, "us": T, "rmse": {"counted": rmse(adaptive), "uniform": rmse(flat)},
                       "total_paths": {"counted": total, "uniform": p_same * n_hit}}, f, indent=1)


if __name__ == "__main__":
    main()
