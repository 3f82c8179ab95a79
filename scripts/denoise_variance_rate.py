#!/usr/bin/env python3
"""Time of the variance-guided a-trous filter (c2rt_denoise_variance_device) on lecture5.sdl, three channels, five levels,
everything resident in HBM.  The planes are those of frame 3 of the test sequence (the shipped camera, then three times
moveCamera(10, 2, 5) and rotateCamera(8, 0, 3)): the context's own hit planes, the path planes' `indirect` accumulated
over the four frames by c2rt_temporal_accumulate, its variance and its ages.

  (v L)   the whole call with L = 0 .. levels levels, steady-state ages (min_age 4: the disoccluded pixels are young);
          level l alone is (v l+1) - (v l), taken round by round; L = 0 is stage A and the closing steps
  (y)     the same with every age 0: every hit pixel takes the 7x7 spatial estimate (frame 0 of a sequence)
  (a)     stage A alone in both states: levels == 0 with variance_out, less the closing-steps launch (levels == 0 without)
  (d L)   the YARDSTICK: c2rt_denoise_device with sigma_colour = 0.5 out of --yardstick NAME, libc2rt_NAME.so built from
          the PARENT commit's source (make VARIANT=NAME in a checkout of it) — today's closest equivalent; never the new
          code against itself
  (c)     a device-to-device copy of 64 MB, for the rate a plain copy reaches in this run
  (p)     one c2rt_render_paths_device launch (`indirect` alone) at --paths / --bounces, for the share the filter adds

--variants a,b times libc2rt_a.so, libc2rt_b.so (make VARIANT=...) next to the library itself, interleaved in the same
rounds, and compares their outputs bit for bit: the A/B of a kernel form is a run of this script.  Every window holds
--calls calls behind a warm-up and lies between two device events; the legs are interleaved --rounds times in one process;
median [min..max] per call.

Algorithmic bytes of a level: the packed guides (32 B), the colour (12 B), the variance and its blur g (4 B each) read once,
colour and variance written once, and the blur launch's 4 B read and 4 B written: 76 B per pixel (the plain filter's: 56).

  python scripts/denoise_variance_rate.py [--width 1920 --height 1080] [--yardstick parent] [--variants a,b] [--json out.json]
"""
import argparse
import ctypes as C
import json
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
NAMES = ("c2rt_init", "c2rt_destroy", "c2rt_last_error", "c2rt_denoise_device", "c2rt_denoise_scratch_bytes", "c2rt_denoise_variance_device",
         "c2rt_denoise_variance_scratch_bytes")


def med(v):
    return "%9.1f us [%.1f..%.1f]" % (statistics.median(v), min(v), max(v))


class Lib:
    """a build of the library and a context of its own on device 0 (the product library: the package's)"""

    def __init__(self, variant):
        self.name = variant or "libc2rt"
        if variant:
            self.lib = C.CDLL(os.path.join(ROOT, "chess2rt_amd", "libc2rt_%s.so" % variant), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)   # DEEPBIND: its own launchers
            for name in NAMES:
                if hasattr(self.lib, name):                      # the yardstick has no variance-guided filter
                    fn = getattr(self.lib, name)
                    fn.restype, fn.argtypes = _abi.C2RT_SYMBOLS[name]
        else:
            self.lib = _abi.load_library()
        self.h = C.c_void_p()
        assert self.lib.c2rt_init(0, C.byref(self.h)) == 0

    def check(self, st):
        assert st == 0, self.lib.c2rt_last_error(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--paths", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--yardstick", default="")
    ap.add_argument("--variants", default="")
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
    prev, hist = None, None
    for i in range(FRAMES):                                      # the sequence, through the host calls: once, untimed
        cam = scene.beginFrame()
        hits = ctx.renderHits(cam, opts, planes=("node", "normal", "p", "rgb"))
        indirect = ctx.renderPaths(cam, opts, 4, 2, seed=7 + i, planes=("indirect",))["indirect"]
        acc, hist = ctx.temporalAccumulate(hits, indirect, prev_cam=prev, history=hist)
        prev = cam
        if i + 1 < FRAMES:
            scene.moveCamera(*MOVE)
            scene.rotateCamera(*ROTATE)
    albedo = ctx.renderShading(cam, opts, planes=("albedo",))["albedo"]
    hit = hits["node"] >= 0
    young = hit & (acc["age"] < 4)
    print("lecture5 %dx%d, frame %d of the sequence: %d of %d pixels hit, %d of them younger than 4 (%.1f %%)"
          % (W, H, FRAMES - 1, int(hit.sum()), px, int(young.sum()), 100.0 * young.sum() / max(int(hit.sum()), 1)))
    host = dict(node=hits["node"], normal=hits["normal"], p=hits["p"], rgb=hits["rgb"], albedo=albedo, acc=acc["colour"], variance=acc["variance"],
                age=acc["age"].astype(np.int32), zero=np.zeros((H, W), dtype=np.int32))
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in host.items()}
    t["indirect"] = torch.empty((H, W, 3), dtype=torch.float32, device=dev)

    def paths_launch():
        ctx.renderPathsDevice(cam, opts, a.paths, a.bounces, {"indirect": t["indirect"].data_ptr()}, seed=7, stream=stream)

    libs = [Lib("")] + [Lib(v) for v in a.variants.split(",") if v]
    yard = Lib(a.yardstick) if a.yardstick else None
    g = _abi.DenoiseGuides(node=t["node"].data_ptr(), normal=t["normal"].data_ptr(), p=t["p"].data_ptr(), albedo=t["albedo"].data_ptr(), base=t["rgb"].data_ptr())
    ov = [_abi.DenoiseVarianceOpts(width=W, height=H, levels=L, channels=3, normal_power_log2=5, sigma_plane=1.0, sigma_lum=4.0, var_floor=1e-8, min_age=4,
                                   reserved=0) for L in range(a.levels + 1)]
    od = [_abi.DenoiseOpts(width=W, height=H, levels=L, channels=3, normal_power_log2=5, sigma_plane=1.0, sigma_colour=0.5, reserved=0)
          for L in range(a.levels + 1)]
    need = max(int(lib.lib.c2rt_denoise_variance_scratch_bytes(C.byref(ov[a.levels]))) for lib in libs)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    outs = [torch.empty((H, W, 3), dtype=torch.float32, device=dev) for _ in libs]
    vouts = [torch.empty((H, W), dtype=torch.float32, device=dev) for _ in libs]
    yout = torch.empty((H, W, 3), dtype=torch.float32, device=dev)

    def run(k, L, age="age", vout=True):
        lib = libs[k]
        lib.check(lib.lib.c2rt_denoise_variance_device(lib.h, C.byref(g), C.byref(ov[L]), t["variance"].data_ptr(), t[age].data_ptr(), t["acc"].data_ptr(),
                                                       outs[k].data_ptr(), vouts[k].data_ptr() if vout else None, scratch.data_ptr(), stream))

    def run_yard(L):
        yard.check(yard.lib.c2rt_denoise_device(yard.h, C.byref(g), C.byref(od[L]), t["acc"].data_ptr(), yout.data_ptr(), scratch.data_ptr() if L else None,
                                                stream))

    for age in ("age", "zero"):                                    # warm-up of every shape, and the variants' outputs against the library's
        for k in range(len(libs)):
            for L in range(a.levels + 1):
                run(k, L, age)
            torch.cuda.synchronize()
            if k:
                d = int((outs[k].view(torch.int32) != outs[0].view(torch.int32)).sum()) + int((vouts[k].view(torch.int32) != vouts[0].view(torch.int32)).sum())
                print("%s against %s, %d levels, ages %s: %d of %d values differ" % (libs[k].name, libs[0].name, a.levels, age, d, px * 4))
    if yard:
        for L in range(a.levels + 1):
            run_yard(L)
    paths_launch()
    torch.cuda.synchronize()

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / calls

    src, dst = torch.empty(64 << 20, dtype=torch.uint8, device=dev), torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    T = {(k, L): [] for k in range(len(libs)) for L in range(a.levels + 1)}
    Ty = {k: [] for k in range(len(libs))}
    Ta = {(k, s): [] for k in range(len(libs)) for s in ("age", "zero", "none")}
    Td = {L: [] for L in range(a.levels + 1)}
    Tc, Tp = [], []
    for _ in range(a.rounds):
        for L in range(a.levels + 1):
            for k in range(len(libs)):
                T[k, L].append(window(lambda: run(k, L), a.calls))
            if yard:
                Td[L].append(window(lambda: run_yard(L), a.calls))
        for k in range(len(libs)):
            Ty[k].append(window(lambda: run(k, a.levels, "zero"), a.calls))
            Ta[k, "age"].append(window(lambda: run(k, 0, "age"), a.calls))
            Ta[k, "zero"].append(window(lambda: run(k, 0, "zero"), a.calls))
            Ta[k, "none"].append(window(lambda: run(k, 0, "age", vout=False), a.calls))
        Tc.append(window(lambda: dst.copy_(src), a.calls))
        Tp.append(window(paths_launch, 1))
    copy_rate = 2 * (64 << 20) / statistics.median(Tc) / 1e6
    print("(c) device copy of 64 MB                       %s  %.2f TB/s read + written" % (med(Tc), copy_rate))
    result = {"size": [W, H], "levels": a.levels, "young": int(young.sum()), "hit": int(hit.sum()), "paths_us": Tp, "copy_us": Tc, "libs": {}}
    level_bytes = px * 76
    for k, lib in enumerate(libs):
        print("%s:" % lib.name)
        for L in range(a.levels + 1):
            print("  (v %d) %d levels, steady ages   %s" % (L, L, med(T[k, L])))
        print("  (y)   %d levels, all young     %s" % (a.levels, med(Ty[k])))
        for s, what in (("age", "steady ages"), ("zero", "all young")):
            d = [x - y for x, y in zip(Ta[k, s], Ta[k, "none"])]
            print("  (a)   stage A alone, %-11s %s" % (what, med(d)))
        per = []
        for l in range(a.levels):
            d = [x - y for x, y in zip(T[k, l + 1], T[k, l])]
            per.append(d)
            m = statistics.median(d)
            print("  level %d (step %3d)%s  %s   %.0f MB algorithmic: %.2f TB/s, %.0f %% of the copy's rate"
                  % (l, 1 << l, " + packing" if l == 0 else "          ", med(d), level_bytes / 1e6, level_bytes / m / 1e6, 100 * level_bytes / m / 1e6 / copy_rate))
        result["libs"][lib.name] = {"calls_us": {L: T[k, L] for L in range(a.levels + 1)}, "all_young_us": Ty[k], "levels_us": per,
                                    "stage_a_us": {s: Ta[k, s] for s in ("age", "zero", "none")}}
    whole = statistics.median(T[0, a.levels])
    if yard:
        print("%s (the yardstick: c2rt_denoise_device, sigma_colour 0.5):" % yard.name)
        for L in range(a.levels + 1):
            print("  (d %d) %d levels                %s" % (L, L, med(Td[L])))
        for l in range(a.levels):
            print("  level %d                       %s" % (l, med([x - y for x, y in zip(Td[l + 1], Td[l])])))
        y = statistics.median(Td[a.levels])
        print("the variance-guided call over the yardstick's: %.2f (steady ages), %.2f (all young)" % (whole / y, statistics.median(Ty[0]) / y))
        result["yardstick_us"] = {L: Td[L] for L in range(a.levels + 1)}
    print("(p) c2rt_render_paths_device, indirect alone   %s  -> the %d-level filter adds %.2f %%" % (med(Tp), a.levels, 100 * whole / statistics.median(Tp)))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
