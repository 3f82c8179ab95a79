#!/usr/bin/env python3
"""Time of the a-trous filter (c2rt_denoise_device) on lecture5.sdl at 1920x1080, three channels, five levels, everything
resident in HBM; the guides are the context's own hit planes, the input the path planes' `indirect`.

  (d L)   the whole call with L = 0 .. levels levels (albedo and base given); level l alone is (d l+1) - (d l), taken
          round by round; L = 1 also holds the packing launch
  (t)     the route a caller has without the library's filter: the same arithmetic written in torch on the device, from
          the same planes — its device span between two events, and the host's wall clock around it with a sync (the
          span plus whatever launching some thousand small kernels costs the host); its output against ours, values that
          differ counted
  (p)     one c2rt_render_paths_device launch (`indirect` alone) at --paths / --bounces, for the share the filter adds

--variants a,b times libc2rt_a.so, libc2rt_b.so (make VARIANT=..., the Makefile's development knob) next to the library
itself, interleaved in the same rounds, and compares their outputs bit for bit: the A/B of a kernel form is a run of this
script.  Every window holds --calls calls behind a warm-up and lies between two device events; the legs are interleaved
--rounds times in one process; median [min..max] per call.

Algorithmic bytes of a level: the packed guides (32 B) and the input (4 B x channels) read once, the output written once,
per pixel; over the level's time, against HBM's 8.0 TB/s (the vendor's figure for the MI355X) and the 6.3 TB/s a float4
copy has been measured to reach on it.

  python scripts/denoise_rate.py [--rounds 9] [--calls 20] [--variants a,b] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import chess2rt_amd as c2
from chess2rt_amd import _abi

HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12


def med(v):
    return "%9.1f us [%.1f..%.1f]" % (statistics.median(v), min(v), max(v))


class Lib:
    """a build of the library and a context of its own on device 0 (the product library: the package's)"""

    def __init__(self, variant):
        self.name = variant or "libc2rt"
        if variant:
            self.lib = C.CDLL(os.path.join(ROOT, "chess2rt_amd", "libc2rt_%s.so" % variant), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)   # DEEPBIND: its own launchers, not the first library's
            for name in ("c2rt_init", "c2rt_destroy", "c2rt_last_error", "c2rt_denoise_device", "c2rt_denoise_scratch_bytes"):
                fn = getattr(self.lib, name)
                fn.restype, fn.argtypes = _abi.C2RT_SYMBOLS[name]
        else:
            self.lib = _abi.load_library()
        self.h = C.c_void_p()
        assert self.lib.c2rt_init(0, C.byref(self.h)) == 0

    def denoise(self, g, o, src, dst, scratch, stream):
        st = self.lib.c2rt_denoise_device(self.h, C.byref(g), C.byref(o), src, dst, scratch, stream)
        assert st == 0, self.lib.c2rt_last_error(self.h)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def torch_filter(node, normal, p, image, levels, power, sigma_plane, albedo, base):
    """the contract of include/c2rt.h in torch (no colour term), as tests/denoise_reference.py has it in numpy"""
    H, W = node.shape
    K = [1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16]
    nf, pf = normal.to(torch.float32), p.to(torch.float32)
    inv_plane = 1.0 / torch.tensor(sigma_plane, dtype=torch.float32, device=node.device)
    hit = node >= 0
    Cur = image
    for l in range(levels):
        s = 1 << l
        pad = 2 * s
        node_p = torch.nn.functional.pad(node, (pad, pad, pad, pad), value=-1)
        nf_p = torch.nn.functional.pad(nf, (0, 0, pad, pad, pad, pad))
        pf_p = torch.nn.functional.pad(pf, (0, 0, pad, pad, pad, pad))
        C_p = torch.nn.functional.pad(Cur, (0, 0, pad, pad, pad, pad))
        total, sumw = torch.zeros_like(Cur), torch.zeros((H, W), dtype=torch.float32, device=node.device)
        for j in range(-2, 3):
            for i in range(-2, 3):
                ys, xs = slice(pad + j * s, pad + j * s + H), slice(pad + i * s, pad + i * s + W)
                if i == 0 and j == 0:
                    w, keep, Ct = torch.full_like(sumw, K[2] * K[2]), hit, Cur
                else:
                    Ct = C_p[ys, xs]
                    nt = nf_p[ys, xs]
                    dn = dot3(nf, nt)
                    wn = dn
                    for _ in range(power):
                        wn = wn * wn
                    e = dot3(nf, pf_p[ys, xs] - pf) * inv_plane
                    w = ((K[i + 2] * K[j + 2]) * wn) * (1.0 / (1.0 + e * e))
                    keep = hit & (node_p[ys, xs] == node) & (dn > 0) & (w > 0)
                total = torch.where(keep[..., None], total + w[..., None] * Ct, total)
                sumw = torch.where(keep, sumw + w, sumw)
        Cur = torch.where(hit[..., None], total / sumw[..., None], Cur)
    return base + albedo * Cur


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--paths", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--variants", default="")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    W, H, px = a.width, a.height, a.width * a.height
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    scene = c2.parseSceneFromFile(os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl"))
    scene.setFrameSize(W, H)
    scene.setAA(False)
    scene.setDof(False)
    cam, opts = scene.beginFrame(), scene.renderOpts(taps=_abi.TAPS_1)
    ctx = c2.Context(0)
    ctx.uploadScene(scene.desc)
    t = dict(node=torch.empty((H, W), dtype=torch.int32, device=dev), normal=torch.empty((H, W, 3), dtype=torch.float64, device=dev),
             p=torch.empty((H, W, 3), dtype=torch.float64, device=dev), rgb=torch.empty((H, W, 3), dtype=torch.float32, device=dev),
             albedo=torch.empty((H, W, 3), dtype=torch.float32, device=dev), indirect=torch.empty((H, W, 3), dtype=torch.float32, device=dev))
    ctx.renderHitsDevice(cam, opts, {k: t[k].data_ptr() for k in ("node", "normal", "p", "rgb")}, stream=stream)
    ctx.renderShadingDevice(cam, opts, {"albedo": t["albedo"].data_ptr()}, stream=stream)

    def paths_launch():
        ctx.renderPathsDevice(cam, opts, a.paths, a.bounces, {"indirect": t["indirect"].data_ptr()}, seed=7, stream=stream)

    paths_launch()
    torch.cuda.synchronize()
    print("lecture5 %dx%d, %d paths x %d bounces: %d of %d pixels hit" % (W, H, a.paths, a.bounces, int((t["node"] >= 0).sum()), px))

    libs = [Lib("")] + [Lib(v) for v in a.variants.split(",") if v]
    g = _abi.DenoiseGuides(node=t["node"].data_ptr(), normal=t["normal"].data_ptr(), p=t["p"].data_ptr(), albedo=t["albedo"].data_ptr(), base=t["rgb"].data_ptr())
    o = [_abi.DenoiseOpts(width=W, height=H, levels=L, channels=3, normal_power_log2=5, sigma_plane=1.0, sigma_colour=0.0, reserved=0) for L in range(a.levels + 1)]
    scratch = torch.empty(max(c2.denoise_scratch_bytes(W, H, 3, a.levels), 16), dtype=torch.uint8, device=dev)
    outs = [torch.empty((H, W, 3), dtype=torch.float32, device=dev) for _ in libs]

    def run(k, L):
        libs[k].denoise(g, o[L], t["indirect"].data_ptr(), outs[k].data_ptr(), scratch.data_ptr() if L else None, stream)

    for k in range(len(libs)):                                       # warm-up of every shape, and the outputs against the library's
        for L in range(a.levels + 1):
            run(k, L)
        torch.cuda.synchronize()
        if k:
            same = int((outs[k].view(torch.int32) != outs[0].view(torch.int32)).sum())
            print("%s against %s, %d levels: %d of %d values differ" % (libs[k].name, libs[0].name, a.levels, same, px * 3))

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / calls

    T = {(k, L): [] for k in range(len(libs)) for L in range(a.levels + 1)}
    Tp = []
    for _ in range(a.rounds):
        for L in range(a.levels + 1):
            for k in range(len(libs)):
                T[k, L].append(window(lambda: run(k, L), a.calls))
        Tp.append(window(paths_launch, 1))
    result = {"size": [W, H], "levels": a.levels, "paths_us": Tp, "libs": {}}
    level_bytes = px * (32 + 12 + 12)
    for k, lib in enumerate(libs):
        print("%s:" % lib.name)
        for L in range(a.levels + 1):
            print("  (d %d) %d levels            %s" % (L, L, med(T[k, L])))
        per = []
        for l in range(a.levels):
            d = [x - y for x, y in zip(T[k, l + 1], T[k, l])]
            per.append(d)
            m = statistics.median(d)
            print("  level %d (step %3d)%s  %s   %.0f MB algorithmic: %.2f TB/s, %.0f %% of 8.0 TB/s (spec), %.0f %% of 6.3 TB/s (copy)"
                  % (l, 1 << l, " + packing" if l == 0 else "          ", med(d), level_bytes / 1e6, level_bytes / m / 1e6,
                     100 * level_bytes / (m * 1e-6) / HBM_SPEC, 100 * level_bytes / (m * 1e-6) / HBM_COPY))
        result["libs"][lib.name] = {"calls_us": {L: T[k, L] for L in range(a.levels + 1)}, "levels_us": per}
    whole = statistics.median(T[0, a.levels])
    print("(p) c2rt_render_paths_device, indirect alone   %s  -> the %d-level filter adds %.2f %%" % (med(Tp), a.levels, 100 * whole / statistics.median(Tp)))

    if not a.no_torch:
        def tf():
            return torch_filter(t["node"], t["normal"], t["p"], t["indirect"], a.levels, 5, 1.0, t["albedo"], t["rgb"])

        ref = tf()
        torch.cuda.synchronize()
        run(0, a.levels)
        torch.cuda.synchronize()
        diff = int((ref.view(torch.int32) != outs[0].view(torch.int32)).sum())
        span, wall = [], []
        for _ in range(max(3, a.rounds // 2)):
            t0 = time.perf_counter()
            span.append(window(tf, 1))
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e6 / 2)      # window() runs tf twice: once to settle, once timed
        print("(t) the same filter in torch: device span %s, host wall clock %s; %d of %d values differ from the library's"
              % (med(span), med(wall), diff, px * 3))
        print("    the library's call is %.1f x shorter than the span" % (statistics.median(span) / whole))
        result["torch"] = {"span_us": span, "wall_us": wall, "values_differing": diff}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
