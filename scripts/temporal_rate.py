#!/usr/bin/env python3
"""Time of the temporal accumulation (c2rt_temporal_accumulate_device) on lecture5.sdl, everything resident in HBM: the
guides are the context's own hit planes of a camera one small step (Camera.move, Camera.rotate) past the camera whose
frame left the history, so that the motion is coherent; the input is the path planes' `indirect` (one channel: its red).

  (t W H C)  the call at W x H with C channels, all three planes asked for, against a previous history
  (f W H C)  the same with no previous history (the first frame: no gather)
  (l)        ONE a-trous level of c2rt_denoise_device at the same size, three channels: the call with two levels minus the
             call with one, taken round by round
  (p)        one c2rt_render_paths_device launch (`indirect` alone) at --paths / --bounces

--variants a,b times libc2rt_a.so, libc2rt_b.so (builds that differ in c2rt_temporal.o) next to the library itself,
interleaved in the same rounds, and compares their planes and histories bit for bit: the A/B of a lane mapping is a run of
this script.  Every window holds --calls calls behind a warm-up and lies between two device events; the legs are
interleaved --rounds times in one process; median [min..max] per call.

Algorithmic bytes per pixel: 52 of guides and 4 C of input read, about 32 + 4 C + 8 of history read where the motion is
coherent, as much written, and 4 C + 8 of planes written; over the call's time, against HBM's 8.0 TB/s (the vendor's
figure for the MI355X) and the 6.3 TB/s a float4 copy has been measured to reach on it (profiles/denoise.md).

  python scripts/temporal_rate.py [--sizes 1920x1080,3840x2160] [--rounds 9] [--calls 20] [--variants a,b] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import chess2rt_amd as c2
from chess2rt_amd import _abi

HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12
MIN_NORMAL_DOT, MAX_PLANE_DIST, MAX_AGE = 0.9, 0.1, 32


def med(v):
    return "%9.1f us [%.1f..%.1f]" % (statistics.median(v), min(v), max(v))


class Lib:
    """a build of the library and a context of its own on device 0 (the product library: the package's)"""

    def __init__(self, variant):
        self.name = variant or "libc2rt"
        if variant:
            self.lib = C.CDLL(os.path.join(ROOT, "chess2rt_amd", "libc2rt_%s.so" % variant), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)   # DEEPBIND: its own launchers, not the first library's
            for name in ("c2rt_init", "c2rt_destroy", "c2rt_last_error", "c2rt_temporal_accumulate_device"):
                fn = getattr(self.lib, name)
                fn.restype, fn.argtypes = _abi.C2RT_SYMBOLS[name]
        else:
            self.lib = _abi.load_library()
        self.h = C.c_void_p()
        assert self.lib.c2rt_init(0, C.byref(self.h)) == 0

    def accumulate(self, cam, g, o, src, prev, out, planes, stream):
        st = self.lib.c2rt_temporal_accumulate_device(self.h, None if cam is None else C.byref(cam), C.byref(g), C.byref(o), src, prev, out, C.byref(planes), stream)
        assert st == 0, self.lib.c2rt_last_error(self.h)


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--paths", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--variants", default="")
    ap.add_argument("--json")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    ctx = c2.Context(0)
    libs = [Lib("")] + [Lib(v) for v in a.variants.split(",") if v]
    result = {"sizes": {}}
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        px = W * H
        scene = c2.parseSceneFromFile(os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl"))
        scene.setFrameSize(W, H)
        scene.setAA(False)
        scene.setDof(False)
        opts = scene.renderOpts(taps=_abi.TAPS_1)
        cams = [scene.beginFrame()]
        scene.moveCamera(1.0, 0.2, 0.5)
        scene.rotateCamera(0.8, 0.0, 0.3)
        cams.append(scene.beginFrame())
        ctx.uploadScene(scene.desc)

        def planes_of(cam, seed):
            t = dict(node=torch.empty((H, W), dtype=torch.int32, device=dev), normal=torch.empty((H, W, 3), dtype=torch.float64, device=dev),
                     p=torch.empty((H, W, 3), dtype=torch.float64, device=dev), indirect=torch.empty((H, W, 3), dtype=torch.float32, device=dev))
            ctx.renderHitsDevice(cam, opts, {k: t[k].data_ptr() for k in ("node", "normal", "p")}, stream=stream)
            ctx.renderPathsDevice(cam, opts, a.paths, a.bounces, {"indirect": t["indirect"].data_ptr()}, seed=seed, stream=stream)
            torch.cuda.synchronize()
            t["red"] = t["indirect"][..., 0].contiguous()
            return t

        f0, f1 = planes_of(cams[0], 7), planes_of(cams[1], 8)

        def paths_launch():
            ctx.renderPathsDevice(cams[1], opts, a.paths, a.bounces, {"indirect": f1["indirect"].data_ptr()}, seed=8, stream=stream)

        print("lecture5 %dx%d: %d of %d pixels hit" % (W, H, int((f1["node"] >= 0).sum()), px))
        entry = {"temporal_us": {}, "first_us": {}}
        T, Tf = {}, {}
        state = {}
        for ch in (3, 1):
            o = _abi.TemporalOpts(width=W, height=H, channels=ch, max_age=MAX_AGE, min_normal_dot=MIN_NORMAL_DOT, max_plane_dist=MAX_PLANE_DIST)
            need = c2.temporal_history_bytes(W, H, ch)
            src0, src1 = (f["indirect"] if ch == 3 else f["red"] for f in (f0, f1))
            g0 = _abi.TemporalGuides(node=f0["node"].data_ptr(), normal=f0["normal"].data_ptr(), p=f0["p"].data_ptr())
            g1 = _abi.TemporalGuides(node=f1["node"].data_ptr(), normal=f1["normal"].data_ptr(), p=f1["p"].data_ptr())
            prev = torch.empty(need, dtype=torch.uint8, device=dev)
            none = _abi.TemporalPlanes()
            libs[0].accumulate(None, g0, o, src0.data_ptr(), None, prev.data_ptr(), none, stream)
            outs = []
            for k, lib in enumerate(libs):
                buf = dict(hist=torch.empty(need, dtype=torch.uint8, device=dev), colour=torch.empty((H, W, ch), dtype=torch.float32, device=dev),
                           variance=torch.empty((H, W), dtype=torch.float32, device=dev), age=torch.empty((H, W), dtype=torch.int32, device=dev))
                buf["planes"] = _abi.TemporalPlanes(colour=buf["colour"].data_ptr(), variance=buf["variance"].data_ptr(), age=buf["age"].data_ptr())
                outs.append(buf)
                lib.accumulate(cams[0], g1, o, src1.data_ptr(), prev.data_ptr(), buf["hist"].data_ptr(), buf["planes"], stream)
                torch.cuda.synchronize()
                if k:
                    differ = sum(int((buf[n].view(torch.uint8) != outs[0][n].view(torch.uint8)).sum()) for n in ("hist", "colour", "variance", "age"))
                    print("%s against %s, %d channels: %d bytes of planes and history differ" % (lib.name, libs[0].name, ch, differ))
            age = outs[0]["age"]
            print("  %d channels: %d pixels found their history (age 2), %d restarted, %d missed" % (ch, int((age == 2).sum()), int((age == 1).sum()), int((age == 0).sum())))
            state[ch] = (o, g1, src1, prev, outs)
            for k in range(len(libs)):
                T[k, ch], Tf[k, ch] = [], []

        do = [_abi.DenoiseOpts(width=W, height=H, levels=L, channels=3, normal_power_log2=5, sigma_plane=1.0, sigma_colour=0.0, reserved=0) for L in (1, 2)]
        dg = _abi.DenoiseGuides(node=f1["node"].data_ptr(), normal=f1["normal"].data_ptr(), p=f1["p"].data_ptr())
        scratch = torch.empty(c2.denoise_scratch_bytes(W, H, 3, 2), dtype=torch.uint8, device=dev)
        dout = torch.empty((H, W, 3), dtype=torch.float32, device=dev)

        def denoise(L):
            ctx.denoiseDevice({"node": dg.node, "normal": dg.normal, "p": dg.p}, W, H, f1["indirect"].data_ptr(), dout.data_ptr(), scratch.data_ptr(), levels=L,
                              stream=stream)

        def run(k, ch, first):
            o, g1, src1, prev, outs = state[ch]
            libs[k].accumulate(None if first else cams[0], g1, o, src1.data_ptr(), None if first else prev.data_ptr(), outs[k]["hist"].data_ptr(),
                               outs[k]["planes"], stream)

        Tl, Tp = [], []
        for _ in range(a.rounds):
            for ch in (3, 1):
                for k in range(len(libs)):
                    T[k, ch].append(window(lambda: run(k, ch, False), a.calls))
                    Tf[k, ch].append(window(lambda: run(k, ch, True), a.calls))
            d1, d2 = window(lambda: denoise(1), a.calls), window(lambda: denoise(2), a.calls)
            Tl.append(d2 - d1)
            Tp.append(window(paths_launch, 1))
        for k, lib in enumerate(libs):
            print("%s:" % lib.name)
            for ch in (3, 1):
                nbytes = px * (52 + 4 * ch + 2 * (32 + 4 * ch + 8) + 4 * ch + 8)
                m = statistics.median(T[k, ch])
                print("  (t %d %d %d) with history  %s   %.0f MB algorithmic: %.2f TB/s, %.0f %% of 8.0 TB/s (spec), %.0f %% of 6.3 TB/s (copy: %.1f us)"
                      % (W, H, ch, med(T[k, ch]), nbytes / 1e6, nbytes / m / 1e6, 100 * nbytes / (m * 1e-6) / HBM_SPEC, 100 * nbytes / (m * 1e-6) / HBM_COPY,
                         nbytes / HBM_COPY * 1e6))
                print("  (f %d %d %d) first frame   %s" % (W, H, ch, med(Tf[k, ch])))
            entry["temporal_us"][lib.name] = {ch: T[k, ch] for ch in (3, 1)}
            entry["first_us"][lib.name] = {ch: Tf[k, ch] for ch in (3, 1)}
        whole = statistics.median(T[0, 3])
        print("(l) one a-trous level (two levels minus one), 3 channels   %s  -> the accumulation is %.2f of a level" % (med(Tl), whole / statistics.median(Tl)))
        print("(p) c2rt_render_paths_device, indirect alone, %d x %d   %s  -> the accumulation adds %.2f %%"
              % (a.paths, a.bounces, med(Tp), 100 * whole / statistics.median(Tp)))
        entry["level_us"], entry["paths_us"] = Tl, Tp
        result["sizes"][size] = entry
        del state, f0, f1, scratch, dout
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
