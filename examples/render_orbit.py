#!/usr/bin/env python3
"""A turn of the camera in N steps, rendered with ONE call (Context.renderFrames: one mask pre-pass launch and one
frame launch for all N frames) and saved as N BMPs.

  python examples/render_orbit.py tests/golden/scenes/lecture5.sdl /tmp/orbit --frames 16 --size 640 360
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chess2rt_amd as c2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("out_prefix")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"))
    ap.add_argument("--no-aa", action="store_true")
    args = ap.parse_args()
    scene = c2.parseSceneFromFile(args.scene)
    if args.size:
        scene.setFrameSize(*args.size)
    if args.no_aa:
        scene.setAA(False)
    scene.setDof(False)                    # a batch renders pinhole cameras; depth of field goes frame by frame
    cams = []
    for _ in range(args.frames):
        cams.append(scene.beginFrame())
        scene.rotateCamera(360.0 / args.frames, 0, 0)
    ctx = c2.Context()
    ctx.uploadScene(scene.desc)
    t = time.perf_counter()
    frames = ctx.renderFrames(cams, scene.renderOpts())   # (N, H, W, 3) float32 linear RGB
    dt = time.perf_counter() - t
    for i, frame in enumerate(frames):
        with open("%s_%03d.bmp" % (args.out_prefix, i), "wb") as f:
            f.write(c2.saveBmp(frame))
    print("%s: %d frames of %dx%d in one call, %.2f ms incl. the copy back" % (scene.name, len(frames), frames.shape[2], frames.shape[1], dt * 1e3))


if __name__ == "__main__":
    main()
