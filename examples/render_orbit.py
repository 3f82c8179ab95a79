#!/usr/bin/env python3
"""A turn of the camera in N steps, rendered with ONE call (Context.renderFrames: one mask pre-pass launch and one
frame launch for all N frames) and saved as N BMPs.  With --adaptive the call is Context.renderFramesAdaptive: one ray
per pixel, the edge test, and four more rays only where it flags — one detection and one refinement launch for all N
frames; the flags are saved next to the frames.

  python examples/render_orbit.py tests/golden/scenes/lecture5.sdl /tmp/orbit --frames 16 --size 640 360
  python examples/render_orbit.py tests/golden/scenes/lecture5.sdl /tmp/orbit --frames 16 --size 640 360 --adaptive
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import chess2rt_amd as c2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("out_prefix")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"))
    ap.add_argument("--no-aa", action="store_true")
    ap.add_argument("--adaptive", action="store_true", help="five taps only where the edge test flags (implies anti-aliasing)")
    args = ap.parse_args()
    scene = c2.parseSceneFromFile(args.scene)
    if args.size:
        scene.setFrameSize(*args.size)
    if args.no_aa and args.adaptive:
        ap.error("--adaptive refines to five taps: not with --no-aa")
    if args.no_aa:
        scene.setAA(False)
    if args.adaptive:
        scene.setAA(True)
    scene.setDof(False)                    # a batch renders pinhole cameras; depth of field goes frame by frame
    cams = []
    for _ in range(args.frames):
        cams.append(scene.beginFrame())
        scene.rotateCamera(360.0 / args.frames, 0, 0)
    ctx = c2.Context()
    ctx.uploadScene(scene.desc)
    t = time.perf_counter()
    masks = None
    if args.adaptive:
        frames, masks = ctx.renderFramesAdaptive(cams, scene.renderOpts())   # + (N, H, W) uint8 flags
    else:
        frames = ctx.renderFrames(cams, scene.renderOpts())   # (N, H, W, 3) float32 linear RGB
    dt = time.perf_counter() - t
    for i, frame in enumerate(frames):
        with open("%s_%03d.bmp" % (args.out_prefix, i), "wb") as f:
            f.write(c2.saveBmp(frame))
        if masks is not None:
            with open("%s_%03d_flags.bmp" % (args.out_prefix, i), "wb") as f:
                f.write(c2.saveBmp(np.repeat(masks[i][..., None], 3, axis=2).astype(np.float32)))
    if masks is not None:
        print("adaptive: %.2f %% of the pixels took five rays" % (100.0 * float(masks.mean())))
    print("%s: %d frames of %dx%d in one call, %.2f ms incl. the copy back" % (scene.name, len(frames), frames.shape[2], frames.shape[1], dt * 1e3))


if __name__ == "__main__":
    main()
