#!/usr/bin/env python3
"""A scene's camera with adaptive anti-aliasing through Context.renderFrameAdaptive: one ray per pixel, the reference's
edge test on the result, four more rays for the pixels it flags.  Writes the frame and the flags (white = refined).

  python examples/render_adaptive.py tests/golden/scenes/lecture5.sdl /tmp/frame.bmp /tmp/flags.bmp --size 640 480
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chess2rt_amd as c2
from chess2rt_amd import _abi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("frame_bmp")
    ap.add_argument("flags_bmp")
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), default=(640, 480))
    ap.add_argument("--threshold", type=float, default=_abi.AA_THRESHOLD_REF)
    args = ap.parse_args()
    scene = c2.parseSceneFromFile(args.scene)
    scene.setFrameSize(*args.size)
    scene.setDof(False)                                  # the edge test compares one ray per pixel: no lens
    cam = scene.beginFrame()
    ctx = c2.Context()
    ctx.uploadScene(scene.desc)
    frame, mask = ctx.renderFrameAdaptive(cam, scene.renderOpts(taps=_abi.TAPS_REF5), threshold=args.threshold)
    with open(args.frame_bmp, "wb") as f:
        f.write(c2.saveBmp(frame))
    with open(args.flags_bmp, "wb") as f:
        f.write(c2.saveBmp(np.repeat(mask.astype(np.float32)[..., None], 3, axis=2)))
    print("%s: %dx%d, %d of %d pixels refined (%.1f %%)" % (scene.name, args.size[0], args.size[1], int(mask.sum()), mask.size, 100.0 * mask.mean()))


if __name__ == "__main__":
    main()
