#!/usr/bin/env python3
"""One scene at four sampling patterns through the sample-table calls: one tap, the reference's five, a 4x4 grid over the
whole frame (Context.renderFrameTaps), and the 4x4 grid on the pixels the edge test flags only
(Context.renderFrameAdaptiveTaps).  Writes taps1.bmp, taps5.bmp, taps16.bmp, adaptive16.bmp and adaptive16_flags.bmp (white
= refined) into the output directory.

  python examples/render_supersampled.py tests/golden/scenes/lecture5.sdl /tmp/supersampled --size 640 480
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chess2rt_amd as c2
from chess2rt_amd import _abi


def write(path, rgb):
    with open(path, "wb") as f:
        f.write(c2.saveBmp(rgb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("out_dir")
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), default=(640, 480))
    ap.add_argument("--threshold", type=float, default=_abi.AA_THRESHOLD_REF)
    args = ap.parse_args()
    scene = c2.parseSceneFromFile(args.scene)
    scene.setFrameSize(*args.size)
    scene.setDof(False)                                  # a tap is one ray: no lens
    cam = scene.beginFrame()
    opts = scene.renderOpts(taps=_abi.TAPS_1)            # the table is the pattern: opts.taps is ignored
    ctx = c2.Context()
    ctx.uploadScene(scene.desc)
    os.makedirs(args.out_dir, exist_ok=True)
    grid = c2.tap_grid(4)
    for name, table in (("taps1", c2.tap_grid(1)), ("taps5", c2.TAPS_REF5_TABLE), ("taps16", grid)):
        write(os.path.join(args.out_dir, name + ".bmp"), ctx.renderFrameTaps(cam, opts, table))
    frame, mask = ctx.renderFrameAdaptiveTaps(cam, opts, grid, threshold=args.threshold)
    write(os.path.join(args.out_dir, "adaptive16.bmp"), frame)
    write(os.path.join(args.out_dir, "adaptive16_flags.bmp"), np.repeat(mask.astype(np.float32)[..., None], 3, axis=2))
    print("%s: %dx%d at 1, 5 and 16 taps; adaptive: %d of %d pixels refined to 16 taps (%.1f %%)"
          % (scene.name, args.size[0], args.size[1], int(mask.sum()), mask.size, 100.0 * mask.mean()))


if __name__ == "__main__":
    main()
