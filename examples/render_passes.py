#!/usr/bin/env python3
"""The render passes of a scene's camera through Context.renderShading: one call, one launch, and the terms of every
pixel's colour come back apart — the material colour (albedo), the light that reaches the surface, Phong's highlight and,
per light, the shadow mask.  The passes recombine to the frame, rgb == albedo * light (+ specular on a Phong node), bit
for bit; the script asserts it on what it got before it writes <stem>_albedo.bmp, <stem>_light.bmp, <stem>_specular.bmp,
<stem>_beauty.bmp and <stem>_shadow_<l>.bmp (white: light l reaches the pixel, grey: it does not, black: no surface).

  python examples/render_passes.py tests/golden/scenes/lecture5.sdl /tmp/passes --size 640 480
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chess2rt_amd as c2
from chess2rt_amd import _abi


def write(path, image):
    with open(path, "wb") as f:
        f.write(c2.saveBmp(np.ascontiguousarray(image, dtype=np.float32)))
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("stem", help="the images are written as <stem>_<pass>.bmp")
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), default=(640, 480))
    args = ap.parse_args()
    scene = c2.parseSceneFromFile(args.scene)
    scene.setFrameSize(*args.size)
    scene.setAA(False)
    scene.setDof(False)                                  # a pixel's terms are one ray's: no lens
    d = scene.desc.contents
    ctx = c2.Context()
    ctx.uploadScene(scene.desc)
    pl = ctx.renderShading(scene.beginFrame(), scene.renderOpts())
    node, hit = pl["node"], pl["node"] >= 0

    # the reference's own last statement, in float32: Lambert returns diffuse * lightContrib, Phong adds its specular
    shader = np.array([d.node_shader[i] for i in range(d.n_nodes)], dtype=np.int64)
    phong_shader = np.array([d.shader_type[i] for i in range(d.n_shaders)]) == _abi.SHADER_PHONG
    phong = np.zeros(node.shape, dtype=bool)
    phong[hit] = phong_shader[shader[node[hit]]]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        res = pl["albedo"] * pl["light"]
        again = np.where(phong[..., None], res + pl["specular"], res).astype(np.float32)
    same = (again.view(np.uint32) == pl["rgb"].view(np.uint32)) | (np.isnan(again) & np.isnan(pl["rgb"]))
    assert same[hit].all(), "the passes do not recombine to the frame"
    assert not pl["rgb"][~hit].view(np.uint32).any() and not pl["visible"][~hit].any()

    files = [write(args.stem + "_albedo.bmp", pl["albedo"]), write(args.stem + "_light.bmp", pl["light"]),
             write(args.stem + "_specular.bmp", pl["specular"]), write(args.stem + "_beauty.bmp", pl["rgb"])]
    for l in range(min(d.n_lights, 32)):
        reached = ((pl["visible"] >> np.uint32(l)) & 1).astype(bool)
        mask = np.where(hit, np.where(reached, 1.0, 0.25), 0.0).astype(np.float32)
        files.append(write("%s_shadow_%d.bmp" % (args.stem, l), np.repeat(mask[..., None], 3, axis=2)))
    print("%s: %dx%d, %d of %d pixels hit, %d on Phong nodes, %d in the shadow of every light; the passes recombine bit for bit"
          % (scene.name, args.size[0], args.size[1], int(hit.sum()), node.size, int(phong.sum()), int((hit & (pl["visible"] == 0)).sum())))
    print("\n".join(files))


if __name__ == "__main__":
    main()
