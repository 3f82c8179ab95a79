#!/usr/bin/env python3
"""An orbit around a scene as a global-illumination SEQUENCE, frame by frame, with and without history.  Every frame
draws its own noise (seed + i); without history the speckle of the indirect light dances from frame to frame, with it
every pixel's world point is projected into the previous camera, the accumulated value is fetched where the surface is
the same one, and the new sample is folded into a running mean (Context.temporalAccumulate) before the a-trous filter
runs.  The script writes <stem>_NN_raw.bmp (the filter alone) and <stem>_NN_temporal.bmp (accumulation, then the filter)
for every frame — with --variance also <stem>_NN_variance.bmp, the accumulated plane through the variance-guided filter
(Context.denoiseVariance, fed by the accumulation's variance and age planes) — and prints, per frame, how many pixels found their history and the speckle of the indirect light — the mean
difference between neighbouring hit pixels — before and after the accumulation.

--posed NODE DX DY DZ slides one node of the scene by (DX, DY, DZ) per frame (Context.updateScene) while the camera orbits
— or stands still, with --step 0 0 — and hands the accumulation the node's two poses (temporalAccumulate's `motion`), so
that the sliding piece keeps its history as the board under it does; the script then also prints how many of the piece's
pixels found their history, against how many the plain call finds for the same frame.

--adaptive lets the history steer the sampler as well: frame 0 is traced with --young paths per pixel, every later frame
with the counts Context.pathCounts makes of the previous history (its variance at the point each pixel sees now, times the
count that variance was sampled with, times --paths-per-variance, within --min-paths .. --paths) through
Context.renderPathsCounted; the script prints the mean count per frame.  (Not together with --posed: the count rule does not
follow moved nodes.)

  python examples/render_temporal.py tests/golden/scenes/lecture5.sdl /tmp/orbit --size 640 480 --frames 8 --paths 4
  python examples/render_temporal.py tests/golden/scenes/lecture5.sdl /tmp/adaptive --adaptive --paths 32 --young 8
  python examples/render_temporal.py tests/golden/scenes/lecture5.sdl /tmp/slide --posed 1 4 0 -3 --step 0 0
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chess2rt_amd as c2


def write(path, image):
    with open(path, "wb") as f:
        f.write(c2.saveBmp(np.ascontiguousarray(image, dtype=np.float32)))
    return path


def roughness(image, hit):
    """mean absolute difference between horizontal neighbours that are both hits"""
    both = hit[:, 1:] & hit[:, :-1]
    return float(np.abs(image[:, 1:] - image[:, :-1])[both].mean()) if both.any() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("stem", help="the images are written as <stem>_NN_raw.bmp and <stem>_NN_temporal.bmp")
    ap.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), default=(640, 480))
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--paths", type=int, default=4)
    ap.add_argument("--step", type=float, nargs=2, metavar=("MOVE", "YAW"), default=(6.0, 2.0),
                    help="per frame: Camera.move to the right by MOVE, Camera.rotate by -YAW degrees, which keeps the scene's middle in view")
    ap.add_argument("--max-age", type=int, default=32, help="the running mean stops growing at this many samples")
    ap.add_argument("--min-normal-dot", type=float, default=0.9)
    ap.add_argument("--max-plane-dist", type=float, default=0.1)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--variance", action="store_true", help="also write <stem>_NN_variance.bmp: the variance-guided filter of the accumulated plane")
    ap.add_argument("--sigma-lum", type=float, default=4.0, help="--variance: luminance differences count in local standard deviations times this")
    ap.add_argument("--min-age", type=int, default=4, help="--variance: pixels younger than this take a spatial variance estimate")
    ap.add_argument("--posed", type=float, nargs=4, metavar=("NODE", "DX", "DY", "DZ"),
                    help="slide node NODE by (DX, DY, DZ) per frame and let the accumulation follow it")
    ap.add_argument("--adaptive", action="store_true", help="trace each pixel with the number of paths its history's variance asks for; --paths is the cap")
    ap.add_argument("--min-paths", type=int, default=2, help="--adaptive: the fewest paths of a pixel with a history")
    ap.add_argument("--young", type=int, default=None, help="--adaptive: paths of a pixel without a history (default: --paths)")
    ap.add_argument("--paths-per-variance", type=float, default=2000.0, help="--adaptive: paths asked for per unit of per-path luminance variance")
    args = ap.parse_args()
    if args.adaptive and args.posed:
        sys.exit("--adaptive: the count rule does not follow moved nodes; not together with --posed")
    scene = c2.parseSceneFromFile(args.scene)
    scene.setFrameSize(*args.size)
    scene.setAA(False)
    scene.setDof(False)
    depth = max(1, min(scene.settings.max_trace_depth, 8))
    ctx = c2.Context()
    ctx.uploadScene(scene.desc)
    opts = scene.renderOpts()
    prev_cam, history, counts = None, None, None
    young = min(args.young or args.paths, args.paths)
    node, pose, prev_pose = None, None, None
    if args.posed:
        node = int(args.posed[0])
        desc = scene.desc.contents
        if not 0 <= node < desc.n_nodes:
            sys.exit("--posed: the scene has nodes 0 .. %d" % (desc.n_nodes - 1))
        base = np.ctypeslib.as_array(desc.node_transform, shape=(desc.n_nodes, 30))[node].copy()
    for i in range(args.frames):
        cam = scene.beginFrame()
        motion = None
        if args.posed:
            pose = base.copy()
            pose[27:30] += i * np.array(args.posed[1:])          # the offset: Transform.translate
            ctx.updateScene(nodes={node: pose})
            motion = {node: (prev_pose, pose)} if i else {}
        hits = ctx.renderHits(cam, opts, planes=("node", "normal", "p", "rgb"))
        albedo = ctx.renderShading(cam, opts, planes=("albedo",))["albedo"]
        if args.adaptive:
            if i == 0:
                counts = np.full(hits["node"].shape, young, dtype=np.uint8)
            else:
                counts = ctx.pathCounts(hits, prev_cam=prev_cam, history=history, prev_counts=counts, min_paths=args.min_paths, max_paths=args.paths,
                                        young_paths=young, paths_per_variance=args.paths_per_variance, prev_paths=young,
                                        min_normal_dot=args.min_normal_dot, max_plane_dist=args.max_plane_dist, planes=())["counts"]
            indirect = ctx.renderPathsCounted(cam, opts, counts, args.paths, depth, seed=args.seed + i, planes=("indirect",))["indirect"]
            on = hits["node"] >= 0
            print("frame %2d: %.2f paths per hit pixel (%d .. %d), %.1f %% of them at the cap of %d"
                  % (i, float(counts[on].mean()) if on.any() else 0.0, int(counts[on].min()) if on.any() else 0, int(counts[on].max()) if on.any() else 0,
                     100.0 * float((counts[on] >= args.paths).mean()) if on.any() else 0.0, args.paths))
        else:
            indirect = ctx.renderPaths(cam, opts, args.paths, depth, seed=args.seed + i, planes=("indirect",))["indirect"]
        if args.posed and i:
            plain = ctx.temporalAccumulate(hits, indirect, prev_cam=prev_cam, history=history, max_age=args.max_age, min_normal_dot=args.min_normal_dot,
                                           max_plane_dist=args.max_plane_dist, planes=("age",))[0]["age"]
        acc, history = ctx.temporalAccumulate(hits, indirect, prev_cam=prev_cam, history=history, max_age=args.max_age,
                                              min_normal_dot=args.min_normal_dot, max_plane_dist=args.max_plane_dist, motion=motion)
        frames = {"raw": ctx.denoise(hits, indirect, levels=args.levels, albedo=albedo, base=hits["rgb"]),
                  "temporal": ctx.denoise(hits, acc["colour"], levels=args.levels, albedo=albedo, base=hits["rgb"])}
        if args.variance:
            frames["variance"] = ctx.denoiseVariance(hits, acc["colour"], acc["variance"], acc["age"], levels=args.levels, sigma_lum=args.sigma_lum,
                                                     min_age=args.min_age, albedo=albedo, base=hits["rgb"], variance_out=False)[0]
        hit = hits["node"] >= 0
        found = int((acc["age"] > 1).sum())
        print("frame %2d: %5.1f %% of the hit pixels found their history, mean age %.1f; neighbour-to-neighbour difference of the indirect light %.4f -> %.4f"
              % (i, 100.0 * found / max(int(hit.sum()), 1), float(acc["age"][hit].mean()) if hit.any() else 0.0, roughness(indirect, hit),
                 roughness(acc["colour"], hit)))
        if args.posed and i:
            on = hits["node"] == node
            print("          node %d: %d pixels, %d found their history through its two poses, %d through the plain call"
                  % (node, int(on.sum()), int((acc["age"][on] > 1).sum()), int((plain[on] > 1).sum())))
        for k, image in frames.items():
            write("%s_%02d_%s.bmp" % (args.stem, i, k), image)
        prev_cam, prev_pose = cam, pose
        scene.moveCamera(args.step[0], 0.0, 0.0)
        scene.rotateCamera(-args.step[1], 0.0, 0.0)
    print("wrote %d frames %s under %s_*" % (args.frames, "three times" if args.variance else "twice", args.stem))


if __name__ == "__main__":
    main()
