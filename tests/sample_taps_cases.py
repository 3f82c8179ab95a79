"""Shared by tests/test_sample_taps_abi.py (CPU) and tests/test_gpu_sample_taps.py (GPU): the four tap tables of the sample-table
tests and the golden-scene cases the adaptive ones run on."""
import os

import chess2rt_amd as c2
from chess2rt_amd import _abi
from golden_configs import SCENES

REF5 = c2.TAPS_REF5_TABLE
GRID16 = c2.tap_grid(4)
ODD7 = ((0.0, 0.0), (0.3, 0.3), (-0.25, 0.5), (0.875, 0.125), (1.5, -0.75), (0.1, 0.9), (0.6, 0.6))
SHIFT2 = ((0.5, 0.5), (0.25, 0.75))       # its first tap is not the corner: the whole-frame call only
# around the refinement kernel's pass of 8 taps: one extra tap, exactly one pass (8 extra), one pass and one tap (9 extra)
PAIR2 = ((0.0, 0.0), (0.5, 0.5))
GRID9 = c2.tap_grid(3)
TEN = GRID9 + ((0.9, 0.1),)

ADAPTIVE = [("lecture5.sdl", 67, 45), ("csg_stress.sdl", 96, 72)]
FULL_TILES = ("lecture5.sdl", 24, 17)     # under threshold 0: tiles with all 64 pixels flagged
ADAPTIVE_IDS = ["%s-%dx%d" % (s[:-4], w, h) for s, w, h in ADAPTIVE]


def make_scene(scene_file, width, height):
    """(scene, its camera's frame, one-tap options) of a golden scene at width x height, no AA, no lens"""
    scene = c2.parseSceneFromFile(os.path.join(SCENES, scene_file))
    scene.setFrameSize(width, height)
    scene.setAA(False)
    scene.setDof(False)
    return scene, scene.beginFrame(), scene.renderOpts(taps=_abi.TAPS_1)
