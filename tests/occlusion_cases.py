"""Shared by tests/test_occlusion_abi.py (CPU) and tests/test_gpu_occlusion.py (GPU): the two scenes, their ray sets and
the options of the occlusion tests, loaded once and read-only."""
import functools
import os

import numpy as np

import chess2rt_amd as c2
from chess2rt_amd import _abi
from golden_configs import SCENES
from ray_query_util import eyeless_rays, screen_rays

W, H = 61, 47
K = 16
SEED = 7
RAY_SEED = 11
N_EYELESS = 2000                                  # 31 waves and a quarter: the last wave is partial
RADIUS = {"lecture5": 120.0, "csg_stress": 40.0}
SCENE_NAMES = tuple(RADIUS)
RAY_SETS = ("screen", "eyeless")


@functools.lru_cache(maxsize=None)
def load(name, width=W, height=H):
    """(scene, camera, options) of the scene as shipped, at width x height, AA and depth of field off"""
    scene = c2.parseSceneFromFile(os.path.join(SCENES, name + ".sdl"))
    scene.setFrameSize(width, height)
    scene.setAA(False)
    scene.setDof(False)
    return scene, scene.beginFrame(), scene.renderOpts(taps=_abi.TAPS_1)


@functools.lru_cache(maxsize=None)
def ray_set(name, which):
    scene, cam, _ = load(name)
    rays = screen_rays(cam, W, H) if which == "screen" else eyeless_rays(scene.desc, RAY_SEED, N_EYELESS)
    rays = np.ascontiguousarray(rays)
    rays.setflags(write=False)
    return rays
