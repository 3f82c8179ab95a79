"""Shared by tests/test_temporal_abi.py (CPU) and tests/test_gpu_temporal.py (GPU): the camera sequences of the temporal
tests and their options.  A sequence starts at the scene's shipped camera and repeats ONE step, Camera.move then
Camera.rotate; the step was chosen so that the first pair alone puts pixels and taps into every class of the
reprojection on both scenes (test_temporal_abi.py shows that from the oracle).  The scenes are parsed here, apart from
occlusion_cases.load, whose shared scene objects keep their shipped cameras."""
import functools
import os

import chess2rt_amd as c2
import occlusion_cases as oc
from chess2rt_amd import _abi
from golden_configs import SCENES

W, H = oc.W, oc.H
N_FRAMES = 4
MOVE, ROTATE = (10.0, 2.0, 5.0), (8.0, 0.0, 3.0)      # moveCamera(dx, dy, dz), rotateCamera(dyaw, droll, dpitch)
MIN_NORMAL_DOT, MAX_PLANE_DIST = 0.9, 0.1


@functools.lru_cache(maxsize=None)
def sequence(name, width=W, height=H, n=N_FRAMES):
    """(scene, (camera 0 .. n-1), options): camera 0 is the scene's own, camera i + 1 one step further"""
    scene = c2.parseSceneFromFile(os.path.join(SCENES, name + ".sdl"))
    scene.setFrameSize(width, height)
    scene.setAA(False)
    scene.setDof(False)
    cams = [scene.beginFrame()]
    for _ in range(n - 1):
        scene.moveCamera(*MOVE)
        scene.rotateCamera(*ROTATE)
        cams.append(scene.beginFrame())
    return scene, tuple(cams), scene.renderOpts(taps=_abi.TAPS_1)
