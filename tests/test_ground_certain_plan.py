"""Which frames the planner hands to the short chain for ground tiles (RenderParams::ground_certain_cq,
chess2rt_amd/csrc/scene_plan.cpp: fill_params; ground_certain.h: gc_plan), through the planner's host build
tests/libground_certain_check.so — no GPU.  The scenes are those of tests/test_gpu_ground_certain.py, whose `route`
column this holds to the library's decision."""
import ctypes as C
import os

import pytest

import chess2rt_amd as c2
from chess2rt_amd import _abi

import test_gpu_ground_certain as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def certain():
    L = C.CDLL(os.path.join(ROOT, "tests", "libground_certain_check.so"))
    L.c2rt_ground_certain_of.argtypes = [C.c_void_p, C.POINTER(_abi.CameraFrame), C.POINTER(_abi.RenderOpts), C.c_int, C.POINTER(C.c_uint32)]
    L.c2rt_ground_certain_of.restype = C.c_double

    def of(scene, cam, opts, debug_cull=0):
        fast = C.c_uint32(7)
        cq = L.c2rt_ground_certain_of(C.cast(scene.desc, C.c_void_p), C.byref(cam), C.byref(opts), debug_cull, C.byref(fast))
        assert cq >= 0 and fast.value in (0, 1)
        if cq > 0:  # only ever on top of the ground-tile path
            assert fast.value == 1
        return cq

    return of


def _load(tmp_path, case):
    path = tmp_path / (case["name"] + ".sdl")
    path.write_text(case["sdl"])
    scene = c2.parseSceneFromFile(str(path))
    scene.setFrameSize(case["W"], case["H"])
    cam = scene.beginFrame()
    if case["down"]:
        T.look_down(cam, case)
    if case["limit"]:
        scene.desc.contents.geom_param[1] = case["limit"]
    return scene, cam, scene.renderOpts(taps=case["taps"])


@pytest.mark.parametrize("case", [c for c in T._cases() if c["kind"] == "frame" and c["world"] == 1], ids=lambda c: c["name"])
def test_the_gpu_cases_take_the_route_their_table_says(certain, tmp_path, case):
    scene, cam, opts = _load(tmp_path, case)
    cq = certain(scene, cam, opts)
    print(case["name"], cq)
    if case["route"] == "refused":
        assert cq == 0
    if case["route"] == "taken":
        assert cq > 0
        # cq is the header's constant, not below 2 |o.x| + 2 |o.z| + |L.x| + |L.z|
        L = scene.desc.contents.light_pos
        assert cq >= 2 * abs(cam.pos[0]) + 2 * abs(cam.pos[2]) + abs(L[0]) + abs(L[2])
    assert certain(scene, cam, opts, debug_cull=64) == 0  # the diagnostics switch
    assert certain(scene, cam, opts, debug_cull=16) == 0  # and there is no short chain without the ground-tile path


def test_frames_the_route_is_not_built_for(certain, tmp_path):
    case = T._cases()[0]
    scene, cam, opts = _load(tmp_path, case)
    assert certain(scene, cam, opts) > 0
    assert certain(scene, cam, scene.renderOpts(taps=case["taps"], count_rays=1)) == 0
    below = _abi.CameraFrame.from_buffer_copy(cam)
    below.pos[1] = -165.0  # the eye under the floor
    assert certain(scene, below, opts) == 0
    on = _abi.CameraFrame.from_buffer_copy(cam)
    on.pos[1] = -0.01  # at the floor's height
    assert certain(scene, on, opts) == 0
    far = _abi.CameraFrame.from_buffer_copy(cam)
    far.pos[0] = 2.0 ** 41
    assert certain(scene, far, opts) == 0
    high = _abi.CameraFrame.from_buffer_copy(cam)
    high.pos[1] = 16 * 700.02 + 1  # more than 16 light heights up
    assert certain(scene, high, opts) == 0
