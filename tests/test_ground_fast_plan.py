"""Which frames the planner hands to the ground-tile path (RenderParams::ground_fast, chess2rt_amd/csrc/scene_plan.cpp:
fill_params), through the planner's host build tests/libground_fast_check.so — no GPU.  The scenes are those of
tests/test_gpu_ground_tiles.py, whose `eligible` column this holds to the library's decision."""
import ctypes as C
import os

import pytest

import chess2rt_amd as c2
from chess2rt_amd import _abi

import test_gpu_ground_tiles as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ground_fast():
    L = C.CDLL(os.path.join(ROOT, "tests", "libground_fast_check.so"))
    L.c2rt_ground_fast_of.argtypes = [C.c_void_p, C.POINTER(_abi.CameraFrame), C.POINTER(_abi.RenderOpts), C.c_int,
                                      C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    L.c2rt_ground_fast_of.restype = C.c_int

    def of(scene, cam, opts, debug_cull=0):
        node, n_cull = C.c_int32(-2), C.c_uint32(0)
        r = L.c2rt_ground_fast_of(C.cast(scene.desc, C.c_void_p), C.byref(cam), C.byref(opts), debug_cull, C.byref(node), C.byref(n_cull))
        assert r in (0, 1), r
        if r:  # never without a mask table and a ground node
            assert n_cull.value > 0 and node.value >= 0
        return r

    return of


def _load(tmp_path, case):
    path = tmp_path / (case["name"] + ".sdl")
    path.write_text(case["sdl"])
    scene = c2.parseSceneFromFile(str(path))
    scene.setFrameSize(case["W"], case["H"])
    kw = dict(prepass_bucket=48) if case["kind"] == "prepass" else {}
    return scene, scene.beginFrame(), scene.renderOpts(taps=case["taps"], **kw)


@pytest.mark.parametrize("case", G._cases(), ids=lambda c: c["name"])
def test_the_gpu_cases_are_as_eligible_as_their_table_says(ground_fast, tmp_path, case):
    scene, cam, opts = _load(tmp_path, case)
    assert ground_fast(scene, cam, opts) == (1 if case["eligible"] else 0)
    assert ground_fast(scene, cam, opts, debug_cull=16) == 0  # the diagnostics switch
    assert ground_fast(scene, cam, opts, debug_cull=15) == 0  # and without culling rectangles there is no table


def test_frames_the_path_is_not_built_for(ground_fast, tmp_path):
    case = G._cases()[0]
    scene, cam, opts = _load(tmp_path, case)
    assert ground_fast(scene, cam, opts) == 1
    counted = scene.renderOpts(taps=case["taps"], count_rays=1)
    assert ground_fast(scene, cam, counted) == 0          # counted frames run exact:: throughout
    stereo = _abi.CameraFrame.from_buffer_copy(cam)
    stereo.stereo_separation = 2.0
    assert ground_fast(scene, stereo, opts) == 0
    dof = _abi.CameraFrame.from_buffer_copy(cam)
    dof.dof, dof.num_samples = 1, 4
    assert ground_fast(scene, dof, opts) == 0
    # a second light: the multi-light instances carry no ground path
    two = dict(case, name="two_lights", sdl=G._lecture5(lights='  Lights {\n    PointLight {\n      name "a"\n      pos -90 700 350\n'
                                                        '      color 1 1 1\n      power 800000\n    }\n    PointLight {\n      name "b"\n'
                                                        '      pos 200 500 -50\n      color 1 1 1\n      power 300000\n    }\n  }\n\n'))
    scene2, cam2, opts2 = _load(tmp_path, two)
    assert ground_fast(scene2, cam2, opts2) == 0
