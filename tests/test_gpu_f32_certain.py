"""The certain-float routes of a frame (chess2rt_amd/csrc/f32_certain.h: sphere u,v for bitmap textures, the Phong
lobe) on the GPU.

Function level: tests/certain_f32_check (built by make from tests/certain_f32_check.hip) holds the two out-of-line
wrappers to the routines they stand in for, on the device, float for float.

Frame level: frames at the smallest sizes that still hold the cases, compared with the oracle as
tests/test_gpu_parity.py compares (parity_util: TOL per channel, one-sided NaN / inf fail); each case prints how many
floats differ at all.  The scenes are lecture5.sdl with one thing changed."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import chess2rt_amd as c2
import oracle_lib as orc
from chess2rt_amd import _abi
from golden_configs import SCENES
from parity_util import TOL, maxdiff

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LECTURE5 = open(os.path.join(SCENES, "lecture5.sdl")).read()
GLOBE_TEXTURE = 'BitmapTexture {\n      name  "world"\n      file  "world.bmp"\n    }'
assert GLOBE_TEXTURE in LECTURE5 and "exponent  60" in LECTURE5 and "exponent  80" in LECTURE5


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_wrappers_equal_the_routines_they_stand_in_for_on_the_device():
    """2^26 operands per routine, structured and random: c2_sphere_uv_bitmap + the bitmap pipeline == c2_sphere_uv + the
    same pipeline, c2_pow_f32 == (float)pow, float for float; at most 1e-4 of the random lanes take the fallback (CPU
    simulation: 2.5e-7 to 8e-7); every operand constructed onto a float midpoint or a floor jump takes it."""
    out = subprocess.run([os.path.join(HERE, "certain_f32_check"), "26"], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["operands_per_routine"] >= 1 << 26
    for k in ("uv_mismatches", "pow_mismatches", "pow_route_accepted", "constructed_uv_accepted", "constructed_uv_not_exact_doubles",
              "constructed_uv_mismatches", "constructed_pow_accepted", "constructed_pow_mismatches"):
        assert rep[k] == 0, (k, rep)
    assert rep["uv_random"] >= 1 << 25 and rep["uv_random_fallback"] <= 1e-4 * rep["uv_random"]
    assert rep["pow_random"] >= 1 << 25 and rep["pow_random_fallback"] <= 1e-4 * rep["pow_random"]
    assert rep["constructed_uv"] > 1000 and rep["constructed_pow"] > 1000   # the constructions did land on ambiguities


def load(tmp_path, text, size, name="s.sdl"):
    for f in ("floor.bmp", "world.bmp"):
        if not (tmp_path / f).exists():
            shutil.copy(os.path.join(SCENES, f), tmp_path / f)
    (tmp_path / name).write_text(text)
    scene = c2.parseSceneFromFile(str(tmp_path / name))
    scene.setFrameSize(*size)
    return scene


def check_frame(ctx, scene, what, taps=_abi.TAPS_REF5):
    """the frame of the scene's camera against the oracle, by test_gpu_parity's rule; counted and production instances
    (the fixture renders both and insists on equal bits)"""
    cam = scene.beginFrame()
    opts = scene.renderOpts(taps=taps, count_rays=1)
    ctx.uploadScene(scene.desc)
    gpu = ctx.renderFrame(cam, opts)
    rays = ctx.rayStats()
    st = {}
    ref = orc.render_frame(scene.desc, cam, opts, 0, st)
    md, nbad, nne = maxdiff(gpu, ref)
    print("%s: max|d|=%.3g, >TOL: %d, !=: %d of %d floats" % (what, md, nbad, nne, gpu.size))
    assert gpu.shape == ref.shape and md <= TOL and nbad == 0, (what, md, nbad)
    assert rays == (st["primary"], st["shadow"]), what
    return cam, gpu, ref


def test_lecture5_full_strips_and_batch(gpu_ctx, tmp_path):
    scene = load(tmp_path, LECTURE5, (160, 120))
    cam, full, _ = check_frame(gpu_ctx, scene, "lecture5 160x120 x5")
    # two-rank strips: every rank's rows are the full frame's
    H = 120
    for rank in range(2):
        o = scene.renderOpts(taps=_abi.TAPS_REF5, strip_height=8, strip_rank=rank, strip_world=2)
        rows = [y for y in range(H) if (y // 8) % 2 == rank]
        assert np.array_equal(bits(gpu_ctx.renderFrame(cam, o)), bits(full[rows])), rank
    # a two-camera batch: each frame against the oracle and against the single frame
    scene.rotateCamera(9.0, 0, 0)
    cam2 = scene.beginFrame()
    opts = scene.renderOpts(taps=_abi.TAPS_REF5)
    batch = gpu_ctx.renderFrames([cam, cam2], opts)
    for i, c in enumerate((cam, cam2)):
        ref = orc.render_frame(scene.desc, c, opts, 0, {})
        md, nbad, nne = maxdiff(batch[i], ref)
        print("batch frame %d: max|d|=%.3g, !=: %d" % (i, md, nne))
        assert md <= TOL and nbad == 0
        assert np.array_equal(bits(batch[i]), bits(gpu_ctx.renderFrame(c, opts)))


def test_globe_fills_the_frame(gpu_ctx, tmp_path):
    """camera 65 from the centre of the R = 50 globe at fov 90: every sample's closest hit is the textured sphere"""
    text = LECTURE5.replace("pos    0 165 0", "pos    100 50 255").replace("pitch  -30", "pitch  0")
    scene = load(tmp_path, text, (64, 48))
    _, gpu, ref = check_frame(gpu_ctx, scene, "globe fills 64x48 x5")
    assert len(np.unique(bits(gpu).reshape(-1, 3), axis=0)) > 1000   # texels, not one colour


@pytest.mark.parametrize("scaling", [4, 0.005])
def test_bitmap_sphere_with_scaling(gpu_ctx, tmp_path, scaling):
    text = LECTURE5.replace(GLOBE_TEXTURE, GLOBE_TEXTURE[:-1] + "  scaling %r\n    }" % scaling)
    assert text != LECTURE5
    check_frame(gpu_ctx, load(tmp_path, text, (96, 72)), "globe scaling %r" % scaling)


@pytest.mark.parametrize("texture", ['Checker "world" { color1 0.9 0.1 0.2; color2 0.15 0.8 0.95; size 0.05 }',
                                     'Procedure2 "world" { freqU 7 11 3; freqV 5 2 13; colorU { color 0.2 0.1 0.3; color 0.1 0.3 0.2; color 0.3 0.2 0.1 }; '
                                     'colorV { color 0.1 0.2 0.1; color 0.2 0.1 0.2; color 0.1 0.1 0.3 } }'])
def test_checker_and_procedure2_spheres_take_the_exact_doubles(gpu_ctx, tmp_path, texture):
    """their readers use u, v as doubles (a floor of u / size, a sine of u * freq): nothing may change for them"""
    text = LECTURE5.replace(GLOBE_TEXTURE, texture)
    assert text != LECTURE5
    check_frame(gpu_ctx, load(tmp_path, text, (96, 72)), texture.split()[0] + " sphere")


@pytest.mark.parametrize("exponent", [1, 2, 60, 1024, 1025, 2.5, 0])
def test_phong_exponents_on_both_routes(gpu_ctx, tmp_path, exponent):
    """1, 2, 60, 1024: the integer route; 1025, 2.5, 0: pow"""
    text = LECTURE5.replace("exponent  60", "exponent  %r" % exponent).replace("exponent  80", "exponent  %r" % exponent)
    check_frame(gpu_ctx, load(tmp_path, text, (96, 72)), "Phong exponent %r" % exponent)


def test_several_lights(gpu_ctx, tmp_path):
    """the light-loop instance: shade()'s second call site"""
    second = '    PointLight {\n      name  "light2"\n      pos    200 300 -50\n      color  1 0.8 0.6\n      power  300000\n    }\n  }\n\n  Geometries {'
    text = LECTURE5.replace("  }\n\n  Geometries {", second, 1)
    assert text != LECTURE5
    scene = load(tmp_path, text, (96, 72))
    assert scene.desc.contents.n_lights == 2
    check_frame(gpu_ctx, scene, "two lights")


def test_adaptive_frame(gpu_ctx, tmp_path):
    """the refinement kernel shades through the exact u,v (trace_closest), the frames through the certain-float route:
    a flagged pixel is the five-tap frame's, an unflagged one the one-tap frame's, bit for bit — and both frames are the
    oracle's by the parity rule"""
    scene = load(tmp_path, LECTURE5, (160, 120))
    cam, five, _ = check_frame(gpu_ctx, scene, "lecture5 160x120 x5")
    _, one, _ = check_frame(gpu_ctx, scene, "lecture5 160x120 x1", taps=_abi.TAPS_1)
    frame, mask = gpu_ctx.renderFrameAdaptive(cam, scene.renderOpts(taps=_abi.TAPS_REF5))
    flagged = mask != 0
    assert 0 < flagged.sum() < flagged.size
    assert np.array_equal(bits(frame)[flagged], bits(five)[flagged])
    assert np.array_equal(bits(frame)[~flagged], bits(one)[~flagged])
