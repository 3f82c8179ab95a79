"""The mask pre-pass drops a CsgDiff(L, Sphere) node from tiles whose rays provably miss it
(chess2rt_amd/csrc/csg_void.h).  On the host, through the same classifier (tests/libcsg_void_check.so): every
primary ray (5 taps) of a tile called void, and every ground shadow ray towards light 0 of a tile called
shadow-void, gets no hit on the node in the oracle — lecture5 at three sizes, fuzzed Diff(cube | sphere, sphere)
scenes under random cameras, and adversarial set-ups where the test must refuse or be right."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import csg_void_tiles as cv  # noqa: E402

LECTURE5 = os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl")


def _load(path, W, H):
    import chess2rt_amd as c2

    scene = c2.parseSceneFromFile(path)
    scene.setFrameSize(W, H)
    return scene, scene.beginFrame()


def _check_all(scene, cam, W, H, sample=0, seed=0):
    """classify every candidate node, oracle-check the void tiles (all, or `sample` of them); -> void tile count"""
    desc = scene.desc
    gn, _ = cv.ground_of(desc)
    D = cv._fields(desc)
    light = [D.light_pos[i] for i in range(3)] if D.n_lights else [0.0, 0.0, 0.0]
    total = 0
    for cand in cv.void_candidates(desc):
        cls = cv.classify(desc, cam, W, H, cand)
        tiles = list(zip(*np.nonzero(cls)))
        total += len(tiles)
        if sample and len(tiles) > sample:
            rng = np.random.default_rng(seed)
            tiles = [tiles[i] for i in rng.choice(len(tiles), size=sample, replace=False)]
        for ty, tx in tiles:
            cv.check_tile(desc, cam, W, H, cand[0], int(ty), int(tx), int(cls[ty, tx]), light, gn)
    return total


@pytest.mark.parametrize("W,H,sample", [(640, 480, 0), (1920, 1080, 300), (3840, 2160, 200)])
def test_lecture5_void_tiles_miss_the_csg(W, H, sample):
    scene, cam = _load(LECTURE5, W, H)
    n = _check_all(scene, cam, W, H, sample=sample, seed=W)
    assert n > 0.1 * (W // 8) * (H // 8) * 0.2  # a real share of the CsgDiff's tiles


def test_lecture5_headline_share():
    """go / no-go figure of the change: well over 15 % of the tiles the node's rectangle keeps come out void"""
    scene, cam = _load(LECTURE5, 3840, 2160)
    (cand,) = cv.void_candidates(scene.desc)
    cls = cv.classify(scene.desc, cam, 3840, 2160, cand)
    keep = cv.node_rect_tiles(cam, 3840, 2160, cand[1], cand[2])
    assert ((cls & 1) != 0)[keep].mean() > 0.3


CAMERA = "Camera {{ pos {pos}; yaw {yaw:.6g}; pitch {pitch:.6g}; roll {roll:.6g}; fov {fov:.6g} }}"


def _diff_scene(r, left_kind, c, half, R, cam, light, off=(0, 0, 0)):
    left = ('Cube "L" {{ center {0} {1} {2}; side {3:.9g} }}' if left_kind == "Cube" else
            'Sphere "L" {{ center {0} {1} {2}; R {3:.9g} }}').format(c[0], c[1], c[2], 2 * half if left_kind == "Cube" else half)
    return """Scene {{
  GlobalSettings {{ frameWidth 64; frameHeight 48; ambientLightColor 0.2 0.2 0.2; AAEnabled true }}
  {cam}
  Lights {{
    PointLight "l" {{ pos {lx:.9g} {ly:.9g} {lz:.9g}; color 1 1 1; power 800000 }}
  }}
  Geometries {{
    Plane "floor" {{ y -0.01 }}
    {left}
    Sphere "S" {{ center {c0} {c1} {c2}; R {R:.17g} }}
    CsgDiff "D" {{ left "L"; right "S" }}
  }}
  Shaders {{
    Lambert "sh" {{ color 0.5 0.5 0.5 }}
  }}
  Nodes {{
    Node "floor" {{ geometry "floor"; shader "sh" }}
    Node "d" {{ geometry "D"; shader "sh"; translate {o0} {o1} {o2} }}
  }}
}}
""".format(cam=cam, lx=light[0], ly=light[1], lz=light[2], left=left, c0=c[0], c1=c[1], c2=c[2], R=R,
           o0=off[0], o1=off[1], o2=off[2])


def _cam(pos, yaw, pitch, roll=0.0, fov=90.0):
    return CAMERA.format(pos=" ".join("%.9g" % v for v in pos), yaw=yaw, pitch=pitch, roll=roll, fov=fov)


def _run(tmp_path, sdl, name, W=64, H=48):
    p = tmp_path / (name + ".sdl")
    p.write_text(sdl)
    scene, cam = _load(str(p), W, H)
    return _check_all(scene, cam, W, H)


@pytest.mark.parametrize("seed", range(24))
def test_fuzzed_diff_scenes(tmp_path, seed):
    r = random.Random(1000 + seed)
    kind = r.choice(["Cube", "Sphere"])
    c = (r.uniform(-60, 60), r.uniform(20, 80), r.uniform(80, 260))
    half = r.uniform(10, 60)
    # the subtracted sphere: from barely touching the left child to swallowing it
    R = half * (r.uniform(1.0, 1.8) if kind == "Cube" else r.uniform(0.6, 1.6))
    target = (c[0] + r.uniform(-30, 30), c[1] + r.uniform(-30, 30), c[2] + r.uniform(-30, 30))
    pos = (r.uniform(-200, 200), r.uniform(5, 300), r.uniform(-150, 80))
    d = [target[i] - pos[i] for i in range(3)]
    import math

    yaw = math.degrees(math.atan2(d[0], d[2])) + r.uniform(-15, 15)
    pitch = math.degrees(math.atan2(d[1], math.hypot(d[0], d[2]))) + r.uniform(-10, 10)
    light = (r.uniform(-300, 300), r.uniform(150, 800), r.uniform(-100, 500))
    off = (r.uniform(-20, 20), r.uniform(0, 20), r.uniform(-20, 20)) if r.random() < 0.5 else (0, 0, 0)
    sdl = _diff_scene(r, kind, c, half, R, _cam(pos, yaw, pitch, r.uniform(-20, 20), r.uniform(30, 100)), light, off)
    _run(tmp_path, sdl, "fuzz%d" % seed, 320, 240)


def _lecture5_like(R, pos, yaw=0.0, pitch=-30.0, light=(-90, 700, 350)):
    return _diff_scene(None, "Cube", (-100, 60, 200), 50, R, _cam(pos, yaw, pitch), light)


def test_sphere_just_large_enough(tmp_path):
    # half-diagonal of the cube face: 50 * sqrt(2) ~ 70.71 — edges poke out below it, vanish above it
    for R in (70.7106, 70.7107, 70.71068, 86.6025, 86.6026, 90.0):
        _run(tmp_path, _lecture5_like(R, (0, 165, 0)), "big%g" % R, 160, 120)


def test_tangent_rays(tmp_path):
    # the sphere tangent to the cube's faces (R = half side) and the eye level with the top face
    for R, pos in ((50.0, (0, 110, 0)), (50.0, (-100, 110, 0)), (50.000001, (-100, 60, 0)), (70.0, (-100, 110, -40))):
        _run(tmp_path, _lecture5_like(R, pos, pitch=0.0 if pos[1] == 110 else -10.0), "tan%g_%g" % (R, pos[0]), 160, 120)


def test_eye_inside_sphere_and_box(tmp_path):
    # inside the sphere but outside the box, inside both, inside the box near a corner (outside the sphere)
    for pos, yaw, pitch in (((-100, 60, 135), 0.0, 0.0), ((-100, 60, 200), 30.0, -20.0), ((-140, 100, 160), 45.0, 10.0)):
        _run(tmp_path, _lecture5_like(70.0, pos, yaw, pitch), "in%g_%g" % (pos[0], pos[2]), 160, 120)


def test_light_inside_box_refuses_shadow(tmp_path):
    sdl = _lecture5_like(70.0, (0, 165, 0), light=(-100, 60, 200))
    _run(tmp_path, sdl, "light_in", 160, 120)


@pytest.mark.gpu
def test_gpu_frames_with_void_tiles_match_oracle(gpu_ctx):
    """lecture5 at 1920x1080, 5 taps, where the pre-pass drops the CsgDiff from thousands of tiles: bit-equal to
    the oracle (uncounted frame: the production instance, which reads the masks)."""
    import oracle_lib

    scene, cam = _load(LECTURE5, 1920, 1080)
    (cand,) = cv.void_candidates(scene.desc)
    assert int(((cv.classify(scene.desc, cam, 1920, 1080, cand) & 1) != 0).sum()) > 1000
    opts = scene.renderOpts()
    gpu_ctx.uploadScene(scene.desc)
    gpu = gpu_ctx.renderFrame(cam, opts)
    ref = oracle_lib.render_frame(scene.desc, cam, opts)
    assert gpu.shape == ref.shape and np.array_equal(gpu, ref)
