"""Dark ground tiles (chess2rt_amd/csrc/csg_void.h: tile_dark_by; scene_plan.cpp: plan_dark_nodes, dark_cull_of): the
mask pre-pass calls a primary-ground tile dark when one node provably occludes every shadow ray from its footprint
towards light 0.  On the host, through the same classifier and the planner itself (tests/libground_dark_check.so,
scripts/ground_dark_tiles.py): every pixel and all 5 taps of a dark tile hit the ground first, and the shadow ray from
p + N * 1e-6 gets a hit on the claimed node before the light, in the oracle.  A classifier whose convex set is too
large must be caught by that check, and frames the derivation does not cover get no dark tile at all."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import ground_dark_tiles as gd  # noqa: E402
import test_gpu_ground_tiles as G  # noqa: E402  (lecture5 with edited lines; importing it runs nothing)

LECTURE5 = os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl")


def _load(path, W, H):
    import chess2rt_amd as c2

    scene = c2.parseSceneFromFile(path)
    scene.setFrameSize(W, H)
    return scene, scene.beginFrame(), scene.renderOpts(taps=5)


def _edited(tmp_path, name, W=640, H=480, **edits):
    path = tmp_path / (name + ".sdl")
    path.write_text(G._lecture5(**edits))
    return _load(str(path), W, H)


@pytest.fixture(scope="module")
def lecture5_640():
    scene, cam, opts = _load(LECTURE5, 640, 480)
    frame, per_node = gd.dark_tiles(scene.desc, cam, opts, 640, 480)
    return scene, cam, frame, per_node


def test_every_dark_tile_of_lecture5_640x480_ray_by_ray(lecture5_640):
    scene, cam, frame, per_node = lecture5_640
    total = rays = 0
    kinds = set()
    for k, tiles in per_node:
        n, r = gd.check_tiles(scene.desc, cam, 640, 480, frame, k.node, tiles)
        print("node %d kind %d: %d dark tiles, %d shadow rays occluded" % (k.node, k.kind, n, r))
        total += n
        rays += r
        if n:
            kinds.add(k.kind)
    assert total > 0 and rays == total * 64 * 5
    assert kinds == {gd.KIND_SPHERE, gd.KIND_CSG_DIFF}  # both proofs are exercised


def test_a_seeded_sample_of_the_headline_frame():
    scene, cam, opts = _load(LECTURE5, 3840, 2160)
    frame, per_node = gd.dark_tiles(scene.desc, cam, opts, 3840, 2160)
    assert frame.d.n == len(per_node) >= 2
    union = np.zeros((270, 480), dtype=bool)
    for k, tiles in per_node:
        n, r = gd.check_tiles(scene.desc, cam, 3840, 2160, frame, k.node, tiles, sample=30, seed=k.node)
        print("node %d kind %d: %d dark tiles, %d sampled, %d shadow rays occluded" % (k.node, k.kind, int(tiles.sum()), n, r))
        assert n == min(30, int(tiles.sum())) and r == n * 320
        union |= tiles
    # the go / no-go of the change: at least 3 % of the headline frame's tiles
    assert union.sum() >= 0.03 * union.size, int(union.sum())


def test_a_convex_set_that_reaches_into_the_ball_is_caught(lecture5_640):
    """the mutation: the CsgDiff's cuts placed as for a ball of 0.6 R — the set then holds points inside the real
    ball, tiles whose shadow rays pass through the hollow are called dark, and the oracle check must raise"""
    scene, cam, _, _ = lecture5_640
    opts = scene.renderOpts(taps=5)
    frame, per_node = gd.dark_tiles(scene.desc, cam, opts, 640, 480,
                                    mutate=lambda k: gd.with_radius(k, 0.6) if k.kind == gd.KIND_CSG_DIFF else k)
    mutated = [(k, t) for k, t in per_node if k.kind == gd.KIND_CSG_DIFF]
    assert mutated and all(t.any() for _, t in mutated)
    with pytest.raises(AssertionError, match="not occluded"):
        for k, tiles in mutated:
            gd.check_tiles(scene.desc, cam, 640, 480, frame, k.node, tiles)


def test_frames_the_derivation_does_not_cover_have_no_dark_tile(tmp_path, lecture5_640):
    scene, cam, frame, _ = lecture5_640
    assert frame.d.n >= 2
    # the diagnostics switch
    assert gd.dark_frame(scene.desc, cam, scene.renderOpts(taps=5), debug_cull=32).d.n == 0
    # a camera below the floor: eye and light on opposite sides of the ground
    s, c, o = _edited(tmp_path, "camera_under_floor", cam_pos="0 -165 0", pitch="30")
    assert gd.dark_frame(s.desc, c, o).d.n == 0 and gd.dark_tiles(s.desc, c, o, 640, 480)[1] == []
    # a light below the box's top (and below the globe's): neither set lies under the light's height
    s, c, o = _edited(tmp_path, "low_light", light_pos="-90 90 350")
    nodes = [k.node for k, _ in gd.dark_tiles(s.desc, c, o, 640, 480)[1]]
    assert 1 not in nodes and 2 not in nodes, nodes
    # an unlit light
    s, c, o = _edited(tmp_path, "power_0", power="0")
    assert gd.dark_frame(s.desc, c, o).d.n == 0
    # an eye beyond the distance the margins were derived for
    far = type(cam).from_buffer_copy(cam)
    far.pos[1] = 2 * frame.d.eye_max
    assert gd.dark_frame(scene.desc, far, scene.renderOpts(taps=5)).d.n == 0
