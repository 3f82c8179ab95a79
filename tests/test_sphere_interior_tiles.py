"""Sphere-interior tiles (chess2rt_amd/csrc/csg_void.h: sphere_interior_tile; scene_plan.cpp: sphere_cull_of): the mask
pre-pass claims a tile for lean::sphere_tile when every primary ray's closest hit provably lies on one Sphere node and no
other node can occlude its shadow rays towards light 0.  On the host, through the same classifier and the planner itself
(tests/libsphere_interior_check.so, scripts/sphere_interior_tiles.py): every pixel and all 5 taps of a claimed tile hit
the claimed node first in the oracle, and the shadow ray from p + N * 1e-6 is hit by no other node before the light.  A
classifier whose inner ball is too large must be caught by that check, and what the derivation does not cover gets no
claim at all."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import csg_void_tiles as cv  # noqa: E402
import sphere_interior_tiles as si  # noqa: E402
import sphere_tile_scenes as T  # noqa: E402

LECTURE5 = os.path.join(ROOT, "tests", "golden", "scenes", "lecture5.sdl")
GLOBE, BALLS = 1, (3, 4, 5)


def _load(path, W, H):
    import chess2rt_amd as c2

    scene = c2.parseSceneFromFile(path)
    scene.setFrameSize(W, H)
    return scene, scene.beginFrame(), scene.renderOpts(taps=5)


def _edited(tmp_path, name, text, W=64, H=48):
    import shutil

    for f in ("floor.bmp", "world.bmp"):
        if not (tmp_path / f).exists():
            shutil.copy(os.path.join(T.SCENES, f), str(tmp_path / f))
    path = tmp_path / (name + ".sdl")
    path.write_text(text)
    return _load(str(path), W, H)


ANY_SIZE = 256  # C2RT_DEBUG_CULL bit 8: the claim whatever the frame's size (as shipped: six million samples and more)


def _claims(scene, cam, opts, W, H, debug_cull=ANY_SIZE):
    frame = si.Frame(scene.desc, cam, opts, debug_cull)
    node, claim = frame.classify(W, H)
    return frame, node, claim


@pytest.fixture(scope="module")
def lecture5_640():
    scene, cam, opts = _load(LECTURE5, 640, 480)
    return (scene, cam) + _claims(scene, cam, opts, 640, 480)


def test_every_claimed_tile_of_lecture5_640x480_sample_by_sample(lecture5_640):
    scene, cam, frame, node, claim = lecture5_640
    assert frame.interior == sum(1 << n for n in (GLOBE,) + BALLS) and frame.n_lights == 1
    tiles = samples = 0
    for n in (GLOBE,) + BALLS:
        t, s, selfs = si.check_tiles(scene.desc, cam, 640, 480, frame, node, claim, n)
        print("node %d: %d claimed tiles, %d samples, %d shadow rays hit the sphere itself" % (n, t, s, selfs))
        assert t > 0 and s == t * 64 * 5
        tiles += t
        samples += s
    assert tiles == int(((claim & 1) != 0).sum()) >= 150


def test_a_seeded_sample_of_the_headline_frame():
    scene, cam, opts = _load(LECTURE5, 3840, 2160)
    frame, node, claim = _claims(scene, cam, opts, 3840, 2160)
    for n in (GLOBE,) + BALLS:
        mine = int((((claim & 1) != 0) & (node == n)).sum())
        t, s, selfs = si.check_tiles(scene.desc, cam, 3840, 2160, frame, node, claim, n, sample=30, seed=n)
        print("node %d: %d claimed tiles, %d sampled, %d samples, %d self-shadowed" % (n, mine, t, s, selfs))
        assert t == min(30, mine) == 30 and s == t * 320
    # the go / no-go of the change: at least 5 % of the headline frame's tiles
    claimed = int(((claim & 1) != 0).sum())
    assert claimed >= 0.05 * claim.size, claimed
    # a claimed tile's primary mask is its sphere and the ground, nothing else
    th, tw = claim.shape
    pm, _, nd, cl = frame.classify_tiles([cv.tile_bounds(r, c, 0, 2160) for r in range(th) for c in range(tw)])
    live = pm[(cl & 1) != 0] & 0x3F
    assert np.array_equal(live, (1 | (1 << nd[(cl & 1) != 0])).astype(np.uint32))


def test_an_inner_ball_that_is_too_large_is_caught(lecture5_640):
    """the mutation: the claim evaluated as if every ball had 1.05 R — tiles at the silhouette, some of whose rays miss
    the real ball, are claimed, and the oracle check must raise"""
    scene, cam, frame, node, claim = lecture5_640
    mnode, mclaim = frame.classify(640, 480, r_scale=1.05)
    assert ((mclaim & 1) != 0).sum() > ((claim & 1) != 0).sum()
    with pytest.raises(AssertionError, match="closest node"):
        for n in (GLOBE,) + BALLS:
            si.check_tiles(scene.desc, cam, 640, 480, frame, mnode, mclaim, n)


def test_what_the_derivation_does_not_cover_is_not_claimed(tmp_path, lecture5_640):
    scene, cam, frame, node, claim = lecture5_640
    X = T.texts()
    opts = scene.renderOpts(taps=5)
    # the diagnostics switch (it wins over bit 8), and the size condition: 640x480 x5 and 1080p x1 are too small to pay
    # for the test, 1080p x5 and 4K x1 are not
    assert si.Frame(scene.desc, cam, opts, debug_cull=128 | ANY_SIZE).interior == 0
    assert not _claims(scene, cam, opts, 640, 480, debug_cull=128 | ANY_SIZE)[2].any()
    assert si.Frame(scene.desc, cam, opts).interior == 0
    for (W, H, taps), want in (((1920, 1080, 1), False), ((1920, 1080, 5), True), ((3840, 2160, 1), True)):
        s, c, _ = _load(LECTURE5, W, H)
        assert (si.Frame(s.desc, c, s.renderOpts(taps=taps)).interior != 0) == want, (W, H, taps)
    # a second object in the primary mask: where the globe's tiles also keep a ball, nothing is claimed
    th, tw = claim.shape
    pm, _, _, cl = frame.classify_tiles([cv.tile_bounds(r, c, 0, 480) for r in range(th) for c in range(tw)])
    both = ((pm >> GLOBE) & 1 != 0) & ((pm & 0x3C) != 0)
    assert both.sum() > 0 and not (cl[both] & 1).any()

    def globe_claims(name, text):
        s, c, o = _edited(tmp_path, name, text)
        f, nd, cl = _claims(s, c, o, 64, 48)
        return f, int((((cl & 1) != 0) & (nd == GLOBE)).sum()), int(((cl & 2) != 0).sum())

    # the baseline of the refusals below: the globe fills the frame and every tile is claimed
    f, n, _ = globe_claims("globe", X["globe"])
    assert (f.interior >> GLOBE) & 1 and n == 48
    # the eye inside R + m
    assert globe_claims("eye_inside", X["globe"].replace("pos    100 50 255", "pos    100 50 300"))[1] == 0
    # the ball dipping under the ground
    assert "center  100 50 320" in X["globe"]
    assert globe_claims("dipping", X["globe"].replace("center  100 50 320", "center  100 49 320"))[1] == 0
    # an occluder whose bounding ball meets the shadow cone: the three balls under the globe
    f, n, primary_ok = globe_claims("balls_under", X["globe_balls_under"])
    assert primary_ok == 48 and 0 < n < 48
    # a light below the patch's height (other nodes are left in the shadow mask)
    assert globe_claims("low_light", X["globe"].replace(T.LIGHT, "pos    -90 20 350"))[1] == 0
    # a checker sphere
    checker = X["globe"].replace(T.GLOBE_TEXTURE, 'Checker {\n      name  "world"\n      color1  0.9 0.1 0.2\n      color2  0.1 0.8 0.9\n      size  0.1\n    }')
    f, n, _ = globe_claims("checker", checker)
    assert not (f.interior >> GLOBE) & 1 and n == 0 and f.interior != 0
    # a rotated node
    s, c, o = _edited(tmp_path, "rotated", X["globe"])
    s.rotateNode("globe", 10.0, 20.0, 30.0)
    f = si.Frame(s.desc, c, o, ANY_SIZE)
    assert not (f.interior >> GLOBE) & 1 and not ((f.classify(64, 48)[1] & 1) != 0).any()


def test_no_light_and_self_shadow_scenes_are_what_their_names_say(tmp_path):
    """the two device cases whose point is a branch of the path: without a light and a floor the planner has no ground node
    and no light, and every tile is claimed with no shadow condition; with the light behind the ball every sample of every
    tile is self-shadowed (the oracle's shadow ray hits the ball itself)"""
    X = T.texts()
    s, c, o = _edited(tmp_path, "no_light", X["no_light"])
    f, nd, cl = _claims(s, c, o, 64, 48)
    assert f.n_lights == 0 and f.ground_node == -1 and int(((cl & 1) != 0).sum()) == 48 and np.array_equal(cl & 1, (cl >> 1) & 1)
    t, samples, selfs = si.check_tiles(s.desc, c, 64, 48, f, nd, cl, 0)  # (without the floor the globe is node 0)
    assert t == 48 and samples == 48 * 320 and selfs == 0
    s, c, o = _edited(tmp_path, "self_shadowed", X["ball_self_shadowed"])
    f, nd, cl = _claims(s, c, o, 64, 48)
    t, samples, selfs = si.check_tiles(s.desc, c, 64, 48, f, nd, cl, 4)  # (S3; the scenes have no CsgDiff node)
    assert t == 48 and samples == selfs == 48 * 320
    s, c, o = _edited(tmp_path, "lit", X["ball"])
    f, nd, cl = _claims(s, c, o, 64, 48)
    t, samples, selfs = si.check_tiles(s.desc, c, 64, 48, f, nd, cl, 4)  # (S3; the scenes have no CsgDiff node)
    assert t == 48 and selfs < samples // 4  # most of the cap is lit: the two cases differ, and the lit branch runs
