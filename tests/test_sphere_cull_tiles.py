"""The mask pre-pass drops a Sphere node from tiles whose rays provably pass it by (chess2rt_amd/csrc/csg_void.h:
cone_misses_ball).  On the host, through the same classifier (tests/libsphere_cull_check.so): every primary ray
(64 pixels x 5 taps) of a tile the classifier drops the node from, and every ground shadow ray towards light 0 of a
tile that loses the node from its shadow mask, gets no hit on the node in the oracle — lecture5 at three sizes, fuzzed
scenes of spheres under random cameras and lights, and adversarial set-ups where the test must refuse or be right.

A tile counts as dropped where the test's answer is used: the node's screen rectangle keeps it (primary), resp. the
tile's ground footprint meets the node's shadow rectangle (shadow); elsewhere the rectangles have dropped it already."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import csg_void_tiles as cv  # noqa: E402
import sphere_cull_scenes as S  # noqa: E402
import sphere_cull_tiles as sc  # noqa: E402


def _load(path, W, H):
    import chess2rt_amd as c2

    scene = c2.parseSceneFromFile(path)
    scene.setFrameSize(W, H)
    return scene, scene.beginFrame()


def _shadow_tiles(desc, cam, W, H, ball):
    """bool (tiles_y, tiles_x): tiles whose ground footprint (corner rays, +1 px) may meet the shadow of the ball's
    box from light 0 — generously: the x,z rectangle of the projected box grown by a tenth; all tiles when in doubt"""
    D = cv._fields(desc)
    tw, th = (W + 7) // 8, (H + 7) // 8
    every = np.ones((th, tw), dtype=bool)
    _, gy = cv.ground_of(desc)
    if gy is None or not D.n_lights:
        return every
    L = np.array([D.light_pos[i] for i in range(3)])
    xs, zs = [], []
    for k in range(8):
        w = np.array([ball.c[i] + (ball.R if k >> i & 1 else -ball.R) for i in range(3)])
        w[1] = max(w[1], gy) if L[1] > gy else min(w[1], gy)
        den = L[1] - w[1]
        if not abs(den) > 1e-9 * (abs(L[1]) + 1) or (L[1] - gy) / den <= 0:
            return every
        f = (L[1] - gy) / den
        xs.append(L[0] + (w[0] - L[0]) * f)
        zs.append(L[2] + (w[2] - L[2]) * f)
    gx, gz = 0.1 * (max(xs) - min(xs)) + 1, 0.1 * (max(zs) - min(zs)) + 1
    x0, x1, z0, z1 = min(xs) - gx, max(xs) + gx, min(zs) - gz, max(zs) + gz
    pos, ul = np.array(cam.pos), np.array(cam.up_left)
    du, dv = np.array(cam.up_right) - ul, np.array(cam.down_left) - ul
    px = np.arange(tw + 1) * 8.0
    py = np.minimum(np.arange(th + 1) * 8.0, H)
    X, Y = np.meshgrid(px, py)
    d = ul[None, None, :] + du * (X / cam.frame_width)[..., None] + dv * (Y / cam.frame_height)[..., None] - pos
    with np.errstate(all="ignore"):
        t = (gy - pos[1]) / d[..., 1]
        hx, hz = pos[0] + d[..., 0] * t, pos[2] + d[..., 2] * t
    bad = ~(t > 0) | ~np.isfinite(hx) | ~np.isfinite(hz)

    def corners(a):
        return np.stack([a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:]])

    cb = corners(bad).any(axis=0)
    cx, cz = corners(hx), corners(hz)
    slack = 0.5 * (cx.max(axis=0) - cx.min(axis=0)) + 0.5 * (cz.max(axis=0) - cz.min(axis=0))  # the +1 px and more
    meets = (cx.max(axis=0) + slack >= x0) & (cx.min(axis=0) - slack <= x1) & (cz.max(axis=0) + slack >= z0) & (cz.min(axis=0) - slack <= z1)
    return meets | cb


def _check_all(scene, cam, W, H, sample=0, seed=0):
    """classify every sphere entry of the frame, oracle-check the dropped tiles (all, or `sample` per node and kind);
    -> (primary drops, shadow drops)"""
    desc = scene.desc
    gn, _ = cv.ground_of(desc)
    D = cv._fields(desc)
    light = [D.light_pos[i] for i in range(3)] if D.n_lights else [0.0, 0.0, 0.0]
    reach, entries = sc.frame_sphere_cull(desc, cam)
    balls = {b.node: b for b in sc.sphere_candidates(desc)}
    totals = [0, 0]
    for e in entries:
        b = balls[e["node"]]
        cls = sc.classify(desc, cam, W, H, e, reach)
        keep = cv.node_rect_tiles(cam, W, H, [b.c[i] - b.R for i in range(3)], [b.c[i] + b.R for i in range(3)])
        used = (((cls & 1) != 0) & keep, ((cls & 2) != 0) & _shadow_tiles(desc, cam, W, H, b))
        for kind, grid in enumerate(used):
            tiles = list(zip(*np.nonzero(grid)))
            totals[kind] += len(tiles)
            if sample and len(tiles) > sample:
                rng = np.random.default_rng(seed + 17 * e["node"] + kind)
                tiles = [tiles[i] for i in rng.choice(len(tiles), size=sample, replace=False)]
            for ty, tx in tiles:
                cv.check_tile(desc, cam, W, H, e["node"], int(ty), int(tx), 1 << kind, light, gn)
    return tuple(totals)


@pytest.mark.parametrize("W,H,sample", [(640, 480, 0), (1920, 1080, 200), (3840, 2160, 200)])
def test_lecture5_dropped_tiles_miss_the_spheres(W, H, sample):
    scene, cam = _load(S.LECTURE5, W, H)
    assert [b.node for b in sc.sphere_candidates(scene.desc)] == [1, 3, 4, 5]
    reach, entries = sc.frame_sphere_cull(scene.desc, cam)
    assert [e["flags"] for e in entries] == [3, 3, 3, 3]
    prim, shad = _check_all(scene, cam, W, H, sample=sample, seed=W)
    print("lecture5 %dx%d: %d primary drops, %d shadow drops checked against" % (W, H, prim, shad))
    assert prim > 0.03 * ((W + 7) // 8) * ((H + 7) // 8) and shad > 0


def test_lecture5_headline_share():
    """The cull works at 4K: profiles/r06_variants.md records 55.1 / 57.6 / 59.7 / 61.8 % of the rectangle tiles of
    nodes 1 / 3 / 4 / 5 dropped by the cone test, and 7.85 % of the frame's tiles left without an object rectangle"""
    scene, cam = _load(S.LECTURE5, 3840, 2160)
    rows, before, after, total = sc.table(scene.desc, cam, 3840, 2160)
    assert [r[0] for r in rows] == [1, 3, 4, 5]
    for node, keep, dropped, alone, shadow in rows:
        assert dropped > 0.45 * keep, (node, keep, dropped)
    assert before - after > 0.06 * total


def _run(tmp_path, sdl, name, W, H, sample=0):
    p = tmp_path / (name + ".sdl")
    p.write_text(sdl)
    scene, cam = _load(str(p), W, H)
    return scene, cam, _check_all(scene, cam, W, H, sample=sample)


def test_fuzzed_sphere_scenes(tmp_path):
    prim = shad = 0
    for seed in range(24):
        _, _, (p, s) = _run(tmp_path, S.fuzz_scene(seed), "fuzz%d" % seed, 160, 120, sample=40)
        prim += p
        shad += s
    print("fuzz: %d primary drops, %d shadow drops" % (prim, shad))
    assert prim >= 200 and shad >= 20


def test_adversarial_scenes(tmp_path):
    got = {}
    for name, sdl in S.adversarial():
        scene, cam, counts = _run(tmp_path, sdl, name, 160, 120)
        reach, entries = sc.frame_sphere_cull(scene.desc, cam)
        got[name] = (counts, {e["node"]: e for e in entries}, scene, cam, reach)
    # the eye inside the ball or its padding: refused everywhere; just outside: the test may answer (and was checked)
    for name in ("eye_inside", "eye_in_pad"):
        counts, entries, scene, cam, reach = got[name]
        assert not np.any(sc.classify(scene.desc, cam, 160, 120, entries[1], reach) & 1), name
    # the ball behind the eye is dropped from every tile it is asked about, the one in front from some
    counts, entries, scene, cam, reach = got["behind"]
    assert np.all(sc.classify(scene.desc, cam, 160, 120, entries[1], reach) & 1)
    assert 0 < int((sc.classify(scene.desc, cam, 160, 120, entries[2], reach) & 1).sum()) < 300
    # the light below a ball's top: no shadow test for that ball, the low ball keeps it
    counts, entries, scene, cam, reach = got["light_low"]
    assert entries[1]["flags"] == 1 and entries[2]["flags"] == 3
    assert got["light_level"][1][1]["flags"] == 1
    # the straddling ball keeps its flags (the ground does not matter to the argument) and both kinds of drops occur
    assert got["straddle"][1][1]["flags"] == 3 and got["straddle"][0][0] > 0 and got["straddle"][0][1] > 0
    # at 1e6 the margin (scale^2 / R) swallows the scene: the test is right by refusing nearly everything
    counts, entries, scene, cam, reach = got["far1e6"]
    assert entries[1]["rp"] - 50.0 > 100.0
    assert got["translated"][1][1]["c"] == [-40.0, 50.0, 220.0] and got["translated"][0][0] > 0
    # a frame of nearly 180 degrees: its tiles' pyramids are narrow, the test answers (the balls are a few pixels wide)
    counts, entries, scene, cam, reach = got["fov179"]
    assert np.any(sc.classify(scene.desc, cam, 160, 120, entries[1], reach) & 1)


def _misses(apex, dirs, c, rp):
    tan_t, ok = C.c_double(), C.c_int()
    flat = (C.c_double * 12)(*[float(x) for d in dirs for x in d])
    r = sc.lib().c2rt_cone_misses_ball(cv._a3(apex), flat, cv._a3(c), rp, C.byref(tan_t), C.byref(ok))
    return bool(r), tan_t.value, bool(ok.value)


def _min_distance(apex, dirs, c, rng, n=4000):
    """the least distance from c to sampled rays of the pyramid (edges and rim included)"""
    w = rng.random((n, 4))
    w[: n // 4, 2:] = 0  # faces between edges 0 and 1
    w[n // 4: n // 2, :2] = 0
    w[-8:] = np.repeat(np.eye(4), 2, axis=0)
    d = w @ np.asarray(dirs, dtype=float)
    d /= np.linalg.norm(d, axis=1)[:, None]
    v = np.asarray(c, dtype=float) - np.asarray(apex, dtype=float)
    t = np.maximum(d @ v, 0.0)
    return float(np.linalg.norm(v[None, :] - d * t[:, None], axis=1).min())


def test_cone_misses_ball_against_sampled_rays():
    """random pyramids and balls: a claimed miss holds for every sampled ray; a ball tangent to a corner ray is kept
    just inside the tangent distance and dropped a little outside it"""
    rng = np.random.default_rng(5)
    claimed = 0
    for _ in range(400):
        apex = rng.uniform(-100, 100, 3)
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        a = np.cross(axis, rng.normal(size=3))
        a /= np.linalg.norm(a)
        b = np.cross(axis, a)
        h, k = rng.uniform(0.002, 0.6), rng.uniform(0.002, 0.6)
        dirs = [axis - h * a - k * b, axis + h * a - k * b, axis + h * a + k * b, axis - h * a + k * b]
        c = apex + rng.normal(size=3) * rng.uniform(1, 300)
        rp = rng.uniform(0.1, 80)
        miss, tan_t, ok = _misses(apex, dirs, c, rp)
        assert ok
        if miss:
            claimed += 1
            assert _min_distance(apex, dirs, c, rng) > rp
    assert claimed > 100
    # tangent to corner ray 2 of a square pyramid along +z: the ball's centre off that ray by rp * (1 -/+ eps)
    apex, h = np.zeros(3), 0.01
    dirs = [[-h, -h, 1], [h, -h, 1], [h, h, 1], [-h, h, 1]]
    e = np.array(dirs[2]) / np.linalg.norm(dirs[2])
    out = np.array([1, 1, -2 * h])  # perpendicular to the corner ray, pointing away from the axis
    out = out / np.linalg.norm(out)
    for rp in (0.5, 15.0):
        assert not _misses(apex, dirs, 200 * e + out * rp * (1 - 1e-6), rp)[0]
        assert not _misses(apex, dirs, 200 * e + out * rp, rp)[0]
        assert _misses(apex, dirs, 200 * e + out * rp * (1 + 1e-6) + out * 1e-6, rp)[0]


def test_cone_misses_ball_refusals():
    dirs = [[-0.1, -0.1, 1], [0.1, -0.1, 1], [0.1, 0.1, 1], [-0.1, 0.1, 1]]
    assert _misses([0, 0, 0], dirs, [50, 0, 10], 5.0)[0]
    assert _misses([0, 0, 0], dirs, [0, 0, -10], 5.0)[0]           # wholly behind the apex
    assert not _misses([0, 0, 0], dirs, [0, 0, -10], 10.0)[0]      # the apex on the padded ball
    assert not _misses([0, 0, 0], dirs, [0, 0, -10], 12.0)[0]      # the apex inside it
    assert not _misses([0, 0, 0], dirs, [0, 0, 100], 5.0)[0]       # on the axis
    wide = [[1, 0, -0.1], [0, 1, 1], [-1, 0, -0.1], [0, -1, 1]]  # two edges behind the axis' plane
    miss, _, ok = _misses([0, 0, 0], wide, [0, 0, -1000], 1.0)     # 90 degrees or more
    assert not ok and not miss
    for bad in (math.nan, math.inf):
        assert not _misses([0, 0, 0], dirs, [50, bad, 10], 5.0)[0]
        assert not _misses([bad, 0, 0], dirs, [50, 0, 10], 5.0)[0]
        assert not _misses([0, 0, 0], dirs, [50, 0, 10], bad)[0]
        assert not _misses([0, 0, 0], [[bad, -0.1, 1]] + dirs[1:], [50, 0, 10], 5.0)[0]
    assert not _misses([0, 0, 0], dirs, [1e200, 0, 10], 5.0)[0]


def test_margin_grows_with_scale_squared_over_radius():
    m = sc.lib().c2rt_sphere_margin
    assert m(300.0, 15.0) == cv.lib().c2rt_void_margin(300.0) + 1e-9 * 300.0 * 300.0 / 15.0
    vm = cv.lib().c2rt_void_margin
    assert math.isclose(m(3e6, 15.0) - vm(3e6), 100 * (m(3e5, 15.0) - vm(3e5)), rel_tol=1e-9)
    assert math.isclose(m(3e6, 1.5) - vm(3e6), 10 * (m(3e6, 15.0) - vm(3e6)), rel_tol=1e-9)
