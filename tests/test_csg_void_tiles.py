"""The mask pre-pass drops a CsgDiff(L, Sphere) node from tiles whose rays provably miss it
(chess2rt_amd/csrc/csg_void.h).  On the host, through the same classifier (tests/libcsg_void_check.so): every
primary ray (5 taps) of a tile called void, and every ground shadow ray towards light 0 of a tile called
shadow-void, gets no hit on the node in the oracle — lecture5 at three sizes, fuzzed Diff(cube | sphere, sphere)
scenes under random cameras, and adversarial set-ups where the test must refuse or be right."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import csg_void_scenes as S  # noqa: E402
import csg_void_tiles as cv  # noqa: E402

LECTURE5 = S.LECTURE5


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
            cv.check_tile(desc, cam, W, H, cand.node, int(ty), int(tx), int(cls[ty, tx]), light, gn)
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


def _run(tmp_path, sdl, name, W=64, H=48):
    p = tmp_path / (name + ".sdl")
    p.write_text(sdl)
    scene, cam = _load(str(p), W, H)
    return _check_all(scene, cam, W, H)


@pytest.mark.parametrize("seed", range(24))
def test_fuzzed_diff_scenes(tmp_path, seed):
    _run(tmp_path, S.fuzz_scene(seed), "fuzz%d" % seed, 320, 240)


def test_sphere_just_large_enough(tmp_path):
    for name, sdl in S.just_large_enough():
        _run(tmp_path, sdl, name, 160, 120)


def test_tangent_rays(tmp_path):
    for name, sdl in S.tangent_rays():
        _run(tmp_path, sdl, name, 160, 120)


def test_eye_inside_sphere_and_box(tmp_path):
    for name, sdl in S.eye_inside():
        _run(tmp_path, sdl, name, 160, 120)


def test_light_inside_box_refuses_shadow(tmp_path):
    for name, sdl in S.light_inside_box():
        _run(tmp_path, sdl, name, 160, 120)


@pytest.mark.parametrize("granted", [True, False])
def test_light_below_the_ground(tmp_path, granted):
    """The ground above the light (h < 0): the shadow test where the box lies between them, not where the light is
    level with the box; every claimed ray checked in the oracle"""
    p = tmp_path / "below.sdl"
    p.write_text(S.light_below_ground(granted))
    scene, cam = _load(str(p), 320, 240)
    (cand,) = cv.void_candidates(scene.desc)
    assert cand.flags == (3 if granted else 1)
    assert _check_all(scene, cam, 320, 240) > 0
    if granted:
        cls = cv.classify(scene.desc, cam, 320, 240, cand)
        assert int(((cls & 2) != 0).sum()) > 0


@pytest.mark.parametrize("n_cand", [2, 4, 5])
def test_several_candidates(tmp_path, n_cand):
    """The library tests the first four CsgDiff(Cube | Sphere, Sphere) nodes under identity matrices; rotated, scaled,
    Diff(Sphere, Cube) and Diff(L, L) nodes are no candidates.  Every claim checked in the oracle."""
    p = tmp_path / "cand.sdl"
    p.write_text(S.several_candidates(n_cand))
    scene, cam = _load(str(p), 640, 480)
    assert [c.node for c in cv.void_candidates(scene.desc)] == [2, 3, 5, 6][:n_cand]
    assert _check_all(scene, cam, 640, 480, sample=60) > (50 if n_cand >= 3 else 5)


def test_candidates_below_kmaxcullnodes_only(tmp_path):
    p = tmp_path / "idx.sdl"
    p.write_text(S.candidates_at_0_31_33())
    scene, cam = _load(str(p), 640, 480)
    assert scene.desc.contents.n_nodes == 36
    assert cv.ground_of(scene.desc) == (1, -0.01)
    assert [c.node for c in cv.void_candidates(scene.desc)] == [0, 31]
    assert _check_all(scene, cam, 640, 480, sample=60) > 20


@pytest.mark.parametrize("world,sh", [(1, 1), (2, 8), (3, 4), (8, 12)])
def test_strip_tiles_through_the_per_tile_entry(world, sh):
    """The tiles a strip-sharded frame's pre-pass evaluates (tile_bounds: a tile spans two strips at heights 4 and 12)
    classified through c2rt_void_classify_tiles; every claimed ray of every row in the tile's frame-row span checked
    in the oracle (a sample per rank).  Unsharded, the per-tile entry reproduces c2rt_void_classify."""
    from chess2rt_amd.sharding import local_rows

    W, H = 640, 480
    scene, cam = _load(LECTURE5, W, H)
    (cand,) = cv.void_candidates(scene.desc)
    gn, _ = cv.ground_of(scene.desc)
    D = cv._fields(scene.desc)
    light = [D.light_pos[i] for i in range(3)]
    claimed = 0
    for rank in range(world):
        rows = local_rows(H, sh, rank, world) if world > 1 else H
        bounds = [cv.tile_bounds(r, c, 0, rows, sh, rank, world) for r in range((rows + 7) // 8) for c in range((W + 7) // 8)]
        if world > 1 and sh % 8:
            assert any(b[2] - b[1] > 7 for b in bounds)  # tiles spanning two strips
        cls = cv.classify_tiles(scene.desc, cam, bounds, cand)
        if world == 1:
            assert np.array_equal(cls, cv.classify(scene.desc, cam, W, H, cand).ravel())
        idx = list(np.nonzero(cls)[0])
        claimed += len(idx)
        rng = np.random.default_rng(rank)
        for k in rng.choice(idx, size=min(25, len(idx)), replace=False) if idx else []:
            cv.check_tile_bounds(scene.desc, cam, W, H, cand.node, bounds[k], int(cls[k]), light, gn)
    assert claimed > 20


def test_second_light_shadows_tiles_that_are_shadow_void_for_light_0(tmp_path):
    """The shadow test covers light 0 only: on tiles where it drops the node for light 0, light 1 still finds the
    node in its way (the frames must show that shadow: tests/test_gpu_csg_void.py renders these scenes)"""
    import ctypes as C

    import oracle_lib
    from oracle_lib import OrcHit

    p = tmp_path / "lights.sdl"
    p.write_text(S.several_lights(2))
    W, H = 320, 240
    scene, cam = _load(str(p), W, H)
    (cand,) = cv.void_candidates(scene.desc)
    cls = cv.classify(scene.desc, cam, W, H, cand)
    gn, _ = cv.ground_of(scene.desc)
    D = cv._fields(scene.desc)
    L1 = [D.light_pos[3 + i] for i in range(3)]
    L = oracle_lib.lib()
    o, d = (C.c_double * 3)(), (C.c_double * 3)()
    shadowed = 0
    for ty, tx in zip(*np.nonzero(cls & 2)):
        for y in range(ty * 8, min(ty * 8 + 8, H)):
            for x in range(tx * 8, min(tx * 8 + 8, W)):
                L.orc_screen_ray(C.byref(cam), float(x), float(y), o, d)
                gh = OrcHit()
                gh.dist = 1e99
                if L.orc_node_intersect(scene.desc, cand.node, o, d, C.byref(gh)) or not L.orc_node_intersect(scene.desc, gn, o, d, C.byref(gh)):
                    continue
                frm = [gh.p[i] + 1e-6 for i in range(3)]
                v = [L1[i] - frm[i] for i in range(3)]
                dist = sum(t * t for t in v) ** 0.5
                sh = OrcHit()
                sh.dist = dist
                shadowed += bool(L.orc_node_intersect(scene.desc, cand.node, cv._a3(frm), cv._a3([t / dist for t in v]), C.byref(sh)))
    assert shadowed > 0


def _first_violation(scene, cam, W, H, cand, factor):
    """(tiles the classifier adds when the ball is inflated by `factor`, the first of them with a ray that hits the
    node in the oracle, or None)"""
    D = cv._fields(scene.desc)
    gn, _ = cv.ground_of(scene.desc)
    light = [D.light_pos[i] for i in range(3)]
    base = cv.classify(scene.desc, cam, W, H, cand)
    big = cv.classify(scene.desc, cam, W, H, cand, r_override=cand.R * factor)
    added = list(zip(*np.nonzero(big & ~base)))
    for ty, tx in added:
        try:
            cv.check_tile(scene.desc, cam, W, H, cand.node, int(ty), int(tx), int(big[ty, tx] & ~base[ty, tx]), light, gn)
        except AssertionError:
            return len(added), (ty, tx)
    return len(added), None


def test_mutation_inflated_ball_is_caught_on_lecture5():
    """A classifier that is too generous must fail the oracle check.  The bound has slack: on lecture5 at 640x480
    (R = 70) a ball of 72 adds tiles none of whose rays hits the node, 74 adds one such tile, 77 (x 1.10) dozens."""
    scene, cam = _load(LECTURE5, 640, 480)
    (cand,) = cv.void_candidates(scene.desc)
    n_added, bad = _first_violation(scene, cam, 640, 480, cand, 1.10)
    assert n_added > 100 and bad is not None
    _, bad = _first_violation(scene, cam, 640, 480, cand, 1.0)
    assert bad is None


def test_mutation_inflated_ball_is_caught_near_tangent(tmp_path):
    """Harder: a sphere barely larger than the cube's face half-diagonal (R = 71 against 70.71), seen from close by
    at 1280x960, where the thick segment is thinner: x 1.02 adds 761 tiles none of whose rays hits the node, x 1.04
    adds 1581, and some of their rays do."""
    p = tmp_path / "tangent.sdl"
    p.write_text(S.lecture5_like(71.0, (-100, 160, 60), 0.0, -35.0))
    scene, cam = _load(str(p), 1280, 960)
    (cand,) = cv.void_candidates(scene.desc)
    n_added, bad = _first_violation(scene, cam, 1280, 960, cand, 1.04)
    assert n_added > 1000 and bad is not None


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
