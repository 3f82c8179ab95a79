"""The CsgDiff void-tile pre-pass on the device (chess2rt_amd/csrc/csg_void.h, c2rt_tile_mask.inc: tile_mask_entry).

test_device_drops_equal_host_claims reads the mask table back through the diagnostics build's c2rt_debug_tile_masks
(tests/csg_void_device.py) at void_flags_mask 0, 1 and 3 and insists that the device dropped a node from exactly
the tiles the host classifier (tests/libcsg_void_check.so, which tests/test_csg_void_tiles.py checks ray by ray in
the oracle) calls void — tile bounds restated from tile_mask_entry for ragged, strip-sharded and full frames — and
that the VoidCull the library built equals its Python restatement bit for bit.  The frame tests render the same
scene families (tests/csg_void_scenes.py) with both kernel instances and compare them with the oracle: a pre-pass
that claimed too much would show there."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chess2rt_amd as c2
import csg_void_scenes as S
import oracle_lib as orc
from parity_util import TOL, maxdiff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import csg_void_tiles as cv  # noqa: E402

pytestmark = pytest.mark.gpu

# Runs in a child process on the diagnostics library.  Every case: (name, sdl text or None = lecture5, W, H,
# taps, strip_height, strip_world); strips: every rank.  Prints one JSON line per frame configuration.
_CHILD = r'''
import json, os, sys, tempfile
sys.path[:0] = [os.path.join(os.getcwd(), "tests"), os.path.join(os.getcwd(), "scripts")]
import chess2rt_amd as c2, csg_void_device as dev, csg_void_scenes as S, csg_void_tiles as cv
cases = json.loads(sys.argv[1])
debug_cull = int(os.environ.get("C2RT_DEBUG_CULL", "0"))
ctx = c2.Context(0)
tmp = tempfile.mkdtemp()
for name, sdl, W, H, taps, sh, world in cases:
    path = S.LECTURE5
    if sdl is not None:
        path = os.path.join(tmp, name + ".sdl")
        open(path, "w").write(sdl)
    scene = c2.parseSceneFromFile(path)
    scene.setFrameSize(W, H)
    cam = scene.beginFrame()
    ctx.uploadScene(scene.desc)
    for rank in range(world):
        opts = scene.renderOpts(taps=taps, strip_height=sh, strip_rank=rank, strip_world=world)
        counts = dev.compare(ctx, scene.desc, cam, opts, debug_cull)
        keep = 0
        for cand in cv.void_candidates(scene.desc):
            keep += int(cv.node_rect_tiles(cam, W, H, cand.lo, cand.hi).sum())
        print(json.dumps(dict(name=name, rank=rank, world=world, candidates=[c.node for c in cv.void_candidates(scene.desc)],
                              counts=counts and {str(k): v for k, v in counts.items()}, rect_tiles=keep)), flush=True)
print("ok")
'''


def _run_child(cases, env_extra=None, timeout=600):
    env = dict(os.environ, C2RT_LIB_VARIANT="diag", **(env_extra or {}))
    p = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(cases)], capture_output=True, text=True, timeout=timeout,
                       env=env, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout[-4000:] + p.stderr[-4000:]
    rows = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    for r in rows:
        print("%-28s rank %d/%d  candidates %s  drops (primary, shadow) %s" % (r["name"], r["rank"], r["world"], r["candidates"], r["counts"]))
    return rows


def _cases():
    c = [("lecture5_640", None, 640, 480, 5, 0, 1), ("lecture5_333x217", None, 333, 217, 4, 0, 1),
         ("lecture5_4k", None, 3840, 2160, 5, 0, 1)]
    c += [("lecture5_strips_%d_%d" % (world, sh), None, 640, 480, 5, sh, world) for world, sh in ((2, 8), (3, 4), (8, 12))]
    c += [("fuzz%d" % s, S.fuzz_scene(s), 320, 240, 5, 0, 1) for s in range(24)]
    c += [("fuzz%d_%dx%d" % (s, W, H), S.fuzz_scene(s), W, H, 1, 0, 1) for s in range(4) for W, H in ((161, 97), (1, 70), (333, 217))]
    c += [(name, sdl, 160, 120, 5, 0, 1) for name, sdl in S.adversarial()]
    c += [("below_granted", S.light_below_ground(True), 320, 240, 5, 0, 1),
          ("below_refused", S.light_below_ground(False), 320, 240, 5, 0, 1)]
    c += [("lights%d" % n, S.several_lights(n), 320, 240, 5, 0, 1) for n in (2, 3, 4)]
    c += [("cand%d" % n, S.several_candidates(n), 640, 480, 1, 0, 1) for n in (2, 4, 5)]
    c += [("cand_0_31_33", S.candidates_at_0_31_33(), 640, 480, 1, 0, 1), ("translated", S.translated_candidate(), 320, 240, 5, 0, 1)]
    c += [("cand5_strips_3_12", S.several_candidates(5), 640, 480, 1, 12, 3)]
    return c


def test_device_drops_equal_host_claims():
    rows = _run_child(_cases())
    by = {}
    for r in rows:
        by.setdefault(r["name"], []).append(r)
    assert set(by) == {c[0] for c in _cases()}

    def total(name, k):
        return sum(v[k] for r in by[name] for v in (r["counts"] or {}).values())

    # not vacuous: the designed scenes drop the node, from primary masks and (where the scene allows) shadow masks
    assert total("lecture5_640", 0) >= 50 and total("lecture5_640", 1) >= 1
    for name in ("lecture5_strips_2_8", "lecture5_strips_3_4", "lecture5_strips_8_12"):
        assert total(name, 0) >= 25, name
    assert total("below_granted", 0) >= 1 and total("below_refused", 1) == 0
    assert sum(total("fuzz%d" % s, 0) for s in range(24)) >= 10
    for n in (2, 3, 4):
        assert total("lights%d" % n, 0) >= 5
    for n in (4, 5):
        assert {r["candidates"] == [2, 3, 5, 6] for r in by["cand%d" % n]} == {True}
        assert total("cand%d" % n, 0) >= 50
    assert by["cand_0_31_33"][0]["candidates"] == [0, 31]
    assert by["cand_0_31_33"][0]["counts"]["0"][0] >= 10 and by["cand_0_31_33"][0]["counts"]["31"][0] >= 10
    assert total("translated", 0) >= 5
    # the headline frame: DESIGN.md 4.1 records ~43 % of the node's rectangle tiles dropped at 4K
    k4 = by["lecture5_4k"][0]
    share = total("lecture5_4k", 0) / k4["rect_tiles"]
    print("lecture5 4K: %d of %d rectangle tiles dropped (%.1f %%)" % (total("lecture5_4k", 0), k4["rect_tiles"], 100 * share))
    assert share > 0.3


def test_voidcull_follows_the_frames_culling_switches():
    """C2RT_DEBUG_CULL=4 (diagnostics build: no shadow-ray culling): the frame's VoidCull loses its shadow flags
    (prepare_tile_masks) — and the device then drops nothing from word 1"""
    rows = _run_child([("lecture5_640", None, 640, 480, 5, 0, 1), ("below_granted", S.light_below_ground(True), 320, 240, 5, 0, 1)],
                      env_extra=dict(C2RT_DEBUG_CULL="4"))
    assert all(v[1] == 0 for r in rows for v in r["counts"].values())
    assert sum(v[0] for r in rows for v in r["counts"].values()) >= 50


# ---- frames against the oracle ------------------------------------------------------------------------------------

def _scene(tmp_path, name, sdl, W, H):
    path = S.LECTURE5
    if sdl is not None:
        path = tmp_path / (name + ".sdl")
        path.write_text(sdl)
    scene = c2.parseSceneFromFile(str(path))
    scene.setFrameSize(W, H)
    return scene


def _host_primary_claims(scene, cam, W, H):
    return sum(int(((cv.classify(scene.desc, cam, W, H, cand) & 1) != 0).sum()) for cand in cv.void_candidates(scene.desc))


def _frame_check(ctx, scene, cam, opts, exact=True):
    ctx.uploadScene(scene.desc)
    gpu = ctx.renderFrame(cam, opts)
    st = {}
    ref = orc.render_frame(scene.desc, cam, opts, 0, st if opts.count_rays else None)
    assert gpu.shape == ref.shape
    if exact:
        assert np.array_equal(gpu.view(np.uint32), ref.view(np.uint32))
    else:
        md, nbad, _ = maxdiff(gpu, ref)
        assert md <= TOL and nbad == 0, md
    if opts.count_rays:
        assert ctx.rayStats() == (st["primary"], st["shadow"])


def _families():
    f = [("fuzz%d" % s, S.fuzz_scene(s), 320, 240, 5) for s in range(24)]
    f += [("fuzz%d_%dx%d_t%d" % (s, W, H, t), S.fuzz_scene(s), W, H, t) for s in (0, 1) for W, H in ((161, 97), (1, 70), (333, 217))
          for t in (1, 5)]
    f += [(name, sdl, 160, 120, 5) for name, sdl in S.adversarial()]
    f += [("below_granted", S.light_below_ground(True), 320, 240, 5), ("below_refused", S.light_below_ground(False), 320, 240, 5)]
    f += [("lights%d" % n, S.several_lights(n), 320, 240, 5) for n in (2, 3, 4)]
    f += [("cand%d" % n, S.several_candidates(n), 640, 480, 1) for n in (2, 4, 5)]
    f += [("cand_0_31_33", S.candidates_at_0_31_33(), 640, 480, 1), ("translated", S.translated_candidate(), 320, 240, 5)]
    return f


_FAMILY_MIN_CLAIMS = {"below_granted": 1, "lights2": 5, "cand5": 50, "cand_0_31_33": 50, "translated": 5}


@pytest.mark.parametrize("family", ["fuzz", "adversarial", "designed"])
def test_void_scene_frames_match_oracle(gpu_ctx, tmp_path, family):
    """Lambert scenes: counted and production frames bit-equal to the oracle, ray counts equal"""
    names = {n for n, *_ in S.adversarial()}
    claims = 0
    for name, sdl, W, H, taps in _families():
        kind = "fuzz" if name.startswith("fuzz") else "adversarial" if name in names else "designed"
        if kind != family:
            continue
        scene = _scene(tmp_path, name, sdl, W, H)
        cam = scene.beginFrame()
        n = _host_primary_claims(scene, cam, W, H)
        assert n >= _FAMILY_MIN_CLAIMS.get(name, 0), (name, n)
        claims += n
        _frame_check(gpu_ctx, scene, cam, scene.renderOpts(taps=taps, count_rays=1))
    print("%s: %d host-claimed void tiles" % (family, claims))
    assert claims >= 10


@pytest.mark.parametrize("world,sh", [(2, 8), (3, 4), (8, 12)])
def test_lecture5_strip_frames_match_oracle_rows(gpu_ctx, world, sh):
    """Strip-sharded lecture5 (Phong: the suite's tolerance) at strip heights where a tile spans two strips"""
    scene = _scene(None, "lecture5", None, 640, 480)
    cam = scene.beginFrame()
    for rank in range(world):
        _frame_check(gpu_ctx, scene, cam, scene.renderOpts(count_rays=1, strip_height=sh, strip_rank=rank, strip_world=world),
                     exact=False)


def test_lecture5_chunked_4k_frame_matches_oracle(gpu_ctx):
    """A pinned host frame renders in row chunks that share one mask table (render_to_host)"""
    scene = _scene(None, "lecture5", None, 3840, 2160)
    scene.setAA(False)
    cam = scene.beginFrame()
    assert _host_primary_claims(scene, cam, 3840, 2160) > 10000
    opts = scene.renderOpts()
    gpu_ctx.uploadScene(scene.desc)
    out = np.empty((2160, 3840, 3), dtype=np.float32)
    gpu_ctx.pinHostBuffer(out)
    try:
        gpu_ctx.renderFrameInto(cam, opts, out)
    finally:
        gpu_ctx.unpinHostBuffer(out)
    ref = orc.render_frame(scene.desc, cam, opts, 0)
    md, nbad, _ = maxdiff(out, ref)
    assert md <= TOL and nbad == 0, md


def test_multi_device_context_void_frames_match_oracle(tmp_path):
    """Context(devices=[0, 0, 0]): three slots deal 8-row strips and each runs its own pre-pass"""
    ctx = c2.Context(devices=[0, 0, 0])
    try:
        for name, sdl, W, H in (("lecture5", None, 640, 480), ("fuzz3", S.fuzz_scene(3), 333, 217),
                                ("below_granted", S.light_below_ground(True), 320, 240)):
            scene = _scene(tmp_path, name, sdl, W, H)
            cam = scene.beginFrame()
            assert _host_primary_claims(scene, cam, W, H) >= 1 or name == "fuzz3"
            _frame_check(ctx, scene, cam, scene.renderOpts(count_rays=1), exact=sdl is not None)
    finally:
        ctx.close()


def test_lecture5_moving_camera_frames_match_oracle(gpu_ctx):
    """moveCamera / rotateCamera into the sphere, into the box and the sphere, into the box's corner outside the
    sphere, and out: every frame against the oracle"""
    scene = _scene(None, "lecture5", None, 320, 240)
    cam = scene.beginFrame()
    _frame_check(gpu_ctx, scene, cam, scene.renderOpts(count_rays=1), exact=False)
    for dyaw, droll, dpitch, dx, dy, dz in S.camera_path():
        scene.rotateCamera(dyaw, droll, dpitch)
        scene.moveCamera(dx, dy, dz)
        cam = scene.beginFrame()
        _frame_check(gpu_ctx, scene, cam, scene.renderOpts(count_rays=1), exact=False)
