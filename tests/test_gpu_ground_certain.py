"""Ground tiles through the short fp64 chain (chess2rt_amd/csrc/ground_certain.h; c2rt_trace.inc:
lean::ground_tile_certain; RenderParams::ground_certain_cq, scene_plan.cpp: fill_params).

Every case is rendered in one child process on the diagnostics library (the same kernel objects as the product
library's), three ways: the production frame, the COUNTED frame of the same camera (opts.count_rays: exact:: through
the general path, no ground path at all) and the CPU oracle's frame.  All three must be the same bits.  The number of
tiles that left the short chain comes from c2rt_get_ground_bails, read around the production frame; the number of
ground-only tiles from the mask table (c2rt_debug_tile_masks, as tests/test_gpu_ground_tiles.py reads it).  Frames are
61x47 (partial edge tiles) and 160x96."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import test_gpu_ground_tiles as G  # noqa: E402  (lecture5 with lines replaced, the floor shaders)

pytestmark = pytest.mark.gpu

_CHILD = r'''
import ctypes as C, json, os, sys
sys.path[:0] = [os.path.join(os.getcwd(), "tests"), os.path.join(os.getcwd(), "scripts")]
import numpy as np
import chess2rt_amd as c2, csg_void_device as vdev, oracle_lib as orc
outdir, cases = sys.argv[1], json.load(open(sys.argv[2]))
ctx = c2.Context(0)
L = orc.lib()
for case in cases:
    name = case["name"]
    path = os.path.join(outdir, name + ".sdl")
    open(path, "w").write(case["sdl"])
    scene = c2.parseSceneFromFile(path)
    scene.setFrameSize(case["W"], case["H"])
    scene.setAA(case["taps"] == 5)
    cams = [scene.beginFrame()]
    if case["down"]:  # straight down from `eye`, the image plane one unit below it, k world units per pixel on it
        (ex, ey, ez), k, W, H = case["down"]["eye"], case["down"]["k"], case["W"], case["H"]
        cam = cams[0]
        ul = (ex - W * k / 2, ey - 1.0, ez + H * k / 2)
        for i in range(3):
            cam.pos[i] = (ex, ey, ez)[i]
            cam.up_left[i] = ul[i]
            cam.up_right[i] = ul[i] + (W * k if i == 0 else 0.0)
            cam.down_left[i] = ul[i] - (H * k if i == 2 else 0.0)
    if case["kind"] == "batch":
        scene.rotateCamera(20, 0, 5)
        scene.moveCamera(-30, 10, 40)
        cams.append(scene.beginFrame())
    if case["limit"]:  # the scene files give a plane no `limit`: set in the description, which the oracle reads too
        scene.desc.contents.geom_param[1] = case["limit"]
    ctx.uploadScene(scene.desc)
    arrays, ground_only, dark, bails, redos, n = {}, 0, 0, 0, 0, 0
    world = case["world"]
    for rank in range(world):
        kw = dict(taps=case["taps"])
        if world > 1:
            kw.update(strip_height=case["sh"], strip_rank=rank, strip_world=world)
        opts = scene.renderOpts(**kw)
        counted = scene.renderOpts(count_rays=1, **kw)
        for cam in cams:
            t = vdev.read_tile_masks(ctx, cam, opts, 3)
            if t is not None:
                ground_only += int(((t[0][..., 2] & 2) != 0).sum())
                dark += int(((t[0][..., 2] & 6) == 4).sum())
        b0, r0 = ctx.groundBails(), ctx.exactRedos()
        if case["kind"] == "batch":
            import torch
            buf = torch.zeros((len(cams), ctx.localRows(opts), opts.width, 3), dtype=torch.float32, device="cuda")
            ctx.renderFramesDevice(cams, opts, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = list(buf.cpu().numpy())
        else:
            got = [ctx.renderFrame(cams[0], opts)]
        bails += ctx.groundBails() - b0
        redos += ctx.exactRedos() - r0
        if case["kind"] == "rgb32":
            packed = ctx.renderFrameRGB32(cams[0], opts)
            enc = np.array([[L.orc_color_to_rgb32((C.c_float * 3)(*px)) for px in row] for row in got[0]], dtype=np.uint32)
            arrays["packed"], arrays["encoded"] = packed, enc
        for cam, f in zip(cams, got):
            arrays["frame%d" % n] = f
            arrays["counted%d" % n] = ctx.renderFrame(cam, counted)
            arrays["ref%d" % n] = orc.render_frame(scene.desc, cam, opts, 0)
            n += 1
    np.savez(os.path.join(outdir, name + ".npz"), **arrays)
    print(json.dumps(dict(name=name, n=n, ground_only=ground_only, dark=dark, bails=int(bails), redos=int(redos))), flush=True)
print("ok")
'''


def look_down(cam, case):
    """the child's camera edit, for tests/test_ground_certain_plan.py"""
    (ex, ey, ez), k, W, H = case["down"]["eye"], case["down"]["k"], case["W"], case["H"]
    ul = (ex - W * k / 2, ey - 1.0, ez + H * k / 2)
    for i in range(3):
        cam.pos[i] = (ex, ey, ez)[i]
        cam.up_left[i] = ul[i]
        cam.up_right[i] = ul[i] + (W * k if i == 0 else 0.0)
        cam.down_left[i] = ul[i] - (H * k if i == 2 else 0.0)


def _edit(text, old, new):
    assert text.count(old) == 1, old
    return text.replace(old, new)


def _case(name, sdl, W=160, H=96, taps=5, kind="frame", sh=0, world=1, down=None, route="taken", bails=None, limit=None):
    """route: "taken" (the host hands the frame to the short chain: at least one tile goes through it or bails from it),
    "refused" (the host must not: no bail may be counted), "any"; bails: "few" (at most 1 % of the ground-only tiles),
    "some" (at least one), None"""
    return dict(name=name, sdl=sdl, W=W, H=H, taps=taps, kind=kind, sh=sh, world=world, down=down, route=route, bails=bails, limit=limit)


def _cases():
    plain = G._lecture5()
    # the floor at y = 0 under a bitmap of scaling 1/8, seen straight down from (4000, 256, 4000) — above every box of the
    # scene, which would otherwise lie behind the eye plane and keep the pre-pass from culling, and far from all of them —
    # at 1/16 unit per pixel on the image plane: pixel (x, y) lands on p.x = 4000 + 16 (x - W/2), so p.x * s is an integer
    # at every pixel centre — up to the roundings of the screen ray, which put it on either side: the interval straddles
    # a floor
    flat = _edit(plain, "y  -0.01", "y  0")
    down = dict(eye=[4000.0, 256.0, 4000.0], k=1.0 / 16)
    c = [_case("lecture5_%dx%d_t%d" % (w, h, t), plain, w, h, t, bails="few") for w, h in ((61, 47), (160, 96)) for t in (1, 5)]
    c.append(_case("down_on_integer_texels", _edit(flat, "scaling  0.005", "scaling  0.125"), down=down, bails="some"))
    c.append(_case("down_61x47", _edit(flat, "scaling  0.005", "scaling  0.37"), 61, 47, down=down))
    c.append(_case("scaling_1000", _edit(plain, "scaling  0.005", "scaling  1000"), bails="some"))
    c.append(_case("grazing_pitch_-2", G._lecture5(pitch="-2"), route="any"))
    c.append(_case("eye_1e-3_above", G._lecture5(cam_pos="0 -0.009 0"), route="any"))
    c.append(_case("eye_below", G._lecture5(cam_pos="0 -165 0", pitch="30"), route="refused"))
    c.append(_case("light_1e-3_above", G._lecture5(light_pos="-90 -0.009 350"), route="refused"))
    c.append(_case("light_below", G._lecture5(light_pos="-90 -700 350"), route="refused"))
    # the light exactly above the hit point of pixel (100, 56) of the downward frame
    c.append(_case("light_above_a_hit", _edit(_edit(flat, "scaling  0.005", "scaling  0.37"), "pos    -90 700 350", "pos    4320 700 3872"), down=down))
    # `limit` through the downward frame's footprint (x in [2720, 5280], z in [3232, 4768]): tiles inside, outside and across
    c.append(_case("limit_crossing", _edit(flat, "scaling  0.005", "scaling  0.37"), down=down, route="any", limit=4100.3))
    c.append(_case("plain_floor", G._lecture5(floor_shader=G._floor("Lambert", "      color   0.7 0.6 0.5\n"))))
    c.append(_case("checker_floor", G._lecture5(textures=G._CHECKER, floor_shader=G._floor("Lambert", '      texture "chk"\n')), route="refused"))
    c.append(_case("dark_tiles", plain, 320, 240, route="any"))
    c.append(_case("strips_2x8", plain, sh=8, world=2))
    c.append(_case("rgb32", plain, kind="rgb32"))
    c.append(_case("batch_two_cameras", plain, kind="batch"))
    return c


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    base = tmp_path_factory.mktemp("ground_certain")
    cases = _cases()
    with open(str(base / "cases.json"), "w") as f:
        json.dump(cases, f)
    env = dict(os.environ, C2RT_LIB_VARIANT="diag")
    p = subprocess.run([sys.executable, "-c", _CHILD, str(base), str(base / "cases.json")], capture_output=True, text=True,
                       timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout[-4000:] + p.stderr[-4000:]
    rows = {r["name"]: r for r in (json.loads(line) for line in p.stdout.splitlines() if line.startswith("{"))}
    assert set(rows) == {c["name"] for c in cases}
    return base, rows


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"])
def test_the_short_chain_renders_the_parents_bits(rendered, case):
    base, rows = rendered
    r, name = rows[case["name"]], case["name"]
    a = np.load(str(base / (name + ".npz")))
    print("%s: %d frames, %d ground-only tiles, %d dark, %d bails, %d redos" % (name, r["n"], r["ground_only"], r["dark"], r["bails"], r["redos"]))
    assert r["n"] >= 1
    for i in range(r["n"]):
        f, counted, ref = a["frame%d" % i], a["counted%d" % i], a["ref%d" % i]
        assert f.shape == counted.shape == ref.shape and not np.isnan(f).any()
        ne_counted = int((f.view(np.uint32) != counted.view(np.uint32)).sum())
        ne_ref = int((f.view(np.uint32) != ref.view(np.uint32)).sum())
        print("  frame %d: %d values differ from the counted frame, %d from the oracle's" % (i, ne_counted, ne_ref))
        assert ne_counted == 0 and ne_ref == 0, (name, i, ne_counted, ne_ref)
    if case["kind"] == "rgb32":
        assert np.array_equal(a["packed"], a["encoded"])
    if case["route"] == "refused":
        assert r["bails"] == 0
    if case["bails"] == "few":
        assert r["ground_only"] >= 1, "vacuous: no ground-only tile"
        assert r["bails"] <= 0.01 * r["ground_only"], (r["bails"], r["ground_only"])
    if case["bails"] == "some":
        assert r["ground_only"] >= 1 and r["bails"] > 0
    if case["down"]:
        assert r["ground_only"] >= 8, "vacuous: the downward frame has no ground-only tiles"
    if name == "dark_tiles":
        assert r["dark"] >= 1, "vacuous: no dark tile"
