"""Ground-only tiles through their own path (chess2rt_amd/csrc/c2rt_trace.inc: lean::ground_tile;
RenderParams::ground_fast, scene_plan.cpp: fill_params).

Every case is rendered twice on the diagnostics library, each time in a child process: with the path on, and with
C2RT_DEBUG_CULL=16, which leaves every tile to the general path.  The two frames must be the same bits, and each is
compared with the oracle's frame (tests/parity_util.py; the cases marked `exact`: float for float).  The number of
ground-only tiles of the frame comes from the mask table (c2rt_debug_tile_masks, tests/csg_void_device.py): an
eligible case has at least 8 of them, so that the path has something to render (but for the eye at the floor's own
height, where the pre-pass can find none: _cases); an ineligible one (Phong or Procedure2 floor, no light and hence
no ground node, the prepass preview) must simply not change.  Where a case
expects tiles outside the lean windows, c2rt_get_exact_redos is read."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]

from parity_util import TOL, maxdiff  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")

_CHILD = r'''
import ctypes as C, json, os, sys
sys.path[:0] = [os.path.join(os.getcwd(), "tests"), os.path.join(os.getcwd(), "scripts")]
import numpy as np
import chess2rt_amd as c2, csg_void_device as vdev, oracle_lib as orc
outdir, with_oracle, cases = sys.argv[1], sys.argv[2] == "1", json.load(open(sys.argv[3]))
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
    if case["eye"]:  # the same view from another eye point, the camera's frame scaled about it
        cam, scale = cams[0], case["cam_scale"]
        for corner in (cam.up_left, cam.up_right, cam.down_left):
            for i in range(3):
                corner[i] = case["eye"][i] + (corner[i] - cam.pos[i]) * scale
        for i in range(3):
            cam.pos[i] = case["eye"][i]
    if case["kind"] == "batch":
        scene.rotateCamera(20, 0, 5)
        scene.moveCamera(-30, 10, 40)
        cams.append(scene.beginFrame())
    ctx.uploadScene(scene.desc)
    frames, refs, ground_only, redos, extra = [], [], 0, 0, {}
    world = case["world"]
    for rank in range(world):
        kw = dict(taps=case["taps"])
        if world > 1:
            kw.update(strip_height=case["sh"], strip_rank=rank, strip_world=world)
        if case["kind"] == "prepass":
            kw.update(prepass_bucket=48)
        opts = scene.renderOpts(**kw)
        for cam in cams:
            t = vdev.read_tile_masks(ctx, cam, opts, 3)
            if t is not None:
                ground_only += int(((t[0][..., 2] & 2) != 0).sum())
        before = ctx.exactRedos()
        if case["kind"] == "batch":
            import torch
            buf = torch.zeros((len(cams), ctx.localRows(opts), opts.width, 3), dtype=torch.float32, device="cuda")
            ctx.renderFramesDevice(cams, opts, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = list(buf.cpu().numpy())
        else:
            got = [ctx.renderFrame(cams[0], opts)]
            if case["kind"] == "rgb32":
                extra.setdefault("packed", []).append(ctx.renderFrameRGB32(cams[0], opts))
        redos += ctx.exactRedos() - before
        frames += got
        if with_oracle:
            refs += [orc.render_frame(scene.desc, cam, opts, 0) for cam in cams]
    if "packed" in extra:  # the display frame is the encoding of the float frame, pixel for pixel (Color.toRGB32)
        flt, packed = frames[0], extra["packed"][0]
        enc = np.array([[L.orc_color_to_rgb32((C.c_float * 3)(*px)) for px in row] for row in flt], dtype=np.uint32)
        extra["packed_is_encoding"] = bool(np.array_equal(enc, packed))
    arrays = {"frame%d" % i: f for i, f in enumerate(frames)}
    arrays.update({"ref%d" % i: f for i, f in enumerate(refs)})
    if "packed" in extra:
        arrays["packed"] = extra["packed"][0]
    np.savez(os.path.join(outdir, name + ".npz"), **arrays)
    print(json.dumps(dict(name=name, n=len(frames), ground_only=ground_only, redos=int(redos),
                          packed_is_encoding=extra.get("packed_is_encoding"))), flush=True)
print("ok")
'''


def _lecture5(**edits):
    """lecture5.sdl with some of its lines replaced; the bitmaps by absolute path, so that the copy loads from anywhere"""
    text = open(os.path.join(SCENES, "lecture5.sdl")).read()
    for bmp in ("floor.bmp", "world.bmp"):
        text = text.replace('"%s"' % bmp, '"%s"' % os.path.join(SCENES, bmp))
    swaps = {
        "cam_pos": ("pos    0 165 0", "pos    %s"),
        "pitch": ("pitch  -30", "pitch  %s"),
        "light_pos": ("pos    -90 700 350", "pos    %s"),
        "power": ("power  800000", "power  %s"),
        "floor_shader": ('Lambert {\n      name    "floor_shader"\n      texture "bmp"\n    }', "%s"),
        "textures": ("  Textures {\n", "  Textures {\n%s\n"),
        "lights": (text[text.index("  Lights {"):text.index("  Geometries {")], "%s"),
    }
    for key, value in edits.items():
        old, new = swaps[key]
        assert text.count(old) == 1, key
        text = text.replace(old, new % value)
    return text


_CHECKER = '    Checker {\n      name "chk"\n      color1 0.9 0.9 0.9\n      color2 0.1 0.3 0.1\n      size 37\n    }'
_PROC2 = ('    Procedure2 {\n      name "proc2"\n      freqU 0.01 0.25 0.01\n      freqV 0.01 0.25 0.01\n'
          '      colorU {\n        color 0.7 0.1 0.2\n        color 0.3 0.4 0.9\n        color 0.5 0.8 0.1\n      }\n'
          '      colorV {\n        color 0.2 0.6 0.1\n        color 0.1 0.1 0.8\n        color 0.6 0.2 0.4\n      }\n    }')


def _floor(kind, body):
    return '%s {\n      name    "floor_shader"\n%s    }' % (kind, body)


def _case(name, sdl, W=160, H=120, taps=5, kind="frame", sh=0, world=1, eligible=True, tiles=None, redos=False, exact=False,
          eye=None, cam_scale=1.0):
    """eligible: the host hands the frame to the path (RenderParams::ground_fast); tiles: the frame must have at least 8
    ground-only tiles (every eligible case but one); redos: tiles outside the lean windows are expected; exact: the
    frame must equal the oracle's float for float"""
    return dict(name=name, sdl=sdl, W=W, H=H, taps=taps, kind=kind, sh=sh, world=world, eligible=eligible,
                tiles=eligible if tiles is None else tiles, redos=redos, exact=exact, eye=eye, cam_scale=cam_scale)


def _cases():
    plain = _lecture5()
    c = [_case("lecture5_%dx%d_t%d" % (w, h, t), plain, w, h, t) for w, h in ((160, 120), (333, 217)) for t in (1, 5)]
    c += [_case("lecture5_strips_%d_%d" % (world, sh), plain, 640, 480, 5, sh=sh, world=world) for world, sh in ((2, 8), (3, 4))]
    c.append(_case("rgb32", plain, kind="rgb32"))
    c.append(_case("prepass48", plain, kind="prepass", eligible=False))  # a preview has no mask table
    c.append(_case("batch_two_cameras", plain, kind="batch"))
    c.append(_case("checker_floor", _lecture5(textures=_CHECKER, floor_shader=_floor("Lambert", '      texture "chk"\n'))))
    c.append(_case("plain_floor", _lecture5(floor_shader=_floor("Lambert", "      color   0.7 0.6 0.5\n"))))
    c.append(_case("phong_floor", _lecture5(floor_shader=_floor("Phong", '      texture "bmp"\n      exponent 30\n')), eligible=False))
    c.append(_case("procedure2_floor", _lecture5(textures=_PROC2, floor_shader=_floor("Lambert", '      texture "proc2"\n')), eligible=False))
    # ambient only: without a light the scene has no ground node (nothing to refine shadow masks for), hence no
    # ground-only tile; a light of power 0 keeps them and is skipped by its `lit` bit
    c.append(_case("no_light", _lecture5(lights="  Lights {\n  }\n\n"), eligible=False))
    c.append(_case("power_0", _lecture5(power="0")))
    # every sample's shadow pre-check fails (eye and light on opposite sides of the floor): the general path, same wave
    c.append(_case("light_below_floor", _lecture5(light_pos="-90 -700 350"), exact=True))
    c.append(_case("camera_under_floor", _lecture5(cam_pos="0 -165 0", pitch="30")))
    # the upper tiles look along and above the horizon: `away` lanes, rays within 1e-9 of parallel
    c.append(_case("pitch_0", _lecture5(pitch="0")))
    # Operands outside the lean windows.  A zero numerator: the eye at the floor's height.  (No tile of such a frame is
    # ground-only, whatever the camera: the pre-pass accepts a tile's footprint only where its corner rays meet the
    # plane at t > 0, and t = (y - eye.y) / dir.y is 0 for every ray.  The case holds the path to changing nothing.)
    c.append(_case("eye_on_floor_height", _lecture5(cam_pos="0 -0.01 0"), tiles=False, redos=True, exact=True))
    # The eye at y = 1e80.  The scene file's camera cannot look down from there — its image plane lies one unit in
    # front of the eye and up_left.y == pos.y in fp64: every ray is horizontal, Plane.intersect rejects it before its
    # division and nothing leaves a window.  So the camera's frame is scaled with the eye's height: the same view, rays
    # of length 1e80 whose squared length is beyond the window — every tile is redone, ground-only ones by the path's
    # own say-so.
    c.append(_case("eye_at_1e80", plain, redos=True, exact=True, eye=[0.0, 1e80, 0.0], cam_scale=1e80))
    return c


def _run_child(cases, outdir, env_extra, with_oracle):
    os.makedirs(outdir)
    with open(os.path.join(outdir, "cases.json"), "w") as f:
        json.dump(cases, f)
    env = dict(os.environ, C2RT_LIB_VARIANT="diag", **env_extra)
    p = subprocess.run([sys.executable, "-c", _CHILD, outdir, "1" if with_oracle else "0", os.path.join(outdir, "cases.json")],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout[-4000:] + p.stderr[-4000:]
    return {r["name"]: r for r in (json.loads(line) for line in p.stdout.splitlines() if line.startswith("{"))}, p.stderr


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    """every case with the path on (and the oracle's frames), then with C2RT_DEBUG_CULL=16: two child processes in all"""
    base = tmp_path_factory.mktemp("ground_tiles")
    cases = _cases()
    on, _ = _run_child(cases, str(base / "on"), {}, True)
    off, err = _run_child(cases, str(base / "off"), dict(C2RT_DEBUG_CULL="16"), False)
    assert "C2RT_DEBUG_CULL=16" in err  # the hook announces itself, as for the other bits
    assert set(on) == set(off) == {c["name"] for c in cases}
    return base, on, off


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"])
def test_ground_tiles_render_the_same_bits_with_the_path_on_and_off(rendered, case):
    base, on, off = rendered
    name = case["name"]
    a, b = np.load(str(base / "on" / (name + ".npz"))), np.load(str(base / "off" / (name + ".npz")))
    r_on, r_off = on[name], off[name]
    print("%s: %d frames, %d ground-only tiles, redos on %d / off %d" % (name, r_on["n"], r_on["ground_only"], r_on["redos"], r_off["redos"]))
    assert r_on["n"] == r_off["n"] >= 1 and r_on["ground_only"] == r_off["ground_only"]
    if case["tiles"]:
        assert r_on["ground_only"] >= 8, "vacuous: the frame has no ground-only tiles for the path to render"
    for i in range(r_on["n"]):
        fa, fb, ref = a["frame%d" % i], b["frame%d" % i], a["ref%d" % i]
        assert fa.shape == ref.shape and bool(np.any(fa)) == bool(np.any(ref))  # (from 1e80 nothing is in reach: a black frame)
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), (name, i, maxdiff(fa, fb))
        for which, f in (("on", fa), ("off", fb)):
            md, nbad, nne = maxdiff(f, ref)
            print("  frame %d, path %s: max |gpu - oracle| = %.3g, %d values differ" % (i, which, md, nne))
            assert np.array_equal(np.isnan(f), np.isnan(ref)), (name, i, which)
            assert md <= TOL and nbad == 0, (name, i, which, md, nbad)
            if case["exact"]:
                assert nne == 0, (name, i, which, md, nne)
    if case["kind"] == "rgb32":
        assert np.array_equal(a["packed"], b["packed"]) and r_on["packed_is_encoding"] and r_off["packed_is_encoding"]
    if case["redos"]:
        assert r_on["redos"] >= 1 and r_off["redos"] >= 1, (r_on["redos"], r_off["redos"])
