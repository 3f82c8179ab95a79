"""Sphere-interior tiles on the device (chess2rt_amd/csrc/csg_void.h: sphere_interior_tile; c2rt_tile_mask.inc:
tile_mask_entry writes bit 3 of the mask table's third word; lean::sphere_tile renders such a tile with its one sphere
and nothing else).

Small frames in which a ball fills most of the view — lecture5.sdl without its CsgDiff node (behind the eye its box
keeps the whole frame), the camera 65 in front of the globe's centre or 20 in front of a Phong ball moved off to the
side —, each rendered in a child process on the diagnostics library, once with C2RT_DEBUG_CULL=256 (the path as shipped,
less the condition that keeps it to frames of six million samples and more) and once with C2RT_DEBUG_CULL=128 (no
sphere-interior tiles).  In every case the device's bit-3 tiles equal the host classifier's claims tile for tile
(scripts/sphere_interior_tiles.py, which tests/test_sphere_interior_tiles.py checks sample by sample in the oracle),
the two frames are the same bits, the frame equals the oracle's float for float, and c2rt_get_sphere_bails does not
move."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import sphere_tile_scenes as T  # noqa: E402

SCENES = T.SCENES
_TEXTS = T.texts()
GLOBE, BALL = _TEXTS["globe"], _TEXTS["ball"]
GLOBE_SHADER, GLOBE_TEXTURE = T.GLOBE_SHADER, T.GLOBE_TEXTURE


def _phong(e):
    return GLOBE.replace(GLOBE_SHADER, 'Phong {\n      name      "globe_shader"\n      color     0.7 0.4 0.2\n      exponent  %s\n    }' % e)


def _case(name, text, size=(64, 48), taps=5, ranks=1, strip=0, rgb32=False, batch=False, scale=1.0, min_claimed=20, redos=False):
    return dict(name=name, text=text, size=list(size), taps=taps, ranks=ranks, strip=strip, rgb32=rgb32, batch=batch, scale=scale,
                min_claimed=min_claimed, redos=redos)


CASES = [
    _case("globe_bitmap", GLOBE),
    _case("globe_bitmap_scaling_0005", GLOBE.replace(GLOBE_TEXTURE, GLOBE_TEXTURE[:-6] + '\n      scaling  0.005\n    }')),
    _case("globe_lambert_plain", GLOBE.replace(GLOBE_SHADER, 'Lambert {\n      name    "globe_shader"\n      color   0.7 0.4 0.2\n    }')),
    _case("globe_phong_1", _phong("1")),
    _case("globe_phong_60", _phong("60"), taps=1),
    _case("globe_phong_80", _phong("80")),
    _case("globe_phong_2_5", _phong("2.5")),
    _case("ball_offset_phong", BALL),
    _case("ball_self_shadowed", _TEXTS["ball_self_shadowed"]),
    _case("globe_power_0", GLOBE.replace("power  800000", "power  0")),
    _case("globe_one_tap_edge", GLOBE, size=(60, 44), taps=1),
    _case("globe_edge_5", GLOBE, size=(61, 43)),
    _case("globe_strips", GLOBE, size=(64, 64), ranks=2, strip=8),
    _case("globe_rgb32", GLOBE, rgb32=True),
    _case("globe_batch", GLOBE, batch=True),
    # every coordinate beyond the lean windows: each tile is rendered again through exact::, the claimed ones after the path
    # has raised `bad` and written nothing
    _case("ball_1e80", None, scale=1e80, redos=True),
]
# no light and no floor: the planner has no ground node, the globe is all the primary mask keeps and the claim needs no
# shadow condition; the path's ambient-only branch renders every tile
CASES.append(_case("globe_no_light", _TEXTS["no_light"]))

_CHILD = r'''
import ctypes as C, json, os, sys
sys.path[:0] = [os.path.join(os.getcwd(), "tests"), os.path.join(os.getcwd(), "scripts")]
import numpy as np
import chess2rt_amd as c2, csg_void_device as vdev, csg_void_tiles as cv, sphere_interior_tiles as si, oracle_lib as orc
outdir, with_oracle = sys.argv[1], sys.argv[2] == "1"
cases = json.load(open(sys.argv[3]))
debug_cull = int(os.environ.get("C2RT_DEBUG_CULL", "0"))
ctx = c2.Context(0)
for case in cases:
    name = case["name"]
    W, H = case["size"]
    scene = c2.parseSceneFromFile(os.path.join(outdir, "..", name + ".sdl"))
    scene.setFrameSize(W, H)
    cam0 = scene.beginFrame()
    cams = [cam0]
    if case["batch"]:
        scene.rotateCamera(4, 0, 3)
        cams.append(scene.beginFrame())
    if case["scale"] != 1.0:   # the same picture at 1e80: the description and the camera frame scaled (the file format's camera cannot be)
        s = case["scale"]
        d = scene.desc.contents
        for g in range(d.n_geoms):
            for i in range(4):
                d.geom_param[4 * g + i] *= s
        for n in range(d.n_nodes):
            for i in range(27, 30):
                d.node_transform[30 * n + i] *= s
        for i in range(3 * d.n_lights):
            d.light_pos[i] *= s
        for cam in cams:
            for f in ("pos", "up_left", "up_right", "down_left"):
                v = getattr(cam, f)
                for i in range(3):
                    v[i] *= s
    ctx.uploadScene(scene.desc)
    arrays, claimed, differ = {}, 0, 0
    redos0, bails0 = ctx.exactRedos(), ctx.sphereBails()
    for rank in range(case["ranks"]):
        kw = dict(taps=case["taps"])
        if case["ranks"] > 1:
            kw.update(strip_height=case["strip"], strip_rank=rank, strip_world=case["ranks"])
        opts = scene.renderOpts(**kw)
        for cam in cams:
            m, info, _ = vdev.read_tile_masks(ctx, cam, opts, 3)
            bounds = [cv.tile_bounds(r, c, info["mask_row0"], info["mask_rows"], opts.strip_height or 1,
                                     opts.strip_rank if opts.strip_world > 1 else 0, max(opts.strip_world, 1))
                      for r in range(info["tile_rows"]) for c in range(info["cols"])]
            frame = si.Frame(scene.desc, cam, opts, debug_cull)
            pm, sm, node, claim = frame.classify_tiles(bounds)
            host = ((claim & 1) != 0).reshape(info["tile_rows"], info["cols"])
            dev = (m[..., 2] & 8) != 0
            assert not np.any(m[..., 2] & ~np.uint32(15)) and not np.any(m[..., 3])
            # a claimed tile keeps its sphere and the ground in word 0 and is no ground tile
            assert not np.any(dev & ((m[..., 2] & 7) != 0))
            claimed += int(dev.sum())
            differ += int((dev != host).sum())
        if case["batch"]:
            import torch
            buf = torch.zeros((len(cams), ctx.localRows(opts), opts.width, 3), dtype=torch.float32, device="cuda")
            ctx.renderFramesDevice(cams, opts, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = list(buf.cpu().numpy())
        elif case["rgb32"]:
            got = [ctx.renderFrameRGB32(cams[0], opts)]
        else:
            got = [ctx.renderFrame(cams[0], opts)]
        for i, f in enumerate(got):
            arrays["frame_%d_%d" % (rank, i)] = f
            if with_oracle:
                ref = orc.render_frame(scene.desc, cams[i], opts, 0)
                if case["rgb32"]:
                    ref = np.array([orc.lib().orc_color_to_rgb32((C.c_float * 3)(*px)) for px in ref.reshape(-1, 3)],
                                   dtype=np.uint32).reshape(ref.shape[:2])
                arrays["ref_%d_%d" % (rank, i)] = ref
    np.savez(os.path.join(outdir, name + ".npz"), **arrays)
    print(json.dumps(dict(name=name, claimed=claimed, differ=differ, redos=int(ctx.exactRedos() - redos0),
                          bails=int(ctx.sphereBails() - bails0), frames=sorted(k for k in arrays if k.startswith("frame")))), flush=True)
print("ok")
'''


def _write_scenes(base):
    for f in ("floor.bmp", "world.bmp"):
        shutil.copy(os.path.join(SCENES, f), str(base / f))
    for case in CASES:
        (base / (case["name"] + ".sdl")).write_text(case["text"] or BALL.replace("power  800000", "power  0"))
    (base / "cases.json").write_text(json.dumps([{k: v for k, v in c.items() if k != "text"} for c in CASES]))


def _run_child(base, sub, env_extra, with_oracle):
    outdir = str(base / sub)
    os.makedirs(outdir)
    env = dict(os.environ, C2RT_LIB_VARIANT="diag", **env_extra)
    p = subprocess.run([sys.executable, "-c", _CHILD, outdir, "1" if with_oracle else "0", str(base / "cases.json")], capture_output=True,
                       text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout[-4000:] + p.stderr[-4000:]
    return {r["name"]: r for r in (json.loads(line) for line in p.stdout.splitlines() if line.startswith("{"))}, p.stderr


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    """every case with the path (and the oracle's frames), then with C2RT_DEBUG_CULL=128: two child processes in all"""
    base = tmp_path_factory.mktemp("sphere_tiles")
    _write_scenes(base)
    on, err_on = _run_child(base, "on", dict(C2RT_DEBUG_CULL="256"), True)
    assert "C2RT_DEBUG_CULL=256" in err_on
    off, err = _run_child(base, "off", dict(C2RT_DEBUG_CULL="128"), False)
    assert "C2RT_DEBUG_CULL=128" in err  # the hook announces itself, as for the other bits
    assert set(on) == set(off) == {c["name"] for c in CASES}
    return base, on, off


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_sphere_tiles_on_the_device(rendered, case):
    base, on, off = rendered
    name = case["name"]
    r_on, r_off = on[name], off[name]
    print("%s: %d claimed tiles (switch off: %d), %d differ from the host, bails %d, redos %d / %d" %
          (name, r_on["claimed"], r_off["claimed"], r_on["differ"], r_on["bails"], r_on["redos"], r_off["redos"]))
    # the device's bit 3 is the host classifier's claim, tile for tile; none with the switch off; not vacuous
    assert r_on["differ"] == 0 and r_off["differ"] == 0 and r_off["claimed"] == 0
    assert r_on["claimed"] >= case["min_claimed"], "vacuous: the frame has no sphere-interior tiles for the path to render"
    assert r_on["bails"] == 0 and r_off["bails"] == 0
    if case["redos"]:
        assert r_on["redos"] >= r_on["claimed"] and r_on["redos"] == r_off["redos"]
    else:
        assert r_on["redos"] == r_off["redos"] == 0
    a, b = np.load(str(base / "on" / (name + ".npz"))), np.load(str(base / "off" / (name + ".npz")))
    assert r_on["frames"] == r_off["frames"] and r_on["frames"]
    for key in r_on["frames"]:
        fa, fb, ref = a[key], b[key], a["ref" + key[len("frame"):]]
        assert fa.shape == fb.shape == ref.shape and fa.dtype == ref.dtype and np.any(fa)
        nne_off = int((fa.view(np.uint32) != fb.view(np.uint32)).sum())
        nne_ref = int((fa != ref).sum())
        print("  %s: %d values differ from the frame without the path, %d from the oracle's" % (key, nne_off, nne_ref))
        assert nne_off == 0, (name, key, nne_off)
        assert (fa.dtype != np.float32 or not np.isnan(fa).any()) and nne_ref == 0, (name, key, nne_ref)
