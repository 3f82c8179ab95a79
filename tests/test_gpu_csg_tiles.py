"""Tiles with the ground and one leaf CsgOp node on the device (chess2rt_amd/csrc/c2rt_trace.inc: lean::csg_tile, called
from render_tile on the two mask words it loads anyway; the nodes are the planner's, scene_plan.cpp: plan_csg_tile_nodes).

Same frame, three ways: every case is rendered in child processes on the diagnostics library, as shipped and with
C2RT_DEBUG_CULL=1024 (every tile to the general path).  The frame with the path must equal the frame without it and the
counted frame (exact::, the general path) bit for bit, and the oracle's frame float for float; c2rt_get_csg_tile_bails
must not move, and c2rt_get_exact_redos must move by the same amount both ways (0 except in the two redo cases).

The path was taken: every case is rendered twice more on chess2rt_amd/libc2rt_lanestats.so, which keeps the path and
counts the tiles it rendered (c2rt_get_csg_tiles).  The count must equal the number of tiles whose two mask words — read
back from the device's own table — meet render_tile's condition for a node the host's planner marked
(scripts/csg_tile_census.py: claim_from_masks over tests/libcsg_tile_check.so): more than 0 in every eligible case, 0 in
every ineligible one and in every case with bit 10 set.

The scenes are tests/csg_tile_scenes.py's: lecture5.sdl as shipped; the three operators, cube / sphere in both orders, two
spheres, two cubes that share a face plane; the eye inside the cube; the node translated; a low light (the CsgOp's long
shadow on the floor inside its own tiles, and on itself); a Lambert CsgOp; the floor with a bitmap, a checker and a plain
colour; the light switched off and a light below the floor (the shadow ray's plane test runs); the CsgOp node in front of
the floor in file order (the tie rule); an interleaved strip pair and a two-camera batch; the eye on the cube's top face
plane (a zero numerator: tiles leave the path for exact::) and the scene at 1e80 (beyond csg_certain.h's domain, so the
planner marks nothing, and every tile is rendered again through exact::).  Ineligible, with the same comparisons: no light
at all, two lights, a rotated node, a textured CsgOp node, a Plane child, a nested CsgOp.  Frames are 64x48 and 160x96 at
1 and 5 taps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import csg_tile_scenes as S  # noqa: E402

SIZES = [((64, 48), 5), ((160, 96), 1), ((160, 96), 5), ((64, 48), 1)]


def _case(name, k=0, edit=None, eligible=True, redo=False, **kw):
    size, taps = SIZES[k % 4]
    c = dict(name=name, edit=edit, size=list(size), taps=taps, eligible=eligible, redo=redo, eye=None, ranks=1, batch=False, scale=1.0)
    c.update(kw)
    return c


CASES = [_case("lecture5_%dx%d_x%d" % (s[0], s[1], t), k) for k, (s, t) in enumerate(SIZES)]
CASES += [
    _case("union_cs", 0, op=3), _case("inter_cs", 1, op=4), _case("union_sc", 2, op=3, pair="sc"), _case("inter_sc", 3, op=4, pair="sc"),
    _case("diff_sc", 0, pair="sc"), _case("diff_ss", 1, pair="ss"), _case("union_ss", 2, op=3, pair="ss"),
    _case("union_shared_face_cubes", 2, op=3, pair="cc_shared_face"), _case("diff_shared_face_cubes", 1, pair="cc_shared_face"),
    _case("eye_in_cube", 0, eye=[-145.0, 105.0, 155.0]),  # (in the cube's near corner, outside the sphere child: inside the solid)
    _case("node_translated", 2, translate=[30.0, 5.0, -20.0]),
    _case("low_light_shadows", 2, "light_low"), _case("low_light_union", 1, "light_low", op=3),
    _case("lambert_csgop", 0, "lambert"), _case("floor_checker", 2, "checker"), _case("floor_plain", 1, "plain"),
    _case("light_off", 0, "power_0"), _case("light_below_floor", 2, "light_below"),
    _case("csgop_before_floor", 2, "csg_first"), _case("csgop_before_floor_union", 3, "csg_first", op=3),
    _case("strip_pair", 2, ranks=2), _case("two_camera_batch", 2, batch=True),
    _case("eye_on_face_plane", 2, eye=[0.0, 110.0, 0.0], redo=True),
    _case("scene_1e80", 0, "power_0", scale=1e80, eligible=False, redo=True),
    _case("no_light", 0, no_light=True, eligible=False), _case("two_lights", 0, "two_lights", eligible=False),
    _case("node_rotated", 1, rotate=[25.0, 10.0, 5.0], eligible=False), _case("textured_csgop", 0, "csg_textured", eligible=False),
    _case("plane_child", 0, inel="plane", eligible=False), _case("nested_csgop", 0, inel="nested", eligible=False),
]

_CHILD = r'''
import ctypes as C, json, os, sys
sys.path[:0] = [os.path.join(os.getcwd(), "tests"), os.path.join(os.getcwd(), "scripts")]
import numpy as np
import chess2rt_amd as c2, csg_tile_scenes as S, csg_tile_census as census, csg_void_device as vdev, oracle_lib as orc
outdir, mode = sys.argv[1], sys.argv[2]   # full: with the counted and the oracle's frames; plain; count: tiles taken
cases = json.load(open(sys.argv[3]))
debug_cull = int(os.environ.get("C2RT_DEBUG_CULL", "0"))
ctx = c2.Context(0)
for case in cases:
    name = case["name"]
    W, H = case["size"]
    path = os.path.join(outdir, name + ".sdl")
    open(path, "w").write(S.text(case["edit"]))
    for f in ("floor.bmp", "world.bmp"):
        if not os.path.exists(os.path.join(outdir, f)):
            open(os.path.join(outdir, f), "wb").write(open(os.path.join(S.SCENES, f), "rb").read())
    scene = c2.parseSceneFromFile(path)
    scene.setFrameSize(W, H)
    S.rewrite(scene, case)
    cams = [scene.beginFrame()]
    if case["batch"]:
        scene.rotateCamera(4, 0, 3)
        cams.append(scene.beginFrame())
    if case["eye"]:
        for cam in cams:
            shift = [case["eye"][i] - cam.pos[i] for i in range(3)]
            for f in ("pos", "up_left", "up_right", "down_left"):
                v = getattr(cam, f)
                for i in range(3):
                    v[i] += shift[i]
    if case["scale"] != 1.0:   # the same picture at 1e80: the description and the camera frames scaled
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
    d = scene.desc.contents
    arrays, host = {}, 0
    redos0, bails0, taken0 = ctx.exactRedos(), ctx.csgTileBails(), ctx.csgTiles()
    for rank in range(case["ranks"]):
        kw = dict(taps=case["taps"])
        if case["ranks"] > 1:
            kw.update(strip_height=8, strip_rank=rank, strip_world=case["ranks"])
        opts = scene.renderOpts(**kw)
        if mode == "count":
            # the host's count from the device's own mask words
            for cam in cams:
                eligible, ground, _ = census.eligible_nodes(scene.desc, cam, opts, debug_cull)
                got = vdev.read_tile_masks(ctx, cam, opts, 3)
                if got is not None:
                    m = got[0]
                    host += int((census.claim_from_masks(m[..., 0], m[..., 1], d.n_nodes, ground, eligible) >= 0).sum())
        if case["batch"]:
            import torch
            buf = torch.zeros((len(cams), ctx.localRows(opts), opts.width, 3), dtype=torch.float32, device="cuda")
            ctx.renderFramesDevice(cams, opts, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = list(buf.cpu().numpy())
        else:
            got = [ctx.renderFrame(cams[0], opts)]
        for i, f in enumerate(got):
            arrays["frame_%d_%d" % (rank, i)] = f
            if mode == "full":
                arrays["counted_%d_%d" % (rank, i)] = ctx.renderFrame(cams[i], scene.renderOpts(count_rays=1, **kw))
                arrays["ref_%d_%d" % (rank, i)] = orc.render_frame(scene.desc, cams[i], opts, 0)
    out = dict(name=name, redos=int(ctx.exactRedos() - redos0), bails=int(ctx.csgTileBails() - bails0), taken=int(ctx.csgTiles() - taken0),
               host=host, lit=bool(all(np.any(f) for k, f in arrays.items() if k.startswith("frame"))),
               frames=sorted(k for k in arrays if k.startswith("frame")))
    if mode != "count":
        np.savez(os.path.join(outdir, name + ".npz"), **arrays)
    print(json.dumps(out), flush=True)
print("ok")
'''


def _run_child(base, sub, env_extra, mode, variant="diag"):
    outdir = str(base / sub)
    os.makedirs(outdir)
    env = dict(os.environ, C2RT_LIB_VARIANT=variant, **env_extra)
    p = subprocess.run([sys.executable, "-c", _CHILD, outdir, mode, str(base / "cases.json")], capture_output=True, text=True, timeout=600,
                       env=env, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout[-4000:] + p.stderr[-4000:]
    return {r["name"]: r for r in (json.loads(line) for line in p.stdout.splitlines() if line.startswith("{"))}, p.stderr


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    """every case as shipped (with the counted and the oracle's frames), then with the path off: two child processes"""
    base = tmp_path_factory.mktemp("csg_tiles")
    (base / "cases.json").write_text(json.dumps(CASES))
    on, err_on = _run_child(base, "on", {}, "full")
    off, err = _run_child(base, "off", dict(C2RT_DEBUG_CULL="1024"), "plain")
    assert "C2RT_DEBUG_CULL=1024" in err and "C2RT_DEBUG_CULL" not in err_on
    assert set(on) == set(off) == {c["name"] for c in CASES}
    return base, on, off


@pytest.fixture(scope="module")
def counted_tiles(tmp_path_factory):
    """every case on the lane-statistics library, as shipped and with the path off"""
    assert os.path.exists(os.path.join(ROOT, "chess2rt_amd", "libc2rt_lanestats.so")), "run `make all` (build())"
    base = tmp_path_factory.mktemp("csg_tiles_taken")
    (base / "cases.json").write_text(json.dumps(CASES))
    on, _ = _run_child(base, "on", {}, "count", "lanestats")
    off, err = _run_child(base, "off", dict(C2RT_DEBUG_CULL="1024"), "count", "lanestats")
    assert "C2RT_DEBUG_CULL=1024" in err
    assert set(on) == set(off) == {c["name"] for c in CASES}
    return on, off


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_path_was_taken(counted_tiles, case):
    on, off = counted_tiles
    a, b = on[case["name"]], off[case["name"]]
    print("%s: csg_tile rendered %d tiles, the mask words claim %d; switched off: %d, %d; bails %d; redos %d / %d" %
          (case["name"], a["taken"], a["host"], b["taken"], b["host"], a["bails"], a["redos"], b["redos"]))
    assert a["lit"] and b["lit"]
    assert b["taken"] == 0 and b["host"] == 0, "C2RT_DEBUG_CULL=1024 left the path on"
    assert a["bails"] == 0 and b["bails"] == 0
    if not case["eligible"]:
        assert a["taken"] == 0 and a["host"] == 0, "an ineligible frame reached csg_tile"
    elif case["redo"]:
        # a tile that leaves the path for exact:: is not counted as rendered by it
        assert a["host"] > 0 and a["taken"] <= a["host"] and a["redos"] >= a["host"] - a["taken"] > 0
    else:
        assert a["taken"] == a["host"] > 0
    assert a["redos"] == b["redos"] and (a["redos"] > 0) == case["redo"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_same_frame_three_ways(rendered, case):
    base, on, off = rendered
    name = case["name"]
    assert on[name]["bails"] == off[name]["bails"] == 0
    assert on[name]["redos"] == off[name]["redos"] and (on[name]["redos"] > 0) == case["redo"]
    a, b = np.load(str(base / "on" / (name + ".npz"))), np.load(str(base / "off" / (name + ".npz")))
    assert on[name]["frames"] == off[name]["frames"] and on[name]["frames"]
    for key in on[name]["frames"]:
        fa, fb, cnt, ref = a[key], b[key], a["counted" + key[len("frame"):]], a["ref" + key[len("frame"):]]
        assert fa.shape == fb.shape == cnt.shape == ref.shape and fa.dtype == ref.dtype and np.any(fa)
        n_off = int((fa.view(np.uint32) != fb.view(np.uint32)).sum())
        n_cnt = int((fa.view(np.uint32) != cnt.view(np.uint32)).sum())
        n_ref = int((fa != ref).sum())
        print("  %s %s: %d values differ from the frame without the path, %d from the counted frame, %d from the oracle's" %
              (name, key, n_off, n_cnt, n_ref))
        assert n_off == 0, "differs from the frame with C2RT_DEBUG_CULL=1024"
        assert n_cnt == 0, "differs from the counted frame"
        assert not np.isnan(fa).any() and n_ref == 0, "differs from the oracle: max |d| = %g" % float(np.max(np.abs(fa - ref)))
