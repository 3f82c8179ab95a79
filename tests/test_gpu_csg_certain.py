"""Leaf CsgOps decided by csg_certain.h on the device (c2rt_trace.inc: csg_intersect_leaf).

Every case is rendered in two child processes on the diagnostics library: as shipped, and with C2RT_DEBUG_CULL=512, which
clears the planner's kCsgCertain flags so that every CsgOp takes the literal evaluation.  Per case the production frame
must equal, bit for bit, the frame with the route switched off and the counted frame (the counted instances keep the
literal code), and, float for float, the oracle's frame.

The scenes are lecture5.sdl with its CsgOp rewritten in the descriptor: the three operators over (Cube, Sphere), (Sphere,
Cube), (Sphere, Sphere), (Cube, Cube); the eye inside the sphere child, inside the cube, inside both; the sphere child
dipping below the floor (lecture5's own tree); the node translated, and rotated and scaled (the non-identity instance);
two cubes that share a face plane; two lights; a two-rank strip pair; RGB32; a two-camera batch.  Frames are 61x47 and
160x96 with 1 and 5 taps.

Three ineligible trees ride along — a Plane child, Op(a, a), a nested child — with the same three comparisons.

The lane counter: every case is rendered twice more on chess2rt_amd/libc2rt_lanestats.so (`make all`: the diagnostics library
with the depth-1 frame unit's lane statistics compiled in), as shipped and with C2RT_DEBUG_CULL=512.  The counter of
csg_certain.h's decisions must show certain lanes in every case with an eligible tree, and neither certain nor unsure lanes
in the ineligible cases and in every case with the switch set: the comparisons above are not vacuous."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

CUBE = [-100.0, 60.0, 200.0, 100.0]
SPHERE = [-100.0, 60.0, 200.0, 70.0]
PAIRS = {"cs": ([0] + CUBE, [1] + SPHERE), "sc": ([1] + SPHERE, [0] + CUBE),
         "ss": ([1, -100.0, 60.0, 200.0, 60.0], [1, -60.0, 80.0, 170.0, 50.0]),
         "cc": ([0] + CUBE, [0, -60.0, 90.0, 160.0, 90.0])}
SIZES = [((61, 47), 1), ((160, 96), 5), ((61, 47), 5), ((160, 96), 1)]


def _case(name, **kw):
    c = dict(name=name, op=5, pair="cs", size=[61, 47], taps=5, eye=None, translate=None, rotate=None, light2=False, ranks=1, rgb32=False,
             batch=False, children=None, inel=None)
    c.update(kw)
    return c


CASES = [_case("lecture5_%dx%d_x%d" % (s[0], s[1], t), size=list(s), taps=t) for s, t in SIZES]
for i, (op, opname) in enumerate(((3, "union"), (4, "inter"), (5, "diff"))):
    for j, pair in enumerate(sorted(PAIRS)):
        s, t = SIZES[(i + j) % 4]
        CASES.append(_case("%s_%s" % (opname, pair), op=op, pair=pair, size=list(s), taps=t))
CASES += [
    _case("eye_in_sphere_child", eye=[-100.0, 60.0, 140.0], size=[160, 96], taps=1),
    _case("eye_in_cube", eye=[-145.0, 105.0, 245.0]),
    _case("eye_in_both", op=3, eye=[-100.0, 60.0, 200.0], size=[160, 96], taps=5),
    _case("node_translated", translate=[30.0, 5.0, -20.0], size=[160, 96], taps=5),
    _case("node_rotated_scaled", rotate=[25.0, 10.0, 5.0, 1.2, 0.8, 1.1], size=[160, 96], taps=1),
    _case("shared_face_cubes", op=3, children=([0, -100.0, 60.0, 200.0, 100.0], [0, 0.0, 60.0, 200.0, 100.0]), size=[160, 96], taps=5),
    _case("two_lights", light2=True),
    _case("strip_pair", ranks=2, size=[160, 96], taps=1),
    _case("rgb32", rgb32=True),
    _case("two_camera_batch", batch=True, size=[160, 96], taps=5),
    _case("ineligible_plane_child", inel="plane"),
    _case("ineligible_op_a_a", op=4, inel="same", size=[160, 96], taps=1),
    _case("ineligible_nested_child", inel="nested"),
]

_CHILD = r'''
import ctypes as C, json, os, sys
sys.path[:0] = [os.path.join(os.getcwd(), "tests")]
import numpy as np
import chess2rt_amd as c2, oracle_lib as orc
from chess2rt_amd import _abi
outdir, full, stats = sys.argv[1], sys.argv[2] == "1", sys.argv[2] == "2"
if stats:
    import torch
    lib = _abi.load_library()
    lib.c2rt_debug_set_tile_stats.argtypes = [C.c_void_p, C.c_void_p]
    lib.c2rt_debug_set_tile_stats.restype = None
cases = json.load(open(sys.argv[3]))
pairs = json.load(open(sys.argv[4]))
ctx = c2.Context(0)
for case in cases:
    name = case["name"]
    W, H = case["size"]
    text = open(os.path.join("tests", "golden", "scenes", "lecture5.sdl")).read()
    if case["light2"]:
        i = text.index("PointLight")
        j = text.index("}", i) + 1
        text = text[:j] + "\n    " + text[i:j].replace("light1", "light2").replace("-90 700 350", "150 500 100") + text[j:]
    path = os.path.join(outdir, name + ".sdl")
    open(path, "w").write(text)
    for f in ("floor.bmp", "world.bmp"):
        if not os.path.exists(os.path.join(outdir, f)):
            open(os.path.join(outdir, f), "wb").write(open(os.path.join("tests", "golden", "scenes", f), "rb").read())
    scene = c2.parseSceneFromFile(path)
    scene.setFrameSize(W, H)
    if case["translate"]:
        scene.translateNode("csgNode", case["translate"])
    if case["rotate"]:
        r = case["rotate"]
        scene.rotateNode("csgNode", r[0], r[1], r[2])
        scene.scaleNode("csgNode", r[3], r[4], r[5])
    d = scene.desc.contents
    g = next(d.node_geom[n] for n in range(d.n_nodes) if d.geom_type[d.node_geom[n]] >= _abi.GEOM_CSG_UNION)
    d.geom_type[g] = case["op"]
    kids = case["children"] or pairs[case["pair"]]
    for c, k in zip((d.geom_child[2 * g], d.geom_child[2 * g + 1]), kids):
        d.geom_type[c] = _abi.GEOM_SPHERE if k[0] else _abi.GEOM_CUBE
        for i in range(4):
            d.geom_param[4 * c + i] = k[1 + i]
    l, r = d.geom_child[2 * g], d.geom_child[2 * g + 1]
    if case["inel"] == "plane":
        d.geom_type[r] = _abi.GEOM_PLANE
        for i, v in enumerate((60.0, float("nan"), 0.0, 0.0)):
            d.geom_param[4 * r + i] = v
    elif case["inel"] == "same":
        d.geom_child[2 * g + 1] = l
    elif case["inel"] == "nested":
        others = [k for k in range(d.n_geoms) if k not in (g, l, r) and d.geom_type[k] in (_abi.GEOM_SPHERE, _abi.GEOM_CUBE)]
        d.geom_type[r] = _abi.GEOM_CSG_UNION
        d.geom_child[2 * r], d.geom_child[2 * r + 1] = others[0], others[1]
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
    ctx.uploadScene(scene.desc)
    if stats:
        # {cycles, class} per tile, four lane counters, 9 regions x 3, then csg_certain.h's {certain, unsure} lanes (uint64 each)
        opts = scene.renderOpts(taps=case["taps"])
        tiles = ((W + 7) // 8) * ((ctx.localRows(opts) + 7) // 8)
        buf = torch.zeros((tiles + 4 + 27 + 2, 2), dtype=torch.int32, device="cuda:0")
        lib.c2rt_debug_set_tile_stats(ctx.handle, C.c_void_p(buf.data_ptr()))
        frame = ctx.renderFrame(cams[0], opts)
        torch.cuda.synchronize()
        lib.c2rt_debug_set_tile_stats(ctx.handle, None)
        lane = buf.cpu().numpy()[tiles:].view(np.uint64).ravel()
        print(json.dumps(dict(name=name, certain=int(lane[31]), unsure=int(lane[32]), entered=int(lane[0]), lit=bool(np.any(frame)))), flush=True)
        continue
    arrays = {}
    redos0 = ctx.exactRedos()
    for rank in range(case["ranks"]):
        kw = dict(taps=case["taps"])
        if case["ranks"] > 1:
            kw.update(strip_height=8, strip_rank=rank, strip_world=case["ranks"])
        opts = scene.renderOpts(**kw)
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
            if full:
                if not case["rgb32"]:
                    arrays["counted_%d_%d" % (rank, i)] = ctx.renderFrame(cams[i], scene.renderOpts(count_rays=1, **kw))
                ref = orc.render_frame(scene.desc, cams[i], opts, 0)
                if case["rgb32"]:
                    ref = np.array([orc.lib().orc_color_to_rgb32((C.c_float * 3)(*px)) for px in ref.reshape(-1, 3)],
                                   dtype=np.uint32).reshape(ref.shape[:2])
                arrays["ref_%d_%d" % (rank, i)] = ref
    np.savez(os.path.join(outdir, name + ".npz"), **arrays)
    print(json.dumps(dict(name=name, redos=int(ctx.exactRedos() - redos0), frames=sorted(k for k in arrays if k.startswith("frame")))), flush=True)
print("ok")
'''


def _run_child(base, sub, env_extra, full, variant="diag"):
    outdir = str(base / sub)
    os.makedirs(outdir)
    env = dict(os.environ, C2RT_LIB_VARIANT=variant, **env_extra)
    mode = "2" if variant == "lanestats" else ("1" if full else "0")
    p = subprocess.run([sys.executable, "-c", _CHILD, outdir, mode, str(base / "cases.json"), str(base / "pairs.json")],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), p.stdout[-4000:] + p.stderr[-4000:]
    return {r["name"]: r for r in (json.loads(line) for line in p.stdout.splitlines() if line.startswith("{"))}, p.stderr


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    """every case as shipped (with the counted and the oracle's frames), then with the route off: two child processes in all"""
    base = tmp_path_factory.mktemp("csg_certain")
    (base / "cases.json").write_text(json.dumps(CASES))
    (base / "pairs.json").write_text(json.dumps(PAIRS))
    on, err_on = _run_child(base, "on", {}, True)
    off, err = _run_child(base, "off", dict(C2RT_DEBUG_CULL="512"), False)
    assert "C2RT_DEBUG_CULL=512" in err and "C2RT_DEBUG_CULL" not in err_on
    assert set(on) == set(off) == {c["name"] for c in CASES}
    return base, on, off


@pytest.fixture(scope="module")
def counted_lanes(tmp_path_factory):
    """every case on the lane-statistics library, as shipped and with the route switched off"""
    assert os.path.exists(os.path.join(ROOT, "chess2rt_amd", "libc2rt_lanestats.so")), "run `make all` (build())"
    base = tmp_path_factory.mktemp("csg_certain_lanes")
    (base / "cases.json").write_text(json.dumps(CASES))
    (base / "pairs.json").write_text(json.dumps(PAIRS))
    on, _ = _run_child(base, "on", {}, False, "lanestats")
    off, err = _run_child(base, "off", dict(C2RT_DEBUG_CULL="512"), False, "lanestats")
    assert "C2RT_DEBUG_CULL=512" in err
    assert set(on) == set(off) == {c["name"] for c in CASES}
    return on, off


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_lane_counter(counted_lanes, case):
    on, off = counted_lanes
    a, b = on[case["name"]], off[case["name"]]
    print("%s: %d certain, %d unsure lanes of %d entered; switched off: %d, %d" % (case["name"], a["certain"], a["unsure"], a["entered"],
                                                                                 b["certain"], b["unsure"]))
    assert a["lit"] and b["lit"]
    assert b["certain"] == 0 and b["unsure"] == 0, "C2RT_DEBUG_CULL=512 left the route on"
    if case["inel"]:
        assert a["certain"] == 0 and a["unsure"] == 0, "an ineligible tree was offered to csg_certain.h"
        if case["inel"] != "nested":
            assert a["entered"] > 0          # (a depth-1 tree: the counting unit did run it)
    else:
        assert a["certain"] > 0, "no lane was decided by csg_certain.h"
        assert a["entered"] > 0


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_certain_route_on_the_device(rendered, case):
    base, on, off = rendered
    name = case["name"]
    assert on[name]["redos"] == off[name]["redos"] == 0
    a, b = np.load(str(base / "on" / (name + ".npz"))), np.load(str(base / "off" / (name + ".npz")))
    assert on[name]["frames"] == off[name]["frames"] and on[name]["frames"]
    for key in on[name]["frames"]:
        fa, fb, ref = a[key], b[key], a["ref" + key[len("frame"):]]
        assert fa.shape == fb.shape == ref.shape and fa.dtype == ref.dtype and np.any(fa)
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), "differs from the frame with the route switched off"
        if not case["rgb32"]:
            cnt = a["counted" + key[len("frame"):]]
            assert np.array_equal(fa.view(np.uint32), cnt.view(np.uint32)), "differs from the counted frame"
            assert np.array_equal(fa, ref), "differs from the oracle: max |d| = %g" % float(np.max(np.abs(fa - ref)))
        else:
            assert np.array_equal(fa, ref), "differs from the oracle's RGB32"
