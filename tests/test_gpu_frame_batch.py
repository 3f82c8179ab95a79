"""c2rt_render_frames / c2rt_render_frames_device: a batch of camera frames of one scene with one mask pre-pass
launch and one frame launch (two for nested CSG).  The contract is equality: frame i of a batch holds exactly the
bits c2rt_render_frame_device(ctx, &cams[i], opts, ...) writes, so every case compares uint32 views of the batch
with single-frame renders of the same cameras (and, where stated, with the oracle).  Shapes are the smallest that
reach the mechanism: partial tiles on both axes, more than one group of eight tile rows, several frames."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import chess2rt_amd as c2
import oracle_lib as orc
import scene_fuzz
from chess2rt_amd import _abi
from golden_configs import SCENES
from parity_util import TOL, maxdiff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BATCH = 256  # C2RT_MAX_BATCH_FRAMES, include/c2rt.h


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _walk(scene, steps):
    """one CameraFrame per (rotate, move) step, as the GUI loop makes them (rotate -> beginFrame -> move -> beginFrame)"""
    cams = []
    for rot, mov in steps:
        scene.rotateCamera(*rot)
        scene.beginFrame()
        scene.moveCamera(*mov)
        cams.append(scene.beginFrame())
    return cams


def _orbit(scene, n, yaw=7.0):
    return _walk(scene, [((0, 0, 0), (0, 0, 0))] + [((yaw, 0, 0), (0, 0, 0))] * (n - 1))


def _singles(ctx, cams, opts):
    return np.stack([ctx.renderFrame(cam, opts) for cam in cams])


def _check_batch_equals_singles(ctx, cams, opts, what):
    batch = ctx.renderFrames(cams, opts)
    singles = _singles(ctx, cams, opts)
    assert batch.shape == singles.shape == (len(cams), ctx.localRows(opts), opts.width, 3), what
    for i in range(len(cams)):
        assert np.array_equal(_bits(batch[i]), _bits(singles[i])), "%s: frame %d of the batch differs from the single frame" % (what, i)
    return batch


# lecture5: the file's camera; turned towards the CSG object and walked to its box; INTO the box (box corners behind
# the eye: whole-frame rectangles, the node is kept in every tile); straight down (pitch clamps at -90); high above
LECTURE5_STEPS = [
    ((0, 0, 0), (0, 0, 0)),
    ((-25, 0, 0), (0, 0, 100)),
    ((0, 0, 0), (0, 0, 120)),
    ((0, 0, -100), (0, 0, 0)),
    ((0, 0, 45), (0, 300, 0)),
]


def test_headline_instance_with_mixed_cameras_equals_singles_and_oracle(gpu_ctx):
    """lecture5.sdl at 72x100 with five taps: 9 tile columns (the last one partial), 13 tile rows (the last one
    partial) = two groups of eight tile rows, so frames whose boxed nodes begin below row 64 carry a non-zero
    row_group_start while others do not.  Five cameras of a move / rotate walk, one with the eye inside the CSG
    object's box and one looking straight down.  (RenderParams::n_cull is a property of the scene in this library —
    fill_params — so no camera of lecture5 has n_cull == 0; a box corner behind the eye gives that node a whole-frame
    rectangle instead.  The diagnostics check of that is test_corner_behind_the_eye_keeps_the_node_in_every_tile.)"""
    scene = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    scene.setFrameSize(72, 100)
    scene.setAA(True)
    cams = _walk(scene, LECTURE5_STEPS)
    opts = scene.renderOpts()
    assert opts.taps == 5
    gpu_ctx.uploadScene(scene.desc)
    batch = _check_batch_equals_singles(gpu_ctx, cams, opts, "lecture5 72x100 x5")
    assert len({_bits(f).tobytes() for f in batch}) == len(cams)  # five different frames, not one five times
    for i, cam in enumerate(cams):
        ref = orc.render_frame(scene.desc, cam, opts, 0)
        md, nbad, nne = maxdiff(batch[i], ref)
        print("lecture5 camera %d: max|d|=%.3g, >1e-4: %d, differing floats: %d of %d" % (i, md, nbad, nne, ref.size))
        assert md <= TOL and nbad == 0, i


def _fuzz_scene(tmp_path, text, name):
    shutil.copy(os.path.join(SCENES, "floor.bmp"), str(tmp_path / "floor.bmp"))
    p = tmp_path / name
    p.write_text(text)
    return c2.parseSceneFromFile(str(p))


def _general_matrix_seed():
    """the first fuzz seed with one light and a scaled node: the general (non-identity, single-light) instances"""
    for seed in range(200):
        text = scene_fuzz.random_scene_sdl(seed)
        if text.count("PointLight") == 1 and "; scale " in text:
            return seed, text
    raise AssertionError("no such seed")


@pytest.mark.parametrize("which", ["zaphod", "lecture4", "many_lights", "general_matrix", "csg_stress"])
def test_other_instances_equal_singles(gpu_ctx, tmp_path, which):
    """64x48, three cameras: the planes instance (zaphod.sdl with depth of field off, lecture4.sdl), the multi-light
    instances, the general-matrix instances and the nested-CSG instances (csg_stress.sdl)."""
    if which in ("zaphod", "lecture4", "csg_stress"):
        scene = c2.parseSceneFromFile(os.path.join(SCENES, which + ".sdl"))
        scene.setDof(False)
    elif which == "many_lights":
        scene = _fuzz_scene(tmp_path, scene_fuzz.many_lights_scene_sdl(3), "ml.sdl")
        assert scene.desc.contents.n_lights > 1
    else:
        seed, text = _general_matrix_seed()
        scene = _fuzz_scene(tmp_path, text, "gm.sdl")
        assert scene.desc.contents.n_lights == 1
    scene.setFrameSize(64, 48)
    scene.setAA(False)
    cams = _orbit(scene, 3)
    assert all(cam.dof == 0 and cam.stereo_separation == 0 for cam in cams)
    opts = scene.renderOpts()
    gpu_ctx.uploadScene(scene.desc)
    batch = _check_batch_equals_singles(gpu_ctx, cams, opts, which)
    ref = orc.render_frame(scene.desc, cams[1], opts, 0)
    md, nbad, nne = maxdiff(batch[1], ref)
    print("%s: max|d|=%.3g, differing floats: %d" % (which, md, nne))
    assert md <= TOL and nbad == 0


_DIAG_CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import chess2rt_amd as c2, oracle_lib as orc
from golden_configs import SCENES
ctx = c2.Context(0)
for name, size in (("csg_stress", (96, 64)), ("csg_corner", (64, 48))):
    scene = c2.parseSceneFromFile(os.path.join(SCENES, name + ".sdl"))
    scene.setFrameSize(*size)
    scene.setAA(False)
    cams = [scene.beginFrame()]
    for _ in range(2):
        scene.rotateCamera(6, 0, 0)
        cams.append(scene.beginFrame())
    opts = scene.renderOpts()
    ctx.uploadScene(scene.desc)
    batch = ctx.renderFrames(cams, opts)
    for i, cam in enumerate(cams):
        ref = orc.render_frame(scene.desc, cam, opts, 0)
        one = ctx.renderFrame(cam, opts)
        assert np.array_equal(batch[i].view(np.uint32), one.view(np.uint32)), (name, i, "single")
        assert np.array_equal(batch[i].view(np.uint32), ref.view(np.uint32)), (name, i, "oracle", int((batch[i] != ref).sum()))
print("ok")
'''


@pytest.mark.parametrize("cap", [3])
def test_nested_csg_overflow_is_redone_per_frame(cap):
    """C2RT_CSG_FIRST_CAP (diagnostics build) shrinks the first pass's hit stacks, so most CSG tiles of every frame of
    the batch overflow and are redone by the (2048, n_frames) retry launch, each frame from its own list."""
    env = dict(os.environ, C2RT_CSG_FIRST_CAP=str(cap), C2RT_LIB_VARIANT="diag")
    p = subprocess.run([sys.executable, "-c", _DIAG_CHILD], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr


_MASKS_CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import chess2rt_amd as c2
import csg_void_device as dev
from golden_configs import SCENES
ctx = c2.Context(0)
scene = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
scene.setFrameSize(72, 100)
steps = %r
cams = []
for rot, mov in steps:
    scene.rotateCamera(*rot); scene.beginFrame(); scene.moveCamera(*mov); cams.append(scene.beginFrame())
opts = scene.renderOpts()
ctx.uploadScene(scene.desc)
kept_everywhere = []
for cam in cams:
    table, info, vc = dev.read_tile_masks(ctx, cam, opts, 3)
    pm = table[:, :, 0]
    kept_everywhere.append([n for n in range(scene.desc.contents.n_nodes) if ((pm >> np.uint32(n)) & 1).all()])
print("nodes kept in every tile, per camera:", kept_everywhere)
extra = set(kept_everywhere[2]) - set(kept_everywhere[0])
assert extra, "the camera inside the box keeps no node that the file's camera culls somewhere"
print("ok")
''' % (LECTURE5_STEPS,)


def test_corner_behind_the_eye_keeps_the_node_in_every_tile():
    """The walk of the headline test through c2rt_debug_tile_masks (diagnostics build): with the eye inside the CSG
    object's box a corner of that box lies behind the eye, the node's rectangle is the whole frame and its bit stays
    set in every tile's primary mask — which the file's camera clears in some tiles.  That is the 'no culling for
    this node' frame the batch mixes with culled ones."""
    env = dict(os.environ, C2RT_LIB_VARIANT="diag")
    p = subprocess.run([sys.executable, "-c", _MASKS_CHILD], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    print(p.stdout)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr


EYE_ON_FACE_PLANE = '''Scene { Camera { pos 0 1 -5; fov 60 }
    Lights { PointLight "k" { pos 3 10 -4; color 1 1 1; power 300 } }
    Geometries { Cube "c" { center 0 0.5 0; side 1 }; Sphere "s" { center 0 0.5 0; R 0.6 }; CsgDiff "d" { left "c"; right "s" }; Plane "p" { y 0 } }
    Shaders { Phong "l" { color 0.9 0.4 0.1 }; Lambert "f" { } }
    Nodes { Node "n" { geometry "d"; shader "l" }; Node "g" { geometry "p"; shader "f" } } }'''


def test_exact_redo_inside_a_batch(gpu_ctx, tmp_path):
    """Three cameras, the middle one with its eye exactly on the plane of a cube face (a zero numerator in every ray
    that reaches the face test: those tiles leave the lean windows and are rendered again through the exact path).
    The batch equals the singles and c2rt_get_exact_redos grows by the same amount."""
    p = tmp_path / "face.sdl"
    p.write_text(EYE_ON_FACE_PLANE)
    scene = c2.parseSceneFromFile(str(p))
    scene.setFrameSize(72, 52)
    scene.setAA(False)
    on_plane = scene.beginFrame()
    assert on_plane.pos[1] == 1.0
    scene.moveCamera(0, 0.75, 0)
    above = scene.beginFrame()
    scene.moveCamera(0.5, 0.5, 0.25)
    aside = scene.beginFrame()
    assert above.pos[1] != 1.0 and aside.pos[1] != 1.0
    cams = [above, on_plane, aside]
    opts = scene.renderOpts()
    gpu_ctx.uploadScene(scene.desc)
    r0 = gpu_ctx.exactRedos()
    singles = _singles(gpu_ctx, cams, opts)
    r1 = gpu_ctx.exactRedos()
    batch = gpu_ctx.renderFrames(cams, opts)
    r2 = gpu_ctx.exactRedos()
    print("tiles redone: singles %d, batch %d" % (r1 - r0, r2 - r1))
    assert r1 - r0 > 0 and r2 - r1 == r1 - r0
    assert np.array_equal(_bits(batch), _bits(singles))


def test_strips(gpu_ctx):
    """strip_world = 2, strip_rank = 1, strip_height = 8 on lecture5 72x100: rank 1 owns 48 rows of every frame."""
    scene = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    scene.setFrameSize(72, 100)
    scene.setAA(False)
    cams = _walk(scene, LECTURE5_STEPS[:3])
    opts = scene.renderOpts(strip_world=2, strip_rank=1, strip_height=8)
    gpu_ctx.uploadScene(scene.desc)
    assert gpu_ctx.localRows(opts) == 48
    batch = _check_batch_equals_singles(gpu_ctx, cams, opts, "strips")
    full = gpu_ctx.renderFrame(cams[1], scene.renderOpts())
    rows = [y for y in range(100) if (y // 8) % 2 == 1]
    assert np.array_equal(_bits(batch[1]), _bits(full[rows]))


def test_ordering_without_syncs(gpu_ctx):
    """Batch A, batch B and a single frame enqueued on one stream with nothing in between share the stream's scratch
    slot (mask tables, device table) and stay ordered; then the two batches on two streams (two slots)."""
    import torch

    scene = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    scene.setFrameSize(72, 100)
    scene.setAA(False)
    cams = _orbit(scene, 9, yaw=11.0)
    cams_a, cams_b, cam_c = cams[:4], cams[4:8], cams[8]
    opts = scene.renderOpts()
    gpu_ctx.uploadScene(scene.desc)
    want_a, want_b, want_c = _singles(gpu_ctx, cams_a, opts), _singles(gpu_ctx, cams_b, opts), gpu_ctx.renderFrame(cam_c, opts)

    def fresh(n):
        return torch.full((n, 100, 72, 3), -7.0, dtype=torch.float32, device="cuda:0")

    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    buf_a, buf_b, buf_c = fresh(4), fresh(4), fresh(1)
    torch.cuda.synchronize()
    gpu_ctx.renderFramesDevice(cams_a, opts, buf_a.data_ptr(), s1.cuda_stream)
    gpu_ctx.renderFramesDevice(cams_b, opts, buf_b.data_ptr(), s1.cuda_stream)
    gpu_ctx.renderFrameDevice(cam_c, opts, buf_c.data_ptr(), s1.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(buf_a.cpu().numpy()), _bits(want_a))
    assert np.array_equal(_bits(buf_b.cpu().numpy()), _bits(want_b))
    assert np.array_equal(_bits(buf_c.cpu().numpy()[0]), _bits(want_c))

    buf_a, buf_b = fresh(4), fresh(4)
    torch.cuda.synchronize()
    gpu_ctx.renderFramesDevice(cams_a, opts, buf_a.data_ptr(), s1.cuda_stream)
    gpu_ctx.renderFramesDevice(cams_b, opts, buf_b.data_ptr(), s2.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(buf_a.cpu().numpy()), _bits(want_a))
    assert np.array_equal(_bits(buf_b.cpu().numpy()), _bits(want_b))


def _raw_batch(ctx, cams, n, opts, out, stop=None):
    """c2rt_render_frames with an explicit n_frames; returns the status"""
    lib = _abi.load_library()
    arr = (_abi.CameraFrame * max(len(cams), 1))(*cams)
    return lib.c2rt_render_frames(ctx.handle, arr, n, C.byref(opts), out.ctypes.data_as(C.c_void_p),
                                  stop.ctypes.data_as(C.c_void_p) if stop is not None else None)


def test_edges_and_refusals(gpu_ctx):
    import torch

    scene = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))
    scene.setFrameSize(40, 24)
    scene.setAA(False)
    cams = _orbit(scene, 3)
    opts = scene.renderOpts()
    gpu_ctx.uploadScene(scene.desc)
    lib = _abi.load_library()
    singles = _singles(gpu_ctx, cams, opts)

    # one frame == the single frame
    assert np.array_equal(_bits(gpu_ctx.renderFrames(cams[:1], opts)[0]), _bits(singles[0]))

    def sentinel():
        return np.full((3, 24, 40, 3), -3.0, dtype=np.float32)

    def untouched(a):
        return bool((a == -3.0).all())

    # no frames: OK, nothing written
    out = sentinel()
    assert _raw_batch(gpu_ctx, cams, 0, opts, out) == _abi.OK and untouched(out)
    assert gpu_ctx.renderFrames([], opts).shape == (0, 24, 40, 3)

    # refusals, each decided before anything is enqueued
    dof_cam = _abi.CameraFrame.from_buffer_copy(cams[1])
    dof_cam.dof, dof_cam.num_samples = 1, 4
    stereo_cam = _abi.CameraFrame.from_buffer_copy(cams[1])
    stereo_cam.stereo_separation = 0.5
    counted = _abi.RenderOpts.from_buffer_copy(opts)
    counted.count_rays = 1
    preview = _abi.RenderOpts.from_buffer_copy(opts)
    preview.prepass_bucket = 16
    many = [cams[0]] * (MAX_BATCH + 1)
    cases = [
        ("dof camera", [cams[0], dof_cam, cams[2]], opts, _abi.ERR_UNSUPPORTED, "depth of field"),
        ("stereo camera", [cams[0], stereo_cam, cams[2]], opts, _abi.ERR_UNSUPPORTED, "stereo"),
        ("count_rays", cams, counted, _abi.ERR_UNSUPPORTED, "count_rays"),
        ("prepass_bucket", cams, preview, _abi.ERR_UNSUPPORTED, "prepass_bucket"),
        ("too many", many, opts, _abi.ERR_LIMIT, "at most"),
    ]
    for what, cc, oo, status, word in cases:
        out = sentinel()
        assert _raw_batch(gpu_ctx, cc, len(cc), oo, out) == status, what
        assert word in lib.c2rt_last_error(gpu_ctx.handle).decode(), what
        assert untouched(out), what
        dev = torch.full((3, 24, 40, 3), -3.0, dtype=torch.float32, device="cuda:0")
        arr = (_abi.CameraFrame * len(cc))(*cc)
        st = lib.c2rt_render_frames_device(gpu_ctx.handle, arr, len(cc), C.byref(oo), C.c_void_p(dev.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert st == status and bool((dev == -3.0).all()), what
    # all of these stay available frame by frame
    assert gpu_ctx.renderFrame(dof_cam, opts).shape == (24, 40, 3)
    out = sentinel()
    arr = (_abi.CameraFrame * 3)(*cams)
    assert lib.c2rt_render_frames(gpu_ctx.handle, None, 3, C.byref(opts), out.ctypes.data_as(C.c_void_p), None) == _abi.ERR_INVALID_ARG
    assert lib.c2rt_render_frames(gpu_ctx.handle, arr, 3, None, out.ctypes.data_as(C.c_void_p), None) == _abi.ERR_INVALID_ARG
    assert untouched(out)

    # a multi-device context renders frame by frame
    multi = c2.Context(devices=[0, 0])
    try:
        multi.uploadScene(scene.desc)
        out = sentinel()
        assert _raw_batch(multi, cams, 3, opts, out) == _abi.ERR_UNSUPPORTED and untouched(out)
        assert "multi-device" in lib.c2rt_last_error(multi.handle).decode()
    finally:
        multi.close()

    # host variant == device variant
    host = gpu_ctx.renderFrames(cams, opts)
    dev = torch.full((3, 24, 40, 3), -3.0, dtype=torch.float32, device="cuda:0")
    gpu_ctx.renderFramesDevice(cams, opts, dev.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(host), _bits(dev.cpu().numpy())) and np.array_equal(_bits(host), _bits(singles))

    # a raised stop flag: cancelled before the launches
    stop = np.ones(1, dtype=np.uint8)
    out = sentinel()
    assert _raw_batch(gpu_ctx, cams, 3, opts, out, stop) == _abi.ERR_CANCELLED and untouched(out)
    with pytest.raises(c2.C2rtError) as e:
        gpu_ctx.renderFrames(cams, opts, stop_flag=stop)
    assert e.value.status == _abi.ERR_CANCELLED
