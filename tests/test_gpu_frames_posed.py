"""c2rt_render_frames_posed / _device: an animation in one launch pair.  Frame i of the batch equals
c2rt_update_scene(poses[i]) + c2rt_render_frame(cams[i]) on a scratch context, and the frame of a fresh upload of the
description patched by poses[i]; the context's own scene is unchanged.  96x64 and 100x52 frames."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import chess2rt_amd as c2
import scene_update_util as U
from chess2rt_amd import _abi
from query_test_util import same, scratch_ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lecture5(size=(100, 52)):
    scene = c2.parseSceneFromFile(os.path.join(U.SCENES, "lecture5.sdl"))
    scene.setFrameSize(*size)
    scene.setAA(False)
    return scene


def _cams(scene, n, yaw=8.0):
    cams = [scene.beginFrame()]
    for _ in range(n - 1):
        scene.rotateCamera(yaw, 0, 0)
        cams.append(scene.beginFrame())
    return cams


def _yardsticks(scratch, base, cams, poses, opts):
    """per frame: update + single frame on the scratch context (re-uploaded first: poses are relative to the scene as
    it is), and a fresh upload of the patched description"""
    out = []
    for cam, (nodes, lights) in zip(cams, poses):
        scratch.uploadScene(base.d)
        scratch.updateScene(nodes, lights)
        a = scratch.renderFrame(cam, opts)
        scratch.uploadScene(base.patched(nodes, lights).d)
        b = scratch.renderFrame(cam, opts)
        assert same(a, b)
        out.append(a)
    return np.stack(out)


# five poses of lecture5: none; the three balls moved (identity matrices throughout); one ball scaled (the general
# instance); the light moved; the CSG object and the globe moved together with the light
def _five_poses():
    return [
        ({}, None),
        ({3: U.xf(("translate", 60, 15, 220)), 4: U.xf(("translate", 10, 45, 180)), 5: U.xf(("translate", -40, 15, 140))}, None),
        ({4: U.xf(("scale", 1.5, 2, 1.5), ("translate", 50, 30, 206))}, None),
        (None, {0: dict(pos=(150, 500, 100), power=500000.0)}),
        ({2: U.xf(("translate", 30, 0, 40)), 1: U.xf(("translate", -20, 10, -60))}, {0: dict(pos=(-200, 400, 300))}),
    ]


@pytest.mark.parametrize("taps", [_abi.TAPS_1, _abi.TAPS_REF5])
def test_five_poses_five_cameras(gpu_ctx, scratch_ctx, taps):
    scene = _lecture5()
    cams = _cams(scene, 5)
    opts = scene.renderOpts(taps=taps)
    base = U.Desc(scene.desc)
    poses = _five_poses()
    want = _yardsticks(scratch_ctx, base, cams, poses, opts)
    assert len({f.tobytes() for f in want}) == 5
    gpu_ctx.uploadScene(base.d)
    unposed = gpu_ctx.renderFrame(cams[1], opts)
    got = gpu_ctx.renderFramesPosed(cams, poses, opts)
    for i in range(5):
        assert same(got[i], want[i]), "frame %d" % i
    # the context's scene is unchanged, on the device and on the host
    assert same(gpu_ctx.renderFrame(cams[1], opts), unposed)
    assert same(gpu_ctx.renderFramesPosed(cams[1:2], [({}, None)], opts)[0], unposed)


def test_identity_and_general_poses_share_a_launch(gpu_ctx, scratch_ctx):
    """frames 0 and 2 leave every matrix the identity, frames 1 and 3 do not: one launch, the general instance"""
    scene = _lecture5((96, 64))
    cams = _cams(scene, 4)
    opts = scene.renderOpts()
    base = U.Desc(scene.desc)
    poses = [({3: U.xf(("translate", 60, 15, 220))}, None), ({3: U.xf(("scale", 2, 1, 2), ("translate", 60, 15, 220))}, None),
             ({}, None), ({1: U.xf(("rotate", 30, 10, 0))}, None)]
    want = _yardsticks(scratch_ctx, base, cams, poses, opts)
    gpu_ctx.uploadScene(base.d)
    got = gpu_ctx.renderFramesPosed(cams, poses, opts)
    for i in range(4):
        assert same(got[i], want[i]), "frame %d" % i


def test_plane_instance_frames_are_grouped(gpu_ctx, scratch_ctx, tmp_path):
    """a planes-only scene: frames 0, 2 and 4 keep the plane instance, frames 1 and 3 rotate a plane out of it: two
    groups, each frame where it belongs in the output"""
    scene = U.load_text(tmp_path, U.planes_only(), "planes.sdl", (100, 52))
    cams = _cams(scene, 5, yaw=5.0)
    opts = scene.renderOpts()
    base = U.Desc(scene.desc)
    poses = [({}, None), ({1: U.xf(("rotate", 0, 20, 0))}, None), ({1: U.xf(("translate", 0, -20, 0))}, None),
             ({0: U.xf(("rotate", 10, 5, 0))}, None), ({0: U.xf(("scale", 2, 3, 2))}, None)]
    want = _yardsticks(scratch_ctx, base, cams, poses, opts)
    gpu_ctx.uploadScene(base.d)
    got = gpu_ctx.renderFramesPosed(cams, poses, opts)
    for i in range(5):
        assert same(got[i], want[i]), "frame %d" % i


def test_strips(gpu_ctx, scratch_ctx):
    scene = _lecture5((96, 64))
    cams = _cams(scene, 3)
    opts = scene.renderOpts(strip_world=3, strip_rank=1, strip_height=8)
    assert gpu_ctx.localRows(opts) == 24
    base = U.Desc(scene.desc)
    poses = _five_poses()[1:4]
    want = _yardsticks(scratch_ctx, base, cams, poses, opts)
    gpu_ctx.uploadScene(base.d)
    got = gpu_ctx.renderFramesPosed(cams, poses, opts)
    assert same(got, want)
    scratch_ctx.uploadScene(base.patched(*poses[2]).d)
    full = scratch_ctx.renderFrame(cams[2], scene.renderOpts())
    assert same(got[2], full[[y for y in range(64) if (y // 8) % 3 == 1]])


def test_edges_and_refusals(gpu_ctx):
    import torch

    scene = _lecture5((40, 24))
    cams = _cams(scene, 3)
    opts = scene.renderOpts()
    gpu_ctx.uploadScene(scene.desc)
    lib = _abi.load_library()
    t = U.xf(("translate", 0, 90, 200))
    good = [c2.makePose({3: t}), c2.makePose(), c2.makePose(None, {0: dict(power=1.0)})]
    arr = (_abi.CameraFrame * 3)(*cams)

    def call(poses, n=3, cams_arr=arr, oo=opts, device=False):
        parr = (_abi.ScenePose * 3)(*poses) if poses is not None else None
        if device:
            dev = torch.full((3, 24, 40, 3), -3.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            st = lib.c2rt_render_frames_posed_device(gpu_ctx.handle, cams_arr, parr, n, C.byref(oo), C.c_void_p(dev.data_ptr()), None)
            torch.cuda.synchronize()
            return st, bool((dev == -3.0).all())
        out = np.full((3, 24, 40, 3), -3.0, dtype=np.float32)
        st = lib.c2rt_render_frames_posed(gpu_ctx.handle, cams_arr, parr, n, C.byref(oo), out.ctypes.data_as(C.c_void_p), None)
        return st, bool((out == -3.0).all())

    for device in (False, True):
        assert call(good, n=0, device=device) == (_abi.OK, True)
        assert call(None, device=device) == (_abi.ERR_INVALID_ARG, True)
        assert "null poses" in lib.c2rt_last_error(gpu_ctx.handle).decode()
        bad = c2.makePose({9: t})
        assert call([good[0], good[1], bad], device=device) == (_abi.ERR_INVALID_ARG, True)
        assert "frame 2: pose: node_index[0] = 9 out of range" in lib.c2rt_last_error(gpu_ctx.handle).decode()
        twice = c2.makePose({3: t, 4: t})
        twice.node_index[1] = 3
        assert call([good[0], twice, good[2]], device=device) == (_abi.ERR_INVALID_ARG, True)
        assert "frame 1: pose: node_index[1] = 3 is listed twice" in lib.c2rt_last_error(gpu_ctx.handle).decode()
        dof = _abi.CameraFrame.from_buffer_copy(cams[1])
        dof.dof, dof.num_samples = 1, 4
        assert call(good, cams_arr=(_abi.CameraFrame * 3)(cams[0], dof, cams[2]), device=device) == (_abi.ERR_UNSUPPORTED, True)
        counted = _abi.RenderOpts.from_buffer_copy(opts)
        counted.count_rays = 1
        assert call(good, oo=counted, device=device) == (_abi.ERR_UNSUPPORTED, True)
        st, untouched = call(good, device=device)
        assert st == _abi.OK and not untouched
    assert gpu_ctx.renderFramesPosed([], [], opts).shape == (0, 24, 40, 3)


_NESTED_CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import pathlib, tempfile
import chess2rt_amd as c2
import scene_update_util as U
tmp = pathlib.Path(tempfile.mkdtemp())
scene = U.load_text(tmp, U.nested_csg(), "nested.sdl", (96, 64))
assert scene.desc.contents.n_nodes == 3
cams = [scene.beginFrame()]
for _ in range(2):
    scene.rotateCamera(6, 0, 0)
    cams.append(scene.beginFrame())
opts = scene.renderOpts()
base = U.Desc(scene.desc)
poses = [({1: U.xf(("translate", 20, 0, -30))}, None), ({}, None), ({1: U.xf(("scale", 1.2, 1, 1.2)), 2: U.xf(("translate", 40, 0, 0))}, {0: dict(pos=(100, 500, 100))})]
ctx, fresh = c2.Context(0), c2.Context(0)
ctx.uploadScene(base.d)
got = ctx.renderFramesPosed(cams, poses, opts)
for i, (cam, pose) in enumerate(zip(cams, poses)):
    fresh.uploadScene(base.patched(*pose).d)
    assert got[i].tobytes() == fresh.renderFrame(cam, opts).tobytes(), i
    fresh.uploadScene(base.d)
    fresh.updateScene(*pose)
    assert got[i].tobytes() == fresh.renderFrame(cam, opts).tobytes(), (i, "update")
print("ok")
'''


def test_nested_csg_retry_launch_per_posed_frame():
    """a depth-2 scene under C2RT_CSG_FIRST_CAP (diagnostics build): most CSG tiles overflow the first pass's hit stacks
    and are redone by the retry launch, each posed frame from its own list and its own node table"""
    env = dict(os.environ, C2RT_CSG_FIRST_CAP="3", C2RT_LIB_VARIANT="diag")
    p = subprocess.run([sys.executable, "-c", _NESTED_CHILD], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout + p.stderr
