"""c2rt_update_scene on the GPU: after an update the context behaves, in every entry point and in every bit, as a second
context freshly uploaded with the patched description does.  The yardstick is always that fresh c2rt_upload_scene (and
the oracle on the same description for the one-tap frame), never the update itself.  Frames are 96x64 and 100x52:
several 8x8 tiles, a partial tile on each edge of the second size, culling rectangles that cross tiles."""
import ctypes as C
import os

import numpy as np
import pytest

import chess2rt_amd as c2
import oracle_lib as orc
import scene_update_util as U
from chess2rt_amd import _abi
from parity_util import TOL, maxdiff

pytestmark = pytest.mark.gpu

SEQUENCES = U.sequences()
SIZES = ((96, 64), (100, 52))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.itemsize == 1 or a.dtype.names else a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def fresh_ctx(gpu_ctx):
    ctx = type(gpu_ctx)(0)  # the checked context of conftest.py: counted frames through lean:: and exact::
    yield ctx
    ctx.close()


def _copy(struct, **kw):
    out = type(struct).from_buffer_copy(struct)
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def _queries(cam):
    """512 rays from around the eye into the scene and 512 segments from points of the scene's volume towards light 0's
    first position: fixed, computed once"""
    r = np.random.RandomState(7)
    rays = np.empty((512, 6))
    rays[:, :3] = np.array(cam.pos[:]) + r.uniform(-5, 5, (512, 3))
    d = r.uniform([-1, -1.2, 0.3], [1, 0.1, 1.5], (512, 3))
    rays[:, 3:] = d / np.linalg.norm(d, axis=1, keepdims=True)
    seg = np.empty((512, 6))
    seg[:, :3] = r.uniform([-200, 0.5, 50], [200, 120, 400], (512, 3))
    seg[:, 3:] = (-90, 700, 350)
    return rays, seg


def everything(ctx, cam, opts, rays, seg):
    """what every entry point returns for (cam, opts): name -> array"""
    out = {}
    out["taps1"] = ctx.renderFrame(cam, _copy(opts, taps=_abi.TAPS_1))
    out["taps5"] = ctx.renderFrame(cam, _copy(opts, taps=_abi.TAPS_REF5))
    out["dof4"] = ctx.renderFrame(_copy(cam, dof=1, num_samples=4, focal_plane_dist=250.0, disc_multiplier=2.0), _copy(opts, taps=_abi.TAPS_1, seed=11))
    for name, plane in ctx.renderHits(cam, opts).items():
        out["hits." + name] = plane
    rec, rgb = ctx.traceRays(rays)
    out["rays.rec"], out["rays.rgb"] = rec, rgb
    out["visible"] = ctx.testVisibility(seg)
    out["adaptive"], out["adaptive.mask"] = ctx.renderFrameAdaptive(cam, _copy(opts, taps=_abi.TAPS_REF5))
    out["counted"] = ctx.renderFrame(cam, _copy(opts, taps=_abi.TAPS_1, count_rays=1))
    out["ray_stats"] = np.array(ctx.rayStats(), dtype=np.uint64)
    probe = ctx.renderPixel(cam, opts, opts.width // 2, opts.height // 2)
    out["probe"] = np.frombuffer(bytes(probe), dtype=np.uint8)
    return out


@pytest.mark.parametrize("case", ["sphere_moves", "ground_l5", "ground_planes", "csg_translated", "light0", "light2_of_three", "forty"])
def test_update_equals_fresh_upload_everywhere(gpu_ctx, fresh_ctx, tmp_path, case):
    key, seq = SEQUENCES[case]
    scene = U.load_case_scene(key, tmp_path)
    cur = U.Desc(scene.desc)
    gpu_ctx.uploadScene(cur.d)
    gen = gpu_ctx.sceneGeneration
    for k, (nodes, lights) in enumerate(seq):
        w, h = SIZES[k % 2]
        scene.setFrameSize(w, h)
        cam, opts = scene.beginFrame(), scene.renderOpts()
        rays, seg = _queries(cam)
        gpu_ctx.updateScene(nodes, lights)
        assert gpu_ctx.sceneGeneration == gen
        cur = cur.patched(nodes, lights)
        fresh_ctx.uploadScene(cur.d)
        got, want = everything(gpu_ctx, cam, opts, rays, seg), everything(fresh_ctx, cam, opts, rays, seg)
        for name in want:
            assert same(got[name], want[name]), "%s update %d: %s differs from the fresh upload's" % (case, k, name)
        ref = orc.render_frame(C.pointer(cur.d), cam, _copy(opts, taps=_abi.TAPS_1), 0)
        md, nbad, _ = maxdiff(got["taps1"], ref)
        assert md <= TOL and nbad == 0, (case, k, md)


def _lecture5(size=(96, 64)):
    scene = c2.parseSceneFromFile(os.path.join(U.SCENES, "lecture5.sdl"))
    scene.setFrameSize(*size)
    scene.setAA(False)
    return scene


def _fresh_frames(fresh_ctx, base, poses, cam, opts):
    """the fresh-upload frame after each pose of a cumulative sequence"""
    frames, cur = [], base
    for nodes, lights in poses:
        cur = cur.patched(nodes, lights)
        fresh_ctx.uploadScene(cur.d)
        frames.append(fresh_ctx.renderFrame(cam, opts))
    return frames


def test_ordering_without_syncs(gpu_ctx, fresh_ctx):
    """frame, update, frame, update, frame on one stream into three buffers with no host sync until the end; then the
    same with a three-frame batch in place of each frame"""
    import torch

    scene = _lecture5()
    cam, opts = scene.beginFrame(), scene.renderOpts()
    base = U.Desc(scene.desc)
    poses = [({}, None), ({3: U.xf(("translate", 60, 15, 200))}, {0: dict(pos=(50, 600, 200))}), ({3: U.xf(("scale", 1, 2, 1), ("translate", 20, 30, 180))}, None)]
    want = _fresh_frames(fresh_ctx, base, poses, cam, opts)
    assert not same(want[0], want[1]) and not same(want[1], want[2])
    scene.rotateCamera(9, 0, 0)
    cams = [cam, scene.beginFrame(), cam]
    want_b = [np.stack([f for c in cams for f in _fresh_frames(fresh_ctx, base, poses[:k + 1], c, opts)[-1:]]) for k in range(3)]

    for batch in (False, True):
        gpu_ctx.uploadScene(base.d)
        s = torch.cuda.Stream()
        n = 3 if batch else 1
        bufs = [torch.full((n, 64, 96, 3), -7.0, dtype=torch.float32, device="cuda:0") for _ in range(3)]
        torch.cuda.synchronize()
        for k in range(3):
            if k:
                gpu_ctx.updateScene(*poses[k], stream=s.cuda_stream)
            if batch:
                gpu_ctx.renderFramesDevice(cams, opts, bufs[k].data_ptr(), s.cuda_stream)
            else:
                gpu_ctx.renderFrameDevice(cam, opts, bufs[k].data_ptr(), s.cuda_stream)
        torch.cuda.synchronize()
        for k in range(3):
            got = bufs[k].cpu().numpy()
            assert same(got, want_b[k] if batch else want[k][None]), "batch %s, buffer %d" % (batch, k)


def test_a_refused_update_changes_nothing(gpu_ctx):
    scene = _lecture5()
    cam, opts = scene.beginFrame(), scene.renderOpts()
    lib = _abi.load_library()
    empty = c2.Context(0)
    try:
        assert lib.c2rt_update_scene(empty.handle, C.byref(c2.makePose({0: U.xf()})), None) == _abi.ERR_NO_SCENE
        assert "no scene" in lib.c2rt_last_error(empty.handle).decode()
    finally:
        empty.close()
    gpu_ctx.uploadScene(scene.desc)
    gpu_ctx.updateScene({4: U.xf(("translate", 10, 40, 150))})
    before = gpu_ctx.renderFrame(cam, opts)
    t = U.xf(("translate", 0, 90, 200))
    bad = [
        (None, "null pose"),
        (c2.makePose({6: t}), "node_index[0] = 6 out of range"),
        (c2.makePose({3: t}, {1: dict(power=1.0)}), "light_index[0] = 1 out of range"),
    ]
    twice = c2.makePose({3: t, 4: t})
    twice.node_index[1] = 3
    bad.append((twice, "node_index[1] = 3 is listed twice"))
    no_xf = c2.makePose({3: t})
    no_xf.node_transform = None
    bad.append((no_xf, "null node_transform"))
    no_light = c2.makePose(None, {0: dict(power=1.0)})
    no_light.light_power = None
    bad.append((no_light, "null light_pos, light_color and light_power"))
    for pose, word in bad:
        st = lib.c2rt_update_scene(gpu_ctx.handle, C.byref(pose) if pose is not None else None, None)
        assert st == _abi.ERR_INVALID_ARG, word
        assert word in lib.c2rt_last_error(gpu_ctx.handle).decode(), word
        assert same(gpu_ctx.renderFrame(cam, opts), before), word
    gpu_ctx.updateScene()  # an empty pose
    assert same(gpu_ctx.renderFrame(cam, opts), before)


def test_instance_flips(gpu_ctx, fresh_ctx):
    """lecture5 at 96x64: every matrix the identity -> a scaled ball (the general instance) -> the identity again; each
    frame and each growth of c2rt_get_exact_redos equals the fresh context's"""
    scene = _lecture5()
    cam, opts = scene.beginFrame(), scene.renderOpts()
    base = U.Desc(scene.desc)
    poses = [({3: U.xf(("scale", 1.5, 1, 1.5), ("translate", 100, 15, 256))}, None), ({3: base.transform(3)}, None)]
    gpu_ctx.uploadScene(base.d)
    fresh_ctx.uploadScene(base.d)
    cur = base
    first = None
    for k, (nodes, lights) in enumerate([({}, None)] + poses):
        gpu_ctx.updateScene(nodes, lights)
        cur = cur.patched(nodes, lights)
        fresh_ctx.uploadScene(cur.d)
        r0, q0 = gpu_ctx.exactRedos(), fresh_ctx.exactRedos()
        a, b = gpu_ctx.renderFrame(cam, opts), fresh_ctx.renderFrame(cam, opts)
        assert same(a, b), k
        assert gpu_ctx.exactRedos() - r0 == fresh_ctx.exactRedos() - q0, k
        first = a if first is None else first
    assert same(a, first)


def test_generation_and_the_host_mirror(gpu_ctx, fresh_ctx):
    scene = _lecture5()
    cam, opts = scene.beginFrame(), scene.renderOpts()
    base = U.Desc(scene.desc)
    r = c2.Renderer(scene, gpu_ctx)
    r.renderRT()
    gen = gpu_ctx.sceneGeneration
    assert gen != 0
    # a moved node: pushed as an update, the generation stays the scene's own, no re-upload
    scene.translateNode("S1", (-40, 20, -60), gpu_ctx)
    scene.setLight("light1", pos=(0, 650, 300), ctx=gpu_ctx)
    moved = base.patched({3: U.xf(("translate", 100, 15, 256), ("translate", -40, 20, -60))}, {0: dict(pos=(0, 650, 300))})
    assert scene.nodeIndex("S1") == 3 and scene.lightIndex("light1") == 0 and scene.nodeIndex("nobody") == -1
    assert np.array_equal(scene.nodeTransform("S1"), moved.transform(3))
    assert gpu_ctx.sceneGeneration == gen
    got = r.renderRT()
    assert gpu_ctx.sceneGeneration == gen
    fresh_ctx.uploadScene(moved.d)
    want = fresh_ctx.renderFrame(cam, opts)
    assert same(got, want) and not same(got, _fresh_frames(fresh_ctx, base, [({}, None)], cam, opts)[0])
    # the context moves on to another scene: the next change is not pushed, the next render re-uploads
    other = _lecture5()
    gpu_ctx.uploadScene(other.desc)
    gen2 = gpu_ctx.sceneGeneration
    scene.scaleNode("S2", 1, 2, 1, gpu_ctx)
    assert gpu_ctx.sceneGeneration == gen2
    assert same(gpu_ctx.renderFrame(cam, opts), _fresh_frames(fresh_ctx, base, [({}, None)], cam, opts)[0])  # still the other scene
    got = r.renderRT()
    assert gpu_ctx.sceneGeneration not in (gen, gen2)
    moved2 = moved.patched({4: U.xf(("translate", 100, 15, 206), ("scale", 1, 2, 1))})  # lecture5.sdl: S2 at 100 15 206
    assert np.array_equal(scene.nodeTransform("S2"), moved2.transform(4))
    fresh_ctx.uploadScene(moved2.d)
    assert same(got, fresh_ctx.renderFrame(cam, opts))


def test_multi_slot_context(fresh_ctx):
    scene = _lecture5((100, 52))
    cam, opts = scene.beginFrame(), scene.renderOpts()
    base = U.Desc(scene.desc)
    nodes, lights = {3: U.xf(("translate", 30, 15, 180)), 1: U.xf(("scale", 1, 1.5, 1))}, {0: dict(pos=(100, 500, 250), power=600000.0)}
    fresh_ctx.uploadScene(base.patched(nodes, lights).d)
    want = fresh_ctx.renderFrame(cam, opts)
    multi = c2.Context(devices=[0, 0, 0])
    try:
        multi.uploadScene(base.d)
        assert not same(multi.renderFrame(cam, opts), want)
        import torch

        s = torch.cuda.Stream()
        with pytest.raises(c2.C2rtError) as e:
            multi.updateScene(nodes, lights, stream=s.cuda_stream)
        assert e.value.status == _abi.ERR_INVALID_ARG and "hip_stream must be null" in str(e.value)
        multi.updateScene(nodes, lights)
        assert same(multi.renderFrame(cam, opts), want)
        dev = torch.full((52, 100, 3), -7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        multi.renderFrameDevice(cam, opts, dev.data_ptr(), 0)
        torch.cuda.synchronize()
        assert same(dev.cpu().numpy(), want)
    finally:
        multi.close()
