"""Ray queries on the GPU (c2rt_trace_rays*, c2rt_test_visibility*) against the CPU oracle, the context's own frames
and its pixel probe.  The reference of the records is ray_query_util.oracle_trace, which tests/test_ray_queries_abi.py
entitles: the reference's trace() loop over orc_node_intersect.  Tolerances are the probe test's
(tests/test_gpu_parity.py): node and leaf equal, dist and p bit for bit, normal 1e-15, u, v 1e-12, colour TOL."""
import ctypes as C
import functools
import os
import shutil
import tempfile

import numpy as np
import pytest

import chess2rt_amd as c2
import oracle_lib as orc
from chess2rt_amd import _abi
from chess2rt_amd.api import RAY_HIT_DTYPE
from golden_configs import SCENES
from parity_util import TOL, maxdiff
from query_test_util import SENTINEL
from ray_query_util import (assert_records_match_oracle, bits, csg_node_mask, eyeless_rays, light_positions, oracle_trace,
                            oracle_visibility, record_from_trace_result, screen_rays, visibility_segments)
from scene_fuzz import many_nodes_scene_sdl, random_scene_sdl

pytestmark = pytest.mark.gpu

W, H = 61, 47            # 2 867 rays: 44 full waves and a 51-lane tail

# test 5's scenes: name -> (how to get the SDL, seed of the ray set).  The fuzz seeds are the first whose tree has
# exactly that CSG depth and whose ray set meets the preconditions below on the oracle alone (found on the CPU).
FUZZ_SEEDS = {0: 9, 1: 9, 2: 9, 3: 8, 4: 47}      # CSG depth -> scene_fuzz seed
EYELESS = {
    "lecture5": ("file", "lecture5.sdl", 1),
    "csg_stress": ("file", "csg_stress.sdl", 1),
    "fuzz_depth0": ("fuzz", FUZZ_SEEDS[0], 0),
    "fuzz_depth1": ("fuzz", FUZZ_SEEDS[1], 1),
    "fuzz_depth2": ("fuzz", FUZZ_SEEDS[2], 2),
    "fuzz_depth3": ("fuzz", FUZZ_SEEDS[3], 3),
    "fuzz_depth4": ("fuzz", FUZZ_SEEDS[4], 4),
    "many_nodes_31": ("many", 30, 1),      # 31 nodes: inside the 32-node culling mask
    "many_nodes_41": ("many", 40, 1),      # 41 nodes: nodes 32.. lie beyond it
}
_TMP = tempfile.mkdtemp(prefix="c2rt_rayq_")
shutil.copy(os.path.join(SCENES, "floor.bmp"), os.path.join(_TMP, "floor.bmp"))


def csg_depth(desc):
    d = desc.contents

    def depth(g):
        if d.geom_type[g] < _abi.GEOM_CSG_UNION:
            return 0
        return 1 + max(depth(d.geom_child[2 * g]), depth(d.geom_child[2 * g + 1]))
    return max(depth(d.node_geom[n]) for n in range(d.n_nodes))


@functools.lru_cache(maxsize=None)
def eyeless_case(name):
    """(scene, rays, oracle records) of one of test 5's scenes, computed once and shared (treated as read-only)"""
    kind, arg, extra = EYELESS[name]
    if kind == "file":
        scene = c2.parseSceneFromFile(os.path.join(SCENES, arg))
        ray_seed = extra
    else:
        text = random_scene_sdl(arg, max_depth=extra) if kind == "fuzz" else many_nodes_scene_sdl(extra, arg)
        path = os.path.join(_TMP, name + ".sdl")
        with open(path, "w") as f:
            f.write(text)
        scene = c2.parseSceneFromFile(path)
        ray_seed = 7
        if kind == "fuzz":
            assert csg_depth(scene.desc) == extra, (name, csg_depth(scene.desc))
    rays = eyeless_rays(scene.desc, ray_seed, 2000)
    want = oracle_trace(scene.desc, rays)
    return scene, rays, want


def check_eyeless_preconditions(name, scene, want):
    n = len(want)
    hit = want["closest_node"] >= 0
    assert hit.sum() >= 0.2 * n and (~hit).sum() >= 0.2 * n, (name, int(hit.sum()), n)
    csg = csg_node_mask(scene.desc)
    if csg.any():
        on_csg = int(csg[want["closest_node"][hit]].sum())
        assert on_csg >= 50, (name, on_csg)
    if scene.desc.contents.n_nodes > 32:
        assert int((want["closest_node"] >= 32).sum()) >= 20, name


def sentinel_buffers(n, extra=8):
    rec = np.full((n + extra) * RAY_HIT_DTYPE.itemsize, SENTINEL, dtype=np.uint8)
    rgb = np.full((n + extra) * 12, SENTINEL, dtype=np.uint8)
    return rec, rgb


def trace_raw(ctx, rays, n, rec, rgb):
    """c2rt_trace_rays over the first n rays into raw byte buffers (either may be None)"""
    lib = _abi.load_library()
    return lib.c2rt_trace_rays(ctx.handle, rays.ctypes.data_as(C.c_void_p) if rays is not None else None, n,
                               rec.ctypes.data_as(C.c_void_p) if rec is not None else None,
                               rgb.ctypes.data_as(C.c_void_p) if rgb is not None else None)


# ---- 3: counts around the wave size ---------------------------------------------------------------------------


def test_counts_around_the_wave_size(gpu_ctx):
    scene, rays, _ = eyeless_case("lecture5")
    rays = np.ascontiguousarray(rays[:130])
    gpu_ctx.uploadScene(scene.desc)
    full_rec, full_rgb = gpu_ctx.traceRays(rays)
    segs = np.ascontiguousarray(np.hstack([rays[:, :3], rays[::-1, :3] + [0.0, 40.0, 0.0]]))
    full_vis = gpu_ctx.testVisibility(segs)
    assert 0 < int((full_rec["closest_node"] >= 0).sum()) < 130 and 0 < int(full_vis.sum()) < 130
    lib = _abi.load_library()
    for n in (1, 63, 64, 65, 127, 130):
        rec, rgb = sentinel_buffers(n)
        assert trace_raw(gpu_ctx, rays, n, rec, rgb) == _abi.OK
        assert np.array_equal(rec[:n * 80], bits(full_rec[:n])), n
        assert np.array_equal(rgb[:n * 12], bits(full_rgb[:n]).ravel()), n
        assert (rec[n * 80:] == SENTINEL).all() and (rgb[n * 12:] == SENTINEL).all(), n
        vis = np.full(n + 64, SENTINEL, dtype=np.uint8)
        assert lib.c2rt_test_visibility(gpu_ctx.handle, segs.ctypes.data_as(C.c_void_p), n, vis.ctypes.data_as(C.c_void_p)) == _abi.OK
        assert np.array_equal(vis[:n], full_vis[:n]) and (vis[n:] == SENTINEL).all(), n


# ---- 4: a frame's own rays reproduce the frame -----------------------------------------------------------------

# nodes the oracle shows hidden at 61x47 (no pixel's closest node): none in these four scenes
HIDDEN_AT_61x47 = {"lecture5.sdl": set(), "csg_stress.sdl": set(), "zaphod.sdl": set(), "lecture4-proc-texture.sdl": set()}
# The files' own cameras look down at their floors (0 - 4 % of the rays miss at this size); the test's camera is the
# file's with its pitch raised by this many degrees, so that at least a tenth of the rays leave the scene while every
# node is still some ray's closest (both asserted on the oracle before any GPU call).
PITCH_UP = {"lecture5.sdl": 5.0, "csg_stress.sdl": 5.0, "zaphod.sdl": 40.0, "lecture4-proc-texture.sdl": 5.0}


@functools.lru_cache(maxsize=None)
def frame_case(scene_file):
    scene = c2.parseSceneFromFile(os.path.join(SCENES, scene_file))
    scene.setFrameSize(W, H)
    scene.setAA(False)
    scene.setDof(False)
    hc = scene.camera
    hc.pitch += PITCH_UP[scene_file]
    scene.camera = hc
    cam = scene.beginFrame()
    opts = scene.renderOpts(taps=_abi.TAPS_1)
    rays = screen_rays(cam, W, H)
    want = oracle_trace(scene.desc, rays)
    return scene, cam, opts, rays, want


@pytest.mark.parametrize("scene_file", sorted(HIDDEN_AT_61x47))
def test_a_frames_own_rays_reproduce_the_frame(gpu_ctx, scene_file):
    scene, cam, opts, rays, want = frame_case(scene_file)
    n = W * H
    # preconditions, on the oracle side
    hit = want["closest_node"] >= 0
    assert hit.sum() >= 0.1 * n and (~hit).sum() >= 0.1 * n, (scene_file, int(hit.sum()))
    seen = set(int(v) for v in want["closest_node"][hit])
    assert seen | HIDDEN_AT_61x47[scene_file] == set(range(scene.desc.contents.n_nodes)), (scene_file, sorted(seen))
    gpu_ctx.uploadScene(scene.desc)
    rec, rgb = gpu_ctx.traceRays(rays)
    frame = gpu_ctx.renderFrame(cam, opts)
    assert np.array_equal(bits(rgb), bits(frame.reshape(n, 3))), "%s: query colours differ from the context's own 1-tap frame" % scene_file
    ref = orc.render_frame(scene.desc, cam, opts, 0)
    md, nbad, nne = maxdiff(rgb, ref.reshape(n, 3))
    print("%s: rgb vs oracle frame max|d|=%.3g, !=: %d" % (scene_file, md, nne))
    assert md <= TOL and nbad == 0
    assert_records_match_oracle(rec, want, scene_file)
    rng = np.random.RandomState(5)
    pts = [(int(rng.randint(0, W)), int(rng.randint(0, H))) for _ in range(100)] + [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    for (x, y) in pts:
        g = record_from_trace_result(gpu_ctx.renderPixel(cam, opts, x, y))
        assert bits(np.array([g], dtype=RAY_HIT_DTYPE)).tobytes() == bits(rec[y * W + x:y * W + x + 1]).tobytes(), (scene_file, x, y)
        o = record_from_trace_result(orc.render_pixel(scene.desc, cam, opts, x, y))
        assert_records_match_oracle(rec[y * W + x:y * W + x + 1], np.array([o], dtype=RAY_HIT_DTYPE), (scene_file, x, y))


# ---- 5: rays that share no eye ----------------------------------------------------------------------------------


@pytest.mark.parametrize("name", sorted(EYELESS))
def test_rays_that_share_no_eye(gpu_ctx, name):
    scene, rays, want = eyeless_case(name)
    check_eyeless_preconditions(name, scene, want)
    gpu_ctx.uploadScene(scene.desc)
    rec, rgb = gpu_ctx.traceRays(rays)
    assert_records_match_oracle(rec, want, name)
    perm = np.random.RandomState(9).permutation(len(rays))
    rec2, rgb2 = gpu_ctx.traceRays(np.ascontiguousarray(rays[perm]))
    assert np.array_equal(bits(rec2), bits(rec[perm])) and np.array_equal(bits(rgb2), bits(rgb[perm])), "%s: shuffling is not a permutation" % name


# ---- 6: visibility ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", sorted(EYELESS))
def test_visibility_matches_the_oracle(gpu_ctx, name):
    scene, rays, want = eyeless_case(name)
    segs = visibility_segments(scene.desc, want, 21)
    ref = oracle_visibility(scene.desc, segs)
    frac = ref.mean()
    assert 0.15 <= frac <= 0.85, (name, frac)
    gpu_ctx.uploadScene(scene.desc)
    vis = gpu_ctx.testVisibility(segs)
    assert vis.dtype == np.uint8 and set(np.unique(vis)) <= {0, 1}
    assert np.array_equal(vis, ref), (name, int((vis != ref).sum()))


def test_a_lambert_pixel_is_lit_exactly_when_its_light_is_visible(gpu_ctx):
    """lecture4: one light, Lambert shading — for the frame rays that hit, colour above the ambient term alone
    exactly when the segment from the hit point to the light is visible (and the surface faces the light)."""
    scene, cam, opts, rays, want = frame_case("lecture4-proc-texture.sdl")
    d = scene.desc.contents
    assert d.n_lights == 1 and all(d.shader_type[d.node_shader[n]] == _abi.SHADER_LAMBERT for n in range(d.n_nodes))
    gpu_ctx.uploadScene(scene.desc)
    rec, rgb = gpu_ctx.traceRays(rays)
    hit = rec["closest_node"] >= 0
    light = light_positions(scene.desc)[0]
    nrm = rec["normal"][hit]
    facing = np.where((rays[hit, 3:] * nrm).sum(axis=1, keepdims=True) < 0, nrm, -nrm)   # faceforward
    frm = rec["p"][hit] + facing * 1e-6
    vis = gpu_ctx.testVisibility(np.hstack([frm, np.broadcast_to(light, frm.shape)])).astype(bool)
    toward = ((light - rec["p"][hit]) * facing).sum(axis=1) > 0
    # no ambient term (asserted): a pixel is lit exactly when some channel is not zero
    assert list(d.ambient) == [0.0, 0.0, 0.0]
    lit = (rgb[hit] != 0).any(axis=1)
    assert np.array_equal(lit, vis & toward)
    assert not (rgb[~hit] != 0).any()
    assert 0 < int((vis & toward).sum())


# ---- 7: bad lanes stay private ------------------------------------------------------------------------------------


def test_bad_lanes_stay_private(gpu_ctx):
    scene, rays, _ = eyeless_case("lecture5")
    gpu_ctx.uploadScene(scene.desc)
    clean_rec, clean_rgb = gpu_ctx.traceRays(rays)
    dirty = rays.copy()
    bad = np.arange(0, len(rays), 7)
    for k, i in enumerate(bad):
        if k % 4 == 0:
            dirty[i, 3:] = 0.0
        elif k % 4 == 1:
            dirty[i, 0] = np.nan
        elif k % 4 == 2:
            dirty[i, 4] = np.inf
        else:
            dirty[i, :3] = 1e80
    rec, rgb = gpu_ctx.traceRays(dirty)     # returns: every loop of the trace is bounded
    good = np.ones(len(rays), dtype=bool)
    good[bad] = False
    assert np.array_equal(bits(rec[good]), bits(clean_rec[good])) and np.array_equal(bits(rgb[good]), bits(clean_rgb[good]))
    want = oracle_trace(scene.desc, dirty[bad])
    assert_records_match_oracle(rec[bad], want, "bad lanes")


# ---- 8: statuses ----------------------------------------------------------------------------------------------------


def test_statuses_are_decided_before_anything_is_touched(gpu_ctx):
    scene, rays, _ = eyeless_case("lecture5")
    gpu_ctx.uploadScene(scene.desc)
    lib = _abi.load_library()
    h = gpu_ctx.handle
    small = np.ascontiguousarray(rays[:4])
    rec, rgb = sentinel_buffers(4)
    vis = np.full(16, SENTINEL, dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.c2rt_trace_rays(h, None, 0, None, None) == _abi.OK
    assert lib.c2rt_trace_rays_device(h, None, 0, None, None, None) == _abi.OK
    assert lib.c2rt_test_visibility(h, None, 0, None) == _abi.OK
    assert lib.c2rt_test_visibility_device(h, None, 0, None, None) == _abi.OK
    assert lib.c2rt_trace_rays(h, None, 4, vp(rec), vp(rgb)) == _abi.ERR_INVALID_ARG
    assert lib.c2rt_trace_rays(h, vp(small), 4, None, None) == _abi.ERR_INVALID_ARG
    assert lib.c2rt_trace_rays_device(h, vp(small), 4, None, None, None) == _abi.ERR_INVALID_ARG
    assert lib.c2rt_test_visibility(h, None, 4, vp(vis)) == _abi.ERR_INVALID_ARG
    assert lib.c2rt_test_visibility(h, vp(small), 4, None) == _abi.ERR_INVALID_ARG
    assert lib.c2rt_trace_rays(h, vp(small), _abi.MAX_RAYS + 1, vp(rec), vp(rgb)) == _abi.ERR_LIMIT
    assert lib.c2rt_trace_rays_device(h, vp(small), _abi.MAX_RAYS + 1, vp(rec), vp(rgb), None) == _abi.ERR_LIMIT
    assert lib.c2rt_test_visibility(h, vp(small), _abi.MAX_RAYS + 1, vp(vis)) == _abi.ERR_LIMIT
    fresh = c2.Context(0)
    try:
        assert lib.c2rt_trace_rays(fresh.handle, vp(small), 4, vp(rec), vp(rgb)) == _abi.ERR_NO_SCENE
        assert lib.c2rt_test_visibility(fresh.handle, vp(small), 4, vp(vis)) == _abi.ERR_NO_SCENE
        assert lib.c2rt_trace_rays(fresh.handle, None, 0, None, None) == _abi.OK
    finally:
        fresh.close()
    assert (rec == SENTINEL).all() and (rgb == SENTINEL).all() and (vis == SENTINEL).all()


# ---- 9: streams and the multi-slot context ----------------------------------------------------------------------------


def test_device_variants_on_streams_and_multi_slot_context(gpu_ctx):
    import torch

    scene, cam, opts, rays, _ = frame_case("lecture5.sdl")
    n = W * H
    gpu_ctx.uploadScene(scene.desc)
    want_rec, want_rgb = gpu_ctx.traceRays(rays)
    want_frame = gpu_ctx.renderFrame(cam, opts)
    dev = torch.device("cuda:0")
    rays_t = torch.from_numpy(rays).to(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    f1 = torch.full((H, W, 3), -1.0, dtype=torch.float32, device=dev)
    f2 = torch.full((H, W, 3), -1.0, dtype=torch.float32, device=dev)
    rec_t = torch.full((n * 80,), SENTINEL, dtype=torch.uint8, device=dev)
    rgb_t = torch.full((n, 3), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    # a frame, a ray batch of that frame's rays, another frame: one stream, no host sync in between
    gpu_ctx.renderFrameDevice(cam, opts, f1.data_ptr(), s1.cuda_stream)
    gpu_ctx.traceRaysDevice(rays_t.data_ptr(), n, rec_t.data_ptr(), rgb_t.data_ptr(), s1.cuda_stream)
    gpu_ctx.renderFrameDevice(cam, opts, f2.data_ptr(), s1.cuda_stream)
    s1.synchronize()
    for f in (f1, f2):
        assert np.array_equal(bits(f.cpu().numpy()), bits(want_frame))
    assert np.array_equal(rec_t.cpu().numpy(), bits(want_rec)) and np.array_equal(bits(rgb_t.cpu().numpy()), bits(want_rgb))
    # two streams concurrently: hits only on one, colours only on the other, and visibility
    half = n // 2
    rec_a = torch.full((half * 80,), SENTINEL, dtype=torch.uint8, device=dev)
    rgb_b = torch.full((n - half, 3), -1.0, dtype=torch.float32, device=dev)
    # from the eye to a point behind the hit (blocked) or, for a miss, 100 units out (free): both answers occur
    reach = np.where(want_rec["closest_node"] >= 0, want_rec["dist"] * 1.5, 100.0)
    segs = np.ascontiguousarray(np.hstack([rays[:, :3], rays[:, :3] + rays[:, 3:] * reach[:, None]]))
    segs_t = torch.from_numpy(segs).to(dev)
    vis_t = torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gpu_ctx.traceRaysDevice(rays_t.data_ptr(), half, rec_a.data_ptr(), 0, s1.cuda_stream)
    gpu_ctx.traceRaysDevice(rays_t.data_ptr() + half * 48, n - half, 0, rgb_b.data_ptr(), s2.cuda_stream)
    gpu_ctx.testVisibilityDevice(segs_t.data_ptr(), n, vis_t.data_ptr(), s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(rec_a.cpu().numpy(), bits(want_rec[:half]))
    assert np.array_equal(bits(rgb_b.cpu().numpy()), bits(want_rgb[half:]))
    want_vis = gpu_ctx.testVisibility(segs)
    assert np.array_equal(vis_t.cpu().numpy(), want_vis) and 0 < int(want_vis.sum()) < n
    # a multi-slot context (both slots on device 0) answers from its lead device
    multi = c2.Context(devices=[0, 0])
    try:
        multi.uploadScene(scene.desc)
        m_rec, m_rgb = multi.traceRays(rays)
        assert np.array_equal(bits(m_rec), bits(want_rec)) and np.array_equal(bits(m_rgb), bits(want_rgb))
        assert np.array_equal(multi.testVisibility(segs), want_vis)
    finally:
        multi.close()


# ---- 10: the Python face ------------------------------------------------------------------------------------------------


def test_python_face(gpu_ctx):
    scene, rays, _ = eyeless_case("csg_stress")
    rays = rays[:200]
    gpu_ctx.uploadScene(scene.desc)
    rec, rgb = gpu_ctx.traceRays(rays)
    rec_only, none_rgb = gpu_ctx.traceRays(rays, colors=False)
    none_rec, rgb_only = gpu_ctx.traceRays(rays, hits=False)
    assert none_rgb is None and none_rec is None
    assert np.array_equal(bits(rec_only), bits(rec)) and np.array_equal(bits(rgb_only), bits(rgb))
    assert rec.dtype == RAY_HIT_DTYPE and rec.shape == (200,) and rgb.dtype == np.float32 and rgb.shape == (200, 3)
    for name in ("closest_node", "leaf_geom", "dist", "u", "v", "p", "normal"):
        assert rec.dtype.fields[name][1] == getattr(_abi.RayHit, name).offset, name
    assert rec.dtype.itemsize == C.sizeof(_abi.RayHit) == 80
    with pytest.raises(ValueError):
        gpu_ctx.traceRays(np.zeros((3, 5)))
    with pytest.raises(c2.C2rtError):
        gpu_ctx.traceRays(rays, hits=False, colors=False)


# ---- 11: host chunking ------------------------------------------------------------------------------------------------

CHUNKED = (1 << 18) + 5          # the host variants stage 2^18 records per chunk: a second chunk of one partial wave
GUARD = 256                      # sentinel bytes behind each device output


def tiled(a, n):
    return np.ascontiguousarray(np.tile(a, (n // len(a) + 1, 1))[:n])


def guarded_bytes(torch, size):
    return torch.full((size + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0")


def payload(t, size, what):
    raw = t.cpu().numpy()
    assert (raw[size:] == SENTINEL).all(), "guard behind %s" % what
    return raw[:size]


@pytest.mark.parametrize("colours", (True, False), ids=("hits+rgb", "hits"))
def test_host_chunks_of_rays_equal_the_device_call(gpu_ctx, colours):
    import torch

    scene, base, _ = eyeless_case("lecture5")
    gpu_ctx.uploadScene(scene.desc)
    n = CHUNKED
    rays = tiled(base, n)
    base_rec, base_rgb = gpu_ctx.traceRays(base, colors=colours)
    rec, rgb = gpu_ctx.traceRays(rays, colors=colours)
    reps = np.arange(n) % len(base)
    assert np.array_equal(bits(rec), bits(base_rec[reps])), "records of the tiled rays"
    assert 0 < int((rec["closest_node"] >= 0).sum()) < n
    s1 = torch.cuda.Stream(torch.device("cuda:0"))
    rays_t = torch.from_numpy(rays).to("cuda:0")
    rec_t = guarded_bytes(torch, n * 80)
    rgb_t = guarded_bytes(torch, n * 12) if colours else None
    torch.cuda.synchronize()
    gpu_ctx.traceRaysDevice(rays_t.data_ptr(), n, rec_t.data_ptr(), rgb_t.data_ptr() if colours else 0, s1.cuda_stream)
    s1.synchronize()
    assert payload(rec_t, n * 80, "hits").tobytes() == bits(rec).tobytes()
    if colours:
        assert np.array_equal(bits(rgb), bits(base_rgb[reps]))
        assert payload(rgb_t, n * 12, "rgb").tobytes() == bits(rgb).tobytes()
    else:
        assert rgb is None


def test_host_chunks_of_segments_equal_the_device_call(gpu_ctx):
    import torch

    scene, _, want = eyeless_case("lecture5")
    gpu_ctx.uploadScene(scene.desc)
    base = visibility_segments(scene.desc, want, 21)
    n = CHUNKED
    segs = tiled(base, n)
    vis = gpu_ctx.testVisibility(segs)
    assert np.array_equal(vis, gpu_ctx.testVisibility(base)[np.arange(n) % len(base)])
    assert 0 < int(vis.sum()) < n
    s1 = torch.cuda.Stream(torch.device("cuda:0"))
    segs_t = torch.from_numpy(segs).to("cuda:0")
    vis_t = guarded_bytes(torch, n)
    torch.cuda.synchronize()
    gpu_ctx.testVisibilityDevice(segs_t.data_ptr(), n, vis_t.data_ptr(), s1.cuda_stream)
    s1.synchronize()
    assert np.array_equal(payload(vis_t, n, "visible"), vis)
