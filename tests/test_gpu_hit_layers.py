"""Hit layers on the GPU (c2rt_trace_rays_layers*, c2rt_render_hit_layers*): every surface along a ray or pixel, in order.
The yardstick is the definition (hit_layers_util.walk_layers) over the context's own single-hit query — bit for bit —
and over the CPU oracle's trace, which tests/test_hit_layers_abi.py entitles and whose preconditions it asserts."""
import ctypes as C
import os

import numpy as np
import pytest

import chess2rt_amd as c2
from chess2rt_amd import _abi
from chess2rt_amd.api import HIT_PLANES, RAY_HIT_DTYPE
from golden_configs import SCENES
from hit_layers_util import (FRAME_LAYERS, FRAME_SCENES, LAYERS, TRUNCATED, bits_equal_where_written, eyeless_layers, frame_layers,
                             layer_rays, walk_layers, written)
from parity_util import TOL, maxdiff
from ray_query_util import assert_records_match_oracle, bits
from test_gpu_ray_queries import EYELESS, H, SENTINEL, W

pytestmark = pytest.mark.gpu

GUARD = 256          # sentinel bytes behind each device output


def assert_layers_equal(got, want, K, what, colours=True):
    """(records, rgb, count) against (records, count, rgb), bit for bit on every slot the rule writes"""
    g_rec, g_rgb, g_count = got
    w_rec, w_count, w_rgb = want
    assert np.array_equal(g_count, w_count), (what, "count")
    m = written(w_count, K)
    assert bits_equal_where_written(g_rec, w_rec, m), (what, "records")
    if colours:
        assert bits_equal_where_written(g_rgb, w_rgb, m), (what, "colours")


# ---- 1, 2: the contract and the oracle ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", sorted(EYELESS))
def test_layers_are_the_walk_over_the_contexts_own_single_hit_query(gpu_ctx, name):
    scene, rays, _, _ = eyeless_layers(name)
    gpu_ctx.uploadScene(scene.desc)
    got = gpu_ctx.traceRayLayers(rays, LAYERS)
    want = walk_layers(lambda r: gpu_ctx.traceRays(r), rays, LAYERS, with_rgb=True)
    assert got[0].shape == (LAYERS, len(rays)) and got[0].dtype == RAY_HIT_DTYPE and got[1].shape == (LAYERS, len(rays), 3)
    assert got[2].shape == (len(rays),) and got[2].dtype == np.uint8 and int(got[2].max()) <= LAYERS
    assert_layers_equal(got, want, LAYERS, name)


@pytest.mark.parametrize("name", sorted(EYELESS))
def test_layers_match_the_oracles_walk(gpu_ctx, name):
    scene, rays, o_recs, o_count = eyeless_layers(name)
    gpu_ctx.uploadScene(scene.desc)
    recs, rgb, count = gpu_ctx.traceRayLayers(rays, LAYERS)
    assert np.array_equal(count, o_count), (name, int((count != o_count).sum()))
    worst = 0.0
    for k in range(LAYERS):
        idx = np.nonzero(o_count >= k)[0]         # the rays whose slot k is written
        if idx.size == 0:
            continue
        assert_records_match_oracle(recs[k, idx], o_recs[k, idx], "%s layer %d" % (name, k))
        idx2, stepped = layer_rays(rays, o_recs, o_count, k)
        assert np.array_equal(idx, idx2)
        _, want_rgb = gpu_ctx.traceRays(stepped, hits=False)
        md, nbad, _ = maxdiff(rgb[k, idx], want_rgb)
        worst = max(worst, md)
        assert md <= TOL and nbad == 0, (name, k, md)
    print("%s: colours of the oracle's stepped rays max|d| = %.3g" % (name, worst))


# ---- 3: truncation and the single layer --------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ("lecture5", "csg_stress", "fuzz_depth2"))
def test_truncation_and_the_single_layer(gpu_ctx, name):
    scene, rays, _, _ = eyeless_layers(name)
    gpu_ctx.uploadScene(scene.desc)
    rec8, rgb8, count8 = gpu_ctx.traceRayLayers(rays, LAYERS)
    rec3, rgb3, count3 = gpu_ctx.traceRayLayers(rays, TRUNCATED)
    assert np.array_equal(count3, np.minimum(count8, TRUNCATED))
    assert int((count8 >= TRUNCATED).sum()) >= 100
    m = written(count3, TRUNCATED)
    assert bits_equal_where_written(rec3, rec8[:TRUNCATED], m) and bits_equal_where_written(rgb3, rgb8[:TRUNCATED], m)
    rec1, rgb1, count1 = gpu_ctx.traceRayLayers(rays, 1)
    one_rec, one_rgb = gpu_ctx.traceRays(rays)
    assert np.array_equal(bits(rec1[0]), bits(one_rec)) and np.array_equal(bits(rgb1[0]), bits(one_rgb))
    assert np.array_equal(count1, (one_rec["closest_node"] >= 0).astype(np.uint8))
    assert np.array_equal(bits(rec8[0]), bits(one_rec)) and np.array_equal(bits(rgb8[0]), bits(one_rgb))


# ---- 4: what is not written ----------------------------------------------------------------------------------------------------


def device_run(ctx, rays_t, n, K, want_hits, want_rgb, want_count):
    """the device variant into 0xA5-filled torch tensors with guards; returns the raw bytes of the three outputs (or None)"""
    import torch

    dev = rays_t.device
    sizes = {"hits": K * n * 80, "rgb": K * n * 12, "count": n}
    asked = {"hits": want_hits, "rgb": want_rgb, "count": want_count}
    t = {k: torch.full((sizes[k] + GUARD,), SENTINEL, dtype=torch.uint8, device=dev) for k in sizes if asked[k]}
    torch.cuda.synchronize()
    ptr = lambda k: t[k].data_ptr() if k in t else 0
    ctx.traceRayLayersDevice(rays_t.data_ptr(), n, K, ptr("hits"), ptr("rgb"), ptr("count"), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = {}
    for k in sizes:
        if k in t:
            raw = t[k].cpu().numpy()
            assert (raw[sizes[k]:] == SENTINEL).all(), "guard behind %s" % k
            out[k] = raw[:sizes[k]]
        else:
            out[k] = None
    return out


@pytest.mark.parametrize("name", ("lecture5", "csg_stress"))
def test_slots_behind_the_final_miss_are_not_touched(gpu_ctx, name):
    import torch

    scene, rays, _, _ = eyeless_layers(name)
    n, K = len(rays), LAYERS
    gpu_ctx.uploadScene(scene.desc)
    want_rec, want_rgb, want_count = gpu_ctx.traceRayLayers(rays, K)
    rays_t = torch.from_numpy(rays).to("cuda:0")
    full = device_run(gpu_ctx, rays_t, n, K, True, True, True)
    count = full["count"]
    assert np.array_equal(count, want_count)
    m = written(count, K)
    assert (~m).sum() >= n                      # there is something to leave alone
    hits = full["hits"].reshape(K, n, 80)
    rgb = full["rgb"].reshape(K, n, 12)
    assert (hits[~m] == SENTINEL).all() and (rgb[~m] == SENTINEL).all()
    assert np.array_equal(hits[m], bits(want_rec).reshape(K, n, 80)[m]) and np.array_equal(rgb[m], bits(want_rgb).reshape(K, n, 12)[m])
    for combo in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)):
        part = device_run(gpu_ctx, rays_t, n, K, *combo)
        for k in ("hits", "rgb", "count"):
            if part[k] is not None:
                assert np.array_equal(part[k], full[k]), (name, combo, k)      # the written bits AND the untouched 0xA5


# ---- 5: tails and layout -------------------------------------------------------------------------------------------------------


def test_tails_and_layer_major_layout(gpu_ctx):
    import torch

    scene, rays, _, _ = eyeless_layers("csg_stress")
    gpu_ctx.uploadScene(scene.desc)
    K = 5
    full_rec, full_rgb, full_count = gpu_ctx.traceRayLayers(rays[:130], K)
    assert int(full_count[:63].max()) >= 3
    for n in (1, 63, 64, 65, 127):
        sub = np.ascontiguousarray(rays[:n])
        rec, rgb, count = gpu_ctx.traceRayLayers(sub, K)
        m = written(count, K)
        assert np.array_equal(count, full_count[:n]), n
        assert bits_equal_where_written(rec, np.ascontiguousarray(full_rec[:, :n]), m), n
        assert bits_equal_where_written(rgb, np.ascontiguousarray(full_rgb[:, :n]), m), n
        # the device variant: layer k of ray i at k * n + i, nothing outside the K * n slots
        out = device_run(gpu_ctx, torch.from_numpy(sub).to("cuda:0"), n, K, True, True, True)
        flat = out["hits"].reshape(K * n, 80)
        for k in range(K):
            for i in range(n):
                if m[k, i]:
                    assert flat[k * n + i].tobytes() == bits(full_rec[k, i:i + 1]).tobytes(), (n, k, i)
                else:
                    assert (flat[k * n + i] == SENTINEL).all(), (n, k, i)
        assert np.array_equal(out["rgb"].reshape(K, n, 12)[m], bits(np.ascontiguousarray(full_rgb[:, :n])).reshape(K, n, 12)[m]), n


# ---- 6: odd rays ---------------------------------------------------------------------------------------------------------------


def test_odd_rays_end_at_max_layers_and_stay_private(gpu_ctx):
    scene, rays, _, _ = eyeless_layers("lecture5")
    gpu_ctx.uploadScene(scene.desc)
    K = LAYERS
    clean = gpu_ctx.traceRayLayers(rays, K)
    dirty = rays.copy()
    bad = np.arange(0, len(rays), 7)
    for j, i in enumerate(bad):
        if j % 5 == 0:
            dirty[i, 3:] = 0.0
        elif j % 5 == 1:
            dirty[i, 0] = np.nan
        elif j % 5 == 2:
            dirty[i, 4] = np.inf
        elif j % 5 == 3:
            dirty[i, :3] = 1e300
        else:
            dirty[i, 3:] *= 1e-300          # a step that does not move the ray
    rec, rgb, count = gpu_ctx.traceRayLayers(dirty, K)        # returns: the walk is bounded by max_layers
    assert int(count.max()) <= K
    good = np.ones(len(rays), dtype=bool)
    good[bad] = False
    assert np.array_equal(count[good], clean[2][good])
    m = written(count, K) & good[None, :]
    assert bits_equal_where_written(rec, clean[0], m) and bits_equal_where_written(rgb, clean[1], m)
    for kk in (1, 16):
        _, _, c = gpu_ctx.traceRayLayers(dirty, kk, colors=False)
        assert int(c.max()) <= kk


# ---- 7: the frame face ---------------------------------------------------------------------------------------------------------

ALL_PLANES = tuple(HIT_PLANES)


def planes_from_records(recs, rgb, rows):
    """c2rt_hit_planes' arrays of [K][rows * W] records"""
    K = recs.shape[0]
    sh = (K, rows, W)
    return {"node": recs["closest_node"].reshape(sh), "leaf": recs["leaf_geom"].reshape(sh), "dist": recs["dist"].reshape(sh),
            "uv": np.stack([recs["u"], recs["v"]], axis=-1).reshape(sh + (2,)), "p": recs["p"].reshape(sh + (3,)),
            "normal": recs["normal"].reshape(sh + (3,)), "rgb": rgb.reshape(sh + (3,))}


def assert_planes_equal(got, want, count, K, names, what):
    m = written(count.ravel(), K).reshape((K,) + count.shape)
    for name in names:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (what, name)
        assert bits_equal_where_written(got[name], np.ascontiguousarray(want[name]), m), (what, name)


@pytest.mark.parametrize("scene_file", FRAME_SCENES)
def test_frame_face(gpu_ctx, scene_file):
    scene, cam, opts, rays, _, o_count = frame_layers(scene_file)
    K = FRAME_LAYERS
    gpu_ctx.uploadScene(scene.desc)
    got = gpu_ctx.renderHitLayers(cam, opts, K)
    count = got["count"]
    assert count.shape == (H, W) and count.dtype == np.uint8
    assert np.array_equal(count.ravel(), np.minimum(o_count, K))
    # layer 0 is renderHits
    single = gpu_ctx.renderHits(cam, opts)
    for name in ALL_PLANES:
        assert np.array_equal(bits(got[name][0]), bits(single[name])), (scene_file, name)
    # every layer is traceRayLayers over the camera's screen rays
    recs, rgb, rcount = gpu_ctx.traceRayLayers(rays, K)
    assert np.array_equal(rcount, count.ravel())
    want = planes_from_records(recs, rgb, H)
    assert_planes_equal(got, want, count, K, ALL_PLANES, scene_file)
    # plane subsets
    for subset in (("node", "dist"), ("rgb",), ()):
        part = gpu_ctx.renderHitLayers(cam, opts, K, planes=subset)
        assert set(part) == set(subset) | {"count"} and np.array_equal(part["count"], count), (scene_file, subset)
        assert_planes_equal(part, got, count, K, subset, (scene_file, subset))
    # strips: each rank's compact rows are the full frame's rows
    world = 3
    for rank in range(world):
        so = type(opts).from_buffer_copy(opts)
        so.strip_height, so.strip_rank, so.strip_world = 8, rank, world
        part = gpu_ctx.renderHitLayers(cam, so, K)
        ys = [y for y in range(H) if (y // 8) % world == rank]
        assert part["count"].shape == (len(ys), W) and np.array_equal(part["count"], count[ys])
        full_rows = {name: got[name][:, ys] for name in ALL_PLANES}
        assert_planes_equal(part, full_rows, count[ys], K, ALL_PLANES, (scene_file, "rank", rank))


def test_renderer_face_equals_the_contexts(gpu_ctx):
    scene = c2.parseSceneFromFile(os.path.join(SCENES, "lecture5.sdl"))      # a scene of its own: the renderer uploads it
    scene.setFrameSize(W, H)
    scene.setAA(False)
    scene.setDof(False)
    K = 4
    r = c2.Renderer(scene, gpu_ctx)
    got = r.renderHitLayers(K, planes=("node", "dist", "p", "rgb"))
    cam = scene.beginFrame()
    opts = scene.renderOpts(taps=_abi.TAPS_1)
    want = gpu_ctx.renderHitLayers(cam, opts, K, planes=("node", "dist", "p", "rgb"))
    assert np.array_equal(got["count"], want["count"]) and int(want["count"].max()) >= 3
    assert_planes_equal(got, want, want["count"], K, ("node", "dist", "p", "rgb"), "renderer")


def test_frame_device_variant_leaves_later_slots_alone(gpu_ctx):
    import torch

    scene, cam, opts, _, _, _ = frame_layers("csg_stress.sdl")
    K = FRAME_LAYERS
    gpu_ctx.uploadScene(scene.desc)
    want = gpu_ctx.renderHitLayers(cam, opts, K)
    count = want["count"]
    px = W * H
    t = {}
    for name, (dtype, comps) in HIT_PLANES.items():
        t[name] = torch.full((K * px * comps * np.dtype(dtype).itemsize + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    tc = torch.full((px + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu_ctx.renderHitLayersDevice(cam, opts, K, {k: v.data_ptr() for k, v in t.items()}, tc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    raw_count = tc.cpu().numpy()
    assert np.array_equal(raw_count[:px].reshape(H, W), count) and (raw_count[px:] == SENTINEL).all()
    m = written(count.ravel(), K)
    assert (~m).any()
    for name, (dtype, comps) in HIT_PLANES.items():
        size = comps * np.dtype(dtype).itemsize
        raw = t[name].cpu().numpy()
        assert (raw[K * px * size:] == SENTINEL).all(), name
        raw = raw[:K * px * size].reshape(K, px, size)
        assert (raw[~m] == SENTINEL).all(), name
        assert np.array_equal(raw[m], bits(want[name]).reshape(K, px, size)[m]), name


# ---- 8: statuses ---------------------------------------------------------------------------------------------------------------


def test_statuses_in_order_with_the_outputs_untouched(gpu_ctx):
    scene, cam, opts, rays, _, _ = frame_layers("lecture5.sdl")
    gpu_ctx.uploadScene(scene.desc)
    lib = _abi.load_library()
    h = gpu_ctx.handle
    small = np.ascontiguousarray(rays[:4])
    K = 2
    rec = np.full(K * 4 * 80 + 64, SENTINEL, dtype=np.uint8)
    rgb = np.full(K * 4 * 12 + 64, SENTINEL, dtype=np.uint8)
    cnt = np.full(4 + 64, SENTINEL, dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    err = lambda: lib.c2rt_last_error(h).decode()

    def ray_call(rays_, n, layers, r=rec, g=rgb, c=cnt):
        a = lib.c2rt_trace_rays_layers(h, vp(rays_), n, layers, vp(r), vp(g), vp(c))
        b = lib.c2rt_trace_rays_layers_device(h, vp(rays_), n, layers, vp(r), vp(g), vp(c), None)   # refused before any pointer is read
        assert a == b, (a, b)
        return a

    assert ray_call(None, 0, 0, None, None, None) == _abi.OK                       # n == 0 whatever else is passed
    assert ray_call(None, 4, 0, None, None, None) == _abi.ERR_INVALID_ARG and "null input" in err()
    assert ray_call(small, _abi.MAX_RAYS + 1, 0, None, None, None) == _abi.ERR_LIMIT and "rays" in err()
    assert ray_call(small, 4, 0, None, None, None) == _abi.ERR_INVALID_ARG and "max_layers is 0" in err()
    assert ray_call(small, 4, _abi.MAX_HIT_LAYERS + 1, None, None, None) == _abi.ERR_LIMIT and "layers" in err()
    assert ray_call(small, 4, K, None, None, None) == _abi.ERR_INVALID_ARG and "no output" in err()
    fresh = c2.Context(0)
    try:
        assert lib.c2rt_trace_rays_layers(fresh.handle, vp(small), 4, 0, None, None, None) == _abi.ERR_NO_SCENE      # before max_layers
        assert lib.c2rt_trace_rays_layers(fresh.handle, None, 0, 0, None, None, None) == _abi.OK
    finally:
        fresh.close()
    assert (rec == SENTINEL).all() and (rgb == SENTINEL).all() and (cnt == SENTINEL).all()

    # the frame face
    px = W * H
    node = np.full(K * px * 4 + 64, SENTINEL, dtype=np.uint8)
    fcnt = np.full(px + 64, SENTINEL, dtype=np.uint8)
    pl = _abi.HitPlanes()
    pl.node = node.ctypes.data
    empty = _abi.HitPlanes()

    def frame_call(cam_, opts_, layers, planes, c):
        cp = C.byref(cam_) if cam_ is not None else None
        op = C.byref(opts_) if opts_ is not None else None
        pp = C.byref(planes) if planes is not None else None
        a = lib.c2rt_render_hit_layers(h, cp, op, layers, pp, vp(c))
        b = lib.c2rt_render_hit_layers_device(h, cp, op, layers, pp, vp(c), None)
        assert a == b, (a, b)
        return a

    dof_cam = type(cam).from_buffer_copy(cam)
    dof_cam.dof, dof_cam.num_samples = 1, 4
    stereo_cam = type(cam).from_buffer_copy(cam)
    stereo_cam.stereo_separation = 0.5
    counted = type(opts).from_buffer_copy(opts)
    counted.count_rays = 1
    preview = type(opts).from_buffer_copy(opts)
    preview.prepass_bucket = 8
    bad_size = type(opts).from_buffer_copy(opts)
    bad_size.width = 0
    assert frame_call(None, opts, 0, None, None) == _abi.ERR_INVALID_ARG                     # a frame call's come first
    assert frame_call(cam, bad_size, 0, None, None) == _abi.ERR_INVALID_ARG
    assert frame_call(cam, opts, 0, None, None) == _abi.ERR_INVALID_ARG and err() == "null planes"
    assert frame_call(dof_cam, opts, 0, pl, fcnt) == _abi.ERR_INVALID_ARG and "max_layers is 0" in err()
    assert frame_call(dof_cam, opts, _abi.MAX_HIT_LAYERS + 1, pl, fcnt) == _abi.ERR_LIMIT and "layers" in err()
    assert frame_call(dof_cam, opts, K, empty, None) == _abi.ERR_INVALID_ARG and "no output" in err()
    assert frame_call(dof_cam, counted, K, pl, fcnt) == _abi.ERR_UNSUPPORTED and err() == "depth of field: a pixel's record is one ray's, a lens has many per pixel"
    assert frame_call(stereo_cam, counted, K, pl, fcnt) == _abi.ERR_UNSUPPORTED and err() == "stereo: a pixel's record is one ray's, a stereo camera has two per pixel"
    assert frame_call(cam, counted, K, pl, fcnt) == _abi.ERR_UNSUPPORTED and err() == "count_rays: the hit planes do not count rays"
    assert frame_call(cam, preview, K, pl, fcnt) == _abi.ERR_UNSUPPORTED and err() == "prepass_bucket: a preview's pixels share the sample of their block"
    assert (node == SENTINEL).all() and (fcnt == SENTINEL).all()

    # after the refusals the calls succeed on the same context
    assert lib.c2rt_trace_rays_layers(h, vp(small), 4, K, vp(rec), vp(rgb), vp(cnt)) == _abi.OK
    assert (rec[K * 4 * 80:] == SENTINEL).all() and (rgb[K * 4 * 12:] == SENTINEL).all() and (cnt[4:] == SENTINEL).all()
    want_rec, _, want_count = gpu_ctx.traceRayLayers(small, K)
    assert np.array_equal(cnt[:4], want_count)
    m = written(want_count, K)
    assert np.array_equal(rec[:K * 4 * 80].reshape(K, 4, 80)[m], bits(want_rec).reshape(K, 4, 80)[m])
    assert lib.c2rt_render_hit_layers(h, C.byref(cam), C.byref(opts), K, C.byref(empty), vp(fcnt)) == _abi.OK       # count alone
    assert np.array_equal(fcnt[:px].reshape(H, W), gpu_ctx.renderHitLayers(cam, opts, K, planes=())["count"]) and (fcnt[px:] == SENTINEL).all()
    with pytest.raises(c2.C2rtError):
        gpu_ctx.traceRayLayers(small, K + 1 + _abi.MAX_HIT_LAYERS)
    with pytest.raises(ValueError):
        gpu_ctx.traceRayLayers(np.zeros((3, 5)), K)


# ---- 9: after a pose -----------------------------------------------------------------------------------------------------------


def test_layers_see_an_updated_scene_on_the_same_stream(gpu_ctx):
    import torch

    import scene_update_util as U

    scene, rays, _, _ = eyeless_layers("lecture5")
    n, K = len(rays), LAYERS
    nodes = {3: U.xf(("translate", 60, 15, 200))}          # tests/test_gpu_scene_update.py's move of lecture5's node 3
    patched = U.Desc(scene.desc).patched(nodes, None)
    fresh = c2.Context(0)
    try:
        fresh.uploadScene(patched.d)
        want = fresh.traceRayLayers(rays, K)
    finally:
        fresh.close()
    gpu_ctx.uploadScene(scene.desc)
    before = gpu_ctx.traceRayLayers(rays, K)
    assert not np.array_equal(before[2], want[2]) or not bits_equal_where_written(before[0], want[0], written(want[2], K))
    dev = torch.device("cuda:0")
    rays_t = torch.from_numpy(rays).to(dev)
    rec_t = torch.zeros((K * n * 80,), dtype=torch.uint8, device=dev)
    rgb_t = torch.zeros((K, n, 3), dtype=torch.float32, device=dev)
    cnt_t = torch.zeros((n,), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    gpu_ctx.updateScene(nodes, None, stream=s.cuda_stream)
    gpu_ctx.traceRayLayersDevice(rays_t.data_ptr(), n, K, rec_t.data_ptr(), rgb_t.data_ptr(), cnt_t.data_ptr(), s.cuda_stream)
    s.synchronize()
    count = cnt_t.cpu().numpy()
    assert np.array_equal(count, want[2])
    m = written(count, K)
    assert np.array_equal(rec_t.cpu().numpy().reshape(K, n, 80)[m], bits(want[0]).reshape(K, n, 80)[m])
    assert np.array_equal(bits(rgb_t.cpu().numpy()).reshape(K, n, 12)[m], bits(want[1]).reshape(K, n, 12)[m])


# ---- 10: host chunking -----------------------------------------------------------------------------------------------------------


# 2^18 / max_layers rays per host chunk: a second chunk of one partial wave; 3 does not divide 2^18
@pytest.mark.parametrize("K,n", ((16, 16384 + 5), (3, 87381 + 5)))
def test_host_chunks_of_rays_equal_the_device_call(gpu_ctx, K, n):
    import torch
    from test_gpu_ray_queries import eyeless_case

    scene, base, _ = eyeless_case("csg_stress")
    gpu_ctx.uploadScene(scene.desc)
    rays = np.ascontiguousarray(np.tile(base, (n // len(base) + 1, 1))[:n])
    rec, rgb, count = gpu_ctx.traceRayLayers(rays, K)
    base_count = gpu_ctx.traceRayLayers(base, K, hits=False, colors=False)[2]
    assert np.array_equal(count, base_count[np.arange(n) % len(base)])
    s1 = torch.cuda.Stream(torch.device("cuda:0"))
    rays_t = torch.from_numpy(rays).to("cuda:0")
    sizes = {"hits": K * n * 80, "rgb": K * n * 12, "count": n}
    t = {k: torch.full((v + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0") for k, v in sizes.items()}
    torch.cuda.synchronize()
    gpu_ctx.traceRayLayersDevice(rays_t.data_ptr(), n, K, t["hits"].data_ptr(), t["rgb"].data_ptr(), t["count"].data_ptr(), s1.cuda_stream)
    s1.synchronize()
    raw = {k: t[k].cpu().numpy() for k in t}
    for k, size in sizes.items():
        assert (raw[k][size:] == SENTINEL).all(), "guard behind %s" % k
    assert np.array_equal(raw["count"][:n], count)
    m = written(count, K)
    tail = n - (1 << 18) // K                  # the rays of the host's second chunk
    assert m[:, -tail:].any() and (~m[:, -tail:]).any() and (~m[:, :-tail]).any()
    hits = raw["hits"][:sizes["hits"]].reshape(K, n, 80)
    cols = raw["rgb"][:sizes["rgb"]].reshape(K, n, 12)
    # the caller's bytes behind a ray's final miss stay, on both sides of the host's chunk boundary (the device variant's
    # contract; the host variant's slots there are unspecified, include/c2rt.h)
    assert (hits[~m] == SENTINEL).all() and (cols[~m] == SENTINEL).all()
    assert np.array_equal(hits[m], bits(rec).reshape(K, n, 80)[m]) and np.array_equal(cols[m], bits(rgb).reshape(K, n, 12)[m])


# 640 x 30: chunks of 25 and 5 rows at 16 layers; 16400 x 2: 2^18 / 16 / width is 0, one row per chunk
@pytest.mark.parametrize("w,h,names", ((640, 30, ALL_PLANES), (16400, 2, ("node", "dist"))), ids=("640x30", "16400x2"))
def test_host_chunks_of_a_frame_equal_the_device_call(gpu_ctx, w, h, names):
    import torch

    K = 16
    scene = c2.parseSceneFromFile(os.path.join(SCENES, "csg_stress.sdl"))
    scene.setFrameSize(w, h)
    scene.setAA(False)
    scene.setDof(False)
    cam, opts = scene.beginFrame(), scene.renderOpts(taps=_abi.TAPS_1)
    gpu_ctx.uploadScene(scene.desc)
    host = gpu_ctx.renderHitLayers(cam, opts, K, planes=names)
    count = host["count"]
    px = w * h
    s1 = torch.cuda.Stream(torch.device("cuda:0"))
    size = {name: HIT_PLANES[name][1] * np.dtype(HIT_PLANES[name][0]).itemsize for name in names}
    t = {name: torch.full((K * px * size[name] + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0") for name in names}
    tc = torch.full((px + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu_ctx.renderHitLayersDevice(cam, opts, K, {k: v.data_ptr() for k, v in t.items()}, tc.data_ptr(), s1.cuda_stream)
    s1.synchronize()
    raw_count = tc.cpu().numpy()
    assert np.array_equal(raw_count[:px].reshape(h, w), count) and (raw_count[px:] == SENTINEL).all()
    m = written(count.ravel(), K)
    assert int(count[-1].max()) >= 1 and (~m[:, -w:]).any()             # layers to copy and slots to leave in the last chunk
    for name in names:
        raw = t[name].cpu().numpy()
        assert (raw[K * px * size[name]:] == SENTINEL).all(), name
        raw = raw[:K * px * size[name]].reshape(K, px, size[name])
        assert (raw[~m] == SENTINEL).all(), name
        assert np.array_equal(raw[m], bits(host[name]).reshape(K, px, size[name])[m]), name
