"""Gather planes on the GPU (c2rt_render_gather*, c2rt_trace_rays_gather*).  Composition is the contract: the planes are,
BIT FOR BIT and with no sample excused, what tests/gather_reference.py makes of the context's own records
(c2rt_trace_rays), of the context's own records and colours for the rays the reference spawns (c2rt_trace_rays) and of
the context's own albedo (c2rt_trace_rays_shading); the spawned rays' records also match the oracle's.  Then the camera
call against the ray call, strips, sample counts, plane subsets, seeds, the occlusion planes' directions, misses and
garbage, max_trace_depth == 0, the host variants' chunks, a posed scene, the mirrors, and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import chess2rt_amd as c2
import gather_reference as gr
import occlusion_cases as oc
import query_test_util as Q
import scene_update_util as U
from chess2rt_amd import _abi
from chess2rt_amd.api import GATHER_PLANES, RAY_HIT_DTYPE
from query_test_util import GATHER, check_device_against_host, check_filled, device_planes, guarded, last_error, lib, raw_call, struct_of, untouched
from query_test_util import gather_options as g_opts
from ray_query_util import assert_records_match_oracle, bits, oracle_trace, scene_extent

pytestmark = pytest.mark.gpu

W, H, K, SEED = oc.W, oc.H, oc.K, oc.SEED
PLANES = tuple(GATHER_PLANES)
_cases = {}
same_planes = functools.partial(Q.same_planes, names=PLANES)


def composed(ctx, rays, samples, seed, idx=None):
    """the planes by composition on the context's own single-purpose queries; also (records, hit, spawned rays, their
    records)"""
    rec, _ = ctx.traceRays(rays, colors=False)
    idx = np.arange(len(rays)) if idx is None else idx
    hit, N, sp = gr.spawned(rec, rays[:, 3:], idx, samples, seed)
    ask = np.ascontiguousarray(sp[hit].reshape(-1, 6))
    node = np.full((len(rays), samples), -1, dtype=np.int32)
    rgb = np.zeros((len(rays), samples, 3), dtype=np.float32)
    srec = np.zeros(0, dtype=RAY_HIT_DTYPE)
    if len(ask):
        srec, srgb = ctx.traceRays(ask)
        node[hit] = srec["closest_node"].reshape(-1, samples)
        rgb[hit] = srgb.reshape(-1, samples, 3)
    albedo = ctx.traceRaysShading(rays, planes=("albedo",))["albedo"]
    return gr.planes(rec, N, sp, node, rgb, albedo, samples), (rec, hit, ask, srec)


def case(gpu_ctx, name):
    """uploads the scene and returns {ray set: (rays, planes of the fused call, planes by composition, (records, hit,
    spawned rays, their records))} — the queries run once per scene and are shared by the tests below (read-only)"""
    scene, _, _ = oc.load(name)
    gpu_ctx.uploadScene(scene.desc)
    if name not in _cases:
        out = {}
        for which in oc.RAY_SETS:
            rays = oc.ray_set(name, which)
            got = gpu_ctx.traceRaysGather(rays, K, SEED)
            want, parts = composed(gpu_ctx, rays, K, SEED)
            out[which] = (rays, got, want, parts)
        _cases[name] = out
    return _cases[name]


def nonzero(plane):
    return (np.ascontiguousarray(plane).view(np.uint32).reshape(-1, 3) != 0).any(axis=1)


# ---- composition -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_planes_are_the_composition_of_the_contexts_own_queries(gpu_ctx, name):
    scene, _, _ = oc.load(name)
    for which, (rays, got, want, (rec, hit, ask, srec)) in case(gpu_ctx, name).items():
        what = "%s %s" % (name, which)
        assert set(got) == set(PLANES)
        for p in PLANES:
            dtype, comps = GATHER_PLANES[p]
            assert got[p].dtype == dtype and got[p].shape == ((len(rays),) if comps == 1 else (len(rays), comps)), (what, p)
        mixed, full, empty = gr.mask_kinds(got["hits"], hit, K)
        lit = int(nonzero(got["indirect"])[hit].sum())
        print("%s: %d rays, %d hits, %d mixed, %d full, %d empty masks, %d hits with a non-zero indirect"
              % (what, len(rays), int(hit.sum()), mixed, full, empty, lit))
        same_planes(got, want, what)
        assert np.array_equal(got["node"], rec["closest_node"]), what
        # the records the masks are made of are the oracle's for the same rays
        assert_records_match_oracle(srec, oracle_trace(scene.desc, ask), what)
        assert mixed >= 100 and lit >= 100, what
        # bounce == albedo * indirect, recomputed from the returned planes
        albedo = gpu_ctx.traceRaysShading(rays, planes=("albedo",))["albedo"]
        again = (albedo * got["indirect"]).astype(np.float32)
        again[~hit] = 0
        assert again.tobytes() == got["bounce"].tobytes(), what


# ---- the camera call is the ray call on the frame's screen rays; strips ----------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_camera_call_equals_ray_call_and_strips(gpu_ctx, name):
    scene, cam, opts = oc.load(name)
    rays, want, _, _ = case(gpu_ctx, name)["screen"]
    full = gpu_ctx.renderGather(cam, opts, K, SEED)
    for p in PLANES:
        assert full[p].shape[:2] == (H, W), p
    same_planes(full, want, "%s frame against its screen rays" % name)
    # opts.seed is ignored, as the hit planes ignore it
    other = _abi.RenderOpts.from_buffer_copy(opts)
    other.seed = 99
    same_planes(gpu_ctx.renderGather(cam, other, K, SEED), full, "%s opts.seed" % name)
    Q.check_strips(gpu_ctx, scene, lambda o: gpu_ctx.renderGather(cam, o, K, SEED), full, H, 3, 8, PLANES, name)


# ---- sample counts -----------------------------------------------------------------------------------------------------


def test_sample_counts(gpu_ctx):
    name = "lecture5"
    rays, _, _, (rec, hit, _, _) = case(gpu_ctx, name)["screen"]
    p64 = gpu_ctx.traceRaysGather(rays, 64, SEED)
    assert not p64["hits"][~hit].any() and (~hit).any()
    assert ((p64["hits"][hit] >> np.uint64(63)) & np.uint64(1)).any()                 # the last bit is reached
    for k in (1, 31, 32, 33, 64):
        low = np.uint64((1 << k) - 1)
        got = p64 if k == 64 else gpu_ctx.traceRaysGather(rays, k, SEED)
        assert not (got["hits"] & ~low).any(), k                                     # bits at and above K are zero
        assert np.array_equal(got["hits"], p64["hits"] & low), k
        if k in (1, 33, 64):
            same_planes(got, composed(gpu_ctx, rays, k, SEED)[0], "K = %d" % k)


# ---- plane independence and seeds ------------------------------------------------------------------------------------------


def test_plane_independence_and_seeds(gpu_ctx):
    name = "csg_stress"
    scene, cam, opts = oc.load(name)
    c = case(gpu_ctx, name)
    rays, full_rays = c["eyeless"][0], c["eyeless"][1]
    full = gpu_ctx.renderGather(cam, opts, K, SEED)
    subsets = [(p,) for p in PLANES] + [("node", "hits"), ("hits", "indirect")]
    Q.check_plane_subsets(GATHER, gpu_ctx, cam, opts, rays, g_opts(K, SEED), subsets, full, full_rays, W * H, name, align=8)
    hits = gpu_ctx.renderHits(cam, opts, planes=("node",))
    alone = gpu_ctx.renderGather(cam, opts, K, SEED, planes=("node",))
    assert list(alone) == ["node"] and bits(alone["node"]).tobytes() == bits(hits["node"]).tobytes()
    with pytest.raises(ValueError):
        gpu_ctx.renderGather(cam, opts, K, SEED, planes=("depth",))
    # the same seed: the same planes; another seed: other directions
    same_planes(gpu_ctx.traceRaysGather(rays, K, SEED), full_rays, "second call")
    other = gpu_ctx.traceRaysGather(rays, K, SEED + 1)
    assert np.array_equal(other["node"], full_rays["node"])
    changed = int((other["hits"] != full_rays["hits"]).sum())
    print("seed %d -> %d: %d of %d masks change" % (SEED, SEED + 1, changed, len(rays)))
    assert changed >= 100
    same_planes(other, composed(gpu_ctx, rays, K, SEED + 1)[0], "seed + 1")
    big = (1 << 40) + 5                                                  # the seed's high word reaches the key
    same_planes(gpu_ctx.traceRaysGather(rays[:256], K, big), composed(gpu_ctx, rays[:256], K, big)[0], "64-bit seed")


# ---- the directions are the occlusion planes' ------------------------------------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_hits_are_the_occlusion_planes_closed_samples(gpu_ctx, name):
    """with the occlusion planes at the same seed and a radius beyond the scene, a spawned ray hits a node exactly where
    the segment is occluded; where a spawned ray's hit lies beyond the radius (the unbounded floor) the ray is left out"""
    scene, _, _ = oc.load(name)
    rays, got, _, (rec, hit, ask, srec) = case(gpu_ctx, name)["screen"]
    _, half, _ = scene_extent(scene.desc)
    radius = 4.0 * 2.0 * float(np.max(half))
    occ = gpu_ctx.traceRaysOcclusion(rays, K, radius, SEED, planes=("node", "open"))
    assert np.array_equal(occ["node"], got["node"])
    low = np.uint64((1 << K) - 1)
    dist = srec["dist"].reshape(-1, K)
    near = ((srec["closest_node"].reshape(-1, K) < 0) | (dist < radius)).all(axis=1)
    print("%s: radius %g, %d of %d hits have every spawned hit inside it" % (name, radius, int(near.sum()), int(hit.sum())))
    assert near.sum() >= 0.9 * hit.sum()
    assert np.array_equal(got["hits"][hit][near], (~occ["open"][hit][near]) & low)


# ---- misses and bad rays -----------------------------------------------------------------------------------------------------


def test_misses_and_garbage_rays(gpu_ctx):
    name = "lecture5"
    rays0, want, _, (rec, hit, _, _) = case(gpu_ctx, name)["eyeless"]
    miss = ~hit
    assert miss.sum() >= 100
    assert (want["node"][miss] == -1).all() and not want["hits"][miss].any()
    assert not want["indirect"][miss].view(np.uint32).any() and not want["bounce"][miss].view(np.uint32).any()   # +0, +0, +0
    Q.check_garbage_lanes(lambda rays: gpu_ctx.traceRaysGather(rays, K, SEED), rays0, want, hit, PLANES, "hits", K)


# ---- max_trace_depth == 0 ----------------------------------------------------------------------------------------------------


def test_max_trace_depth_zero_draws_nothing(gpu_ctx):
    name = "lecture5"
    scene, cam, opts = oc.load(name)
    rays, want, _, (rec, hit, _, _) = case(gpu_ctx, name)["screen"]
    flat = _abi.SceneDesc.from_buffer_copy(scene.desc.contents)
    assert flat.max_trace_depth > 0
    flat.max_trace_depth = 0
    gpu_ctx.uploadScene(flat)
    try:
        for got in (gpu_ctx.traceRaysGather(rays, K, SEED), gpu_ctx.renderGather(cam, opts, K, SEED)):
            assert np.array_equal(got["node"].reshape(-1), want["node"]) and hit.any()
            for p in ("hits", "indirect", "bounce"):
                assert not bits(got[p]).any(), p
    finally:
        gpu_ctx.uploadScene(scene.desc)


# ---- host variants -----------------------------------------------------------------------------------------------------------


def test_host_variants_equal_the_device_variants(gpu_ctx):
    import torch

    name = "lecture5"
    scene, cam, opts = oc.load(name)
    base = case(gpu_ctx, name)["screen"]
    dev = torch.device("cuda:0")
    s1 = torch.cuda.Stream(dev)
    # the frame at 61x47
    host = gpu_ctx.renderGather(cam, opts, K, SEED)
    t = device_planes(GATHER_PLANES, W * H, dev, guard_bytes=64)
    torch.cuda.synchronize()
    gpu_ctx.renderGatherDevice(cam, opts, K, {k: v.data_ptr() for k, v in t.items()}, seed=SEED, stream=s1.cuda_stream)
    s1.synchronize()
    check_device_against_host(GATHER_PLANES, t, host, W * H, "61x47")
    # 2^18 + 70 rays, K = 2: the second chunk starts at a non-zero index, and its rays draw the samples of THEIR index
    n = (1 << 18) + 70
    reps = np.arange(n) % len(base[0])
    rays = np.ascontiguousarray(base[0][reps])
    host = gpu_ctx.traceRaysGather(rays, 2, SEED)
    t = device_planes(GATHER_PLANES, n, dev, guard_bytes=64)
    rays_t = torch.from_numpy(rays).to(dev)
    torch.cuda.synchronize()
    gpu_ctx.traceRaysGatherDevice(rays_t.data_ptr(), n, 2, {k: v.data_ptr() for k, v in t.items()}, seed=SEED, stream=s1.cuda_stream)
    s1.synchronize()
    check_device_against_host(GATHER_PLANES, t, host, n, "2^18 + 70 rays")
    assert np.array_equal(host["node"], base[1]["node"][reps])
    # the tail behind the chunk boundary against the composition at its own indices; a copy of a ray elsewhere in the
    # array draws other directions
    tail = np.arange((1 << 18) - 30, n)
    want, _ = composed(gpu_ctx, rays[tail], 2, SEED, idx=tail)
    for p in PLANES:
        assert bits(host[p][tail]).tobytes() == bits(want[p]).tobytes(), p
    first = np.arange(len(base[0]))
    assert (host["hits"][first] != host["hits"][first + len(base[0])]).any()
    assert (host["indirect"][first] != host["indirect"][first + len(base[0])]).any()


# ---- a posed scene and the mirrors ---------------------------------------------------------------------------------------------


def test_posed_scene_and_mirrors(gpu_ctx):
    name = "lecture5"
    scene, cam, opts = oc.load(name)
    rays, before, _, _ = case(gpu_ctx, name)["screen"]
    frame = gpu_ctx.renderGather(cam, opts, K, SEED)
    # Renderer.renderGather and the host mirror are the Context call for the scene's own camera
    got = c2.Renderer(scene, gpu_ctx).renderGather(K, SEED)
    assert set(got) == set(PLANES)
    same_planes(got, frame, "Renderer.renderGather")
    sub = c2.Renderer(scene, gpu_ctx).renderGather(K, SEED, planes=("bounce",))
    assert list(sub) == ["bounce"] and bits(sub["bounce"]).tobytes() == bits(frame["bounce"]).tobytes()
    raw = guarded(GATHER_PLANES, PLANES, W * H, align=8)
    pl, g = struct_of(_abi.GatherPlanes, raw), g_opts(K, SEED)
    assert lib().c2rt_host_render_gather(gpu_ctx.handle, scene._h, C.byref(g), C.byref(pl)) == _abi.OK, last_error(gpu_ctx)
    check_filled(GATHER_PLANES, raw, frame, W * H, "c2rt_host_render_gather")
    # a ball moves: the call sees the posed scene
    gpu_ctx.uploadScene(scene.desc)
    gpu_ctx.updateScene({3: U.xf(("translate", 60, 15, 200))})
    try:
        posed = gpu_ctx.traceRaysGather(rays, K, SEED)
        want, _ = composed(gpu_ctx, rays, K, SEED)
        same_planes(posed, want, "posed")
        same_planes(gpu_ctx.renderGather(cam, opts, K, SEED), want, "posed frame")
        assert int((posed["hits"] != before["hits"]).sum()) >= 30 and not np.array_equal(posed["node"], before["node"])
    finally:
        gpu_ctx.uploadScene(scene.desc)


# ---- refusals ------------------------------------------------------------------------------------------------------------------


BAD_G = [  # (options, status, the whole message), in the documented order
    (dict(samples=0), _abi.ERR_INVALID_ARG, "gather samples is 0: at least one sample"),
    (dict(reserved=1), _abi.ERR_INVALID_ARG, "c2rt_gather_opts.reserved is 1: must be 0"),
    (dict(samples=65), _abi.ERR_LIMIT, "65 gather samples (at most 64)"),
]


def test_frame_refusals_leave_the_outputs_untouched(gpu_ctx):
    name = "lecture5"
    scene, cam, opts = oc.load(name)
    want = case(gpu_ctx, name)["screen"][1]
    n = W * H
    L = lib()

    def copy_cam(**kw):
        return Q.with_fields(cam, **kw)

    def copy_opts(**kw):
        return Q.with_fields(opts, **kw)

    bufs = guarded(GATHER_PLANES, PLANES, n, align=8)
    pl, none = struct_of(_abi.GatherPlanes, bufs), _abi.GatherPlanes()
    good = g_opts(K, SEED)
    dof = copy_cam(dof=1, num_samples=4)

    def both(c, o, g, planes):
        """the host and the device variant decide the same before anything is enqueued (the pointers are never used)"""
        a = (None if c is None else C.byref(c), C.byref(o), None if g is None else C.byref(g), None if planes is None else C.byref(planes))
        st = L.c2rt_render_gather(gpu_ctx.handle, *a)
        msg = last_error(gpu_ctx)
        assert L.c2rt_render_gather_device(gpu_ctx.handle, *a, None) == st and last_error(gpu_ctx) == msg
        return st, msg

    # a frame call's own statuses come first, in c2rt_render_hits' order
    assert both(None, opts, good, pl)[0] == _abi.ERR_INVALID_ARG
    st, msg = both(cam, copy_opts(width=0), None, None)
    hp = _abi.HitPlanes(node=bufs["node"].ctypes.data)
    assert st == L.c2rt_render_hits(gpu_ctx.handle, C.byref(cam), C.byref(copy_opts(width=0)), C.byref(hp)) != _abi.OK and msg == last_error(gpu_ctx)
    # then the options, each with its own message
    st, msg = both(cam, opts, None, pl)
    assert st == _abi.ERR_INVALID_ARG and msg == "null gather options"
    for kw, status, text in BAD_G:
        st, msg = both(cam, opts, g_opts(**{**dict(samples=K), **kw}), pl)
        assert st == status and msg == text, (kw, st, msg)
    # two rules at once: samples == 0 and reserved before the limit, the options before the planes, the planes before
    # the modes
    st, msg = both(cam, opts, g_opts(samples=0, reserved=3), pl)
    assert st == _abi.ERR_INVALID_ARG and msg == "gather samples is 0: at least one sample"
    st, msg = both(cam, opts, g_opts(samples=65, reserved=3), pl)
    assert st == _abi.ERR_INVALID_ARG and msg == "c2rt_gather_opts.reserved is 3: must be 0"
    assert both(cam, opts, g_opts(samples=65), None)[0] == _abi.ERR_LIMIT
    assert both(cam, opts, None, None)[1] == "null gather options"
    st, msg = both(cam, opts, good, None)
    assert st == _abi.ERR_INVALID_ARG and msg == "null planes"
    st, msg = both(cam, opts, good, none)
    assert st == _abi.ERR_INVALID_ARG and msg == "no plane asked for: all four pointers of c2rt_gather_planes are null"
    assert both(dof, opts, good, none)[0] == _abi.ERR_INVALID_ARG
    assert both(dof, opts, g_opts(samples=65), pl)[0] == _abi.ERR_LIMIT
    # then the modes in which a pixel is not one ray
    for c, o, cause in [(dof, opts, "depth of field: a pixel's gather is one ray's, a lens has many per pixel"),
                        (copy_cam(stereo_separation=0.5), opts, "stereo: a pixel's gather is one ray's, a stereo camera has two per pixel"),
                        (cam, copy_opts(count_rays=1), "count_rays: the gather planes do not count rays"),
                        (cam, copy_opts(prepass_bucket=48), "prepass_bucket: a preview's pixels share the sample of their block")]:
        st, msg = both(c, o, good, pl)
        assert st == _abi.ERR_UNSUPPORTED and msg == cause, (cause, st, msg)
    assert both(copy_cam(dof=1, num_samples=4, stereo_separation=0.5), copy_opts(count_rays=1), good, pl)[1] == "depth of field: a pixel's gather is one ray's, a lens has many per pixel"
    fresh = c2.Context(0)
    try:
        a = (C.byref(cam), C.byref(opts))
        assert L.c2rt_render_gather(fresh.handle, *a, C.byref(good), C.byref(pl)) == _abi.ERR_NO_SCENE and "no scene" in last_error(fresh)
        assert L.c2rt_render_gather(fresh.handle, *a, None, None) == _abi.ERR_NO_SCENE          # the frame checks come first
    finally:
        fresh.close()
    assert untouched(bufs)
    # afterwards the same context fills a correct plane set
    assert raw_call(GATHER, gpu_ctx, bufs, cam, opts, options=good) == _abi.OK, last_error(gpu_ctx)
    check_filled(GATHER_PLANES, bufs, want, n, "after the refusals")


def test_ray_refusals_leave_the_outputs_untouched(gpu_ctx):
    name = "lecture5"
    rays, want, _, _ = case(gpu_ctx, name)["eyeless"]
    n = len(rays)
    bufs = guarded(GATHER_PLANES, PLANES, n, align=8)
    L = lib()
    pl, none = struct_of(_abi.GatherPlanes, bufs), _abi.GatherPlanes()
    good = g_opts(K, SEED)
    bad = g_opts(samples=0, reserved=9)
    rp = rays.ctypes.data_as(C.c_void_p)
    for fn, tail in ((L.c2rt_trace_rays_gather, ()), (L.c2rt_trace_rays_gather_device, (None,))):
        assert fn(None, rp, n, C.byref(good), C.byref(pl), *tail) == _abi.ERR_INVALID_ARG          # null context
        assert fn(gpu_ctx.handle, None, 0, None, None, *tail) == _abi.OK                           # n == 0, whatever else
        assert fn(gpu_ctx.handle, None, 0, C.byref(bad), C.byref(none), *tail) == _abi.OK
        assert fn(gpu_ctx.handle, None, n, None, None, *tail) == _abi.ERR_INVALID_ARG              # null rays before the options
        assert "null input array" in last_error(gpu_ctx)
        assert fn(gpu_ctx.handle, rp, _abi.MAX_RAYS + 1, None, None, *tail) == _abi.ERR_LIMIT      # the limit before the options
        assert "rays in one call" in last_error(gpu_ctx)
        assert fn(gpu_ctx.handle, rp, n, None, C.byref(pl), *tail) == _abi.ERR_INVALID_ARG
        assert last_error(gpu_ctx) == "null gather options"
        for kw, status, text in BAD_G:
            g = g_opts(**{**dict(samples=K), **kw})
            assert fn(gpu_ctx.handle, rp, n, C.byref(g), C.byref(pl), *tail) == status and last_error(gpu_ctx) == text, (kw, last_error(gpu_ctx))
        assert fn(gpu_ctx.handle, rp, n, C.byref(bad), None, *tail) == _abi.ERR_INVALID_ARG and last_error(gpu_ctx) == "gather samples is 0: at least one sample"
        assert fn(gpu_ctx.handle, rp, n, C.byref(g_opts(samples=65)), None, *tail) == _abi.ERR_LIMIT   # the options before the planes
        assert fn(gpu_ctx.handle, rp, n, C.byref(good), None, *tail) == _abi.ERR_INVALID_ARG
        assert last_error(gpu_ctx) == "null planes"
        assert fn(gpu_ctx.handle, rp, n, C.byref(good), C.byref(none), *tail) == _abi.ERR_INVALID_ARG
        assert last_error(gpu_ctx) == "no plane asked for: all four pointers of c2rt_gather_planes are null"
    fresh = c2.Context(0)
    try:
        fn = L.c2rt_trace_rays_gather
        assert fn(fresh.handle, rp, n, C.byref(good), C.byref(pl)) == _abi.ERR_NO_SCENE and "no scene" in last_error(fresh)
        assert fn(fresh.handle, rp, n, None, None) == _abi.ERR_NO_SCENE                            # no scene before the options
        assert fn(fresh.handle, rp, _abi.MAX_RAYS + 1, C.byref(good), C.byref(pl)) == _abi.ERR_LIMIT  # the limit before the scene
        assert fn(fresh.handle, None, 0, None, None) == _abi.OK
    finally:
        fresh.close()
    assert untouched(bufs)
    assert raw_call(GATHER, gpu_ctx, bufs, rays=rays, n=n, options=good) == _abi.OK, last_error(gpu_ctx)
    check_filled(GATHER_PLANES, bufs, want, n, "after the refusals")
