"""Occlusion planes on the GPU (c2rt_render_occlusion*, c2rt_trace_rays_occlusion*).  Composition is the contract: the
planes are, BIT FOR BIT and with no sample excused, what tests/occlusion_reference.py makes of the context's own records
(c2rt_trace_rays) and of the context's own answers (c2rt_test_visibility) for the segments the reference builds; those
answers also equal the oracle's.  Then the camera call against the ray call, strips, sample counts, plane subsets,
seeds, misses and garbage, the host variants' chunks, a posed scene, the mirrors, and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import chess2rt_amd as c2
import occlusion_cases as oc
import occlusion_reference as ocr
import query_test_util as Q
import scene_update_util as U
from chess2rt_amd import _abi
from chess2rt_amd.api import OCCLUSION_PLANES
from query_test_util import OCCLUSION, check_device_against_host, check_filled, device_planes, guarded, last_error, lib, raw_call, struct_of, untouched
from query_test_util import occlusion_options as occ_opts
from ray_query_util import bits, oracle_visibility

pytestmark = pytest.mark.gpu

W, H, K, SEED = oc.W, oc.H, oc.K, oc.SEED
PLANES = tuple(OCCLUSION_PLANES)
_cases = {}
same_planes = functools.partial(Q.same_planes, names=PLANES)


def composed(ctx, rays, samples, radius, seed, idx=None):
    """the planes by composition on the context's own single-purpose queries; also (records, hit, segments, answers)"""
    rec, _ = ctx.traceRays(rays, colors=False)
    idx = np.arange(len(rays)) if idx is None else idx
    hit, res, seg, _ = ocr.samples(rec, rays[:, 3:], idx, samples, radius, seed)
    vis = np.zeros((len(rays), samples), dtype=np.uint8)
    ask = np.ascontiguousarray(seg[hit].reshape(-1, 6))
    got = ctx.testVisibility(ask) if len(ask) else np.zeros(0, dtype=np.uint8)
    vis[hit] = got.reshape(-1, samples)
    return ocr.planes(rec, res, vis, samples), (rec, hit, ask, got)


def case(gpu_ctx, name):
    """uploads the scene and returns {ray set: (rays, planes of the fused call, planes by composition, (records, hit,
    segments, answers))} — the queries run once per scene and are shared by the tests below (read-only)"""
    scene, _, _ = oc.load(name)
    gpu_ctx.uploadScene(scene.desc)
    if name not in _cases:
        out = {}
        for which in oc.RAY_SETS:
            rays = oc.ray_set(name, which)
            got = gpu_ctx.traceRaysOcclusion(rays, K, oc.RADIUS[name], SEED)
            want, parts = composed(gpu_ctx, rays, K, oc.RADIUS[name], SEED)
            out[which] = (rays, got, want, parts)
        _cases[name] = out
    return _cases[name]


# ---- 4: composition ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_planes_are_the_composition_of_the_contexts_own_queries(gpu_ctx, name):
    scene, _, _ = oc.load(name)
    for which, (rays, got, want, (rec, hit, ask, answers)) in case(gpu_ctx, name).items():
        what = "%s %s" % (name, which)
        assert set(got) == set(PLANES)
        for p in PLANES:
            dtype, comps = OCCLUSION_PLANES[p]
            assert got[p].dtype == dtype and got[p].shape == ((len(rays),) if comps == 1 else (len(rays), comps)), (what, p)
        mixed, full, empty = ocr.mask_kinds(got["open"], hit, K)
        print("%s: %d rays, %d hits, %d mixed, %d full, %d empty masks" % (what, len(rays), int(hit.sum()), mixed, full, empty))
        same_planes(got, want, what)
        assert np.array_equal(got["node"], rec["closest_node"]), what
        # the answers the masks are made of are the oracle's for the same segments
        assert np.array_equal(answers, oracle_visibility(scene.desc, ask)), "%s: visibility differs from the oracle" % what
        assert mixed >= 100 and (which != "eyeless" or empty >= 1), what


# ---- 5: the camera call is the ray call on the frame's screen rays; strips ------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_camera_call_equals_ray_call_and_strips(gpu_ctx, name):
    scene, cam, opts = oc.load(name)
    rays, want, _, _ = case(gpu_ctx, name)["screen"]
    full = gpu_ctx.renderOcclusion(cam, opts, K, oc.RADIUS[name], SEED)
    for p in PLANES:
        assert full[p].shape[:2] == (H, W), p
    same_planes(full, want, "%s frame against its screen rays" % name)
    # opts.seed is ignored, as the hit planes ignore it
    other = _abi.RenderOpts.from_buffer_copy(opts)
    other.seed = 99
    same_planes(gpu_ctx.renderOcclusion(cam, other, K, oc.RADIUS[name], SEED), full, "%s opts.seed" % name)
    Q.check_strips(gpu_ctx, scene, lambda o: gpu_ctx.renderOcclusion(cam, o, K, oc.RADIUS[name], SEED), full, H, 3, 8, PLANES, name)


# ---- 6: sample counts --------------------------------------------------------------------------------------------------


def popcount(a):
    return np.array([bin(int(x)).count("1") for x in np.asarray(a).reshape(-1)], dtype=np.int64)


def test_sample_counts(gpu_ctx):
    name = "lecture5"
    rays, _, _, (rec, hit, _, _) = case(gpu_ctx, name)["screen"]
    radius = oc.RADIUS[name]
    p64 = gpu_ctx.traceRaysOcclusion(rays, 64, radius, SEED)
    assert (p64["open"][~hit] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (~hit).any()
    assert ((p64["open"][hit] >> np.uint64(63)) & np.uint64(1)).any()                 # the last bit is reached
    want64, _ = composed(gpu_ctx, rays, 64, radius, SEED)
    same_planes(p64, want64, "K = 64")
    for k in (1, 31, 32, 33, 64):
        low = np.uint64((1 << k) - 1)
        got = p64 if k == 64 else gpu_ctx.traceRaysOcclusion(rays, k, radius, SEED)
        assert not (got["open"] & ~low).any(), k                                     # bits at and above K are zero
        assert np.array_equal(got["open"][hit], p64["open"][hit] & low), k
        assert (got["open"][~hit] == low).all(), k
        want_ao = popcount(got["open"]).astype(np.float32) / np.float32(k)
        assert got["ao"].tobytes() == want_ao.tobytes(), k
        if k in (1, 33):
            same_planes(got, composed(gpu_ctx, rays, k, radius, SEED)[0], "K = %d" % k)


# ---- 7: plane independence and seeds ---------------------------------------------------------------------------------------


def test_plane_independence_and_seeds(gpu_ctx):
    name = "csg_stress"
    scene, cam, opts = oc.load(name)
    c = case(gpu_ctx, name)
    rays, full_rays = c["eyeless"][0], c["eyeless"][1]
    radius = oc.RADIUS[name]
    full = gpu_ctx.renderOcclusion(cam, opts, K, radius, SEED)
    subsets = [(p,) for p in PLANES] + [("open", "bent"), ("node", "ao")]
    Q.check_plane_subsets(OCCLUSION, gpu_ctx, cam, opts, rays, occ_opts(K, radius, SEED), subsets, full, full_rays, W * H, name, align=8)
    hits = gpu_ctx.renderHits(cam, opts, planes=("node",))
    alone = gpu_ctx.renderOcclusion(cam, opts, K, radius, SEED, planes=("node",))
    assert list(alone) == ["node"] and bits(alone["node"]).tobytes() == bits(hits["node"]).tobytes()
    with pytest.raises(ValueError):
        gpu_ctx.renderOcclusion(cam, opts, K, radius, SEED, planes=("depth",))
    # the same seed: the same planes; another seed: other directions
    same_planes(gpu_ctx.traceRaysOcclusion(rays, K, radius, SEED), full_rays, "second call")
    other = gpu_ctx.traceRaysOcclusion(rays, K, radius, SEED + 1)
    assert np.array_equal(other["node"], full_rays["node"])
    changed = int((other["open"] != full_rays["open"]).sum())
    print("seed %d -> %d: %d of %d masks change" % (SEED, SEED + 1, changed, len(rays)))
    assert changed >= 100
    same_planes(other, composed(gpu_ctx, rays, K, radius, SEED + 1)[0], "seed + 1")
    big = (1 << 40) + 5                                                  # the seed's high word reaches the key
    same_planes(gpu_ctx.traceRaysOcclusion(rays[:256], K, radius, big), composed(gpu_ctx, rays[:256], K, radius, big)[0], "64-bit seed")


# ---- 8: misses and bad rays ------------------------------------------------------------------------------------------------


def test_misses_and_garbage_rays(gpu_ctx):
    name = "lecture5"
    rays0, want, _, (rec, hit, _, _) = case(gpu_ctx, name)["eyeless"]
    miss = ~hit
    assert miss.sum() >= 100
    assert (want["node"][miss] == -1).all() and (want["open"][miss] == np.uint64((1 << K) - 1)).all()
    assert want["ao"][miss].tobytes() == np.ones(int(miss.sum()), dtype=np.float32).tobytes()
    assert not want["bent"][miss].view(np.uint64).any()                   # +0, +0, +0
    Q.check_garbage_lanes(lambda rays: gpu_ctx.traceRaysOcclusion(rays, K, oc.RADIUS[name], SEED), rays0, want, hit, PLANES, "open", K)


# ---- 9: host variants ------------------------------------------------------------------------------------------------------


def test_host_variants_equal_the_device_variants(gpu_ctx):
    import torch

    name = "lecture5"
    scene, cam, opts = oc.load(name)
    base = case(gpu_ctx, name)["screen"]
    radius = oc.RADIUS[name]
    dev = torch.device("cuda:0")
    s1 = torch.cuda.Stream(dev)
    # the frame at 61x47
    host = gpu_ctx.renderOcclusion(cam, opts, K, radius, SEED)
    t = device_planes(OCCLUSION_PLANES, W * H, dev, guard_bytes=64)
    torch.cuda.synchronize()
    gpu_ctx.renderOcclusionDevice(cam, opts, K, radius, {k: v.data_ptr() for k, v in t.items()}, seed=SEED, stream=s1.cuda_stream)
    s1.synchronize()
    check_device_against_host(OCCLUSION_PLANES, t, host, W * H, "61x47")
    # 2^18 + 70 rays, K = 2: the second chunk starts at a non-zero index, and its rays draw the samples of THEIR index
    n = (1 << 18) + 70
    reps = np.arange(n) % len(base[0])
    rays = np.ascontiguousarray(base[0][reps])
    host = gpu_ctx.traceRaysOcclusion(rays, 2, radius, SEED)
    t = device_planes(OCCLUSION_PLANES, n, dev, guard_bytes=64)
    rays_t = torch.from_numpy(rays).to(dev)
    torch.cuda.synchronize()
    gpu_ctx.traceRaysOcclusionDevice(rays_t.data_ptr(), n, 2, radius, {k: v.data_ptr() for k, v in t.items()}, seed=SEED, stream=s1.cuda_stream)
    s1.synchronize()
    check_device_against_host(OCCLUSION_PLANES, t, host, n, "2^18 + 70 rays")
    assert np.array_equal(host["node"], base[1]["node"][reps])
    # the tail behind the chunk boundary against the composition at its own indices; a copy of a ray elsewhere in the
    # array draws other directions
    tail = np.arange((1 << 18) - 30, n)
    want, _ = composed(gpu_ctx, rays[tail], 2, radius, SEED, idx=tail)
    for p in PLANES:
        assert bits(host[p][tail]).tobytes() == bits(want[p]).tobytes(), p
    first = np.arange(len(base[0]))
    assert (host["open"][first] != host["open"][first + len(base[0])]).any()


# ---- 10: a posed scene and the mirrors -----------------------------------------------------------------------------------------


def test_posed_scene_and_mirrors(gpu_ctx):
    name = "lecture5"
    scene, cam, opts = oc.load(name)
    rays, before, _, _ = case(gpu_ctx, name)["screen"]
    radius = oc.RADIUS[name]
    frame = gpu_ctx.renderOcclusion(cam, opts, K, radius, SEED)
    # Renderer.renderOcclusion and the host mirror are the Context call for the scene's own camera
    got = c2.Renderer(scene, gpu_ctx).renderOcclusion(K, radius, SEED)
    assert set(got) == set(PLANES)
    same_planes(got, frame, "Renderer.renderOcclusion")
    sub = c2.Renderer(scene, gpu_ctx).renderOcclusion(K, radius, SEED, planes=("ao",))
    assert list(sub) == ["ao"] and bits(sub["ao"]).tobytes() == bits(frame["ao"]).tobytes()
    raw = guarded(OCCLUSION_PLANES, PLANES, W * H, align=8)
    pl, occ = struct_of(_abi.OcclusionPlanes, raw), occ_opts(K, radius, SEED)
    assert lib().c2rt_host_render_occlusion(gpu_ctx.handle, scene._h, C.byref(occ), C.byref(pl)) == _abi.OK, last_error(gpu_ctx)
    check_filled(OCCLUSION_PLANES, raw, frame, W * H, "c2rt_host_render_occlusion")
    # a ball moves: the call sees the posed scene
    gpu_ctx.uploadScene(scene.desc)
    gpu_ctx.updateScene({3: U.xf(("translate", 60, 15, 200))})
    try:
        posed = gpu_ctx.traceRaysOcclusion(rays, K, radius, SEED)
        want, (rec, hit, _, _) = composed(gpu_ctx, rays, K, radius, SEED)
        same_planes(posed, want, "posed")
        same_planes(gpu_ctx.renderOcclusion(cam, opts, K, radius, SEED), want, "posed frame")
        assert int((posed["open"] != before["open"]).sum()) >= 30 and not np.array_equal(posed["node"], before["node"])
    finally:
        gpu_ctx.uploadScene(scene.desc)


# ---- 11: refusals ------------------------------------------------------------------------------------------------------------


BAD_OCC = [  # (options, status, the whole message), in the documented order
    (dict(radius=float("nan")), _abi.ERR_INVALID_ARG, "occlusion radius nan: a finite length above 0"),
    (dict(radius=float("inf")), _abi.ERR_INVALID_ARG, "occlusion radius inf: a finite length above 0"),
    (dict(radius=0.0), _abi.ERR_INVALID_ARG, "occlusion radius 0: a finite length above 0"),
    (dict(radius=-1.0), _abi.ERR_INVALID_ARG, "occlusion radius -1: a finite length above 0"),
    (dict(samples=0), _abi.ERR_INVALID_ARG, "occlusion samples is 0: at least one sample"),
    (dict(reserved=1), _abi.ERR_INVALID_ARG, "c2rt_occlusion_opts.reserved is 1: must be 0"),
    (dict(samples=65), _abi.ERR_LIMIT, "65 occlusion samples (at most 64)"),
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

    bufs = guarded(OCCLUSION_PLANES, PLANES, n, align=8)
    pl, none = struct_of(_abi.OcclusionPlanes, bufs), _abi.OcclusionPlanes()
    good = occ_opts(K, oc.RADIUS[name], SEED)
    dof = copy_cam(dof=1, num_samples=4)

    def both(c, o, occ, planes):
        """the host and the device variant decide the same before anything is enqueued (the pointers are never used)"""
        a = (None if c is None else C.byref(c), C.byref(o), None if occ is None else C.byref(occ), None if planes is None else C.byref(planes))
        st = L.c2rt_render_occlusion(gpu_ctx.handle, *a)
        msg = last_error(gpu_ctx)
        assert L.c2rt_render_occlusion_device(gpu_ctx.handle, *a, None) == st and last_error(gpu_ctx) == msg
        return st, msg

    # a frame call's own statuses come first, in c2rt_render_hits' order
    assert both(None, opts, good, pl)[0] == _abi.ERR_INVALID_ARG
    st, msg = both(cam, copy_opts(width=0), None, None)
    hp = _abi.HitPlanes(node=bufs["node"].ctypes.data)
    assert st == L.c2rt_render_hits(gpu_ctx.handle, C.byref(cam), C.byref(copy_opts(width=0)), C.byref(hp)) != _abi.OK and msg == last_error(gpu_ctx)
    # then the options, each with its own message
    st, msg = both(cam, opts, None, pl)
    assert st == _abi.ERR_INVALID_ARG and msg == "null occlusion options"
    for kw, status, text in BAD_OCC:
        st, msg = both(cam, opts, occ_opts(**{**dict(samples=K, radius=oc.RADIUS[name]), **kw}), pl)
        assert st == status and msg == text, (kw, st, msg)
    # two rules at once: the radius before the samples, samples == 0 and reserved before the limit, the options before
    # the planes, the planes before the modes
    assert both(cam, opts, occ_opts(samples=0, radius=-1.0), pl)[1] == "occlusion radius -1: a finite length above 0"
    assert both(cam, opts, occ_opts(samples=65, radius=0.0), pl)[0] == _abi.ERR_INVALID_ARG
    st, msg = both(cam, opts, occ_opts(samples=65, reserved=3), pl)
    assert st == _abi.ERR_INVALID_ARG and msg == "c2rt_occlusion_opts.reserved is 3: must be 0"
    assert both(cam, opts, occ_opts(samples=65), None)[0] == _abi.ERR_LIMIT
    assert both(cam, opts, None, None)[1] == "null occlusion options"
    st, msg = both(cam, opts, good, None)
    assert st == _abi.ERR_INVALID_ARG and msg == "null planes"
    st, msg = both(cam, opts, good, none)
    assert st == _abi.ERR_INVALID_ARG and msg == "no plane asked for: all four pointers of c2rt_occlusion_planes are null"
    assert both(dof, opts, good, none)[0] == _abi.ERR_INVALID_ARG
    assert both(dof, opts, occ_opts(samples=65), pl)[0] == _abi.ERR_LIMIT
    # then the modes in which a pixel is not one ray
    for c, o, cause in [(dof, opts, "depth of field: a pixel's occlusion is one ray's, a lens has many per pixel"),
                        (copy_cam(stereo_separation=0.5), opts, "stereo: a pixel's occlusion is one ray's, a stereo camera has two per pixel"),
                        (cam, copy_opts(count_rays=1), "count_rays: the occlusion planes do not count rays"),
                        (cam, copy_opts(prepass_bucket=48), "prepass_bucket: a preview's pixels share the sample of their block")]:
        st, msg = both(c, o, good, pl)
        assert st == _abi.ERR_UNSUPPORTED and msg == cause, (cause, st, msg)
    assert both(copy_cam(dof=1, num_samples=4, stereo_separation=0.5), copy_opts(count_rays=1), good, pl)[1] == "depth of field: a pixel's occlusion is one ray's, a lens has many per pixel"
    fresh = c2.Context(0)
    try:
        a = (C.byref(cam), C.byref(opts))
        assert L.c2rt_render_occlusion(fresh.handle, *a, C.byref(good), C.byref(pl)) == _abi.ERR_NO_SCENE and "no scene" in last_error(fresh)
        assert L.c2rt_render_occlusion(fresh.handle, *a, None, None) == _abi.ERR_NO_SCENE          # the frame checks come first
    finally:
        fresh.close()
    assert untouched(bufs)
    # afterwards the same context fills a correct plane set
    assert raw_call(OCCLUSION, gpu_ctx, bufs, cam, opts, options=good) == _abi.OK, last_error(gpu_ctx)
    check_filled(OCCLUSION_PLANES, bufs, want, n, "after the refusals")


def test_ray_refusals_leave_the_outputs_untouched(gpu_ctx):
    name = "lecture5"
    rays, want, _, _ = case(gpu_ctx, name)["eyeless"]
    n = len(rays)
    bufs = guarded(OCCLUSION_PLANES, PLANES, n, align=8)
    L = lib()
    pl, none = struct_of(_abi.OcclusionPlanes, bufs), _abi.OcclusionPlanes()
    good = occ_opts(K, oc.RADIUS[name], SEED)
    bad = occ_opts(samples=0, radius=-1.0, reserved=9)
    rp = rays.ctypes.data_as(C.c_void_p)
    for fn, tail in ((L.c2rt_trace_rays_occlusion, ()), (L.c2rt_trace_rays_occlusion_device, (None,))):
        assert fn(None, rp, n, C.byref(good), C.byref(pl), *tail) == _abi.ERR_INVALID_ARG          # null context
        assert fn(gpu_ctx.handle, None, 0, None, None, *tail) == _abi.OK                           # n == 0, whatever else
        assert fn(gpu_ctx.handle, None, 0, C.byref(bad), C.byref(none), *tail) == _abi.OK
        assert fn(gpu_ctx.handle, None, n, None, None, *tail) == _abi.ERR_INVALID_ARG              # null rays before the options
        assert "null input array" in last_error(gpu_ctx)
        assert fn(gpu_ctx.handle, rp, _abi.MAX_RAYS + 1, None, None, *tail) == _abi.ERR_LIMIT      # the limit before the options
        assert "rays in one call" in last_error(gpu_ctx)
        assert fn(gpu_ctx.handle, rp, n, None, C.byref(pl), *tail) == _abi.ERR_INVALID_ARG
        assert last_error(gpu_ctx) == "null occlusion options"
        for kw, status, text in BAD_OCC:
            occ = occ_opts(**{**dict(samples=K, radius=oc.RADIUS[name]), **kw})
            assert fn(gpu_ctx.handle, rp, n, C.byref(occ), C.byref(pl), *tail) == status and last_error(gpu_ctx) == text, (kw, last_error(gpu_ctx))
        assert fn(gpu_ctx.handle, rp, n, C.byref(bad), None, *tail) == _abi.ERR_INVALID_ARG and last_error(gpu_ctx) == "occlusion radius -1: a finite length above 0"
        assert fn(gpu_ctx.handle, rp, n, C.byref(occ_opts(samples=65)), None, *tail) == _abi.ERR_LIMIT   # the options before the planes
        assert fn(gpu_ctx.handle, rp, n, C.byref(good), None, *tail) == _abi.ERR_INVALID_ARG
        assert last_error(gpu_ctx) == "null planes"
        assert fn(gpu_ctx.handle, rp, n, C.byref(good), C.byref(none), *tail) == _abi.ERR_INVALID_ARG
        assert last_error(gpu_ctx) == "no plane asked for: all four pointers of c2rt_occlusion_planes are null"
    fresh = c2.Context(0)
    try:
        fn = L.c2rt_trace_rays_occlusion
        assert fn(fresh.handle, rp, n, C.byref(good), C.byref(pl)) == _abi.ERR_NO_SCENE and "no scene" in last_error(fresh)
        assert fn(fresh.handle, rp, n, None, None) == _abi.ERR_NO_SCENE                            # no scene before the options
        assert fn(fresh.handle, rp, _abi.MAX_RAYS + 1, C.byref(good), C.byref(pl)) == _abi.ERR_LIMIT  # the limit before the scene
        assert fn(fresh.handle, None, 0, None, None) == _abi.OK
    finally:
        fresh.close()
    assert untouched(bufs)
    assert raw_call(OCCLUSION, gpu_ctx, bufs, rays=rays, n=n, options=good) == _abi.OK, last_error(gpu_ctx)
    check_filled(OCCLUSION_PLANES, bufs, want, n, "after the refusals")
