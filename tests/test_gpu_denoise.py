"""The a-trous filter on the GPU (c2rt_denoise*, c2rt_render_paths_denoised).  The arithmetic is the contract: every output
is, BIT FOR BIT and with no pixel excused, what tests/denoise_reference.py makes of the same guides and input — the
context's own hit planes, path planes and occlusion planes of lecture5 and csg_stress, whose taps fall into every branch
of the filter (tests/test_denoise_abi.py counts them from the oracle alone), then synthetic frames for the shapes and
the edge cases.  Then the device variant against the host variant, the tie to the path planes' radiance, the one-call
frame and its mirror against the composition, and every refusal in the documented order."""
import ctypes as C
import itertools

import numpy as np
import pytest

import chess2rt_amd as c2
import denoise_reference as dr
import occlusion_cases as oc
import query_test_util as Q
from chess2rt_amd import _abi
from query_test_util import DeviceBytes, SENTINEL, last_error, lib
from ray_query_util import bits

pytestmark = pytest.mark.gpu

W, H, SEED = oc.W, oc.H, oc.SEED
P, B = 8, 2
GUARD = 256
_frames = {}


def frames(ctx, name):
    """uploads the scene and returns its planes at 61x47, rendered once and shared read-only: the guides (node, normal, p),
    rgb, albedo, the path planes' indirect and radiance (P = 8, B = 2), ao, and a seeded noise plane"""
    scene, cam, opts = oc.load(name)
    ctx.uploadScene(scene.desc)
    if name not in _frames:
        f = dict(ctx.renderHits(cam, opts, planes=("node", "normal", "p", "rgb")))
        f["albedo"] = ctx.renderShading(cam, opts, planes=("albedo",))["albedo"]
        f.update(ctx.renderPaths(cam, opts, P, B, seed=SEED, planes=("indirect", "radiance")))
        f["ao"] = ctx.renderOcclusion(cam, opts, oc.K, oc.RADIUS[name], seed=SEED, planes=("ao",))["ao"]
        f["noise"] = np.random.RandomState(SEED).uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
        for a in f.values():
            a.setflags(write=False)
        _frames[name] = f
    return _frames[name]


def both(ctx, g, image, what, **kw):
    """the host variant and the reference on the same inputs: the same bits (a NaN is any NaN)"""
    got = ctx.denoise(g, image, **kw)
    want = dr.denoise(g["node"], g["normal"], g["p"], image, kw.get("levels", 5), kw.get("normal_power_log2", 5), kw.get("sigma_plane", 1.0),
                      kw.get("sigma_colour", 0.0), albedo=kw.get("albedo"), base=kw.get("base"))
    assert got.shape == image.shape and got.dtype == np.float32
    n = dr.count_differing(got, want)
    assert n == 0, "%s: %d of %d values differ" % (what, n, want.size)
    return got


# ---- 1. bit for bit against the reference --------------------------------------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_scene_frames_match_the_reference(gpu_ctx, name):
    f = frames(gpu_ctx, name)
    assert np.isfinite(f["indirect"]).all() and (f["node"] < 0).sum() >= 50
    for src, levels, power, sc in itertools.product(("indirect", "noise"), (0, 1, 2, 5), (0, 5), (0.0, 0.5)):
        got = both(gpu_ctx, f, f[src], (name, src, levels, power, sc), levels=levels, normal_power_log2=power, sigma_colour=sc)
        assert bits(got).tobytes() == bits(dr.denoise(f["node"], f["normal"], f["p"], f[src], levels, power, 1.0, sc)).tobytes()   # no NaN to excuse
        if levels >= 2:
            assert dr.count_differing(got, f[src]) > got.size // 2                                    # the filter does something
    closing = (dict(), dict(albedo=f["albedo"]), dict(base=f["rgb"]), dict(albedo=f["albedo"], base=f["rgb"]))
    for kw, levels, sc in itertools.product(closing, (0, 1, 2, 5), (0.0, 0.5)):
        both(gpu_ctx, f, f["indirect"], (name, tuple(kw), levels, sc), levels=levels, sigma_colour=sc, **kw)


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_one_channel_ao_matches_the_reference(gpu_ctx, name):
    f = frames(gpu_ctx, name)
    assert f["ao"].shape == (H, W)
    for levels, power, sc in itertools.product((0, 1, 2, 5), (0, 5), (0.0, 0.5)):
        both(gpu_ctx, f, f["ao"], (name, "ao", levels, power, sc), levels=levels, normal_power_log2=power, sigma_colour=sc)
    both(gpu_ctx, f, f["ao"], (name, "ao closing"), levels=2, albedo=f["noise"][..., 0], base=f["noise"][..., 1])
    both(gpu_ctx, f, f["ao"].reshape(H, W, 1), (name, "ao, (H, W, 1)"), levels=3)


# ---- 2. the device variant ---------------------------------------------------------------------------------------------------


def test_device_variant_on_a_stream_behind_the_planes(gpu_ctx):
    """hit planes, path planes and the filter enqueued back to back on one non-default stream, no sync in between: the host
    variant's bits; the guards around `out` and the scratch keep the pattern; `in` and the guides are what was rendered"""
    name = "lecture5"
    f = frames(gpu_ctx, name)
    _, cam, opts = oc.load(name)
    hip = Q.hip_runtime()
    px = W * H
    levels, sc = 5, 0.5
    need = c2.denoise_scratch_bytes(W, H, 3, levels, 5, 1.0, sc)
    assert need == px * 44
    dev = {"node": DeviceBytes(px * 4), "normal": DeviceBytes(px * 24), "p": DeviceBytes(px * 24), "rgb": DeviceBytes(px * 12),
           "indirect": DeviceBytes(px * 12), "out": DeviceBytes(GUARD + px * 12 + GUARD), "scratch": DeviceBytes(GUARD + need + GUARD)}
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        at = {k: d.ptr.value for k, d in dev.items()}
        gpu_ctx.renderHitsDevice(cam, opts, {k: at[k] for k in ("node", "normal", "p", "rgb")}, stream=stream.value)
        gpu_ctx.renderPathsDevice(cam, opts, P, B, {"indirect": at["indirect"]}, seed=SEED, stream=stream.value)
        gpu_ctx.denoiseDevice({"node": at["node"], "normal": at["normal"], "p": at["p"], "base": at["rgb"]}, W, H, at["indirect"], at["out"] + GUARD,
                              at["scratch"] + GUARD, levels=levels, sigma_colour=sc, stream=stream.value)
        assert hip.hipStreamSynchronize(stream) == 0
        got = {k: d.get() for k, d in dev.items()}
    finally:
        assert hip.hipStreamDestroy(stream) == 0
        Q.free_all(dev)
    want = gpu_ctx.denoise(f, f["indirect"], levels=levels, sigma_colour=sc, base=f["rgb"])
    out = got["out"]
    assert (out[:GUARD] == SENTINEL).all() and (out[GUARD + px * 12:] == SENTINEL).all()
    assert out[GUARD:GUARD + px * 12].tobytes() == bits(want).tobytes()
    assert (got["scratch"][:GUARD] == SENTINEL).all() and (got["scratch"][GUARD + need:] == SENTINEL).all()
    assert not (got["scratch"][GUARD:GUARD + need] == SENTINEL).all()
    for k in ("node", "normal", "p", "rgb", "indirect"):
        assert got[k].tobytes() == bits(f[k]).tobytes(), k


def test_device_variant_no_level_needs_no_scratch(gpu_ctx):
    f = frames(gpu_ctx, "csg_stress")
    px = W * H
    assert c2.denoise_scratch_bytes(W, H, 3, 0) == 0
    dev = {k: DeviceBytes(bits(f[k]).nbytes) for k in ("node", "normal", "p", "albedo", "rgb", "indirect")}
    dev["out"] = DeviceBytes(px * 12 + GUARD)
    try:
        for k in ("node", "normal", "p", "albedo", "rgb", "indirect"):
            assert dev[k].hip.hipMemcpy(dev[k].ptr, bits(f[k]).ctypes.data, dev[k].nbytes, 1) == 0
        at = {k: d.ptr.value for k, d in dev.items()}
        gpu_ctx.denoiseDevice({"node": at["node"], "normal": at["normal"], "p": at["p"], "albedo": at["albedo"], "base": at["rgb"]}, W, H,
                              at["indirect"], at["out"], 0, levels=0)
        assert dev["out"].hip.hipDeviceSynchronize() == 0
        out = dev["out"].get()
    finally:
        Q.free_all(dev)
    assert out[:px * 12].tobytes() == bits(f["radiance"]).tobytes() and (out[px * 12:] == SENTINEL).all()


# ---- 3. shapes -----------------------------------------------------------------------------------------------------------------


def synthetic(h, w, seed, channels=3):
    """a few nodes in patches and misses among them, normals scattered about +z, points near a plane"""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    node = (((xs // 5) + 2 * (ys // 3)) % 3).astype(np.int32)
    node[rng.uniform(size=(h, w)) < 0.1] = -1
    normal = rng.uniform(-0.6, 0.6, (h, w, 3))
    normal[..., 2] = 1.0
    normal[rng.uniform(size=(h, w)) < 0.05] *= -1.0
    p = np.stack([xs * 0.25, ys * 0.25, rng.uniform(-0.5, 0.5, (h, w))], axis=-1)
    img = rng.uniform(0.0, 2.0, (h, w, channels)).astype(np.float32)
    return dict(node=node, normal=normal, p=p), img


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (3, 3), (64, 8), (65, 9), (130, 67)])
def test_shapes_and_steps_beyond_the_frame(gpu_ctx, w, h):
    g, img = synthetic(h, w, 100 * w + h)
    for levels in (1, 3, 8):
        both(gpu_ctx, g, img, (w, h, levels), levels=levels, normal_power_log2=1, sigma_colour=0.7, sigma_plane=0.5)
    both(gpu_ctx, g, img[..., 0], (w, h, "one channel"), levels=8, normal_power_log2=0)
    both(gpu_ctx, g, img, (w, h, "closing"), levels=8, normal_power_log2=3, albedo=img[::-1].copy(), base=img[:, ::-1].copy())


# ---- 4. edge cases -------------------------------------------------------------------------------------------------------------


def flat(h, w):
    ys, xs = np.mgrid[0:h, 0:w]
    normal = np.zeros((h, w, 3))
    normal[..., 2] = 1.0
    return dict(node=np.zeros((h, w), dtype=np.int32), normal=normal, p=np.stack([xs, ys, 0 * xs], axis=-1).astype(np.float64))


def test_normal_term_underflows_to_zero_and_to_a_subnormal(gpu_ctx):
    """power 7 is dn^128: dn = 0.5 gives 2^-128, a subnormal that must be kept (the weight counts), dn = 0.25 gives 2^-256,
    zero: the tap is dropped by !(w > 0)"""
    g = flat(9, 9)
    g["normal"][4, 3] = (np.sqrt(0.75), 0.0, 0.5)
    g["normal"][4, 5] = (np.sqrt(1.0 - 0.0625), 0.0, 0.25)
    img = np.random.RandomState(1).uniform(0, 1, (9, 9, 3)).astype(np.float32)
    img[4, 3] = 1e36                                                   # times 2^-128 * K: about 2e-4, visible in the centre's sum
    counts = {}
    want = dr.denoise(g["node"], g["normal"], g["p"], img, 1, 7, 1.0, counts=counts)
    assert counts["dropped"] > 0 and counts["soft"] > 0
    without = dict(g, node=g["node"].copy())
    without["node"][4, 3] = 1
    assert dr.count_differing(want[4, 4], dr.denoise(without["node"], g["normal"], g["p"], img, 1, 7, 1.0)[4, 4]) > 0   # the subnormal weight matters
    got = both(gpu_ctx, g, img, "underflow", levels=1, normal_power_log2=7)
    assert np.isfinite(got).all()


@pytest.mark.parametrize("sc", [0.0, 0.5])
def test_nan_and_infinite_colour_reach_what_the_reference_says(gpu_ctx, sc):
    g, img = synthetic(20, 33, 9)
    g["node"][8:12, 14:20] = 1
    img[10, 16] = (np.nan, np.inf, 1.0)
    got = both(gpu_ctx, g, img, ("nan colour", sc), levels=3, normal_power_log2=1, sigma_colour=sc)
    bad = ~np.isfinite(got)
    assert bad[10, 16].any()
    if sc > 0:
        assert bad.sum() == 2                                      # the colour term drops the tap everywhere else
    else:
        assert bad.sum() > 2 and not bad[g["node"] != 1].any()     # it spreads, on its own node only


def test_nan_normal_overflowing_p_and_misses_only(gpu_ctx):
    g, img = synthetic(20, 33, 10)
    g["normal"][5, 7] = np.nan
    g["p"][9, 20] = (1e300, 0.0, -1e300)
    g["p"][3, 3] = np.nan
    got = both(gpu_ctx, g, img, "nan guides", levels=4, normal_power_log2=2, sigma_colour=0.3)
    hit = g["node"] >= 0
    ok = np.ones_like(hit)
    ok[5, 7] = False
    assert np.isfinite(got[hit & ok]).all()
    g, img = synthetic(11, 13, 11)
    g["node"][:] = -1
    got = both(gpu_ctx, g, img, "misses only", levels=5)
    assert got.tobytes() == img.tobytes()
    got = both(gpu_ctx, g, img, "misses only, closing", levels=5, albedo=img, base=img)
    assert got.tobytes() == (img + img * img).tobytes()


# ---- 5. the tie ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_no_level_is_the_path_planes_radiance(gpu_ctx, name):
    f = frames(gpu_ctx, name)
    got = gpu_ctx.denoise(f, f["indirect"], levels=0, albedo=f["albedo"], base=f["rgb"])
    assert bits(got).tobytes() == bits(f["radiance"]).tobytes()


# ---- 6. the frame in one call -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_render_paths_denoised_is_the_composition(gpu_ctx, name):
    f = frames(gpu_ctx, name)
    scene, cam, opts = oc.load(name)
    for levels, sc in ((0, 0.0), (1, 0.0), (4, 0.5)):
        want = gpu_ctx.denoise(f, f["indirect"], levels=levels, sigma_colour=sc, albedo=f["albedo"], base=f["rgb"])
        got = gpu_ctx.renderPathsDenoised(cam, opts, P, B, seed=SEED, levels=levels, sigma_colour=sc)
        assert got.shape == (H, W, 3) and bits(got).tobytes() == bits(want).tobytes(), (name, levels, sc)
    mirror = c2.Renderer(scene, gpu_ctx).renderPathsDenoised(P, B, seed=SEED, levels=4, sigma_colour=0.5)
    assert bits(mirror).tobytes() == bits(want).tobytes()
    assert bits(f["radiance"]).tobytes() == bits(gpu_ctx.renderPathsDenoised(cam, opts, P, B, seed=SEED, levels=0)).tobytes()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------


def test_refusals_in_the_documented_order(gpu_ctx):
    """Every refusal of c2rt_denoise_device with every LATER violation present as well: the status and message are the
    first one's.  Nothing is enqueued: `out` and the scratch keep the pattern."""
    px = 8 * 8
    L = lib()
    dev = {k: DeviceBytes(n) for k, n in (("node", px * 4), ("normal", px * 24), ("p", px * 24), ("in", px * 12), ("out", px * 12), ("scratch", px * 44))}
    at = {k: d.ptr.value for k, d in dev.items()}
    good = dict(ctx=gpu_ctx.handle, opts=True, guides=True, width=8, height=8, channels=3, sigma_plane=1.0, sigma_colour=0.0, reserved=0, levels=5,
                normal_power_log2=5, node=at["node"], normal=at["normal"], p=at["p"], inp=at["in"], out=at["out"], scratch=at["scratch"])
    E, LIM = _abi.ERR_INVALID_ARG, _abi.ERR_LIMIT
    steps = [  # (fields that turn bad, status, word of the message)
        (dict(ctx=None), E, None),
        (dict(opts=False), E, "null denoise options"),
        (dict(guides=False), E, "null denoise guides"),
        (dict(width=0), E, "above 0"),
        (dict(channels=2), E, "channels"),
        (dict(sigma_plane=float("nan")), E, "sigma_plane"),
        (dict(sigma_colour=-1.0), E, "sigma_colour"),
        (dict(reserved=1), E, "reserved"),
        (dict(levels=9), LIM, "levels"),
        (dict(normal_power_log2=8), LIM, "normal_power_log2"),
        (dict(node=None), E, "node"),
        (dict(normal=None), E, "normal"),
        (dict(p=None), E, ": p"),
        (dict(inp=None), E, "null denoise input"),
        (dict(out=None), E, "null denoise output"),
        (dict(out=at["in"]), E, "output is the input"),
        (dict(out=at["scratch"]), E, "output is the scratch"),
        (dict(inp=at["scratch"]), E, "input is the scratch"),
        (dict(scratch=None), E, "null denoise scratch"),
        (dict(scratch=at["scratch"] + 4), E, "16-byte"),
    ]

    def call(v):
        o = _abi.DenoiseOpts(width=v["width"], height=v["height"], levels=v["levels"], channels=v["channels"], normal_power_log2=v["normal_power_log2"],
                             sigma_plane=v["sigma_plane"], sigma_colour=v["sigma_colour"], reserved=v["reserved"])
        g = _abi.DenoiseGuides(node=v["node"], normal=v["normal"], p=v["p"])
        return L.c2rt_denoise_device(v["ctx"], C.byref(g) if v["guides"] else None, C.byref(o) if v["opts"] else None, v["inp"], v["out"], v["scratch"], None)

    try:
        assert call(good) == _abi.OK, last_error(gpu_ctx)
        assert dev["out"].hip.hipDeviceSynchronize() == 0
        assert not (dev["scratch"].get() == SENTINEL).all()         # the valid call ran (its guides are all misses: out = in)
        for d in (dev["out"], dev["scratch"]):
            assert d.hip.hipMemset(d.ptr, SENTINEL, d.nbytes) == 0
        for i, (_, status, word) in enumerate(steps):
            v = dict(good)
            later = steps[i:] if i < 15 else steps[i:i + 1]          # the pointer identities exclude one another
            for bad, _, _ in reversed(later):
                v.update(bad)
            if i in (13, 14):                                          # a null pointer equals no other
                v.update(scratch=at["scratch"])
            assert call(v) == status, (i, word, last_error(gpu_ctx))
            if word:
                assert word in last_error(gpu_ctx), (i, word, last_error(gpu_ctx))
        assert dev["out"].hip.hipDeviceSynchronize() == 0
        assert (dev["out"].get() == SENTINEL).all() and (dev["scratch"].get() == SENTINEL).all()
        for k in ("node", "normal", "p", "in"):
            assert (dev[k].get() == SENTINEL).all()
    finally:
        Q.free_all(dev)


def test_refusals_of_the_host_variant_and_of_the_frame_call(gpu_ctx):
    f = frames(gpu_ctx, "lecture5")
    _, cam, opts = oc.load("lecture5")
    L = lib()
    out = Q.sentinel_bytes(W * H * 12)
    img = np.ascontiguousarray(f["indirect"])
    g = _abi.DenoiseGuides(node=f["node"].ctypes.data, normal=f["normal"].ctypes.data, p=f["p"].ctypes.data)

    def o(**kw):
        v = dict(width=W, height=H, levels=3, channels=3, normal_power_log2=5, sigma_plane=1.0, sigma_colour=0.0, reserved=0)
        v.update(kw)
        return _abi.DenoiseOpts(**v)

    for opt, inp, outp, status, word in ((o(height=0), img.ctypes.data, out.ctypes.data, _abi.ERR_INVALID_ARG, "above 0"),
                                         (o(sigma_plane=0.0), img.ctypes.data, out.ctypes.data, _abi.ERR_INVALID_ARG, "sigma_plane"),
                                         (o(sigma_colour=float("inf")), img.ctypes.data, out.ctypes.data, _abi.ERR_INVALID_ARG, "sigma_colour"),
                                         (o(levels=9), img.ctypes.data, out.ctypes.data, _abi.ERR_LIMIT, "levels"),
                                         (o(), None, out.ctypes.data, _abi.ERR_INVALID_ARG, "input"),
                                         (o(), img.ctypes.data, None, _abi.ERR_INVALID_ARG, "output"),
                                         (o(), img.ctypes.data, img.ctypes.data, _abi.ERR_INVALID_ARG, "is the input")):
        assert L.c2rt_denoise(gpu_ctx.handle, C.byref(g), C.byref(opt), inp, outp) == status, word
        assert word in last_error(gpu_ctx)
    pg = _abi.PathOpts(seed=SEED, paths=P, bounces=B)
    strips = Q.with_fields(opts, strip_world=2, strip_height=8)
    for cam_, opts_, pg_, d, outp, status, word in ((cam, opts, Q.with_fields(pg, paths=0), o(), out.ctypes.data, _abi.ERR_INVALID_ARG, "paths"),
                                                    (cam, opts, pg, None, out.ctypes.data, _abi.ERR_INVALID_ARG, "null denoise options"),
                                                    (cam, opts, pg, o(), None, _abi.ERR_INVALID_ARG, "null output"),
                                                    (Q.with_fields(cam, stereo_separation=0.1), opts, pg, o(), out.ctypes.data, _abi.ERR_UNSUPPORTED, "stereo"),
                                                    (cam, strips, pg, o(), out.ctypes.data, _abi.ERR_UNSUPPORTED, "strip_world"),
                                                    (cam, opts, pg, o(width=W + 1), out.ctypes.data, _abi.ERR_INVALID_ARG, "the frame has"),
                                                    (cam, opts, pg, o(channels=1), out.ctypes.data, _abi.ERR_INVALID_ARG, "a frame has 3"),
                                                    (cam, opts, pg, o(normal_power_log2=8), out.ctypes.data, _abi.ERR_LIMIT, "normal_power_log2")):
        st = L.c2rt_render_paths_denoised(gpu_ctx.handle, C.byref(cam_), C.byref(opts_), C.byref(pg_), None if d is None else C.byref(d), outp)
        assert st == status, (word, last_error(gpu_ctx))
        assert word in last_error(gpu_ctx), (word, last_error(gpu_ctx))
    assert Q.untouched([out])
