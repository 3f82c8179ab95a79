"""The temporal accumulation on the GPU (c2rt_temporal_accumulate*, c2rt_render_paths_sequence).  The arithmetic is the
contract: every plane and the whole history are, BIT FOR BIT and with no pixel excused (a NaN equal to any NaN), what
tests/temporal_reference.py makes of the same guides, input, camera and history — over four-frame camera sequences of
lecture5 and csg_stress whose pixels and taps fall into every class of the reprojection (tests/test_temporal_abi.py counts
them from the oracle alone), then synthetic frames for the shapes and the edge values.  Then the device variant against
the host variant, a tie to the plain mean that does not go through the reference, the sequence call against the
composition, and every refusal in the documented order."""
import ctypes as C
import itertools

import numpy as np
import pytest

import chess2rt_amd as c2
import occlusion_cases as oc
import query_test_util as Q
import temporal_cases as tc
import temporal_reference as tr
from chess2rt_amd import _abi
from query_test_util import DeviceBytes, SENTINEL, last_error, lib
from ray_query_util import bits

pytestmark = pytest.mark.gpu

W, H, SEED = tc.W, tc.H, oc.SEED
P, B = 8, 2
GUARD = 256
OPTS = dict(min_normal_dot=tc.MIN_NORMAL_DOT, max_plane_dist=tc.MAX_PLANE_DIST)
_frames = {}


def frames(ctx, name):
    """uploads the scene and returns, for each camera of its sequence, the planes at 61x47, rendered once and shared
    read-only: the guides (node, normal, p), rgb, albedo, the path planes' indirect (P = 8, B = 2, seed + i) and ao"""
    scene, cams, opts = tc.sequence(name)
    ctx.uploadScene(scene.desc)
    if name not in _frames:
        out = []
        for i, cam in enumerate(cams):
            f = dict(ctx.renderHits(cam, opts, planes=("node", "normal", "p", "rgb")))
            f["albedo"] = ctx.renderShading(cam, opts, planes=("albedo",))["albedo"]
            f["indirect"] = ctx.renderPaths(cam, opts, P, B, seed=SEED + i, planes=("indirect",))["indirect"]
            f["ao"] = ctx.renderOcclusion(cam, opts, oc.K, oc.RADIUS[name], seed=SEED + i, planes=("ao",))["ao"]
            for a in f.values():
                a.setflags(write=False)
            out.append(f)
        _frames[name] = out
    return _frames[name]


def both(ctx, g, image, what, prev_cam=None, history=None, counts=None, **kw):
    """the host variant and the reference on the same inputs: the same bits in every plane and in the history"""
    got, hist = ctx.temporalAccumulate(g, image, prev_cam=prev_cam, history=history, **kw)
    want = tr.accumulate(g["node"], g["normal"], g["p"], image, kw["max_age"], kw["min_normal_dot"], kw["max_plane_dist"], prev_cam=prev_cam,
                         history=history, counts=counts)
    h, w = g["node"].shape
    ch = 1 if image.ndim == 2 else image.shape[2]
    assert got["colour"].shape == image.shape and got["colour"].dtype == np.float32 and got["variance"].shape == (h, w) and got["age"].dtype == np.uint32
    n = tr.count_differing(got["colour"], want["colour"])
    assert n == 0, "%s: %d of %d colour values differ" % (what, n, image.size)
    n = tr.count_differing(got["variance"], want["variance"])
    assert n == 0, "%s: %d of %d variances differ" % (what, n, h * w)
    assert np.array_equal(got["age"], want["age"]), what
    assert hist.dtype == np.uint8 and hist.size == c2.temporal_history_bytes(w, h, ch)
    n = tr.history_differing(hist, want["history"], h, w, ch)
    assert n == 0, "%s: %d values of the history differ" % (what, n)
    return got, hist


# ---- 1. real sequences, bit for bit against the reference ----------------------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_scene_sequences_match_the_reference(gpu_ctx, name):
    fs = frames(gpu_ctx, name)
    _, cams, _ = tc.sequence(name)
    assert all(np.isfinite(f["indirect"]).all() for f in fs)
    for plane, max_age in itertools.product(("indirect", "ao"), (1, 3, 65535)):
        hist, counts = None, {}
        for i, f in enumerate(fs):
            got, hist = both(gpu_ctx, f, f[plane], (name, plane, max_age, i), prev_cam=cams[i - 1] if i else None, history=hist, counts=counts,
                             max_age=max_age, **OPTS)
            assert not np.isnan(got["colour"]).any()                                                     # no NaN to excuse
            assert got["age"].max() == min(i + 1, max_age) and (got["age"][f["node"] < 0] == 0).all()
        for k in ("full", "partial", "disoccluded", "outside", "miss", "first", "tap_other", "tap_normal", "tap_plane"):
            assert counts[k] >= 50, (k, counts)
        if max_age > 1:
            assert got["variance"].max() > 0


# ---- 2. shapes -----------------------------------------------------------------------------------------------------------------


def camera_struct(pos, up_left, up_right, down_left):
    cam = _abi.CameraFrame()
    for name, v in (("pos", pos), ("up_left", up_left), ("up_right", up_right), ("down_left", down_left)):
        setattr(cam, name, (C.c_double * 3)(*[float(x) for x in v]))
    return cam


def sheared_camera():
    pos = np.array([0.5, -0.25, 0.125])
    return camera_struct(pos, pos + (-1.1, 0.9, 1.0), pos + (1.0, 1.0, 1.2), pos + (-0.9, -1.0, 0.9))


def synthetic(h, w, seed, cam, jitter, channels=3):
    """guides whose points lie where `cam` sees its pixels (x + dx, y + dy), |dx|, |dy| <= jitter, at depths about 5: a few
    nodes in patches and misses among them, normals scattered about one direction, some turned round"""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    node = (((xs // 5) + 2 * (ys // 3)) % 3).astype(np.int32)
    node[rng.uniform(size=(h, w)) < 0.1] = -1
    normal = rng.uniform(-0.25, 0.25, (h, w, 3))
    normal[..., 2] = -1.0
    normal[rng.uniform(size=(h, w)) < 0.05] *= -1.0
    pos, ul, ur, dl = (np.array(list(getattr(cam, k))) for k in ("pos", "up_left", "up_right", "down_left"))
    sx = (xs + rng.uniform(-jitter, jitter, (h, w)))[..., None]
    sy = (ys + rng.uniform(-jitter, jitter, (h, w)))[..., None]
    depth = rng.uniform(4.9, 5.1, (h, w))[..., None]
    p = pos + depth * ((ul - pos) + (ur - ul) * (sx / w) + (dl - ul) * (sy / h))
    img = rng.uniform(0.0, 2.0, (h, w, channels)).astype(np.float32)
    return dict(node=node, normal=normal, p=p), img


@pytest.mark.parametrize("w,h", [(1, 1), (63, 1), (1, 70), (65, 2), (8, 8), (130, 9), (61, 47)])
def test_shapes_on_synthetic_guides_with_a_sheared_previous_camera(gpu_ctx, w, h):
    cam = sheared_camera()
    kw = dict(max_age=4, min_normal_dot=0.8, max_plane_dist=0.2)
    for channels in (3, 1):
        hist, counts = None, {}
        for i in range(3):
            g, img = synthetic(h, w, 1000 * w + 10 * h + i, cam, 0.0 if i == 0 else 1.5, channels)
            _, hist = both(gpu_ctx, g, img if channels == 3 else img[..., 0], (w, h, channels, i), prev_cam=cam if i else None, history=hist, counts=counts, **kw)
        if (w, h) == (61, 47):
            for k in ("miss", "first", "outside", "disoccluded", "partial", "full", "tap_outside", "tap_other", "tap_normal", "tap_plane", "tap_kept"):
                assert counts[k] >= 20, (k, counts)


# ---- 3. edge values --------------------------------------------------------------------------------------------------------------


def axis_camera(w, h):
    """pixel (i, j) looks through (i, j, 1) from the origin: a point (sx, sy, 1) reprojects to (sx, sy)"""
    return camera_struct((0, 0, 0), (0, 0, 1), (w, 0, 1), (0, h, 1))


def plane_frame(w, h, seed, channels=3):
    ys, xs = np.mgrid[0:h, 0:w]
    normal = np.zeros((h, w, 3))
    normal[..., 2] = -1.0
    p = np.stack([xs, ys, np.ones_like(xs)], axis=-1).astype(np.float64)
    img = np.random.RandomState(seed).uniform(0.0, 2.0, (h, w, channels)).astype(np.float32)
    return dict(node=np.zeros((h, w), dtype=np.int32), normal=normal, p=p), img


def test_nan_infinite_and_overflowing_guides_and_colour(gpu_ctx):
    w, h = 33, 20
    cam = sheared_camera()
    kw = dict(max_age=8, min_normal_dot=0.8, max_plane_dist=0.2)
    g0, img0 = synthetic(h, w, 5, cam, 0.0)
    g0["normal"][4, 4] = np.nan
    g0["p"][5, 6] = (1e300, -1e300, 1.0)
    img0[7, 7] = (np.nan, np.inf, -np.inf)
    _, hist = both(gpu_ctx, g0, img0, "edge values, first frame", **kw)
    g1, img1 = synthetic(h, w, 6, cam, 1.0)
    g1["p"][3, 3] = np.nan
    g1["p"][3, 4] = (np.inf, 0.0, 1.0)
    g1["p"][3, 5] = (1e300, 1e300, 1e300)
    g1["p"][3, 6] = (1e39, 1e39, 1e39)                   # finite in fp64, in the frame's direction or not; infinite as pf
    g1["normal"][6, 3] = np.nan
    g1["normal"][6, 4] = (np.inf, 0.0, -1.0)
    g1["normal"][6, 5] = 1e300
    img1[9, 9] = (np.nan, 1.0, np.inf)
    got, hist = both(gpu_ctx, g1, img1, "edge values, second frame", prev_cam=cam, history=hist, **kw)
    assert np.isnan(got["colour"]).any() and (got["age"][3, 3:6] == np.where(g1["node"][3, 3:6] >= 0, 1, 0)).all()
    g2, img2 = synthetic(h, w, 7, cam, 1.0)
    both(gpu_ctx, g2, img2, "edge values, third frame: NaN from the history", prev_cam=cam, history=hist, **kw)


def test_ages_at_the_limit_in_a_hand_built_history(gpu_ctx):
    w, h = 16, 8
    cam = axis_camera(w, h)
    g, img = plane_frame(w, h, 11)
    hs = {k: v.copy() for k, v in tr.split_history(tr.accumulate(g["node"], g["normal"], g["p"], img, 8, 0.5, 0.25)["history"], h, w, 3).items()}
    hs["age"][:] = 65534
    hs["age"][0, 0], hs["age"][0, 1], hs["age"][0, 2], hs["age"][0, 3] = 65535, 0xFFFFFFFF, 0, 70000
    hist = tr.join_history(hs["nf"], hs["node"], hs["pf"], hs["age"], hs["c"], hs["m"])
    _, img2 = plane_frame(w, h, 12)
    got, _ = both(gpu_ctx, g, img2, "ages at the limit", prev_cam=cam, history=hist, max_age=65535, min_normal_dot=0.5, max_plane_dist=0.25)
    assert list(got["age"][0, :5]) == [65535, 65535, 1, 65535, 65535]
    got, _ = both(gpu_ctx, g, img2, "ages beyond a smaller limit", prev_cam=cam, history=hist, max_age=7, min_normal_dot=0.5, max_plane_dist=0.25)
    assert list(got["age"][0, :5]) == [7, 7, 1, 7, 7]


def test_bilinear_weights_that_underflow(gpu_ctx):
    """fx = fy = 1e-30: the far tap's weight is 1e-60, zero in fp32, and is dropped by !(w > 0); fx = fy = 1e-20: 1e-40, a
    subnormal that must count"""
    w, h = 16, 8
    cam = axis_camera(w, h)
    g, img = plane_frame(w, h, 13)
    _, hist = both(gpu_ctx, g, img, "underflow, first frame", max_age=8, min_normal_dot=0.5, max_plane_dist=0.25)
    g2, img2 = plane_frame(w, h, 14)
    g2["p"][2, 2] = (1e-30, 1e-30, 1.0)
    g2["p"][2, 3] = (5.0 + 2.0 ** -50, 3.0 + 2.0 ** -50, 1.0)
    g2["p"][2, 4] = (1e-20, 1e-20, 1.0)
    big = hist.copy()
    tr.split_history(big, h, w, 3)["c"][1, 1] = 1e38          # times 1e-40: about 0.01 in the pixel that keeps the subnormal weight
    counts = {}
    got, _ = both(gpu_ctx, g2, img2, "underflow", prev_cam=cam, history=big, counts=counts, max_age=8, min_normal_dot=0.5, max_plane_dist=0.25)
    with_zero = tr.accumulate(g2["node"], g2["normal"], g2["p"], img2, 8, 0.5, 0.25, prev_cam=cam, history=hist)
    assert tr.count_differing(got["colour"][2, 4], with_zero["colour"][2, 4]) > 0         # the subnormal weight matters
    assert tr.count_differing(got["colour"][2, 2], with_zero["colour"][2, 2]) == 0         # the underflowed one does not
    assert np.isfinite(got["colour"]).all()


def test_misses_only_and_no_history(gpu_ctx):
    w, h = 13, 11
    cam = axis_camera(w, h)
    g, img = plane_frame(w, h, 15)
    g["node"][:] = -1
    got, hist = both(gpu_ctx, g, img, "misses only, first frame", max_age=8, min_normal_dot=0.5, max_plane_dist=0.25)
    assert got["colour"].tobytes() == img.tobytes() and not got["age"].any() and not bits(got["variance"]).any()
    g2, img2 = plane_frame(w, h, 16)
    got, hist = both(gpu_ctx, g2, img2, "hits over a history of misses", prev_cam=cam, history=hist, max_age=8, min_normal_dot=0.5, max_plane_dist=0.25)
    assert got["colour"].tobytes() == img2.tobytes() and (got["age"] == 1).all()
    got, _ = both(gpu_ctx, g, img, "misses over a history of hits", prev_cam=cam, history=hist, max_age=8, min_normal_dot=0.5, max_plane_dist=0.25)
    assert got["colour"].tobytes() == img.tobytes() and not got["age"].any()
    only, hist = gpu_ctx.temporalAccumulate(g2, img2, planes=("age",), max_age=8, min_normal_dot=0.5, max_plane_dist=0.25)
    assert list(only) == ["age"] and (only["age"] == 1).all()
    none, hist2 = gpu_ctx.temporalAccumulate(g2, img2, planes=(), max_age=8, min_normal_dot=0.5, max_plane_dist=0.25)
    assert none == {} and hist2.tobytes() == hist.tobytes()


# ---- 4. the device variant ---------------------------------------------------------------------------------------------------


def test_device_variant_on_a_stream_behind_the_planes(gpu_ctx):
    """hit planes, path planes and the accumulation enqueued back to back on one non-default stream, no sync in between: the
    host variant's bits; the guards around every output and the history keep the pattern; the inputs are what was rendered"""
    name = "lecture5"
    fs = frames(gpu_ctx, name)
    _, cams, opts = tc.sequence(name)
    hip = Q.hip_runtime()
    px = W * H
    need = c2.temporal_history_bytes(W, H, 3)
    assert need == px * 52
    kw = dict(max_age=8, **OPTS)
    _, hist0 = gpu_ctx.temporalAccumulate(fs[0], fs[0]["indirect"], **kw)
    want, want_hist = gpu_ctx.temporalAccumulate(fs[1], fs[1]["indirect"], prev_cam=cams[0], history=hist0, **kw)
    dev = {"node": DeviceBytes(px * 4), "normal": DeviceBytes(px * 24), "p": DeviceBytes(px * 24), "indirect": DeviceBytes(px * 12),
           "prev": DeviceBytes(need), "hist": DeviceBytes(GUARD + need + GUARD), "colour": DeviceBytes(GUARD + px * 12 + GUARD),
           "variance": DeviceBytes(GUARD + px * 4 + GUARD), "age": DeviceBytes(GUARD + px * 4 + GUARD)}
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        at = {k: d.ptr.value for k, d in dev.items()}
        assert hip.hipMemcpy(dev["prev"].ptr, hist0.ctypes.data, need, 1) == 0
        gpu_ctx.renderHitsDevice(cams[1], opts, {k: at[k] for k in ("node", "normal", "p")}, stream=stream.value)
        gpu_ctx.renderPathsDevice(cams[1], opts, P, B, {"indirect": at["indirect"]}, seed=SEED + 1, stream=stream.value)
        gpu_ctx.temporalAccumulateDevice({k: at[k] for k in ("node", "normal", "p")}, W, H, at["indirect"], at["prev"], at["hist"] + GUARD,
                                         planes={k: at[k] + GUARD for k in ("colour", "variance", "age")}, prev_cam=cams[0], stream=stream.value, **kw)
        assert hip.hipStreamSynchronize(stream) == 0
        got = {k: d.get() for k, d in dev.items()}
    finally:
        assert hip.hipStreamDestroy(stream) == 0
        Q.free_all(dev)
    for k, payload in (("colour", bits(want["colour"])), ("variance", bits(want["variance"])), ("age", bits(want["age"])), ("hist", want_hist)):
        n = payload.nbytes
        assert (got[k][:GUARD] == SENTINEL).all() and (got[k][GUARD + n:] == SENTINEL).all() and got[k].size == n + 2 * GUARD, k
        assert got[k][GUARD:GUARD + n].tobytes() == payload.tobytes(), k
    for k in ("node", "normal", "p", "indirect"):
        assert got[k].tobytes() == bits(fs[1][k]).tobytes(), k
    assert got["prev"].tobytes() == hist0.tobytes()


# ---- 5. the tie to the plain mean ---------------------------------------------------------------------------------------------


def test_still_camera_accumulates_the_mean_of_its_inputs(gpu_ctx):
    """prev_cam == cam, K = 6 frames of seeds s .. s + 5, max_age >= K: a hit pixel whose 3x3 neighbours share its node finds
    itself (and nothing else of weight), so that it holds the mean of its six inputs — compared in float64, with no use of
    the reference.  The bound: step k computes c + (in - c) * (1f / k) with four roundings (the subtraction, 1f / k, the
    product, the sum), each at most 2^-24 of a magnitude that does not exceed m, the largest |in| seen; the error of c is
    carried with a factor 1 - 1/k <= 1: 4 K 2^-24 m in all.  1e-9 covers the leakage of a neighbour through a bilinear
    weight of the order of the reprojection's 1e-13 (the neighbours hold values of the same magnitude)."""
    name, K = "lecture5", 6
    scene, cams, opts = tc.sequence(name)
    f0 = frames(gpu_ctx, name)[0]
    cam = cams[0]
    ins = [f0["indirect"]] + [gpu_ctx.renderPaths(cam, opts, P, B, seed=SEED + k, planes=("indirect",))["indirect"] for k in range(1, K)]
    hist = None
    for k in range(K):
        got, hist = gpu_ctx.temporalAccumulate(f0, ins[k], prev_cam=cam if k else None, history=hist, max_age=K + 2, **OPTS)
    node = f0["node"]
    inner = np.zeros((H, W), dtype=bool)
    inner[1:-1, 1:-1] = node[1:-1, 1:-1] >= 0
    m = np.zeros((H, W))
    stack = np.abs(np.stack(ins).astype(np.float64)).max(axis=(0, 3))
    for dy, dx in itertools.product((-1, 0, 1), repeat=2):
        ys, xs = slice(1 + dy, H - 1 + dy), slice(1 + dx, W - 1 + dx)
        inner[1:-1, 1:-1] &= node[ys, xs] == node[1:-1, 1:-1]
        m[1:-1, 1:-1] = np.maximum(m[1:-1, 1:-1], stack[ys, xs])
    assert inner.sum() >= 1000
    mean = np.stack(ins).astype(np.float64).mean(axis=0)
    err = np.abs(got["colour"].astype(np.float64) - mean).max(axis=2)
    tol = 4 * K * 2.0 ** -24 * m + 1e-9
    print("still camera: largest error over its bound %.3f, %d pixels" % ((err[inner] / tol[inner]).max(), inner.sum()))
    assert (err[inner] <= tol[inner]).all()
    assert (got["age"][inner] == K).all()
    assert got["variance"][inner].max() > 0 and (got["variance"] >= 0).all()


# ---- 6. the sequence in one call ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_render_paths_sequence_is_the_composition(gpu_ctx, name):
    fs = frames(gpu_ctx, name)
    scene, cams, opts = tc.sequence(name)
    kw = dict(max_age=8, **OPTS)
    want, hist = [], None
    for i in range(3):
        acc, hist = gpu_ctx.temporalAccumulate(fs[i], fs[i]["indirect"], prev_cam=cams[i - 1] if i else None, history=hist, planes=("colour",), **kw)
        want.append(gpu_ctx.denoise(fs[i], acc["colour"], levels=3, sigma_colour=0.5, albedo=fs[i]["albedo"], base=fs[i]["rgb"]))
    got = gpu_ctx.renderPathsSequence(cams[:3], opts, P, B, seed=SEED, levels=3, sigma_colour=0.5, **kw)
    assert got.shape == (3, H, W, 3) and got.dtype == np.float32
    for i in range(3):
        assert bits(got[i]).tobytes() == bits(want[i]).tobytes(), (name, i)
    one = gpu_ctx.renderPathsSequence(cams[:1], opts, P, B, seed=SEED, levels=3, sigma_colour=0.5, **kw)
    assert bits(one[0]).tobytes() == bits(gpu_ctx.renderPathsDenoised(cams[0], opts, P, B, seed=SEED, levels=3, sigma_colour=0.5)).tobytes()
    # a second call finds the staging large enough and the two histories stale: the same frames; generation and uploaded
    # scene are what they were
    generation = gpu_ctx.sceneGeneration
    again = gpu_ctx.renderPathsSequence(cams[:3], opts, P, B, seed=SEED, levels=3, sigma_colour=0.5, **kw)
    assert bits(again).tobytes() == bits(got).tobytes()
    assert gpu_ctx.sceneGeneration == generation
    assert bits(gpu_ctx.renderHits(cams[0], opts, planes=("rgb",))["rgb"]).tobytes() == bits(fs[0]["rgb"]).tobytes()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------


def test_refusals_in_the_documented_order(gpu_ctx):
    """Every refusal of c2rt_temporal_accumulate_device with every LATER violation present as well (where two set the same
    argument, the earlier one's value): the status and message are the first one's.  Nothing is enqueued: the outputs and
    the history keep the pattern."""
    px = 8 * 8
    L = lib()
    need = px * 52
    dev = {k: DeviceBytes(n) for k, n in (("node", px * 4), ("normal", px * 24), ("p", px * 24), ("in", px * 12), ("prev", need), ("hist", need + 16),
                                          ("colour", px * 12), ("variance", px * 4), ("age", px * 4))}
    at = {k: d.ptr.value for k, d in dev.items()}
    cam = axis_camera(8, 8)
    flat = camera_struct((0, 0, 0), (0, 0, 1), (8, 0, 1), (4, 0, 1))            # its three corners on one line: U x V = 0, det = 0
    good = dict(ctx=gpu_ctx.handle, opts=True, guides=True, planes=True, cam=cam, width=8, height=8, channels=3, max_age=8, min_normal_dot=0.9,
                max_plane_dist=0.1, reserved=(0, 0), node=at["node"], normal=at["normal"], p=at["p"], inp=at["in"], prev=at["prev"], hist=at["hist"],
                colour=at["colour"])
    E, LIM = _abi.ERR_INVALID_ARG, _abi.ERR_LIMIT
    steps = [  # (fields that turn bad, status, word of the message)
        (dict(ctx=None), E, None),
        (dict(opts=False), E, "null temporal options"),
        (dict(guides=False), E, "null temporal guides"),
        (dict(width=0), E, "above 0"),
        (dict(channels=2), E, "channels"),
        (dict(min_normal_dot=1.0), E, "min_normal_dot"),
        (dict(max_plane_dist=float("nan")), E, "max_plane_dist"),
        (dict(reserved=(0, 1)), E, "reserved"),
        (dict(max_age=0), LIM, "max_age"),
        (dict(node=None), E, "node"),
        (dict(normal=None), E, "normal"),
        (dict(p=None), E, ": p"),
        (dict(inp=None), E, "null temporal input"),
        (dict(hist=None), E, "null history out"),
        (dict(planes=False), E, "null temporal planes"),
        (dict(cam=None), E, "null prev_cam"),
        (dict(cam=flat), E, "degenerate previous camera"),
        (dict(hist=at["prev"]), E, "history out is the previous history"),
        (dict(colour=at["in"]), E, "colour plane is the input"),
        (dict(hist=at["hist"] + 4), E, "16-byte"),
    ]

    def call(v):
        o = _abi.TemporalOpts(width=v["width"], height=v["height"], channels=v["channels"], max_age=v["max_age"], min_normal_dot=v["min_normal_dot"],
                              max_plane_dist=v["max_plane_dist"], reserved=v["reserved"])
        g = _abi.TemporalGuides(node=v["node"], normal=v["normal"], p=v["p"])
        pl = _abi.TemporalPlanes(colour=v["colour"], variance=at["variance"], age=at["age"])
        return L.c2rt_temporal_accumulate_device(v["ctx"], None if v["cam"] is None else C.byref(v["cam"]), C.byref(g) if v["guides"] else None,
                                                 C.byref(o) if v["opts"] else None, v["inp"], v["prev"], v["hist"], C.byref(pl) if v["planes"] else None, None)

    outputs = ("hist", "colour", "variance", "age")
    try:
        assert call(good) == _abi.OK, last_error(gpu_ctx)
        assert dev["hist"].hip.hipDeviceSynchronize() == 0
        for k in ("hist", "variance", "age"):                                  # the valid call ran (its guides are all misses: colour = in)
            assert not (dev[k].get()[:px * 4] == SENTINEL).all(), k
        assert (dev["hist"].get()[need:] == SENTINEL).all()
        assert call(dict(good, prev=None, cam=None)) == _abi.OK, last_error(gpu_ctx)      # the first frame needs neither
        assert call(dict(good, max_age=65536)) == LIM and "max_age" in last_error(gpu_ctx)
        assert call(dict(good, prev=at["prev"] + 4)) == E and "16-byte" in last_error(gpu_ctx)
        for bad in (float("inf"), -0.5, float("nan")):
            assert call(dict(good, min_normal_dot=bad)) == E and "min_normal_dot" in last_error(gpu_ctx)
        for bad in (float("inf"), 0.0, -1.0):
            assert call(dict(good, max_plane_dist=bad)) == E and "max_plane_dist" in last_error(gpu_ctx)
        assert dev["hist"].hip.hipDeviceSynchronize() == 0
        for k in outputs:
            assert dev[k].hip.hipMemset(dev[k].ptr, SENTINEL, dev[k].nbytes) == 0
        for i, (_, status, word) in enumerate(steps):
            v = dict(good)
            for bad, _, _ in reversed(steps[i:]):
                v.update(bad)
            assert call(v) == status, (i, word, last_error(gpu_ctx))
            if word:
                assert word in last_error(gpu_ctx), (i, word, last_error(gpu_ctx))
        assert dev["hist"].hip.hipDeviceSynchronize() == 0
        for k in dev:
            assert (dev[k].get() == SENTINEL).all(), k
    finally:
        Q.free_all(dev)


def test_refusals_of_the_host_variant_and_of_the_sequence_call(gpu_ctx):
    fs = frames(gpu_ctx, "lecture5")
    _, cams, opts = tc.sequence("lecture5")
    L = lib()
    f = fs[1]
    px = W * H
    img = np.ascontiguousarray(f["indirect"])
    prev = np.zeros(px * 52 + 1, dtype=np.uint8)[1:]                            # a host history needs no alignment
    hist, colour = Q.sentinel_bytes(px * 52), Q.sentinel_bytes(px * 12)
    g = _abi.TemporalGuides(node=f["node"].ctypes.data, normal=f["normal"].ctypes.data, p=f["p"].ctypes.data)
    pl = _abi.TemporalPlanes(colour=colour.ctypes.data)

    def t(**kw):
        v = dict(width=W, height=H, channels=3, max_age=8, min_normal_dot=0.9, max_plane_dist=0.1)
        v.update(kw)
        return _abi.TemporalOpts(**v)

    E = _abi.ERR_INVALID_ARG
    for cam, opt, inp, hp, ho, planes, status, word in ((cams[0], t(height=0), img.ctypes.data, prev.ctypes.data, hist.ctypes.data, pl, E, "above 0"),
                                                        (cams[0], t(max_age=70000), img.ctypes.data, prev.ctypes.data, hist.ctypes.data, pl, _abi.ERR_LIMIT, "max_age"),
                                                        (cams[0], t(), None, prev.ctypes.data, hist.ctypes.data, pl, E, "input"),
                                                        (cams[0], t(), img.ctypes.data, prev.ctypes.data, None, pl, E, "history out"),
                                                        (cams[0], t(), img.ctypes.data, prev.ctypes.data, hist.ctypes.data, None, E, "planes"),
                                                        (None, t(), img.ctypes.data, prev.ctypes.data, hist.ctypes.data, pl, E, "prev_cam"),
                                                        (cams[0], t(), img.ctypes.data, hist.ctypes.data, hist.ctypes.data, pl, E, "previous history"),
                                                        (cams[0], t(), img.ctypes.data, prev.ctypes.data, hist.ctypes.data,
                                                         _abi.TemporalPlanes(colour=img.ctypes.data), E, "is the input")):
        st = L.c2rt_temporal_accumulate(gpu_ctx.handle, None if cam is None else C.byref(cam), C.byref(g), C.byref(opt), inp, hp, ho,
                                        None if planes is None else C.byref(planes))
        assert st == status, (word, last_error(gpu_ctx))
        assert word in last_error(gpu_ctx), (word, last_error(gpu_ctx))
    assert Q.untouched([hist, colour])
    assert L.c2rt_temporal_accumulate(gpu_ctx.handle, C.byref(cams[0]), C.byref(g), C.byref(t()), img.ctypes.data, prev.ctypes.data, hist.ctypes.data,
                                      C.byref(pl)) == _abi.OK, last_error(gpu_ctx)                      # the unaligned host history is fine
    assert not Q.untouched([hist]) and not Q.untouched([colour])

    out = Q.sentinel_bytes(3 * px * 12)
    pg = _abi.PathOpts(seed=SEED, paths=P, bounces=B)
    d = _abi.DenoiseOpts(width=W, height=H, levels=3, channels=3, normal_power_log2=5, sigma_plane=1.0, sigma_colour=0.0, reserved=0)
    arr = (_abi.CameraFrame * 3)(*cams[:3])
    lens = (_abi.CameraFrame * 3)(cams[0], Q.with_fields(cams[1], dof=1, num_samples=4), cams[2])
    stereo = (_abi.CameraFrame * 3)(Q.with_fields(cams[0], stereo_separation=0.1), cams[1], cams[2])
    flat = (_abi.CameraFrame * 3)(cams[0], Q.with_fields(cams[1], up_right=cams[1].up_left), cams[2])
    U = _abi.ERR_UNSUPPORTED
    for cams_, n, pg_, t_, d_, outp, status, word in ((None, 3, pg, t(), d, out.ctypes.data, E, "camera"),
                                                      (arr, 3, Q.with_fields(pg, paths=0), t(), d, out.ctypes.data, E, "paths"),
                                                      (arr, 3, pg, t(), None, out.ctypes.data, E, "null denoise options"),
                                                      (arr, 0, pg, None, d, None, E, "null output"),
                                                      (stereo, 3, pg, t(), d, out.ctypes.data, U, "stereo"),
                                                      (arr, 3, pg, t(), Q.with_fields(d, levels=9), out.ctypes.data, _abi.ERR_LIMIT, "levels"),
                                                      (arr, 0, pg, None, d, out.ctypes.data, E, "n_frames"),
                                                      (arr, 3, pg, None, d, out.ctypes.data, E, "null temporal options"),
                                                      (arr, 3, pg, t(width=W + 1), d, out.ctypes.data, E, "the frame has"),
                                                      (arr, 3, pg, t(channels=1), d, out.ctypes.data, E, "a frame has 3"),
                                                      (arr, 3, pg, t(max_age=0), d, out.ctypes.data, _abi.ERR_LIMIT, "max_age"),
                                                      (lens, 3, pg, t(), d, out.ctypes.data, U, "camera 1: depth of field"),
                                                      (flat, 3, pg, t(), d, out.ctypes.data, E, "degenerate previous camera")):
        st = L.c2rt_render_paths_sequence(gpu_ctx.handle, cams_, n, C.byref(opts), C.byref(pg_), None if t_ is None else C.byref(t_),
                                          None if d_ is None else C.byref(d_), outp)
        assert st == status, (word, last_error(gpu_ctx))
        assert word in last_error(gpu_ctx), (word, last_error(gpu_ctx))
    assert Q.untouched([out])


def test_multi_device_context_runs_on_its_lead_device(gpu_ctx):
    fs = frames(gpu_ctx, "csg_stress")
    _, cams, _ = tc.sequence("csg_stress")
    kw = dict(max_age=8, **OPTS)
    _, hist0 = gpu_ctx.temporalAccumulate(fs[0], fs[0]["indirect"], **kw)
    want, want_hist = gpu_ctx.temporalAccumulate(fs[1], fs[1]["indirect"], prev_cam=cams[0], history=hist0, **kw)
    two = c2.Context(devices=[0, 0])
    try:
        assert two.deviceCount == 2
        got, hist = two.temporalAccumulate(fs[1], fs[1]["indirect"], prev_cam=cams[0], history=hist0, **kw)      # no uploaded scene needed
    finally:
        two.close()
    for k in ("colour", "variance", "age"):
        assert bits(got[k]).tobytes() == bits(want[k]).tobytes(), k
    assert hist.tobytes() == want_hist.tobytes()
