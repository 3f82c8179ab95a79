"""The accumulation that follows moved nodes on the GPU (c2rt_temporal_accumulate_motion*,
c2rt_render_paths_sequence_posed*).  The arithmetic is the contract: every plane and the whole history are, BIT FOR BIT and
with no pixel excused (a NaN equal to any NaN), what tests/temporal_motion_reference.py makes of the same guides, input,
camera, history and motion — over the posed three-frame sequence of lecture5_like whose pixels fall into every class
(tests/test_temporal_motion_abi.py counts them from the oracle alone), then the synthetic moved patch at the shapes where a
launch can go wrong.  Then the equivalence with the static call, special values, the device variant, the two sequence
calls against the six-call composition, every refusal in the documented order, and a two-slot context."""
import ctypes as C

import numpy as np
import pytest

import chess2rt_amd as c2
import query_test_util as Q
import scene_update_util as su
import temporal_cases as tc
import temporal_motion_cases as mc
import temporal_motion_reference as tm
import temporal_reference as tr
from chess2rt_amd import _abi
from query_test_util import DeviceBytes, SENTINEL, last_error, lib
from ray_query_util import bits

pytestmark = pytest.mark.gpu

W, H = mc.W, mc.H
P, B, SEED = 2, 2, 77
GUARD = 256
LIGHT_MOVED = {0: dict(pos=(-60.0, 650.0, 300.0))}          # frame 1 of the sequence calls also moves the light
LIGHT_BASE = {0: dict(pos=su.LIGHT0[0])}


def both(ctx, g, image, what, prev_cam=None, history=None, motion=None, counts=None, **kw):
    """the host variant and the restatement on the same inputs: the same bits in every plane and in the history"""
    got, hist = ctx.temporalAccumulate(g, image, prev_cam=prev_cam, history=history, motion=motion, **kw)
    want = tm.accumulate(g["node"], g["normal"], g["p"], image, kw["max_age"], kw["min_normal_dot"], kw["max_plane_dist"], prev_cam=prev_cam,
                         history=history, motion=motion, counts=counts)
    h, w = g["node"].shape
    ch = 1 if image.ndim == 2 else image.shape[2]
    n = tr.count_differing(got["colour"], want["colour"])
    assert n == 0, "%s: %d of %d colour values differ" % (what, n, image.size)
    n = tr.count_differing(got["variance"], want["variance"])
    assert n == 0, "%s: %d of %d variances differ" % (what, n, h * w)
    assert np.array_equal(got["age"], want["age"]), what
    assert hist.dtype == np.uint8 and hist.size == c2.temporal_history_bytes(w, h, ch)
    n = tr.history_differing(hist, want["history"], h, w, ch)
    assert n == 0, "%s: %d values of the history differ" % (what, n)
    return got, hist


@pytest.fixture(scope="module")
def seq(gpu_ctx, tmp_path_factory):
    """the posed sequence, rendered once and shared read-only: per frame the guides, rgb, albedo and indirect of the scene
    under that frame's pose (c2rt_update_scene with the base patched by the pose)"""
    scene, cams, opts, poses, base = mc.posed_sequence(tmp_path_factory.mktemp("motion"))
    gpu_ctx.uploadScene(scene.desc)
    frames = []
    for i, cam in enumerate(cams):
        gpu_ctx.updateScene(nodes=mc.full_pose(poses, base, i), lights=LIGHT_MOVED if i == 1 else LIGHT_BASE)
        f = dict(gpu_ctx.renderHits(cam, opts, planes=("node", "normal", "p", "rgb")))
        f["albedo"] = gpu_ctx.renderShading(cam, opts, planes=("albedo",))["albedo"]
        f["indirect"] = gpu_ctx.renderPaths(cam, opts, P, B, seed=SEED + i, planes=("indirect",))["indirect"]
        for a in f.values():
            a.setflags(write=False)
        frames.append(f)
    return dict(scene=scene, cams=cams, opts=opts, poses=poses, base=base, frames=frames)


def upload_base(ctx, seq):
    ctx.uploadScene(seq["scene"].desc)


# ---- 1. the posed sequence, bit for bit against the restatement ----------------------------------------------------------


@pytest.mark.parametrize("channels", [3, 1])
def test_posed_sequence_matches_the_restatement(gpu_ctx, seq, channels):
    fs, cams, poses, base = seq["frames"], seq["cams"], seq["poses"], seq["base"]
    hist, counts, static_hist = None, {}, None
    for i, f in enumerate(fs):
        img = f["indirect"] if channels == 3 else np.ascontiguousarray(f["indirect"][..., 0])
        motion = mc.frame_motion(poses, base, i) if i else None
        got, hist = both(gpu_ctx, f, img, ("posed sequence", channels, i), prev_cam=cams[i - 1] if i else None, history=hist, motion=motion,
                         counts=counts, **mc.SEQ_OPTS)
        assert not np.isnan(got["colour"]).any()
        if i == 1:                                                                          # what the static call makes of the same frame
            static, _ = gpu_ctx.temporalAccumulate(f, img, prev_cam=cams[0], history=static_hist, **mc.SEQ_OPTS)
            on = np.isin(f["node"], list(motion))
            assert (got["age"][on] == 2).sum() >= 50 + (static["age"][on] == 2).sum()       # the moved nodes found more
            assert np.array_equal(got["age"][~on], static["age"][~on])
        static_hist = hist
    for k in ("moved_kept", "moved_rejected", "unlisted_history"):
        assert counts[k] >= 50, (k, counts)


# ---- 2. shapes: the moved patch ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (63, 1), (64, 1), (65, 3), (61, 47), (257, 3)])
def test_moved_patch_at_every_shape(gpu_ctx, w, h):
    """1 and 16 listed nodes, the patch's node first, last or absent: listed, every pixel of the patch comes out age 2
    (the reference-free anchor of tests/test_temporal_motion_abi.py); absent, age 1, as through the static call"""
    cam, g0, hist0, c0, g1, in1, prev, cur, patch = mc.anchor(w, h)
    for n_listed in (1, 16):
        for where in ("first", "last", "absent"):
            motion = mc.anchor_motion(prev, cur, n_listed, where)
            assert len(motion) == n_listed and (mc.ANCHOR_NODE in motion) == (where != "absent")
            got, _ = both(gpu_ctx, g1, in1, (w, h, n_listed, where), prev_cam=cam, history=hist0, motion=motion, **mc.ANCHOR_OPTS)
            assert (got["age"][patch] == (1 if where == "absent" else 2)).all() and (got["age"][~patch] == 0).all()
            if where != "absent":
                want = c0.astype(np.float64) + (in1.astype(np.float64) - c0.astype(np.float64)) / 2
                assert (np.abs(got["colour"].astype(np.float64) - want)[patch] <= 1e-5 * np.abs(want)[patch]).all()
    cam, g0, hist1, c1, g1, in1c, prev, cur, patch = mc.anchor(w, h, 1)                     # one channel
    both(gpu_ctx, g1, in1c[..., 0], (w, h, "one channel"), prev_cam=cam, history=hist1, motion={mc.ANCHOR_NODE: (prev, cur)}, **mc.ANCHOR_OPTS)


# ---- 3. equivalence with the static call ----------------------------------------------------------------------------------


def test_empty_and_null_motion_are_the_static_call(gpu_ctx):
    scene, cams, opts = tc.sequence("lecture5")
    gpu_ctx.uploadScene(scene.desc)
    kw = dict(max_age=8, min_normal_dot=tc.MIN_NORMAL_DOT, max_plane_dist=tc.MAX_PLANE_DIST)
    fs = []
    for i, cam in enumerate(cams[:3]):
        f = dict(gpu_ctx.renderHits(cam, opts, planes=("node", "normal", "p")))
        f["indirect"] = gpu_ctx.renderPaths(cam, opts, P, B, seed=SEED + i, planes=("indirect",))["indirect"]
        fs.append(f)
    hs = hm = None
    null = _abi.TemporalMotion()
    for i, f in enumerate(fs):
        cam = cams[i - 1] if i else None
        before = hs
        s, hs = gpu_ctx.temporalAccumulate(f, f["indirect"], prev_cam=cam, history=before, **kw)
        m, hm = gpu_ctx.temporalAccumulate(f, f["indirect"], prev_cam=cam, history=hm, motion={}, **kw)
        # a history written by one call is read by the other; a list of nodes no pixel lies on changes nothing either
        n, hn = gpu_ctx.temporalAccumulate(f, f["indirect"], prev_cam=cam, history=before,
                                           motion=null if i < 2 else {90: (su.xf(), su.xf(("translate", 1, 2, 3)))}, **kw)
        for k in ("colour", "variance", "age"):
            assert bits(m[k]).tobytes() == bits(s[k]).tobytes() and bits(n[k]).tobytes() == bits(s[k]).tobytes(), (i, k)
        assert hm.tobytes() == hs.tobytes() and hn.tobytes() == hs.tobytes(), i
    assert (s["age"] == 3).sum() > 500


# ---- 4. special values ---------------------------------------------------------------------------------------------------------


def test_nan_infinite_and_zero_transforms(gpu_ctx):
    cam, g0, hist0, c0, g1, in1, prev, cur, patch = mc.anchor(61, 47)
    zero = np.zeros(30)
    for what, pose in (("NaN in cur.inverseTransform", (prev, su.xf_with(10, float("nan")))), ("infinite prev offset", (su.xf_with(28, float("inf")), cur)),
                       ("-infinity in prev.transform", (su.xf_with(4, float("-inf")), cur)), ("NaN in cur.transform", (prev, su.xf_with(0, float("nan")))),
                       ("zero cur", (prev, zero)), ("zero prev", (zero, cur)), ("both zero", (zero, zero))):
        got, _ = both(gpu_ctx, g1, in1, what, prev_cam=cam, history=hist0, motion={mc.ANCHOR_NODE: pose, 3: (prev, cur)}, **mc.ANCHOR_OPTS)
        assert (got["age"][patch] == 1).all() and got["colour"][patch].tobytes() == in1[patch].tobytes(), what
        assert np.isfinite(got["colour"]).all()
    # a non-rigid motion (a scale) is followed too: the squared tests carry the carried normal's length
    scaled = su.xf(("scale", 1.5, 0.7, 1.2), *mc.ANCHOR_CUR)
    g = dict(node=g1["node"], normal=mc.moved_normal(g0["normal"], prev, cur), p=mc.moved_point(g0["p"], prev, scaled))
    got, _ = both(gpu_ctx, g, in1, "scaled", prev_cam=cam, history=hist0, motion={mc.ANCHOR_NODE: (prev, scaled)},
                  **dict(mc.ANCHOR_OPTS, min_normal_dot=0.0))
    assert (got["age"][patch] == 2).all()


# ---- 5. the device variant ---------------------------------------------------------------------------------------------------


def test_device_variant_on_a_stream_behind_the_planes(gpu_ctx, seq):
    """frame 2 of the posed sequence: hit planes, path planes and the motion accumulation enqueued back to back on one
    non-default stream; the host variant's bits, and the guards around every output keep the pattern"""
    upload_base(gpu_ctx, seq)
    fs, cams, opts, poses, base = seq["frames"], seq["cams"], seq["opts"], seq["poses"], seq["base"]
    hip = Q.hip_runtime()
    px = W * H
    need = c2.temporal_history_bytes(W, H, 3)
    kw = mc.SEQ_OPTS
    motion = mc.frame_motion(poses, base, 2)
    _, hist1 = gpu_ctx.temporalAccumulate(fs[1], fs[1]["indirect"], **kw)
    want, want_hist = gpu_ctx.temporalAccumulate(fs[2], fs[2]["indirect"], prev_cam=cams[1], history=hist1, motion=motion, **kw)
    assert (want["age"][np.isin(fs[2]["node"], list(motion))] == 2).sum() >= 50
    dev = {"node": DeviceBytes(px * 4), "normal": DeviceBytes(px * 24), "p": DeviceBytes(px * 24), "indirect": DeviceBytes(px * 12),
           "prev": DeviceBytes(need), "hist": DeviceBytes(GUARD + need + GUARD), "colour": DeviceBytes(GUARD + px * 12 + GUARD),
           "variance": DeviceBytes(GUARD + px * 4 + GUARD), "age": DeviceBytes(GUARD + px * 4 + GUARD)}
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        at = {k: d.ptr.value for k, d in dev.items()}
        assert hip.hipMemcpy(dev["prev"].ptr, hist1.ctypes.data, need, 1) == 0
        gpu_ctx.updateScene(nodes=mc.full_pose(poses, base, 2), stream=stream.value)
        gpu_ctx.renderHitsDevice(cams[2], opts, {k: at[k] for k in ("node", "normal", "p")}, stream=stream.value)
        gpu_ctx.renderPathsDevice(cams[2], opts, P, B, {"indirect": at["indirect"]}, seed=SEED + 2, stream=stream.value)
        gpu_ctx.temporalAccumulateDevice({k: at[k] for k in ("node", "normal", "p")}, W, H, at["indirect"], at["prev"], at["hist"] + GUARD,
                                         planes={k: at[k] + GUARD for k in ("colour", "variance", "age")}, prev_cam=cams[1], stream=stream.value,
                                         motion=motion, **kw)
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
        assert got[k].tobytes() == bits(fs[2][k]).tobytes(), k


# ---- 6. the posed sequences in one call --------------------------------------------------------------------------------------


@pytest.mark.parametrize("variance", [False, True])
def test_posed_sequence_calls_are_the_composition(gpu_ctx, seq, variance):
    upload_base(gpu_ctx, seq)
    fs, cams, opts, poses, base = seq["frames"], seq["cams"], seq["opts"], seq["poses"], seq["base"]
    kw = mc.SEQ_OPTS
    before = gpu_ctx.renderHits(cams[0], opts, planes=("rgb",))["rgb"]
    assert bits(before).tobytes() == bits(fs[0]["rgb"]).tobytes()
    want, hist = [], None
    for i, f in enumerate(fs):
        planes = ("colour", "variance", "age") if variance else ("colour",)
        acc, hist = gpu_ctx.temporalAccumulate(f, f["indirect"], prev_cam=cams[i - 1] if i else None, history=hist, planes=planes,
                                               motion=mc.frame_motion(poses, base, i) if i else {}, **kw)
        if variance:
            want.append(gpu_ctx.denoiseVariance(f, acc["colour"], acc["variance"], acc["age"], levels=3, albedo=f["albedo"], base=f["rgb"], variance_out=False)[0])
        else:
            want.append(gpu_ctx.denoise(f, acc["colour"], levels=3, sigma_colour=0.5, albedo=f["albedo"], base=f["rgb"]))
    pairs = [(poses[i], LIGHT_MOVED if i == 1 else None) for i in range(len(cams))]
    generation = gpu_ctx.sceneGeneration
    for _ in range(2):                                                                      # the second call finds the scene put back
        if variance:
            got = gpu_ctx.renderPathsSequencePosedVariance(cams, pairs, opts, P, B, seed=SEED, levels=3, **kw)
        else:
            got = gpu_ctx.renderPathsSequencePosed(cams, pairs, opts, P, B, seed=SEED, levels=3, sigma_colour=0.5, **kw)
        assert got.shape == (3, H, W, 3) and got.dtype == np.float32
        for i in range(3):
            assert bits(got[i]).tobytes() == bits(want[i]).tobytes(), (variance, i)
    assert gpu_ctx.sceneGeneration == generation
    assert bits(gpu_ctx.renderHits(cams[0], opts, planes=("rgb",))["rgb"]).tobytes() == bits(before).tobytes()
    # no pose at all: the unposed call's frames
    still = [({}, None)] * 3
    if variance:
        a, b = gpu_ctx.renderPathsSequencePosedVariance(cams, still, opts, P, B, seed=SEED, levels=3, **kw), gpu_ctx.renderPathsSequenceVariance(cams, opts, P, B, seed=SEED, levels=3, **kw)
    else:
        a, b = gpu_ctx.renderPathsSequencePosed(cams, still, opts, P, B, seed=SEED, levels=3, **kw), gpu_ctx.renderPathsSequence(cams, opts, P, B, seed=SEED, levels=3, **kw)
    assert bits(a).tobytes() == bits(b).tobytes()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------


def test_refusals_in_the_documented_order(gpu_ctx):
    """Every refusal of c2rt_temporal_accumulate_motion_device with every LATER violation present as well (where two set
    the same argument, the earlier one's value): status and message are the first one's; the motion's own stand behind
    "null planes" and before the previous camera's.  Nothing is enqueued: outputs and history keep the pattern."""
    px = 8 * 8
    L = lib()
    need = px * 52
    dev = {k: DeviceBytes(n) for k, n in (("node", px * 4), ("normal", px * 24), ("p", px * 24), ("in", px * 12), ("prev", need), ("hist", need + 16),
                                          ("colour", px * 12), ("variance", px * 4), ("age", px * 4))}
    at = {k: d.ptr.value for k, d in dev.items()}
    cam = mc.camera_struct((0, 0, 0), (0, 0, 1), (8, 0, 1), (0, 8, 1))
    flat = mc.camera_struct((0, 0, 0), (0, 0, 1), (8, 0, 1), (4, 0, 1))
    xfs = np.ascontiguousarray([su.xf(("translate", k, 0, 0)) for k in range(17)])
    idx = np.arange(17, dtype=np.uint32)
    twice = np.array([4, 9, 2, 9], dtype=np.uint32)
    good = dict(ctx=gpu_ctx.handle, opts=True, guides=True, planes=True, cam=cam, width=8, height=8, channels=3, max_age=8, min_normal_dot=0.9,
                max_plane_dist=0.1, reserved=(0, 0), node=at["node"], normal=at["normal"], p=at["p"], inp=at["in"], prev=at["prev"], hist=at["hist"],
                colour=at["colour"], m_reserved=0, m_n=4, m_index=idx, m_prev=xfs, m_cur=xfs)
    E, LIM = _abi.ERR_INVALID_ARG, _abi.ERR_LIMIT
    steps = [
        (dict(ctx=None), E, None),
        (dict(opts=False), E, "null temporal options"),
        (dict(guides=False), E, "null temporal guides"),
        (dict(width=0), E, "above 0"),
        (dict(channels=2), E, "channels"),
        (dict(min_normal_dot=1.0), E, "min_normal_dot"),
        (dict(max_plane_dist=float("nan")), E, "max_plane_dist"),
        (dict(reserved=(0, 1)), E, "c2rt_temporal_opts.reserved"),
        (dict(max_age=0), LIM, "max_age"),
        (dict(node=None), E, "node"),
        (dict(normal=None), E, "normal"),
        (dict(p=None), E, ": p"),
        (dict(inp=None), E, "null temporal input"),
        (dict(hist=None), E, "null history out"),
        (dict(planes=False), E, "null temporal planes"),
        (dict(m_reserved=1), E, "c2rt_temporal_motion.reserved"),
        (dict(m_n=17), LIM, "17 moved nodes"),
        (dict(m_index=None), E, "null node_index"),
        (dict(m_prev=None), E, "null prev_transform"),
        (dict(m_cur=None), E, "null cur_transform"),
        (dict(m_index=twice), E, "node_index[3] = 9 is listed twice"),
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
        m = _abi.TemporalMotion(n_nodes=v["m_n"], reserved=v["m_reserved"])
        for field, key, ptr in (("node_index", "m_index", _abi._u32p), ("prev_transform", "m_prev", _abi._f64p), ("cur_transform", "m_cur", _abi._f64p)):
            if v[key] is not None:
                setattr(m, field, v[key].ctypes.data_as(ptr))
        return L.c2rt_temporal_accumulate_motion_device(v["ctx"], None if v["cam"] is None else C.byref(v["cam"]), C.byref(g) if v["guides"] else None,
                                                        C.byref(o) if v["opts"] else None, C.byref(m), v["inp"], v["prev"], v["hist"],
                                                        C.byref(pl) if v["planes"] else None, None)

    try:
        assert call(good) == _abi.OK, last_error(gpu_ctx)
        assert call(dict(good, m_n=16)) == _abi.OK, last_error(gpu_ctx)                      # the limit itself is fine
        assert call(dict(good, m_n=0, m_index=None, m_prev=None, m_cur=None)) == _abi.OK, last_error(gpu_ctx)      # an empty list needs no arrays
        assert call(dict(good, prev=None, cam=None, m_index=twice)) == E                    # checked also where there is no history to use it on
        assert call(dict(good, prev=None, cam=None)) == _abi.OK, last_error(gpu_ctx)        # a motion without a history is fine
        assert dev["hist"].hip.hipDeviceSynchronize() == 0
        for k in ("hist", "colour", "variance", "age"):
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


def test_refusals_of_the_host_variant_and_of_the_posed_sequence_calls(gpu_ctx, seq, tmp_path):
    upload_base(gpu_ctx, seq)
    fs, cams, opts, poses = seq["frames"], seq["cams"], seq["opts"], seq["poses"]
    L = lib()
    f = fs[1]
    px = W * H
    img = np.ascontiguousarray(f["indirect"])
    prev = np.zeros(px * 52, dtype=np.uint8)
    hist, colour = Q.sentinel_bytes(px * 52), Q.sentinel_bytes(px * 12)
    g = _abi.TemporalGuides(node=f["node"].ctypes.data, normal=f["normal"].ctypes.data, p=f["p"].ctypes.data)
    pl = _abi.TemporalPlanes(colour=colour.ctypes.data)
    t = _abi.TemporalOpts(width=W, height=H, channels=3, max_age=8, min_normal_dot=0.9, max_plane_dist=0.1)
    E, LIM, U = _abi.ERR_INVALID_ARG, _abi.ERR_LIMIT, _abi.ERR_UNSUPPORTED
    ok = c2.makeMotion({2: (su.xf(), su.xf(("translate", 1, 0, 0))), 3: (su.xf(), su.xf())})
    twice = np.array([3, 3], dtype=np.uint32)
    for m, planes, status, word in ((Q.with_fields(ok, reserved=7), pl, E, "reserved"), (Q.with_fields(ok, n_nodes=17), pl, LIM, "moved nodes"),
                                    (Q.with_fields(ok, cur_transform=None), pl, E, "cur_transform"),
                                    (Q.with_fields(ok, node_index=twice.ctypes.data_as(_abi._u32p)), pl, E, "node_index[1] = 3"),
                                    (ok, None, E, "planes"), (Q.with_fields(ok, reserved=7), None, E, "planes")):
        st = L.c2rt_temporal_accumulate_motion(gpu_ctx.handle, C.byref(cams[0]), C.byref(g), C.byref(t), C.byref(m), img.ctypes.data, prev.ctypes.data,
                                               hist.ctypes.data, None if planes is None else C.byref(planes))
        assert st == status and word in last_error(gpu_ctx), (word, st, last_error(gpu_ctx))
    assert Q.untouched([hist, colour])

    out = Q.sentinel_bytes(3 * px * 12)
    pg = _abi.PathOpts(seed=SEED, paths=P, bounces=B)
    d = _abi.DenoiseOpts(width=W, height=H, levels=3, channels=3, normal_power_log2=5, sigma_plane=1.0, sigma_colour=0.0, reserved=0)
    dv = _abi.DenoiseVarianceOpts(width=W, height=H, levels=3, channels=3, normal_power_log2=5, sigma_plane=1.0, sigma_lum=4.0, var_floor=1e-6, min_age=4, reserved=0)
    arr = (_abi.CameraFrame * 3)(*cams)
    lens = (_abi.CameraFrame * 3)(cams[0], Q.with_fields(cams[1], dof=1, num_samples=4), cams[2])
    good = [c2.makePose(p, None) for p in poses]
    parr = (_abi.ScenePose * 3)(*good)
    out_of_range, no_such_light = c2.makePose({99: su.xf()}, None), c2.makePose(None, {5: dict(pos=(0, 0, 0))})       # (named: a pose owns its arrays)
    bad_index = (_abi.ScenePose * 3)(good[0], out_of_range, good[2])
    bad_light = (_abi.ScenePose * 3)(good[0], good[1], no_such_light)
    before = gpu_ctx.renderHits(cams[0], opts, planes=("rgb",))["rgb"]
    for posed_call, filt in ((L.c2rt_render_paths_sequence_posed, d), (L.c2rt_render_paths_sequence_posed_variance, dv)):
        for cams_, poses_, n, t_, outp, status, word in ((None, parr, 3, t, out.ctypes.data, E, "camera"),
                                                         (arr, None, 3, None, out.ctypes.data, E, "null temporal options"),      # the unposed call's come first
                                                         (lens, None, 3, t, out.ctypes.data, U, "camera 1: depth of field"),
                                                         (arr, None, 3, t, out.ctypes.data, E, "null poses"),
                                                         (arr, bad_index, 3, t, out.ctypes.data, E, "frame 1: "),
                                                         (arr, bad_light, 3, t, out.ctypes.data, E, "frame 2: ")):
            st = posed_call(gpu_ctx.handle, cams_, poses_, n, C.byref(opts), C.byref(pg), None if t_ is None else C.byref(t_), C.byref(filt), outp)
            assert st == status and word in last_error(gpu_ctx), (word, st, last_error(gpu_ctx))
    assert Q.untouched([out])
    assert bits(gpu_ctx.renderHits(cams[0], opts, planes=("rgb",))["rgb"]).tobytes() == bits(before).tobytes()

    # more than 16 moved nodes between two frames: a limit, naming the frame; 16 are fine
    forty = su.forty_nodes(tmp_path)
    forty.setDof(False)
    cam40 = forty.beginFrame()
    opts40 = forty.renderOpts(taps=_abi.TAPS_1)
    gpu_ctx.uploadScene(forty.desc)
    try:
        base40 = su.Desc(forty.desc)
        moved = lambda nodes: {n: np.concatenate([base40.transform(n)[:27], base40.transform(n)[27:] + (0.5, 0.25, 0.0)]) for n in nodes}
        t40 = _abi.TemporalOpts(width=opts40.width, height=opts40.height, channels=3, max_age=8, min_normal_dot=0.9, max_plane_dist=0.1)
        d40 = Q.with_fields(d, width=opts40.width, height=opts40.height)
        out40 = Q.sentinel_bytes(3 * opts40.width * opts40.height * 12)
        cams40 = (_abi.CameraFrame * 3)(cam40, cam40, cam40)
        # 9 + 8 nodes: 17 entries; 8 + 8: 16; 9 + 9 that share node 9 in the same pose: its entry is dropped, 16 are left
        for first, second, status in ((range(1, 10), range(10, 18), LIM), (range(1, 9), range(9, 17), _abi.OK), (range(1, 10), range(9, 18), _abi.OK)):
            ps = [c2.makePose({}, None), c2.makePose(moved(first), None), c2.makePose(moved(second), None)]   # frame 2: both sets differ from frame 1
            st = L.c2rt_render_paths_sequence_posed(gpu_ctx.handle, cams40, (_abi.ScenePose * 3)(*ps), 3, C.byref(opts40), C.byref(pg), C.byref(t40),
                                                    C.byref(d40), out40.ctypes.data)
            assert st == status, (st, last_error(gpu_ctx))
            if status != _abi.OK:
                assert "frame 2: 17 nodes moved" in last_error(gpu_ctx), last_error(gpu_ctx)
                assert Q.untouched([out40])
    finally:
        upload_base(gpu_ctx, seq)


# ---- 8. a two-slot context ---------------------------------------------------------------------------------------------------


def test_multi_device_context_runs_on_its_lead_device(gpu_ctx, seq):
    fs, cams, poses, base = seq["frames"], seq["cams"], seq["poses"], seq["base"]
    kw = mc.SEQ_OPTS
    motion = mc.frame_motion(poses, base, 1)
    _, hist0 = gpu_ctx.temporalAccumulate(fs[0], fs[0]["indirect"], **kw)
    want, want_hist = gpu_ctx.temporalAccumulate(fs[1], fs[1]["indirect"], prev_cam=cams[0], history=hist0, motion=motion, **kw)
    two = c2.Context(devices=[0, 0])
    try:
        assert two.deviceCount == 2
        got, hist = two.temporalAccumulate(fs[1], fs[1]["indirect"], prev_cam=cams[0], history=hist0, motion=motion, **kw)      # no uploaded scene needed
    finally:
        two.close()
    for k in ("colour", "variance", "age"):
        assert bits(got[k]).tobytes() == bits(want[k]).tobytes(), k
    assert hist.tobytes() == want_hist.tobytes()
