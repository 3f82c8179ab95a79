"""The variance-guided a-trous filter on the GPU (c2rt_denoise_variance*, c2rt_render_paths_sequence_variance).  The
arithmetic is the contract: `out` and `variance_out` are, BIT FOR BIT and with no pixel excused (a NaN equal to any NaN),
what tests/denoise_variance_reference.py makes of the same guides, planes and options — over frames 0 and 3 of the
camera sequences of lecture5 and csg_stress, accumulated by the context's own temporal stage (tests/
test_denoise_variance_abi.py counts their classes from the oracle alone), then synthetic frames for the shapes and the
edge values.  Then the tie to c2rt_denoise, a scaling property that does not go through the reference, the device variant
against the host variant, the sequence call against the composition, and every refusal in the documented order."""
import ctypes as C
import itertools

import numpy as np
import pytest

import chess2rt_amd as c2
import denoise_variance_cases as vc
import denoise_variance_reference as vr
import occlusion_cases as oc
import query_test_util as Q
import temporal_cases as tc
from chess2rt_amd import _abi
from query_test_util import DeviceBytes, SENTINEL, last_error, lib
from ray_query_util import bits

pytestmark = pytest.mark.gpu

W, H, SEED = tc.W, tc.H, oc.SEED
P, B = 8, 2
GUARD = 256
TEMPORAL = dict(max_age=vc.MAX_AGE, min_normal_dot=tc.MIN_NORMAL_DOT, max_plane_dist=tc.MAX_PLANE_DIST)
_frames = {}


def frames(ctx, name):
    """uploads the scene and returns, for each camera of its sequence, the planes at 61x47, rendered and accumulated once
    and shared read-only: the guides (node, normal, p), rgb, albedo, the path planes' indirect (P = 8, B = 2, seed + i)
    and ao, and what Context.temporalAccumulate makes of indirect and of ao along the sequence (acc, variance, age and
    acc_ao, variance_ao, age_ao)"""
    scene, cams, opts = tc.sequence(name)
    ctx.uploadScene(scene.desc)
    if name not in _frames:
        out, hist, hist_ao = [], None, None
        for i, cam in enumerate(cams):
            f = dict(ctx.renderHits(cam, opts, planes=("node", "normal", "p", "rgb")))
            f["albedo"] = ctx.renderShading(cam, opts, planes=("albedo",))["albedo"]
            f["indirect"] = ctx.renderPaths(cam, opts, P, B, seed=SEED + i, planes=("indirect",))["indirect"]
            f["ao"] = ctx.renderOcclusion(cam, opts, oc.K, oc.RADIUS[name], seed=SEED + i, planes=("ao",))["ao"]
            t, hist = ctx.temporalAccumulate(f, f["indirect"], prev_cam=cams[i - 1] if i else None, history=hist, **TEMPORAL)
            f["acc"], f["variance"], f["age"] = t["colour"], t["variance"], t["age"]
            t, hist_ao = ctx.temporalAccumulate(f, f["ao"], prev_cam=cams[i - 1] if i else None, history=hist_ao, **TEMPORAL)
            f["acc_ao"], f["variance_ao"], f["age_ao"] = t["colour"], t["variance"], t["age"]
            for a in f.values():
                a.setflags(write=False)
            out.append(f)
        _frames[name] = out
    return _frames[name]


def both(ctx, g, image, variance, age, what, counts=None, **kw):
    """the host variant and the reference on the same inputs: the same bits in both planes (a NaN is any NaN)"""
    got, gotv = ctx.denoiseVariance(g, image, variance, age, **kw)
    want, wantv = vr.denoise_variance(g["node"], g["normal"], g["p"], image, variance, age, counts=counts, **kw)
    assert got.shape == image.shape and got.dtype == np.float32 and gotv.shape == g["node"].shape and gotv.dtype == np.float32
    n = vr.count_differing(got, want)
    assert n == 0, "%s: %d of %d colour values differ" % (what, n, want.size)
    n = vr.count_differing(gotv, wantv)
    assert n == 0, "%s: %d of %d variances differ" % (what, n, wantv.size)
    return got, gotv


# ---- 1. real sequences, bit for bit against the reference ----------------------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_scene_frames_match_the_reference(gpu_ctx, name):
    fs = frames(gpu_ctx, name)
    for i in (0, 3):
        f = fs[i]
        assert np.isfinite(f["acc"]).all() and (f["node"] < 0).sum() >= 50
        closing = (dict(), dict(albedo=f["albedo"], base=f["rgb"]))
        for levels, sl, min_age, kw in itertools.product((0, 1, 2, 5), (0.0, vc.SIGMA_LUM), (0, vc.MIN_AGE), closing):
            counts = {}
            got, gotv = both(gpu_ctx, f, f["acc"], f["variance"], f["age"], (name, i, levels, sl, min_age, tuple(kw)), counts=counts, levels=levels,
                             sigma_lum=sl, min_age=min_age, **kw)
            assert not np.isnan(got).any() and not np.isnan(gotv).any()                                   # no NaN to excuse
            if min_age:
                assert counts["young"] >= (50 if i else 1000)                                             # frame 0: every hit pixel is young
            if i and min_age:
                assert counts["temporal"] >= 50
            if levels >= 2:
                assert vr.count_differing(got, f["acc"]) > got.size // 2                                  # the filter does something
            if levels == 5 and sl:
                print(name, i, min_age, {k: v for k, v in counts.items() if k != "levels"})
                assert counts["soft_lum"] >= 20
        both(gpu_ctx, f, f["acc_ao"], f["variance_ao"], f["age_ao"], (name, i, "ao"), levels=3, sigma_lum=vc.SIGMA_LUM, min_age=vc.MIN_AGE)
        both(gpu_ctx, f, f["acc_ao"].reshape(H, W, 1), f["variance_ao"], None, (name, i, "ao, (H, W, 1), no age"), levels=2, sigma_lum=2.0)
        both(gpu_ctx, f, f["acc_ao"], f["variance_ao"], f["age_ao"], (name, i, "ao closing"), levels=0, min_age=vc.MIN_AGE,
             albedo=f["acc"][..., 0], base=f["acc"][..., 1])
    out, none = gpu_ctx.denoiseVariance(fs[3], fs[3]["acc"], fs[3]["variance"], fs[3]["age"], levels=3, variance_out=False)
    assert none is None
    assert bits(out).tobytes() == bits(gpu_ctx.denoiseVariance(fs[3], fs[3]["acc"], fs[3]["variance"], fs[3]["age"], levels=3)[0]).tobytes()


# ---- 2. the tie to c2rt_denoise, on the GPU ---------------------------------------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_no_luminance_term_is_the_plain_filter(gpu_ctx, name):
    f = frames(gpu_ctx, name)[3]
    for levels, kw in itertools.product((0, 1, 4), (dict(), dict(albedo=f["albedo"], base=f["rgb"]))):
        got, _ = gpu_ctx.denoiseVariance(f, f["acc"], f["variance"], f["age"], levels=levels, sigma_lum=0.0, min_age=vc.MIN_AGE, **kw)
        want = gpu_ctx.denoise(f, f["acc"], levels=levels, sigma_colour=0.0, **kw)
        assert bits(got).tobytes() == bits(want).tobytes(), (name, levels, tuple(kw))


# ---- 3. scaling: a property that needs no reference ----------------------------------------------------------------------------


def test_scaling_by_powers_of_two_commutes_with_the_filter(gpu_ctx):
    """Every operation of the contract commutes with a power of two where nothing is subnormal or overflows: 4 in, 16
    variance and 16 var_floor give 4 out and 16 variance_out, bit for bit (dl^2 and sl2 g + var_floor both take 16, the
    luminance factor is unchanged, the weights are unchanged; the spatial estimate is a variance of 4 l: 16 v)."""
    f = frames(gpu_ctx, "lecture5")[3]
    # The precondition, made to hold: lecture5's accumulated light goes down to 2e-38 in its darkest pixels, where a product
    # with a weight is subnormal and rounds differently from four times itself.  Values below 2^-20 (black on any display)
    # (in the accumulated plane and in the base) and variances below 2^-60 are set to zero, which scales exactly; power 0
    # keeps every weight's square normal.
    acc = np.where(np.abs(f["acc"]) < np.float32(2.0 ** -20), np.float32(0), f["acc"])
    var = np.where(np.abs(f["variance"]) < np.float32(2.0 ** -60), np.float32(0), f["variance"])
    rgb = np.where(np.abs(f["rgb"]) < np.float32(2.0 ** -20), np.float32(0), f["rgb"])
    changed, changed_v = int((acc != f["acc"]).sum()), int((var != f["variance"]).sum())
    print("scaling: %d of %d colour values and %d of %d variances set to zero" % (changed, acc.size, changed_v, var.size))
    assert changed < acc.size // 20 and changed_v < var.size // 20                                   # it is still the lecture5 frame
    kw = dict(levels=4, normal_power_log2=0, sigma_lum=vc.SIGMA_LUM, min_age=vc.MIN_AGE, albedo=f["albedo"])
    floor = 2.0 ** -26
    out, vout = gpu_ctx.denoiseVariance(f, acc, var, f["age"], var_floor=floor, base=rgb, **kw)
    out4, vout16 = gpu_ctx.denoiseVariance(f, acc * np.float32(4), var * np.float32(16), f["age"], var_floor=16 * floor, base=rgb * np.float32(4), **kw)
    for what, a in (("in", acc), ("variance", var), ("out", out), ("variance_out", vout), ("4 out", out4), ("16 variance_out", vout16)):
        nz = np.abs(a[a != 0])
        print("scaling: %s within [%.3g, %.3g]" % (what, nz.min(), nz.max()))
        assert np.isfinite(a).all() and nz.min() >= 2.0 ** -100 and nz.max() <= 2.0 ** 100, what      # far from subnormal (2^-126) and overflow
    assert (vout[f["node"] >= 0] > 0).sum() >= 1000
    assert bits(out4).tobytes() == bits(out * np.float32(4)).tobytes()
    assert bits(vout16).tobytes() == bits(vout * np.float32(16)).tobytes()


# ---- 4. shapes -----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (3, 3), (64, 8), (65, 9), (130, 67)])
def test_shapes_and_steps_beyond_the_frame(gpu_ctx, w, h):
    g, img, variance, age = vc.synthetic(h, w, 100 * w + h)
    young = np.zeros_like(age)
    for levels in (1, 3, 8):
        both(gpu_ctx, g, img, variance, age, (w, h, levels, "mixed ages"), levels=levels, normal_power_log2=1, sigma_plane=0.5, sigma_lum=2.0,
             min_age=vc.MIN_AGE)
        both(gpu_ctx, g, img, variance, young, (w, h, levels, "all young"), levels=levels, normal_power_log2=0, sigma_plane=0.5, sigma_lum=2.0, min_age=64)
    both(gpu_ctx, g, img[..., 0], variance, age, (w, h, "one channel"), levels=8, normal_power_log2=0, min_age=vc.MIN_AGE)
    both(gpu_ctx, g, img, variance, age, (w, h, "closing"), levels=8, normal_power_log2=3, min_age=vc.MIN_AGE, albedo=img[::-1].copy(),
         base=img[:, ::-1].copy())
    both(gpu_ctx, g, img, variance, age, (w, h, "no level"), levels=0, min_age=vc.MIN_AGE, base=img[:, ::-1].copy())


# ---- 5. edge values --------------------------------------------------------------------------------------------------------------


def test_nan_infinite_negative_and_zero_variance(gpu_ctx):
    f = frames(gpu_ctx, "lecture5")[3]
    bad = vc.inject(f["variance"], f["node"])
    counts = {}
    got, gotv = both(gpu_ctx, f, f["acc"], bad, f["age"], "injected variance", counts=counts, levels=3, sigma_lum=vc.SIGMA_LUM, var_floor=vc.TINY_FLOOR,
                     min_age=vc.MIN_AGE)
    assert counts["dropped_lum"] >= 20 and np.isnan(gotv).any() and not np.isnan(got).any()    # a NaN variance weighs, it is never a colour
    both(gpu_ctx, f, f["acc"], bad, None, "injected variance, no age", levels=5, sigma_lum=vc.SIGMA_LUM, var_floor=vc.VAR_FLOOR)
    zero = np.zeros_like(f["variance"])
    counts = {}
    both(gpu_ctx, f, f["acc"], zero, None, "no variance: var_floor alone", counts=counts, levels=3, sigma_lum=vc.SIGMA_LUM, var_floor=vc.VAR_FLOOR)
    assert counts["soft_lum"] >= 1000
    counts = {}
    both(gpu_ctx, f, f["acc"], zero, None, "inv_l overflows", counts=counts, levels=3, sigma_lum=vc.SIGMA_LUM, var_floor=vc.TINY_FLOOR)
    assert counts["dropped_lum"] >= 1000


def test_nan_input_in_a_young_window_misses_only_and_age_zero(gpu_ctx):
    g, img, variance, age = vc.synthetic(23, 31, 9)
    img = img.copy()
    ys, xs = np.nonzero(g["node"] >= 0)
    img[ys[40], xs[40]] = (np.nan, 1.0, 2.0)
    img[ys[200], xs[200]] = (np.inf, 1.0, 2.0)
    got, gotv = both(gpu_ctx, g, img, variance, np.zeros_like(age), "NaN input, every pixel young with age 0", levels=0, min_age=5, normal_power_log2=0)
    assert not np.isnan(gotv).any()                            # a NaN estimate becomes +0f
    both(gpu_ctx, g, img, variance, np.zeros_like(age), "NaN input, filtered", levels=2, min_age=5, sigma_lum=vc.SIGMA_LUM, normal_power_log2=0)
    both(gpu_ctx, g, img, variance, np.full_like(age, 0xFFFFFFFF), "ages at the top", levels=1, min_age=64)
    miss = dict(g, node=np.full_like(g["node"], -1))
    got, gotv = both(gpu_ctx, miss, img, variance, age, "misses only", levels=3, min_age=vc.MIN_AGE, base=img[::-1].copy())
    assert not bits(gotv).any()
    got, gotv = both(gpu_ctx, miss, img, variance, age, "misses only, no level", levels=0, min_age=vc.MIN_AGE)
    assert vr.same_bits(got, img) and not bits(gotv).any()


# ---- 6. the device variant ---------------------------------------------------------------------------------------------------


def test_device_variant_on_a_stream_behind_the_planes(gpu_ctx):
    """hit planes, path planes, the accumulation and the filter enqueued back to back on one non-default stream, no sync in
    between: the host variant's bits; the guards around `out`, `variance_out` and the scratch keep the pattern; the inputs are
    what was rendered"""
    name = "lecture5"
    fs = frames(gpu_ctx, name)
    _, cams, opts = tc.sequence(name)
    hip = Q.hip_runtime()
    px = W * H
    levels = 5
    need = c2.denoise_variance_scratch_bytes(W, H, 3, levels, min_age=vc.MIN_AGE)
    hist_bytes = c2.temporal_history_bytes(W, H, 3)
    assert need == px * 56
    _, hist0 = gpu_ctx.temporalAccumulate(fs[0], fs[0]["indirect"], planes=(), **TEMPORAL)
    t, _ = gpu_ctx.temporalAccumulate(fs[1], fs[1]["indirect"], prev_cam=cams[0], history=hist0, **TEMPORAL)
    want, wantv = gpu_ctx.denoiseVariance(fs[1], t["colour"], t["variance"], t["age"], levels=levels, sigma_lum=vc.SIGMA_LUM, min_age=vc.MIN_AGE,
                                          base=fs[1]["rgb"])
    dev = {"node": DeviceBytes(px * 4), "normal": DeviceBytes(px * 24), "p": DeviceBytes(px * 24), "rgb": DeviceBytes(px * 12),
           "indirect": DeviceBytes(px * 12), "prev": DeviceBytes(hist_bytes), "hist": DeviceBytes(hist_bytes), "variance": DeviceBytes(px * 4),
           "age": DeviceBytes(px * 4), "out": DeviceBytes(GUARD + px * 12 + GUARD), "vout": DeviceBytes(GUARD + px * 4 + GUARD),
           "scratch": DeviceBytes(GUARD + need + GUARD)}
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        at = {k: d.ptr.value for k, d in dev.items()}
        assert hip.hipMemcpy(dev["prev"].ptr, hist0.ctypes.data, hist_bytes, 1) == 0
        gpu_ctx.renderHitsDevice(cams[1], opts, {k: at[k] for k in ("node", "normal", "p", "rgb")}, stream=stream.value)
        gpu_ctx.renderPathsDevice(cams[1], opts, P, B, {"indirect": at["indirect"]}, seed=SEED + 1, stream=stream.value)
        gpu_ctx.temporalAccumulateDevice({k: at[k] for k in ("node", "normal", "p")}, W, H, at["indirect"], at["prev"], at["hist"],
                                         planes={"variance": at["variance"], "age": at["age"]}, prev_cam=cams[0], stream=stream.value, **TEMPORAL)
        gpu_ctx.denoiseVarianceDevice({"node": at["node"], "normal": at["normal"], "p": at["p"], "base": at["rgb"]}, W, H, at["variance"], at["age"],
                                      at["hist"] + px * 32, at["out"] + GUARD, at["vout"] + GUARD, at["scratch"] + GUARD, levels=levels,
                                      sigma_lum=vc.SIGMA_LUM, min_age=vc.MIN_AGE, stream=stream.value)
        assert hip.hipStreamSynchronize(stream) == 0
        got = {k: d.get() for k, d in dev.items()}
    finally:
        assert hip.hipStreamDestroy(stream) == 0
        Q.free_all(dev)
    for k, payload in (("out", bits(want)), ("vout", bits(wantv))):
        n = payload.nbytes
        assert (got[k][:GUARD] == SENTINEL).all() and (got[k][GUARD + n:] == SENTINEL).all() and got[k].size == n + 2 * GUARD, k
        assert got[k][GUARD:GUARD + n].tobytes() == payload.tobytes(), k
    assert (got["scratch"][:GUARD] == SENTINEL).all() and (got["scratch"][GUARD + need:] == SENTINEL).all()
    assert not (got["scratch"][GUARD:GUARD + need] == SENTINEL).all()
    for k in ("node", "normal", "p", "rgb", "indirect"):
        assert got[k].tobytes() == bits(fs[1][k]).tobytes(), k
    assert got["variance"].tobytes() == bits(t["variance"]).tobytes() and got["age"].tobytes() == bits(t["age"]).tobytes()
    assert got["prev"].tobytes() == hist0.tobytes()


def test_device_variant_without_level_age_or_variance_out(gpu_ctx):
    """levels == 0 and min_age == 0 need no scratch; without variance_out only `out` is written"""
    f = frames(gpu_ctx, "csg_stress")[3]
    px = W * H
    assert c2.denoise_variance_scratch_bytes(W, H, 3, 0, min_age=0) == 0
    keys = ("node", "normal", "p", "albedo", "rgb", "acc", "variance")
    dev = {k: DeviceBytes(bits(f[k]).nbytes) for k in keys}
    dev["out"] = DeviceBytes(px * 12 + GUARD)
    dev["vout"] = DeviceBytes(px * 4 + GUARD)
    try:
        for k in keys:
            assert dev[k].hip.hipMemcpy(dev[k].ptr, bits(f[k]).ctypes.data, dev[k].nbytes, 1) == 0
        at = {k: d.ptr.value for k, d in dev.items()}
        ptrs = {"node": at["node"], "normal": at["normal"], "p": at["p"], "albedo": at["albedo"], "base": at["rgb"]}
        gpu_ctx.denoiseVarianceDevice(ptrs, W, H, at["variance"], 0, at["acc"], at["out"], 0, 0, levels=0, min_age=0)
        assert dev["out"].hip.hipDeviceSynchronize() == 0
        out, vout = dev["out"].get(), dev["vout"].get()
        assert (vout == SENTINEL).all() and (out[px * 12:] == SENTINEL).all()
        want, wantv = gpu_ctx.denoiseVariance(f, f["acc"], f["variance"], None, levels=0, min_age=0, albedo=f["albedo"], base=f["rgb"])
        assert out[:px * 12].tobytes() == bits(want).tobytes()
        gpu_ctx.denoiseVarianceDevice(ptrs, W, H, at["variance"], 0, at["acc"], at["out"], at["vout"], 0, levels=0, min_age=0)
        assert dev["out"].hip.hipDeviceSynchronize() == 0
        vout = dev["vout"].get()
        assert vout[:px * 4].tobytes() == bits(wantv).tobytes() and (vout[px * 4:] == SENTINEL).all()
    finally:
        Q.free_all(dev)


# ---- 7. the sequence in one call ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_render_paths_sequence_variance_is_the_composition(gpu_ctx, name):
    fs = frames(gpu_ctx, name)
    scene, cams, opts = tc.sequence(name)
    kw = dict(levels=3, sigma_lum=vc.SIGMA_LUM, min_age=vc.MIN_AGE)
    want = [gpu_ctx.denoiseVariance(f, f["acc"], f["variance"], f["age"], albedo=f["albedo"], base=f["rgb"], variance_out=False, **kw)[0] for f in fs]
    got = gpu_ctx.renderPathsSequenceVariance(cams, opts, P, B, seed=SEED, **TEMPORAL, **kw)
    assert got.shape == (4, H, W, 3) and got.dtype == np.float32
    for i in range(4):
        assert bits(got[i]).tobytes() == bits(want[i]).tobytes(), (name, i)
    one = gpu_ctx.renderPathsSequenceVariance(cams[:1], opts, P, B, seed=SEED, **TEMPORAL, **kw)
    assert one.shape == (1, H, W, 3) and bits(one[0]).tobytes() == bits(want[0]).tobytes()
    plain = gpu_ctx.renderPathsSequence(cams[:2], opts, P, B, seed=SEED, levels=3, sigma_colour=0.0, **TEMPORAL)
    tie = gpu_ctx.renderPathsSequenceVariance(cams[:2], opts, P, B, seed=SEED, levels=3, sigma_lum=0.0, min_age=vc.MIN_AGE, **TEMPORAL)
    assert bits(tie).tobytes() == bits(plain).tobytes()
    generation = gpu_ctx.sceneGeneration
    again = gpu_ctx.renderPathsSequenceVariance(cams, opts, P, B, seed=SEED, **TEMPORAL, **kw)
    assert bits(again).tobytes() == bits(got).tobytes() and gpu_ctx.sceneGeneration == generation


def test_two_slot_context_runs_on_its_lead_device(gpu_ctx):
    fs = frames(gpu_ctx, "csg_stress")
    scene, cams, opts = tc.sequence("csg_stress")
    f = fs[3]
    kw = dict(levels=3, sigma_lum=vc.SIGMA_LUM, min_age=vc.MIN_AGE)
    want, wantv = gpu_ctx.denoiseVariance(f, f["acc"], f["variance"], f["age"], **kw)
    seq = gpu_ctx.renderPathsSequenceVariance(cams[:2], opts, P, B, seed=SEED, **TEMPORAL, **kw)
    two = c2.Context(devices=[0, 0])
    try:
        assert two.deviceCount == 2
        got, gotv = two.denoiseVariance(f, f["acc"], f["variance"], f["age"], **kw)               # no uploaded scene needed
        two.uploadScene(scene.desc)
        got_seq = two.renderPathsSequenceVariance(cams[:2], opts, P, B, seed=SEED, **TEMPORAL, **kw)
    finally:
        two.close()
    assert bits(got).tobytes() == bits(want).tobytes() and bits(gotv).tobytes() == bits(wantv).tobytes()
    assert bits(got_seq).tobytes() == bits(seq).tobytes()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------


def test_refusals_in_the_documented_order(gpu_ctx):
    """Every refusal of c2rt_denoise_variance_device with every LATER violation present as well (where two set the same
    argument, the earlier one's value): the status and message are the first one's.  Nothing is enqueued: the outputs and
    the scratch keep the pattern."""
    px = 8 * 8
    L = lib()
    need = px * 56
    dev = {k: DeviceBytes(n) for k, n in (("node", px * 4), ("normal", px * 24), ("p", px * 24), ("variance", px * 4), ("age", px * 4), ("in", px * 12),
                                          ("out", px * 12), ("vout", px * 4), ("scratch", need + 16))}
    at = {k: d.ptr.value for k, d in dev.items()}
    good = dict(ctx=gpu_ctx.handle, opts=True, guides=True, width=8, height=8, levels=5, channels=3, power=5, sigma_plane=1.0, sigma_lum=4.0, var_floor=1e-8,
                min_age=4, reserved=0, node=at["node"], normal=at["normal"], p=at["p"], variance=at["variance"], inp=at["in"], out=at["out"],
                vout=at["vout"], scratch=at["scratch"])
    E, LIM = _abi.ERR_INVALID_ARG, _abi.ERR_LIMIT
    steps = [  # (fields that turn bad, status, word of the message)
        (dict(ctx=None), E, None),
        (dict(opts=False), E, "null variance denoise options"),
        (dict(guides=False), E, "null denoise guides"),
        (dict(width=0), E, "above 0"),
        (dict(channels=2), E, "channels"),
        (dict(sigma_plane=0.0), E, "sigma_plane"),
        (dict(sigma_lum=-1.0), E, "sigma_lum"),
        (dict(var_floor=0.0), E, "var_floor"),
        (dict(reserved=1), E, "reserved"),
        (dict(levels=9), LIM, "levels"),
        (dict(power=8), LIM, "normal_power_log2"),
        (dict(min_age=65), LIM, "min_age"),
        (dict(node=None), E, "node"),
        (dict(normal=None), E, "normal"),
        (dict(p=None), E, ": p"),
        (dict(variance=None), E, "null variance plane"),
        (dict(inp=None), E, "null denoise input"),
        (dict(out=None), E, "null denoise output"),
        (dict(out=at["in"]), E, "output is the input"),
        (dict(vout=at["variance"]), E, "variance output is the variance plane"),
        (dict(out=at["scratch"]), E, "denoise output is the scratch"),
        (dict(vout=at["scratch"]), E, "variance output is the scratch"),
        (dict(scratch=None), E, "null denoise scratch"),
        (dict(scratch=at["scratch"] + 4), E, "16-byte"),
    ]

    def call(v):
        o = _abi.DenoiseVarianceOpts(width=v["width"], height=v["height"], levels=v["levels"], channels=v["channels"], normal_power_log2=v["power"],
                                     sigma_plane=v["sigma_plane"], sigma_lum=v["sigma_lum"], var_floor=v["var_floor"], min_age=v["min_age"],
                                     reserved=v["reserved"])
        g = _abi.DenoiseGuides(node=v["node"], normal=v["normal"], p=v["p"])
        return L.c2rt_denoise_variance_device(v["ctx"], C.byref(g) if v["guides"] else None, C.byref(o) if v["opts"] else None, v["variance"], at["age"],
                                              v["inp"], v["out"], v["vout"], v["scratch"], None)

    outputs = ("out", "vout", "scratch")
    try:
        assert call(good) == _abi.OK, last_error(gpu_ctx)
        assert dev["out"].hip.hipDeviceSynchronize() == 0
        for k in ("vout", "scratch"):                                           # the valid call ran (its guides are all misses: out = in)
            assert not (dev[k].get()[:px * 4] == SENTINEL).all(), k
        assert (dev["scratch"].get()[need:] == SENTINEL).all()
        assert call(dict(good, vout=None)) == _abi.OK, last_error(gpu_ctx)
        for bad in (float("inf"), float("nan")):
            assert call(dict(good, sigma_lum=bad)) == E and "sigma_lum" in last_error(gpu_ctx)
        for bad in (float("inf"), float("nan"), -1e-8):
            assert call(dict(good, var_floor=bad)) == E and "var_floor" in last_error(gpu_ctx)
        assert dev["out"].hip.hipDeviceSynchronize() == 0
        for k in outputs:
            assert dev[k].hip.hipMemset(dev[k].ptr, SENTINEL, dev[k].nbytes) == 0
        # the last two of the order, apart from the list below (they set `inp` and `variance`, which earlier entries compare
        # against): an input that is the scratch, behind the scratch's own refusals
        assert call(dict(good, inp=at["scratch"])) == E and "denoise input is the scratch" in last_error(gpu_ctx)
        assert call(dict(good, variance=at["scratch"])) == E and "variance plane is the scratch" in last_error(gpu_ctx)
        assert call(dict(good, inp=at["scratch"], variance=at["scratch"])) == E and "denoise input is the scratch" in last_error(gpu_ctx)
        assert call(dict(good, scratch=at["scratch"] + 4, inp=at["scratch"] + 4, variance=at["scratch"] + 4)) == E and "16-byte" in last_error(gpu_ctx)
        assert call(dict(good, vout=at["scratch"], inp=at["scratch"])) == E and "variance output is the scratch" in last_error(gpu_ctx)
        for i, (_, status, word) in enumerate(steps):
            v = dict(good)
            for bad, _, _ in reversed(steps[i:]):
                if not (word and "is the scratch" in word and "scratch" in bad):      # an output can only equal a scratch that is there
                    v.update(bad)
            assert call(v) == status, (i, word, last_error(gpu_ctx))
            if word:
                assert word in last_error(gpu_ctx), (i, word, last_error(gpu_ctx))
        assert dev["out"].hip.hipDeviceSynchronize() == 0
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
    img, var = np.ascontiguousarray(f["acc"]), np.ascontiguousarray(f["variance"])
    out, vout = Q.sentinel_bytes(px * 12), Q.sentinel_bytes(px * 4)
    g = _abi.DenoiseGuides(node=f["node"].ctypes.data, normal=f["normal"].ctypes.data, p=f["p"].ctypes.data)

    def d(**kw):
        v = dict(width=W, height=H, levels=3, channels=3, normal_power_log2=5, sigma_plane=1.0, sigma_lum=4.0, var_floor=1e-8, min_age=4, reserved=0)
        v.update(kw)
        return _abi.DenoiseVarianceOpts(**v)

    E, LIM, U = _abi.ERR_INVALID_ARG, _abi.ERR_LIMIT, _abi.ERR_UNSUPPORTED
    for opt, gd, v_, in_, out_, vout_, status, word in ((d(height=0), g, var.ctypes.data, img.ctypes.data, out.ctypes.data, vout.ctypes.data, E, "above 0"),
                                                        (d(var_floor=0.0), g, var.ctypes.data, img.ctypes.data, out.ctypes.data, vout.ctypes.data, E, "var_floor"),
                                                        (d(min_age=65), g, var.ctypes.data, img.ctypes.data, out.ctypes.data, vout.ctypes.data, LIM, "min_age"),
                                                        (d(), _abi.DenoiseGuides(node=f["node"].ctypes.data, normal=f["normal"].ctypes.data), var.ctypes.data,
                                                         img.ctypes.data, out.ctypes.data, vout.ctypes.data, E, ": p"),
                                                        (d(), g, None, img.ctypes.data, out.ctypes.data, vout.ctypes.data, E, "null variance plane"),
                                                        (d(), g, var.ctypes.data, None, out.ctypes.data, vout.ctypes.data, E, "input"),
                                                        (d(), g, var.ctypes.data, img.ctypes.data, None, vout.ctypes.data, E, "output"),
                                                        (d(), g, var.ctypes.data, out.ctypes.data, out.ctypes.data, vout.ctypes.data, E, "is the input"),
                                                        (d(), g, vout.ctypes.data, img.ctypes.data, out.ctypes.data, vout.ctypes.data, E, "is the variance plane")):
        st = L.c2rt_denoise_variance(gpu_ctx.handle, C.byref(gd), C.byref(opt), v_, f["age"].ctypes.data, in_, out_, vout_)
        assert st == status, (word, last_error(gpu_ctx))
        assert word in last_error(gpu_ctx), (word, last_error(gpu_ctx))
    assert Q.untouched([out, vout])

    seq = Q.sentinel_bytes(3 * px * 12)
    pg = _abi.PathOpts(seed=SEED, paths=P, bounces=B)
    t = _abi.TemporalOpts(width=W, height=H, channels=3, max_age=8, min_normal_dot=0.9, max_plane_dist=0.1)
    arr = (_abi.CameraFrame * 3)(*cams[:3])
    lens = (_abi.CameraFrame * 3)(cams[0], Q.with_fields(cams[1], dof=1, num_samples=4), cams[2])
    stereo = (_abi.CameraFrame * 3)(Q.with_fields(cams[0], stereo_separation=0.1), cams[1], cams[2])
    flat = (_abi.CameraFrame * 3)(cams[0], Q.with_fields(cams[1], up_right=cams[1].up_left), cams[2])
    strips = Q.with_fields(opts, strip_world=2)
    for cams_, n, o_, pg_, t_, d_, outp, status, word in ((None, 3, opts, pg, t, d(), seq.ctypes.data, E, "camera"),
                                                          (arr, 3, opts, Q.with_fields(pg, paths=0), t, d(), seq.ctypes.data, E, "paths"),
                                                          (arr, 3, opts, pg, t, None, seq.ctypes.data, E, "null denoise options"),
                                                          (arr, 0, opts, pg, None, d(), None, E, "null output"),
                                                          (stereo, 3, opts, pg, t, d(), seq.ctypes.data, U, "stereo"),
                                                          (arr, 3, strips, pg, t, d(), seq.ctypes.data, U, "strip_world"),
                                                          (arr, 3, opts, pg, t, d(width=W + 1), seq.ctypes.data, E, "the frame has"),
                                                          (arr, 3, opts, pg, t, d(channels=1), seq.ctypes.data, E, "a frame has 3"),
                                                          (arr, 3, opts, pg, t, d(sigma_lum=float("nan")), seq.ctypes.data, E, "sigma_lum"),
                                                          (arr, 3, opts, pg, t, d(levels=9), seq.ctypes.data, LIM, "levels"),
                                                          (arr, 3, opts, pg, t, d(min_age=65), seq.ctypes.data, LIM, "min_age"),
                                                          (arr, 0, opts, pg, None, d(), seq.ctypes.data, E, "n_frames"),
                                                          (arr, 3, opts, pg, None, d(), seq.ctypes.data, E, "null temporal options"),
                                                          (arr, 3, opts, pg, Q.with_fields(t, width=W + 1), d(), seq.ctypes.data, E, "the frame has"),
                                                          (arr, 3, opts, pg, Q.with_fields(t, max_age=0), d(), seq.ctypes.data, LIM, "max_age"),
                                                          (lens, 3, opts, pg, t, d(), seq.ctypes.data, U, "camera 1: depth of field"),
                                                          (flat, 3, opts, pg, t, d(), seq.ctypes.data, E, "degenerate previous camera")):
        st = L.c2rt_render_paths_sequence_variance(gpu_ctx.handle, cams_, n, C.byref(o_), C.byref(pg_), None if t_ is None else C.byref(t_),
                                                   None if d_ is None else C.byref(d_), outp)
        assert st == status, (word, last_error(gpu_ctx))
        assert word in last_error(gpu_ctx), (word, last_error(gpu_ctx))
    assert Q.untouched([seq])
