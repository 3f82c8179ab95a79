"""Counted path planes and path counts on the GPU (c2rt_render_paths_counted*, c2rt_trace_rays_paths_counted*,
c2rt_path_counts*, c2rt_render_paths_sequence_adaptive).  The oracle of the counted planes is the uniform call: a sample
given c >= 1 paths holds, BIT FOR BIT and with no sample excused, what c2rt_render_paths / c2rt_trace_rays_paths writes for
it with paths = c; a sample given 0 holds the record's node, the ray's own colour and zeros.  Then the two launch orders
against each other, counts at or above the cap, plane subsets, the guards behind every plane and the scratch, the host
variants and their chunks, strips, a posed scene; c2rt_path_counts against tests/path_counts_reference.py over the
four-frame camera sequences; the sequence call against the composition; and every refusal in the documented order."""
import ctypes as C

import numpy as np
import pytest

import chess2rt_amd as c2
import denoise_variance_cases as vc
import occlusion_cases as oc
import path_counts_reference as cr
import query_test_util as Q
import scene_update_util as U
import temporal_cases as tc
import temporal_reference as tr
from chess2rt_amd import _abi
from chess2rt_amd.api import PATH_PLANES
from query_test_util import DeviceBytes, SENTINEL, guarded, last_error, lib, struct_of, untouched
from ray_query_util import bits

pytestmark = pytest.mark.gpu

W, H, SEED = oc.W, oc.H, oc.SEED
CAP, B = 8, 4
PLANES = tuple(PATH_PLANES)
VALUES = np.array([0, 1, 2, 3, 5, 8, CAP, 200], dtype=np.uint8)
GUARD = 256
_uniform, _loaded = {}, {}


def p_opts(paths=CAP, bounces=B, seed=SEED):
    return _abi.PathOpts(seed=seed, paths=paths, bounces=bounces)


def mix(i, salt=0):
    """a fixed hash of the sample index (a 32-bit multiply-xorshift)"""
    x = (np.asarray(i, dtype=np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B1) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = x * np.uint64(0x85EBCA77) & np.uint64(0xFFFFFFFF)
    return x ^ (x >> np.uint64(13))


def tile_wave():
    """the wave of every pixel of the W x H frame in the camera calls' natural order: the 8x8 tile"""
    ys, xs = np.mgrid[0:H, 0:W]
    return ((ys // 8) * ((W + 7) // 8) + xs // 8).reshape(-1)


def layout(wave):
    """a counts plane over the samples whose wave (in natural order) is wave[i]: wave 1 all zeros, wave 2 all equal (5),
    wave 3 a single lane at the cap among ones, the rest VALUES by the hash"""
    n = len(wave)
    counts = VALUES[(mix(np.arange(n)) % np.uint64(len(VALUES))).astype(np.int64)].copy()
    counts[wave == 1] = 0
    counts[wave == 2] = 5
    lone = np.flatnonzero(wave == 3)
    counts[lone] = 1
    counts[lone[len(lone) // 2]] = CAP
    return counts


def load(ctx, name):
    scene, cam, opts = oc.load(name)
    ctx.uploadScene(scene.desc)
    return scene, cam, opts


def uniform(ctx, name, form, c):
    """the uniform call's planes at paths = c, samples flattened: computed once per scene and form, read-only"""
    key = (name, form, c)
    if key not in _uniform:
        scene, cam, opts = oc.load(name)
        got = ctx.renderPaths(cam, opts, c, B, SEED) if form == "frame" else ctx.traceRaysPaths(oc.ray_set(name, "eyeless"), c, B, SEED)
        got = {p: np.ascontiguousarray(a.reshape((-1,) + a.shape[(2 if form == "frame" else 1):])) for p, a in got.items()}
        for a in got.values():
            a.setflags(write=False)
        _uniform[key] = got
    return _uniform[key]


def expected(ctx, name, form, counts, rgb):
    """what the contract makes of `counts` (flat): every sample the uniform call's of its own c; class 0 the node, zeros and
    the ray's own colour"""
    c = np.minimum(counts, CAP)
    want = {p: np.zeros_like(uniform(ctx, name, form, CAP)[p]) for p in PLANES}
    want["node"][...] = uniform(ctx, name, form, CAP)["node"]
    want["radiance"][c == 0] = rgb[c == 0]
    for k in np.unique(c[c > 0]):
        u = uniform(ctx, name, form, int(k))
        assert np.array_equal(u["node"], want["node"])
        for p in PLANES:
            want[p][c == k] = u[p][c == k]
    return want


def flat(got):
    return {p: a.reshape((-1,) + ((3,) if PATH_PLANES[p][1] == 3 else ())) for p, a in got.items()}


def same(got, want, what, names=PLANES):
    for p in names:
        assert got[p].dtype == want[p].dtype and got[p].size == want[p].size, (what, p)
        differ = (bits(got[p]).reshape(len(want[p]), -1) != bits(want[p]).reshape(len(want[p]), -1)).any(axis=1)
        assert not differ.any(), "%s: plane %s differs at %d samples, first %d" % (what, p, differ.sum(), np.flatnonzero(differ)[0])


def on_device(ctx, name, form, counts, cap=CAP, bounces=B, seed=SEED, count_order=False, names=PLANES, rays=None):
    """the _device variant into guarded device planes (and a guarded scratch in count order): the planes as flat arrays;
    everything behind a plane and behind the scratch keeps the pattern"""
    scene, cam, opts = oc.load(name)
    rays = oc.ray_set(name, "eyeless") if rays is None and form == "rays" else rays
    n = len(counts)
    dev = {p: DeviceBytes(Q.plane_bytes(PATH_PLANES, p, n) + GUARD) for p in names}
    dev["counts"] = DeviceBytes(n)
    need = c2.paths_counted_scratch_bytes(n)
    if count_order:
        dev["scratch"] = DeviceBytes(need + GUARD)
    if form == "rays":
        dev["rays"] = DeviceBytes(rays.nbytes)
    try:
        hip = dev["counts"].hip
        assert hip.hipMemcpy(dev["counts"].ptr, counts.ctypes.data, n, 1) == 0
        if form == "rays":
            assert hip.hipMemcpy(dev["rays"].ptr, rays.ctypes.data, rays.nbytes, 1) == 0
        ptrs = {p: dev[p].ptr.value for p in names}
        scratch = dev["scratch"].ptr.value if count_order else 0
        if form == "frame":
            ctx.renderPathsCountedDevice(cam, opts, dev["counts"].ptr.value, cap, bounces, ptrs, seed=seed, scratch_ptr=scratch)
        else:
            ctx.traceRaysPathsCountedDevice(dev["rays"].ptr.value, n, dev["counts"].ptr.value, cap, bounces, ptrs, seed=seed, scratch_ptr=scratch)
        assert hip.hipDeviceSynchronize() == 0
        out = {}
        for p in names:
            raw, nb = dev[p].get(), Q.plane_bytes(PATH_PLANES, p, n)
            assert (raw[nb:] == SENTINEL).all(), (p, "guard")
            dtype, comps = PATH_PLANES[p]
            out[p] = raw[:nb].view(dtype).reshape((n,) if comps == 1 else (n, comps))
        if count_order:
            raw = dev["scratch"].get()
            assert (raw[need:] == SENTINEL).all(), "scratch guard"
            if set(names) == {"node"}:
                assert (raw == SENTINEL).all(), "`node` alone sorts nothing"
            else:
                order = raw[512:512 + 4 * n].view(np.uint32)
                assert np.array_equal(np.sort(order), np.arange(n)), "the scratch holds a permutation"
                c = np.minimum(counts, cap)[order]
                assert (np.diff(c.astype(int)) <= 0).all(), "heaviest class first"
        assert (dev["counts"].get() == counts).all()
        return out
    finally:
        Q.free_all(dev)


def samples(ctx, name, form):
    """(counts in the form's natural layout, flat; the ray's own colour, flat; the hit mask)"""
    scene, cam, opts = load(ctx, name)
    if form == "frame":
        counts = layout(tile_wave())
        rgb = ctx.renderHits(cam, opts, planes=("rgb",))["rgb"].reshape(-1, 3)
    else:
        rays = oc.ray_set(name, "eyeless")
        counts = layout(np.arange(len(rays)) // 64)
        rgb = ctx.traceRays(rays, hits=False)[1]
    return counts, rgb, uniform(ctx, name, form, CAP)["node"] >= 0


def call_host(ctx, name, form, counts, cap=CAP, bounces=B, seed=SEED, planes=PLANES):
    scene, cam, opts = oc.load(name)
    if form == "frame":
        return flat(ctx.renderPathsCounted(cam, opts, counts.reshape(H, W), cap, bounces, seed, planes=planes))
    return flat(ctx.traceRaysPathsCounted(oc.ray_set(name, "eyeless"), counts, cap, bounces, seed, planes=planes))


# ---- 1. counted against uniform ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("form", ["frame", "rays"])
@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_every_sample_is_the_uniform_call_of_its_own_count(gpu_ctx, name, form):
    counts, rgb, hit = samples(gpu_ctx, name, form)
    n = len(counts)
    assert n % 64 != 0 and set(np.unique(counts)) == set(int(v) for v in VALUES)
    c = np.minimum(counts, CAP)
    per_class = {int(k): int((hit & (c == k)).sum()) for k in np.unique(c)}
    print(name, form, "hit samples per class", per_class)
    assert set(per_class) == {0, 1, 2, 3, 5, 8} and min(per_class.values()) >= 20, per_class
    want = expected(gpu_ctx, name, form, counts, rgb)
    got = call_host(gpu_ctx, name, form, counts)
    same(got, want, (name, form))
    # class 0, spelled out: the record's node, no segment, +0 three times twice, the ray's own colour
    z = c == 0
    assert (z & hit).sum() >= 20 and np.array_equal(got["node"][z], uniform(gpu_ctx, name, form, 1)["node"][z])
    assert not got["segments"][z].any() and not bits(got["indirect"][z]).any() and not bits(got["bounce"][z]).any()
    assert bits(got["radiance"][z]).tobytes() == bits(rgb[z]).tobytes() and bits(rgb[z & hit]).any()
    # the classes differ from one another where it matters: a sample at 2 paths is not the sample at 8
    two = (c == 2) & hit
    assert (bits(got["indirect"][two]) != bits(uniform(gpu_ctx, name, form, CAP)["indirect"][two])).any()


# ---- 2. the two launch orders ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("form", ["frame", "rays"])
@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_natural_order_and_count_order_give_the_same_bits(gpu_ctx, name, form):
    counts, rgb, _ = samples(gpu_ctx, name, form)
    for what, plane in (("mixed", counts), ("all equal", np.full_like(counts, 3))):
        want = expected(gpu_ctx, name, form, plane, rgb)
        natural = on_device(gpu_ctx, name, form, plane)
        sorted_ = on_device(gpu_ctx, name, form, plane, count_order=True)
        same(natural, want, (name, form, what, "natural order"))
        same(sorted_, want, (name, form, what, "count order"))
    # `node` alone reads no count and sorts nothing: the scratch keeps the pattern (on_device checks its guard; here all of it)
    alone = on_device(gpu_ctx, name, form, counts, count_order=True, names=("node",))
    assert np.array_equal(alone["node"], uniform(gpu_ctx, name, form, CAP)["node"])


# ---- 3. counts at or above the cap; subsets ----------------------------------------------------------------------------------


def test_counts_at_or_above_the_cap_are_the_uniform_call(gpu_ctx):
    name = "csg_stress"
    for form in ("frame", "rays"):
        counts, _, _ = samples(gpu_ctx, name, form)
        high = np.array([CAP, CAP + 1, 200, 255], dtype=np.uint8)[(mix(np.arange(len(counts)), 3) % np.uint64(4)).astype(np.int64)]
        same(call_host(gpu_ctx, name, form, high), uniform(gpu_ctx, name, form, CAP), (name, form, "host"))
        same(on_device(gpu_ctx, name, form, high, count_order=True), uniform(gpu_ctx, name, form, CAP), (name, form, "count order"))
        # the cap is the call's: the same plane under a cap of 3
        same(call_host(gpu_ctx, name, form, high, cap=3), uniform(gpu_ctx, name, form, 3), (name, form, "cap 3"))


def test_plane_subsets_do_not_change_a_plane(gpu_ctx):
    name = "lecture5"
    scene, cam, opts = load(gpu_ctx, name)
    L = lib()
    for form in ("frame", "rays"):
        counts, rgb, _ = samples(gpu_ctx, name, form)
        n = len(counts)
        full = expected(gpu_ctx, name, form, counts, rgb)
        rays = oc.ray_set(name, "eyeless")
        for subset in [(p,) for p in PLANES] + [("node", "segments"), ("segments", "indirect"), ("indirect", "radiance")]:
            bufs = guarded(PATH_PLANES, PLANES, n, align=8)
            pl, g = struct_of(_abi.PathPlanes, {k: bufs[k] for k in subset}), p_opts()
            if form == "frame":
                st = L.c2rt_render_paths_counted(gpu_ctx.handle, C.byref(cam), C.byref(opts), C.byref(g), counts.ctypes.data_as(C.c_void_p), C.byref(pl))
            else:
                st = L.c2rt_trace_rays_paths_counted(gpu_ctx.handle, rays.ctypes.data_as(C.c_void_p), n, C.byref(g), counts.ctypes.data_as(C.c_void_p), C.byref(pl))
            assert st == _abi.OK, last_error(gpu_ctx)
            assert untouched({k: v for k, v in bufs.items() if k not in subset}), (form, subset)
            Q.check_filled(PATH_PLANES, bufs, full, n, (form, subset), subset)
            if len(subset) == 2:
                same(on_device(gpu_ctx, name, form, counts, count_order=True, names=subset), full, (form, subset, "count order"), subset)


# ---- 4. host variants, chunks, strips, a posed scene --------------------------------------------------------------------------


def test_host_chunks_equal_the_device_variants(gpu_ctx):
    """2^18 + 70 rays under a cap of 2, B = 2: the second chunk starts at a non-zero index; its counts are the caller's at
    THAT index and its rays draw the paths of their own index.  The device variants take the array whole, in both orders
    (count order over 257 blocks of the sort)."""
    name = "lecture5"
    load(gpu_ctx, name)
    base = oc.ray_set(name, "eyeless")
    n = (1 << 18) + 70
    reps = np.arange(n) % len(base)
    rays = np.ascontiguousarray(base[reps])
    counts = np.array([0, 1, 2, 200], dtype=np.uint8)[(mix(np.arange(n), 9) % np.uint64(4)).astype(np.int64)]
    host = gpu_ctx.traceRaysPathsCounted(rays, counts, 2, 2, SEED)
    for count_order in (False, True):
        dev = on_device(gpu_ctx, name, "rays", counts, cap=2, bounces=2, count_order=count_order, rays=rays)
        same(dev, host, ("2^18 + 70 rays", count_order))
    c = np.minimum(counts, 2)
    for k in (1, 2):
        u = gpu_ctx.traceRaysPaths(rays, k, 2, SEED)
        same({p: host[p][c == k] for p in PLANES}, {p: u[p][c == k] for p in PLANES}, ("chunks", k))
    tail = np.arange((1 << 18), n)
    assert set(c[tail]) == {0, 1, 2} and not host["segments"][c == 0].any()


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_strips(gpu_ctx, name):
    scene, cam, opts = load(gpu_ctx, name)
    counts, rgb, _ = samples(gpu_ctx, name, "frame")
    grid = counts.reshape(H, W)
    want = expected(gpu_ctx, name, "frame", counts, rgb)
    full = {p: a.reshape((H, W) + a.shape[1:]) for p, a in want.items()}

    def render(o):
        rows = [y for y in range(H) if (y // 8) % 3 == o.strip_rank]
        return gpu_ctx.renderPathsCounted(cam, o, np.ascontiguousarray(grid[rows]), CAP, B, SEED)

    Q.check_strips(gpu_ctx, scene, render, full, H, 3, 8, PLANES, name)
    # a strip on the device, count order: the pixel's row in the FRAME comes from its index in the strip
    o = scene.renderOpts(taps=_abi.TAPS_1, strip_height=8, strip_rank=1, strip_world=3)
    rows = [y for y in range(H) if (y // 8) % 3 == 1]
    local = np.ascontiguousarray(grid[rows]).reshape(-1)
    dev = {p: DeviceBytes(Q.plane_bytes(PATH_PLANES, p, len(local)) + GUARD) for p in PLANES}
    dev["counts"], dev["scratch"] = DeviceBytes(len(local)), DeviceBytes(c2.paths_counted_scratch_bytes(len(local)) + GUARD)
    try:
        assert dev["counts"].hip.hipMemcpy(dev["counts"].ptr, local.ctypes.data, len(local), 1) == 0
        gpu_ctx.renderPathsCountedDevice(cam, o, dev["counts"].ptr.value, CAP, B, {p: dev[p].ptr.value for p in PLANES}, seed=SEED,
                                         scratch_ptr=dev["scratch"].ptr.value)
        assert dev["counts"].hip.hipDeviceSynchronize() == 0
        for p in PLANES:
            nb = Q.plane_bytes(PATH_PLANES, p, len(local))
            raw = dev[p].get()
            assert raw[:nb].tobytes() == bits(full[p][rows]).tobytes() and (raw[nb:] == SENTINEL).all(), p
    finally:
        Q.free_all(dev)


def test_posed_scene(gpu_ctx):
    name = "lecture5"
    scene, cam, opts = load(gpu_ctx, name)
    counts, _, _ = samples(gpu_ctx, name, "frame")
    before = call_host(gpu_ctx, name, "frame", counts)
    gpu_ctx.updateScene({3: U.xf(("translate", 60, 15, 200))})
    try:
        rgb = gpu_ctx.renderHits(cam, opts, planes=("rgb",))["rgb"].reshape(-1, 3)
        c = np.minimum(counts, CAP)
        posed = call_host(gpu_ctx, name, "frame", counts)
        sorted_ = on_device(gpu_ctx, name, "frame", counts, count_order=True)
        for k in (1, 2, 3, 5, 8):
            u = flat(gpu_ctx.renderPaths(cam, opts, k, B, SEED))
            for got in (posed, sorted_):
                same({p: got[p][c == k] for p in PLANES}, {p: u[p][c == k] for p in PLANES}, ("posed", k))
        assert bits(posed["radiance"][c == 0]).tobytes() == bits(rgb[c == 0]).tobytes()
        assert not np.array_equal(posed["node"], before["node"]) and (posed["segments"] != before["segments"]).sum() >= 30
    finally:
        gpu_ctx.uploadScene(scene.desc)


# ---- 5. c2rt_path_counts against the restatement --------------------------------------------------------------------------------

TEMPORAL = dict(max_age=vc.MAX_AGE, min_normal_dot=tc.MIN_NORMAL_DOT, max_plane_dist=tc.MAX_PLANE_DIST)
GATES = dict(min_normal_dot=tc.MIN_NORMAL_DOT, max_plane_dist=tc.MAX_PLANE_DIST)
# min 2 / max 16 / young 6, old enough from age 2; paths_per_variance so that the sequences' variances (P = 8, B = 2) fall below
# min_paths, between and above max_paths (the test prints and asserts the classes)
RULE = dict(min_paths=2, max_paths=16, young_paths=6, min_age=2, paths_per_variance=400.0, prev_paths=8)
_sequences = {}


def sequence(ctx, name):
    """for each camera of the four-frame sequence: the guides, the uniform indirect (P = 8, B = 2, seed + i) and the history
    the library's own accumulation leaves behind it; rendered once, read-only"""
    scene, cams, opts = tc.sequence(name)
    ctx.uploadScene(scene.desc)
    if name not in _sequences:
        out, hist = [], None
        for i, cam in enumerate(cams):
            f = dict(ctx.renderHits(cam, opts, planes=("node", "normal", "p")))
            f["indirect"] = ctx.renderPaths(cam, opts, 8, 2, seed=SEED + i, planes=("indirect",))["indirect"]
            _, hist = ctx.temporalAccumulate(f, f["indirect"], prev_cam=cams[i - 1] if i else None, history=hist, planes=(), **TEMPORAL)
            f["history"] = hist
            for a in f.values():
                a.setflags(write=False)
            out.append(f)
        _sequences[name] = out
    return _sequences[name]


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_path_counts_match_the_restatement(gpu_ctx, name):
    fs = sequence(gpu_ctx, name)
    _, cams, _ = tc.sequence(name)
    px = W * H
    for with_counts in (True, False):
        classes = {}
        prev_counts = None
        for i, f in enumerate(fs):
            kw = dict(prev_cam=cams[i - 1] if i else None, history=fs[i - 1]["history"] if i else None)
            given = prev_counts if (with_counts and i) else None
            got = gpu_ctx.pathCounts(f, prev_counts=given, **kw, **GATES, **RULE)
            want = cr.path_counts(f["node"], f["normal"], f["p"], 3, prev_counts=given, classes=classes, **kw, **GATES, **RULE)
            what = (name, with_counts, i)
            assert got["counts"].dtype == np.uint8 and got["counts"].shape == (H, W) and got["variance"].dtype == np.float32 and got["age"].dtype == np.uint32
            assert np.array_equal(got["counts"], want["counts"]), (what, int((got["counts"] != want["counts"]).sum()))
            assert tr.count_differing(got["variance"], want["variance"]) == 0 and np.array_equal(got["age"], want["age"]), what
            if i:
                assert got["age"].max() == i and (got["counts"][f["node"] < 0] == 0).all()
            # the counts "traced" next: a plane with every value of the rule in it, and zeros, which the rule reads as 1
            prev_counts = np.where(mix(np.arange(px), i).reshape(H, W) % np.uint64(5) == 0, 0, want["counts"]).astype(np.uint8)
        print(name, "prev_counts" if with_counts else "prev_paths", classes)
        assert min(classes[k] for k in cr.CLASSES) >= 20, classes
        assert sum(classes.values()) == 4 * px
    # the device variant against the host variant, frame 2: every plane, then counts alone
    i, f = 2, fs[2]
    host = gpu_ctx.pathCounts(f, prev_cam=cams[1], history=fs[1]["history"], prev_counts=prev_counts, **GATES, **RULE)
    dev = {k: DeviceBytes(bits(f[k]).nbytes) for k in ("node", "normal", "p")}
    dev.update(history=DeviceBytes(fs[1]["history"].nbytes), prev=DeviceBytes(px), counts=DeviceBytes(px + GUARD), variance=DeviceBytes(px * 4 + GUARD),
               age=DeviceBytes(px * 4 + GUARD))
    try:
        hip = dev["node"].hip
        for k, a in (("node", f["node"]), ("normal", f["normal"]), ("p", f["p"]), ("history", fs[1]["history"]), ("prev", prev_counts)):
            assert hip.hipMemcpy(dev[k].ptr, bits(a).ctypes.data, dev[k].nbytes, 1) == 0
        at = {k: d.ptr.value for k, d in dev.items()}
        ptrs = {k: at[k] for k in ("node", "normal", "p")}
        gpu_ctx.pathCountsDevice(ptrs, W, H, at["history"], at["prev"], at["counts"], prev_cam=cams[1], **GATES, **RULE)
        assert hip.hipDeviceSynchronize() == 0
        assert (dev["variance"].get() == SENTINEL).all() and (dev["age"].get() == SENTINEL).all()
        raw = dev["counts"].get()
        assert raw[:px].tobytes() == host["counts"].tobytes() and (raw[px:] == SENTINEL).all()
        gpu_ctx.pathCountsDevice(ptrs, W, H, at["history"], at["prev"], at["counts"], at["variance"], at["age"], prev_cam=cams[1], **GATES, **RULE)
        assert hip.hipDeviceSynchronize() == 0
        for k, n in (("counts", px), ("variance", px * 4), ("age", px * 4)):
            raw = dev[k].get()
            assert raw[:n].tobytes() == bits(host[k]).tobytes() and (raw[n:] == SENTINEL).all(), k
    finally:
        Q.free_all(dev)


# ---- 6. the sequence in one call ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", oc.SCENE_NAMES)
def test_render_paths_sequence_adaptive_is_the_composition(gpu_ctx, name):
    scene, cams, opts = tc.sequence(name)
    gpu_ctx.uploadScene(scene.desc)
    cams = cams[:3]
    rule = dict(min_paths=2, max_paths=CAP, young_paths=6, min_age=1, paths_per_variance=400.0)
    kw = dict(levels=3, sigma_lum=vc.SIGMA_LUM, min_age=vc.MIN_AGE)
    want, hist, counts, seen = [], None, None, set()
    for i, cam in enumerate(cams):
        f = dict(gpu_ctx.renderHits(cam, opts, planes=("node", "normal", "p", "rgb")))
        albedo = gpu_ctx.renderShading(cam, opts, planes=("albedo",))["albedo"]
        if i == 0:
            counts = np.full((H, W), rule["young_paths"], dtype=np.uint8)
        else:
            counts = gpu_ctx.pathCounts(f, prev_cam=cams[i - 1], history=hist, prev_counts=counts, prev_paths=rule["young_paths"], planes=(), **GATES, **rule)["counts"]
            seen |= set(np.unique(counts))
        indirect = gpu_ctx.renderPathsCounted(cam, opts, counts, CAP, 2, seed=SEED + i, planes=("indirect",))["indirect"]
        t, hist = gpu_ctx.temporalAccumulate(f, indirect, prev_cam=cams[i - 1] if i else None, history=hist, **TEMPORAL)
        want.append(gpu_ctx.denoiseVariance(f, t["colour"], t["variance"], t["age"], albedo=albedo, base=f["rgb"], variance_out=False, **kw)[0])
    assert len(seen) >= 4 and 0 in seen, seen                                                  # the sampler really varied the counts
    generation = gpu_ctx.sceneGeneration
    args = dict(seed=SEED, min_paths=2, max_paths=CAP, young_paths=6, count_min_age=1, paths_per_variance=400.0, **TEMPORAL, **kw)
    got = gpu_ctx.renderPathsSequenceAdaptive(cams, opts, CAP, 2, **args)
    assert got.shape == (3, H, W, 3) and got.dtype == np.float32
    for i in range(3):
        assert bits(got[i]).tobytes() == bits(want[i]).tobytes(), (name, i)
    one = gpu_ctx.renderPathsSequenceAdaptive(cams[:1], opts, CAP, 2, **args)
    assert bits(one[0]).tobytes() == bits(want[0]).tobytes()
    assert gpu_ctx.sceneGeneration == generation
    # the context's scene is the one uploaded: a plain frame afterwards is the frame before
    uniform_frame = gpu_ctx.renderPathsSequenceVariance(cams[:1], opts, 6, 2, seed=SEED, **TEMPORAL, **kw)
    assert bits(uniform_frame[0]).tobytes() == bits(want[0]).tobytes()                         # young_paths everywhere is the uniform call at 6


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------


def test_counted_refusals_leave_the_outputs_untouched(gpu_ctx):
    name = "lecture5"
    scene, cam, opts = load(gpu_ctx, name)
    counts, rgb, _ = samples(gpu_ctx, name, "frame")
    L = lib()
    n = W * H
    bufs = guarded(PATH_PLANES, PLANES, n, align=8)
    pl, none, good = struct_of(_abi.PathPlanes, bufs), _abi.PathPlanes(), p_opts()
    cp = counts.ctypes.data_as(C.c_void_p)
    scratch = Q.sentinel_bytes(c2.paths_counted_scratch_bytes(n), 16)
    E, LIM, UNS = _abi.ERR_INVALID_ARG, _abi.ERR_LIMIT, _abi.ERR_UNSUPPORTED
    dof = Q.with_fields(cam, dof=1, num_samples=4)

    def frame(c, o, g, cnt, planes, scratch_ptr=None, device_only=False):
        a = (None if c is None else C.byref(c), C.byref(o), None if g is None else C.byref(g), cnt, None if planes is None else C.byref(planes))
        st = L.c2rt_render_paths_counted_device(gpu_ctx.handle, *a, scratch_ptr, None)
        msg = last_error(gpu_ctx)
        if not device_only:
            assert L.c2rt_render_paths_counted(gpu_ctx.handle, *a) == st and last_error(gpu_ctx) == msg
        return st, msg

    # the path call's own come first, in its order, with null counts and a misaligned scratch present as well
    odd = scratch.ctypes.data + 4
    assert frame(None, opts, good, None, pl, odd)[0] == E
    assert frame(cam, opts, None, None, pl, odd) == (E, "null path options")
    assert frame(cam, opts, p_opts(paths=0), None, pl, odd) == (E, "paths is 0: at least one path")
    assert frame(cam, opts, p_opts(paths=65), None, pl, odd) == (LIM, "65 paths (at most 64)")
    assert frame(cam, opts, p_opts(bounces=9), None, pl, odd) == (LIM, "9 bounces (at most 8)")
    assert frame(cam, opts, good, None, None, odd) == (E, "null planes")
    assert frame(cam, opts, good, None, none, odd) == (E, "no plane asked for: all five pointers of c2rt_path_planes are null")
    assert frame(dof, opts, good, None, pl, odd) == (UNS, "depth of field: a pixel's paths are one ray's, a lens has many per pixel")
    assert frame(cam, Q.with_fields(opts, count_rays=1), good, None, pl, odd) == (UNS, "count_rays: the path planes do not count rays")
    # then the counts, then the scratch's alignment (the device variants only)
    assert frame(cam, opts, good, None, pl, odd) == (E, "null counts")
    assert frame(cam, opts, good, cp, pl, odd, device_only=True) == (E, "the count-order scratch is not 16-byte aligned")
    fresh = c2.Context(0)
    try:
        assert L.c2rt_render_paths_counted(fresh.handle, C.byref(cam), C.byref(opts), C.byref(good), None, C.byref(pl)) == _abi.ERR_NO_SCENE
    finally:
        fresh.close()

    rays = oc.ray_set(name, "eyeless")
    rcounts = layout(np.arange(len(rays)) // 64)
    rbufs = guarded(PATH_PLANES, PLANES, len(rays), align=8)
    rpl = struct_of(_abi.PathPlanes, rbufs)
    rp, rcp, m = rays.ctypes.data_as(C.c_void_p), rcounts.ctypes.data_as(C.c_void_p), len(rays)
    for fn, tail in ((L.c2rt_trace_rays_paths_counted, ()), (L.c2rt_trace_rays_paths_counted_device, (odd, None))):
        assert fn(None, rp, m, C.byref(good), rcp, C.byref(rpl), *tail) == E
        assert fn(gpu_ctx.handle, None, 0, None, None, None, *tail) == _abi.OK                         # n == 0, whatever else
        assert fn(gpu_ctx.handle, None, m, None, None, None, *tail) == E and "null input array" in last_error(gpu_ctx)
        assert fn(gpu_ctx.handle, rp, _abi.MAX_RAYS + 1, None, None, None, *tail) == LIM
        assert fn(gpu_ctx.handle, rp, m, None, None, C.byref(rpl), *tail) == E and last_error(gpu_ctx) == "null path options"
        assert fn(gpu_ctx.handle, rp, m, C.byref(p_opts(paths=65)), None, None, *tail) == LIM
        assert fn(gpu_ctx.handle, rp, m, C.byref(good), None, None, *tail) == E and last_error(gpu_ctx) == "null planes"
        assert fn(gpu_ctx.handle, rp, m, C.byref(good), None, C.byref(none), *tail) == E and "no plane asked for" in last_error(gpu_ctx)
        assert fn(gpu_ctx.handle, rp, m, C.byref(good), None, C.byref(rpl), *tail) == E and last_error(gpu_ctx) == "null counts"
    assert L.c2rt_trace_rays_paths_counted_device(gpu_ctx.handle, rp, m, C.byref(good), rcp, C.byref(rpl), odd, None) == E
    assert last_error(gpu_ctx) == "the count-order scratch is not 16-byte aligned"
    assert untouched(bufs) and untouched(rbufs) and untouched([scratch])
    # afterwards the same context fills a correct plane set
    assert L.c2rt_render_paths_counted(gpu_ctx.handle, C.byref(cam), C.byref(opts), C.byref(good), cp, C.byref(pl)) == _abi.OK, last_error(gpu_ctx)
    Q.check_filled(PATH_PLANES, bufs, expected(gpu_ctx, name, "frame", counts, rgb), n, "after the refusals")


def test_path_counts_refusals_in_the_documented_order(gpu_ctx):
    """Every refusal of c2rt_path_counts_device with every LATER violation present as well (where two set the same
    argument, the earlier one's value): the status and message are the first one's.  Nothing is enqueued: the outputs keep
    the pattern.  max_age is not looked at: it is 0 throughout."""
    px = 8 * 8
    L = lib()
    dev = {k: DeviceBytes(n) for k, n in (("node", px * 4), ("normal", px * 24), ("p", px * 24), ("history", px * 52 + 16), ("prev", px), ("counts", px),
                                          ("variance", px * 4), ("age", px * 4))}
    at = {k: d.ptr.value for k, d in dev.items()}
    _, cams, _ = tc.sequence("lecture5")
    cam = cams[0]
    flat_cam = Q.with_fields(cam, up_right=cam.up_left)
    good = dict(ctx=gpu_ctx.handle, opts=True, guides=True, pc=True, width=8, height=8, channels=3, min_normal_dot=0.9, max_plane_dist=0.1, t_reserved=0,
                min_paths=2, max_paths=32, young_paths=16, min_age=2, prev_paths=8, ppv=100.0, pc_reserved=0, node=at["node"], normal=at["normal"], p=at["p"],
                counts=at["counts"], cam=cam, history=at["history"])
    E, LIM = _abi.ERR_INVALID_ARG, _abi.ERR_LIMIT
    steps = [  # (fields that turn bad, status, word of the message)
        (dict(ctx=None), E, None),
        (dict(opts=False), E, "null temporal options"),
        (dict(guides=False), E, "null temporal guides"),
        (dict(width=0), E, "above 0"),
        (dict(channels=2), E, "channels"),
        (dict(min_normal_dot=1.0), E, "min_normal_dot"),
        (dict(max_plane_dist=0.0), E, "max_plane_dist"),
        (dict(t_reserved=1), E, "c2rt_temporal_opts.reserved"),
        (dict(pc=False), E, "null path count options"),
        (dict(min_paths=0), E, "min_paths is 0"),
        (dict(min_paths=65, max_paths=65), LIM, "min_paths is 65"),
        (dict(max_paths=1), E, "below min_paths"),
        (dict(max_paths=65), LIM, "max_paths is 65"),
        (dict(young_paths=0), E, "young_paths is 0"),
        (dict(young_paths=65), LIM, "young_paths is 65"),
        (dict(min_age=65536), LIM, "min_age is 65536"),
        (dict(prev_paths=0), E, "prev_paths is 0"),
        (dict(prev_paths=65), LIM, "prev_paths is 65"),
        (dict(ppv=float("nan")), E, "paths_per_variance"),
        (dict(pc_reserved=1), E, "c2rt_path_count_opts.reserved"),
        (dict(node=None), E, "node"),
        (dict(normal=None), E, "normal"),
        (dict(p=None), E, ": p"),
        (dict(counts=None), E, "null counts"),
        (dict(cam=None), E, "null prev_cam"),
        (dict(cam=flat_cam), E, "degenerate previous camera"),
        (dict(history=at["history"] + 4), E, "16-byte"),
    ]

    def call(v, host=False):
        o = _abi.TemporalOpts(width=v["width"], height=v["height"], channels=v["channels"], max_age=0, min_normal_dot=v["min_normal_dot"],
                              max_plane_dist=v["max_plane_dist"], reserved=(0, v["t_reserved"]))
        pc = _abi.PathCountOpts(min_paths=v["min_paths"], max_paths=v["max_paths"], young_paths=v["young_paths"], min_age=v["min_age"],
                                paths_per_variance=v["ppv"], prev_paths=v["prev_paths"], reserved=(v["pc_reserved"], 0))
        g = _abi.TemporalGuides(node=v["node"], normal=v["normal"], p=v["p"])
        a = (v["ctx"], None if v["cam"] is None else C.byref(v["cam"]), C.byref(g) if v["guides"] else None, C.byref(o) if v["opts"] else None,
             C.byref(pc) if v["pc"] else None, v["history"], at["prev"], v["counts"], at["variance"], at["age"])
        return L.c2rt_path_counts_device(*a, None)

    outputs = ("counts", "variance", "age")
    try:
        hip = dev["node"].hip
        assert hip.hipMemset(dev["node"].ptr, 0xFF, px * 4) == 0                      # all misses: counts 0, variance +0, age 0
        assert call(good) == _abi.OK, last_error(gpu_ctx)
        assert hip.hipDeviceSynchronize() == 0
        for k in outputs:
            assert not dev[k].get().any(), k                                          # the valid call ran
        assert call(dict(good, history=None, cam=None)) == _abi.OK, last_error(gpu_ctx)
        for bad in (float("inf"), 0.0, -1.0):
            assert call(dict(good, ppv=bad)) == E and "paths_per_variance" in last_error(gpu_ctx)
        assert hip.hipDeviceSynchronize() == 0
        for k in outputs:
            assert hip.hipMemset(dev[k].ptr, SENTINEL, dev[k].nbytes) == 0
        for i, (_, status, word) in enumerate(steps):
            v = dict(good)
            for bad, _, _ in reversed(steps[i:]):
                v.update(bad)
            assert call(v) == status, (i, word, last_error(gpu_ctx))
            if word:
                assert word in last_error(gpu_ctx), (i, word, last_error(gpu_ctx))
        assert hip.hipDeviceSynchronize() == 0
        for k in outputs:
            assert (dev[k].get() == SENTINEL).all(), k
    finally:
        Q.free_all(dev)
    # the host variant decides the same, and needs no alignment
    fs = sequence(gpu_ctx, "lecture5")
    f = fs[1]
    out = Q.sentinel_bytes(W * H)
    g = _abi.TemporalGuides(node=f["node"].ctypes.data, normal=f["normal"].ctypes.data, p=f["p"].ctypes.data)
    o = _abi.TemporalOpts(width=W, height=H, channels=3, max_age=0, min_normal_dot=0.9, max_plane_dist=0.1)
    pc = _abi.PathCountOpts(**dict(RULE, min_paths=0))
    hist = np.concatenate([np.zeros(1, dtype=np.uint8), fs[0]["history"]])[1:]                # a history at an odd address
    args = (C.byref(cams[0]), C.byref(g), C.byref(o))
    assert L.c2rt_path_counts(gpu_ctx.handle, *args, C.byref(pc), hist.ctypes.data, None, out.ctypes.data, None, None) == E and "min_paths is 0" in last_error(gpu_ctx)
    pc = _abi.PathCountOpts(**RULE)
    assert L.c2rt_path_counts(gpu_ctx.handle, *args, C.byref(pc), hist.ctypes.data, None, None, None, None) == E and last_error(gpu_ctx) == "null counts"
    assert L.c2rt_path_counts(gpu_ctx.handle, None, *args[1:], C.byref(pc), hist.ctypes.data, None, out.ctypes.data, None, None) == E and "null prev_cam" in last_error(gpu_ctx)
    assert untouched([out])
    assert L.c2rt_path_counts(gpu_ctx.handle, *args, C.byref(pc), hist.ctypes.data, None, out.ctypes.data, None, None) == _abi.OK, last_error(gpu_ctx)
    want = cr.path_counts(f["node"], f["normal"], f["p"], 3, prev_cam=cams[0], history=fs[0]["history"], **GATES, **RULE)["counts"]
    assert out.tobytes() == want.tobytes()


def test_adaptive_sequence_refusals(gpu_ctx):
    scene, cams, opts = tc.sequence("lecture5")
    gpu_ctx.uploadScene(scene.desc)
    L = lib()
    px = W * H
    seq = Q.sentinel_bytes(3 * px * 12)
    pg = _abi.PathOpts(seed=SEED, paths=CAP, bounces=2)
    t = _abi.TemporalOpts(width=W, height=H, channels=3, max_age=8, min_normal_dot=0.9, max_plane_dist=0.1)
    d = _abi.DenoiseVarianceOpts(width=W, height=H, levels=3, channels=3, normal_power_log2=5, sigma_plane=1.0, sigma_lum=4.0, var_floor=1e-8, min_age=4)
    arr = (_abi.CameraFrame * 3)(*cams[:3])
    flat_cams = (_abi.CameraFrame * 3)(cams[0], Q.with_fields(cams[1], up_right=cams[1].up_left), cams[2])

    def pc(**kw):
        return _abi.PathCountOpts(**dict(dict(min_paths=2, max_paths=CAP, young_paths=6, min_age=1, paths_per_variance=400.0, prev_paths=6), **kw))

    E, LIM = _abi.ERR_INVALID_ARG, _abi.ERR_LIMIT
    bad = pc(min_paths=0, max_paths=9)
    for cams_, n, pg_, t_, d_, pc_, outp, status, word in (
            (None, 3, pg, t, d, None, seq.ctypes.data, E, "camera"),                                      # the variance call's first, in its order
            (arr, 3, Q.with_fields(pg, paths=0), t, d, None, seq.ctypes.data, E, "paths is 0"),
            (arr, 3, pg, t, None, None, seq.ctypes.data, E, "null denoise options"),
            (arr, 3, pg, t, d, None, None, E, "null output"),
            (arr, 3, pg, t, Q.with_fields(d, levels=9), None, seq.ctypes.data, LIM, "levels"),
            (arr, 0, pg, t, d, None, seq.ctypes.data, E, "n_frames"),
            (arr, 3, pg, None, d, None, seq.ctypes.data, E, "null temporal options"),
            (arr, 3, pg, Q.with_fields(t, max_age=0), d, bad, seq.ctypes.data, LIM, "max_age"),
            (flat_cams, 3, pg, t, d, None, seq.ctypes.data, E, "degenerate previous camera"),
            (arr, 3, pg, t, d, None, seq.ctypes.data, E, "null path count options"),                       # then the new ones
            (arr, 3, pg, t, d, bad, seq.ctypes.data, E, "min_paths is 0"),
            (arr, 3, pg, t, d, pc(max_paths=65), seq.ctypes.data, LIM, "max_paths is 65"),
            (arr, 3, pg, t, d, pc(paths_per_variance=0.0, max_paths=9), seq.ctypes.data, E, "paths_per_variance"),
            (arr, 3, pg, t, d, pc(reserved=(0, 1), max_paths=9), seq.ctypes.data, E, "c2rt_path_count_opts.reserved"),
            (arr, 3, pg, t, d, pc(max_paths=9), seq.ctypes.data, E, "above the cap")):
        st = L.c2rt_render_paths_sequence_adaptive(gpu_ctx.handle, cams_, n, C.byref(opts), C.byref(pg_), None if t_ is None else C.byref(t_),
                                                   None if d_ is None else C.byref(d_), None if pc_ is None else C.byref(pc_), outp)
        assert st == status, (word, last_error(gpu_ctx))
        assert word in last_error(gpu_ctx), (word, last_error(gpu_ctx))
    assert untouched([seq])
