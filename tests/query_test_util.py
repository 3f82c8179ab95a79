"""Shared by the GPU tests of the query families (hit, shading, occlusion and gather planes, their batch, tap and
adaptive relatives): the helpers that decide whether a failure is seen — the sentinel, the guards behind every buffer,
the bit compare — the raw library access, and one descriptor per plane family.  A new family's test starts here."""
import collections
import ctypes as C

import numpy as np
import pytest

import chess2rt_amd as c2
import occlusion_cases as oc
from chess2rt_amd import _abi
from chess2rt_amd.api import GATHER_PLANES, HIT_PLANES, OCCLUSION_PLANES, SHADE_PLANES
from ray_query_util import bits

SENTINEL = 0xA5


# ---- library access ----------------------------------------------------------------------------------------------------


def lib():
    return _abi.load_library()


def last_error(ctx):
    return lib().c2rt_last_error(ctx.handle).decode(errors="replace")


def hip_runtime():
    """the HIP runtime the library is linked against, reached through the library's own handle (a second copy of the
    runtime, as C.CDLL("libamdhip64.so") can map, must not be handed the first one's streams or pointers)"""
    hip = lib()
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


@pytest.fixture(scope="module")
def scratch_ctx():
    ctx = c2.Context(0)
    yield ctx
    ctx.close()


def with_fields(struct, **kw):
    """a copy of a ctypes struct with the named fields set"""
    s = type(struct).from_buffer_copy(struct)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


# ---- bits ----------------------------------------------------------------------------------------------------------------


def float_bits(a):
    """float32 as its words, so that a count of differences is a count of floats; anything else as bytes"""
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bits(a).tobytes() == bits(b).tobytes()


def same_planes(got, want, what, names):
    for name in names:
        assert got[name].dtype == want[name].dtype and got[name].size == want[name].size, (what, name)
        assert bits(got[name]).tobytes() == bits(want[name]).tobytes(), "%s: plane %s differs" % (what, name)


# ---- guarded buffers ---------------------------------------------------------------------------------------------------


def guard_size(itemsize, guard_elems=None, guard_bytes=None):
    """the guard behind a buffer in bytes, stated in elements of the buffer's type or in bytes: one of the two"""
    assert (guard_elems is None) != (guard_bytes is None)
    return guard_bytes if guard_elems is None else guard_elems * itemsize


def sentinel_bytes(nbytes, align=1):
    """`nbytes` of SENTINEL, rounded up to a multiple of `align`, at an address that is one"""
    nbytes = -(-nbytes // align) * align
    raw = np.full(nbytes + align, SENTINEL, dtype=np.uint8)
    first = -raw.ctypes.data % align
    return raw[first:first + nbytes]


def plane_bytes(table, name, samples):
    dtype, comps = table[name]
    return samples * comps * np.dtype(dtype).itemsize


def guarded(table, names, samples, guard_elems=64, align=1):
    """{name: host byte buffer of the plane plus `guard_elems` elements of its type, all SENTINEL}"""
    return {n: sentinel_bytes(plane_bytes(table, n, samples) + guard_size(np.dtype(table[n][0]).itemsize, guard_elems), align) for n in names}


def frame_and_mask(pixels, guard_elems=None, guard_bytes=None):
    """host buffers of a float32 frame and a byte mask of `pixels` pixels, a guard behind each, all SENTINEL"""
    return sentinel_bytes(pixels * 12 + guard_size(4, guard_elems, guard_bytes)), sentinel_bytes(pixels + guard_size(1, guard_elems, guard_bytes))


def struct_of(struct_cls, bufs):
    """the plane struct whose members point at `bufs` ({name: host buffer, DeviceBytes or address}); the others stay null"""
    pl = struct_cls()
    for n, b in bufs.items():
        setattr(pl, n, b.ctypes.data if isinstance(b, np.ndarray) else b.ptr.value if isinstance(b, DeviceBytes) else b)
    return pl


def untouched(bufs):
    """every byte of every buffer ({name: buffer} or any iterable of buffers) is still SENTINEL"""
    return all((b == SENTINEL).all() for b in (bufs.values() if isinstance(bufs, dict) else bufs))


def payload_and_guard(buf, nbytes):
    return buf[:nbytes], buf[nbytes:]


def holds(buf, want):
    """the byte buffer holds the bits of `want`, then nothing but SENTINEL"""
    payload, guard = payload_and_guard(buf, bits(want).nbytes)
    return payload.tobytes() == bits(want).tobytes() and bool((guard == SENTINEL).all())


def check_filled(table, bufs, want, n, what, names=None):
    """bufs[name] holds the bits of want[name], `n` samples, then nothing but SENTINEL"""
    for name in (table if names is None else names):
        assert bits(want[name]).nbytes == plane_bytes(table, name, n), (what, name)
        assert holds(bufs[name], want[name]), (what, name)


class DeviceBytes:
    """`nbytes` of device memory filled with SENTINEL, allocated by the library's own runtime"""

    def __init__(self, nbytes):
        self.hip, self.nbytes, self.ptr = hip_runtime(), nbytes, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), nbytes) == 0
        assert self.hip.hipMemset(self.ptr, SENTINEL, nbytes) == 0
        assert self.hip.hipDeviceSynchronize() == 0

    def get(self):
        out = np.empty(self.nbytes, dtype=np.uint8)
        assert self.hip.hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0     # hipMemcpyDeviceToHost
        return out

    def free(self):
        if self.ptr:
            assert self.hip.hipFree(self.ptr) == 0
            self.ptr = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def guarded_device(table, names, samples, guard_elems=64):
    return {n: DeviceBytes(plane_bytes(table, n, samples) + guard_size(np.dtype(table[n][0]).itemsize, guard_elems)) for n in names}


def fetch(dev):
    """the buffers of guarded_device copied back (after a device sync)"""
    assert hip_runtime().hipDeviceSynchronize() == 0
    return {n: d.get() for n, d in dev.items()}


def free_all(dev):
    for d in dev.values():
        d.free()


def device_planes(table, n, dev, guard_elems=None, guard_bytes=None):
    """{name: torch byte tensor on `dev` of the plane plus its guard, all SENTINEL}"""
    import torch

    return {name: torch.full((plane_bytes(table, name, n) + guard_size(np.dtype(table[name][0]).itemsize, guard_elems, guard_bytes),), SENTINEL,
                             dtype=torch.uint8, device=dev) for name in table}


def check_device_against_host(table, t, host, n, what):
    check_filled(table, {name: t[name].cpu().numpy() for name in table}, host, n, what)


# ---- the plane families ------------------------------------------------------------------------------------------------

# table: {plane: (dtype, components)}; struct: the _abi struct of the plane pointers; frame .. rays_device: the names of
# the C entry points (None where the family has none); options: builds the family's option struct (None: it has none)
Family = collections.namedtuple("Family", "table struct frame frame_device rays rays_device options")


def occlusion_options(samples=oc.K, radius=50.0, seed=oc.SEED, reserved=0):
    return _abi.OcclusionOpts(radius=radius, seed=seed, samples=samples, reserved=reserved)


def gather_options(samples=oc.K, seed=oc.SEED, reserved=0):
    return _abi.GatherOpts(seed=seed, samples=samples, reserved=reserved)


HITS = Family(HIT_PLANES, _abi.HitPlanes, "c2rt_render_hits", "c2rt_render_hits_device", None, None, None)
SHADING = Family(SHADE_PLANES, _abi.ShadePlanes, "c2rt_render_shading", "c2rt_render_shading_device", "c2rt_trace_rays_shading",
                 "c2rt_trace_rays_shading_device", None)
OCCLUSION = Family(OCCLUSION_PLANES, _abi.OcclusionPlanes, "c2rt_render_occlusion", "c2rt_render_occlusion_device",
                   "c2rt_trace_rays_occlusion", "c2rt_trace_rays_occlusion_device", occlusion_options)
GATHER = Family(GATHER_PLANES, _abi.GatherPlanes, "c2rt_render_gather", "c2rt_render_gather_device", "c2rt_trace_rays_gather",
                "c2rt_trace_rays_gather_device", gather_options)


def raw_call(family, ctx, bufs, cam=None, opts=None, rays=None, n=None, options=None, null_struct=False, device=False, stream=None):
    """One of the family's entry points through the raw library: the frame call of (cam, opts), or with `n` the ray call
    over the first n of `rays`; host, or with `device` the device variant on `stream`.  Planes not in `bufs` are passed as
    null, and so are a context, camera, frame options, rays or family options of None."""
    def ref(x):
        return None if x is None else C.byref(x)

    if n is None:
        name, head = (family.frame_device if device else family.frame), [ref(cam), ref(opts)]
    else:
        name, head = (family.rays_device if device else family.rays), [None if rays is None else rays.ctypes.data_as(C.c_void_p), n]
    pl = struct_of(family.struct, bufs)
    args = [None if ctx is None else ctx.handle] + head + ([ref(options)] if family.options else []) + [None if null_struct else C.byref(pl)]
    return getattr(lib(), name)(*(args + ([stream] if device else [])))


def check_plane_subsets(family, ctx, cam, opts, rays, options, subsets, full, full_rays, pixels, what, align=1):
    """frame and ray call for every subset: what is not asked for is null in the struct and its buffer keeps the pattern;
    what is asked for holds the planes of the full calls (`full`, `pixels` samples, and `full_rays`)"""
    names = tuple(family.table)
    for subset in subsets:
        bufs, rbufs = guarded(family.table, names, pixels, align=align), guarded(family.table, names, len(rays), align=align)
        assert raw_call(family, ctx, {k: bufs[k] for k in subset}, cam, opts, options=options) == _abi.OK, last_error(ctx)
        assert raw_call(family, ctx, {k: rbufs[k] for k in subset}, rays=rays, n=len(rays), options=options) == _abi.OK, last_error(ctx)
        for b in (bufs, rbufs):
            assert untouched({k: v for k, v in b.items() if k not in subset}), (what, subset)
        check_filled(family.table, bufs, full, pixels, (what, subset), subset)
        check_filled(family.table, rbufs, full_rays, len(rays), (what, subset), subset)


def check_garbage_lanes(trace, rays0, want, hit, names, mask, K):
    """NaN and 0 in the middle of one wave and 1e300 in another: the call returns, every other ray keeps its planes, and
    whatever a garbage lane holds, its word of the plane `mask` has no bit at or above K"""
    rays = rays0.copy()
    wave = 5
    lanes = np.arange(64 * wave, 64 * wave + 64)
    assert hit[lanes].sum() >= 16
    where = {64 * wave + 21: np.nan, 64 * wave + 40: 0.0}                 # in the middle of one wave
    for i, v in where.items():
        rays[i] = v
    rays[64 * 9 + 3] = 1e300                                             # and one of 1e300 in another wave
    got = trace(rays)                                                    # the call returns
    keep = np.ones(len(rays), dtype=bool)
    keep[list(where) + [64 * 9 + 3]] = False
    assert keep[lanes].sum() == 62
    for p in names:
        assert bits(got[p][keep]).tobytes() == bits(want[p][keep]).tobytes(), p
    for i in where:
        assert not (int(got[mask][i]) >> K), i


def check_strips(ctx, scene, render, full, height, world, strip, names, what):
    """render(options of rank r of `world`) is the rows of `full` that rank owns, and every row has one owner"""
    seen = np.zeros(height, dtype=int)
    for rank in range(world):
        o = scene.renderOpts(taps=_abi.TAPS_1, strip_height=strip, strip_rank=rank, strip_world=world)
        rows = [y for y in range(height) if (y // strip) % world == rank]
        assert ctx.localRows(o) == len(rows)
        got = render(o)
        for name in names:
            assert got[name].shape[0] == len(rows)
            assert bits(got[name]).tobytes() == bits(full[name][rows]).tobytes(), (what, rank, name)
        seen[rows] += 1
    assert (seen == 1).all()
