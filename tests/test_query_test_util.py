"""tests/query_test_util.py on the CPU: the helpers every query family's GPU test sees its failures through.  A wrong
one blinds all of those files at once, so the sentinel, the guards, the bit compare and the plane structs are held to
numpy and ctypes here."""
import ctypes as C

import numpy as np
import pytest

import query_test_util as Q
from chess2rt_amd.api import GATHER_PLANES, HIT_PLANES, OCCLUSION_PLANES, SHADE_PLANES

FAMILIES = {"hits": Q.HITS, "shading": Q.SHADING, "occlusion": Q.OCCLUSION, "gather": Q.GATHER}
TABLES = {"hits": HIT_PLANES, "shading": SHADE_PLANES, "occlusion": OCCLUSION_PLANES, "gather": GATHER_PLANES}
SAMPLES = (1, 63, 64, 65)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_plane_bytes_is_numpys_item_size_times_the_components(family):
    fam = FAMILIES[family]
    assert fam.table is TABLES[family] and [f[0] for f in fam.struct._fields_] == list(fam.table)
    for name, (dtype, comps) in TABLES[family].items():
        for samples in SAMPLES:
            assert Q.plane_bytes(fam.table, name, samples) == np.zeros((samples, comps), dtype=dtype).nbytes, (name, samples)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_guarded_is_the_plane_and_its_guard_all_sentinel(family):
    table = FAMILIES[family].table
    for samples in SAMPLES:
        for guard in (64, 1, 0):
            plain = Q.guarded(table, tuple(table), samples, guard_elems=guard)
            aligned = Q.guarded(table, tuple(table), samples, guard_elems=guard, align=8)
            assert set(plain) == set(aligned) == set(table)
            for name, (dtype, comps) in table.items():
                exact = Q.plane_bytes(table, name, samples) + guard * np.dtype(dtype).itemsize
                for buf, size in ((plain[name], exact), (aligned[name], (exact + 7) // 8 * 8)):
                    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.nbytes == size, (name, samples, guard)
                    assert buf.tobytes() == bytes([0xA5]) * size, (name, samples, guard)
                assert aligned[name].ctypes.data % 8 == 0, (name, samples)
    assert len(Q.guarded(table, ("node",), 5)) == 1 and Q.SENTINEL == 0xA5


def test_guard_units_are_stated():
    assert Q.guard_size(8, guard_elems=64) == 512 and Q.guard_size(8, guard_bytes=64) == 64
    for kw in ({}, dict(guard_elems=1, guard_bytes=1)):
        with pytest.raises(AssertionError):
            Q.guard_size(4, **kw)
    frame, mask = Q.frame_and_mask(35, guard_elems=64)
    assert (frame.nbytes, mask.nbytes) == (35 * 12 + 256, 35 + 64) and Q.untouched((frame, mask))
    frame, mask = Q.frame_and_mask(35, guard_bytes=64)
    assert (frame.nbytes, mask.nbytes) == (35 * 12 + 64, 35 + 64) and Q.untouched((frame, mask))


@pytest.mark.parametrize("align", [1, 8])
def test_untouched_sees_every_single_byte(align):
    samples = 65
    bufs = Q.guarded(OCCLUSION_PLANES, tuple(OCCLUSION_PLANES), samples, align=align)
    assert Q.untouched(bufs) and Q.untouched(bufs.values()) and Q.untouched(list(bufs.values())) and Q.untouched(b for b in bufs.values())
    assert Q.untouched({}) and Q.untouched(())
    for name, buf in bufs.items():
        nb = Q.plane_bytes(OCCLUSION_PLANES, name, samples)
        payload, guard = Q.payload_and_guard(buf, nb)
        assert payload.nbytes == nb and payload.nbytes + guard.nbytes == buf.nbytes and guard.nbytes >= 64
        assert payload.ctypes.data == buf.ctypes.data and guard.ctypes.data == buf.ctypes.data + nb          # views, not copies
        for at in (0, nb // 2, nb - 1, nb, nb + guard.nbytes // 2, buf.nbytes - 1):       # payload and guard, first and last
            for value in (0xA4, 0x00):
                buf[at] = value
                assert not Q.untouched(bufs) and not Q.untouched(list(bufs.values())) and not Q.untouched((buf,)), (name, at)
                assert Q.untouched({k: v for k, v in bufs.items() if k != name})
                buf[at] = Q.SENTINEL
            assert Q.untouched(bufs)


def test_check_filled_sees_the_payload_and_the_guard():
    n = 63
    want = {name: (np.arange(n * comps) % 7).astype(dtype).reshape((n,) if comps == 1 else (n, comps)) for name, (dtype, comps) in GATHER_PLANES.items()}
    bufs = Q.guarded(GATHER_PLANES, tuple(GATHER_PLANES), n, align=8)
    for name in GATHER_PLANES:
        bufs[name][:want[name].nbytes] = want[name].view(np.uint8).reshape(-1)
    Q.check_filled(GATHER_PLANES, bufs, want, n, "filled")
    Q.check_filled(GATHER_PLANES, bufs, want, n, "filled", ("hits",))
    nb = Q.plane_bytes(GATHER_PLANES, "hits", n)
    for at in (0, nb - 1, nb, bufs["hits"].nbytes - 1):
        bufs["hits"][at] ^= 1
        with pytest.raises(AssertionError):
            Q.check_filled(GATHER_PLANES, bufs, want, n, "one byte off")
        Q.check_filled(GATHER_PLANES, bufs, want, n, "the other planes", ("node", "indirect", "bounce"))
        bufs["hits"][at] ^= 1
    Q.check_filled(GATHER_PLANES, bufs, want, n, "restored")


def test_same_and_same_planes_compare_bits():
    f32 = lambda *words: np.array(words, dtype=np.uint32).view(np.float32)
    f64 = lambda *words: np.array(words, dtype=np.uint64).view(np.float64)
    pairs = [(f32(0x00000000), f32(0x80000000)),                           # +0 and -0
             (f64(0), f64(1 << 63)),
             (f32(0x7FC00000), f32(0x7FC00001)),                           # two NaNs, different payloads
             (f32(0x7FC00000), f32(0xFFC00000)),
             (f64(0x7FF8000000000000), f64(0x7FF8000000000001))]
    for a, b in pairs:
        with np.errstate(invalid="ignore"):
            assert (a == b).all() or (np.isnan(a) & np.isnan(b)).all()      # what a value compare would let through
        assert not Q.same(a, b) and Q.same(a, a.copy()) and Q.same(b, b.copy())
        Q.same_planes({"p": a}, {"p": a.copy()}, "equal bits", ("p",))
        with pytest.raises(AssertionError):
            Q.same_planes({"p": a}, {"p": b}, "different bits", ("p",))
        Q.same_planes({"p": a, "q": a}, {"p": a.copy(), "q": b}, "the plane that is not named", ("p",))
    nan = f32(0x7FC00000, 0x3F800000)
    assert Q.same(nan, nan.copy()) and not (nan == nan.copy()).all()
    # shape and type are part of the answer, whatever the bytes
    zeros = np.zeros(4, dtype=np.float32)
    assert not Q.same(zeros, zeros.reshape(2, 2)) and not Q.same(zeros, zeros.view(np.int32)) and Q.same(zeros[::2], np.zeros(2, dtype=np.float32))
    with pytest.raises(AssertionError):
        Q.same_planes({"p": zeros}, {"p": zeros.view(np.int32)}, "types", ("p",))
    with pytest.raises(AssertionError):
        Q.same_planes({"p": zeros}, {"p": zeros[:2]}, "sizes", ("p",))
    assert Q.float_bits(zeros).dtype == np.uint32 and Q.float_bits(zeros.view(np.int32)).dtype == np.uint8


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_struct_of_leaves_the_planes_not_named_null(family):
    fam = FAMILIES[family]
    names = tuple(fam.table)
    bufs = Q.guarded(fam.table, names, 9)
    for subset in [()] + [(n,) for n in names] + [names[:2], names]:
        pl = Q.struct_of(fam.struct, {k: bufs[k] for k in subset})
        assert isinstance(pl, fam.struct)
        for name in names:
            got = C.cast(getattr(pl, name), C.c_void_p).value
            assert got == (bufs[name].ctypes.data if name in subset else None), (subset, name)
    pl = Q.struct_of(fam.struct, {names[0]: 0x10})                          # a bare address is taken as it is
    assert C.cast(getattr(pl, names[0]), C.c_void_p).value == 0x10


def test_with_fields_copies():
    opts = Q.gather_options(samples=3, seed=5)
    other = Q.with_fields(opts, samples=65, reserved=2)
    assert (opts.samples, opts.seed, opts.reserved) == (3, 5, 0) and (other.samples, other.seed, other.reserved) == (65, 5, 2)
    occ = Q.occlusion_options(radius=2.5)
    assert type(other) is type(opts) and (occ.radius, occ.reserved) == (2.5, 0) and occ.samples == Q.occlusion_options().samples
