"""Device side of the CsgDiff void-tile checks (tests/test_gpu_csg_void.py): reads back the mask pre-pass's table
through the diagnostics hook c2rt_debug_tile_masks (chess2rt_amd/libc2rt_diag.so: load with C2RT_LIB_VARIANT=diag)
and compares the tiles the device dropped a node from with the host classifier's claims
(scripts/csg_void_tiles.py over tests/libcsg_void_check.so)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import csg_void_tiles as cv  # noqa: E402


class VoidNodeC(C.Structure):  # csg_void.h: VoidNode
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3), ("c", C.c_double * 3), ("r2", C.c_double),
                ("node", C.c_uint32), ("flags", C.c_uint32)]


class VoidCullC(C.Structure):  # csg_void.h: VoidCull
    _fields_ = [("n", C.c_uint32), ("pad", C.c_uint32), ("light0", C.c_double * 3), ("v", VoidNodeC * cv.MAX_VOID_NODES)]


def _hook():
    from chess2rt_amd import _abi

    lib = _abi.load_library()
    fn = lib.c2rt_debug_tile_masks  # AttributeError: not the diagnostics build
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(_abi.CameraFrame), C.POINTER(_abi.RenderOpts), C.c_uint32, C.c_void_p, C.c_size_t,
                   C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t]
    return lib, fn


def tile_mask_slot(trow, tcol, cols, mask_rows):
    """tile_mask_slot (c2rt_tile_mask.inc), from its documented formula: eight row classes (tile rows r, r + 8, ...),
    each ceil(ceil(mask_rows / 8) / 8) tile rows of `cols` entries"""
    per_class = ((mask_rows + 7) // 8 + 7) // 8
    return ((trow & 7) * per_class + (trow >> 3)) * cols + tcol


def unslot(raw, cols, tile_rows, mask_rows):
    """the table (entries, 4) in slot layout -> (tile_rows, cols, 4) by tile row / column"""
    tr, tc = np.meshgrid(np.arange(tile_rows), np.arange(cols), indexing="ij")
    return raw[tile_mask_slot(tr, tc, cols, mask_rows)]


def read_tile_masks(ctx, cam, opts, flags_mask):
    """(table (tile_rows, cols, 4) uint32, info dict, VoidCullC) of the pre-pass for this frame with every
    VoidNode::flags ANDed with flags_mask; None if the frame has no table."""
    from chess2rt_amd import _abi

    lib, fn = _hook()
    rows = ctx.localRows(opts)
    cols_max = ((opts.width + 7) // 8 + 63) // 64 * 64 + 64
    words = ((rows + 7) // 8 + 8) * cols_max * 4 + 64
    buf = np.zeros(words, dtype=np.uint32)
    info = (C.c_uint32 * 6)()
    vc = VoidCullC()
    st = fn(ctx.handle, C.byref(cam), C.byref(opts), flags_mask, buf.ctypes.data_as(C.c_void_p), words, info,
            C.byref(vc), C.sizeof(vc))
    if st == _abi.ERR_UNSUPPORTED:
        return None
    if st != _abi.OK:
        raise RuntimeError("c2rt_debug_tile_masks: %s" % lib.c2rt_last_error(ctx.handle).decode())
    d = dict(zip(("cols", "tile_rows", "mask_row0", "mask_rows", "per_class", "entries"), list(info)))
    assert d["tile_rows"] == (d["mask_rows"] + 7) // 8 and d["per_class"] == (d["tile_rows"] + 7) // 8, d
    assert d["entries"] == 8 * d["per_class"] * d["cols"], d
    raw = buf[: 4 * d["entries"]].reshape(-1, 4)
    return unslot(raw, d["cols"], d["tile_rows"], d["mask_rows"]), d, vc


def _bits(a, n):
    return ((a >> np.uint32(n)) & np.uint32(1)).astype(bool)


def compare(ctx, desc, cam, opts, debug_cull=0):
    """Reads the table at void_flags_mask 0, 1 and 3 and asserts (AssertionError with the first differences):
    the VoidCull equals frame_void_nodes bit for bit; per candidate, the tiles where the primary test dropped the
    node (word 0, mask 0 -> 1) are exactly the host's bit-0 claims among the tiles that keep it at mask 0, and
    the tiles where the shadow test dropped it (word 1, mask 1 -> 3) exactly the host's bit-1 claims among the
    primary-ground tiles that keep it at mask 1; nothing else moves but in the direction the void test explains.
    Returns {node: (primary drops, shadow drops)}; None for a frame without a table."""
    t0, t1, t3 = (read_tile_masks(ctx, cam, opts, m) for m in (0, 1, 3))
    if t0 is None:
        assert t1 is None and t3 is None
        return None
    (m0, info, vc0), (m1, info1, vc1), (m3, info3, vc3) = t0, t1, t3
    assert info == info1 == info3
    # 1. the VoidCull: the Python restatement of the library's candidates and margin, bit for bit
    want = cv.frame_void_nodes(desc, cam, debug_cull)
    D = cv._fields(desc)
    assert vc3.n == len(want), (vc3.n, want)
    assert [vc3.light0[i] for i in range(3)] == ([D.light_pos[i] for i in range(3)] if D.n_lights else [0.0] * 3)
    for mask, vc in ((0, vc0), (1, vc1), (3, vc3)):
        assert vc.n == len(want)
        for j, w in enumerate(want):
            v = vc.v[j]
            got = dict(node=v.node, lo=list(v.lo), hi=list(v.hi), c=list(v.c), r2=v.r2, flags=v.flags)
            exp = dict(w, flags=w["flags"] & mask)
            assert got == exp, "VoidCull entry %d at mask %d: device %r, host %r" % (j, mask, got, exp)
    # 2..4. the table
    bounds = [cv.tile_bounds(r, c, info["mask_row0"], info["mask_rows"], opts.strip_height or 1,
                             opts.strip_rank if opts.strip_world > 1 else 0, max(opts.strip_world, 1))
              for r in range(info["tile_rows"]) for c in range(info["cols"])]
    shape = (info["tile_rows"], info["cols"])
    assert not np.any(m0[..., 3]) and not np.any(m1[..., 3]) and not np.any(m3[..., 3])
    cand_mask = np.uint32(sum(1 << w["node"] for w in want if w["node"] < 32))
    # word 0: only candidate bits change, only 1 -> 0, and not between masks 1 and 3
    assert np.array_equal(m0[..., 0] & ~cand_mask, m1[..., 0] & ~cand_mask), "word 0: a non-candidate bit moved"
    assert not np.any(m1[..., 0] & ~m0[..., 0]), "word 0: a bit appeared under the void test"
    assert np.array_equal(m1[..., 0], m3[..., 0]) and np.array_equal(m1[..., 2] & 1, m3[..., 2] & 1)
    # word 2: ground bits only appear; word 1 unchanged where the tile did not become primary-ground, else only loses bits
    assert not np.any(m0[..., 2] & ~m1[..., 2]) and not np.any(m1[..., 2] & ~m3[..., 2]), "word 2: a ground bit vanished"
    same_ground = (m0[..., 2] & 1) == (m1[..., 2] & 1)
    assert np.array_equal(m0[..., 1][same_ground], m1[..., 1][same_ground]), "word 1 moved without a ground change"
    assert not np.any(m1[..., 1] & ~m0[..., 1]) and not np.any(m3[..., 1] & ~m1[..., 1]), "word 1: a bit appeared"
    assert np.array_equal(m1[..., 1] & ~cand_mask, m3[..., 1] & ~cand_mask), "word 1: a non-candidate bit moved"
    counts = {}
    cands = {c.node: c for c in cv.void_candidates(desc)}
    for w in want:
        n = w["node"]
        cand = cands[n]._replace(flags=w["flags"])
        host = cv.classify_tiles(desc, cam, bounds, cand).reshape(shape)
        prim = _bits(m0[..., 0], n) & ~_bits(m1[..., 0], n)
        claim = ((host & 1) != 0) & _bits(m0[..., 0], n)
        shad = _bits(m1[..., 1], n) & ~_bits(m3[..., 1], n)
        sclaim = ((host & 2) != 0) & ((m3[..., 2] & 1) != 0) & _bits(m1[..., 1], n)
        for what, got, exp in (("primary", prim, claim), ("shadow", shad, sclaim)):
            if not np.array_equal(got, exp):
                diff = [(int(r), int(c), bounds[int(r) * shape[1] + int(c)]) for r, c in zip(*np.nonzero(got != exp))]
                raise AssertionError("node %d: %s drops differ from the host's claims (device %d, host %d) at (trow, tcol, "
                                     "(tx0, ty0, ty1)) %s" % (n, what, int(got.sum()), int(exp.sum()), diff[:8]))
        counts[n] = (int(prim.sum()), int(shad.sum()))
    return counts
