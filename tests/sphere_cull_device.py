"""Device side of the sphere-silhouette checks (tests/test_gpu_sphere_cull.py): switches the sphere test of the mask
pre-pass through the diagnostics hook c2rt_debug_sphere_cull (chess2rt_amd/libc2rt_diag.so: C2RT_LIB_VARIANT=diag),
reads the table back through c2rt_debug_tile_masks (tests/csg_void_device.py) and compares the tiles the device
dropped a Sphere node from with the host classifier's claims (scripts/sphere_cull_tiles.py)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import csg_void_device as vdev  # noqa: E402
import csg_void_tiles as cv  # noqa: E402
import sphere_cull_tiles as sc  # noqa: E402


class SphereNodeC(C.Structure):  # csg_void.h: SphereNode
    _fields_ = [("c", C.c_double * 3), ("rp", C.c_double), ("node", C.c_uint32), ("flags", C.c_uint32)]


class SphereCullC(C.Structure):  # csg_void.h: SphereCull
    _fields_ = [("n", C.c_uint32), ("pad", C.c_uint32), ("reach", C.c_double), ("s", SphereNodeC * sc.MAX_SPHERE_NODES)]


def set_sphere_mask(ctx, mask, cam=None, opts=None):
    """every SphereNode::flags of this context's pre-passes is ANDed with `mask` from now on; with cam and opts:
    -> the SphereCull such a pre-pass is given"""
    from chess2rt_amd import _abi

    lib = _abi.load_library()
    fn = lib.c2rt_debug_sphere_cull  # AttributeError: not the diagnostics build
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_abi.CameraFrame), C.POINTER(_abi.RenderOpts), C.c_void_p, C.c_size_t]
    out = SphereCullC() if cam is not None else None
    st = fn(ctx.handle, mask, C.byref(cam) if cam is not None else None, C.byref(opts) if opts is not None else None,
            C.byref(out) if out is not None else None, C.sizeof(SphereCullC))
    if st != _abi.OK:
        raise RuntimeError("c2rt_debug_sphere_cull: %s" % lib.c2rt_last_error(ctx.handle).decode())
    return out


def classes(m, n_nodes):
    """(ground-only, primary-ground with shadow casters, objects in view, nothing) tile counts of a table"""
    w2 = m[..., 2]
    sky = (m[..., 0] & np.uint32((1 << min(n_nodes, 32)) - 1 if n_nodes < 32 else 0xFFFFFFFF)) == 0
    return (int(((w2 & 3) == 3).sum()), int(((w2 & 3) == 1).sum()), int((((w2 & 1) == 0) & ~sky).sum()), int(sky.sum()))


def compare(ctx, desc, cam, opts, debug_cull=0):
    """Reads the table with the sphere switch at 0, 1 and 3 (void test as shipped) and asserts: the SphereCull
    equals frame_sphere_cull bit for bit; per ball, the tiles where the primary test dropped the node (word 0,
    switch 0 -> 1) are exactly the host's bit-0 claims among the tiles that keep it at 0, and the tiles where the
    shadow test dropped it (word 1, switch 1 -> 3) exactly the host's bit-1 claims among the primary-ground tiles
    that keep it at 1; nothing else moves but in the direction the test explains.  Leaves the switch at 3.
    Returns dict(drops={node: (primary, shadow)}, classes_off=..., classes_on=...); None without a table."""
    tabs = []
    for mask in (0, 1, 3):
        got = set_sphere_mask(ctx, mask, cam, opts)
        want = sc.frame_sphere_cull(desc, cam, debug_cull, mask)
        if want is None:
            want = (0.0, [])
        reach, entries = want
        assert got.n == len(entries) and (got.reach == reach or not entries), (mask, got.n, got.reach, want)
        for j, e in enumerate(entries):
            s = got.s[j]
            assert dict(node=s.node, c=list(s.c), rp=s.rp, flags=s.flags) == e, (mask, j, e)
        tabs.append(vdev.read_tile_masks(ctx, cam, opts, 3))
    if tabs[0] is None:
        assert tabs[1] is None and tabs[2] is None
        return None
    (m0, info, _), (m1, info1, _), (m3, info3, _) = tabs
    assert info == info1 == info3
    reach, entries = sc.frame_sphere_cull(desc, cam, debug_cull, 3) or (0.0, [])
    bounds = [cv.tile_bounds(r, c, info["mask_row0"], info["mask_rows"], opts.strip_height or 1,
                             opts.strip_rank if opts.strip_world > 1 else 0, max(opts.strip_world, 1))
              for r in range(info["tile_rows"]) for c in range(info["cols"])]
    shape = (info["tile_rows"], info["cols"])
    ball_mask = np.uint32(sum(1 << e["node"] for e in entries))
    for m in (m0, m1, m3):
        assert not np.any(m[..., 3])
    assert np.array_equal(m0[..., 0] & ~ball_mask, m1[..., 0] & ~ball_mask), "word 0: another node's bit moved"
    assert not np.any(m1[..., 0] & ~m0[..., 0]), "word 0: a bit appeared under the sphere test"
    assert np.array_equal(m1[..., 0], m3[..., 0]) and np.array_equal(m1[..., 2] & 1, m3[..., 2] & 1)
    assert not np.any(m0[..., 2] & ~m1[..., 2]) and not np.any(m1[..., 2] & ~m3[..., 2]), "word 2: a ground bit vanished"
    same_ground = (m0[..., 2] & 1) == (m1[..., 2] & 1)
    assert np.array_equal(m0[..., 1][same_ground], m1[..., 1][same_ground]), "word 1 moved without a ground change"
    assert not np.any(m1[..., 1] & ~m0[..., 1]) and not np.any(m3[..., 1] & ~m1[..., 1]), "word 1: a bit appeared"
    assert np.array_equal(m1[..., 1] & ~ball_mask, m3[..., 1] & ~ball_mask), "word 1: another node's bit moved"
    drops = {}
    for e in entries:
        n = e["node"]
        host = sc.classify_tiles(desc, cam, bounds, e, reach).reshape(shape)
        prim = vdev._bits(m0[..., 0], n) & ~vdev._bits(m1[..., 0], n)
        claim = ((host & 1) != 0) & vdev._bits(m0[..., 0], n)
        shad = vdev._bits(m1[..., 1], n) & ~vdev._bits(m3[..., 1], n)
        sclaim = ((host & 2) != 0) & ((m3[..., 2] & 1) != 0) & vdev._bits(m1[..., 1], n)
        for what, got, exp in (("primary", prim, claim), ("shadow", shad, sclaim)):
            if not np.array_equal(got, exp):
                diff = [(int(r), int(c), bounds[int(r) * shape[1] + int(c)]) for r, c in zip(*np.nonzero(got != exp))]
                raise AssertionError("node %d: %s drops differ from the host's claims (device %d, host %d) at (trow, tcol, "
                                     "(tx0, ty0, ty1)) %s" % (n, what, int(got.sum()), int(exp.sum()), diff[:8]))
        drops[n] = (int(prim.sum()), int(shad.sum()), int(vdev._bits(m0[..., 0], n).sum()))
    nn = cv._fields(desc).n_nodes
    return dict(drops=drops, classes_off=classes(m0, nn), classes_on=classes(m3, nn))
