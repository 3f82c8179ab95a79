"""The Python layer's plane families (chess2rt_amd/api.py: _PlaneFamily), each against its ctypes struct and the sample
sizes the library stages by (c2rt_api.cpp, Family<S>::bytes).  No library handle, no GPU."""
import ctypes as C

import numpy as np
import pytest

from chess2rt_amd import _abi, api

# family, its public table, its struct, bytes per sample (the figures next to Family<S>::bytes), the noun of its ValueError
FAMILIES = [
    (api._HIT, api.HIT_PLANES, _abi.HitPlanes, 92, "hit"),
    (api._SHADE, api.SHADE_PLANES, _abi.ShadePlanes, 56, "shading"),
    (api._OCCLUSION, api.OCCLUSION_PLANES, _abi.OcclusionPlanes, 40, "occlusion"),
    (api._GATHER, api.GATHER_PLANES, _abi.GatherPlanes, 36, "gather"),
]
IDS = [f[4] for f in FAMILIES]


@pytest.mark.parametrize("fam,table,struct,sample_bytes,noun", FAMILIES, ids=IDS)
def test_table_is_the_struct(fam, table, struct, sample_bytes, noun):
    assert fam.table is table and fam.struct is struct
    assert list(table) == [f[0] for f in struct._fields_]
    assert C.sizeof(struct) == len(table) * C.sizeof(C.c_void_p)      # nothing but pointers
    assert sum(np.dtype(d).itemsize * c for d, c in table.values()) == sample_bytes


@pytest.mark.parametrize("fam,table,struct,sample_bytes,noun", FAMILIES, ids=IDS)
@pytest.mark.parametrize("shape", [(5,), (3, 4)])
def test_new_allocates_the_planes_named_and_no_other(fam, table, struct, sample_bytes, noun, shape):
    names = list(table)
    for asked in (names, names[1::2], names[:1], []):
        pl, out = fam.new(iter(asked), shape)
        assert isinstance(pl, struct) and list(out) == asked
        for n in names:
            if n not in asked:
                assert getattr(pl, n) is None, n
                continue
            dtype, comps = table[n]
            assert out[n].dtype == np.dtype(dtype) and out[n].flags["C_CONTIGUOUS"], n
            assert out[n].shape == (shape if comps == 1 else shape + (comps,)), n
            assert getattr(pl, n) == out[n].ctypes.data, n


@pytest.mark.parametrize("fam,table,struct,sample_bytes,noun", FAMILIES, ids=IDS)
def test_device_keeps_pointers_and_maps_zero_and_none_to_null(fam, table, struct, sample_bytes, noun):
    names = list(table)
    ptrs = {n: 256 * (k + 1) for k, n in enumerate(names)}
    pl = fam.device(ptrs)
    assert isinstance(pl, struct) and [getattr(pl, n) for n in names] == list(ptrs.values())
    pl = fam.device({names[0]: 0, names[1]: None, names[-1]: 4096})
    assert getattr(pl, names[0]) is None and getattr(pl, names[1]) is None and getattr(pl, names[-1]) == 4096
    assert all(getattr(pl, n) is None for n in names[2:-1])
    assert all(getattr(fam.device({}), n) is None for n in names)


@pytest.mark.parametrize("fam,table,struct,sample_bytes,noun", FAMILIES, ids=IDS)
def test_unknown_name_is_refused_in_the_words_of_the_family(fam, table, struct, sample_bytes, noun):
    want = "unknown %s plane 'depth_of' (one of %s)" % (noun, ", ".join(table))
    with pytest.raises(ValueError) as e:
        fam.new((next(iter(table)), "depth_of"), (2, 2))
    assert str(e.value) == want
    with pytest.raises(ValueError) as e:
        fam.device({"depth_of": 64})
    assert str(e.value) == want


def test_the_messages_as_they_were_written_out():
    """the four texts, literally, as the four copies of the check spelled them"""
    for fam, text in ((api._HIT, "unknown hit plane 'x' (one of node, leaf, dist, uv, p, normal, rgb)"),
                      (api._SHADE, "unknown shading plane 'x' (one of node, albedo, light, specular, visible, rgb)"),
                      (api._OCCLUSION, "unknown occlusion plane 'x' (one of node, open, ao, bent)"),
                      (api._GATHER, "unknown gather plane 'x' (one of node, hits, indirect, bounce)")):
        with pytest.raises(ValueError) as e:
            fam.device({"x": 1})
        assert str(e.value) == text


def test_rays_array():
    rays = api._rays_array([[0, 0, 0, 0, 0, 1]] * 3)
    assert rays.shape == (3, 6) and rays.dtype == np.float64 and rays.flags["C_CONTIGUOUS"]
    assert api._rays_array(np.zeros((0, 6))).shape == (0, 6)
    for bad, what, shape in ((np.zeros((4, 5)), "rays", "(4, 5)"), (np.zeros(6), "segments", "(6,)"), (np.zeros((2, 6, 1)), "rays", "(2, 6, 1)")):
        with pytest.raises(ValueError) as e:
            api._rays_array(bad, what)
        assert str(e.value) == "%s: expected shape (n, 6), got %s" % (what, shape)
