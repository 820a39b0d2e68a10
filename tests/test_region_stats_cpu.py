"""tests/region_stats_ref.py against the definitions written out as loops, against the statistics grow_ref and label_ref already
give, and on the cases whose faces can be counted by hand; scene.region_measures on a hand-computed record.  No GPU."""
import math

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import grow_ref as gr
from tests import label_ref as lr
from tests import region_stats_ref as rs


def test_dtype_is_the_abi_record():
    assert rs.DTYPE == ffi.REGION_STATS_DTYPE and rs.DTYPE.itemsize == 104
    assert [rs.DTYPE.fields[k][1] for k in rs.DTYPE.names] == [getattr(ffi.RegionStats, k).offset for k in rs.DTYPE.names]


@pytest.mark.parametrize("dims", ((1, 1, 1), (7, 6, 5), (5, 1, 3), (1, 4, 1), (2, 2, 2)))
def test_ref_equals_the_triple_loop(dims):
    X, Y, Z = dims
    rng = np.random.default_rng(X * 100 + Y * 10 + Z)
    vol = rng.integers(-32768, 32768, (Z, Y, X)).astype(np.int16)
    for density in (0.0, 0.1, 0.5, 1.0):
        region = rng.random((Z, Y, X)) < density
        assert rs.record(vol, region).tobytes() == rs.record_by_loops(vol, region).tobytes(), (dims, density)
    labels = rng.integers(0, 5, (Z, Y, X)).astype(np.uint32)
    table = rs.label_records(vol, labels, 3)
    for k in range(3):
        assert table[k].tobytes() == rs.record_by_loops(vol, labels == k + 1).tobytes()


def test_ref_equals_grow_refs_statistics():
    vol = scene.phantom(24)
    z = 12
    y, x = np.argwhere(gr.admissible(vol, 500, 1200)[z])[0]
    region, _ = gr.grow(vol, [(int(x), int(y), z)], 500, 1200)
    assert region.sum() > 50
    want = gr.stats(vol, region)
    got = rs.as_dict(rs.record(vol, region))
    assert {k: got[k] for k in want} == want
    assert {k: rs.as_dict(rs.record(vol, np.zeros_like(region)))[k] for k in want} == gr.stats(vol, np.zeros_like(region))


def test_ref_equals_label_refs_table():
    vol = gr.random_volume((33, 12, 9), 3)
    ranks, table, info = lr.label(vol, -1000, -280)
    n = info["n_components"]
    assert n > 20
    got = rs.label_records(vol, ranks, n + 2)
    assert np.array_equal(got["count"][:n], table["count"]) and (got["count"][n:] == 0).all()
    assert np.array_equal(got["bbox_lo"][:n], table["bbox_lo"]) and np.array_equal(got["bbox_hi"][:n], table["bbox_hi"])
    assert int(got["count"].sum()) == info["n_voxels"]
    for k in (0, 1, n // 2, n - 1, n):  # the table at once against the record of one region at a time
        assert got[k].tobytes() == rs.record(vol, ranks == k + 1).tobytes(), k


def test_faces_by_hand():
    vol = np.zeros((4, 5, 6), np.int16)
    one = np.zeros(vol.shape, bool)
    one[1, 2, 3] = True  # an inner voxel: two faces per axis, none on the border
    r = rs.as_dict(rs.record(vol, one))
    assert (r["faces"], r["border_faces"], r["sum_pos"], r["bbox_lo"], r["bbox_hi"]) == ((2, 2, 2), (0, 0, 0), (3, 2, 1), (3, 2, 1), (4, 3, 2))
    corner = np.zeros(vol.shape, bool)
    corner[0, 0, 0] = True
    r = rs.as_dict(rs.record(vol, corner))
    assert (r["faces"], r["border_faces"]) == ((1, 1, 1), (1, 1, 1))
    full = np.ones(vol.shape, bool)  # no face inside the volume, every face of the box on the border
    r = rs.as_dict(rs.record(vol, full))
    assert (r["faces"], r["border_faces"]) == ((0, 0, 0), (2 * 5 * 4, 2 * 6 * 4, 2 * 6 * 5))
    slab = np.zeros((1, 5, 6), np.int16)  # dim_z == 1: every voxel counts twice along z
    part = np.zeros(slab.shape, bool)
    part[0, 1:3, 2:5] = True
    r = rs.as_dict(rs.record(slab, part))
    assert (r["count"], r["faces"], r["border_faces"]) == (6, (4, 6, 0), (0, 0, 12))


def test_histogram_identity():
    rng = np.random.default_rng(9)
    vol = rng.integers(-32768, 32768, (6, 7, 9)).astype(np.int16)
    region = rng.random(vol.shape) < 0.6
    count = int(region.sum())
    for lo, width, n in ((-32768, 1, 65536), (-32768, 4096, 16), (-100, 7, 30), (32767, 1, 1), (0, 1 << 30, 2), (-32768, 65536, 1)):
        hist, below, above = rs.histogram(vol, region, lo, width, n)
        assert hist.dtype == np.uint64 and len(hist) == n and int(hist.sum()) + below + above == count
        v = vol[region].astype(np.int64)
        assert below == int((v < lo).sum()) and above == int((v >= lo + n * width).sum())
        for b in (0, n // 2, n - 1):
            assert int(hist[b]) == int(((v >= lo + b * width) & (v < lo + (b + 1) * width)).sum())


def test_region_measures_by_hand():
    rec = {"count": 4, "sum": 20, "sum_sq": 120, "vmin": 2, "vmax": 8, "sum_pos": (6, 10, 2), "bbox_lo": (1, 2, 0), "bbox_hi": (3, 4, 1),
           "faces": (4, 4, 0), "border_faces": (0, 0, 8)}
    m = scene.region_measures(rec, (0.5, 0.5, 2.0))
    assert m["count"] == 4 and m["volume"] == 4 * 0.5 * 0.5 * 2.0
    assert m["mean"] == 5.0 and m["std"] == math.sqrt(120 / 4 - 25.0)
    assert m["centroid"] == (2.0, 3.0, 1.0)
    assert m["area"] == 4 * 1.0 + 4 * 1.0 and m["area_with_border"] == 8.0 + 8 * 0.25
    row = np.zeros((), rs.DTYPE)
    for k, v in rec.items():
        row[k] = v
    assert scene.region_measures(row, (0.5, 0.5, 2.0)) == m
    empty = scene.region_measures(np.zeros((), rs.DTYPE))
    assert (empty["count"], empty["volume"], empty["mean"], empty["std"], empty["centroid"], empty["area"]) == (0, 0.0, None, None, None, 0.0)
