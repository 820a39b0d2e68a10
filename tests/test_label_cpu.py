"""The numpy restatement of clwh_segment_label (tests/label_ref.py) against grow_ref's region growing, the ranking rule on a
hand-made tie, the fixtures' counts the GPU test relies on, and the two entry points' behaviour without a device."""
import ctypes as C

import numpy as np

from cl_volume_renderer_amd import ffi, scene
from tests import grow_ref as gr
from tests import label_ref as lr

INVALID_VALUE = 1


def test_components_equal_growth_from_their_first_voxels():
    for connectivity in (6, 26):
        vol = gr.random_volume((33, 40, 35), 7)
        lo, hi = gr.WINDOWS[connectivity]
        ranks, table, res = lr.label(vol, lo, hi, connectivity)
        assert res["n_components"] == len(table) > 100 and res["n_voxels"] == int(table["count"].sum()) == int((ranks > 0).sum())
        assert np.array_equal(ranks > 0, gr.admissible(vol, lo, hi))
        for rank in (1, 2, 3, len(table) // 2, len(table)):
            rec = table[rank - 1]
            region, _ = gr.grow(vol, [tuple(rec["first"])], lo, hi, connectivity)
            assert np.array_equal(region, ranks == rank), (connectivity, rank)
            stats = gr.stats(vol, region)
            assert stats["count"] == rec["count"] and stats["bbox_lo"] == tuple(rec["bbox_lo"]) and stats["bbox_hi"] == tuple(rec["bbox_hi"])
            z, y, x = np.argwhere(region)[0]
            assert (x, y, z) == tuple(rec["first"])  # the member with the smallest flat index
        assert np.all(np.diff(table["count"].astype(np.int64)) <= 0)


def test_ranking_on_a_hand_made_tie():
    adm = np.zeros((2, 3, 9), bool)
    adm[0, 0, 0:2] = True   # 2 voxels, first = 0
    adm[0, 0, 4:7] = True   # 3 voxels, first = 4
    adm[0, 2, 0:2] = True   # 2 voxels, first = 18
    adm[1, 1, 3:6] = True   # 3 voxels, first = 39
    adm[1, 2, 8] = True     # 1 voxel
    ranks, table, res = lr.label_admissible(adm, 6)
    assert res == {"n_components": 5, "n_voxels": 11}
    assert table["count"].tolist() == [3, 3, 2, 2, 1]
    assert table["first"].tolist() == [[4, 0, 0], [3, 1, 1], [0, 0, 0], [0, 2, 0], [8, 2, 1]]
    assert ranks[0, 0].tolist() == [3, 3, 0, 0, 1, 1, 1, 0, 0] and ranks[1, 1, 4] == 2 and ranks[0, 2, 1] == 4 and ranks[1, 2, 8] == 5
    assert table["bbox_lo"][1].tolist() == [3, 1, 1] and table["bbox_hi"][1].tolist() == [6, 2, 2]
    _, short, res = lr.label_admissible(adm, 6, capacity=2)
    assert len(short) == 2 and res["n_components"] == 5
    assert np.array_equal(lr.selection(ranks, 3, 4), (ranks == 3) | (ranks == 4))
    assert lr.packed_selection(ranks, 1, 5).tobytes() == scene.mask_pack(adm).tobytes()


def test_fixtures_are_what_the_gpu_test_claims():
    for connectivity in (6, 26):
        _, table, res = lr.label(lr.two_serpentines(), 100, 100, connectivity)
        assert table["count"].tolist() == [2739, 2739] and table["first"].tolist() == [[0, 0, 1], [0, 1, 3]]
        _, table, res = lr.label(lr.comb(), 100, 100, connectivity)
        assert table["count"].tolist() == [19890] and table["first"].tolist() == [[0, 0, 0]]
        assert lr.label(lr.comb(False), 100, 100, connectivity)[2]["n_components"] == 9
        for a, b in (((63, 15, 15), (64, 16, 16)), ((63, 15, 5), (64, 16, 5))):
            assert lr.label(lr.contact(a, b), 100, 100, connectivity)[2]["n_components"] == (2 if connectivity == 6 else 1)
        _, table, res = lr.label(scene.phantom(96), 500, 1200, connectivity)
        assert table["count"].tolist() == [30548, 30548]
        _, table, res = lr.label(scene.phantom(48), 500, 1200, connectivity)
        assert table["count"].tolist() == [3940, 3940]
    ranks, table, res = lr.label(lr.checkerboard(), 100, 100, 6)
    assert res["n_components"] == 11970 and np.array_equal(ranks[ranks > 0], np.arange(1, 11971))  # raster order
    assert lr.label(lr.checkerboard(), 100, 100, 26)[2]["n_components"] == 1
    vol = gr.random_volume((70, 40, 36), 7)
    _, table, res = lr.label(vol, *gr.WINDOWS[6])
    sizes, n = np.unique(table["count"], return_counts=True)
    assert res["n_components"] == 3858 and int(n[n > 1].sum()) == 3838  # the tie rule decides most ranks


def test_binding_structs_match_the_header():
    assert C.sizeof(ffi.LabelComponent) == 48 and ffi.LABEL_COMPONENT_DTYPE.itemsize == 48
    assert [ffi.LABEL_COMPONENT_DTYPE.fields[k][1] for k in ("count", "first", "bbox_lo", "bbox_hi", "reserved")] == [0, 8, 20, 32, 44]
    assert C.sizeof(ffi.LabelResult) == 24 and C.sizeof(ffi.LabelDesc) == 88 and C.sizeof(ffi.LabelsToMaskDesc) == 40
    assert (ffi.LABEL_26, ffi.LABEL_FROM_MASK) == (1, 2)


def test_entry_points_exist_and_refuse_null_without_a_device():
    L = ffi.lib()
    assert "clwh_segment_label" in ffi.EXPORTED_SYMBOLS and "clwh_labels_to_mask" in ffi.EXPORTED_SYMBOLS
    d, res = ffi.LabelDesc(), ffi.LabelResult()
    d.result = C.pointer(res)
    assert L.clwh_segment_label(None, C.byref(d)) == INVALID_VALUE
    assert L.clwh_segment_label(C.c_void_p(1), None) == INVALID_VALUE  # (desc is tested before ctx is used)
    m = ffi.LabelsToMaskDesc()
    assert L.clwh_labels_to_mask(None, C.byref(m)) == INVALID_VALUE
    assert L.clwh_labels_to_mask(C.c_void_p(1), None) == INVALID_VALUE
    assert res.as_dict() == {"n_components": 0, "n_voxels": 0}
