"""clwh_segment_label and clwh_labels_to_mask on the GPU against the contract's numpy restatement (tests/label_ref.py): equal bytes of
labels, table, result and mask, no tolerance anywhere.  The labels buffer is pre-filled with 0xFFFFFFFF, the table with a pattern."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import grow_ref as gr
from tests import label_ref as lr
from tests import mesh_ref as mr
from tests.grow_ref import RANDOM_DIMS, WINDOWS, random_volume
from tests.test_gpu_mesh import check as check_mesh
from tests.view_helpers import ROOT, host_lib, image_of

pytestmark = pytest.mark.gpu

INVALID_VALUE, SIZE_MISMATCH = 1, 9
L26, FROM_MASK = ffi.LABEL_26, ffi.LABEL_FROM_MASK
REC = ffi.LABEL_COMPONENT_DTYPE
PATTERN = 0xA5


class Labeller:
    """a volume on the device with a labels buffer of its size (and four words behind it that nobody may write) and a table;
    every call checks labels, table and result against the reference"""

    def __init__(self, ctx, vol, volume=None):
        self.ctx, self.vol = ctx, vol
        Z, Y, X = vol.shape
        self.dims = (X, Y, Z)
        self.volume, self.owner = (volume, None) if volume is not None else image_of(ctx, vol)
        self.labels = ctx.buffer(4 * (vol.size + 4), np.uint32, (vol.size + 4,))
        self.calls = 0

    def raw(self, lo, hi, flags=0, box=None, mask=None, capacity=None, n_records=0):
        """(labels words, table bytes or None, contract fields) as the device wrote them; capacity None: no table"""
        self.labels.push(np.full(self.vol.size + 4, 0xFFFFFFFF, np.uint32))
        table = self.ctx.buffer_from(np.full(48 * max(n_records, 1), PATTERN, np.uint8)) if capacity is not None else None
        status, res = self.ctx.label_components_raw(self.volume, lo, hi, flags, box, mask, self.labels, table, capacity or 0)
        assert status == 0, status
        words = self.labels.pull()
        assert (words[self.vol.size:] == 0xFFFFFFFF).all()  # nothing behind the X * Y * Z words is written
        got = table.pull() if table is not None else None
        if table is not None:
            table.release()
        self.calls += 1
        return words[:self.vol.size].reshape(self.vol.shape), got, res.as_dict()

    def check(self, lo, hi, connectivity=6, box=None, mask=None, mask_image=None, what=""):
        """reference == device == device again, with a table of n + 5 records; returns the reference's (ranks, table, result)"""
        ranks, table, res = lr.label(self.vol, lo, hi, connectivity, box, mask_image)
        n = res["n_components"]
        want = np.concatenate([table.view(np.uint8), np.full(48 * 5, PATTERN, np.uint8)])  # records from n on keep their pre-fill
        flags = (L26 if connectivity == 26 else 0) | (FROM_MASK if mask is not None else 0)
        for turn in ("first", "again"):
            got = self.raw(lo, hi, flags, box, mask, n + 5, n + 5)
            assert got[2] == res, (what, turn, got[2], res)
            assert np.array_equal(got[0] > 0, ranks > 0), (what, turn, "admissible")
            assert np.array_equal(got[0], ranks), (what, turn, "ranks", int((got[0] != ranks).sum()))
            assert np.array_equal(got[1], want), (what, turn, "table", got[1][:48 * min(n, 2)].view(REC), table[:2])
        return ranks, table, res

    def release(self):
        for m in (self.labels, self.volume, self.owner):
            if m is not None:
                m.release()


@pytest.mark.parametrize("dims", RANDOM_DIMS)
def test_random_volumes_equal_the_reference(gpu_ctx, dims):
    vol = random_volume(dims, 7)
    g = Labeller(gpu_ctx, vol)
    total = 0
    for connectivity in (6, 26):
        lo, hi = WINDOWS[connectivity]
        _, table, res = g.check(lo, hi, connectivity, what=(dims, connectivity))
        assert 243 <= res["n_components"] <= 3858
        sizes, n = np.unique(table["count"], return_counts=True)
        assert int(n[n > 1].sum()) > res["n_components"] // 2  # most ranks are decided by the tie rule
        total += res["n_components"]
    assert g.calls == 4 and total > 500
    g.release()


def test_two_serpentines(gpu_ctx):
    g = Labeller(gpu_ctx, lr.two_serpentines())
    for connectivity in (6, 26):
        _, table, res = g.check(100, 100, connectivity, what=("serpentines", connectivity))
        assert table["count"].tolist() == [2739, 2739] and table["first"].tolist() == [[0, 0, 1], [0, 1, 3]]
    g.release()


def test_comb(gpu_ctx):
    for joined, n in ((True, 1), (False, 9)):
        g = Labeller(gpu_ctx, lr.comb(joined))
        for connectivity in (6, 26):
            _, table, res = g.check(100, 100, connectivity, what=("comb", joined, connectivity))
            assert res["n_components"] == n and (not joined or table["count"].tolist() == [19890])
            assert table["first"][0].tolist() == [0, 0, 0]
        g.release()


def test_checkerboard(gpu_ctx):
    g = Labeller(gpu_ctx, lr.checkerboard())
    ranks, _, res = g.check(100, 100, 6, what="checkerboard, 6")
    assert res["n_components"] == 11970 and np.array_equal(ranks[ranks > 0], np.arange(1, 11971))
    _, table, res = g.check(100, 100, 26, what="checkerboard, 26")
    assert res["n_components"] == 1 and table["count"][0] == 11970
    g.release()


def test_diagonal_contacts(gpu_ctx):
    for a, b in (((63, 15, 15), (64, 16, 16)), ((63, 15, 5), (64, 16, 5))):
        g = Labeller(gpu_ctx, lr.contact(a, b))
        assert g.check(100, 100, 6, what=(a, b, 6))[2]["n_components"] == 2
        assert g.check(100, 100, 26, what=(a, b, 26))[2]["n_components"] == 1
        g.release()


def test_extremes(gpu_ctx):
    n = 0
    for dims in ((1, 1, 1), (7, 1, 1), (63, 3, 2), (64, 3, 2), (65, 3, 2)):
        X, Y, Z = dims
        vol = np.random.default_rng(X).integers(0, 3, (Z, Y, X)).astype(np.int16)
        g = Labeller(gpu_ctx, vol)
        for connectivity in (6, 26):
            _, _, res = g.check(5, 9, connectivity, what=(dims, "nothing"))
            assert res == {"n_components": 0, "n_voxels": 0}
            _, table, res = g.check(0, 2, connectivity, what=(dims, "everything"))
            assert res == {"n_components": 1, "n_voxels": X * Y * Z} and table["bbox_hi"][0].tolist() == [X, Y, Z] and table["count"][0] == X * Y * Z
            g.check(1, 2, connectivity, what=(dims, "some"))
            n += 3
        labels, table, res = g.raw(5, 9, capacity=3, n_records=3)  # nothing admissible: labels all zero, the table untouched
        assert not labels.any() and (table == PATTERN).all()
        g.release()
    assert n == 30


def test_volume_image_at_an_odd_address(gpu_ctx):
    """rows of a multiple of 8 voxels at a pointer that is 2-byte but not 16-byte aligned: the path for ragged rows must take it"""
    ctx = gpu_ctx
    vol = random_volume((72, 9, 5), 3)
    owner = ctx.buffer_from(np.concatenate([np.zeros(1, np.int16), vol.reshape(-1)]))
    volume = ctx.image_wrap(owner.device_ptr + 2, (72, 9, 5), 1, np.int16)
    assert volume.device_ptr % 16 == 2
    g = Labeller(ctx, vol, volume)
    for connectivity in (6, 26):
        assert g.check(*WINDOWS[connectivity], connectivity, what=("odd address", connectivity))[2]["n_components"] > 20
    g.release()
    owner.release()


def test_boxes_and_masks(gpu_ctx):
    ctx = gpu_ctx
    dims = (70, 40, 36)
    vol = random_volume(dims, 7)
    lo, hi = WINDOWS[6]
    g = Labeller(ctx, vol)
    whole = g.check(lo, hi, what="no box")[2]
    for box in (((0, 0, 0), (70, 40, 36)), ((5, 3, 2), (66, 17, 33)), ((64, 16, 16), (65, 17, 17)), ((0, 0, 20), (70, 40, 21))):
        res = g.check(lo, hi, 6, box, what=box)[2]
        assert res["n_voxels"] <= whole["n_voxels"]
    g.check(*WINDOWS[26], 26, ((5, 3, 2), (66, 17, 33)), what="box, 26")
    for box in (((0, 0, 0), (0, 40, 36)), ((9, 9, 9), (9, 9, 9))):  # empty boxes
        labels, table, res = g.raw(lo, hi, 0, box, capacity=2, n_records=2)
        assert not labels.any() and (table == PATTERN).all() and res == {"n_components": 0, "n_voxels": 0}
    # the mask of a grown region and a tighter window: the region falls apart; the mask is only read
    first, _, _ = gr.largest_component(gr.admissible(vol, lo, hi), 6)
    mask, grown = ctx.grow_region(g.volume, [first], lo, hi)
    region, _ = gr.grow(vol, [first], lo, hi)
    before = mask.pull()
    assert before.tobytes() == gr.packed(region).tobytes() and grown.count == region.sum()
    for connectivity in (6, 26):
        _, table, res = g.check(-1000, -500, connectivity, mask=mask, mask_image=region, what=("from the mask", connectivity))
        assert res["n_components"] > 10 and res["n_voxels"] < grown.count
        assert mask.pull().tobytes() == before.tobytes()
    everything = g.check(-1000, 999, 6, mask=mask, mask_image=region, what="the mask alone")[2]
    assert everything == {"n_components": 1, "n_voxels": int(region.sum())}
    mask.release()
    g.release()


def test_table_capacity(gpu_ctx):
    vol = random_volume((65, 17, 17), 7)
    lo, hi = WINDOWS[6]
    g = Labeller(gpu_ctx, vol)
    ranks, table, res = lr.label(vol, lo, hi)
    n = res["n_components"]
    labels, none, got = g.raw(lo, hi)  # components NULL
    assert none is None and got == res and np.array_equal(labels, ranks)
    labels, short, got = g.raw(lo, hi, capacity=3, n_records=8)  # capacity 3 < n: three records, the rest of the buffer untouched
    assert got == res and np.array_equal(labels, ranks)
    assert np.array_equal(short[:144], table[:3].view(np.uint8)) and (short[144:] == PATTERN).all()
    labels, more, got = g.raw(lo, hi, capacity=n + 5, n_records=n + 5)
    assert np.array_equal(more[:48 * n], table.view(np.uint8)) and (more[48 * n:] == PATTERN).all() and len(more) == 48 * (n + 5)
    # the high-level call: a structured table
    mem, r, t = gpu_ctx.label_components(g.volume, lo, hi, capacity=16)
    assert r.as_dict() == res and np.array_equal(t, table[:16]) and np.array_equal(mem.pull(), ranks)
    mem.release()
    g.release()


def test_components_equal_growth_on_the_device(gpu_ctx):
    ctx = gpu_ctx
    dims = (70, 40, 36)
    vol = random_volume(dims, 7)
    volume = ctx.image_from(vol)
    for connectivity in (6, 26):
        lo, hi = WINDOWS[connectivity]
        labels, res, table = ctx.label_components(volume, lo, hi, connectivity, capacity=5000)
        n = int(res.n_components)
        assert n == len(table) > 200
        ranks = labels.pull()
        for rank in (1, 2, n):
            rec = table[rank - 1]
            mask, grown = ctx.grow_region(volume, [tuple(int(v) for v in rec["first"])], lo, hi, connectivity)
            assert mask.pull().tobytes() == scene.mask_pack(ranks == rank).tobytes(), (connectivity, rank)
            assert (grown.count, tuple(grown.bbox_lo), tuple(grown.bbox_hi)) == (rec["count"], tuple(rec["bbox_lo"]), tuple(rec["bbox_hi"]))
            mask.release()
        labels.release()
    volume.release()


RAGGED = ((130, 3, 7), (1, 1, 1), (64, 16, 16), (72, 5, 4))


def test_labels_to_mask_and_apply(gpu_ctx):
    ctx = gpu_ctx
    checked = 0
    for dims in RAGGED:
        X, Y, Z = dims
        vol = np.random.default_rng(X).integers(0, 4, (Z, Y, X)).astype(np.int16)
        vol[0, 0, 0] = 1
        ranks, table, res = lr.label(vol, 1, 1)
        n = res["n_components"]
        volume, owner = image_of(ctx, vol)
        labels = ctx.buffer(4 * vol.size, np.uint32, vol.shape)
        status, got = ctx.label_components_raw(volume, 1, 1, labels=labels)
        assert status == 0 and got.as_dict() == res and np.array_equal(labels.pull(), ranks)
        words = scene.mask_words_per_row(X) * Y * Z
        mask = ctx.buffer(4 * (words + 2), np.uint32, (words + 2,))
        for rank_lo, rank_hi in ((1, 1), (2, max(n, 2)), (1, n), (n + 1, 0xFFFFFFFF)):
            mask.push(np.full(words + 2, 0xFFFFFFFF, np.uint32))  # ones: the padding must become zero
            assert ctx.labels_to_mask_raw(labels, mask, dims, rank_lo, rank_hi) == 0
            bits = mask.pull()
            assert bits[:words].tobytes() == lr.packed_selection(ranks, rank_lo, rank_hi).tobytes(), (dims, rank_lo, rank_hi)
            assert (bits[words:] == 0xFFFFFFFF).all()
            for fill, invert in ((-32768, False), (77, True)):
                out, out_owner = image_of(ctx, np.full_like(vol, 5))
                assert ctx.apply_mask_raw(volume, mask, out, fill, ffi.MASK_INVERT if invert else 0) == 0
                want = gr.apply_mask(vol, lr.selection(ranks, rank_lo, rank_hi), fill, invert)
                assert np.array_equal((out_owner or out).pull(np.int16, vol.shape), want), (dims, rank_lo, rank_hi, fill, invert)
                for m in (out, out_owner):
                    if m is not None:
                        m.release()
                checked += 1
        own = ctx.labels_to_mask(labels, dims, 1, n)  # the allocating call
        assert own.pull().tobytes() == scene.mask_pack(ranks > 0).tobytes()
        for m in (own, mask, labels, volume, owner):
            if m is not None:
                m.release()
    assert checked == 32
    # a labels buffer at an address that is 4-byte but not 16-byte aligned, rows of 8: the ragged path
    vol = random_volume((72, 5, 4), 2)
    ranks, _, _ = lr.label(vol, *WINDOWS[6])
    owner = ctx.buffer_from(np.concatenate([np.zeros(1, np.uint32), ranks.reshape(-1)]))
    shifted = ctx.wrap(owner.device_ptr + 4, 4 * ranks.size)
    mask = ctx.labels_to_mask(shifted, (72, 5, 4), 2, 9)
    assert mask.pull().tobytes() == lr.packed_selection(ranks, 2, 9).tobytes()
    for m in (mask, shifted, owner):
        m.release()


def test_keep_components(gpu_ctx):
    ctx = gpu_ctx
    vol = random_volume((70, 40, 36), 7)
    lo, hi = WINDOWS[6]
    ranks, table, res = lr.label(vol, lo, hi)
    volume = ctx.image_from(vol)
    mask, got, kept = ctx.keep_components(volume, lo, hi, largest=3)
    assert kept == 3 and got.as_dict() == res and mask.pull().tobytes() == lr.packed_selection(ranks, 1, 3).tobytes()
    mask.release()
    big = int(table["count"][4])
    want = int((table["count"] >= big).sum())
    mask, got, kept = ctx.keep_components(volume, lo, hi, min_count=big)
    assert kept == want and mask.pull().tobytes() == lr.packed_selection(ranks, 1, want).tobytes()
    mask.release()
    mask, got, kept = ctx.keep_components(volume, lo, hi, min_count=10 ** 6)
    assert kept == 0 and not mask.pull().any()
    mask.release()
    with pytest.raises(ValueError, match="larger capacity"):
        ctx.keep_components(volume, lo, hi, min_count=1, capacity=16)
    with pytest.raises(ValueError):
        ctx.keep_components(volume, lo, hi)
    volume.release()


def test_phantom_end_to_end_mesh_of_the_largest_bone_shell(gpu_ctx):
    ctx = gpu_ctx
    vol = scene.phantom(96)
    g = Labeller(ctx, vol)
    ranks, table, res = g.check(500, 1200, 6, what="bone")
    assert res["n_components"] == 2 and table["count"].tolist() == [30548, 30548]
    labels, table26, res26 = g.raw(500, 1200, L26, capacity=4, n_records=4)
    assert res26 == res and table26[:96].view(REC)["count"].tolist() == [30548, 30548]
    mask, _, kept = ctx.keep_components(g.volume, 500, 1200, largest=1)
    assert kept == 1
    ctx.apply_mask(g.volume, mask, fill=-32768)
    masked = gr.apply_mask(vol, ranks == 1)
    assert np.array_equal(g.volume.pull(), masked)
    pos, nrm, tri, keys = ctx.mesh_isosurface(g.volume, 500.0, normals=True, keys=True)
    want = mr.mesh(masked, 500.0)
    assert len(want.keys) > 30000
    check_mesh((keys, pos.view(np.uint32), nrm.view(np.uint32), tri), want, "mesh of the phantom's largest bone shell")
    mask.release()
    g.release()


def test_status_codes_and_nothing_written(gpu_ctx):
    ctx = gpu_ctx
    vol = random_volume((70, 12, 9), 3)
    volume = ctx.image_from(vol)
    n = vol.size
    labels = ctx.buffer_from(np.full(n + 4, 0xA5A5A5A5, np.uint32))
    short = ctx.buffer_from(np.full(n - 1, 0xA5A5A5A5, np.uint32))
    table = ctx.buffer_from(np.full(48 * 4, PATTERN, np.uint8))
    words = scene.mask_words_per_row(70) * 12 * 9
    mask = ctx.buffer_from(np.full(words, 0xA5A5A5A5, np.uint32))
    short_mask = ctx.buffer_from(np.full(words - 1, 0xA5A5A5A5, np.uint32))
    frame = ctx.image([64, 32], 4, np.uint8, (32, 64, 4))
    as_image = ctx.image([4, 4, n // 16 + 1], 1, np.uint32)
    odd_labels = ctx.wrap(labels.device_ptr + 2, 4 * n)
    odd_table = ctx.wrap(table.device_ptr + 4, 48 * 3)
    odd_mask = ctx.wrap(mask.device_ptr + 4, 4 * words - 4)
    huge = ctx.image_wrap(volume.device_ptr, (1 << 31, 1, 1), 1, np.int16)     # never read: refused by its dims
    two31 = ctx.image_wrap(volume.device_ptr, (1 << 16, 1 << 15, 1), 1, np.int16)  # each dim fits, the product is 2^31

    def status(**kw):
        args = dict(volume=volume, lo=-1000, hi=0, flags=0, box=None, mask=None, labels=labels, components=table, capacity=4)
        args.update(kw)
        st, res = ctx.label_components_raw(**args)
        if st != 0:
            assert res.as_dict() == {"n_components": 0, "n_voxels": 0} and res.passes == 0
        return st

    def untouched():
        return all((m.pull(np.uint8, (m.nbytes,)) == PATTERN).all() for m in (labels, short, table, mask, short_mask))

    L = ffi.lib()
    d, res = ffi.LabelDesc(), ffi.LabelResult()
    d.volume, d.labels, d.lo, d.hi = volume.h, labels.h, -1000, 0
    assert L.clwh_segment_label(ctx.h, C.byref(d)) == INVALID_VALUE  # result is NULL
    d.result = C.pointer(res)
    assert L.clwh_segment_label(None, C.byref(d)) == INVALID_VALUE and L.clwh_segment_label(ctx.h, None) == INVALID_VALUE
    assert status(volume=None) == INVALID_VALUE and status(volume=frame) == INVALID_VALUE and status(volume=labels) == INVALID_VALUE
    assert status(labels=None) == INVALID_VALUE and status(labels=as_image) == INVALID_VALUE and status(labels=odd_labels) == INVALID_VALUE
    assert status(components=as_image) == INVALID_VALUE and status(components=odd_table, capacity=3) == INVALID_VALUE
    assert status(components=None, capacity=1) == INVALID_VALUE
    for bad in (None, as_image, odd_mask):
        assert status(flags=FROM_MASK, mask=bad) == INVALID_VALUE
    assert status(flags=4) == INVALID_VALUE and status(flags=-1) == INVALID_VALUE and status(flags=1 << 16) == INVALID_VALUE
    for lo, hi in ((1, 0), (-32769, 0), (0, 32768), (-40000, 40000)):
        assert status(lo=lo, hi=hi) == INVALID_VALUE, (lo, hi)
    for box in (((0, 0, 0), (71, 12, 9)), ((0, 0, 0), (70, 13, 9)), ((0, 0, 0), (70, 12, 10)), ((5, 0, 0), (4, 12, 9)), ((0, 0, 3), (70, 12, 2)),
                ((71, 0, 0), (0, 0, 0)), ((0, 0, 0), (0, 0, 1 << 31))):
        assert status(box=box) == INVALID_VALUE, box
    assert status(volume=huge) == INVALID_VALUE and status(volume=two31) == INVALID_VALUE
    assert status(labels=short) == SIZE_MISMATCH and status(capacity=5) == SIZE_MISMATCH and status(capacity=1 << 62) == SIZE_MISMATCH
    assert status(flags=FROM_MASK, mask=short_mask) == SIZE_MISMATCH
    assert status(labels=short, flags=4) == INVALID_VALUE  # INVALID_VALUE before SIZE_MISMATCH
    assert untouched()
    # and the same arguments without the defect are accepted: limits included
    assert status(lo=-32768, hi=32767) == 0 and status(flags=3, mask=mask) == 0 and status(box=((70, 12, 9), (70, 12, 9))) == 0
    assert status(components=None, capacity=0) == 0 and status(components=table, capacity=0) == 0 and status(mask=odd_mask) == 0  # no flag: ignored
    assert (mask.pull() == 0xA5A5A5A5).all()
    ranks, want, _ = lr.label(vol, -1000, 0, capacity=4)
    assert status() == 0 and np.array_equal(labels.pull()[:n].reshape(vol.shape), ranks) and (labels.pull()[n:] == 0xA5A5A5A5).all()
    assert np.array_equal(table.pull(np.uint8), want.view(np.uint8))

    # clwh_labels_to_mask
    def to_mask(**kw):
        args = dict(labels=labels, mask=mask, dims=(70, 12, 9), rank_lo=1, rank_hi=2)
        args.update(kw)
        return ctx.labels_to_mask_raw(**args)

    m = ffi.LabelsToMaskDesc()
    m.labels, m.mask, m.rank_lo, m.rank_hi = labels.h, mask.h, 1, 1
    m.dims[0], m.dims[1], m.dims[2] = 70, 12, 9
    assert L.clwh_labels_to_mask(None, C.byref(m)) == INVALID_VALUE and L.clwh_labels_to_mask(ctx.h, None) == INVALID_VALUE
    assert to_mask(labels=None) == INVALID_VALUE and to_mask(labels=as_image) == INVALID_VALUE and to_mask(labels=odd_labels) == INVALID_VALUE
    assert to_mask(mask=None) == INVALID_VALUE and to_mask(mask=volume) == INVALID_VALUE and to_mask(mask=odd_mask) == INVALID_VALUE
    assert to_mask(dims=(0, 12, 9)) == INVALID_VALUE and to_mask(dims=(70, 12, 0)) == INVALID_VALUE
    assert to_mask(dims=(1 << 31, 1, 1)) == INVALID_VALUE and to_mask(dims=(1 << 16, 1 << 15, 1)) == INVALID_VALUE
    assert to_mask(rank_lo=0) == INVALID_VALUE and to_mask(rank_lo=3, rank_hi=2) == INVALID_VALUE
    assert to_mask(labels=short) == SIZE_MISMATCH and to_mask(mask=short_mask) == SIZE_MISMATCH
    assert to_mask(labels=short, rank_lo=0) == INVALID_VALUE
    assert (mask.pull() == 0xA5A5A5A5).all() and (short_mask.pull() == 0xA5A5A5A5).all()
    assert to_mask() == 0 and mask.pull().tobytes() == lr.packed_selection(ranks, 1, 2).tobytes()
    assert to_mask(rank_lo=0xFFFFFFFF, rank_hi=0xFFFFFFFF) == 0 and not mask.pull().any()
    for x in (two31, huge, odd_mask, odd_table, odd_labels, as_image, frame, short_mask, mask, table, short, labels, volume):
        x.release()


def _phantom48_reference():
    vol = scene.phantom(48)
    ranks, table, res = lr.label(vol, 500, 1200)
    assert res["n_components"] == 2 and table["count"].tolist() == [3940, 3940]
    return vol, ranks, table, res


def test_host_mirror_labels_selects_and_applies():
    n = 48
    vol, ranks, table, res = _phantom48_reference()
    env = scene.env_map(64, 32)
    L = host_lib(clvr_host_label_components=(C.c_uint, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(C.c_ulonglong),
                                                          C.POINTER(C.c_ulonglong), C.c_void_p]),
                 clvr_host_select_components=(None, [C.c_void_p, C.c_uint, C.c_uint]),
                 clvr_host_apply_mask=(None, [C.c_void_p, C.c_int, C.c_int]),
                 clvr_host_extract_mesh=(None, [C.c_void_p, C.c_float, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong),
                                                C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_float)),
                                                C.POINTER(C.POINTER(C.c_ulonglong)), C.POINTER(C.POINTER(C.c_uint))]))
    h = L.clvr_host_create()
    try:
        L.clvr_host_load(h, vol.ctypes.data, n, n, n, env.ctypes.data, 64, 32)
        nc, nvox = C.c_ulonglong(0), C.c_ulonglong(0)
        records = np.full(8, 0, REC)
        for flags in (0, L26):
            written = L.clvr_host_label_components(h, 500, 1200, flags, 8, C.byref(nc), C.byref(nvox), records.ctypes.data)
            assert (written, nc.value, nvox.value) == (2, 2, res["n_voxels"]) and np.array_equal(records[:2], table)
        written = L.clvr_host_label_components(h, 500, 1200, 0, 1, C.byref(nc), C.byref(nvox), records.ctypes.data)
        assert (written, nc.value) == (1, 2)
        L.clvr_host_select_components(h, 2, 2)
        L.clvr_host_apply_mask(h, -32768, 0)
        nv, nt = C.c_ulonglong(0), C.c_ulonglong(0)
        p, q = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
        k, t = C.POINTER(C.c_ulonglong)(), C.POINTER(C.c_uint)()
        L.clvr_host_extract_mesh(h, 500.0, 0, C.byref(nv), C.byref(nt), C.byref(p), C.byref(q), C.byref(k), C.byref(t))
        want = mr.mesh(gr.apply_mask(vol, ranks == 2), 500.0)
        assert (nv.value, nt.value) == (len(want.keys), len(want.tris)) and nv.value > 5000
    finally:
        L.clvr_host_destroy(h)


def test_headless_components_then_mesh(tmp_path):
    vol, ranks, table, res = _phantom48_reference()
    scene.write_nrrd(str(tmp_path / "v.nrrd"), vol)
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(np.random.default_rng(5).random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    files = [str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", "64", "64"]

    def run(*options):
        out = subprocess.run([exe] + list(options) + files + [str(tmp_path / "m.ply")], capture_output=True, text=True, timeout=120)
        return out.returncode, [json.loads(s) for s in out.stdout.strip().splitlines() if s.startswith("{")], out.stderr

    code, lines, err = run("--components=500,1200,largest=1", "--mesh=500")
    assert code == 0, err
    c = lines[0]
    assert (c["n_components"], c["n_voxels"], c["selected"]) == (2, res["n_voxels"], [1, 1])
    assert (c["components"], c["connectivity"], c["mode"], c["fill"]) == ([500, 1200], 6, "keep", -32768)
    assert len(c["largest"]) == 2
    for got, want in zip(c["largest"], table):
        assert (got["count"], got["first"], got["bbox_lo"], got["bbox_hi"]) == (3940, want["first"].tolist(), want["bbox_lo"].tolist(), want["bbox_hi"].tolist())
    want = mr.mesh(gr.apply_mask(vol, ranks == 1), 500.0)
    assert (lines[-1]["vertices"], lines[-1]["triangles"]) == (len(want.keys), len(want.tris))
    pos, nrm, tri = scene.read_ply(str(tmp_path / "m.ply"))
    rows = lambda p, q: np.sort(np.ascontiguousarray(np.concatenate([p, q], axis=1)).view([("", np.uint32)] * 6).reshape(-1))
    assert np.array_equal(rows(pos.view(np.uint32), nrm.view(np.uint32)), rows(want.pos, want.nrm))
    _, ids = np.unique(np.concatenate([pos.view(np.uint32), want.pos]), axis=0, return_inverse=True)
    ids = ids.reshape(-1)
    assert np.array_equal(mr.canonical(ids[:len(pos)][tri]), mr.canonical(ids[len(pos):][mr.index_triangles(want)]))
    # min=N with 26-connectivity, remove, a fill of its own: both shells have N voxels, one more has none
    code, lines, err = run("--components=500,1200,26,min=3940,remove,fill=-1000", "--mesh=500")
    assert code == 0, err
    assert lines[0]["selected"] == [1, 2] and (lines[0]["connectivity"], lines[0]["mode"], lines[0]["fill"]) == (26, "remove", -1000)
    assert lines[-1]["vertices"] == len(mr.mesh(gr.apply_mask(vol, ranks > 0, -1000, True), 500.0).keys)
    code, lines, err = run("--components=500,1200,min=3941", "--mesh=500")
    assert code == 0 and lines[0]["selected"] == [0, 0] and lines[-1]["vertices"] == 0
    for bad in (("--components=500",), ("--components=1200,500",), ("--components=500,1200,18",), ("--components=500,1200,",),
                ("--components=500,1200,largest=0",), ("--components=500,1200,largest=1,min=5",), ("--components",),
                ("--components=500,1200", "--grow=1,2,3,500,1200")):
        assert run(*bad)[0] == 1, bad
