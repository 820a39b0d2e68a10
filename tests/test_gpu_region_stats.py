"""clwh_mask_statistics and clwh_label_statistics on the GPU against the contract's numpy restatement (tests/region_stats_ref.py): equal
bytes of records, tables and histograms, no tolerance anywhere.  Outputs on the device are allocated too long and pre-filled with a
pattern that must survive behind what the call writes."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import distance_ref as dr
from tests import grow_ref as gr
from tests import label_ref as lr
from tests import region_stats_ref as rs
from tests.view_helpers import ROOT, host_lib

pytestmark = pytest.mark.gpu

INVALID_VALUE, SIZE_MISMATCH = 1, 9
PATTERN = 0xA5A5A5A5
REC = 104
# 1 voxel; rows that are no multiple of 8, 32 or 64; whole words; a word boundary inside a row plus padding; three words per row with
# ragged rows; the dim = 1 faces along y and z, and along x and y; many blocks (cross-block atomics, the grid-stride loop)
SHAPES = ((1, 1, 1), (37, 19, 11), (64, 16, 16), (70, 9, 5), (130, 3, 2), (200, 1, 1), (1, 1, 200), (128, 128, 96))
SMALL = SHAPES[:-1]


def volume_of(dims, seed=1):
    X, Y, Z = dims
    return np.random.default_rng(seed).integers(-32768, 32768, (Z, Y, X)).astype(np.int16)


class image_of:
    """vol [z][y][x] as an S16 image on the device; a row of one voxel (which clwh_image_create refuses, like the reference's wrapper)
    is a buffer adopted as an image"""

    def __init__(self, ctx, vol):
        self.owner = None
        if vol.shape[2] > 1:
            self.mem = ctx.image_from(vol)
        else:
            self.owner = ctx.buffer_from(vol)
            self.mem = ctx.image_wrap(self.owner.device_ptr, vol.shape[::-1], 1, np.int16, vol.shape)

    def release(self):
        self.mem.release()
        if self.owner is not None:
            self.owner.release()


def garbage(mask):
    """the mask's words with every bit at x >= X and every padding word set"""
    Z, Y, X = mask.shape
    wpr = scene.mask_words_per_row(X)
    padded = np.ones((Z, Y, wpr * 32), np.uint8)
    padded[:, :, :X] = mask
    return np.packbits(padded, axis=2, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def record_bytes(stats):
    return bytes(memoryview(stats))


def mask_stats(ctx, volume, words, hist=None):
    """(record as a rs.DTYPE scalar, hist | None, below, above) of one call; the mask is read only"""
    mask = ctx.buffer_from(words)
    try:
        stats, counts, below, above = ctx.mask_statistics(volume, mask, hist)
        assert np.array_equal(mask.pull(), words)
        return np.frombuffer(record_bytes(stats), rs.DTYPE)[0], counts, below, above
    finally:
        mask.release()


def same_record(got, want, what):
    assert got.tobytes() == want.tobytes(), (what, rs.as_dict(got), rs.as_dict(want))


def label_stats(ctx, vol, labels, capacity, tail=2):
    """the table as the device wrote it, twice into a poisoned buffer that is `tail` records too long"""
    image, lab = image_of(ctx, vol), ctx.buffer_from(np.ascontiguousarray(labels, np.uint32))
    volume = image.mem
    table = ctx.buffer(REC * (capacity + tail), np.uint8)
    out = None
    try:
        for turn in ("first", "again"):
            table.push(np.full(REC * (capacity + tail) // 4, PATTERN, np.uint32))
            assert ctx.label_statistics_raw(volume, lab, table, capacity) == 0
            raw = table.pull(np.uint8)
            assert (raw[REC * capacity:].view(np.uint32) == PATTERN).all(), (turn, "written behind the table")
            got = raw[:REC * capacity].view(rs.DTYPE).copy()
            assert out is None or got.tobytes() == out.tobytes(), turn
            out = got
        assert np.array_equal(lab.pull().reshape(-1), np.asarray(labels, np.uint32).reshape(-1))
        return out
    finally:
        for m in (table, lab, image):
            m.release()


def same_table(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = [k for k in range(len(want)) if got[k].tobytes() != want[k].tobytes()]
        raise AssertionError((what, len(bad), bad[:3], rs.as_dict(got[bad[0]]), rs.as_dict(want[bad[0]])))


# ---- 1. masks
@pytest.mark.parametrize("dims", SHAPES)
def test_mask_records_equal_the_reference(gpu_ctx, dims):
    X, Y, Z = dims
    vol = volume_of(dims)
    image = image_of(gpu_ctx, vol)
    volume = image.mem
    rng = np.random.default_rng(7)
    corner = np.zeros(vol.shape, bool)
    corner[Z - 1, 0, X - 1] = True
    cases = {"empty": np.zeros(vol.shape, bool), "full": np.ones(vol.shape, bool), "corner": corner,
             "half": rng.random(vol.shape) < 0.5, "sparse": rng.random(vol.shape) < 0.01}
    try:
        for name, region in cases.items():
            want = rs.record(vol, region)
            same_record(mask_stats(gpu_ctx, volume, scene.mask_pack(region))[0], want, (dims, name))
            same_record(mask_stats(gpu_ctx, volume, garbage(region))[0], want, (dims, name, "padding set"))
        assert mask_stats(gpu_ctx, volume, scene.mask_pack(cases["empty"]))[0].tobytes() == bytes(REC)
    finally:
        image.release()


@pytest.mark.parametrize("value", (-32768, 32767))
def test_extreme_volumes(gpu_ctx, value):
    dims = (128, 128, 96)
    vol = np.full(dims[::-1], value, np.int16)
    volume = gpu_ctx.image_from(vol)
    try:
        full = np.ones(vol.shape, bool)
        got = mask_stats(gpu_ctx, volume, scene.mask_pack(full))[0]
        same_record(got, rs.record(vol, full), value)
        n = 128 * 128 * 96
        assert (int(got["sum"]), int(got["sum_sq"])) == (n * value, n * value * value)
    finally:
        volume.release()


def test_a_volume_and_labels_that_are_not_16_byte_aligned(gpu_ctx):
    # rows of a multiple of 8 voxels at pointers the 16-byte loads cannot take: the lane-by-lane path
    dims = X, Y, Z = (72, 9, 5)
    vol = volume_of(dims, 12)
    owner = gpu_ctx.buffer_from(np.concatenate([np.zeros(1, np.int16), vol.reshape(-1)]))
    volume = gpu_ctx.image_wrap(owner.device_ptr + 2, dims, 1, np.int16)
    assert volume.device_ptr % 16 == 2
    labels = np.random.default_rng(1).integers(0, 6, vol.shape).astype(np.uint32)
    lab_owner = gpu_ctx.buffer_from(np.concatenate([np.zeros(1, np.uint32), labels.reshape(-1)]))
    lab = gpu_ctx.wrap(lab_owner.device_ptr + 4, 4 * X * Y * Z)
    table = gpu_ctx.buffer(REC * 4, np.uint8)
    try:
        region = labels > 2
        same_record(mask_stats(gpu_ctx, volume, garbage(region))[0], rs.record(vol, region), "mask")
        assert gpu_ctx.label_statistics_raw(volume, lab, table, 4) == 0
        same_table(table.pull(np.uint8).view(rs.DTYPE), rs.label_records(vol, labels, 4), "labels")
    finally:
        for m in (table, lab, lab_owner, volume, owner):
            m.release()


def _bone(n):
    vol = scene.phantom(n)
    z = n // 2
    y, x = np.argwhere(gr.admissible(vol, 500, 1200)[z])[0]
    return vol, (int(x), int(y), z)


def test_record_of_a_grown_region_equals_grows_result(gpu_ctx):
    vol, seed = _bone(64)
    volume = gpu_ctx.image_from(vol)
    mask, res = gpu_ctx.grow_region(volume, [seed], 500, 1200)
    try:
        stats, counts, below, above = gpu_ctx.mask_statistics(volume, mask)
        mine, grown = stats.as_dict(), res.as_dict()
        assert grown["count"] > 1000 and {k: mine[k] for k in grown} == grown
        assert (counts, below, above) == (None, 0, 0)
        region = scene.mask_unpack(mask.pull(), (64, 64, 64))
        assert record_bytes(stats) == rs.record(vol, region).tobytes()
    finally:
        mask.release()
        volume.release()


def test_record_after_morphology_and_algebra(gpu_ctx):
    vol, seed = _bone(48)
    dims = (48, 48, 48)
    volume = gpu_ctx.image_from(vol)
    mask, _ = gpu_ctx.grow_region(volume, [seed], 500, 1200)
    wide = gpu_ctx.mask_morph(mask, dims, ffi.MORPH_CLOSE, 9)
    ring = gpu_ctx.mask_morph(mask, dims, ffi.MORPH_DILATE, 4)
    gpu_ctx.mask_combine(ring, mask, ffi.MASK_ANDNOT, dims, out=ring)
    try:
        for m, name in ((wide, "closed"), (ring, "margin")):
            region = scene.mask_unpack(m.pull(), dims)
            assert region.any()
            stats = gpu_ctx.mask_statistics(volume, m)[0]
            assert record_bytes(stats) == rs.record(vol, region).tobytes(), name
    finally:
        for m in (ring, wide, mask, volume):
            m.release()


# ---- 2. histograms
HIST_CASES = {"every value": (-32768, 1, 65536), "wide": (-32768, 4096, 16), "tails": (-100, 7, 30), "one bin of all": (-32768, 65536, 1),
              "last value": (32767, 1, 1)}


@pytest.mark.parametrize("dims", ((37, 19, 11), (64, 16, 16), (128, 128, 96)))
def test_histograms_equal_the_reference(gpu_ctx, dims):
    vol = volume_of(dims, 3)
    volume = gpu_ctx.image_from(vol)
    region = np.random.default_rng(11).random(vol.shape) < 0.5
    words = garbage(region)
    want_record = rs.record(vol, region)
    try:
        for name, (lo, width, n) in HIST_CASES.items():
            got, counts, below, above = mask_stats(gpu_ctx, volume, words, (lo, width, n))
            want = rs.histogram(vol, region, lo, width, n)
            same_record(got, want_record, (dims, name))
            assert counts.dtype == np.uint64 and np.array_equal(counts, want[0]) and (below, above) == want[1:], (dims, name)
            assert int(counts.sum()) + below + above == int(want_record["count"])
    finally:
        volume.release()


def test_hot_bin_and_the_words_behind_the_histogram(gpu_ctx):
    dims = (128, 128, 96)
    vol = np.full(dims[::-1], 40, np.int16)  # CT: a region whose voxels all fall into one bin
    vol[::7, ::5, ::3] = 41
    volume = gpu_ctx.image_from(vol)
    region = np.ones(vol.shape, bool)
    mask = gpu_ctx.buffer_from(scene.mask_pack(region))
    n = 256
    table = gpu_ctx.buffer_from(np.full(2 * (n + 3), PATTERN, np.uint32))
    try:
        for lo, width in ((0, 1), (-1000, 8), (41, 1), (-32768, 1)):
            table.push(np.full(2 * (n + 3), PATTERN, np.uint32))
            status, res = gpu_ctx.mask_statistics_raw(volume, mask, table, lo, width, n)
            assert status == 0
            raw = table.pull(np.uint32)
            assert (raw[2 * n:] == PATTERN).all(), "written behind n_bins words"
            want = rs.histogram(vol, region, lo, width, n)
            assert np.array_equal(raw[:2 * n].view(np.uint64), want[0]) and (int(res.hist_below), int(res.hist_above)) == want[1:]
            assert record_bytes(res.stats) == rs.record(vol, region).tobytes()
    finally:
        for m in (table, mask, volume):
            m.release()


# ---- 3. labels
@pytest.mark.parametrize("dims", SHAPES)
def test_one_rank_owns_the_volume(gpu_ctx, dims):
    vol = volume_of(dims, 5)
    labels = np.ones(vol.shape, np.uint32)
    got = label_stats(gpu_ctx, vol, labels, 3)
    same_table(got, rs.label_records(vol, labels, 3), dims)
    assert got[0].tobytes() == rs.record(vol, labels == 1).tobytes() and got[1:].tobytes() == bytes(2 * REC)


@pytest.mark.parametrize("dims", SMALL)
def test_every_voxel_a_rank_of_its_own(gpu_ctx, dims):
    X, Y, Z = dims
    n = X * Y * Z
    vol = volume_of(dims, 6)
    labels = (np.random.default_rng(2).permutation(n) + 1).astype(np.uint32).reshape(Z, Y, X)
    same_table(label_stats(gpu_ctx, vol, labels, n + 5), rs.label_records(vol, labels, n + 5), dims)
    # a capacity below the number of ranks: the dropped ranks still make faces for their neighbours
    cap = max(1, n // 3)
    same_table(label_stats(gpu_ctx, vol, labels, cap), rs.label_records(vol, labels, cap), (dims, cap))


@pytest.mark.parametrize("dims", SHAPES)
def test_caller_made_labels(gpu_ctx, dims):
    X, Y, Z = dims
    vol = volume_of(dims, 8)
    rng = np.random.default_rng(4)
    # a few ranks in blobs and runs, with 0, ranks far above the capacity and 0xFFFFFFFF between them; ranks touch by faces
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    labels = (((x // 5) + (y // 3) * 2 + (z // 2) * 3) % 9).astype(np.uint32)
    noise = rng.random(vol.shape)
    labels[noise < 0.05] = 0xFFFFFFFF
    labels[(noise >= 0.05) & (noise < 0.1)] = 1 << 30
    labels[(noise >= 0.1) & (noise < 0.2)] = rng.integers(0, 40, vol.shape).astype(np.uint32)[(noise >= 0.1) & (noise < 0.2)]
    for capacity in (6, 40):  # ranks 7 and 8 dropped, rank 40 absent
        got = label_stats(gpu_ctx, vol, labels, capacity)
        same_table(got, rs.label_records(vol, labels, capacity), (dims, capacity))
    assert got[39].tobytes() == bytes(REC)


def test_two_ranks_that_touch(gpu_ctx):
    vol = volume_of((70, 9, 5), 9)
    labels = np.full(vol.shape, 2, np.uint32)
    labels[:, :, :33] = 1
    got = label_stats(gpu_ctx, vol, labels, 2)
    same_table(got, rs.label_records(vol, labels, 2), "halves")
    assert tuple(got["faces"][0]) == tuple(got["faces"][1]) == (9 * 5, 0, 0)  # the one plane between them counts for both


def test_label_then_statistics_on_the_phantom(gpu_ctx):
    vol = scene.phantom(64)
    volume = gpu_ctx.image_from(vol)
    labels, res, table = gpu_ctx.label_components(volume, 500, 1200, capacity=64)
    n = min(int(res.n_components), 64)
    stats = gpu_ctx.label_statistics(volume, labels, 64)
    again = gpu_ctx.label_statistics(volume, labels, 64)
    try:
        got = stats.pull()
        assert got.dtype == rs.DTYPE and n >= 1 and again.pull().tobytes() == got.tobytes()
        assert np.array_equal(got["count"][:n], table["count"])
        assert np.array_equal(got["bbox_lo"][:n], table["bbox_lo"]) and np.array_equal(got["bbox_hi"][:n], table["bbox_hi"])
        ranks = labels.pull()
        assert np.array_equal(ranks, lr.label(vol, 500, 1200)[0])
        same_table(got, rs.label_records(vol, ranks, 64), "phantom")
    finally:
        for m in (again, stats, labels, volume):
            m.release()


# ---- 4. the C++ mirror and clvr_headless
def test_host_mirror_measures():
    n = 48
    vol, seed = _bone(n)
    region, _ = gr.grow(vol, [seed], 500, 1200)
    env = scene.env_map(64, 32)
    L = host_lib(clvr_host_grow_region=(None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p]),
                 clvr_host_label_components=(C.c_uint, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(C.c_ulonglong),
                                                         C.POINTER(C.c_ulonglong), C.c_void_p]),
                 clvr_host_measure_mask=(None, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
                 clvr_host_measure_labels=(None, [C.c_void_p, C.c_uint, C.c_void_p]))
    h = L.clvr_host_create()
    try:
        L.clvr_host_load(h, vol.ctypes.data, n, n, n, env.ctypes.data, 64, 32)
        seeds = np.array(seed, np.uint32)
        result = ffi.GrowResult()
        L.clvr_host_grow_region(h, seeds.ctypes.data, 1, 500, 1200, 0, C.byref(result))
        out = ffi.MaskStatsResult()
        L.clvr_host_measure_mask(h, 0, 0, 0, None, C.byref(out))
        assert record_bytes(out.stats) == rs.record(vol, region).tobytes() and (out.hist_below, out.hist_above) == (0, 0)
        hist = np.full(17, 77, np.uint64)
        L.clvr_host_measure_mask(h, 600, 50, 16, hist.ctypes.data, C.byref(out))
        want = rs.histogram(vol, region, 600, 50, 16)
        assert np.array_equal(hist[:16], want[0]) and hist[16] == 77 and (out.hist_below, out.hist_above) == want[1:]
        nc, nv = C.c_ulonglong(0), C.c_ulonglong(0)
        records = np.zeros(8, ffi.LABEL_COMPONENT_DTYPE)
        L.clvr_host_label_components(h, 500, 1200, 0, 8, C.byref(nc), C.byref(nv), records.ctypes.data)
        table = np.zeros(12, rs.DTYPE)
        L.clvr_host_measure_labels(h, 12, table.ctypes.data)
        same_table(table, rs.label_records(vol, lr.label(vol, 500, 1200)[0], 12), "mirror")
    finally:
        L.clvr_host_destroy(h)


def test_headless_measure(tmp_path):
    vol, seed = _bone(48)
    Z, Y, X = vol.shape
    header = "NRRD0004\ntype: short\ndimension: 3\nsizes: %d %d %d\nendian: little\nencoding: raw\n\n" % (X, Y, Z)
    with open(tmp_path / "v.nrrd", "wb") as f:
        f.write(header.encode("ascii") + np.ascontiguousarray(vol, "<i2").tobytes())
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(np.random.default_rng(5).random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    files = [str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", "64", "64"]

    def run(*options):
        out = subprocess.run([exe] + list(options) + files + [str(tmp_path / "m.ply")], capture_output=True, text=True, timeout=120)
        return out.returncode, [json.loads(s) for s in out.stdout.strip().splitlines() if s.startswith("{")], out.stderr

    def printed(rec):
        d = rs.as_dict(rec)
        d["min"], d["max"] = d.pop("vmin"), d.pop("vmax")
        return {k: (list(v) if isinstance(v, tuple) else v) for k, v in d.items()}

    bone, _ = gr.grow(vol, [seed], 500, 1200)
    code, lines, err = run("--grow=%d,%d,%d,500,1200,dilate=2,measure,remove,fill=-1000" % seed, "--mesh=-20000")
    assert code == 0, err
    grown = dr.morph(bone, (256, 256, 256), dr.DILATE, scene.radius_sq(2))
    assert lines[0]["count"] == int(bone.sum()) and lines[1] == {"measure": printed(rs.record(vol, grown))}  # of the volume as loaded
    code, lines, err = run("--components=500,1200,largest=3,measure", "--mesh=-20000")
    assert code == 0, err
    ranks = lr.label(vol, 500, 1200)[0]
    keep = min(3, int(ranks.max()))
    assert lines[1] == {"measure_components": [printed(r) for r in rs.label_records(vol, ranks, keep)]}
    assert "measure" not in run("--grow=%d,%d,%d,500,1200" % seed, "--mesh=-20000")[1][1]  # no item: no second line of it
    for bad in ("measure=1", "measure,", "measured"):
        assert run("--grow=%d,%d,%d,500,1200," % seed + bad)[0] == 1, bad


# ---- 5. status
def test_status_codes_and_nothing_written(gpu_ctx):
    ctx = gpu_ctx
    dims = X, Y, Z = (70, 12, 9)
    n, words = X * Y * Z, scene.mask_words_per_row(X) * Y * Z
    fill = lambda k: ctx.buffer_from(np.full(k, PATTERN, np.uint32))
    vol = volume_of(dims)
    volume = ctx.image_from(vol)
    wrong_kind = ctx.image([X, Y, Z], 1, np.uint8)
    as_image = ctx.image([4, 4, n // 4 + 1], 1, np.uint32)
    mask, short_mask = fill(words), fill(words - 1)
    bins, cap = 64, 5
    hist, short_hist = fill(2 * bins + 2), fill(2 * bins - 1)
    labels, short_labels = fill(n), fill(n - 1)
    table, short_table = fill(REC * cap // 4 + 2), fill(REC * cap // 4 - 1)
    odd_mask = ctx.wrap(mask.device_ptr + 4, 4 * words - 4)
    odd_hist = ctx.wrap(hist.device_ptr + 4, 8 * bins)
    odd_labels = ctx.wrap(labels.device_ptr + 2, 4 * n - 4)
    odd_table = ctx.wrap(table.device_ptr + 4, REC * cap)
    flat = ctx.image_wrap(volume.device_ptr, (1 << 16, 1 << 15, 1), 1, np.int16)  # never read: each dim fits, the product is 2^31
    huge = ctx.image_wrap(volume.device_ptr, (1 << 31, 1, 1), 1, np.int16)

    def mstat(**kw):
        args = dict(volume=volume, mask=mask, hist=hist, hist_lo=0, bin_width=1, n_bins=bins, flags=0)
        args.update(kw)
        status, res = ctx.mask_statistics_raw(**args)
        assert bytes(memoryview(res)) == bytes(C.sizeof(res)) or status == 0  # the host result is untouched on an error
        return status

    def lstat(**kw):
        args = dict(volume=volume, labels=labels, stats=table, capacity=cap, flags=0)
        args.update(kw)
        return ctx.label_statistics_raw(**args)

    L = ffi.lib()
    assert L.clwh_mask_statistics(None, C.byref(ffi.MaskStatsDesc())) == INVALID_VALUE and L.clwh_mask_statistics(ctx.h, None) == INVALID_VALUE
    assert L.clwh_label_statistics(None, C.byref(ffi.LabelStatsDesc())) == INVALID_VALUE and L.clwh_label_statistics(ctx.h, None) == INVALID_VALUE
    cases = [mstat(result=False)]
    cases += [mstat(volume=bad) for bad in (None, wrong_kind, mask)] + [lstat(volume=bad) for bad in (None, wrong_kind, mask)]
    cases += [mstat(mask=bad) for bad in (None, as_image, odd_mask)]
    cases += [mstat(flags=1), mstat(flags=-1), lstat(flags=1), lstat(flags=-1)]
    cases += [mstat(hist=as_image), mstat(hist=odd_hist)]
    cases += [mstat(n_bins=0), mstat(n_bins=-1), mstat(n_bins=65537), mstat(bin_width=0), mstat(bin_width=-3), mstat(hist_lo=-32769), mstat(hist_lo=32768)]
    cases += [mstat(hist=None, n_bins=1), mstat(hist=None, n_bins=bins)]
    cases += [lstat(labels=bad) for bad in (None, as_image, odd_labels)] + [lstat(stats=bad) for bad in (None, as_image, odd_table)]
    cases += [lstat(capacity=0), lstat(capacity=(1 << 24) + 1), lstat(capacity=1 << 40)]
    cases += [mstat(volume=flat), lstat(volume=flat), mstat(volume=huge), lstat(volume=huge)]
    assert cases == [INVALID_VALUE] * len(cases), cases
    sizes = [mstat(mask=short_mask), mstat(hist=short_hist), mstat(hist=hist, n_bins=bins + 2), lstat(labels=short_labels), lstat(stats=short_table),
             lstat(capacity=cap + 1)]
    assert sizes == [SIZE_MISMATCH] * len(sizes), sizes
    # INVALID_VALUE before SIZE_MISMATCH
    assert mstat(mask=short_mask, flags=2) == INVALID_VALUE and mstat(hist=short_hist, bin_width=0) == INVALID_VALUE
    assert lstat(labels=short_labels, capacity=0) == INVALID_VALUE and lstat(stats=short_table, flags=1) == INVALID_VALUE
    for m in (mask, short_mask, hist, short_hist, labels, short_labels, table, short_table):
        assert (m.pull(np.uint32, (m.nbytes // 4,)) == PATTERN).all()  # nothing was written
    # and the same arguments without the defect are accepted, limits included
    assert mstat() == 0 and mstat(hist=None, n_bins=0, hist_lo=99999, bin_width=-1) == 0
    assert mstat(hist_lo=-32768, bin_width=(1 << 31) - 1, n_bins=1) == 0 and mstat(hist_lo=32767, n_bins=bins) == 0
    assert (hist.pull()[2 * bins:] == PATTERN).all() and (mask.pull() == PATTERN).all()
    assert lstat() == 0
    raw = table.pull(np.uint32)
    assert (raw[REC * cap // 4:] == PATTERN).all()
    want = rs.label_records(vol, np.full(vol.shape, PATTERN, np.uint32), cap)
    assert raw[:REC * cap // 4].tobytes() == want.tobytes() == bytes(REC * cap)  # the pattern is a rank above the capacity
    for x in (huge, flat, odd_table, odd_labels, odd_hist, odd_mask, short_table, table, short_labels, labels, short_hist, hist, short_mask, mask,
              as_image, wrong_kind, volume):
        x.release()
