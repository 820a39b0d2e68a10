"""clwh_segment_grow and clwh_volume_apply_mask on the GPU against the contract's numpy restatement (tests/grow_ref.py): equal bytes
and equal integers, no tolerance anywhere.  Every family keeps a tally so that no comparison is empty."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import grow_ref as gr
from tests import mesh_ref as mr
from tests import projection_ref as pr
from tests.grow_ref import RANDOM_DIMS, WINDOWS, random_case, random_volume
from tests.test_gpu_mesh import check as check_mesh
from tests.view_helpers import ROOT, Proj, host_lib, image_of

pytestmark = pytest.mark.gpu

INVALID_VALUE, SIZE_MISMATCH = 1, 9
G26, FROM_MASK, DENSE = ffi.GROW_26, ffi.GROW_FROM_MASK, ffi.GROW_DENSE


class Tally:
    def __init__(self):
        self.calls = self.voxels = self.tiles = self.max_rounds = self.empty = self.padding_words = 0

    def add(self, region, rounds, words, dims):
        self.calls += 1
        self.voxels += int(region.sum())
        self.empty += not region.any()
        self.tiles = max(self.tiles, gr.tiles_spanned(region))
        self.max_rounds = max(self.max_rounds, rounds)
        self.padding_words += len(words) - (dims[0] + 31) // 32 * dims[1] * dims[2]


class Grower:
    """a volume on the device with a mask buffer of its size; every call checks mask and statistics against the reference"""

    def __init__(self, ctx, vol, tally=None):
        self.ctx, self.vol, self.tally = ctx, vol, tally if tally is not None else Tally()
        Z, Y, X = vol.shape
        self.dims = (X, Y, Z)
        self.volume, self.owner = image_of(ctx, vol)
        self.n_words = scene.mask_words_per_row(X) * Y * Z
        self.mask = ctx.buffer(4 * self.n_words, np.uint32, (self.n_words,))

    def raw(self, seeds, lo, hi, flags=0, box=None, prefill=0xFFFFFFFF):
        """(words, contract fields, rounds) as the device wrote them"""
        if prefill is not None:
            self.mask.push(np.full(self.n_words, prefill, np.uint32) if np.isscalar(prefill) else prefill)
        status, res = self.ctx.grow_region_raw(self.volume, seeds, lo, hi, flags, box, self.mask)
        assert status == 0, status
        return self.mask.pull(), res.as_dict(), int(res.rounds)

    def check(self, seeds, lo, hi, connectivity=6, box=None, from_mask=None, what=""):
        """reference == worklist == worklist again == dense; returns the reference's region"""
        want, _ = gr.grow(self.vol, seeds, lo, hi, connectivity, box, from_mask)
        words, stats = gr.packed(want), gr.stats(self.vol, want)
        flags = (G26 if connectivity == 26 else 0) | (FROM_MASK if from_mask is not None else 0)
        prefill = gr.packed(from_mask) if from_mask is not None else 0xFFFFFFFF  # without FROM_MASK: garbage on entry is ignored
        got = self.raw(seeds, lo, hi, flags, box, prefill)
        assert np.array_equal(scene.mask_unpack(got[0], self.dims), want), (what, int(want.sum()), int(scene.mask_unpack(got[0], self.dims).sum()))
        assert got[0].tobytes() == words.tobytes(), (what, "padding")
        assert got[1] == stats, (what, got[1], stats)
        again = self.raw(seeds, lo, hi, flags, box, prefill)
        assert again[0].tobytes() == words.tobytes() and again[1] == stats, (what, "again")
        dense = self.raw(seeds, lo, hi, flags | DENSE, box, prefill)
        assert dense[0].tobytes() == words.tobytes() and dense[1] == stats, (what, "dense")
        self.tally.add(want, got[2], got[0], self.dims)
        return want

    def release(self):
        for m in (self.mask, self.volume, self.owner):
            if m is not None:
                m.release()


@pytest.mark.parametrize("dims", RANDOM_DIMS)
def test_random_volumes_equal_the_reference_worklist_and_dense(gpu_ctx, dims):
    tally = Tally()
    for seed in range(3):
        g = Grower(gpu_ctx, random_volume(dims, seed), tally)
        for connectivity in (6, 26):
            vol, first, region, depth, n = random_case(dims, seed, connectivity)
            lo, hi = WINDOWS[connectivity]
            want = g.check([first], lo, hi, connectivity, what=(dims, seed, connectivity))
            assert np.array_equal(want, region)
        g.release()
    assert tally.calls == 6 and tally.voxels > 6 * 1500 and tally.tiles >= 5 and tally.max_rounds >= 2 and tally.empty == 0, vars(tally)


def test_ragged_volumes_and_padding(gpu_ctx):
    tally = Tally()
    for dims in ((130, 3, 7), (1, 1, 1), (64, 16, 16)):
        X, Y, Z = dims
        vol = np.random.default_rng(7).integers(0, 3, (Z, Y, X)).astype(np.int16)
        vol[0, 0, 0] = vol[-1, -1, -1] = 1
        g = Grower(gpu_ctx, vol, tally)
        for connectivity in (6, 26):
            for seeds in ([(0, 0, 0)], [(X - 1, Y - 1, Z - 1)], [(0, 0, 0), (X - 1, Y - 1, Z - 1)]):
                g.check(seeds, 1, 2, connectivity, what=(dims, connectivity, seeds))  # (the buffer is pre-filled with 0xFF)
        whole = g.check([(0, 0, 0)], 0, 2, 6, what=(dims, "everything"))
        assert whole.all()
        g.release()
    assert tally.calls == 21 and tally.padding_words > 0 and tally.voxels > 3000 and tally.empty == 0, vars(tally)


def test_serpentine_is_followed_to_its_end(gpu_ctx):
    vol = gr.serpentine()
    g = Grower(gpu_ctx, vol)
    for connectivity in (6, 26):
        region = g.check([(0, 0, 1)], 100, 100, connectivity, what=("serpentine", connectivity))
        assert int(region.sum()) == 2739
    words, stats, rounds = g.raw([(0, 0, 1)], 100, 100)
    assert stats["count"] == 2739 and stats["bbox_lo"] == (0, 0, 1) and stats["bbox_hi"] == (136, 39, 2) and stats["sum"] == 273900
    assert rounds >= 2 and g.tally.max_rounds >= 2 and g.tally.tiles == 9, vars(g.tally)
    # from the far end, and from the middle
    g.check([(0, 38, 1)], 100, 100, what="from the end")
    g.check([(70, 20, 1)], 100, 100, what="from the middle")
    g.release()


def test_connectivity_across_tile_borders(gpu_ctx):
    joined = 0
    for a, b in (((63, 15, 15), (64, 16, 16)),   # a corner across a tile corner
                 ((63, 15, 5), (64, 16, 5)),     # an edge across a tile edge along z
                 ((10, 15, 15), (10, 16, 16)),   # ... along x
                 ((63, 3, 15), (64, 3, 16)),     # ... along y
                 ((63, 15, 15), (64, 15, 15)), ((3, 15, 2), (3, 16, 2)), ((3, 2, 15), (3, 2, 16))):  # faces: both join
        vol = np.zeros((20, 20, 70), np.int16)
        vol[a[2], a[1], a[0]] = vol[b[2], b[1], b[0]] = 1
        g = Grower(gpu_ctx, vol)
        face = sum(abs(p - q) for p, q in zip(a, b)) == 1
        for seed in (a, b):
            assert g.check([seed], 1, 1, 6, what=(a, b, 6)).sum() == (2 if face else 1)
            assert g.check([seed], 1, 1, 26, what=(a, b, 26)).sum() == 2
            joined += 1
        g.release()
    assert joined == 14


def test_seed_lists(gpu_ctx):
    dims = (70, 40, 36)
    vol, first, region, _, _ = random_case(dims, 0, 6)
    lo, hi = WINDOWS[6]
    adm = gr.admissible(vol, lo, hi)
    lab = gr.labels(adm, 6)
    ids, counts = np.unique(lab[lab >= 0], return_counts=True)
    order = np.argsort(-counts, kind="stable")
    picks = [(int(i % 70), int(i // 70 % 40), int(i // 2800)) for i in ids[order[:4]]]  # the first voxels of the four largest components
    g = Grower(gpu_ctx, vol)
    union = g.check(picks, lo, hi, what="four components")
    assert np.array_equal(union, np.isin(lab, ids[order[:4]])) and union.sum() == counts[order[:4]].sum()
    outside = [tuple(int(v) for v in p[::-1]) for p in np.argwhere(~adm)[:3]]
    assert np.array_equal(g.check([first] + outside, lo, hi, what="a seed outside the window adds nothing"), region)
    empty = g.check(outside, lo, hi, what="no admissible seed")
    assert not empty.any()
    words, stats, rounds = g.raw(outside, lo, hi)
    assert stats == {"count": 0, "bbox_lo": (0, 0, 0), "bbox_hi": (0, 0, 0), "sum": 0, "sum_sq": 0, "vmin": 0, "vmax": 0} and not words.any()
    assert np.array_equal(g.check([first] * 5 + picks[1:2] * 3, lo, hi, what="duplicates"), np.isin(lab, [ids[order[0]], ids[order[1]]]))
    # 65536 seeds: every voxel of the first 65536 (admissible or not), duplicates to fill up
    flat = np.arange(65536) % vol.size
    many = np.stack([flat % 70, flat // 70 % 40, flat // 2800], axis=1)
    assert len(many) == ffi.GROW_MAX_SEEDS
    g.check(many, lo, hi, what="65536 seeds")
    g.check(many, *WINDOWS[26], connectivity=26, what="65536 seeds, 26")
    assert g.tally.calls == 6 and g.tally.empty == 1
    g.release()


def test_growth_from_the_mask(gpu_ctx):
    dims = (70, 40, 36)
    vol, first, _, _, _ = random_case(dims, 1, 6)
    g = Grower(gpu_ctx, vol)
    narrow = g.check([first], -1000, -400, what="narrow")
    # the device's own narrow mask stays in the buffer: continue from it without touching it
    g.raw([first], -1000, -400)
    status, res = gpu_ctx.grow_region_raw(g.volume, None, -1000, -280, FROM_MASK, None, g.mask)
    wide, _ = gr.grow(vol, None, -1000, -280, from_mask=narrow)
    assert status == 0 and g.mask.pull().tobytes() == gr.packed(wide).tobytes() and res.as_dict() == gr.stats(vol, wide)
    assert narrow.sum() < wide.sum()
    assert np.array_equal(g.check(None, -1000, -280, from_mask=narrow, what="wide from narrow"), wide)
    # a window that excludes earlier voxels clears them
    moved = g.check(None, -600, -280, from_mask=wide, what="moved window")
    assert (wide & ~moved).any() and not (moved & ~gr.admissible(vol, -600, -280)).any()
    # seeds and mask together, 26-connected; and garbage in the padding of the mask on entry does not survive
    g.check([first], *WINDOWS[26], connectivity=26, from_mask=narrow, what="seeds and mask")
    dirty = gr.packed(narrow).reshape(-1, scene.mask_words_per_row(70)).copy()
    dirty[:, 2] |= np.uint32(0xFFFFFFC0)  # x >= 70
    dirty[:, 3] = 0xFFFFFFFF
    got = g.raw(None, -1000, -280, FROM_MASK, None, dirty.reshape(-1))
    assert got[0].tobytes() == gr.packed(wide).tobytes() and got[1] == gr.stats(vol, wide)
    none = g.check(None, 500, 600, from_mask=wide, what="nothing admissible")
    assert not none.any() and g.tally.calls == 5
    g.release()


def test_boxes(gpu_ctx):
    vol = np.zeros((20, 36, 140), np.int16)
    vol[10, 18, :] = 100
    vol[3:17, 18, 70] = 100
    g = Grower(gpu_ctx, vol)
    whole = g.check([(5, 18, 10)], 100, 100, what="no box")
    assert whole.sum() == 140 + 13
    for box, count in ((((0, 0, 0), (0, 0, 0)), 153), (((0, 0, 0), (140, 36, 20)), 153),
                       (((0, 0, 0), (66, 36, 20)), 66),        # cuts the bar in two: the seed's side only
                       (((3, 18, 10), (131, 19, 11)), 128),    # one voxel thick, unaligned
                       (((6, 0, 0), (140, 36, 20)), 0),        # the seed lies outside the box
                       (((0, 0, 0), (0, 36, 20)), None), (((9, 9, 9), (9, 9, 9)), None), (((0, 36, 0), (140, 36, 20)), None)):  # empty boxes
        if count is None:
            assert box[1] != (0, 0, 0)
            words, stats, rounds = g.raw([(5, 18, 10)], 100, 100, 0, box)
            assert not words.any() and stats["count"] == 0 and stats["bbox_hi"] == (0, 0, 0) and rounds == 0
            continue
        region = g.check([(5, 18, 10)], 100, 100, box=box, what=box)
        assert region.sum() == count
    g.release()


def test_status_codes_and_nothing_written(gpu_ctx):
    ctx = gpu_ctx
    vol = random_volume((70, 12, 9), 3)
    volume = ctx.image_from(vol)
    n = scene.mask_words_per_row(70) * 12 * 9
    pattern = np.full(n + 4, 0xA5A5A5A5, np.uint32)
    mask = ctx.buffer_from(pattern)
    short = ctx.buffer_from(pattern[:n - 1])
    frame = ctx.image([64, 32], 4, np.uint8, (32, 64, 4))
    as_image = ctx.image([4, 4, n // 16 + 1], 1, np.uint32)
    odd = ctx.wrap(mask.device_ptr + 4, 4 * n)
    huge = ctx.image_wrap(volume.device_ptr, (1 << 31, 1, 1), 1, np.int16)  # never read: refused by its dims
    ok_seed = [(1, 2, 3)]

    def status(**kw):
        args = dict(volume=volume, seeds=ok_seed, lo=-1000, hi=0, flags=0, box=None, mask=mask)
        args.update(kw)
        st, res = ctx.grow_region_raw(**args)
        if st != 0:
            assert res.as_dict()["count"] == 0 and res.rounds == 0
        return st

    def untouched():
        return (mask.pull() == 0xA5A5A5A5).all() and (short.pull() == 0xA5A5A5A5).all()

    L = ffi.lib()
    d, res = ffi.GrowDesc(), ffi.GrowResult()
    seeds = np.array(ok_seed, np.uint32)
    d.volume, d.mask, d.lo, d.hi, d.n_seeds = volume.h, mask.h, -1000, 0, 1
    d.seeds = seeds.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.clwh_segment_grow(None, C.byref(d)) == INVALID_VALUE and L.clwh_segment_grow(ctx.h, None) == INVALID_VALUE
    assert L.clwh_segment_grow(ctx.h, C.byref(d)) == INVALID_VALUE  # result is NULL
    d.result = C.pointer(res)
    d.seeds = None
    assert L.clwh_segment_grow(ctx.h, C.byref(d)) == INVALID_VALUE  # n_seeds > 0 with NULL seeds
    assert untouched()
    assert status(volume=None) == INVALID_VALUE and status(volume=frame) == INVALID_VALUE and status(volume=mask) == INVALID_VALUE
    assert status(mask=None) == INVALID_VALUE and status(mask=as_image) == INVALID_VALUE and status(mask=volume) == INVALID_VALUE
    assert status(mask=odd) == INVALID_VALUE
    assert status(flags=8) == INVALID_VALUE and status(flags=-1) == INVALID_VALUE and status(flags=1 << 16) == INVALID_VALUE
    for lo, hi in ((1, 0), (-32769, 0), (0, 32768), (-40000, 40000)):
        assert status(lo=lo, hi=hi) == INVALID_VALUE, (lo, hi)
    for box in (((0, 0, 0), (71, 12, 9)), ((0, 0, 0), (70, 13, 9)), ((0, 0, 0), (70, 12, 10)), ((5, 0, 0), (4, 12, 9)), ((0, 0, 3), (70, 12, 2)),
                ((71, 0, 0), (0, 0, 0)), ((0, 0, 0), (0, 0, 1 << 31))):
        assert status(box=box) == INVALID_VALUE, box
    assert status(seeds=np.zeros((65537, 3), np.uint32)) == INVALID_VALUE
    assert status(seeds=None) == INVALID_VALUE and status(seeds=np.zeros((0, 3), np.uint32)) == INVALID_VALUE  # no seeds, no FROM_MASK
    for bad in ((70, 0, 0), (0, 12, 0), (0, 0, 9), (0xFFFFFFFF, 0, 0)):
        assert status(seeds=[ok_seed[0], bad]) == INVALID_VALUE, bad
    assert status(volume=huge) == INVALID_VALUE
    assert status(mask=short) == SIZE_MISMATCH and status(mask=short, flags=FROM_MASK, seeds=None) == SIZE_MISMATCH
    assert status(mask=short, flags=8) == INVALID_VALUE  # INVALID_VALUE before SIZE_MISMATCH
    assert untouched()
    # and the same arguments without the defect are accepted: limits included
    assert status(lo=-32768, hi=32767) == 0 and status(flags=7) == 0 and status(box=((70, 12, 9), (70, 12, 9))) == 0
    assert status(seeds=np.zeros((65536, 3), np.uint32)) == 0 and status(seeds=None, flags=FROM_MASK) == 0
    got = mask.pull()
    assert (got[n:] == 0xA5A5A5A5).all()  # nothing behind the layout's words is written
    want, _ = gr.grow(vol, ok_seed, -1000, 0)
    assert status() == 0 and mask.pull()[:n].tobytes() == gr.packed(want).tobytes()
    for m in (huge, odd, as_image, frame, short, mask, volume):
        m.release()


RAGGED = ((130, 3, 7), (1, 1, 1), (64, 16, 16), (72, 5, 4))


def test_apply_mask_keep_and_invert(gpu_ctx):
    ctx = gpu_ctx
    n = 0
    for dims in RAGGED:
        X, Y, Z = dims
        rng = np.random.default_rng(X)
        vol = rng.integers(-32768, 32768, (Z, Y, X)).astype(np.int16)
        region = rng.random((Z, Y, X)) < 0.5
        words = gr.packed(region)
        words.reshape(-1, scene.mask_words_per_row(X))[:, -1] |= np.uint32(0x80000000 if X % 64 else 0)  # padding bits are not voxels
        mask = ctx.buffer_from(words)
        volume, owner = image_of(ctx, vol)
        out, out_owner = image_of(ctx, np.full_like(vol, 77))
        for fill, invert in ((-32768, False), (123, True), (32767, False), (0, True)):
            want = gr.apply_mask(vol, region, fill, invert)
            assert ctx.apply_mask_raw(volume, mask, out, fill, ffi.MASK_INVERT if invert else 0) == 0
            assert np.array_equal((out_owner or out).pull(np.int16, vol.shape), want), (dims, fill, invert, "out of place")
            assert np.array_equal((owner or volume).pull(np.int16, vol.shape), vol)  # the input is only read
            n += 1
        ctx.apply_mask(volume, mask, fill=-5, invert=True)  # in place
        assert np.array_equal((owner or volume).pull(np.int16, vol.shape), gr.apply_mask(vol, region, -5, True)), (dims, "in place")
        for m in (out, out_owner, volume, owner, mask):
            if m is not None:
                m.release()
    assert n == 16


def test_apply_mask_is_seen_by_the_views(gpu_ctx):
    """after an in-place apply the projections (dense and skipping) show the masked array: without the version bump the bricked copy
    of the old content would answer.  The same through a second handle of the same pointer."""
    ctx = gpu_ctx
    X, Y, Z = 24, 16, 40
    a = scene.phantom(40, dims=(X, Y, Z))
    pos, d = scene.default_camera(40)
    volume = ctx.image_from(a)
    p = Proj(ctx, (64, 48), (64, 48))
    want = lambda v: pr.project(v, pos, d, (64, 48), (64, 48))[pr.MAX]
    Proj.check(p.run(volume, pos, d, pr.MAX), want(a), "before")  # the derived copy of the unmasked content exists now
    g = Grower(ctx, a)
    region = g.check([(12, 8, 3)], -1100, -900, what="air")  # the air around the ball, from a voxel on the z = 3 slice's centre line
    assert 1000 < region.sum() < a.size
    g.raw([(12, 8, 3)], -1100, -900)
    masked = gr.apply_mask(a, region, 2000, True)  # the air becomes the brightest value: every pixel changes
    ctx.apply_mask(volume, g.mask, fill=2000, invert=True)
    assert not np.array_equal(want(masked)[0], want(a)[0])
    for dense in (False, True):
        Proj.check(p.run(volume, pos, d, pr.MAX, dense=dense), want(masked), "after the apply, dense=%s" % dense)
    # through a wrap: the mask applied with volume_out = another handle of the same pointer
    alias = ctx.image_wrap(volume.device_ptr, (X, Y, Z), 1, np.int16)
    Proj.check(p.run(alias, pos, d, pr.MAX), want(masked), "through the wrap")
    twice = gr.apply_mask(masked, region, -1000, True)
    assert ctx.apply_mask_raw(volume, g.mask, alias, -1000, ffi.MASK_INVERT) == 0
    for through in (volume, alias):
        for dense in (False, True):
            Proj.check(p.run(through, pos, d, pr.MAX, dense=dense), want(twice), "after the apply through the wrap")
    assert np.array_equal(volume.pull(), twice)
    ctx.finish()
    for m in (alias, volume):
        m.release()
    p.release()
    g.release()


def test_apply_mask_status_codes(gpu_ctx):
    ctx = gpu_ctx
    vol = random_volume((70, 12, 9), 4)
    volume, other = ctx.image_from(vol), ctx.image_from(vol[:, :, :69].copy())
    n = scene.mask_words_per_row(70) * 12 * 9
    mask = ctx.buffer_from(np.zeros(n, np.uint32))
    short = ctx.buffer(4 * n - 4, np.uint32)
    frame = ctx.image([64, 32], 4, np.uint8, (32, 64, 4))
    odd = ctx.wrap(mask.device_ptr + 4, 4 * n)
    huge = ctx.image_wrap(volume.device_ptr, (1 << 31, 1, 1), 1, np.int16)

    def status(**kw):
        args = dict(volume_in=volume, mask=mask, volume_out=volume, fill=0, flags=0)
        args.update(kw)
        return ctx.apply_mask_raw(**args)

    L = ffi.lib()
    d = ffi.ApplyMaskDesc()
    d.volume_in = d.volume_out = volume.h
    d.mask = mask.h
    assert L.clwh_volume_apply_mask(None, C.byref(d)) == INVALID_VALUE and L.clwh_volume_apply_mask(ctx.h, None) == INVALID_VALUE
    assert status(volume_in=None) == INVALID_VALUE and status(volume_out=None) == INVALID_VALUE
    assert status(volume_in=frame) == INVALID_VALUE and status(volume_out=mask) == INVALID_VALUE
    assert status(mask=None) == INVALID_VALUE and status(mask=volume) == INVALID_VALUE and status(mask=odd) == INVALID_VALUE
    assert status(flags=2) == INVALID_VALUE and status(flags=-1) == INVALID_VALUE
    assert status(fill=32768) == INVALID_VALUE and status(fill=-32769) == INVALID_VALUE
    assert status(volume_in=huge, volume_out=huge) == INVALID_VALUE
    assert status(volume_out=other) == SIZE_MISMATCH and status(volume_in=other) == SIZE_MISMATCH
    assert status(mask=short) == SIZE_MISMATCH and status(mask=short, flags=2) == INVALID_VALUE
    assert np.array_equal(volume.pull(), vol)  # nothing was written
    assert status(fill=32767, flags=1) == 0 and status(fill=-32768) == 0
    assert (volume.pull() == -32768).all()  # an empty mask keeps nothing
    for m in (huge, odd, frame, short, mask, other, volume):
        m.release()


def _bone_seed(vol):
    """the first voxel of the phantom's bone shell on the central slice, picked from the reference's admissible image"""
    adm = gr.admissible(vol, 500, 1200)
    z = vol.shape[0] // 2
    y, x = np.argwhere(adm[z])[0]
    return int(x), int(y), int(z)


def test_phantom_end_to_end_mesh_of_the_grown_bone(gpu_ctx):
    ctx = gpu_ctx
    vol = scene.phantom(96)
    seed = _bone_seed(vol)
    g = Grower(ctx, vol)
    region = g.check([seed], 500, 1200, what="bone")
    assert region.sum() > 20000 and g.tally.tiles > 16  # (half of the shell: the slab cuts it in two)
    g.raw([seed], 500, 1200)
    ctx.apply_mask(g.volume, g.mask, fill=-32768)
    masked = gr.apply_mask(vol, region)
    assert np.array_equal(g.volume.pull(), masked)
    pos, nrm, tri, keys = ctx.mesh_isosurface(g.volume, 500.0, normals=True, keys=True)
    want = mr.mesh(masked, 500.0)
    assert len(want.keys) > 30000
    check_mesh((keys, pos.view(np.uint32), nrm.view(np.uint32), tri), want, "mesh of the masked phantom")
    g.release()


def test_host_mirror_grows_and_applies(tmp_path):
    n = 48
    vol = scene.phantom(n)
    env = scene.env_map(64, 32)
    L = host_lib(clvr_host_grow_region=(None, [C.c_void_p, C.POINTER(C.c_uint), C.c_uint, C.c_int, C.c_int, C.c_int, C.POINTER(ffi.GrowResult)]),
                 clvr_host_apply_mask=(None, [C.c_void_p, C.c_int, C.c_int]),
                 clvr_host_extract_mesh=(None, [C.c_void_p, C.c_float, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong),
                                                C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_float)),
                                                C.POINTER(C.POINTER(C.c_ulonglong)), C.POINTER(C.POINTER(C.c_uint))]))
    h = L.clvr_host_create()
    try:
        L.clvr_host_load(h, vol.ctypes.data, n, n, n, env.ctypes.data, 64, 32)
        seed = _bone_seed(vol)
        res = ffi.GrowResult()
        L.clvr_host_grow_region(h, (C.c_uint * 3)(*seed), 1, 500, 1200, 0, C.byref(res))
        region, _ = gr.grow(vol, [seed], 500, 1200)
        assert res.as_dict() == gr.stats(vol, region) and res.count > 2000
        L.clvr_host_apply_mask(h, -32768, 0)
        nv, nt = C.c_ulonglong(0), C.c_ulonglong(0)
        p, q = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
        k, t = C.POINTER(C.c_ulonglong)(), C.POINTER(C.c_uint)()
        L.clvr_host_extract_mesh(h, 500.0, 0, C.byref(nv), C.byref(nt), C.byref(p), C.byref(q), C.byref(k), C.byref(t))
        want = mr.mesh(gr.apply_mask(vol, region), 500.0)
        assert (nv.value, nt.value) == (len(want.keys), len(want.tris)) and nv.value > 5000
    finally:
        L.clvr_host_destroy(h)


def test_headless_grow_then_mesh(tmp_path):
    n = 48
    vol = scene.phantom(n)
    scene.write_nrrd(str(tmp_path / "v.nrrd"), vol)
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(np.random.default_rng(5).random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    seed = _bone_seed(vol)
    files = [str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", "64", "64"]
    out = subprocess.run([exe, "--grow=%d,%d,%d,500,1200" % seed, "--mesh=500"] + files + [str(tmp_path / "m.ply")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(s) for s in out.stdout.strip().splitlines() if s.startswith("{")]
    region, _ = gr.grow(vol, [seed], 500, 1200)
    stats = gr.stats(vol, region)
    grow = lines[0]
    assert grow["count"] == stats["count"] > 2000 and tuple(grow["bbox_lo"]) == stats["bbox_lo"] and tuple(grow["bbox_hi"]) == stats["bbox_hi"]
    assert (grow["min"], grow["max"]) == (stats["vmin"], stats["vmax"]) and abs(grow["mean"] - stats["sum"] / stats["count"]) < 1e-5
    assert (grow["connectivity"], grow["mode"], grow["fill"]) == (6, "keep", -32768)
    want = mr.mesh(gr.apply_mask(vol, region), 500.0)
    assert (lines[-1]["vertices"], lines[-1]["triangles"]) == (len(want.keys), len(want.tris))
    pos, nrm, tri = scene.read_ply(str(tmp_path / "m.ply"))
    rows = lambda p, q: np.sort(np.ascontiguousarray(np.concatenate([p, q], axis=1)).view([("", np.uint32)] * 6).reshape(-1))
    assert np.array_equal(rows(pos.view(np.uint32), nrm.view(np.uint32)), rows(want.pos, want.nrm))
    _, ids = np.unique(np.concatenate([pos.view(np.uint32), want.pos]), axis=0, return_inverse=True)
    ids = ids.reshape(-1)
    assert np.array_equal(mr.canonical(ids[:len(pos)][tri]), mr.canonical(ids[len(pos):][mr.index_triangles(want)]))
    # remove, 26-connected, with a fill of its own, in front of a view: the region's voxels become the fill
    out = subprocess.run([exe, "--grow=%d,%d,%d,500,1200,26,remove,fill=-1000" % seed, "--projection=max"] + files, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(s) for s in out.stdout.strip().splitlines() if s.startswith("{")]
    region26, _ = gr.grow(vol, [seed], 500, 1200, 26)
    assert lines[0]["count"] == int(region26.sum()) and (lines[0]["connectivity"], lines[0]["mode"], lines[0]["fill"]) == (26, "remove", -1000)
    assert lines[-1]["projection"] == "max"
    for bad in ("--grow=1,2,3,500", "--grow=1,2,3,500,1200,18", "--grow=1,2,3,1200,500", "--grow=1,2,3,500,1200,", "--grow=999,2,3,500,1200", "--grow"):
        assert subprocess.run([exe, bad] + files, capture_output=True, text=True, timeout=120).returncode == 1, bad
