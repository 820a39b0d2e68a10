"""clwh_mask_distance, clwh_mask_morph and clwh_mask_combine on the GPU against the contract's numpy restatement
(tests/distance_ref.py): equal bytes of maps and masks, no tolerance anywhere, every case twice.  A map is allocated four words too
long and pre-filled with a pattern that must survive behind X * Y * Z; masks that are outputs are pre-filled with 0xA5 bytes."""
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
from tests import mesh_ref as mr
from tests.grow_ref import RANDOM_DIMS
from tests.view_helpers import ROOT, host_lib

pytestmark = pytest.mark.gpu

INVALID_VALUE, SIZE_MISMATCH = 1, 9
NONE = dr.NONE
PATTERN = 0xA5A5A5A5
WEIGHTS = ((1, 1, 1), (4, 9, 1), (49, 49, 625))
MORPH_OPS = (dr.DILATE, dr.ERODE, dr.OPEN, dr.CLOSE)
MASK_OPS = (dr.AND, dr.OR, dr.XOR, dr.ANDNOT, dr.NOT)


def dims_of(mask):
    Z, Y, X = mask.shape
    return X, Y, Z


def garbage(mask):
    """the mask's words with every bit at x >= X and every padding word set"""
    Z, Y, X = mask.shape
    wpr = scene.mask_words_per_row(X)
    padded = np.ones((Z, Y, wpr * 32), np.uint8)
    padded[:, :, :X] = mask
    return np.packbits(padded, axis=2, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


class Device:
    """the three calls on one context, each made twice ("first", "again") with pre-filled outputs; every check is of equal bytes"""

    def __init__(self, ctx):
        self.ctx = ctx

    def distance(self, words, dims, w=(1, 1, 1), to_clear=False, cap=None):
        """the map as the device wrote it, uint32 [z][y][x]"""
        X, Y, Z = dims
        n = X * Y * Z
        mask = self.ctx.buffer_from(words)
        dist = self.ctx.buffer(4 * (n + 4), np.uint32, (n + 4,))
        out = None
        for turn in ("first", "again"):
            dist.push(np.full(n + 4, PATTERN, np.uint32))
            status = self.ctx.mask_distance_raw(mask, dist, dims, w, NONE if cap is None else cap, ffi.DIST_TO_CLEAR if to_clear else 0)
            assert status == 0, (status, dims, w, turn)
            got = dist.pull()
            assert (got[n:] == PATTERN).all(), (dims, w, turn, "written behind X * Y * Z")
            assert out is None or np.array_equal(out, got[:n]), (dims, w, turn)
            out = got[:n].copy()
        assert np.array_equal(mask.pull(), words)  # read only
        mask.release()
        dist.release()
        return out.reshape(Z, Y, X)

    def morph(self, words, dims, op, radius_sq, w=(1, 1, 1), in_place=False):
        """the mask's words as the device wrote them"""
        n = len(words)
        out = None
        for turn in ("first", "again"):
            mask_in = self.ctx.buffer_from(words)
            mask_out = mask_in if in_place else self.ctx.buffer_from(np.full(n, PATTERN, np.uint32))
            status = self.ctx.mask_morph_raw(mask_in, mask_out, dims, op, radius_sq, w)
            assert status == 0, (status, dims, op, radius_sq, w, turn)
            got = mask_out.pull()
            assert in_place or np.array_equal(mask_in.pull(), words)
            assert out is None or np.array_equal(out, got), (dims, op, radius_sq, w, turn)
            out = got
            mask_in.release()
            if not in_place:
                mask_out.release()
        return out

    def combine(self, a_words, b_words, dims, op, out="fresh"):
        n = len(a_words)
        res = None
        for turn in ("first", "again"):
            a = self.ctx.buffer_from(a_words)
            b = self.ctx.buffer_from(b_words) if b_words is not None else None
            o = {"fresh": None, "a": a, "b": b}[out] or self.ctx.buffer_from(np.full(n, PATTERN, np.uint32))
            status = self.ctx.mask_combine_raw(a, b, o, dims, op)
            assert status == 0, (status, dims, op, out, turn)
            got = o.pull()
            assert res is None or np.array_equal(res, got)
            res = got
            for m in {id(m): m for m in (a, b, o) if m is not None}.values():
                m.release()
        return res


def same(got, want, what):
    assert got.dtype == want.dtype and np.array_equal(got, want), (what, int((got != want).sum()), np.argwhere(got != want)[:3].tolist())


# ---- 1. random masks
# the generator's seed per shape: one whose sparsest mask leaves most of the volume far from every site (asserted below, from the
# reference alone); at 0.0005 the expected mask fills its volume with balls of 8 voxels a little too well
SEED = {(65, 17, 17): 4, (70, 40, 36): 8, (33, 40, 35): 15, (129, 33, 18): 5}


@pytest.mark.parametrize("dims", RANDOM_DIMS)
def test_random_masks_equal_the_reference(gpu_ctx, dims):
    dev = Device(gpu_ctx)
    for density in (0.0005, 0.02, 0.5):
        sites = dr.random_mask(dims, density, SEED[dims])
        for w in WEIGHTS:
            want = dr.random_distance(dims, density, SEED[dims], w, False)
            if density == 0.0005:  # the search must leave a site's neighbourhood: most voxels are far from every site
                assert int((want.astype(np.int64) > 64 * min(w)).sum()) * 2 > want.size, (dims, w)
            for to_clear in (False, True):  # the sites are the set voxels of `sites`, or the clear voxels of its complement
                words = scene.mask_pack(~sites if to_clear else sites)
                same(dev.distance(words, dims, w, to_clear), want, (dims, density, w, to_clear))


# ---- 2. extremes
@pytest.mark.parametrize("dims", ((1, 1, 1), (7, 1, 1), (63, 3, 2), (64, 3, 2), (65, 3, 2)))
def test_empty_and_full_masks(gpu_ctx, dims):
    dev = Device(gpu_ctx)
    X, Y, Z = dims
    empty, full = np.zeros((Z, Y, X), bool), np.ones((Z, Y, X), bool)
    for w in ((1, 1, 1), (49, 49, 625)):
        assert (dev.distance(scene.mask_pack(empty), dims, w) == NONE).all()
        assert (dev.distance(scene.mask_pack(full), dims, w) == 0).all()
        assert (dev.distance(scene.mask_pack(full), dims, w, to_clear=True) == NONE).all()
        assert (dev.distance(scene.mask_pack(empty), dims, w, to_clear=True) == 0).all()
        one = empty.copy()
        one[Z - 1, Y // 2, X // 2] = True
        same(dev.distance(scene.mask_pack(one), dims, w), dr.distance(one, w), (dims, w, "one voxel"))


def test_one_voxel_in_each_corner(gpu_ctx):
    dev = Device(gpu_ctx)
    dims = X, Y, Z = (65, 17, 9)
    for w in ((1, 1, 1), (4, 9, 1)):
        weight_sum = w[0] * (X - 1) ** 2 + w[1] * (Y - 1) ** 2 + w[2] * (Z - 1) ** 2
        for corner in range(8):
            x, y, z = ((X - 1) * (corner & 1), (Y - 1) * (corner >> 1 & 1), (Z - 1) * (corner >> 2))
            m = np.zeros((Z, Y, X), bool)
            m[z, y, x] = True
            got = dev.distance(scene.mask_pack(m), dims, w)
            same(got, dr.distance(m, w), (corner, w))
            assert int(got.max()) == int(got[Z - 1 - z, Y - 1 - y, X - 1 - x]) == weight_sum


# ---- 3. lines longer than any tile
@pytest.mark.parametrize("dims", ((1100, 2, 3), (3, 1100, 2), (2, 3, 1100)))
def test_long_lines(gpu_ctx, dims):
    dev = Device(gpu_ctx)
    X, Y, Z = dims
    axis = dims.index(1100)
    for ends in ((0,), (1099,), (0, 1099)):
        m = np.zeros((Z, Y, X), bool)
        for e in ends:
            at = [1, 1, 1]
            at[axis] = e
            m[at[2] % Z, at[1] % Y, at[0] % X] = True
        for w in ((1, 1, 1), (3, 3, 3)):
            want = dr.distance(m, w)
            assert int(want.max()) >= w[0] * 549 ** 2
            same(dev.distance(scene.mask_pack(m), dims, w), want, (dims, ends, w))
            same(dev.distance(scene.mask_pack(~m), dims, w, to_clear=True), want, (dims, ends, w, "to clear"))
            for cap in (300 * 300, 20 * 20):  # a cap that cuts, far and near (the passes may differ with its reach)
                capped = np.where(want <= cap, want, np.uint32(NONE)).astype(np.uint32)
                assert (capped == NONE).any() and (capped != NONE).any()
                same(dev.distance(scene.mask_pack(m), dims, w, cap=cap), capped, (dims, ends, w, cap))
    # and a morphology along it: the capped passes stop early, the result is the ball's
    got = dev.morph(scene.mask_pack(m), dims, dr.DILATE, 100 * 100, (1, 1, 1))
    same(got, scene.mask_pack(dr.morph(m, (1, 1, 1), dr.DILATE, 100 * 100)), (dims, "dilate by 100"))


# ---- 4. the arithmetic's edge
def test_largest_finite_value_is_not_none(gpu_ctx):
    dev = Device(gpu_ctx)
    dims, w = (2, 2, 2), (2147483647, 2147483646, 1)
    m = np.zeros((2, 2, 2), bool)
    m[0, 0, 0] = True
    got = dev.distance(scene.mask_pack(m), dims, w)
    same(got, dr.distance(m, w), "the edge")
    assert int(got[1, 1, 1]) == 2 ** 32 - 2 != NONE and int(got[0, 1, 1]) == 2 ** 32 - 3
    same(dev.distance(scene.mask_pack(m), dims, w, cap=2 ** 32 - 2), got, "cap at the largest value")
    assert int(dev.distance(scene.mask_pack(m), dims, w, cap=2 ** 32 - 3)[1, 1, 1]) == NONE
    for op in (dr.DILATE, dr.CLOSE):  # NONE as a radius: every finite distance is inside
        assert dev.morph(scene.mask_pack(m), dims, op, NONE, w).tolist() == [3, 0, 3, 0, 3, 0, 3, 0]
    assert not dev.morph(scene.mask_pack(np.zeros((2, 2, 2), bool)), dims, dr.DILATE, NONE, w).any()  # ... and no site is outside
    mask = gpu_ctx.buffer_from(scene.mask_pack(m))
    dist = gpu_ctx.buffer_from(np.full(8, PATTERN, np.uint32))
    for k in range(3):
        more = list(w)
        more[k] += 1
        assert gpu_ctx.mask_distance_raw(mask, dist, dims, more) == INVALID_VALUE
        assert gpu_ctx.mask_morph_raw(mask, mask, dims, dr.DILATE, 1, more) == INVALID_VALUE
    assert (dist.pull() == PATTERN).all()
    mask.release()
    dist.release()


# ---- 5. garbage outside the volume
@pytest.mark.parametrize("X", (65, 33))
def test_garbage_outside_the_volume_is_ignored(gpu_ctx, X):
    dev = Device(gpu_ctx)
    dims = (X, 9, 5)
    a, b = dr.random_mask(dims, 0.05, 21), dr.random_mask(dims, 0.4, 22)
    ga, gb = garbage(a), garbage(b)
    assert not np.array_equal(ga, scene.mask_pack(a)) and np.array_equal(scene.mask_unpack(ga, dims), a)
    for w in ((1, 1, 1), (4, 9, 1)):
        for to_clear in (False, True):
            same(dev.distance(ga, dims, w, to_clear), dr.distance(a, w, to_clear), (X, w, to_clear))
        for op in MORPH_OPS:
            for in_place in (False, True):
                same(dev.morph(ga, dims, op, 5, w, in_place), scene.mask_pack(dr.morph(a, w, op, 5)), (X, w, op, in_place))
    for op in MASK_OPS:
        for out in ("fresh", "a") + (("b",) if op != dr.NOT else ()):
            same(dev.combine(ga, gb, dims, op, out), scene.mask_pack(dr.combine(a, b, op)), (X, op, out))
    same(dev.combine(ga, None, dims, dr.NOT), scene.mask_pack(~a), (X, "NOT without b"))


# ---- 6. cap
def test_cap(gpu_ctx):
    dev = Device(gpu_ctx)
    dims = (70, 40, 36)
    for density, to_clear in ((0.02, False), (0.0005, False), (0.02, True)):
        sites = dr.random_mask(dims, density, 11)
        full = dr.random_distance(dims, density, 11, (1, 1, 1), False)
        words = scene.mask_pack(~sites if to_clear else sites)
        for cap in (0, 1, 8, 9, 1000, NONE):
            want = np.where(full <= np.uint32(cap), full, np.uint32(NONE)).astype(np.uint32)
            same(dev.distance(words, dims, (1, 1, 1), to_clear, cap), want, (density, to_clear, cap))
        assert (full < NONE).all() and (full > 9).any() and (full <= 8).any()  # the small caps cut, the large ones need not


# ---- 7. morphology
def bridged_blocks():
    """70 x 20 x 12: two blocks joined by a bridge one voxel thick, five pinholes in the blocks"""
    m = np.zeros((12, 20, 70), bool)
    m[2:10, 3:17, 3:30] = True
    m[2:10, 3:17, 40:67] = True
    m[6, 10, 30:40] = True
    for x, y, z in ((10, 8, 5), (20, 12, 7), (50, 6, 4), (60, 14, 8), (45, 10, 6)):
        m[z, y, x] = False
    return m


def components(mask):
    return lr.label_admissible(mask, 6)[2]["n_components"]


@pytest.mark.parametrize("w", ((1, 1, 1), (1, 1, 6)))
@pytest.mark.parametrize("shape", ("random", "bridged"))
def test_morphology_equals_the_reference(gpu_ctx, shape, w):
    dev = Device(gpu_ctx)
    m = dr.random_mask((65, 17, 17), 0.3, 31) if shape == "random" else bridged_blocks()
    dims = dims_of(m)
    words = scene.mask_pack(m)
    changed = 0
    for op in MORPH_OPS:
        for radius_sq in (0, 1, 2, 3, 9, 50):
            want = dr.morph(m, w, op, radius_sq)
            assert radius_sq > 0 or np.array_equal(want, m)
            changed += not np.array_equal(want, m)
            for in_place in (False, True):
                same(dev.morph(words, dims, op, radius_sq, w, in_place), scene.mask_pack(want), (shape, w, op, radius_sq, in_place))
    assert changed >= 18  # every op changes the mask at nearly every radius above 0
    if shape == "bridged":
        holes = ~m & np.pad(m, 1)[2:, 1:-1, 1:-1] & np.pad(m, 1)[:-2, 1:-1, 1:-1]  # clear with a set voxel above and below: the pinholes
        assert components(m) == 1 and int(holes.sum()) == 5
        for radius_sq in (1, 2, 3):
            opened, closed = dr.morph(m, w, dr.OPEN, radius_sq), dr.morph(m, w, dr.CLOSE, radius_sq)
            assert components(opened) == 2 and not opened[6, 10, 31:39].any()  # the bridge goes (but for its feet), two blocks stay
            assert closed[holes].all() and closed[6, 10, 30:40].all()  # the pinholes are filled, the bridge stays


# ---- 8. combine
@pytest.mark.parametrize("X", (31, 64, 65))
def test_combine(gpu_ctx, X):
    dev = Device(gpu_ctx)
    dims = (X, 7, 5)
    a, b = dr.random_mask(dims, 0.5, 41), dr.random_mask(dims, 0.3, 42)
    wa, wb = scene.mask_pack(a), scene.mask_pack(b)
    results = set()
    for op in MASK_OPS:
        want = scene.mask_pack(dr.combine(a, b, op))
        results.add(want.tobytes())
        for out in ("fresh", "a", "b"):
            same(dev.combine(wa, wb, dims, op, out), want, (X, op, out))
    assert len(results) == 5


# ---- 9. status
def test_status_codes_and_nothing_written(gpu_ctx):
    ctx = gpu_ctx
    dims = X, Y, Z = (70, 12, 9)
    n, words = X * Y * Z, scene.mask_words_per_row(X) * Y * Z
    fill = lambda k: ctx.buffer_from(np.full(k, PATTERN, np.uint32))
    mask, mask2, out, short_mask = fill(words), fill(words), fill(words), fill(words - 1)
    dist, short_dist = fill(n + 4), fill(n - 1)
    as_image = ctx.image([4, 4, n // 16 + 1], 1, np.uint32)
    odd_mask = ctx.wrap(mask.device_ptr + 4, 4 * words - 4)
    odd_dist = ctx.wrap(dist.device_ptr + 2, 4 * n)
    bad_dims = ((0, 12, 9), (70, 0, 9), (70, 12, 0), (1 << 31, 1, 1), (1 << 16, 1 << 15, 1))
    bad_weights = ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1 << 20, 1, 1), (1, 1 << 26, 1), (1, 1, 1 << 27), (903000, 1, 1))
    assert dr.weights_ok(dims, (901000, 1, 1)) and not any(dr.weights_ok(dims, w) for w in bad_weights)

    def distance(**kw):
        args = dict(mask=mask, dist=dist, dims=dims, weights=(1, 1, 1), cap=NONE, flags=0)
        args.update(kw)
        return ctx.mask_distance_raw(**args)

    def morph(**kw):
        args = dict(mask_in=mask, mask_out=out, dims=dims, op=dr.DILATE, radius_sq=4, weights=(1, 1, 1), flags=0)
        args.update(kw)
        return ctx.mask_morph_raw(**args)

    def combine(**kw):
        args = dict(a=mask, b=mask2, out=out, dims=dims, op=dr.AND)
        args.update(kw)
        return ctx.mask_combine_raw(**args)

    L = ffi.lib()
    for name, desc in (("clwh_mask_distance", ffi.DistanceDesc()), ("clwh_mask_morph", ffi.MorphDesc()), ("clwh_mask_combine", ffi.MaskCombineDesc())):
        assert getattr(L, name)(None, C.byref(desc)) == INVALID_VALUE and getattr(L, name)(ctx.h, None) == INVALID_VALUE
    cases = []
    for bad in (None, as_image, odd_mask):
        cases += [distance(mask=bad), morph(mask_in=bad), morph(mask_out=bad), combine(a=bad), combine(b=bad), combine(out=bad)]
    cases += [distance(dist=None), distance(dist=as_image), distance(dist=odd_dist)]
    cases += [distance(flags=2), distance(flags=-1), distance(flags=1 << 16), morph(flags=1), morph(flags=-1)]
    cases += [morph(op=-1), morph(op=4), combine(op=-1), combine(op=5)]
    for bad in bad_dims:
        cases += [distance(dims=bad), morph(dims=bad), combine(dims=bad)]
    for bad in bad_weights:
        cases += [distance(weights=bad), morph(weights=bad)]
    assert cases == [INVALID_VALUE] * len(cases), cases
    sizes = [distance(mask=short_mask), distance(dist=short_dist), morph(mask_in=short_mask), morph(mask_out=short_mask),
             combine(a=short_mask), combine(b=short_mask), combine(out=short_mask)]
    assert sizes == [SIZE_MISMATCH] * len(sizes), sizes
    # INVALID_VALUE before SIZE_MISMATCH
    assert distance(dist=short_dist, weights=(0, 1, 1)) == INVALID_VALUE and distance(mask=short_mask, flags=2) == INVALID_VALUE
    assert morph(mask_out=short_mask, op=4) == INVALID_VALUE and combine(out=short_mask, op=5) == INVALID_VALUE
    for m in (mask, mask2, out, short_mask, dist, short_dist):
        assert (m.pull(np.uint32, (m.nbytes // 4,)) == PATTERN).all()  # nothing was written
    # and the same arguments without the defect are accepted, limits included
    assert distance() == 0 and distance(weights=(901000, 1, 1), cap=0, flags=1) == 0 and morph(op=3, radius_sq=NONE) == 0
    assert combine(op=dr.NOT, b=None) == 0 and combine(op=dr.NOT, b=as_image) == 0 and combine() == 0
    assert (dist.pull()[n:] == PATTERN).all() and (mask.pull() == PATTERN).all()
    m = scene.mask_unpack(np.full(words, PATTERN, np.uint32), dims)
    same(out.pull(), scene.mask_pack(m), "a AND a of the pattern, padding clean")
    for x in (odd_dist, odd_mask, as_image, short_dist, dist, short_mask, out, mask2, mask):
        x.release()


# ---- 10. the chain: the grown bone's margin of 2 voxels (voxels of 1 x 1 x 2.5), without the bone
SIZES = (1.0, 1.0, 2.5)
MARGIN = 2.0


def _bone_seed(vol):
    adm = gr.admissible(vol, 500, 1200)
    z = vol.shape[0] // 2
    y, x = np.argwhere(adm[z])[0]
    return int(x), int(y), int(z)


def _chain_reference():
    vol = scene.phantom(48)
    seed = _bone_seed(vol)
    bone, _ = gr.grow(vol, [seed], 500, 1200)
    w, r2 = scene.mask_weights(SIZES), scene.radius_sq(MARGIN)
    assert (w, r2) == ((256, 256, 1600), 1024)
    grown = dr.morph(bone, w, dr.DILATE, r2)
    margin = dr.combine(grown, bone, dr.ANDNOT)
    assert 1000 < bone.sum() < margin.sum() and not (margin & bone).any()
    assert w[2] > r2 > 3 * w[0]  # 2.5 > 2: the ball has no neighbour along z, and more than the 26 in the plane
    return vol, seed, bone, grown, margin


def test_chain_grow_dilate_subtract_apply(gpu_ctx):
    ctx = gpu_ctx
    vol, seed, bone, grown, margin = _chain_reference()
    dims = dims_of(bone)
    volume = ctx.image_from(vol)
    mask, res = ctx.grow_region(volume, [seed], 500, 1200)
    assert res.as_dict()["count"] == int(bone.sum())
    wide = ctx.mask_morph(mask, dims, ffi.MORPH_DILATE, scene.radius_sq(MARGIN), scene.mask_weights(SIZES))
    same(wide.pull(), scene.mask_pack(grown), "dilated")
    ring = ctx.mask_combine(wide, mask, ffi.MASK_ANDNOT, dims, out=wide)
    assert ring is wide
    same(ring.pull(), scene.mask_pack(margin), "margin")
    depth = ctx.mask_distance(mask, dims, scene.mask_weights(SIZES), to_clear=True)  # "how deep inside the bone am I"
    same(depth.pull(), dr.distance(bone, scene.mask_weights(SIZES), True), "depth")
    ctx.apply_mask(volume, ring)
    assert np.array_equal(volume.pull(), gr.apply_mask(vol, margin))
    for m in (depth, wide, mask, volume):
        m.release()


def test_host_mirror_chain():
    vol, seed, bone, grown, margin = _chain_reference()
    n = 48
    env = scene.env_map(64, 32)
    L = host_lib(clvr_host_grow_region=(None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p]),
                 clvr_host_apply_mask=(None, [C.c_void_p, C.c_int, C.c_int]),
                 clvr_host_set_voxel_sizes=(None, [C.c_void_p, C.POINTER(C.c_float)]),
                 clvr_host_distance_map=(None, [C.c_void_p, C.c_int, C.c_uint, C.c_void_p]),
                 clvr_host_morph_mask=(C.c_ulonglong, [C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_uint)]),
                 clvr_host_hold_mask=(None, [C.c_void_p]),
                 clvr_host_combine_masks=(None, [C.c_void_p, C.c_int]),
                 clvr_host_extract_mesh=(None, [C.c_void_p, C.c_float, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong),
                                                C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_float)),
                                                C.POINTER(C.POINTER(C.c_ulonglong)), C.POINTER(C.POINTER(C.c_uint))]))
    h = L.clvr_host_create()
    try:
        L.clvr_host_load(h, vol.ctypes.data, n, n, n, env.ctypes.data, 64, 32)
        L.clvr_host_set_voxel_sizes(h, (C.c_float * 3)(*SIZES))
        seeds = np.array(seed, np.uint32)
        result = ffi.GrowResult()
        L.clvr_host_grow_region(h, seeds.ctypes.data, 1, 500, 1200, 0, C.byref(result))
        assert result.count == int(bone.sum())
        w = scene.mask_weights(SIZES)
        got = np.empty(vol.shape, np.uint32)
        L.clvr_host_distance_map(h, 0, NONE, got.ctypes.data)
        same(got, dr.distance(bone, w), "distance to the bone")
        L.clvr_host_distance_map(h, 1, 5000, got.ctypes.data)
        same(got, dr.distance(bone, w, True, 5000), "depth inside the bone, capped")
        L.clvr_host_hold_mask(h)
        info = (C.c_uint * 4)()
        count = L.clvr_host_morph_mask(h, ffi.MORPH_DILATE, MARGIN, info)
        assert (count, list(info)) == (int(grown.sum()), [1024, 256, 256, 1600])
        L.clvr_host_combine_masks(h, ffi.MASK_ANDNOT)
        L.clvr_host_distance_map(h, 0, 0, got.ctypes.data)
        assert np.array_equal(got == 0, margin)
        L.clvr_host_apply_mask(h, -32768, 0)
        nv, nt = C.c_ulonglong(0), C.c_ulonglong(0)
        p, q = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
        k, t = C.POINTER(C.c_ulonglong)(), C.POINTER(C.c_uint)()
        L.clvr_host_extract_mesh(h, -20000.0, 0, C.byref(nv), C.byref(nt), C.byref(p), C.byref(q), C.byref(k), C.byref(t))
        want = mr.mesh(gr.apply_mask(vol, margin), -20000.0)
        assert (nv.value, nt.value) == (len(want.keys), len(want.tris)) and nv.value > 5000
    finally:
        L.clvr_host_destroy(h)


def test_headless_grow_with_a_margin(tmp_path):
    vol, seed, bone, grown, margin = _chain_reference()
    Z, Y, X = vol.shape
    header = ("NRRD0004\ntype: short\ndimension: 3\nsizes: %d %d %d\nspace directions: (1,0,0) (0,1,0) (0,0,2.5)\nendian: little\n"
              "encoding: raw\n\n" % (X, Y, Z))
    with open(tmp_path / "v.nrrd", "wb") as f:
        f.write(header.encode("ascii") + np.ascontiguousarray(vol, "<i2").tobytes())
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(np.random.default_rng(5).random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    files = [str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", "64", "64"]

    def run(*options):
        out = subprocess.run([exe] + list(options) + files + [str(tmp_path / "m.ply")], capture_output=True, text=True, timeout=120)
        return out.returncode, [json.loads(s) for s in out.stdout.strip().splitlines() if s.startswith("{")], out.stderr

    code, lines, err = run("--grow=%d,%d,%d,500,1200,dilate=2" % seed, "--mesh=-20000")
    assert code == 0, err
    assert lines[0]["count"] == int(bone.sum())
    assert lines[0]["morph"] == {"op": "dilate", "radius_sq": 1024, "weight": [256, 256, 1600], "count": int(grown.sum())}
    assert lines[-1]["vertices"] == len(mr.mesh(gr.apply_mask(vol, grown), -20000.0).keys)
    w = (256, 256, 1600)
    code, lines, err = run("--components=500,1200,largest=1,open=1.5,remove,fill=-1000", "--mesh=-20000")
    assert code == 0, err
    ranks = lr.label(vol, 500, 1200)[0]
    opened = dr.morph(ranks == 1, w, dr.OPEN, scene.radius_sq(1.5))
    assert lines[0]["morph"] == {"op": "open", "radius_sq": 576, "weight": [256, 256, 1600], "count": int(opened.sum())}
    assert "morph" not in run("--grow=%d,%d,%d,500,1200" % seed, "--mesh=-20000")[1][0]  # no item: the line is the old one
    for bad in ("dilate=", "dilate=-1", "dilate=x", "dilate=2,erode=1", "dilate", "grow=2"):
        assert run("--grow=%d,%d,%d,500,1200," % seed + bad)[0] == 1, bad
    assert run("--components=500,1200,close=")[0] == 1
