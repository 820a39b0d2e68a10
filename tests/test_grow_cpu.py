"""The mask layout helpers (scene.mask_*), the binding's structs, and the numpy restatement of clwh_segment_grow (tests/grow_ref.py)
checked on the CPU: against scipy's labelling, against its own two-step semantics and box rule, and for the tallies the GPU test's
inputs claim (tests/test_gpu_grow.py), so that those inputs really exercise what they are there for."""
import ctypes as C

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import grow_ref as gr
from tests.grow_ref import RANDOM_DIMS, WINDOWS, random_case, random_volume


def test_pack_unpack_round_trip_on_ragged_dims():
    rng = np.random.default_rng(11)
    for X, Y, Z in ((130, 3, 7), (1, 1, 1), (64, 16, 16), (65, 2, 3), (31, 5, 1), (128, 1, 2)):
        m = rng.random((Z, Y, X)) < 0.5
        m[0, 0, 0] = m[-1, -1, -1] = True
        wpr = scene.mask_words_per_row(X)
        assert wpr == 2 * ((X + 63) // 64) and wpr % 2 == 0 and wpr * 32 >= X
        w = scene.mask_pack(m)
        assert w.dtype == np.uint32 and w.shape == (wpr * Y * Z,)
        for x, y, z in ((0, 0, 0), (X - 1, Y - 1, Z - 1), (X // 2, Y // 2, Z // 2)):  # the header's formula, literally
            assert bool((int(w[(z * Y + y) * wpr + (x >> 5)]) >> (x & 31)) & 1) == bool(m[z, y, x])
        rows = w.reshape(Z * Y, wpr)
        assert int(sum(bin(int(v)).count("1") for v in w)) == int(m.sum())  # no bit beyond x < X: padding is zero
        if X % 32:
            assert not (rows[:, (X - 1) >> 5] >> np.uint32(X % 32)).any()
        assert not rows[:, ((X - 1) >> 5) + 1:].any()
        assert np.array_equal(scene.mask_unpack(w, (X, Y, Z)), m)
        dirty = w.copy().reshape(Z * Y, wpr)
        dirty[:, -1] |= np.uint32(0x80000000) if wpr * 32 > X else np.uint32(0)
        assert np.array_equal(scene.mask_unpack(dirty, (X, Y, Z)), m)  # unpack drops the padding


def test_binding_structs_match_the_header():
    assert C.sizeof(ffi.GrowResult) == 64 and ffi.GrowResult.sum.offset == 32 and ffi.GrowResult.rounds.offset == 56
    assert C.sizeof(ffi.GrowDesc) == 72 and ffi.GrowDesc.seeds.offset == 32 and ffi.GrowDesc.box_lo.offset == 40 and ffi.GrowDesc.result.offset == 64
    assert C.sizeof(ffi.ApplyMaskDesc) == 32 and ffi.ApplyMaskDesc.fill.offset == 24
    assert (ffi.GROW_26, ffi.GROW_FROM_MASK, ffi.GROW_DENSE, ffi.MASK_INVERT, ffi.GROW_MAX_SEEDS) == (1, 2, 4, 1, 65536)
    assert {"clwh_segment_grow", "clwh_volume_apply_mask"} <= set(ffi.EXPORTED_SYMBOLS)
    r = ffi.GrowResult()
    assert r.as_dict() == gr.stats(np.zeros((1, 1, 1), np.int16), np.zeros((1, 1, 1), bool))


@pytest.mark.parametrize("connectivity", [6, 26])
def test_reference_equals_scipy_labelling(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    lo, hi = WINDOWS[connectivity]
    checked = 0
    for dims, seed in (((65, 17, 17), 0), ((33, 40, 35), 1), ((70, 40, 36), 2)):
        vol = random_volume(dims, seed)
        adm = gr.admissible(vol, lo, hi)
        lab, n = ndimage.label(adm, structure)
        # the reference's own labelling names the same partition
        mine = gr.labels(adm, connectivity)
        assert len(np.unique(mine[adm])) == n
        pairs = np.unique(np.stack([mine[adm], lab[adm]]), axis=1)
        assert pairs.shape[1] == n
        first, size, count = gr.largest_component(adm, connectivity)
        assert count == n and size == int(np.bincount(lab.reshape(-1))[1:].max())
        # growth from one voxel of a component is that component, for the largest and for a few others
        rng = np.random.default_rng(seed)
        z, y, x = np.nonzero(adm)
        picks = [first] + [(int(x[i]), int(y[i]), int(z[i])) for i in rng.integers(0, len(x), 5)]
        for sx, sy, sz in picks:
            region, _ = gr.grow(vol, [(sx, sy, sz)], lo, hi, connectivity)
            assert np.array_equal(region, lab == lab[sz, sy, sx])
            checked += 1
        # several seeds: the union of their components; an inadmissible seed adds nothing
        outside = np.argwhere(~adm)[0][::-1]
        region, _ = gr.grow(vol, picks[:3] + [tuple(int(v) for v in outside)], lo, hi, connectivity)
        assert np.array_equal(region, np.isin(lab, [lab[p[2], p[1], p[0]] for p in picks[:3]]))
    assert checked == 18


def test_two_step_growth_is_growth_from_the_mask():
    vol = random_volume((70, 40, 36), 1)
    first = random_case((70, 40, 36), 1, 6)[1]
    narrow, _ = gr.grow(vol, [first], -1000, -400)
    assert 0 < narrow.sum()
    wide, _ = gr.grow(vol, None, -1000, -280, from_mask=narrow)
    # wider window from the narrow result: exactly the union of the wide components that the narrow set touches
    direct, _ = gr.grow(vol, [first], -1000, -280)
    assert narrow.sum() < wide.sum() and np.array_equal(wide, direct) and not (narrow & ~wide).any()
    # a window that excludes earlier voxels clears them: only the admissible bits of the mask are seeds
    moved, _ = gr.grow(vol, None, -600, -280, from_mask=wide)
    adm = gr.admissible(vol, -600, -280)
    assert (wide & ~adm).any() and not (moved & ~adm).any() and np.array_equal(moved & wide, wide & adm)
    # nothing admissible in the mask, no seeds: empty
    none, depth = gr.grow(vol, None, 500, 600, from_mask=wide)
    assert not none.any() and depth == 0 and gr.stats(vol, none)["count"] == 0


def test_box_rule():
    vol = np.zeros((5, 6, 20), np.int16)
    vol[2, 3, :] = 100  # a bar along x
    whole, _ = gr.grow(vol, [(2, 3, 2)], 100, 100)
    assert whole.sum() == 20
    for box in (((0, 0, 0), (0, 0, 0)), ((0, 0, 0), (20, 6, 5)), None):
        assert np.array_equal(gr.grow(vol, [(2, 3, 2)], 100, 100, box=box)[0], whole)
    cut, _ = gr.grow(vol, [(2, 3, 2)], 100, 100, box=((0, 0, 0), (10, 6, 5)))  # hi is exclusive
    assert cut.sum() == 10 and cut[2, 3, :10].all()
    assert gr.stats(vol, cut)["bbox_hi"] == (10, 4, 3) and gr.stats(vol, cut)["bbox_lo"] == (0, 3, 2)
    other, _ = gr.grow(vol, [(2, 3, 2)], 100, 100, box=((10, 0, 0), (20, 6, 5)))  # the seed lies outside the box: not admissible
    assert not other.any()
    empty, _ = gr.grow(vol, [(2, 3, 2)], 100, 100, box=((3, 3, 2), (3, 6, 5)))
    assert not empty.any()
    # a box that cuts a component in two keeps the seed's side
    vol[2, 3, 9] = 0
    vol[2, 2, 8:11] = 100  # a bridge through y = 2
    assert gr.grow(vol, [(2, 3, 2)], 100, 100)[0].sum() == 22
    assert gr.grow(vol, [(2, 3, 2)], 100, 100, box=((0, 3, 0), (20, 6, 5)))[0].sum() == 9


def test_statistics_are_exact_integers():
    vol = np.full((4, 4, 70), 32767, np.int16)
    vol[1, 1, 3] = -32768
    region = np.ones(vol.shape, bool)
    s = gr.stats(vol, region)
    n = vol.size
    assert s == {"count": n, "bbox_lo": (0, 0, 0), "bbox_hi": (70, 4, 4), "sum": 32767 * (n - 1) - 32768,
                 "sum_sq": 32767 ** 2 * (n - 1) + 32768 ** 2, "vmin": -32768, "vmax": 32767}
    assert np.array_equal(gr.apply_mask(vol, vol < 0, fill=7), np.where(vol < 0, vol, 7))
    assert np.array_equal(gr.apply_mask(vol, vol < 0, fill=7, invert=True), np.where(vol < 0, 7, vol))


@pytest.mark.parametrize("dims", RANDOM_DIMS)
def test_random_fixtures_are_what_the_gpu_test_claims(dims):
    """the largest component spans 5-18 tiles, has a geodesic depth of 63-344, and hundreds of other components exist"""
    for seed in range(3):
        for connectivity in (6, 26):
            vol, first, region, depth, n = random_case(dims, seed, connectivity)
            lo, hi = WINDOWS[connectivity]
            assert region[first[2], first[1], first[0]] and lo <= vol[first[2], first[1], first[0]] <= hi
            assert 5 <= gr.tiles_spanned(region) <= 18, (dims, seed, connectivity, gr.tiles_spanned(region))
            assert 63 <= depth <= 344, (dims, seed, connectivity, depth)
            assert n - 1 >= 200, (dims, seed, connectivity, n)
            share = gr.admissible(vol, lo, hi).mean()
            assert abs(share - (0.36 if connectivity == 6 else 0.12)) < 0.01


def test_serpentine_fixture():
    vol = gr.serpentine()
    assert vol.shape == (3, 40, 136) and not vol[0].any() and not vol[2].any()
    region, depth = gr.grow(vol, [(0, 0, 1)], 100, 100)
    assert int(region.sum()) == 2739 == int((vol == 100).sum()) and depth == 2738
    assert gr.tiles_spanned(region) == 9
    assert region[1, 0::2, 63].all() and region[1, 0::2, 64].all() and region[1, 0::2, 128].all()  # every even row crosses x = 64 and 128
    assert region[1, 15, 0] and region[1, 16, 0] and region[1, 31, 0] and region[1, 32, 0]          # and the path crosses y = 16 and 32
    # 26-connectivity shortens the path (diagonal steps around the turns) but reaches the same voxels
    again, depth26 = gr.grow(vol, [(0, 0, 1)], 100, 100, 26)
    assert np.array_equal(again, region) and depth26 < depth


def test_tile_border_fixtures():
    """two voxels that touch only at a corner across a tile corner, and two that touch only along an edge across a tile edge"""
    for a, b, kind in (((63, 15, 15), (64, 16, 16), 3), ((63, 15, 5), (64, 16, 5), 2), ((10, 15, 15), (10, 16, 16), 2)):
        vol = np.zeros((20, 20, 70), np.int16)
        vol[a[2], a[1], a[0]] = vol[b[2], b[1], b[0]] = 1
        assert sum(abs(p - q) for p, q in zip(a, b)) == kind
        assert sum((p >> s) != (q >> s) for p, q, s in zip(a, b, (6, 4, 4))) == kind  # every differing axis crosses a tile face
        assert gr.grow(vol, [a], 1, 1, 6)[0].sum() == 1 and gr.grow(vol, [a], 1, 1, 26)[0].sum() == 2
