"""The numpy restatement of clwh_mask_distance / clwh_mask_morph / clwh_mask_combine (tests/distance_ref.py): the separable passes
against the definition over all pairs (and scipy's transform where it is installed), the morphology against one step of grow_ref's
neighbourhoods, the set inclusions, the integer rules of scene.mask_weights / radius_sq, and the entry points without a device."""
import ctypes as C

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import distance_ref as dr
from tests import grow_ref as gr

INVALID_VALUE = 1


def _case_mask(dims, seed=5):
    """a few dozen sites however large the volume, so that the brute force stays quick"""
    X, Y, Z = dims
    n = X * Y * Z
    m = np.zeros(n, bool)
    m[np.random.default_rng(seed).choice(n, size=min(n, 54), replace=False)] = True
    return m.reshape(Z, Y, X)


@pytest.mark.parametrize("dims,w", dr.CPU_CASES)
def test_separable_equals_the_definition(dims, w):
    m = _case_mask(dims)
    assert np.array_equal(dr.separable(m, w), dr.brute(m, w))
    if m.size > 54:  # the other site kind: distances to the clear voxels of a mask with few of them
        assert np.array_equal(dr.distance(~m, w, to_clear=True), dr.brute(m, w))
    assert np.array_equal(dr.distance(m, w, cap=9), np.where(dr.brute(m, w) <= 9, dr.brute(m, w), dr.NONE))


@pytest.mark.parametrize("dims,w", dr.CPU_CASES)
def test_separable_equals_scipy(dims, w):
    ndimage = pytest.importorskip("scipy.ndimage")
    m = _case_mask(dims)
    edt = ndimage.distance_transform_edt(~m, sampling=np.sqrt(np.array(w[::-1], np.float64)))
    assert np.array_equal(dr.separable(m, w), np.rint(edt ** 2).astype(np.uint32))


def test_no_site_is_none_and_a_full_mask_erodes_to_itself():
    empty, full = np.zeros((3, 4, 5), bool), np.ones((3, 4, 5), bool)
    assert (dr.separable(empty, (1, 1, 1)) == dr.NONE).all() and (dr.brute(empty, (1, 1, 1)) == dr.NONE).all()
    assert (dr.distance(full, (1, 1, 1), to_clear=True) == dr.NONE).all() and (dr.distance(full, (1, 1, 1)) == 0).all()
    for radius_sq in (0, 7, dr.NONE):
        assert dr.morph(full, (1, 1, 1), dr.ERODE, radius_sq).all()
        assert not dr.morph(empty, (1, 1, 1), dr.DILATE, radius_sq).any()


def _dilate_by_offsets(m, connectivity):
    p = np.zeros(tuple(n + 2 for n in m.shape), bool)
    p[1:-1, 1:-1, 1:-1] = m
    out = m.copy()
    Z, Y, X = m.shape
    for dx, dy, dz in gr.offsets(connectivity):
        out |= p[1 + dz:Z + 1 + dz, 1 + dy:Y + 1 + dy, 1 + dx:X + 1 + dx]
    return out


def test_unit_balls_are_the_6_and_26_neighbourhoods():
    m = dr.random_mask((33, 20, 9), 0.02, 3)
    assert np.array_equal(dr.morph(m, (1, 1, 1), dr.DILATE, 1), _dilate_by_offsets(m, 6))
    assert np.array_equal(dr.morph(m, (1, 1, 1), dr.DILATE, 3), _dilate_by_offsets(m, 26))
    assert np.array_equal(dr.morph(m, (1, 1, 1), dr.DILATE, 0), m)
    # eroding is dilating the complement, except that the outside of the volume is not clear
    inner = ~_dilate_by_offsets(~m, 6)
    assert np.array_equal(dr.morph(m, (1, 1, 1), dr.ERODE, 1), inner)


def test_open_is_inside_and_close_is_outside():
    m = dr.random_mask((33, 20, 9), 0.5, 4)
    for w in ((1, 1, 1), (1, 1, 6)):
        for radius_sq in (1, 2, 9):
            o, c = dr.morph(m, w, dr.OPEN, radius_sq), dr.morph(m, w, dr.CLOSE, radius_sq)
            assert not (o & ~m).any() and not (m & ~c).any()
            assert o.sum() < m.sum() < c.sum()


def test_combine_and_clean_padding():
    a, b = dr.random_mask((33, 20, 9), 0.5, 4), dr.random_mask((33, 20, 9), 0.5, 6)
    assert np.array_equal(dr.combine(a, b, dr.ANDNOT), a & ~b) and np.array_equal(dr.combine(a, None, dr.NOT), ~a)
    words = scene.mask_pack(dr.combine(a, None, dr.NOT)).reshape(9 * 20, 2)
    assert (words[:, 1] >> 1 == 0).all() and words[:, 1].any()  # x = 32 is bit 0 of the second word; nothing above it
    assert np.array_equal(scene.mask_unpack(words, (33, 20, 9)), ~a)


def test_float_spacing_becomes_integers_in_one_place():
    assert scene.mask_weights((1, 1, 2.5)) == (256, 256, 1600)
    assert scene.mask_weights((0.7, 0.7, 2.5), per_unit=10) == (49, 49, 625)
    assert scene.mask_weights((1, 1, 0.01)) == (256, 256, 1)  # never 0
    assert scene.radius_sq(2.0) == 1024 and scene.radius_sq(0) == 0 and scene.radius_sq(0.1) == 2  # floor(1.6^2)
    assert dr.weights_ok((2, 2, 2), (2147483647, 2147483646, 1)) and not dr.weights_ok((2, 2, 2), (2147483647, 2147483647, 1))
    assert not dr.weights_ok((5, 5, 5), (1, 0, 1))


def test_binding_structs_match_the_header():
    # (csrc/clwh_distance.hip asserts the same three sizes of the C structures when the library is compiled)
    assert C.sizeof(ffi.DistanceDesc) == 48 and C.sizeof(ffi.MorphDesc) == 56 and C.sizeof(ffi.MaskCombineDesc) == 40
    assert ffi.DistanceDesc.cap.offset == 40 and ffi.MorphDesc.radius_sq.offset == 40 and ffi.MaskCombineDesc.op.offset == 36
    assert ffi.DIST_NONE == dr.NONE == 0xFFFFFFFF and ffi.DIST_TO_CLEAR == 1
    assert (ffi.MORPH_DILATE, ffi.MORPH_ERODE, ffi.MORPH_OPEN, ffi.MORPH_CLOSE) == (dr.DILATE, dr.ERODE, dr.OPEN, dr.CLOSE) == (0, 1, 2, 3)
    assert (ffi.MASK_AND, ffi.MASK_OR, ffi.MASK_XOR, ffi.MASK_ANDNOT, ffi.MASK_NOT) == (dr.AND, dr.OR, dr.XOR, dr.ANDNOT, dr.NOT) == (0, 1, 2, 3, 4)


def test_entry_points_exist_and_refuse_null_without_a_device():
    L = ffi.lib()
    for name, desc in (("clwh_mask_distance", ffi.DistanceDesc()), ("clwh_mask_morph", ffi.MorphDesc()), ("clwh_mask_combine", ffi.MaskCombineDesc())):
        assert name in ffi.EXPORTED_SYMBOLS
        assert getattr(L, name)(None, C.byref(desc)) == INVALID_VALUE
        assert getattr(L, name)(C.c_void_p(1), None) == INVALID_VALUE  # (desc is tested before ctx is used)
