"""The volume filter's contract on the CPU: tests/vfilter_ref.py against scipy.ndimage, scene.gaussian_weights / binomial_weights, the
non-vacuity of the cases the GPU tests share, the compiled kernels' resource usage, and the binding.  No device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from cl_volume_renderer_amd import ffi, scene
from tests import vfilter_cases as vc
from tests import vfilter_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def size_of(radius):
    return tuple(2 * r + 1 for r in radius[::-1])  # scipy's axes are z, y, x


# ---- 1. the reference is scipy's, on every shape and field
@pytest.mark.parametrize("shape", sorted(vc.SHAPES))
def test_reference_equals_scipy(shape):
    n = 0
    for name in vc.FIELDS:
        vol = vc.field(shape, name)
        for label, kind, radius, weights in vc.PARAMS:
            got = vc.reference(shape, name, label)
            assert got.dtype == np.int16 and got.shape == vol.shape
            if kind == vr.MEDIAN:
                want = ndimage.median_filter(vol, size=size_of(radius), mode="nearest")
            elif kind == vr.MIN:
                want = ndimage.minimum_filter(vol, size=size_of(radius), mode="nearest")
            elif kind == vr.MAX:
                want = ndimage.maximum_filter(vol, size=size_of(radius), mode="nearest")
            else:
                want = vol
                for axis in (0, 1, 2):  # x, y, z = scipy's axes 2, 1, 0
                    w = np.asarray(weights[axis], np.int64)
                    full = np.concatenate([w[:0:-1], w])
                    want = ((ndimage.correlate1d(want.astype(np.int64), full, axis=2 - axis, mode="nearest") + 2048) >> 12).astype(np.int16)
            assert np.array_equal(got, want), (shape, name, label)
            n += 1
    assert n == len(vc.FIELDS) * len(vc.PARAMS)


def test_box_extremes_tap_by_tap_equal_axis_by_axis():
    """vfilter_ref switches to axis by axis above 1000 taps: the same function"""
    for shape, radius in (("thin", (4, 6, 5)), ("main", (3, 2, 4)), ("flat", (16, 2, 1))):
        for name in ("random", "ties"):
            vol = vc.field(shape, name)
            for kind in (vr.MIN, vr.MAX):
                assert np.array_equal(vr.extreme(vol, radius, kind), vr.extreme_by_axes(vol, radius, kind)), (shape, radius, name, kind)


# ---- 2. the weights
def test_gaussian_weights():
    assert [w.tolist() for w in scene.gaussian_weights(1.0)] == [[1636, 991, 221, 18]] * 3
    assert [w.tolist() for w in scene.gaussian_weights(0.0)] == [[4096]] * 3 and scene.gaussian_weights(-1.0)[2].tolist() == [4096]
    # millimetres on anisotropic voxels: sigma / spacing per axis
    w = scene.gaussian_weights(1.5, (0.5, 1.5, 3.0))
    assert [v.tolist() for v in w] == [scene.gaussian_weights(3.0)[0].tolist(), [1636, 991, 221, 18], scene.gaussian_weights(0.5)[0].tolist()]
    assert [len(v) - 1 for v in w] == [9, 3, 2]
    assert len(scene.gaussian_weights(5.4)[0]) == 17 and len(scene.gaussian_weights(100.0)[0]) == 17  # the radius stops at 16
    for s in np.arange(0.02, 12.0, 0.01):
        w = scene.gaussian_weights(float(s))[0]
        assert w.dtype == np.uint16
        v = w.astype(np.int64)
        assert v[0] + 2 * v[1:].sum() == 4096 and (v >= 0).all(), s
        assert (np.diff(v[1:]) <= 0).all(), s
        # The centre takes what the rounding of the others leaves.  Up to sigma = 5.87 voxels it is the largest weight; from 5.88 on
        # (a Gaussian cut at 16 < 3 sigma, neighbouring weights 1 % apart) the formula of the contract can leave it up to 5 below w_1.
        assert v[0] >= v[1] if s < 5.875 else v[0] >= v[1] - 5, (s, v[:2])


def test_binomial_weights():
    assert [scene.binomial_weights(p).tolist() for p in (0, 1, 2)] == [[4096], [2048, 1024], [1536, 1024, 256]]
    for p in range(7):
        w = scene.binomial_weights(p).astype(np.int64)
        full = np.array([1])
        for _ in range(p):
            full = np.convolve(full, [1, 2, 1])
        assert np.array_equal(np.concatenate([w[:0:-1], w]) * 4 ** p, full * 4096) and w[0] + 2 * w[1:].sum() == 4096
    with pytest.raises(ValueError):
        scene.binomial_weights(7)


# ---- 3. the shared cases can tell a wrong filter from a right one (the reference alone)
def test_cases_are_not_vacuous():
    vol = vc.field(*vc.MAIN)
    assert (vc.reference(*vc.MAIN, "median 111") != vol).mean() > 0.5
    border = np.ones(vol.shape, bool)
    border[1:-1, 1:-1, 1:-1] = False
    differs = vr.median(vol, (1, 1, 1), "zero") != vc.reference(*vc.MAIN, "median 111")
    assert differs[border].mean() > 0.5 and not differs[~border].any()
    w = vc.PARAM["smooth gauss 1 1 0.6"][3]
    contract = vc.reference(*vc.MAIN, "smooth gauss 1 1 0.6")
    assert (vr.smooth(vol, w, (2, 1, 0)) != contract).mean() > 0.05
    assert (vr.smooth_single_rounding(vol, w) != contract).mean() > 0.05
    # constant fields (-32768 / 32767) and all-zero radii pass through; everything else changes the main field
    for shape in vc.SHAPES:
        for label, kind, radius, _ in vc.PARAMS:
            assert np.array_equal(vc.reference(shape, "constant", label), vc.field(shape, "constant")), (shape, label)
            if not any(radius):
                assert np.array_equal(vc.reference(shape, "random", label), vc.field(shape, "random")), (shape, label)
    for label, kind, radius, _ in vc.PARAMS:
        assert not any(radius) or (vc.reference(*vc.MAIN, label) != vol).mean() > 0.5, label
    # the outermost-tap weights read clamped coordinates on most of a volume thinner than the radius
    assert vc.SHAPES["thin"][0] < 16 and vc.SHAPES["thin"][2] < 16
    bits, words = vc.mask_of("main")
    assert 0.4 < bits.mean() < 0.6 and np.array_equal(scene.mask_unpack(words, vc.SHAPES["main"]), bits)
    assert not np.array_equal(words, scene.mask_pack(bits))  # the padding is garbage
    assert set(np.unique(vc.field("main", "extremes")).tolist()) == {-32768, 32767}


def test_masked_reference_reads_the_unfiltered_volume():
    vol = vc.field(*vc.MAIN)
    bits, _ = vc.mask_of("main")
    got = vr.filtered(vol, vr.MEDIAN, (1, 1, 1), None, bits)
    assert np.array_equal(got[bits], vc.reference(*vc.MAIN, "median 111")[bits]) and np.array_equal(got[~bits], vol[~bits])


# ---- 4. resource usage
def test_no_kernel_uses_scratch_memory():
    text = open(os.path.join(ROOT, "profiles", "filter_resource_usage.txt")).read()
    kernels = re.findall(r"Function Name: (\S+)", text)
    median = ["k_filter_medianILi%dELi%dELi%dEE" % (rx, ry, rz) for rz in (0, 1) for ry in (0, 1) for rx in (0, 1) if rx + ry + rz]
    kinds = (ffi.FILTER_MIN, ffi.FILTER_MAX, ffi.FILTER_SMOOTH)
    lines = ["k_filter_line_xILi%dEE" % kind for kind in kinds] + ["k_filter_line_yzILi%dELi%dEE" % (kind, ring) for kind in kinds for ring in (16, 32, 64)]
    for name in median + lines:
        assert sum(name in k for k in kernels) == 1, name
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)
    spills = re.findall(r"[SV]GPRs Spill: (\d+)", text)
    assert len(scratch) == len(kernels) == 19 and set(scratch) == {"0"} and set(spills) == {"0"}


# ---- 5. the binding
def test_ffi_symbol_and_struct():
    assert C.sizeof(ffi.FilterDesc) == 72 and ffi.FilterDesc.radius.offset == 32 and ffi.FilterDesc.weights.offset == 48
    assert (ffi.FILTER_MEDIAN, ffi.FILTER_MIN, ffi.FILTER_MAX, ffi.FILTER_SMOOTH) == (0, 1, 2, 3)
    assert (ffi.FILTER_MAX_RADIUS, ffi.FILTER_WEIGHT_SUM) == (16, 4096)
    L = ffi.lib()
    assert L.clwh_volume_filter(None, None) == 1  # CLWH_ERR_INVALID_VALUE, before anything touches a device
    assert L.clwh_volume_filter(None, C.byref(ffi.FilterDesc())) == 1
    header = open(os.path.join(ROOT, "include", "clwh.h")).read()
    assert "int clwh_volume_filter(clwh_ctx *ctx, const clwh_filter_desc *desc);" in header
