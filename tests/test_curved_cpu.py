"""The curved view, the section profile and the curve's frames without a GPU: the restatements of tests/curved_ref.py against each
other and against tests/slice_ref.py, scene.curve_frames against its literal restatement and against closed forms, the point of
the feature on the tube of tests/costpath_ref.py, and what the cases of tests/curved_cases.py reach -- so that no comparison of
tests/test_gpu_curved.py is empty."""
import ctypes as C
import math

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import costpath_ref as cp
from tests import curved_cases as cc
from tests import curved_ref as cr
from tests import slice_ref as sr
from tests.test_gpu_slice import Tally
from tests.view_helpers import F, bits, host_lib

SPECIAL_ROWS = (0, 3, 5, 9, 11, 12, 14, 21, 30, 39)


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(bits(got[2]), bits(want[2]))


def test_the_view_equals_the_literal_pixel():
    rng = np.random.default_rng(3)
    checked = 0
    for c in cc.twisted_cases()[1:9:2] + cc.twisted_cases()[9:12]:
        want, _ = cc.reference_of(c)
        w, h = c["region_wh"]
        pixels = [(28, 11), (27, 12), (0, 3), (55, 5)] + [(int(rng.integers(w)), int(rng.integers(h))) for _ in range(8)]
        for x, y in pixels:
            for mode in cc.MODES:
                px, value, t_ext = cr.curved_scalar(c["vol"], c["rows"], x, y, mode, c["n"], c["step"], c["window"])
                frame, values, t_extreme = want[mode]
                assert np.array_equal(px, frame[y, x]) and bits(value) == bits(values[y, x]) and bits(t_ext) == bits(t_extreme[y, x]), (x, y, mode)
                checked += 1
    assert checked == 7 * 12 * 3


@pytest.mark.parametrize("family", ["twisted", "planar"])
def test_every_row_is_a_slice_of_its_own(family):
    """row y of the curved view == region row 0 of slice_ref.slice_view with origin, du, normal of that row (and any dv)"""
    cases = cc.twisted_cases() if family == "twisted" else cc.planar_cases()
    for c in cases:
        want, _ = cc.reference_of(c)
        w, h = c["region_wh"]
        for y in SPECIAL_ROWS:
            r = c["rows"][y]
            one, _ = sr.slice_view(c["vol"], r[0:3], r[3:6], (0.3, -0.2, 0.1), r[6:9], (w, 1), modes=cc.MODES, slab_samples=c["n"], step=c["step"],
                                   window_cw=c["window"])
            for mode in cc.MODES:
                assert _same([a[0] for a in one[mode]], [a[y] for a in want[mode]]), (y, mode)


def test_the_twisted_family_reaches_every_kind():
    tally = Tally()
    for c in cc.twisted_cases():
        stats = cc.reference_of(c)[1]
        tally.add(stats)
        assert sum(stats["skip_changed"].values()) == 0
        assert stats["none"][-8:].all() and stats["none"][9].all(), "the padding rows and the far row keep nothing"
    tally.assert_all()
    print(vars(tally))
    first = cc.reference_of(cc.twisted_cases()[2])[1]  # 64^3, 64 samples
    assert first["none"][11, :28].all() and not first["none"][11, 28:].any(), "pixel 28 sits on the corner (0, 0, 0), which is inside"
    assert not first["none"][12, :28].any() and first["none"][12, 28:].all(), "... and on the corner (X, Y, Z), which is outside"


# ---- the frames
def _paths():
    centre = np.array(cp.tube_paths()[0], np.float64)
    t = np.linspace(0.0, 5.0, 90)
    helix = np.stack([20 + 9 * np.cos(t), 22 + 9 * np.sin(t), 3 + 2.5 * t], axis=1)
    return [("centreline", centre, (1.0, 1.0, 1.0), dict(pixel_mm=0.25, station_mm=0.25)),
            ("centreline, anisotropic, turned slab", centre, (0.7, 0.8, 2.5), dict(pixel_mm=0.3, station_mm=0.45, angle=0.7, slab_samples=17, step_mm=0.4)),
            ("helix of float points", helix, (1.0, 0.5, 1.25), dict(pixel_mm=0.5, station_mm=0.37, smooth_passes=0, angle=-2.0, slab_samples=64)),
            ("two points", np.array([[1, 2, 3], [9, 4, 3]], np.float64), (1.0, 1.0, 1.0), dict(pixel_mm=1.0, station_mm=0.5, smooth_passes=3))]


@pytest.mark.parametrize("what, points, spacing, kw", _paths(), ids=[p[0] for p in _paths()])
def test_curve_frames_equal_the_literal_restatement_bit_for_bit(what, points, spacing, kw):
    rows, s_mm, n = scene.curve_frames(points, spacing, 64, **kw)
    want_rows, want_s, want_n = cr.curve_frames_literal(points, spacing, 64, **kw)
    assert n == want_n and n >= 2 and rows.shape == ((n + 7) // 8 * 8, 9) and rows.dtype == F
    assert np.array_equal(s_mm.view(np.uint64), want_s.view(np.uint64))
    assert np.array_equal(bits(rows), bits(want_rows))
    assert np.array_equal(rows[n:], np.tile(cc.PADDING_ROW, (len(rows) - n, 1)))


@pytest.mark.parametrize("what, points, spacing, kw", _paths(), ids=[p[0] for p in _paths()])
def test_the_host_mirror_frames_equal_the_python_ones_bit_for_bit(what, points, spacing, kw):
    """renderer::curve_frames through libclvr_host.so"""
    L = host_lib(clvr_host_curve_frames=(C.c_ulonglong, [C.c_void_p, C.c_ulonglong, C.POINTER(C.c_double), C.c_int, C.c_double, C.c_double, C.c_int,
                                                         C.c_double, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_ulonglong,
                                                         C.POINTER(C.c_ulonglong)]))
    rows, s_mm, n = scene.curve_frames(points, spacing, 64, **kw)
    pts = np.ascontiguousarray(points, np.float64)
    got_rows, got_s, got_n = np.full((len(rows) + 8, 9), 77, F), np.full(len(rows) + 8, 77.0), C.c_ulonglong(0)
    H = L.clvr_host_curve_frames(pts.ctypes.data, len(pts), (C.c_double * 3)(*spacing), 64, kw["pixel_mm"], kw["station_mm"],
                                 kw.get("smooth_passes", 8), kw.get("angle", 0.0), kw.get("slab_samples", 1), kw.get("step_mm", 0.0) or 0.0,
                                 got_rows.ctypes.data, got_s.ctypes.data, len(got_rows), C.byref(got_n))
    assert (H, got_n.value) == (len(rows), n)
    assert np.array_equal(bits(got_rows[:H]), bits(rows)) and np.all(got_rows[H:] == 77)
    assert np.array_equal(got_s[:n].view(np.uint64), s_mm.view(np.uint64))


def test_curve_frames_refuse_what_is_no_curve():
    for bad in ([(1, 1, 1)], [], [(1, 1, 1), (1, 1, 1), (2, 1, 1)]):
        with pytest.raises(ValueError):
            scene.curve_frames(bad, (1, 1, 1), 8, pixel_mm=0.5, station_mm=0.5)
    with pytest.raises(ValueError):  # one station only
        scene.curve_frames([(0, 0, 0), (1, 0, 0)], (1, 1, 1), 8, pixel_mm=0.5, station_mm=2.0, smooth_passes=0)
    with pytest.raises(ValueError):
        scene.curve_frames([(0, 0, 0), (5, 0, 0)], (1, 0, 1), 8, pixel_mm=0.5, station_mm=0.5)


def test_a_straight_path_in_closed_form():
    cy, cz, width, n_slab = 7, 4, 64, 5
    points = [(i, cy, cz) for i in range(12)]
    rows, s_mm, n = scene.curve_frames(points, (1.0, 1.0, 1.0), width, pixel_mm=0.5, station_mm=0.5, slab_samples=n_slab)
    assert n == 23 and np.array_equal(s_mm, 0.5 * np.arange(23))
    for j in range(n):
        C = np.array([0.5 + 0.5 * j, cy + 0.5, cz + 0.5])
        U, N = np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0])  # |T . e| ties between y and z: the lower index
        want = np.concatenate([C - (width - 1) / 2.0 * 0.5 * U - (n_slab - 1) / 2.0 * 0.5 * N, 0.5 * U, N]).astype(F)
        assert np.array_equal(bits(rows[j]), bits(want)), j


def test_a_circle_in_a_z_plane_keeps_the_frame_vertical():
    theta = np.linspace(0.3, 5.5, 400)
    points = np.stack([30 + 12 * np.cos(theta), 31 + 12 * np.sin(theta), np.full(400, 9.0)], axis=1)
    parts = {}
    rows, _, n = cr.curve_frames_literal(points, (1.0, 1.0, 1.0), 64, pixel_mm=0.5, station_mm=0.5, smooth_passes=0, parts=parts)
    assert n > 100 and np.array_equal(parts["U"], np.tile([0.0, 0.0, 1.0], (n, 1))), "every reflection vector has z = 0"
    got, _, _ = scene.curve_frames(points, (1.0, 1.0, 1.0), 64, pixel_mm=0.5, station_mm=0.5, smooth_passes=0)
    assert np.array_equal(bits(got), bits(rows))
    assert np.array_equal(got[:n, 3:6], np.tile(np.array([0, 0, 0.5], F), (n, 1)))  # du = U * pixel_mm


def test_frames_are_unit_and_orthogonal_on_the_tube_centreline():
    """a dozen binary64 operations on unit vectors give errors of order 2^-52; the bound is four thousand times that, and far below a
    float32 ulp"""
    parts = {}
    cr.curve_frames_literal(cp.tube_paths()[0], (1.0, 1.0, 1.0), 64, pixel_mm=0.25, station_mm=0.25, parts=parts)
    T, U = parts["T"], parts["U"]
    bound = 2.0 ** -40
    worst = (np.abs(np.sqrt((T * T).sum(axis=1)) - 1).max(), np.abs(np.sqrt((U * U).sum(axis=1)) - 1).max(), np.abs((T * U).sum(axis=1)).max())
    print("| |T| - 1 |, | |U| - 1 |, |T . U| at most %.3g %.3g %.3g over %d stations" % (worst + (len(T),)))
    assert len(T) > 200 and max(worst) <= bound


# ---- the point of the feature
def _tube_profile(points, smooth_passes):
    mask = cp.tube()[0]
    rows, s_mm, n = scene.curve_frames(points, (1.0, 1.0, 1.0), 64, pixel_mm=0.25, station_mm=0.25, smooth_passes=smooth_passes, slab_samples=64)
    return cr.section_records(mask, rows[:n], 64, 64, 0.25, connected=True), s_mm


def test_the_tube_has_its_radius_at_every_station_of_its_axis():
    """N(rho <= 4 - sqrt(3)/2 - 0.01) <= count <= N(rho <= 4 + sqrt(3)/2 + 0.01) with N the number of window grid points within rho of
    the window's centre: a sample's voxel centre lies within sqrt(3)/2 of the sample, the mask is "voxel centre within 4 of the axis
    circle", the section plane contains the torus's axis line, so the distance in the plane is the distance to the circle; 0.01 covers
    the float32 rows and the polyline's tangent.  The disc of the lower bound holds the centre and is connected."""
    records, s_mm = _tube_profile(cc.tube_axis_points(), 0)
    g = (np.arange(64) - 31.5) * 0.25
    rho = np.hypot(g[:, None], g[None, :])
    lower, upper = int((rho <= 4 - math.sqrt(3) / 2 - 0.01).sum()), int((rho <= 4 + math.sqrt(3) / 2 + 0.01).sum())
    inner = (s_mm >= 6.0) & (s_mm <= s_mm[-1] - 6.0)  # not within 6 voxels of the removed sector
    counts = records["count"][inner]
    measures = scene.profile_measures(records[inner], 0.25, 0.25)
    print("axis circle: %d stations, count %d .. %d within [%d, %d]; mean area %.2f mm^2 beside pi 4^2 = %.2f; mean diameter %.2f"
          % (inner.sum(), counts.min(), counts.max(), lower, upper, measures["area_mm2"].mean(), math.pi * 16, measures["diameter_mm"].mean()))
    assert inner.sum() > 250 and np.all(counts >= lower) and np.all(counts <= upper)
    assert not measures["cut"].any()
    traced, s2 = _tube_profile(cp.tube_paths()[0], 8)  # the same numbers for the traced centreline: a comparison, no threshold
    inner2 = (s2 >= 6.0) & (s2 <= s2[-1] - 6.0)
    m2 = scene.profile_measures(traced[inner2], 0.25, 0.25)
    print("traced centreline: %d stations, count %d .. %d; mean area %.2f mm^2; mean diameter %.2f"
          % (inner2.sum(), traced["count"][inner2].min(), traced["count"][inner2].max(), m2["area_mm2"].mean(), m2["diameter_mm"].mean()))


def test_profile_measures_by_hand():
    records = np.array([(4, 6, 10, 0), (0, 0, 0, 0), (64 * 64, 64 * 2016, 64 * 2016, 252)], scene.SECTION_RECORD_DTYPE)
    m = scene.profile_measures(records, 0.5, 0.25, width=64, slab_samples=64)
    assert np.array_equal(m["area_mm2"], [0.5, 0.0, 512.0]) and np.array_equal(m["cut"], [False, False, True])
    assert m["diameter_mm"][0] == 2.0 * math.sqrt(0.5 / math.pi) and m["diameter_mm"][1] == 0.0
    assert np.array_equal(m["offset_mm"][0], [(1.5 - 31.5) * 0.5, (2.5 - 31.5) * 0.25]) and np.isnan(m["offset_mm"][1]).all()
    assert np.array_equal(m["offset_mm"][2], [0.0, 0.0])


# ---- what the section cases reach
def test_the_section_cases_reach_what_they_are_for():
    name = {s: j for j, s in enumerate(cc.STATIONS)}
    conn, depths = cc.section_reference(64, 64, True)
    plain, _ = cc.section_reference(64, 64, False)
    assert tuple(conn[name["empty"]]) == tuple(plain[name["empty"]]) == (0, 0, 0, 0)
    full = (64 * 64, 64 * 2016, 64 * 2016, 252)
    assert tuple(conn[name["full"]]) == tuple(plain[name["full"]]) == full
    assert conn[name["clear centre"]]["count"] == 0 and plain[name["clear centre"]]["count"] == 64 * 64 - 256
    assert conn[name["two components"]]["count"] == 64 and plain[name["two components"]]["count"] == 64 + 140
    assert conn[name["touches the border"]]["border"] == 4 and conn[name["touches the border"]]["count"] == 160
    snake = name["serpentine"]
    assert conn[snake]["count"] == plain[snake]["count"] == 32 * 64 + 32 and depths[snake] > 1000, "many flood rounds"
    outside = name["partly outside"]
    assert 0 < conn[outside]["count"] < 64 * 64 and tuple(conn[outside]) == tuple(plain[outside]) and conn[outside]["border"] > 0
    assert conn[name["beyond z"]]["count"] == 0 and plain[name["beyond z"]]["count"] == 0
    assert tuple(conn[name["centre alone"]]) == (1, 32, 31, 0)
    oblique = slice(len(cc.STATIONS), None)
    assert np.all(conn[oblique]["count"] > 100) and np.all(conn[oblique]["count"] < plain[oblique]["count"]), "a component, and debris"
    for width, slab in cc.SECTION_SHAPES:
        c, _ = cc.section_reference(width, slab, True)
        p, _ = cc.section_reference(width, slab, False)
        assert tuple(c[name["full"]]) == tuple(p[name["full"]])
        assert c[name["full"]]["count"] == width * slab and c[name["full"]]["border"] == width * slab - max(width - 2, 0) * max(slab - 2, 0)
        assert np.all(c["count"] <= p["count"]) and np.all(c["sum_x"] <= p["sum_x"]) and len(c) == 13


def test_the_run_fill_identity_of_the_flood():
    """k_curve_profile fills the runs of set bits of S that hold a bit of R (a subset of S) by carry propagation, ((S ^ (S + R)) & S) | R
    upwards and the same on the bit-reversed words downwards: equal to spreading by shifts until nothing changes"""
    M = (1 << 64) - 1
    rev = lambda v: int(format(v, "064b")[::-1], 2)
    up = lambda s, r: ((s ^ ((s + r) & M)) & s) | r
    rng = np.random.default_rng(12)
    words = [int(v) for v in rng.integers(0, 1 << 63, size=6000, dtype=np.int64)]
    for i in range(0, len(words) - 3, 3):
        s = M if i % 30 == 0 else (words[i] << 1 | i & 1) & M | (words[i + 1] & words[i + 2])
        r = s & words[i + 1] & (words[i + 2] << 1)
        want = r
        while True:
            grown = (want | (want << 1) | (want >> 1)) & s & M
            if grown == want:
                break
            want = grown
        assert up(s, r) | rev(up(rev(s), rev(r))) == want, (hex(s), hex(r))


# ---- the library without a device
def test_the_entry_points_refuse_a_null_context_without_a_device():
    L = ffi.lib()
    curved, profile = ffi.CurvedDesc(), ffi.CurveProfileDesc()
    assert L.clwh_render_curved(None, C.byref(curved)) == 1 and L.clwh_curve_profile(None, C.byref(profile)) == 1  # CLWH_ERR_INVALID_VALUE
    assert L.clwh_render_curved(None, None) == 1 and L.clwh_curve_profile(None, None) == 1
    assert (C.sizeof(ffi.CurvedDesc), C.sizeof(ffi.CurveProfileDesc), C.sizeof(ffi.SectionRecord)) == (72, 64, 16)
    assert (ffi.CURVED_DENSE, ffi.PROFILE_CONNECTED) == (1, 1) and ffi.SECTION_RECORD_DTYPE == scene.SECTION_RECORD_DTYPE == cr.RECORD
