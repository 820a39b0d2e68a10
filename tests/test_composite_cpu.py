"""CPU checks of the compositing contract's restatement (tests/composite_ref.py), of the host-only table helper tf_composite_lut and
of the entry point's argument checks that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import composite_ref as cr
from tests import projection_ref as pr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _odd_table(rng, n):
    """alphas that are NaN, negative, zero, denormal, above 1 and infinite among ordinary ones; colours with a NaN and an infinity"""
    lut = rng.random((n, 4)).astype(F)
    lut[:, 3] *= F(0.4)
    special = [np.nan, -0.5, 0.0, -0.0, 1e-42, 1.5, np.inf, -np.inf, 1.0]
    where = rng.permutation(n)[:len(special)]
    lut[where, 3] = np.array(special, F)
    lut[rng.integers(0, n), 0] = np.nan
    lut[rng.integers(0, n), 1] = np.inf
    return lut


CASES = [
    ((5, 4, 3), (np.array([-3.0, 1.5, -2.0], F), scene.camera_direction(0.9, 6.183)), 0.37, (0.0, np.inf), 0.95),
    ((6, 7, 5), (np.array([2.5, 3.0, 2.0], F), scene.camera_direction(1.3, 0.2)), 0.5, (0.0, np.inf), 0.5),
    ((6, 6, 6), (np.array([3.0, 3.0, -4.0], F), np.array([0, 0, 1], F)), 1.0, (5.0, 8.0), np.inf),
    ((1, 1, 1), (np.array([0.5, 0.5, -2.0], F), np.array([0, 0, 1], F)), 0.5, (0.0, np.inf), 1.0),
    ((7, 3, 4), (np.array([-4.0, 5.0, 9.0], F), (np.array([7.5, -3.5, -7.0]) / np.linalg.norm([7.5, -3.5, -7.0])).astype(F)), 0.75,
     (1.0, 40.0), 0.95),
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("flags", [0, cr.SHADE])
@pytest.mark.parametrize("table", ["ordinary", "odd"])
def test_scalar_loop_and_vectorised_form_agree(case, flags, table):
    (X, Y, Z), (pos, d), step, (tn, tf), alpha_stop = CASES[case]
    rng = np.random.default_rng(X * 100 + Y * 10 + Z)
    vol = rng.integers(-6, 7, size=(Z, Y, X)).astype(np.int16)
    if table == "odd":
        lut, lut_first = _odd_table(rng, 16), -8
    else:
        lut, lut_first = rng.random((9, 4)).astype(F) * np.array([1, 1, 1, 0.5], F), -3  # values below -3 / above 5 clamp
        lut[2, 3] = 0
    fw, fh = 24, 16
    frame, rgba, t_first, t_stop, stats = cr.composite(vol, pos, d, (fw, fh), (fw, fh), lut, lut_first, step=step,
                                                       alpha_stop=alpha_stop, flags=flags, ambient=0.25, t_near=tn, t_far=tf)
    contributing = 0
    for y in range(fh):
        for x in range(fw):
            c, t1, t2 = cr.composite_scalar(vol, pos, d, (fw, fh), x, y, lut, lut_first, step=step, alpha_stop=alpha_stop, flags=flags,
                                            ambient=0.25, t_near=tn, t_far=tf)
            assert np.array_equal(_bits(rgba[y, x]), _bits(c)), (x, y)
            assert np.array_equal(_bits([t_first[y, x], t_stop[y, x]]), _bits([t1, t2])), (x, y)
            assert np.array_equal(frame[y, x], cr.quantise(c)), (x, y)
            contributing += not np.isnan(t1)
    assert contributing > 0 and stats["read"] <= stats["kept"]


def _one_voxel(alpha):
    vol = np.zeros((16, 16, 16), np.int16)
    vol[8, 8, 8] = 1000
    pos, d = np.array([8.5, 8.5, -10.0], F), np.array([0, 0, 1], F)
    lut = np.zeros((2048, 4), F)
    lut[1000] = (1.0, 0.5, 0.25, alpha)
    return vol, pos, d, lut


def test_known_answer_one_voxel_crossed_by_two_samples():
    a = F(0.3)
    vol, pos, d, lut = _one_voxel(a)
    frame, rgba, t_first, t_stop, _ = cr.composite(vol, pos, d, (16, 16), (16, 16), lut, 0)
    # pixel (8, 8) is the central ray; p.z = -10 + 0.5 k is in [8, 9) for k = 36, 37
    A = a + (F(1) - a) * a
    assert rgba[8, 8, 3] == A and t_first[8, 8] == 18.0 and np.isnan(t_stop[8, 8])
    assert np.array_equal(rgba[8, 8, :3], np.array([A, F(0) + a * F(0.5) + ((F(1) - a) * a) * F(0.5),
                                                     F(0) + a * F(0.25) + ((F(1) - a) * a) * F(0.25)], F))
    assert tuple(frame[8, 8]) == tuple(int(v * F(255) + F(0.5)) for v in rgba[8, 8])
    assert frame[8, 8, 3] == int(0.51 * 255 + 0.5)
    # a pixel whose ray misses the voxel: kept samples, nothing contributes
    assert tuple(frame[0, 0]) == (0, 0, 0, 0) and np.isnan(t_first[0, 0]) and not rgba[0, 0].any()


def test_known_answer_all_transparent_table():
    vol = scene.phantom(16)
    pos, d = scene.default_camera(16)
    for lut in (np.zeros((64, 4), F), np.full((64, 4), np.nan, F), -np.ones((64, 4), F)):
        frame, rgba, t_first, t_stop, stats = cr.composite(vol, pos, d, (32, 24), (32, 24), lut, 0)
        assert stats["kept"] > 0 and stats["read"] == stats["kept"]
        assert not frame.any() and not rgba.any() and np.isnan(t_first).all() and np.isnan(t_stop).all()


def test_known_answer_alpha_stop_reached_on_the_first_sample():
    vol, pos, d, lut = _one_voxel(0.97)
    frame, rgba, t_first, t_stop, _ = cr.composite(vol, pos, d, (16, 16), (16, 16), lut, 0, alpha_stop=0.95)
    assert t_first[8, 8] == 18.0 and t_stop[8, 8] == 18.0 and rgba[8, 8, 3] == F(0.97)  # the second sample (k = 37) is never read
    _, rgba_inf, _, t_stop_inf, _ = cr.composite(vol, pos, d, (16, 16), (16, 16), lut, 0, alpha_stop=np.inf)
    assert np.isnan(t_stop_inf[8, 8]) and rgba_inf[8, 8, 3] == F(0.97) + (F(1) - F(0.97)) * F(0.97)


def test_known_answer_constant_volume_has_no_gradient():
    vol = np.full((9, 10, 11), 7, np.int16)
    pos, d = scene.default_camera(11)
    lut = np.array([[0.2, 0.4, 0.6, 0.1]], F)
    plain = cr.composite(vol, pos, d, (32, 24), (32, 24), lut, 7, step=0.37)
    shaded = cr.composite(vol, pos, d, (32, 24), (32, 24), lut, 7, step=0.37, flags=cr.SHADE, ambient=0.1)
    for p, s in zip(plain[:4], shaded[:4]):
        assert np.array_equal(p.view(np.uint8), s.view(np.uint8))
    ka, kb = pr.kept_range(pos, d, (11, 10, 9), (32, 24), (32, 24), 0.37)
    assert np.array_equal(~np.isnan(plain[2]), ka <= kb) and (ka <= kb).sum() > 20
    assert np.array_equal(plain[2][ka <= kb], (ka.astype(F) * F(0.37))[ka <= kb])


def test_shading_darkens_a_face_seen_at_an_angle():
    vol = np.zeros((12, 12, 12), np.int16)
    vol[:, :, 6:] = 1000  # a wall whose normal is the x axis
    lut = np.zeros((1001, 4), F)
    lut[1000] = (1.0, 1.0, 1.0, 1.0)
    pos = np.array([-3.0, 6.5, 1.0], F)
    d = (np.array([1.0, 0.0, 1.0]) / np.sqrt(2.0)).astype(F)
    _, rgba, _, _, _ = cr.composite(vol, pos, d, (16, 16), (16, 16), lut, 0, flags=cr.SHADE, ambient=0.0, step=0.25)
    ray = pr.generate_ray(d, np.array(8), np.array(8), 16, 16)
    assert rgba[8, 8, 3] == 1 and rgba[8, 8, 0] == np.abs(F(1000.0) * ray[0]) / np.sqrt(F(1000.0) * F(1000.0))  # |cos| of the angle


def test_counts_on_the_64_cube_phantom():
    """pixels with 0 < A < alpha_stop, terminated pixels and samples read for phantom(64), 96x64, step 0.5, alpha_stop 0.95: the figures
    the feature was specified with (a second, independent implementation of the contract gave them), which the GPU families lean on"""
    vol = scene.phantom(64)
    quoted = {("default", "soft"): (1205, 0, 397787), ("default", "hard"): (57, 1148, 297061),
              ("close", "soft"): (5598, 0, 860859), ("close", "hard"): (180, 5418, 378773)}
    for (pose, name), (partial, terminated, read) in quoted.items():
        pos, d = scene.default_camera(64) if pose == "default" else scene.close_camera(64)
        table = cr.soft_table() if name == "soft" else cr.hard_table()
        _, rgba, _, t_stop, stats = cr.composite(vol, pos, d, (96, 64), (96, 64), table, -1024)
        A = rgba[..., 3]
        assert (int(((A > 0) & (A < F(0.95))).sum()), int((~np.isnan(t_stop)).sum()), stats["read"]) == (partial, terminated, read)


def _host_lib():
    L = C.CDLL(os.path.join(ROOT, "cl_volume_renderer_amd", "libclvr_host.so"))
    L.clvr_host_tf_composite_lut.restype = None
    L.clvr_host_tf_composite_lut.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_float)]
    return L


@pytest.mark.parametrize("rects", [
    [(500.0, 1200.0, 0.0, 4000.0, (1.0, 1.0, 1.0, 1.0))],
    [(500.0, 1200.0, 10.0, 20.0, (0.9, 0.1, 0.2, 0.5)), (1000.0, 1500.5, 0.0, 4000.0, (0.1, 0.2, 0.3, 1.0)),   # overlapping: first wins
     (-2000.0, -1000.0, 0.0, 4000.0, (0.3, 0.3, 0.3, 0.25)), (1100.0, 1100.0, 0.0, 1.0, (0.0, 1.0, 0.0, 1.0))],  # hidden by the first
    [],
])
def test_tf_composite_lut_equals_its_restatement(rects):
    lut_first, lut_len, opacity = -1024, 4096, 0.05
    flat = (C.c_float * max(8 * len(rects), 1))()
    for i, (lo, hi, glo, ghi, c) in enumerate(rects):
        flat[8 * i:8 * i + 8] = [lo, hi, glo, ghi] + list(c)
    out = np.full((lut_len, 4), 7, F)
    _host_lib().clvr_host_tf_composite_lut(flat, len(rects), lut_first, lut_len, opacity, out.ctypes.data_as(C.POINTER(C.c_float)))
    want = cr.tf_composite_lut([(lo, hi, c) for lo, hi, _, _, c in rects], lut_first, lut_len, opacity)
    assert np.array_equal(_bits(out), _bits(want))
    if rects:
        assert (want[:, 3] > 0).sum() >= 701 and tuple(out[1100 + 1024]) == tuple(want[500 + 1024])
        assert not out[499 + 1024].any() or len(rects) > 1


def test_composite_entry_point_refuses_null_arguments():
    L = ffi.lib()
    d = ffi.CompositeDesc()
    d.step, d.lut_len, d.alpha_stop = 0.5, 1, 0.95
    assert L.clwh_render_composite(None, C.byref(d)) == 1  # CLWH_ERR_INVALID_VALUE
    assert L.clwh_render_composite(None, None) == 1
    assert (ffi.COMP_DENSE, ffi.COMP_SHADE) == (1, 2) == (cr.DENSE, cr.SHADE)
    assert "clwh_render_composite" in ffi.EXPORTED_SYMBOLS
