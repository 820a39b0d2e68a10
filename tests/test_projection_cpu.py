"""CPU checks of the intensity-projection contract's restatement (tests/projection_ref.py) and of the entry point's argument checks
that need no device."""
import ctypes as C

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import projection_ref as pr

F = np.float32

POSES = [
    scene.default_camera(64),
    scene.close_camera(64),
    (np.array([31.5, 32.25, 30.0], F), scene.camera_direction(2.1, 0.4)),
    (np.array([32.0, 32.0, -10.0], F), np.array([0, 0, 1], F)),
    (np.array([-5.0, 70.0, 3.0], F), scene.camera_direction(-0.7, 5.5)),
]


@pytest.mark.parametrize("pose", range(len(POSES)))
def test_vectorised_generate_ray_equals_the_oracles(orc, pose):
    pos, d = POSES[pose]
    fw, fh = 96, 72
    xs, ys = np.meshgrid(np.arange(0, fw, 5), np.arange(0, fh, 7))
    got = pr.generate_ray(d, xs, ys, fw, fh)
    L = orc.lib()
    p3, d3, out = (C.c_float * 3)(*pos), (C.c_float * 3)(*d), (C.c_float * 3)()
    for (y, x), g in np.ndenumerate(np.zeros(xs.shape)):
        L.orc_generate_ray(p3, d3, int(xs[y, x]), int(ys[y, x]), fw, fh, out)
        want = np.array(list(out), F)
        assert np.array_equal(got[y, x].view(np.uint32), want.view(np.uint32)), (x, y)


@pytest.mark.parametrize("case", [
    ((5, 4, 3), (np.array([-3.0, 1.5, -2.0], F), scene.camera_direction(0.9, 6.183)), 0.37, (0.0, np.inf)),
    ((6, 7, 5), (np.array([2.5, 3.0, 2.0], F), scene.camera_direction(1.3, 0.2)), 0.5, (0.0, np.inf)),
    ((6, 6, 6), (np.array([3.0, 3.0, -4.0], F), np.array([0, 0, 1], F)), 1.0, (5.0, 8.0)),
    ((1, 1, 1), (np.array([0.5, 0.5, -2.0], F), np.array([0, 0, 1], F)), 0.5, (0.0, np.inf)),
    ((7, 3, 4), (np.array([-4.0, 5.0, 9.0], F), (np.array([7.5, -3.5, -7.0]) / np.linalg.norm([7.5, -3.5, -7.0])).astype(F)), 0.75,
     (1.0, 40.0)),
])
def test_scalar_loop_and_vectorised_form_agree(case):
    (X, Y, Z), (pos, d), step, (tn, tf) = case
    rng = np.random.default_rng(X * 100 + Y * 10 + Z)
    vol = rng.integers(-5, 6, size=(Z, Y, X)).astype(np.int16)
    fw, fh = 24, 16
    got = pr.project(vol, pos, d, (fw, fh), (fw, fh), modes=(pr.MAX, pr.MIN, pr.MEAN), step=step, t_near=tn, t_far=tf)
    kept_pixels = 0
    for y in range(fh):
        for x in range(fw):
            for mode in (pr.MAX, pr.MIN, pr.MEAN):
                v, t = pr.project_scalar(vol, pos, d, (fw, fh), x, y, mode, step, tn, tf)
                gv, gt = got[mode][1][y, x], got[mode][2][y, x]
                assert np.array_equal(np.array([gv, gt], F).view(np.uint32), np.array([v, t], F).view(np.uint32)), (x, y, mode)
            kept_pixels += not np.isnan(got[pr.MAX][1][y, x])
    assert kept_pixels > 0


def _one_bright_voxel():
    vol = np.zeros((16, 16, 16), np.int16)
    vol[8, 8, 8] = 1000
    pos, d = np.array([8.5, 8.5, -10.0], F), np.array([0, 0, 1], F)
    return vol, pos, d


def test_known_answer_bright_voxel_on_the_central_ray():
    vol, pos, d = _one_bright_voxel()
    fw, fh = 16, 16  # pixel (8, 8) is the central ray: d itself
    out = pr.project(vol, pos, d, (fw, fh), (fw, fh), modes=(pr.MAX, pr.MIN, pr.MEAN), window_cw=(500.0, 1000.0))
    frame, values, t = out[pr.MAX]
    # p.z = -10 + 0.5 k is in [8, 9) for k = 36, 37; the first of them wins
    assert values[8, 8] == 1000 and t[8, 8] == 18.0
    assert tuple(frame[8, 8]) == (255, 255, 255, 255)
    assert out[pr.MIN][1][8, 8] == 0 and out[pr.MIN][2][8, 8] == 10.0  # first kept sample: p.z = 0
    assert out[pr.MEAN][1][8, 8] == F(1000.0 * 2 / 32)  # 32 kept samples, two of them in the bright voxel
    assert np.isnan(out[pr.MEAN][2][8, 8])


def test_known_answer_slab_excludes_the_bright_voxel():
    vol, pos, d = _one_bright_voxel()
    out = pr.project(vol, pos, d, (16, 16), (16, 16), modes=(pr.MAX,), t_near=0.0, t_far=17.75, window_cw=(500.0, 1000.0))
    frame, values, t = out[pr.MAX]
    assert values[8, 8] == 0 and t[8, 8] == 10.0
    assert tuple(frame[8, 8]) == (0, 0, 0, 255)  # u = (-0.5 + 0.5) * 255 + 0.5 -> 0
    # a slab entirely before the volume keeps nothing
    out = pr.project(vol, pos, d, (16, 16), (16, 16), modes=(pr.MAX,), t_near=0.0, t_far=9.75)
    assert np.isnan(out[pr.MAX][1][8, 8]) and np.isnan(out[pr.MAX][2][8, 8]) and tuple(out[pr.MAX][0][8, 8]) == (0, 0, 0, 0)


def test_known_answer_constant_volume_first_kept_sample():
    vol = np.full((9, 10, 11), 7, np.int16)
    pos, d = scene.default_camera(11)
    fw, fh = 32, 24
    out = pr.project(vol, pos, d, (fw, fh), (fw, fh), modes=(pr.MAX, pr.MIN, pr.MEAN), step=0.37)
    ka, kb = pr.kept_range(pos, d, (11, 10, 9), (fw, fh), (fw, fh), 0.37)
    hit = ka <= kb
    assert hit.sum() > 20
    first_t = ka.astype(F) * F(0.37)
    for mode in (pr.MAX, pr.MIN):
        assert np.all(out[mode][1][hit] == 7) and np.array_equal(out[mode][2][hit], first_t[hit])
        assert np.all(np.isnan(out[mode][1][~hit]))
    assert np.all(out[pr.MEAN][1][hit] == 7)


def test_kept_range_is_the_set_of_kept_samples():
    pos, d = POSES[4]
    ka, kb = pr.kept_range(pos, d, (20, 9, 13), (40, 32), (40, 32), 0.37, 1.0, 60.0)
    xs, ys = pr.pixel_grid((40, 32))
    dirs = pr.generate_ray(d, xs, ys, 40, 32)
    for k in range(0, 260):
        want = pr.kept(pos, dirs, np.full(xs.shape, k), 0.37, (20, 9, 13), 1.0, 60.0)
        assert np.array_equal(want, (ka <= k) & (k <= kb)), k


def test_projection_entry_point_refuses_null_arguments():
    L = ffi.lib()
    d = ffi.ProjectionDesc()
    d.mode, d.step, d.window_width = ffi.PROJ_MAX, 0.5, 1.0
    assert L.clwh_render_projection(None, C.byref(d)) == 1  # CLWH_ERR_INVALID_VALUE
    assert L.clwh_render_projection(None, None) == 1
    assert ffi.DERIVED_PROJECTION == 4 and (ffi.PROJ_MAX, ffi.PROJ_MIN, ffi.PROJ_MEAN, ffi.PROJ_DENSE) == (0, 1, 2, 1)
