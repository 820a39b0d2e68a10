"""CPU checks of the isosurface contract's restatement (tests/isosurface_ref.py): the vectorised form against the literal scalar
loop, the brick-skipping proof on random volumes, the refined depth and the normal on a ramp, the tie S == T on a constant volume,
and the exact S at the ends of int16 (the bounds the kernel's int32 blend stages rely on)."""
import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import isosurface_ref as ir
from tests import projection_ref as pr

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _toward(pos, target):
    v = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    return (v / np.linalg.norm(v)).astype(F)


CASES = [
    ((5, 4, 3), (np.array([-3.0, 1.5, -2.0], F), _toward((-3.0, 1.5, -2.0), (2.5, 2.0, 1.5))), 0.37, (0.0, np.inf)),
    ((6, 7, 5), (np.array([2.5, 3.0, 2.0], F), scene.camera_direction(1.3, 0.2)), 0.5, (0.0, np.inf)),
    ((6, 6, 6), (np.array([3.0, 3.0, -4.0], F), np.array([0, 0, 1], F)), 1.0, (5.0, 8.0)),
    ((1, 1, 1), (np.array([0.5, 0.5, -2.0], F), np.array([0, 0, 1], F)), 0.5, (0.0, np.inf)),
    ((9, 3, 4), (np.array([-4.0, 5.0, 9.0], F), _toward((-4.0, 5.0, 9.0), (4.5, 1.5, 2.0))), 0.75, (1.0, 40.0)),
]


def test_ffi_names_the_flags_of_the_header():
    assert (ffi.ISO_DENSE, ffi.ISO_BELOW) == (ir.DENSE, ir.BELOW) == (1, 2)
    assert "clwh_render_isosurface" in ffi.EXPORTED_SYMBOLS


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("flags", [0, ir.BELOW])
@pytest.mark.parametrize("refine", [0, 3, 24])
def test_scalar_loop_and_vectorised_form_agree(case, flags, refine):
    (X, Y, Z), (pos, d), step, (tn, tf) = CASES[case]
    rng = np.random.default_rng(X * 100 + Y * 10 + Z)
    vol = rng.integers(-300, 301, size=(Z, Y, X)).astype(np.int16)
    iso = 150.25 if not flags else -150.25
    if vol.size == 1:
        iso = float(vol[0, 0, 0])  # the tie, so that the one voxel is a hit
    fw, fh = 16, 8
    kw = dict(step=step, refine=refine, flags=flags, color=(0.9, 0.5, 1.7), ambient=0.25, t_near=tn, t_far=tf)
    frame, t_hit, normal, stats = ir.isosurface(vol, pos, d, (fw, fh), (fw, fh), iso, **kw)
    for y in range(fh):
        for x in range(fw):
            px, t, nrm = ir.isosurface_scalar(vol, pos, d, (fw, fh), x, y, iso, **kw)
            assert np.array_equal(frame[y, x], px), (x, y)
            assert np.array_equal(_bits(t_hit[y, x]), _bits(t)), (x, y)
            assert np.array_equal(_bits(normal[y, x]), _bits(nrm)), (x, y)
    assert stats["hit"].sum() > 0 and (stats["n"] > 0).sum() > 0
    assert np.array_equal(stats["hit"], ~np.isnan(t_hit)) and np.array_equal(stats["hit"], frame[..., 3] == 255)


@pytest.mark.parametrize("dims", [(19, 11, 13), (9, 17, 25)])
def test_dilated_brick_bounds_hold_for_every_kept_sample(dims):
    """the skip proof: dmin * 2^24 <= S <= dmax * 2^24 with the bounds of the sample's own brick, dilated by one voxel"""
    X, Y, Z = dims
    rng = np.random.default_rng(X + Y + Z)
    vol = rng.integers(-32768, 32768, size=(Z, Y, X)).astype(np.int16)
    dmin, dmax = ir.dilated_brick_bounds(vol)
    samples = 0
    for pos, d in ((np.array([-6.0, Y * 0.4, -5.0], F), _toward((-6.0, Y * 0.4, -5.0), (X / 2, Y / 2, Z / 2))),
                   (np.array([X * 0.5, Y * 0.5, Z * 0.5], F), scene.camera_direction(2.1, 0.4))):
        xs, ys = pr.pixel_grid((24, 16))
        dirs = pr.generate_ray(d, xs, ys, 24, 16).reshape(-1, 3)
        ka, kb = pr.kept_range_dirs(pos, dirs, dims, 0.37)
        for j in range(int((kb - ka).max()) + 1):
            idx = np.nonzero(ka + j <= kb)[0]
            _, p = pr._sample(pos, dirs[idx], ka[idx] + j, 0.37)
            S = ir.field_at(vol, p)
            b = p.astype(np.int64) >> 3
            assert np.all(dmin[b[:, 2], b[:, 1], b[:, 0]] << 24 <= S) and np.all(S <= dmax[b[:, 2], b[:, 1], b[:, 0]] << 24)
            samples += idx.size
    assert samples > 5000


@pytest.mark.parametrize("slope", [10, -10])
@pytest.mark.parametrize("refine", [0, 1, 8, 24])
def test_ramp_depth_is_refined_below_the_step_and_the_normal_is_the_axis(slope, refine):
    X, Y, Z = 40, 8, 8
    vol = np.broadcast_to((slope * np.arange(X)).astype(np.int16), (Z, Y, X)).copy()
    pos, d = np.array([-5.25, 4.3, 4.2], F), np.array([1, 0, 0], F)  # the central pixel's ray is d itself
    iso, step = 12.34 * slope, 0.7
    flags = ir.BELOW if slope < 0 else 0
    px, t_hit, nrm = ir.isosurface_scalar(vol, pos, d, (16, 8), 8, 4, iso, step=step, refine=refine, flags=flags, ambient=0.25)
    # The interpolated ramp is slope * (x - 0.5) for 0.5 <= x <= X - 0.5, so the analytic crossing is at x = 0.5 + iso / slope.  The 8-bit
    # weight floors the fraction of x - 0.5, so the fixed-point field lags the ramp by less than |slope| / 256 and crosses less than 1 / 256
    # later.  Bisection leaves a bracket of step / 2^refine whose upper end is t_hit.  Float32 rounding: t_k, the position and each of the
    # `refine` midpoints round once, each by at most one ulp of a number below 64 (2^-18); T = floor(iso * 2^24) adds less than 2^-24.
    t_cross = 0.5 + iso / slope - float(pos[0])
    bound = step / 2.0 ** refine + 1.0 / 256.0 + (refine + 4) * 2.0 ** -18
    assert -(refine + 4) * 2.0 ** -18 <= float(t_hit) - t_cross <= bound, (float(t_hit), t_cross, bound)
    assert np.array_equal(nrm[:3], np.array([np.sign(slope), 0, 0], F))
    assert abs(float(nrm[3]) - iso) <= abs(slope) * (step / 2.0 ** refine + 1.0 / 256.0) + 1e-3
    assert tuple(px) == (255, 255, 255, 255)  # the light is the ray: c = 1, s = 1
    frame, t_vec, n_vec, stats = ir.isosurface(vol, pos, d, (16, 8), (16, 8), iso, step=step, refine=refine, flags=flags, ambient=0.25)
    assert np.array_equal(_bits(t_vec[4, 8]), _bits(t_hit)) and np.array_equal(_bits(n_vec[4, 8]), _bits(nrm))
    assert stats["refined"][4, 8]


@pytest.mark.parametrize("flags", [0, ir.BELOW])
def test_constant_volume_ties_hit_at_the_first_kept_sample(flags):
    X, Y, Z = 12, 9, 7
    v = 137
    vol = np.full((Z, Y, X), v, np.int16)
    pos, d = np.array([-4.0, 3.0, -6.0], F), _toward((-4.0, 3.0, -6.0), (6.0, 4.5, 3.5))
    wh = (32, 24)
    ka, kb = pr.kept_range(pos, d, (X, Y, Z), wh, wh, 0.5)
    entered = ka <= kb
    assert entered.sum() > 50 and (~entered).sum() > 50
    frame, t_hit, normal, stats = ir.isosurface(vol, pos, d, wh, wh, float(v), flags=flags, color=(0.2, 0.4, 0.6))
    assert np.array_equal(stats["hit"], entered) and np.array_equal(stats["first"], entered) and np.array_equal(stats["flat"], entered)
    assert np.array_equal(_bits(t_hit[entered]), _bits(ka[entered].astype(F) * F(0.5)))
    assert np.all(normal[entered][:, :3] == 0) and np.all(normal[entered][:, 3] == F(v))
    assert np.all(frame[entered] == np.array([51, 102, 153, 255], np.uint8)) and np.all(frame[~entered] == 0)
    beyond = np.nextafter(F(v), F(np.inf) if not flags else F(-np.inf))  # the next float past v on the far side of the tie
    frame, t_hit, normal, stats = ir.isosurface(vol, pos, d, wh, wh, beyond, flags=flags)
    assert not stats["hit"].any() and np.isnan(t_hit).all() and np.all(frame == 0)
    assert np.all(_bits(normal) == 0x7FC00000)


def _staged_blend(vol, p):
    """the blend in the kernel's stages, in int64, with the bounds the kernel's int32 x and y stages rely on"""
    Z, Y, X = vol.shape
    i0, w = ir.cell(p)
    top = np.array([X - 1, Y - 1, Z - 1], np.int64)
    lo, hi = np.maximum(i0, 0), np.minimum(i0 + 1, top)

    def V(cx, cy, cz):
        return vol[cz, cy, cx].astype(np.int64)

    stage_y = []
    for cz in (lo[:, 2], hi[:, 2]):
        stage_x = [V(lo[:, 0], cy, cz) * (256 - w[:, 0]) + V(hi[:, 0], cy, cz) * w[:, 0] for cy in (lo[:, 1], hi[:, 1])]
        assert all(np.abs(s).max() <= 1 << 23 for s in stage_x)
        stage_y.append(stage_x[0] * (256 - w[:, 1]) + stage_x[1] * w[:, 1])
    assert all(s.min() >= -(1 << 31) and s.max() <= (1 << 31) - 1 for s in stage_y)
    return stage_y[0] * (256 - w[:, 2]) + stage_y[1] * w[:, 2]


def test_exact_field_at_the_ends_of_int16():
    X, Y, Z = 11, 7, 9
    rng = np.random.default_rng(3)
    p = (rng.random((4000, 3)) * np.array([X, Y, Z])).astype(F)
    p = np.minimum(p, np.nextafter(np.array([X, Y, Z], F), F(0)))
    lowest = np.full((Z, Y, X), -32768, np.int16)
    S = ir.field_at(lowest, p)
    assert np.all(S == -(1 << 39)) and np.array_equal(_staged_blend(lowest, p), S)
    highest = np.full((Z, Y, X), 32767, np.int16)
    assert np.all(ir.field_at(highest, p) == 32767 << 24) and np.array_equal(_staged_blend(highest, p), ir.field_at(highest, p))
    z, y, x = np.indices((Z, Y, X))
    checker = np.where((x + y + z) & 1, 32767, -32768).astype(np.int16)
    S = ir.field_at(checker, p)
    assert np.array_equal(_staged_blend(checker, p), S)
    i0, w = ir.cell(p)
    for m in range(0, 4000, 97):  # the same sums in Python integers
        want = 0
        for corner in range(8):
            bits = (corner & 1, (corner >> 1) & 1, corner >> 2)
            c = [min(max(int(i0[m, a]) + bits[a], 0), (X, Y, Z)[a] - 1) for a in range(3)]
            wt = 1
            for a in range(3):
                wt *= int(w[m, a]) if bits[a] else 256 - int(w[m, a])
            want += wt * int(checker[c[2], c[1], c[0]])
        assert int(S[m]) == want
    assert S.min() < -(1 << 37) and S.max() > 1 << 37  # both signs, near the ends
    # a hit decision at the extremes: iso = -32768 ties everywhere on the lowest volume, iso = 32767 on the highest
    assert ir.threshold(-32768.0) == -(1 << 39) and ir.threshold(65536.0) == 1 << 40 and ir.threshold(-65536.0) == -(1 << 40)
