"""CPU checks of the slice contract's restatement (tests/slice_ref.py) and of what sits above the C ABI: the vectorised form against
the literal scalar loop, the running-extreme skip proof on random volumes, the voxel-centre identity, MEAN at the ends of int16,
scene.slice_plane, and -- with the reference alone -- the tally of every family tests/test_gpu_slice.py compares on the GPU, so that
none of its comparisons can be empty."""
import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import slice_ref as sr
from tests import test_gpu_slice as gs
from tests.test_isosurface_cpu import CASES

F = np.float32
MODES = (sr.MAX, sr.MIN, sr.MEAN)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_ffi_names_the_values_of_the_header():
    assert (ffi.SLICE_MAX, ffi.SLICE_MIN, ffi.SLICE_MEAN) == (sr.MAX, sr.MIN, sr.MEAN) == (0, 1, 2)
    assert ffi.SLICE_DENSE == sr.DENSE == 1
    assert "clwh_render_slice" in ffi.EXPORTED_SYMBOLS
    d = ffi.SliceDesc()
    assert (d.slab_samples, d.step, len(d.origin), len(d.normal)) == (0, 0.0, 3, 3)
    import os
    header = open(os.path.join(gs.ROOT, "include", "clwh.h")).read()
    assert "CLWH_SLICE_MAX = 0, CLWH_SLICE_MIN = 1, CLWH_SLICE_MEAN = 2" in header and "CLWH_SLICE_DENSE = 1" in header
    assert "int clwh_render_slice(clwh_ctx *ctx, const clwh_slice_desc *desc);" in header


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("n", [1, 5, 33])
def test_scalar_loop_and_vectorised_form_agree(case, n):
    (X, Y, Z), _, step, _ = CASES[case]
    rng = np.random.default_rng(X * 100 + Y * 10 + Z + n)
    vol = rng.integers(-300, 301, size=(Z, Y, X)).astype(np.int16)
    w, h = 16, 8
    origin, du, dv, normal = gs.oblique((X, Y, Z), (w, h), n=n, step=step, a=0.3 + case, b=0.2 * case, spacing=1.4 * max(X, Y, Z) / w)
    window = (10.0, 500.0)
    out, stats = sr.slice_view(vol, origin, du, dv, normal, (w, h), modes=MODES, slab_samples=n, step=step, window_cw=window, chunk=7)
    for mode in MODES:
        frame, values, t_ext = out[mode]
        for y in range(h):
            for x in range(w):
                px, v, t = sr.slice_scalar(vol, origin, du, dv, normal, x, y, mode, slab_samples=n, step=step, window_cw=window)
                assert np.array_equal(frame[y, x], px), (mode, x, y)
                assert np.array_equal(_bits(values[y, x]), _bits(v)) and np.array_equal(_bits(t_ext[y, x]), _bits(t)), (mode, x, y)
        assert np.array_equal(stats["none"], np.isnan(values)) and np.array_equal(stats["none"], frame[..., 3] == 0)
    assert (~stats["none"]).sum() > 0
    assert np.array_equal(stats["none"] | stats["cut"] | stats["full"], np.ones((h, w), bool))


@pytest.mark.parametrize("dims", [(19, 11, 13), (9, 17, 25)])
def test_no_sample_of_a_skipped_brick_changes_the_running_extreme(dims):
    """the skip proof: once best exists and dmax * 2^24 <= best (MIN: dmin * 2^24 >= best) at the ray's first sample in a brick, no
    sample of the ray in that brick is larger (smaller) than best"""
    X, Y, Z = dims
    rng = np.random.default_rng(X + Y + Z)
    vol = rng.integers(-32768, 32768, size=(Z, Y, X)).astype(np.int16)
    samples = skipped = 0
    for a, b, n, step in ((0.6, 0.35, 60, 0.37), (2.0, -0.5, 40, 0.5), (0.1, 1.2, 25, 1.3)):
        origin, du, dv, normal = gs.oblique(dims, (24, 16), n=n, step=step, a=a, b=b, spacing=1.2 * max(dims) / 24)
        _, stats = sr.slice_view(vol, origin, du, dv, normal, (24, 16), slab_samples=n, step=step)
        assert stats["skip_changed"] == {sr.MAX: 0, sr.MIN: 0}
        samples += stats["samples"]
        skipped += sum(stats["skipped"].values())
    assert samples > 5000 and skipped > 0, (samples, skipped)


def test_thin_axial_slice_through_voxel_centres_is_the_plane():
    cases = gs.axis_cases()[11:]
    assert len(cases) == 9
    for z, c in enumerate(cases):
        out, stats = gs.reference_of(c)
        for mode in MODES:
            values = out[mode][1]
            assert np.array_equal(values[:10, :12], c["vol"][z].astype(F))  # all weights are 0: value == (float)V
        assert stats["full"].sum() == 120 and stats["none"].sum() == 16 * 16 - 120


@pytest.mark.parametrize("v", [32767, -32768])
def test_mean_of_8192_samples_at_the_ends_of_int16(v):
    vol = np.full((8, 8, 8), v, np.int16)
    out, stats = sr.slice_view(vol, (0.3, 0.4, 3.7), (0.9, 0, 0), (0, 0.9, 0), (0, 0, 0), (8, 8), modes=MODES, slab_samples=8192, step=0.5)
    assert stats["full"].all() and stats["samples"] == 64 * 8192
    for mode in MODES:
        assert np.all(out[mode][1] == F(v))
    assert np.all(out[sr.MAX][2] == 0) and np.isnan(out[sr.MEAN][2]).all() and stats["tie"][sr.MAX].all()
    px, value, t = sr.slice_scalar(vol, (0.3, 0.4, 3.7), (0.9, 0, 0), (0, 0.9, 0), (0, 0, 0), 3, 5, sr.MEAN, slab_samples=8192)
    assert value == F(v) and 8192 * abs(v) << 24 <= 1 << 52


@pytest.mark.parametrize("orientation", ["axial", "coronal", "sagittal"])
@pytest.mark.parametrize("dims,wh", [((48, 40, 36), (256, 128)), ((20, 70, 33), (64, 96)), ((512, 512, 512), (1920, 1080))])
def test_slice_plane_is_centred_on_the_position_and_fits_the_region(orientation, dims, wh):
    iu, iv, iw = scene.SLICE_AXES[orientation]
    w, h = wh
    position, n, step = 11.25, 33, 0.37
    origin, du, dv, normal = scene.slice_plane(dims, orientation, position, w, h, slab_samples=n, step=step)
    assert all(v.dtype == F and v.shape == (3,) for v in (origin, du, dv, normal))
    o, u, v, nn = (a.astype(np.float64) for a in (origin, du, dv, normal))
    # the middle of the region (between the four central pixels), half the slab in: the volume's centre line at the position
    mid = o + u * (w - 1) / 2 + v * (h - 1) / 2 + nn * ((n - 1) / 2 * float(F(step)))
    want = np.zeros(3)
    want[iu], want[iv], want[iw] = dims[iu] / 2, dims[iv] / 2, position + 0.5
    assert np.allclose(mid, want, rtol=0, atol=1e-3)
    assert np.count_nonzero(u) == 1 and np.count_nonzero(v) == 1 and u[iu] == v[iv] > 0 and np.array_equal(nn, np.eye(3)[iw])
    # the cross-section [0, dim] lies inside the pixels' footprint on both axes, and touches it on one
    lo_u, hi_u = o[iu] - u[iu] / 2, o[iu] + u[iu] * (w - 0.5)
    lo_v, hi_v = o[iv] - v[iv] / 2, o[iv] + v[iv] * (h - 0.5)
    eps = 1e-3
    assert lo_u <= eps and hi_u >= dims[iu] - eps and lo_v <= eps and hi_v >= dims[iv] - eps
    assert abs(lo_u) <= eps or abs(lo_v) <= eps
    thin = scene.slice_plane(dims, orientation, 7.0, w, h)
    assert thin[0][iw] == F(7.5)  # through the centres of the voxels with index 7


def test_slice_plane_feeds_the_reference():
    dims = (12, 10, 9)
    vol = np.random.default_rng(5).integers(-2000, 2000, size=(9, 10, 12)).astype(np.int16)
    plane = scene.slice_plane(dims, "axial", 4.0, 24, 24)
    out, stats = sr.slice_view(vol, *plane, (24, 24), modes=(sr.MAX,))
    values = out[sr.MAX][1]
    assert stats["full"].sum() == 24 * 20  # spacing 0.5: the 12 x 10 cross-section covers 24 x 20 pixels
    assert set(np.unique(values[~np.isnan(values)] * 16) % 1) == {0.0}  # weights 0.25 and 0.75 on two axes


def test_every_gpu_family_exercises_every_kind():
    for cases in (gs.phantom_cases(), gs.random_cases(), gs.axis_cases()):
        gs.reference_tally(cases).assert_all()
    assert all(gs.reference_of(c)[1]["none"].all() for c in gs.random_cases()[2::3])
    gs.check_axis_expectations(gs.axis_cases())
    gs.check_window_expectations(gs.window_cases())
    quiet = gs.reference_tally(gs.phantom_cases()[-2:])
    assert quiet.skipped > 0  # whole bricks of the noise-free phantom are stepped over at entry
    a, b = gs.derived_data_volumes()
    stale = 0
    for vol in (a, b):
        stats = gs.reference_of(gs.derived_data_case(vol))[1]
        assert sum(stats["skipped"].values()) > 0 and stats["cut"].sum() > 0
    # a table left over from `a` would skip bricks of `b` that hold its maximum: the rule with a's bounds on b's samples is wrong
    c = gs.derived_data_case(b)
    from tests import isosurface_ref as ir
    real = ir.dilated_brick_bounds
    try:
        ir.dilated_brick_bounds = lambda vol: real(a)
        _, stats = sr.slice_view(b, c["origin"], c["du"], c["dv"], c["normal"], c["region_wh"], slab_samples=c["n"], step=c["step"])
        stale = sum(stats["skip_changed"].values())
    finally:
        ir.dilated_brick_bounds = real
    assert stale > 0
