"""-m gpu: SDF builder on the MI355X through the C ABI, against the reference's golden vector and the oracle."""
import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests.sdf_event_cases import blobs as _blobs
from tests.sdf_event_cases import reference_host_loop

pytestmark = pytest.mark.gpu


def _upload(ctx, vol):
    Z, Y, X = vol.shape
    v = ctx.image_from(vol.astype(np.int16))
    s = ctx.image([X, Y, Z], 1, np.int8, (Z, Y, X))
    return v, s


def test_fused_build_matches_reference_golden_vector(gpu_ctx, sdf_golden):
    """reference tests/sdf/sdf_test.cpp:6-33 re-run on the HIP path: exact."""
    vol, gold = sdf_golden
    v, s = _upload(gpu_ctx, vol)
    n = gpu_ctx.sdf_build(v, scene.TF_TEST_VALUE_GT_800, s)
    out = s.pull()
    assert np.array_equal(out.reshape(-1).astype(np.int32), gold)
    assert n == 13
    v.release(); s.release()


def test_reference_host_loop_over_the_generic_launch(gpu_ctx, sdf_golden):
    """app/signed_distance_field.cpp:7-35 re-enacted call by call over clwh_kernel_get / clwh_launch,
    i.e. what the reference's unmodified host code would do through the clw_* wrappers."""
    vol, gold = sdf_golden
    launches, out = reference_host_loop(gpu_ctx, vol, scene.TF_TEST_VALUE_GT_800)
    assert launches == 13
    assert np.array_equal(out.reshape(-1).astype(np.int32), gold)


@pytest.mark.parametrize("dims,tf", [
    ((64, 64, 64), "default"), ((64, 64, 64), "gradient"), ((70, 33, 45), "default"), ((40, 96, 24), "gradient"),
])
def test_fused_build_matches_oracle(gpu_ctx, orc, dims, tf):
    src = scene.tf_default_source() if tf == "default" else scene.tf_gradient_source()
    vol = scene.phantom(max(dims), dims=dims)
    want, n_want, _ = orc.sdf_build(vol, orc.parse_tf(src))
    v, s = _upload(gpu_ctx, vol)
    n = gpu_ctx.sdf_build(v, src, s)
    got = s.pull()
    assert np.array_equal(got, want)
    assert n == n_want
    v.release(); s.release()


def test_degenerate_volumes(gpu_ctx, orc):
    """all-event and no-event volumes: nothing to propagate, the loop stops at the first odd layer."""
    for fill in (-1000, 900):
        vol = np.full((16, 16, 16), fill, np.int16)
        want, n_want, _ = orc.sdf_build(vol, orc.parse_tf(scene.tf_default_source()))
        v, s = _upload(gpu_ctx, vol)
        n = gpu_ctx.sdf_build(v, scene.tf_default_source(), s)
        assert np.array_equal(s.pull(), want) and n == n_want == 1
        v.release(); s.release()


def test_unknown_kernel_and_bad_ndrange_are_reported(gpu_ctx):
    with pytest.raises(ffi.ClwhError) as e:
        gpu_ctx.kernel("2d_image_filter.cl", "bilateral_filter")
    assert e.value.status == 5
    k = gpu_ctx.kernel("empty.cl", "empty")
    with pytest.raises(ffi.ClwhError) as e:
        k.launch([10, 8, 1], [4, 4, 1])  # clw_function.hpp:235 asserts global % local == 0
    assert e.value.status == 8
    k.release()


def test_full_sdf_at_256_equals_the_oracle(gpu_ctx, orc):
    """every one of the 16.8 M values and the reference's launch count, against the oracle run here (about 15 s of CPU)"""
    vol = scene.phantom(256)
    tf = scene.tf_default_source()
    v, s = _upload(gpu_ctx, vol)
    n = gpu_ctx.sdf_build(v, tf, s)
    want, launches, _ = orc.sdf_build(vol, orc.parse_tf(tf))
    assert np.array_equal(s.pull(), want)
    assert n == launches
    v.release(); s.release()


@pytest.mark.parametrize("tf_name", ["default", "gradient"])
def test_sdf_at_512_equals_the_committed_oracle_checksum(gpu_ctx, golden_dir, tf_name):
    """the SDF the headline benchmark marches through (512^3; the 7-tap gradient TF of config 3 too): SHA-256, sums
    and launch count of the ORACLE's field, computed once in the build container (5 min of CPU each,
    tests/golden/make_sdf_checksums.py) and committed -- byte-for-byte equality without re-running the oracle."""
    import hashlib
    import json
    import os

    want = json.load(open(os.path.join(golden_dir, "sdf_phantom_checksums.json")))["phantom(512) %s tf" % tf_name]
    vol = scene.phantom(512)
    tf = scene.tf_default_source() if tf_name == "default" else scene.tf_gradient_source()
    v, s = _upload(gpu_ctx, vol)
    n = gpu_ctx.sdf_build(v, tf, s)
    sdf = s.pull()
    assert n == want["launches"]
    assert int(sdf.astype(np.int64).sum()) == want["sum"]
    assert hashlib.sha256(sdf.tobytes()).hexdigest() == want["sha256"]
    v.release(); s.release()


@pytest.mark.parametrize("variant", ["bits", "bits16", "bits_rec_lds", "front"])
@pytest.mark.parametrize("dims", [(200, 170, 150), (65, 49, 17), (2, 40, 40), (130, 3, 7), (31, 97, 129)])
def test_every_build_variant_on_awkward_shapes(gpu_ctx, gpu_ctx_sdf_waves16, gpu_ctx_sdf_rec_lds, gpu_ctx_sdf_front, orc, variant, dims):
    """The bit-parallel build works on regions of 64 x 48 x 16 (or 48) voxels with 8-voxel halos, rows of 32-bit words and a
    clamped neighbourhood at the faces: sizes that are no multiple of any of these, one-voxel-thick volumes, and surfaces that
    run into the faces -- every value and the reference's launch count against the oracle, for all build paths (the 8-wave
    blocks also with their layer records in LDS)."""
    ctx = {"bits": gpu_ctx, "bits16": gpu_ctx_sdf_waves16, "bits_rec_lds": gpu_ctx_sdf_rec_lds, "front": gpu_ctx_sdf_front}[variant]
    vol = _blobs(dims, seed=sum(dims))
    tf = scene.tf_default_source()
    want, n_want, _ = orc.sdf_build(vol, orc.parse_tf(tf))
    v, s = _upload(ctx, vol)
    n = ctx.sdf_build(v, tf, s)
    got = s.pull()
    assert np.array_equal(got, want)
    assert n == n_want
    assert (np.abs(want.astype(np.int32)) > 1).any() or min(dims) < 4  # something was propagated
    v.release(); s.release()


@pytest.mark.parametrize("dims", [(512, 17, 6), (1024, 20, 5), (2048, 5, 3)])
def test_wide_rows_take_the_sixteen_row_seed_and_expand_kernels(gpu_ctx, orc, dims):
    """Rows of 16 / 32 / 64 words (X = 512 / 1024 / 2048) are seeded by k_sdfbit_seed_rows16<16 / 32 / 64> and expanded by
    k_sdfbit_expand16_rows16<32 / 64 / 64>: launch branches that only wide volumes reach.  Y is no multiple of 16, so the last block of
    sixteen rows leaves early for some of them; max_iterations is 127, so all sixteen layer launches run.  Every value and the
    reference's launch count against the oracle."""
    vol = _blobs(dims, seed=sum(dims) + 1)  # (+ 1: the blobs of seed sum(dims) fill (1024, 20, 5) completely -- nothing to build)
    tf = scene.tf_default_source()
    want, n_want, _ = orc.sdf_build(vol, orc.parse_tf(tf))
    v, s = _upload(gpu_ctx, vol)
    n = gpu_ctx.sdf_build(v, tf, s)
    got = s.pull()
    assert np.array_equal(got, want)
    assert n == n_want
    assert (np.abs(want.astype(np.int32)) > 1).any() or min(dims) < 4  # something was propagated
    v.release(); s.release()


def test_rebuild_after_a_transfer_function_change(gpu_ctx, orc):
    """the build's scratch (bit sets, block states, lists) is reused across builds: a second build with another table must not see the first"""
    vol = scene.phantom(96)
    v, s = _upload(gpu_ctx, vol)
    for src in (scene.tf_default_source(), scene.tf_gradient_source(), scene.tf_default_source()):
        want, n_want, _ = orc.sdf_build(vol, orc.parse_tf(src))
        n = gpu_ctx.sdf_build(v, src, s)
        assert np.array_equal(s.pull(), want) and n == n_want
    v.release(); s.release()
