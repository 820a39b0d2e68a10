"""-m gpu: every copy of the event test is_event_gen(value, (short)|gradient|) the SDF builders hold -- event_at<true> under
k_sdfbit_events (X % 8 != 0), k_sdf_base_front and the generic launch's k_sdf_base, the eight-voxel k_sdfbit_events8<true> with its
own neighbour loads, and the hiprtc classifier whose class bytes replace them all for source outside the rule grammar -- on inputs
where the zero border texel, the gradient clause and the wrap of the short decide events (tests/sdf_event_cases.py; that they do is
asserted without a GPU in tests/test_sdf_event_cases_cpu.py).  Every value and the reference's launch count against the oracle,
bit for bit; the oracle runs once per (volume, table)."""
import numpy as np
import pytest

from cl_volume_renderer_amd import ffi
from tests import packed_scene_ref as ps
from tests import sdf_event_cases as ec
from tests.test_gpu_packed_scene import Build, _compare

pytestmark = pytest.mark.gpu


def _build(ctx, v, source, dims):
    """one clwh_sdf_build into an image that held zeros (no value of a finished field): (field, launches)"""
    X, Y, Z = dims
    s = ctx.image([X, Y, Z], 1, np.int8, (Z, Y, X))
    s.push(np.zeros((Z, Y, X), np.int8))
    n = ctx.sdf_build(v, source, s)
    out = s.pull()
    s.release()
    return out, n


def _check(got, want, what):
    (field, n), (want_field, want_n) = got, want
    if not np.array_equal(field, want_field):
        at = tuple(np.argwhere(field != want_field)[0])
        pytest.fail("%s: %d values differ, first at (z, y, x) %s: got %d, want %d" % (what, int((field != want_field).sum()), at, field[at], want_field[at]))
    assert n == want_n, what


@pytest.mark.parametrize("route", ["rules", "free_form"])
@pytest.mark.parametrize("variant", ["bits", "bits16", "bits_rec_lds", "front"])
@pytest.mark.parametrize("case", ec.CASES, ids=[ec.case_id(c) for c in ec.CASES])
def test_every_variant_and_both_routes(gpu_ctx, gpu_ctx_sdf_waves16, gpu_ctx_sdf_rec_lds, gpu_ctx_sdf_front, orc, case, variant, route):
    """rules: k_sdfbit_events<true> (X % 8 != 0) or k_sdfbit_events8<true> in the three bit-parallel builds, k_sdf_base_front<true> in
    the byte front.  free_form: the compiled classifier in front of each of them, which then read class bytes."""
    ctx = {"bits": gpu_ctx, "bits16": gpu_ctx_sdf_waves16, "bits_rec_lds": gpu_ctx_sdf_rec_lds, "front": gpu_ctx_sdf_front}[variant]
    kind, dims, seed, table = case
    want = ec.oracle_sdf(orc, *case)
    v = ctx.image_from(ec.volume(kind, dims, seed))
    try:
        _check(_build(ctx, v, ec.ROUTES[route][table], dims), want, "%s, %s, %s" % (ec.case_id(case), variant, route))
    finally:
        v.release()


@pytest.mark.parametrize("route", ["rules", "free_form"])
@pytest.mark.parametrize("case", ec.GENERIC_LAUNCH_CASES, ids=[ec.case_id(c) for c in ec.GENERIC_LAUNCH_CASES])
def test_layer_kernels_through_the_generic_launch(gpu_ctx, orc, case, route):
    """k_sdf_base<true> (rules) / k_sdf_base on class bytes (free form) and k_sdf_layer, launched one by one as the reference's host
    loop does, on a global size that exceeds the volume on every axis"""
    kind, dims, seed, table = case
    want, want_n = ec.oracle_sdf(orc, *case)
    launches, out = ec.reference_host_loop(gpu_ctx, ec.volume(kind, dims, seed), ec.ROUTES[route][table])
    _check((out, launches), (want, want_n), "%s, generic launch, %s" % (ec.case_id(case), route))


# ---- the class image of a free-form source is cached per context under (device pointer, content version, source text)

DIMS = (70, 33, 45)
BLOBS_A, BLOBS_B = ("blobs", DIMS, sum(DIMS)), ("blobs", DIMS, sum(DIMS) + 1)


def test_class_cache_after_a_push_into_the_same_image(gpu_ctx, orc):
    want_a, want_b = ec.oracle_sdf(orc, *BLOBS_A, "gradient"), ec.oracle_sdf(orc, *BLOBS_B, "gradient")
    assert int((want_a[0] != want_b[0]).sum()) > 1000
    source = ec.FREE_FORM["gradient"]
    v = gpu_ctx.image_from(ec.volume(*BLOBS_A))
    try:
        _check(_build(gpu_ctx, v, source, DIMS), want_a, "first contents")
        v.push(ec.volume(*BLOBS_B))   # the same device pointer, another content version
        _check(_build(gpu_ctx, v, source, DIMS), want_b, "after the push")
        _check(_build(gpu_ctx, v, source, DIMS), want_b, "once more, from the cached classes")
    finally:
        v.release()


def test_class_cache_under_two_sources_on_one_volume(gpu_ctx, orc):
    want = {t: ec.oracle_sdf(orc, *BLOBS_A, t) for t in ("gradient", "wrap")}   # the windows start at 500 and at 600
    assert int((want["gradient"][0] != want["wrap"][0]).sum()) > 1000
    v = gpu_ctx.image_from(ec.volume(*BLOBS_A))
    try:
        for t in ("gradient", "wrap", "gradient"):
            _check(_build(gpu_ctx, v, ec.FREE_FORM[t], DIMS), want[t], "source %s of A, B, A" % t)
    finally:
        v.release()


def test_class_cache_under_two_volumes_of_equal_dims(gpu_ctx, orc):
    want = [ec.oracle_sdf(orc, *b, "gradient") for b in (BLOBS_A, BLOBS_B)]
    source = ec.FREE_FORM["gradient"]
    images = [gpu_ctx.image_from(ec.volume(*b)) for b in (BLOBS_A, BLOBS_B)]
    try:
        for k in (0, 1, 0, 1):
            _check(_build(gpu_ctx, images[k], source, DIMS), want[k], "volume %d of 0, 1, 0, 1" % k)
    finally:
        for v in images:
            v.release()


def test_class_cache_after_a_release_and_an_image_of_other_dims(gpu_ctx, orc):
    """the allocator may hand the released address out again: the key's content version tells the two images apart"""
    source = ec.FREE_FORM["gradient"]
    other = ec.BLOB_CASES[1]   # (65, 49, 17): fewer voxels, other rows
    assert other[1] != DIMS and int(np.prod(other[1])) < int(np.prod(DIMS))
    v = gpu_ctx.image_from(ec.volume(*BLOBS_A))
    try:
        _check(_build(gpu_ctx, v, source, DIMS), ec.oracle_sdf(orc, *BLOBS_A, "gradient"), "first image")
    finally:
        v.release()
    v = gpu_ctx.image_from(ec.volume(*other[:3]))
    try:
        _check(_build(gpu_ctx, v, source, other[1]), ec.oracle_sdf(orc, *other), "second image")
    finally:
        v.release()


# ---- the same classes as k_repack reads them

def test_wrapping_classes_as_the_render_path_sees_them(gpu_ctx, orc):
    """`extremes` under the free-form wrap table through bind_scene's build (tests/test_gpu_packed_scene.py): step bytes, brick minima
    and the compared hit records against the numpy restatement under the numpy event set.  (Render contributions of a free-form table
    that reads `gradient` are not compared: that route is documented as not bit-exact at positions with irregular taps, tf_jit.cpp.)"""
    kind, dims, seed, table = ec.RENDER_CASE
    vol = ec.volume(kind, dims, seed)
    sdf, _ = ec.oracle_sdf(orc, *ec.RENDER_CASE)
    events = ec.events_of(vol, table)
    assert np.array_equal(events, sdf < 0)
    with pytest.raises(ffi.ClwhError):
        ffi.parse_tf(ec.FREE_FORM[table])
    b = Build(gpu_ctx, vol, sdf)
    try:
        b.render(ec.FREE_FORM[table])
        want = ps.PackedScene(vol, sdf, classes=events.astype(np.uint8))
        _compare(b.arrays(), want, "extremes, free-form wrap table")
    finally:
        b.release()
