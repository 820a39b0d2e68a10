"""-m gpu: the arrays k_repack derives from (volume, SDF, transfer function) -- step bytes, hit records, per-brick free values -- read
back whole through clwh_debug_packed_scene and compared, by np.array_equal, with their numpy restatement (tests/packed_scene_ref.py).

Step bytes and brick minima are compared everywhere, padding slots included.  Hit records are compared in every slot of every 4^3
sub-brick that holds a voxel that may be an event under some gradient (`maybe`); k_repack leaves the other sub-bricks alone, so
nothing is required of them -- instead the read side is asserted: no voxel whose step byte has bit 7 set lies in one of them.  The
cameras look away from the volume: no pixel hits, nothing marches, the test is about the build alone."""
import ctypes as C

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import packed_scene_cases as pc
from tests import packed_scene_ref as ps

pytestmark = pytest.mark.gpu

W = H = 8


def _image(ctx, arr):
    """an image of arr [z][y][x] and the memory's owner, if it is another object (an image of width 1 cannot be created, only wrapped)"""
    Z, Y, X = arr.shape
    if X > 1:
        return ctx.image_from(arr), None
    owner = ctx.buffer_from(arr)
    return ctx.image_wrap(owner.device_ptr, (X, Y, Z), 1, arr.dtype, (Z, Y, X)), owner


class Build:
    """volume + SDF on a context and one all-miss launch per transfer function: what bind_scene builds, and no march"""

    def __init__(self, ctx, vol, sdf, share=None):
        self.ctx = ctx
        Z, Y, X = vol.shape
        if share is None:
            self.volume, self.vol_owner = _image(ctx, np.ascontiguousarray(vol, np.int16))
            self.sdf, self.sdf_owner = _image(ctx, np.ascontiguousarray(sdf, np.int8))
        else:   # a second context over the same device memory
            self.volume, self.vol_owner = ctx.image_wrap(share.volume.device_ptr, (X, Y, Z), 1, np.int16, (Z, Y, X)), None
            self.sdf, self.sdf_owner = ctx.image_wrap(share.sdf.device_ptr, (X, Y, Z), 1, np.int8, (Z, Y, X)), None
        self.env = ctx.image_from(scene.env_map(16, 8), channels=4)
        self.accum = ctx.buffer(ffi.accum_len(W, H, 1) * 16, np.float32)
        ctx.buffer_reset(self.accum)
        self.kernels = {}

    def render(self, tf_source):
        if tf_source not in self.kernels:
            self.kernels[tf_source] = self.ctx.kernel("ray_marching.cl", "render", tf_source)
        pos, d = pc.CAMERA_AWAY
        self.kernels[tf_source].render(frame=None, volume=self.volume, sdf=self.sdf, env=self.env, accum=self.accum, cam_pos=pos, cam_dir=d,
                                       seed=1, width=W, height=H, mode=ffi.ACCUM_IMAGE_SPACE, write_frame=False)
        self.ctx.finish()
        hits = C.c_uint32(1)
        ffi._check(ffi.lib().clwh_debug_hit_records(self.ctx.h, None, C.c_uint64(0), C.byref(hits)), "clwh_debug_hit_records")
        assert hits.value == 0   # every pixel misses: no march reads the (possibly synthetic) SDF

    def arrays(self):
        ctx = self.ctx
        stepb, nb = ctx.packed_scene(ffi.SCENE_STEP_BYTES)
        grec, nb_g = ctx.packed_scene(ffi.SCENE_HIT_RECORDS)
        brick_min, nb_m = ctx.packed_scene(ffi.SCENE_BRICK_MIN)
        assert nb == nb_g == nb_m
        return stepb, grec, brick_min, nb

    def release(self):
        for k in self.kernels.values():
            k.release()
        for m in (self.volume, self.sdf, self.vol_owner, self.sdf_owner, self.env, self.accum):
            if m is not None:
                m.release()


def _compare(got, want, what):
    """every array against its restatement; all that differ are named, not only the first"""
    stepb, grec, brick_min, nb = got
    assert nb == want.nb, what
    wrong = []
    if not np.array_equal(stepb, want.stepb):
        at = tuple(np.argwhere(stepb != want.stepb)[0])
        wrong.append("step bytes differ in %d slots, first (brick, slot) %s: got %#x, want %#x" % (int((stepb != want.stepb).sum()), at, stepb[at], want.stepb[at]))
    if not np.array_equal(brick_min, want.brick_min):
        at = int(np.argwhere(brick_min != want.brick_min)[0][0])
        wrong.append("brick minima differ in %d bricks, first %d: got %d, want %d" % (int((brick_min != want.brick_min).sum()), at, brick_min[at], want.brick_min[at]))
    compared = want.compared_slots()
    if not np.array_equal(grec[compared], want.grec[compared]):
        bad = (grec != want.grec).any(axis=2) & compared
        at = tuple(np.argwhere(bad)[0])
        wrong.append("hit records differ in %d of %d compared slots, first (brick, slot) %s: got %s, want %s" % (
            int(bad.sum()), int(compared.sum()), at, [hex(w) for w in grec[at]], [hex(w) for w in want.grec[at]]))
    # the sub-bricks nothing is required of are never read: a record is fetched at a voxel whose step byte has bit 7 set
    if ((stepb & 0x80) != 0)[~compared].any():
        wrong.append("a voxel with bit 7 set lies in a sub-brick whose records are not specified")
    assert not wrong, "%s: %s" % (what, "; ".join(wrong))


def _oracle_sdf(orc, vol, tf_source):
    return orc.sdf_build(vol, orc.parse_tf(tf_source))[0]


@pytest.mark.parametrize("tf", sorted(pc.RULE_TFS))
@pytest.mark.parametrize("dims", pc.REPACK_SHAPES, ids=lambda d: "%dx%dx%d" % d)
def test_phantom_with_the_oracles_sdf(gpu_ctx, orc, dims, tf):
    source = pc.RULE_TFS[tf]
    vol = pc.phantom(dims)
    sdf = _oracle_sdf(orc, vol, source)
    b = Build(gpu_ctx, vol, sdf)
    try:
        b.render(source)
        _compare(b.arrays(), ps.PackedScene(vol, sdf, orc.parse_tf(source).as_tuples()), "%s %s" % (dims, tf))
    finally:
        b.release()


@pytest.mark.parametrize("dims", pc.GRADIENT_SHAPES, ids=lambda d: "%dx%dx%d" % d)
def test_gradient_table_writes_some_sub_bricks_and_leaves_others(gpu_ctx, orc, dims):
    source = scene.tf_gradient_source()
    vol = pc.phantom(dims)
    sdf = _oracle_sdf(orc, vol, source)
    want = ps.PackedScene(vol, sdf, orc.parse_tf(source).as_tuples())
    assert (want.maybe & (want.cls == 0)).sum() >= 100 and 10 * want.written.sum() >= want.written.size   # (tests/test_packed_scene_cpu.py)
    b = Build(gpu_ctx, vol, sdf)
    try:
        b.render(source)
        _compare(b.arrays(), want, "%s gradient" % (dims,))
    finally:
        b.release()


@pytest.mark.parametrize("tf", ["gradient", "three_rects"])
@pytest.mark.parametrize("dims", pc.RANDOM_SHAPES, ids=lambda d: "%dx%dx%d" % d)
def test_random_volume_and_random_sdf(gpu_ctx, orc, dims, tf):
    """central differences of +-65535 in the 17-bit fields, gradients that wrap as shorts, every SDF value"""
    source = pc.RULE_TFS[tf]
    vol, sdf = pc.random_volume(dims), pc.random_sdf(dims)
    b = Build(gpu_ctx, vol, sdf)
    try:
        b.render(source)
        _compare(b.arrays(), ps.PackedScene(vol, sdf, orc.parse_tf(source).as_tuples()), "%s random, %s" % (dims, tf))
    finally:
        b.release()


@pytest.mark.parametrize("dims", pc.REPACK_SHAPES, ids=lambda d: "%dx%dx%d" % d)
def test_every_record_of_a_random_volume(gpu_ctx, orc, dims):
    """a table under which every voxel is an event: every sub-brick is written, so every record of the volume is compared -- the
    phantom's events are a shell and a ball, which leave most block seams uncompared"""
    vol, sdf = pc.random_volume(dims), pc.random_sdf(dims)
    want = ps.PackedScene(vol, sdf, orc.parse_tf(pc.TF_ALL_CLASS_2).as_tuples())
    assert np.array_equal(want.written, ps.real_slots(dims).reshape(-1, 8, ps.SUB_SLOTS).any(axis=2)) and not want.brick_min.any()
    b = Build(gpu_ctx, vol, sdf)
    try:
        b.render(pc.TF_ALL_CLASS_2)
        _compare(b.arrays(), want, "%s every record" % (dims,))
    finally:
        b.release()


@pytest.mark.parametrize("dims", [(128, 16, 16), (80, 9, 9), (72, 40, 56)], ids=lambda d: "%dx%dx%d" % d)
def test_random_sdf_under_the_default_table(gpu_ctx, orc, dims):
    """negative values, 0, 1 and 127 in the step bytes and the minima (the start and hull tables are built from these step bytes too)"""
    source = scene.tf_default_source()
    vol, sdf = pc.phantom(dims), pc.random_sdf(dims)
    b = Build(gpu_ctx, vol, sdf)
    try:
        b.render(source)
        want = ps.PackedScene(vol, sdf, orc.parse_tf(source).as_tuples())
        assert {0, 1, 127} <= set(np.unique(want.stepb & 0x7F).tolist())
        _compare(b.arrays(), want, "%s random SDF" % (dims,))
    finally:
        b.release()


def test_free_form_table(gpu_ctx, orc):
    """the hiprtc route: the classes come from the compiled classifier and `maybe` is exactly class != 0"""
    with pytest.raises(ffi.ClwhError):
        ffi.parse_tf(pc.TF_FREE_FORM)
    dims = (72, 40, 56)
    vol = pc.free_form_volume(dims)
    sdf = pc.random_sdf(dims)
    b = Build(gpu_ctx, vol, sdf)
    try:
        b.render(pc.TF_FREE_FORM)
        want = ps.PackedScene(vol, sdf, classes=pc.free_form_classes(vol))
        assert (want.cls[vol == 31000] == 1).all() and not want.written.all()
        _compare(b.arrays(), want, "free form")
    finally:
        b.release()


def test_large_volume(gpu_ctx, orc):
    """many blocks in flight; a synthetic SDF (the oracle's build of this size takes seconds and the build does not care)"""
    source = scene.tf_gradient_source()
    vol, sdf = pc.phantom(pc.LARGE_SHAPE), pc.random_sdf(pc.LARGE_SHAPE)
    b = Build(gpu_ctx, vol, sdf)
    try:
        b.render(source)
        _compare(b.arrays(), ps.PackedScene(vol, sdf, orc.parse_tf(source).as_tuples()), "large")
    finally:
        b.release()


def test_rebuilds_in_place_and_a_second_context(orc):
    """one context, shape and volume fixed: a table under which every voxel is an event of class 2, then the gradient table (rebuilt in
    place: ensure_packed), then another SDF in the same image; then a second context adopts the entry"""
    dims = (64, 64, 64)
    vol = pc.mixed_volume(dims)   # with sub-bricks that are written although they hold no event
    gradient = scene.tf_gradient_source()
    sdf = _oracle_sdf(orc, vol, gradient)
    ctx0, ctx1 = ffi.Context(0), ffi.Context(0)
    b = Build(ctx0, vol, sdf)
    other = None
    try:
        b.render(pc.TF_ALL_CLASS_2)
        first = ps.PackedScene(vol, sdf, orc.parse_tf(pc.TF_ALL_CLASS_2).as_tuples())
        assert first.written.all() and not first.brick_min.any()
        got = b.arrays()
        _compare(got, first, "every voxel class 2")
        assert (ps.unpack_class(got[1])[ps.real_slots(dims)] == 2).all()
        bytes0 = ctx0.scene_info()[1]

        b.render(gradient)
        assert ctx0.scene_info()[1] == bytes0 and ctx0.scene_info()[2] == 1   # the same allocation, rebuilt
        want = ps.PackedScene(vol, sdf, orc.parse_tf(gradient).as_tuples())
        assert want.brick_min.any()   # minima the first build's zeros would hide under atomicMin
        stepb, grec, brick_min, nb = got = b.arrays()
        _compare(got, want, "gradient table after the class-2 table")
        event = (stepb & 0x80) != 0
        assert np.array_equal(ps.unpack_class(grec)[event], ps.scatter(want.cls, 0)[event]) and (ps.unpack_class(grec)[event] == 1).all()
        # ... and the stale records the invariant protects against are really there
        compared = want.compared_slots()
        assert (ps.unpack_class(grec)[~compared & ps.real_slots(dims)] == 2).any()

        sdf2 = pc.random_sdf(dims, seed=99)
        b.sdf.push(sdf2)
        other = Build(ctx1, vol, sdf2, share=b)   # (before the build: a wrap gives the memory a new content version)
        b.render(gradient)
        want2 = ps.PackedScene(vol, sdf2, orc.parse_tf(gradient).as_tuples())
        assert not np.array_equal(want2.stepb, want.stepb) and not np.array_equal(want2.brick_min, want.brick_min)
        got2 = b.arrays()
        _compare(got2, want2, "after another SDF was pushed")

        other.render(gradient)
        id0, _, holders0 = ctx0.scene_info()
        id1, _, holders1 = ctx1.scene_info()
        assert id1 == id0 and holders0 == holders1 == 2   # adopted, not rebuilt
        theirs = other.arrays()
        assert theirs[3] == got2[3] and all(np.array_equal(a, c) for a, c in zip(theirs[:3], got2[:3]))   # the same bytes, stale ones included
    finally:
        if other is not None:
            other.release()
        b.release()
        ctx1.destroy()
        ctx0.destroy()
