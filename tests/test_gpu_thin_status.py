"""clwh_mask_thin's and clwh_mask_points' exact status for every invalid call, in the order of kinds the header gives, and that nothing
is written on any of them; then that the same arguments without the defect are accepted."""
import ctypes as C

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import thin_ref as tr

pytestmark = pytest.mark.gpu

INVALID_VALUE, SIZE_MISMATCH = 1, 9
PATTERN = 0xA5A5A5A5


def test_status_codes_and_nothing_written(gpu_ctx):
    ctx = gpu_ctx
    dims = X, Y, Z = (70, 12, 9)
    n, words = X * Y * Z, scene.mask_words_per_row(X) * Y * Z
    fill = lambda k: ctx.buffer_from(np.full(k, PATTERN, np.uint32))
    mask, out, anchors, short_mask = fill(words), fill(words), fill(words), fill(words - 1)
    capacity = n  # room for every voxel
    points, values, field = fill(4 * capacity), fill(capacity), fill(n)
    short_points, short_values, short_field = fill(4 * capacity - 1), fill(capacity - 1), fill(n - 1)
    as_image = ctx.image([4, 4, n // 16 + 1], 1, np.uint32)
    odd_mask = ctx.wrap(mask.device_ptr + 4, 4 * words - 4)
    odd_words = ctx.wrap(field.device_ptr + 2, 4 * n - 4)
    bad_dims = ((0, 12, 9), (70, 0, 9), (70, 12, 0), (1 << 31, 1, 1), (1 << 16, 1 << 15, 1))

    def thin(**kw):
        args = dict(mask_in=mask, mask_out=out, dims=dims, flags=0, anchors=anchors, max_iterations=0)
        args.update(kw)
        return ctx.thin_mask_raw(**args)[0]

    def pts(**kw):
        args = dict(mask=mask, dims=dims, points=points, capacity=capacity, map=field, values=values, flags=0)
        args.update(kw)
        return ctx.mask_points_raw(**args)[0]

    L = ffi.lib()
    for name, desc in (("clwh_mask_thin", ffi.ThinDesc()), ("clwh_mask_points", ffi.MaskPointsDesc())):
        assert getattr(L, name)(None, C.byref(desc)) == INVALID_VALUE and getattr(L, name)(ctx.h, None) == INVALID_VALUE
    # NULL result / NULL n_points in an otherwise valid descriptor
    d = ffi.ThinDesc()
    d.mask_in, d.mask_out = mask.h, out.h
    e = ffi.MaskPointsDesc()
    e.mask = mask.h
    for k in range(3):
        d.dims[k] = e.dims[k] = dims[k]
    assert L.clwh_mask_thin(ctx.h, C.byref(d)) == INVALID_VALUE and L.clwh_mask_points(ctx.h, C.byref(e)) == INVALID_VALUE

    cases = []
    for bad in (None, as_image, odd_mask):
        cases += [thin(mask_in=bad), thin(mask_out=bad), pts(mask=bad)]
    cases += [thin(anchors=as_image), thin(anchors=odd_mask)]
    cases += [thin(flags=4), thin(flags=-1), thin(flags=1 << 16), pts(flags=1), pts(flags=-1)]
    for bad in (as_image, odd_words):
        cases += [pts(points=bad), pts(map=bad), pts(values=bad)]
    cases += [pts(map=None), pts(values=None), pts(points=None), pts(points=None, map=None, values=None)]  # (the last: a capacity without points)
    for bad in bad_dims:
        cases += [thin(dims=bad), pts(dims=bad)]
    assert cases == [INVALID_VALUE] * len(cases), cases
    sizes = [thin(mask_in=short_mask), thin(mask_out=short_mask), thin(anchors=short_mask), pts(mask=short_mask), pts(map=short_field),
             pts(points=short_points), pts(values=short_values), pts(capacity=1 << 62)]
    assert sizes == [SIZE_MISMATCH] * len(sizes), sizes
    # INVALID_VALUE before SIZE_MISMATCH, whichever argument carries it
    assert thin(mask_out=short_mask, flags=4) == INVALID_VALUE and thin(anchors=short_mask, dims=bad_dims[0]) == INVALID_VALUE
    assert pts(points=short_points, flags=1) == INVALID_VALUE and pts(mask=short_mask, values=None) == INVALID_VALUE
    # a buffer too small for the count: the count, and nothing written
    true_count = int(scene.mask_unpack(np.full(words, PATTERN, np.uint32), dims).sum())
    assert ctx.mask_points_raw(mask, dims, points, true_count - 1, field, values) == (SIZE_MISMATCH, true_count)
    for m in (mask, out, anchors, short_mask, points, values, field, short_points, short_values, short_field):
        assert (m.pull(np.uint32, (m.nbytes // 4,)) == PATTERN).all()  # nothing was written

    # and the same arguments without the defect are accepted
    assert ctx.mask_points_raw(mask, dims) == (0, true_count) and ctx.mask_points_raw(mask, dims, points, true_count, field, values) == (0, true_count)
    assert pts(map=None, values=None) == 0
    assert thin() == 0 and (out.pull() == scene.mask_pack(scene.mask_unpack(np.full(words, PATTERN, np.uint32), dims))).all(), "every voxel anchored"
    status, res = ctx.thin_mask_raw(mask, out, dims, ffi.THIN_KEEP_ENDS | ffi.THIN_DENSE, None, 3)
    pattern = scene.mask_unpack(np.full(words, PATTERN, np.uint32), dims)
    want, want_res, kept = tr.thin(pattern, tr.KEEP_ENDS, None, 0, (3,))
    assert status == 0 and res.as_dict() == kept[3][1] and np.array_equal(out.pull(), scene.mask_pack(kept[3][0]))
    assert thin(mask_out=mask, anchors=None) == 0  # in place
    assert (anchors.pull() == PATTERN).all()
    for x in (odd_words, odd_mask, as_image, short_field, short_values, short_points, field, values, points, short_mask, anchors, out, mask):
        x.release()
