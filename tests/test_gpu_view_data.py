"""-m gpu: the data the views derive from the volume -- the bricked copy, the per-brick {min, max} table (k_proj_repack), the table of
the bricks dilated by one voxel and the table of the cells of 4^3 bricks (k_iso_dilate, k_iso_coarse) -- read back whole through
clwh_debug_view_data and compared, by np.array_equal, with their numpy restatement (tests/packed_scene_ref.py).  One 8 x 8 projection
builds the first two, one 8 x 8 isosurface the other two."""
import ctypes as C

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi
from tests import packed_scene_cases as pc
from tests import packed_scene_ref as ps
from tests.view_helpers import image_of, pose

pytestmark = pytest.mark.gpu

W = H = 8
BAD_ARGS = 7
ALL = (ffi.VIEW_BRICKS, ffi.VIEW_TABLE, ffi.VIEW_DILATED, ffi.VIEW_COARSE)
NAMES = {ffi.VIEW_BRICKS: "bricks", ffi.VIEW_TABLE: "table", ffi.VIEW_DILATED: "dilated", ffi.VIEW_COARSE: "coarse"}


def _status(ctx, which):
    info = (C.c_int32 * 4)()
    return ffi.lib().clwh_debug_view_data(ctx.h, which, None, C.c_uint64(0), info), tuple(info)


class Views:
    def __init__(self, ctx):
        self.ctx = ctx
        self.frame = ctx.image([W, H], 4, np.uint8, (H, W, 4))

    def projection(self, volume, dims):
        pos, d = pose("default", dims)
        self.ctx.render_projection(self.frame, volume, pos, d, W, H)
        self.ctx.finish()

    def isosurface(self, volume, dims):
        pos, d = pose("default", dims)
        self.ctx.render_isosurface(self.frame, volume, pos, d, W, H, 300.0)
        self.ctx.finish()

    def release(self):
        self.frame.release()


def _compare(ctx, vol, which=ALL, what=""):
    want = ps.ViewData(vol)
    for w in which:
        got, nb = ctx.view_data(w)
        ref = getattr(want, NAMES[w])
        assert nb == want.nb and got.shape == ref.shape, "%s %s" % (NAMES[w], what)
        bad = got != ref
        assert np.array_equal(got, ref), "%s %s: %d entries differ, first %s: got %s, want %s" % (
            NAMES[w], what, int(bad.sum()), tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])])


@pytest.mark.parametrize("kind", ["phantom", "random"])
@pytest.mark.parametrize("dims", pc.VIEW_SHAPES + [pc.LARGE_SHAPE], ids=lambda d: "%dx%dx%d" % d)
def test_all_four_arrays(gpu_ctx, dims, kind):
    ctx = gpu_ctx
    vol = pc.phantom(dims) if kind == "phantom" else pc.random_volume(dims)
    volume, owner = image_of(ctx, vol)
    v = Views(ctx)
    try:
        ctx.invalidate_derived(scene=False, camera=False, projection=True)
        assert _status(ctx, ffi.VIEW_BRICKS)[0] == BAD_ARGS   # no view data yet
        v.projection(volume, dims)
        # the bricked copy alone: the second-level tables are reported as missing and nothing is returned
        nbx, nby, nbz = ps.brick_counts(dims)
        cells = ((nbx + 3) // 4) * ((nby + 3) // 4) * ((nbz + 3) // 4)
        for w in (ffi.VIEW_DILATED, ffi.VIEW_COARSE):
            assert _status(ctx, w) == (BAD_ARGS, (nbx, nby, nbz, cells))
            canary = np.full(16, 0xA5, np.uint8)
            info = (C.c_int32 * 4)()
            assert ffi.lib().clwh_debug_view_data(ctx.h, w, canary.ctypes.data_as(C.c_void_p), C.c_uint64(1 << 40), info) == BAD_ARGS
            assert (canary == 0xA5).all()
        _compare(ctx, vol, (ffi.VIEW_BRICKS, ffi.VIEW_TABLE), "after a projection")
        v.isosurface(volume, dims)
        _compare(ctx, vol, ALL, "after an isosurface")
    finally:
        v.release()
        volume.release()
        if owner is not None:
            owner.release()


def test_tables_follow_the_volume(gpu_ctx):
    ctx = gpu_ctx
    dims = (40, 40, 136)
    a = pc.phantom(dims)
    b = pc.swapped(a)
    assert not np.array_equal(ps.ViewData(a).coarse, ps.ViewData(b).coarse)
    volume, _ = image_of(ctx, a)
    v = Views(ctx)
    other = None
    try:
        v.projection(volume, dims)
        v.isosurface(volume, dims)
        _compare(ctx, a, ALL, "first content")
        volume.push(b)   # the same image, air and ball swapped
        v.projection(volume, dims)
        for w in (ffi.VIEW_DILATED, ffi.VIEW_COARSE):
            assert _status(ctx, w)[0] == BAD_ARGS   # the bricked copy was rebuilt: the old second level is not offered
        _compare(ctx, b, (ffi.VIEW_BRICKS, ffi.VIEW_TABLE), "after a push")
        v.isosurface(volume, dims)
        _compare(ctx, b, ALL, "after a push and an isosurface")
        # a volume of other dims: shapes and contents follow
        dims2 = (70, 33, 45)
        c = pc.random_volume(dims2)
        other, _ = image_of(ctx, c)
        v.isosurface(other, dims2)
        _compare(ctx, c, ALL, "another volume")
        # the same memory wrapped with permuted dims is another volume
        wrapped = ctx.image_wrap(other.device_ptr, (45, 33, 70), 1, np.int16)
        try:
            v.isosurface(wrapped, (45, 33, 70))
            _compare(ctx, c.reshape(70, 33, 45), ALL, "the same memory, other dims")
        finally:
            wrapped.release()
    finally:
        v.release()
        volume.release()
        if other is not None:
            other.release()
