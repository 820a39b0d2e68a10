"""clwh_volume_filter on the GPU against the contract's numpy restatement (tests/vfilter_ref.py) over the cases of
tests/vfilter_cases.py: equal bytes for every kind, no tolerance anywhere; out of place and in place, with a mask (random bits, garbage
padding) and without, through a second handle of the same pointer; device against device; and the rewrite rule."""
import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import projection_ref as pr
from tests import vfilter_cases as vc
from tests import vfilter_ref as vr
from tests.view_helpers import Proj, image_of

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A


class Volumes:
    """the field as an image, a second image for the out-of-place calls, and an alias of the first"""

    def __init__(self, ctx, vol):
        self.ctx, self.vol = ctx, vol
        Z, Y, X = vol.shape
        self.volume, self.owner = image_of(ctx, vol)
        self.out, self.out_owner = image_of(ctx, np.full_like(vol, PATTERN))
        self.alias = ctx.image_wrap(self.volume.device_ptr, (X, Y, Z), 1, np.int16)

    def read(self, which):
        m = {"in": self.owner or self.volume, "out": self.out_owner or self.out}[which]
        return m.pull(np.int16, self.vol.shape)

    def reset(self):
        (self.owner or self.volume).push(self.vol)
        (self.out_owner or self.out).push(np.full_like(self.vol, PATTERN))

    def release(self):
        for m in (self.alias, self.out, self.out_owner, self.volume, self.owner):
            if m is not None:
                m.release()


def run(v, kind, radius, weights, mask, mode):
    """the bytes one call leaves, by mode: "out" (volume_in is only read), "in place", "alias" (volume_out = another handle)"""
    v.reset()
    out = {"out": v.out, "in place": v.volume, "alias": v.alias}[mode]
    status = v.ctx.filter_volume_raw(v.volume, out, kind, radius, weights, mask)
    assert status == 0, (status, kind, radius, mode)
    if mode == "out":
        assert np.array_equal(v.read("in"), v.vol), "volume_in was written"
        return v.read("out")
    assert (v.read("out") == PATTERN).all()
    return v.read("in")


@pytest.mark.parametrize("field", vc.FIELDS)
@pytest.mark.parametrize("shape", sorted(vc.SHAPES))
def test_every_kind_equals_the_reference(gpu_ctx, shape, field):
    vol = vc.field(shape, field)
    bits, words = vc.mask_of(shape)
    v = Volumes(gpu_ctx, vol)
    mask = gpu_ctx.buffer_from(words)
    n = 0
    for label, kind, radius, weights in vc.PARAMS:
        f = vc.reference(shape, field, label)
        for with_mask in (False, True):
            want = np.where(bits, f, vol) if with_mask else f
            for mode in ("out", "in place", "alias"):
                got = run(v, kind, radius, weights, mask if with_mask else None, mode)
                bad = got != want
                assert not bad.any(), (shape, field, label, with_mask, mode, int(bad.sum()), tuple(np.argwhere(bad)[0]))
                n += 1
    assert n == 6 * len(vc.PARAMS) and np.array_equal(mask.pull(), words)  # the mask is only read
    mask.release()
    v.release()


def test_one_call_equals_three_single_axis_calls(gpu_ctx):
    """device against device: MAX over a box is three MAX calls along one axis each; SMOOTH is its three passes issued x, y, z as
    calls, and is NOT the passes issued z, y, x"""
    ctx = gpu_ctx
    vol = vc.field(*vc.MAIN)
    v = Volumes(ctx, vol)
    radius = (3, 9, 16)
    whole = run(v, ffi.FILTER_MAX, radius, None, None, "out")
    v.reset()
    for axis in range(3):
        r = [0, 0, 0]
        r[axis] = radius[axis]
        ctx.filter_volume(v.volume, ffi.FILTER_MAX, r)
    assert np.array_equal(v.read("in"), whole)

    w = scene.gaussian_weights((1.0, 1.0, 0.6))
    identity = np.array([4096], np.uint16)
    v.reset()
    ctx.filter_volume(v.volume, ffi.FILTER_SMOOTH, weights=w, out=v.out)
    whole = v.read("out")
    assert np.array_equal(whole, vc.reference(*vc.MAIN, "smooth gauss 1 1 0.6"))
    results = {}
    for order in ((0, 1, 2), (2, 1, 0)):
        v.reset()
        for axis in order:
            one = [identity] * 3
            one[axis] = w[axis]
            ctx.filter_volume(v.volume, ffi.FILTER_SMOOTH, weights=one)
        results[order] = v.read("in")
    assert np.array_equal(results[(0, 1, 2)], whole)
    assert np.array_equal(results[(2, 1, 0)], vr.smooth(vol, w, (2, 1, 0)))
    assert (results[(2, 1, 0)] != whole).mean() > 0.05
    v.release()


def test_filter_is_seen_by_the_views(gpu_ctx):
    """after filter_volume in place a projection shows the filtered array: without the version bump the bricked copy of the old
    content would answer.  The same for a call whose volume_out is a second handle of the pointer."""
    ctx = gpu_ctx
    X, Y, Z = 24, 16, 40
    a = scene.phantom(40, dims=(X, Y, Z))
    pos, d = scene.default_camera(40)
    volume = ctx.image_from(a)
    alias = ctx.image_wrap(volume.device_ptr, (X, Y, Z), 1, np.int16)
    p = Proj(ctx, (64, 48), (64, 48))
    want = lambda vol: pr.project(vol, pos, d, (64, 48), (64, 48))[pr.MAX]
    Proj.check(p.run(volume, pos, d, pr.MAX), want(a), "before")  # the derived copy of the unfiltered content exists now
    once = vr.extreme(a, (2, 2, 2), vr.MIN)
    assert not np.array_equal(want(once)[0], want(a)[0])
    ctx.filter_volume(volume, ffi.FILTER_MIN, (2, 2, 2))
    for dense in (False, True):
        Proj.check(p.run(volume, pos, d, pr.MAX, dense=dense), want(once), "after the filter, dense=%s" % dense)
    twice = vr.median(once, (1, 1, 1))
    assert not np.array_equal(want(twice)[0], want(once)[0])
    assert ctx.filter_volume_raw(volume, alias, ffi.FILTER_MEDIAN, (1, 1, 1)) == 0
    for through in (volume, alias):
        Proj.check(p.run(through, pos, d, pr.MAX), want(twice), "after the filter through the wrap")
    assert np.array_equal(volume.pull(), twice)
    ctx.finish()
    for m in (alias, volume):
        m.release()
    p.release()
