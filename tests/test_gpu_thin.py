"""clwh_mask_thin and clwh_mask_points on the GPU against the contract's numpy restatement (tests/thin_ref.py) over the cases of
tests/thin_cases.py: equal bytes of the mask and equal iterations, deleted, count_in and count_out, no tolerance anywhere; every call
made twice with pre-filled outputs; worklist and dense, in place and out of place, with clean and with garbage padding."""
import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import thin_cases as tc
from tests import thin_ref as tr
from tests.thin_cases import garbage

pytestmark = pytest.mark.gpu

SIZE_MISMATCH = 9
PATTERN = 0xA5A5A5A5


def thin_on_device(ctx, words, dims, flags, anchor_words, max_iterations, in_place):
    """(the mask's words as the device wrote them, the result's dict)"""
    out = res = None
    anchors = ctx.buffer_from(anchor_words) if anchor_words is not None else None
    for turn in ("first", "again"):
        mask_in = ctx.buffer_from(words)
        mask_out = mask_in if in_place else ctx.buffer_from(np.full(len(words), PATTERN, np.uint32))
        status, result = ctx.thin_mask_raw(mask_in, mask_out, dims, flags, anchors, max_iterations)
        assert status == 0, (status, dims, flags, max_iterations, in_place, turn)
        got = mask_out.pull()
        assert in_place or np.array_equal(mask_in.pull(), words)  # read only
        assert out is None or (np.array_equal(out, got) and res == result.as_dict()), (dims, flags, turn)
        out, res = got, result.as_dict()
        mask_in.release()
        if not in_place:
            mask_out.release()
    if anchors is not None:
        assert np.array_equal(anchors.pull(), anchor_words)  # read only
        anchors.release()
    return out, res


@pytest.mark.parametrize("name", sorted(tc.cases()))
def test_every_case_equals_the_reference(gpu_ctx, name):
    mask, anchors = tc.cases()[name]
    dims = tc.dims_of(mask)
    variant = 0
    for keep_ends in (False, True):
        for anchored in (False, True):
            ref = tc.reference(name, keep_ends, anchored)
            for k in tc.MAX_ITERATIONS:
                want_mask, want = scene.mask_pack(ref[k][0]), ref[k][1]
                for dense in (False, True):
                    for in_place in (False, True):
                        variant += 1
                        dirty = variant % 3 != 0  # two of three with every padding bit set on entry, of the mask and of the anchors
                        words = garbage(mask) if dirty else scene.mask_pack(mask)
                        anchor_words = (garbage(anchors) if dirty else scene.mask_pack(anchors)) if anchored else None
                        flags = (ffi.THIN_KEEP_ENDS if keep_ends else 0) | (ffi.THIN_DENSE if dense else 0)
                        got, res = thin_on_device(gpu_ctx, words, dims, flags, anchor_words, k, in_place)
                        what = (name, keep_ends, anchored, k, dense, in_place, dirty)
                        assert res == want, (what, res, want)
                        assert np.array_equal(got, want_mask), (what, int((scene.mask_unpack(got, dims) != ref[k][0]).sum()))


POINT_CASES = ("noise 129 x 33 x 18 at 0.5", "noise 65 x 33 x 18 at 0.2", "solid 65 x 1 x 1", "solid 1 x 1 x 1", "torus", "bars")


@pytest.mark.parametrize("name", POINT_CASES)
def test_points_equal_the_reference(gpu_ctx, name):
    ctx = gpu_ctx
    full, _ = tc.cases()[name]
    dims = X, Y, Z = tc.dims_of(full)
    sampled = np.random.default_rng(3).integers(0, 1 << 32, (Z, Y, X), dtype=np.uint64).astype(np.uint32)
    field = ctx.buffer_from(sampled)
    for mask in (full, tc.reference(name, True, False)[0][0], np.zeros_like(full)):
        want, want_values = tr.points(mask, sampled)
        n = len(want)
        for words in (scene.mask_pack(mask), garbage(mask)):
            d_mask = ctx.buffer_from(words)
            assert ctx.mask_points_raw(d_mask, dims) == (0, n)  # the counting call
            points = ctx.buffer_from(np.full(4 * (n + 2), PATTERN, np.uint32))
            values = ctx.buffer_from(np.full(n + 2, PATTERN, np.uint32))
            for with_map in (False, True):
                for turn in ("first", "again"):
                    status, count = ctx.mask_points_raw(d_mask, dims, points, n + 2, field if with_map else None, values if with_map else None)
                    assert (status, count) == (0, n), (name, with_map, turn)
                    got = points.pull().reshape(-1, 4)
                    assert np.array_equal(got[:n], want) and (got[n:] == PATTERN).all(), (name, with_map, turn)
                    got_values = values.pull()
                    assert np.array_equal(got_values[:n], want_values) if with_map else (got_values == PATTERN).all()
                    assert (got_values[n:] == PATTERN).all()
            if n > 0:  # too small: the true count, nothing written
                points.push(np.full(4 * (n + 2), PATTERN, np.uint32))
                assert ctx.mask_points_raw(d_mask, dims, points, n - 1) == (SIZE_MISMATCH, n)
                assert (points.pull() == PATTERN).all()
            assert np.array_equal(d_mask.pull(), words)  # read only
            for m in (values, points, d_mask):
                m.release()
    d_mask = ctx.buffer_from(scene.mask_pack(full))
    got_points, got_values = ctx.mask_points(d_mask, dims, field)
    d_mask.release()
    want, want_values = tr.points(full, sampled)
    assert np.array_equal(got_points, want) and np.array_equal(got_values, want_values)
    field.release()


@pytest.mark.parametrize("name", ("noise 70 x 40 x 36 at 0.2", "bars", "hollow box"))
def test_device_against_device(gpu_ctx, name):
    """count_out is clwh_mask_statistics' count of the output, and clwh_segment_label under 26-connectivity finds as many parts in the
    output as in the input"""
    ctx = gpu_ctx
    mask, _ = tc.cases()[name]
    dims = X, Y, Z = tc.dims_of(mask)
    volume = ctx.image_from(np.zeros((Z, Y, X), np.int16))
    d_mask = ctx.buffer_from(scene.mask_pack(mask))
    thin, res = ctx.thin_mask(d_mask, dims, keep_ends=True)
    assert res.as_dict() == tc.reference(name, True, False)[0][1]
    assert int(ctx.mask_statistics(volume, thin)[0].count) == int(res.count_out)
    parts = []
    for m in (d_mask, thin):
        labels, found, _ = ctx.label_components(volume, 0, 0, 26, mask=m, capacity=0)
        parts.append(int(found.n_components))
        labels.release()
    assert parts[0] == parts[1] == tr.invariants(mask)[0]
    for m in (thin, d_mask, volume):
        m.release()


def test_skeleton_of_the_bars(gpu_ctx):
    """Context.skeleton composes the depth map, the thinning, the points and the graph"""
    mask, _ = tc.cases()["bars"]
    dims = tc.dims_of(mask)
    d_mask = gpu_ctx.buffer_from(scene.mask_pack(mask))
    graph = gpu_ctx.skeleton(d_mask, dims, (1.0, 1.0, 1.0))
    want = tc.reference("bars", True, False)[0]
    assert graph["result"].as_dict() == want[1] and np.array_equal(graph["points"], tr.points(want[0])[0])
    assert [n["kind"] for n in graph["nodes"]].count("end") == 6
    assert all(0.0 < b["min_radius"] <= b["mean_radius"] <= 4.0 for b in graph["branches"])  # inside bars 4 voxels across
    d_mask.release()
