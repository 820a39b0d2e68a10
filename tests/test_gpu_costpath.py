"""clwh_cost_geodesic, clwh_cost_trace and clwh_cost_from_field on the GPU against the contract's Python restatement
(tests/costpath_ref.py): equal bytes of both maps, no tolerance anywhere.  Every case runs twice on one context by the worklist and
twice with CLWH_GEO_DENSE; the maps are allocated four words too long and pre-filled with a pattern that must survive behind
X * Y * Z; cost, domain and a separate seed_labels are read only.  On every map that has both outputs the device's trace from the
farthest voxel is compared with the reference's walk.  The tile core is 16 x 16 x 8."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import costpath_ref as cp
from tests import geodesic_ref as g
from tests.view_helpers import ROOT, host_lib

pytestmark = pytest.mark.gpu

INVALID_VALUE, SIZE_MISMATCH = 1, 9
NONE = cp.NONE
PATTERN = 0xA5A5A5A5
BOTH = (6, 26)


def dims_of(a):
    Z, Y, X = a.shape
    return X, Y, Z


def same(got, want, what):
    assert got.dtype == want.dtype and np.array_equal(got, want), (what, int((got != want).sum()), np.argwhere(got != want)[:3].tolist())


def flag_of(connectivity):
    return ffi.GEO_26 if connectivity == 26 else 0


class Device:
    def __init__(self, ctx):
        self.ctx = ctx

    def geodesic(self, cost, seeds=None, connectivity=6, multipliers=None, cap=None, seed_labels=None, domain=None, outputs="both",
                 in_place=False):
        """(dist, labels, result dict) as the device wrote them, uint32 [z][y][x]; an output that was not asked for is None"""
        cost = np.ascontiguousarray(cost, np.uint16)
        dims = X, Y, Z = dims_of(cost)
        n = X * Y * Z
        d_cost = self.ctx.buffer_from(cost)
        words = scene.mask_pack(domain) if domain is not None else None
        d_domain = self.ctx.buffer_from(words) if domain is not None else None
        dist = self.ctx.buffer(4 * (n + 4), np.uint32, (n + 4,)) if outputs in ("both", "dist") else None
        labels = self.ctx.buffer(4 * (n + 4), np.uint32, (n + 4,)) if outputs in ("both", "labels") else None
        given = None
        if seed_labels is not None:
            given = labels if in_place else self.ctx.buffer_from(np.ascontiguousarray(seed_labels, np.uint32))
        base = flag_of(connectivity) | (ffi.GEO_FROM_LABELS if seed_labels is not None else 0)
        first = None
        for turn, dense in (("first", 0), ("again", 0), ("dense", ffi.GEO_DENSE), ("dense again", ffi.GEO_DENSE)):
            for m in (dist, labels):
                if m is not None:
                    m.push(np.full(n + 4, PATTERN, np.uint32))
            if in_place:
                labels.push(np.concatenate([np.asarray(seed_labels, np.uint32).reshape(-1), np.full(4, PATTERN, np.uint32)]))
            status, res = self.ctx.cost_geodesic_raw(d_cost, dims, seeds, d_domain, given, base | dense, multipliers,
                                                     NONE if cap is None else cap, dist, labels)
            assert status == 0, (status, dims, turn)
            got = []
            for m in (dist, labels):
                a = m.pull() if m is not None else None
                assert a is None or (a[n:] == PATTERN).all(), (dims, turn, "written behind X * Y * Z")
                got.append(a[:n].reshape(Z, Y, X).copy() if a is not None else None)
            got.append(res.as_dict())
            if first is None:
                first = got
            for a, b in zip(first[:2], got[:2]):
                assert (a is None and b is None) or np.array_equal(a, b), (dims, turn, "differs from the first call")
            assert first[2] == got[2], (dims, turn)
        if dist is not None and labels is not None:
            self.trace_farthest(d_cost, cost, dist, labels, first, dims, connectivity, multipliers)
        assert np.array_equal(d_cost.pull().reshape(cost.shape), cost), "the cost is read only"
        assert d_domain is None or np.array_equal(d_domain.pull(), words), "the domain is read only"
        if given is not None and not in_place:
            assert np.array_equal(given.pull().reshape(-1), np.asarray(seed_labels, np.uint32).reshape(-1)), "seed_labels is read only"
            given.release()
        for m in (d_cost, d_domain, dist, labels):
            if m is not None:
                m.release()
        return first

    def trace_farthest(self, d_cost, cost, d_dist, d_labels, maps, dims, connectivity, multipliers):
        """clwh_cost_trace over the device's own maps from the farthest reached voxel, with and without the labels"""
        dist, labels = maps[0], maps[1]
        if not (dist != NONE).any():
            return
        z, y, x = np.argwhere(dist == dist[dist != NONE].max())[0]
        for with_labels in (None, labels):
            want, complete = cp.trace(cost, dist, (x, y, z), connectivity, multipliers, with_labels)
            assert complete, (dims, connectivity, "the reference's walk over the device's map")
            got, count = self.ctx.cost_trace(d_cost, d_dist, dims, (x, y, z), d_labels if with_labels is not None else None, connectivity,
                                             multipliers, len(want) + 1)
            assert count == len(want) and got.tolist() == [list(p) for p in want], (dims, connectivity, (x, y, z))

    def check(self, cost, seeds, connectivity=6, multipliers=None, cap=None, seed_labels=None, domain=None, want=None, **kw):
        want = want if want is not None else cp.cost_geodesic(cost, seeds, connectivity, multipliers, cap, seed_labels, domain)
        what = (dims_of(cost), connectivity, multipliers, cap, kw)
        dist, labels, res = self.geodesic(cost, seeds, connectivity, multipliers, cap, seed_labels, domain, **kw)
        if dist is not None:
            same(dist, want[0], what + ("dist",))
        if labels is not None:
            same(labels, want[1], what + ("labels",))
        assert res == g.result(want[0]), what
        return want


# ---- 1. random costs over 1 .. 65535 with a tenth of the voxels 0; domain NULL, given, and given around cost-0 holes
@pytest.mark.parametrize("connectivity", BOTH)
@pytest.mark.parametrize("dims", cp.SHAPES)
def test_random_costs_equal_the_reference(gpu_ctx, dims, connectivity):
    dev = Device(gpu_ctx)
    assert scene.geodesic_weights((1, 1, 1), 10) == cp.CHAMFER
    for with_domain in (False, True):
        cost, domain, seeds, dist, labels = cp.random_case(dims, connectivity, cp.CHAMFER, None, with_domain)
        assert dims == (1, 1, 1) or ((cost == 0).sum() > 0 and (domain is None or (domain & (cost == 0)).sum() > 0))
        dev.check(cost, seeds, connectivity, cp.CHAMFER, domain=domain, want=(dist, labels))
        reached = dist[dist != NONE]
        if len(reached) > 10:  # a cap that cuts the map
            cap = int(np.median(reached))
            cut = dev.check(cost, seeds, connectivity, cp.CHAMFER, cap, domain=domain)
            assert 0 < g.result(cut[0])["reached"] < len(reached) and g.result(cut[0])["max_dist"] <= cap
    # a domain over a cost without walls, anisotropic multipliers
    X, Y, Z = dims
    cost = cp.random_cost(dims, 4, 0.0)
    domain = np.random.default_rng(6).random((Z, Y, X)) < 0.7
    dev.check(cost, cp.random_seeds(domain, 8), connectivity, cp.ANISO, domain=domain)


# ---- 2. the highway: tiles at rest are woken again, rounds after the expensive direct route reached them
@pytest.mark.parametrize("connectivity", BOTH)
def test_highway_lowers_tiles_at_rest(gpu_ctx, connectivity):
    cost, dist, labels = cp.highway_case(connectivity)
    Device(gpu_ctx).check(cost, [cp.HIGHWAY_SEED], connectivity, cp.CHAMFER, want=(dist, labels))
    # not vacuous: final predecessor chains longer in steps than the unit-cost shortest path
    unit = g.geodesic(np.ones(cost.shape, bool), [cp.HIGHWAY_SEED], connectivity)[0]
    longer = 0
    for target in ((2, 34, 3), (40, 34, 3), (2, 18, 3), (30, 30, 6)):
        points, complete = cp.trace(cost, dist, target, connectivity, cp.CHAMFER)
        assert complete
        longer += len(points) - 1 > int(unit[target[2], target[1], target[0]])
    assert longer >= 1
    # and the far tiles' answers come from the corridor, not from the field's direct route
    assert int(dist[3, 34, 2]) < 32 * 10 * 1000


# ---- 3. grow's serpentine as the domain, random costs
@pytest.mark.parametrize("connectivity", BOTH)
def test_serpentine_domain(gpu_ctx, connectivity):
    cost, domain, dist, labels = cp.serpentine_case(connectivity)
    assert (dist != NONE).sum() == domain.sum() == 2739 and int(dist.max(where=dist != NONE, initial=0)) > 2 ** 29
    Device(gpu_ctx).check(cost, [(0, 0, 1, 7)], connectivity, cp.CHAMFER, domain=domain, want=(dist, labels))


# ---- 4. the extremes: multiplier 255 and cost 65535 under CLWH_COST_CAP_MAX
def test_largest_steps_and_the_cap(gpu_ctx):
    dev = Device(gpu_ctx)
    step = 255 * 65535
    line = np.full((1, 1, 300), 65535, np.uint16)
    want = dev.check(line, [(0, 0, 0, 0xFFFFFFFF)], 6, cp.LARGEST, ffi.COST_CAP_MAX)
    last = ffi.COST_CAP_MAX // step
    assert last == 256 and int(want[0][0, 0, last]) == last * step and int(want[0][0, 0, last + 1]) == NONE
    assert int(want[1][0, 0, last]) == 0xFFFFFFFF and int(want[1][0, 0, last + 1]) == 0
    same(dev.check(line, [(0, 0, 0, 0xFFFFFFFF)], 6, cp.LARGEST)[0], want[0], "CLWH_DIST_NONE means the largest cap")
    slab = np.full((9, 17, 17), 65535, np.uint16)
    for cap in (0, step - 1, step, 3 * step, ffi.COST_CAP_MAX):
        capped = dev.check(slab, [(8, 8, 4, 5)], 26, cp.LARGEST, cap)
        assert g.result(capped[0])["reached"] == (1 if cap < step else slab.size if cap >= 8 * step else 27 if cap == step else 343)


# ---- 5. symmetric ties across a tile face: the smaller id wins
def test_symmetric_ties(gpu_ctx):
    dev = Device(gpu_ctx)
    z, y, x = np.indices((12, 20, 40))
    cost = (1 + (y % 3) + 2 * (z % 2)).astype(np.uint16)  # the same on both sides of any plane across x
    for plane in (15, 16):
        for connectivity in BOTH:
            seeds = [(plane + 2, 4, 4, 9), (plane - 2, 4, 4, 4)]
            want = dev.check(cost, seeds, connectivity, cp.CHAMFER)
            each = [cp.cost_geodesic(cost, [s], connectivity, cp.CHAMFER)[0] for s in seeds]
            tie = each[0] == each[1]
            assert tie[:, :, plane].all() and int(tie.sum()) == tie[:, :, plane].size, (plane, connectivity)
            assert (want[1][tie] == 4).all() and {int(v) for v in np.unique(want[1])} == {4, 9}


# ---- 6. the seed rules, the outputs
def test_seed_rules_and_outputs(gpu_ctx):
    dev = Device(gpu_ctx)
    X, Y, Z = dims = (70, 9, 5)
    cost = cp.random_cost(dims, 12, 0.0)
    cost[2, 4, 10] = 0                     # a wall with a seed on it
    domain = np.ones((Z, Y, X), bool)
    domain[:, :, 35] = False               # two halves; the second has no effective seed
    domain[1, 1, 60] = False               # a seed outside the domain
    seeds = [(5, 5, 2, 9), (5, 5, 2, 3), (5, 5, 2, 12), (20, 3, 1, 3), (10, 4, 2, 1), (60, 1, 1, 2), (20, 3, 1, 3)]
    want = dev.check(cost, seeds, 6, (2, 3, 4), domain=domain)
    assert int(want[1][2, 5, 5]) == 3 and (want[1][:, :, 35:] == 0).all() and (want[0][:, :, 35:] == NONE).all()
    assert int(want[0][2, 4, 10]) == NONE and not (want[1] == 1).any() and not (want[1] == 2).any()
    for outputs in ("dist", "labels"):
        dev.check(cost, seeds, 6, (2, 3, 4), domain=domain, want=want, outputs=outputs)
    none = dev.check(cost, [(10, 4, 2, 1), (60, 1, 1, 2)], 26, cp.CHAMFER, domain=domain)
    assert g.result(none[0]) == {"reached": 0, "max_dist": 0}
    dev.check(np.zeros((Z, Y, X), np.uint16), seeds, 26)  # walls everywhere
    dev.check(cost, seeds, 26, cp.CHAMFER, domain=np.zeros((Z, Y, X), bool))
    for d in ((1, 1, 1), (7, 1, 1), (64, 3, 2), (65, 3, 2)):
        full = np.full(d[::-1], 3, np.uint16)
        want = dev.check(full, [(d[0] - 1, 0, d[2] - 1, 5)], 26, cp.CHAMFER)
        assert g.result(want[0])["reached"] == full.size


def test_seeds_from_labels(gpu_ctx):
    dev = Device(gpu_ctx)
    dims = (33, 18, 10)
    cost, domain, seeds, _, _ = cp.random_case(dims, 6, cp.CHAMFER, None, True)
    rng = np.random.default_rng(3)
    given = np.where(rng.random(cost.shape) < 0.01, rng.integers(1, 50, cost.shape), 0).astype(np.uint32)
    D = cp.in_domain(cost, domain)
    assert (given[D] != 0).sum() > 10 and (given[~D] != 0).sum() > 3, "nonzero words inside D and outside it"
    alone = dev.check(cost, None, 6, cp.CHAMFER, seed_labels=given, domain=domain)
    both = dev.check(cost, seeds, 6, cp.CHAMFER, seed_labels=given, domain=domain)
    assert not np.array_equal(alone[1], both[1])
    dev.check(cost, None, 6, cp.CHAMFER, seed_labels=given, domain=domain, want=alone, in_place=True)
    dev.check(cost, seeds, 26, cp.CHAMFER, seed_labels=given, in_place=True, outputs="labels")


# ---- 7. the second oracle: with cost 1 everywhere the call is clwh_mask_geodesic, device against device
@pytest.mark.parametrize("connectivity", BOTH)
def test_unit_cost_equals_mask_geodesic_on_the_device(gpu_ctx, connectivity):
    ctx = gpu_ctx
    for dims in ((33, 18, 10), (70, 9, 5), (65, 33, 9)):
        X, Y, Z = dims
        n = X * Y * Z
        domain = g.random_domain(dims, connectivity)
        seeds = g.random_seeds(domain, 5, 4)
        d_domain, d_cost = ctx.buffer_from(scene.mask_pack(domain)), ctx.buffer_from(np.ones((Z, Y, X), np.uint16))
        maps = [ctx.buffer(4 * n, np.uint32, (n,)) for _ in range(4)]
        for weights, cap in ((cp.CHAMFER, NONE), (cp.ANISO, 80), ((255, 1, 3), NONE)):
            a, ra = ctx.mask_geodesic_raw(d_domain, dims, seeds, None, flag_of(connectivity), weights, cap, maps[0], maps[1])
            b, rb = ctx.cost_geodesic_raw(d_cost, dims, seeds, d_domain, None, flag_of(connectivity), weights, cap, maps[2], maps[3])
            assert (a, b) == (0, 0) and ra.as_dict() == rb.as_dict() and ra.reached > 0
            same(maps[2].pull(), maps[0].pull(), (dims, weights, cap, "dist"))
            same(maps[3].pull(), maps[1].pull(), (dims, weights, cap, "labels"))
        for m in maps + [d_cost, d_domain]:
            m.release()


# ---- 8. the trace
@pytest.mark.parametrize("connectivity", BOTH)
def test_trace(gpu_ctx, connectivity):
    ctx = gpu_ctx
    dims = (33, 18, 10)
    m = cp.CHAMFER
    cost, domain, seeds, dist, labels = cp.random_case(dims, connectivity, m, None, True)
    d_cost, d_dist, d_labels = ctx.buffer_from(cost), ctx.buffer_from(dist), ctx.buffer_from(labels)
    reached = np.argwhere(dist != NONE)
    targets = [reached[np.argmax(dist[dist != NONE])]] + list(reached[:: len(reached) // 7])
    longest = 0
    for z, y, x in targets:
        for with_labels in (None, labels):
            want, complete = cp.trace(cost, dist, (x, y, z), connectivity, m, with_labels)
            assert complete
            for _ in range(2):
                got, n = ctx.cost_trace(d_cost, d_dist, dims, (x, y, z), d_labels if with_labels is not None else None, connectivity, m)
                assert n == len(want) and got.tolist() == [list(p) for p in want], (x, y, z)
            longest = max(longest, len(want))
            if len(want) > 3:  # a capacity below the count: the true count, the first points, nothing behind them
                buf = ctx.buffer_from(np.full(3 * len(want), PATTERN, np.uint32))
                status, n = ctx.cost_trace_raw(d_cost, d_dist, dims, (x, y, z), None if with_labels is None else d_labels,
                                               flag_of(connectivity), m, buf, 3)
                got = buf.pull()
                assert (status, n) == (0, len(want)) and got[:9].reshape(3, 3).tolist() == [list(p) for p in want[:3]]
                assert (got[9:] == PATTERN).all()
                assert ctx.cost_trace_raw(d_cost, d_dist, dims, (x, y, z), None, flag_of(connectivity), m, None, 0) == (0, len(want))
                buf.release()
    assert longest > 8
    z, y, x = np.argwhere(dist == NONE)[0]
    got, n = ctx.cost_trace(d_cost, d_dist, dims, (x, y, z), None, connectivity, m)
    assert n == 0 and len(got) == 0
    # doctored maps: a distance no neighbour explains; a wall under a positive distance.  The points so far, INVALID_VALUE
    z, y, x = targets[0]
    broken = dist.copy()
    broken[z, y, x] += 1
    walled = cost.copy()
    walled[z, y, x] = 0
    d_broken, d_walled = ctx.buffer_from(broken), ctx.buffer_from(walled)
    for c, d in ((d_cost, d_broken), (d_walled, d_dist)):
        buf = ctx.buffer_from(np.full(12, PATTERN, np.uint32))
        status, n = ctx.cost_trace_raw(c, d, dims, (x, y, z), None, flag_of(connectivity), m, buf, 4)
        assert (status, n) == (INVALID_VALUE, 1) and buf.pull().tolist() == [x, y, z] + [PATTERN] * 9
        buf.release()
    # a walk that breaks after two good steps
    want, _ = cp.trace(cost, dist, (x, y, z), connectivity, m)
    assert len(want) > 4
    bx, by, bz = want[2]
    later = dist.copy()
    later[bz, by, bx] -= 1  # the step from want[1] to it no longer sums; whatever the header's walk does then, the device does too
    ref_points, complete = cp.trace(cost, later, (x, y, z), connectivity, m)
    d_later = ctx.buffer_from(later)
    buf = ctx.buffer_from(np.full(3 * len(want), PATTERN, np.uint32))
    status, n = ctx.cost_trace_raw(d_cost, d_later, dims, (x, y, z), None, flag_of(connectivity), m, buf, len(want))
    assert status == (0 if complete else INVALID_VALUE) and n == len(ref_points)
    assert buf.pull()[:3 * n].reshape(n, 3).tolist() == [list(p) for p in ref_points]
    for b in (buf, d_later, d_walled, d_broken, d_labels, d_dist, d_cost):
        b.release()


# ---- 9. clwh_cost_from_field
def field_volume():
    """19 x 7 x 5 with -32768 and 32767 next to each other at a border, in a corner and inside"""
    v = np.random.default_rng(4).integers(-1200, 1200, (5, 7, 19)).astype(np.int16)
    v[0, 0, 0], v[0, 0, 1], v[0, 1, 0], v[1, 0, 0] = -32768, 32767, 32767, 32767
    v[4, 6, 18], v[4, 6, 17] = 32767, -32768
    v[2, 3, 8], v[2, 3, 10], v[2, 2, 9], v[2, 4, 9], v[1, 3, 9], v[3, 3, 9] = -32768, 32767, -32768, 32767, -32768, 32767
    return v


def test_cost_from_field(gpu_ctx):
    ctx = gpu_ctx
    vol = field_volume()
    dims = X, Y, Z = dims_of(vol)
    n = X * Y * Z
    assert int(cp.field_values(vol, cp.SRC_GRADIENT).max()) == 3 * 65535 ** 2
    words = np.random.default_rng(5).integers(0, 3000, (Z, Y, X)).astype(np.uint32)
    words[0, 0, 3], words[4, 6, 18], words[2, 2, 2] = NONE, NONE, 0
    domain = np.random.default_rng(6).random((Z, Y, X)) < 0.6
    image, d_words, d_domain = ctx.image_from(vol), ctx.buffer_from(words), ctx.buffer_from(scene.mask_pack(domain))
    out = ctx.buffer(2 * (n + 4), np.uint16, (n + 4,))
    rng = np.random.default_rng(7)
    tables = {k: rng.integers(0, 65536, k).astype(np.uint16) for k in (1, 2, 37, 65536)}
    sources = ((ffi.COST_SRC_U32, d_words, words), (ffi.COST_SRC_VALUE, image, vol), (ffi.COST_SRC_GRADIENT, image, vol))
    checked = 0
    for kind, source, host in sources:
        s = cp.field_values(host, kind)
        # lo below and above every value, at both ends, in the middle, and at the ends of int64
        for lo in (int(s.min()) - 5, int(s.min()), int(np.median(s)), int(s.max()), int(s.max()) + 5, 0, -2 ** 63, 2 ** 63 - 1):
            for shift in (0, 7, 40):
                for k in (65536, (1, 2, 37)[checked % 3]):  # the largest table, and the small ones in turn
                    table = tables[k]
                    for with_domain in (None, domain):
                        out.push(np.full(n + 4, 0x5A5A, np.uint16))
                        status = ctx.cost_from_field_raw(source, out, dims, table, lo, shift, kind, d_domain if with_domain is not None else None)
                        got = out.pull()
                        want = cp.cost_from_field(host, table, lo, shift, kind, with_domain)
                        assert status == 0 and (got[n:] == 0x5A5A).all(), (kind, lo, shift, k)
                        same(got[:n].reshape(Z, Y, X), want, (kind, lo, shift, k, with_domain is not None))
                        checked += 1
    assert checked > 100
    # two calls in a row with different tables: the second table's copy waits for the first
    a = ctx.cost_from_field(d_words, dims, tables[37], 0, 3)
    b = ctx.cost_from_field(d_words, dims, tables[65536], 0, 0)
    same(a.pull(), cp.cost_from_field(words, tables[37], 0, 3), "first of two")
    same(b.pull(), cp.cost_from_field(words, tables[65536], 0, 0), "second of two")
    assert np.array_equal(d_words.pull(), words) and np.array_equal(image.pull().reshape(vol.shape), vol)
    for m in (a, b, out, d_domain, d_words, image):
        m.release()


# ---- 10. the centreline, end to end
def test_centerline_of_the_tube(gpu_ctx):
    ctx = gpu_ctx
    mask, start, end = cp.tube()
    want, _ = cp.tube_paths()
    dims = dims_of(mask)
    words = scene.mask_pack(mask)
    m = ctx.buffer_from(words)
    for _ in range(2):
        points, n = ctx.centerline(m, dims, start, end)
        assert n == len(want) and points.tolist() == [list(p) for p in want]
    short, n = ctx.centerline(m, dims, start, end, capacity=5)  # a first guess that is too small
    assert n == len(want) and short.tolist() == [list(p) for p in want]
    # a radius of interest instead of the pulled maximum; a start or an end outside the mask
    for max_radius in (2.0, 6.0):
        ref = cp.centerline(mask, start, end, max_radius=max_radius)[0]
        points, n = ctx.centerline(m, dims, start, end, max_radius=max_radius)
        assert n == len(ref) and points.tolist() == [list(p) for p in ref], max_radius
    assert not mask[0, 0, 0]
    assert ctx.centerline(m, dims, (0, 0, 0), end)[1] == 0 and ctx.centerline(m, dims, start, (0, 0, 0))[1] == 0
    with pytest.raises(ValueError):
        ctx.centerline(m, dims, start, end, spacing=(1, 1, 30))
    assert np.array_equal(m.pull(), words)
    assert scene.path_length(points) > 0
    m.release()


def tube_volume():
    return np.where(cp.tube()[0], 100, 0).astype(np.int16)


def test_host_mirror_centerline():
    """renderer::centerline through the host library: the same bytes"""
    mask, start, end = cp.tube()
    want, _ = cp.tube_paths()
    vol = tube_volume()
    Z, Y, X = vol.shape
    env = scene.env_map(64, 32)
    L = host_lib(clvr_host_grow_region=(None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p]),
                 clvr_host_centerline=(C.c_ulonglong, [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.c_int, C.c_float, C.c_uint,
                                                       C.c_void_p, C.c_ulonglong]))
    h = L.clvr_host_create()
    try:
        L.clvr_host_load(h, vol.ctypes.data, X, Y, Z, env.ctypes.data, 64, 32)
        click = np.array(start, np.uint32)
        grown = ffi.GrowResult()
        L.clvr_host_grow_region(h, click.ctypes.data, 1, 100, 100, 0, C.byref(grown))
        assert grown.count == int(mask.sum())
        out = np.zeros((400, 3), np.uint32)
        for max_radius, ref in ((0.0, want), (6.0, cp.centerline(mask, start, end, max_radius=6.0)[0])):
            n = L.clvr_host_centerline(h, (C.c_uint * 3)(*start), (C.c_uint * 3)(*end), ffi.GEO_26, max_radius, 100, out.ctypes.data, 400)
            assert n == len(ref) and out[:n].tolist() == [list(p) for p in ref], max_radius
        assert L.clvr_host_centerline(h, (C.c_uint * 3)(*start), (C.c_uint * 3)(0, 0, 0), ffi.GEO_26, 0.0, 100, out.ctypes.data, 400) == 0
    finally:
        L.clvr_host_destroy(h)


def test_headless_centerline(tmp_path):
    mask, start, end = cp.tube()
    want, _ = cp.tube_paths()
    scene.write_nrrd(str(tmp_path / "v.nrrd"), tube_volume())
    scene.write_hdr(str(tmp_path / "e.hdr"), scene.float_to_rgbe(np.random.default_rng(5).random((16, 32, 3), dtype=np.float32)))
    exe = os.path.join(ROOT, "cl_volume_renderer_amd", "clvr_headless")
    files = [str(tmp_path / "v.nrrd"), str(tmp_path / "e.hdr"), "1", "64", "64", str(tmp_path / "out")]

    def run(*options):
        out = subprocess.run([exe] + list(options) + files, capture_output=True, text=True, timeout=120)
        return out.returncode, [json.loads(s) for s in out.stdout.strip().splitlines() if s.startswith("{")], out.stderr

    grow = "--grow=%d,%d,%d,100,100" % start
    code, lines, err = run(grow + ",centerline=%d,%d,%d,measure" % end, "--mesh=50")
    assert code == 0, err
    assert lines[0]["count"] == int(mask.sum()) and lines[1]["measure"]["count"] == int(mask.sum())
    assert lines[2] == {"centerline": {"from": list(start), "to": list(end), "points": len(want)}}
    text = open(str(tmp_path / "out") + ".centerline.txt").read().splitlines()
    assert [[int(v) for v in s.split()] for s in text] == [list(p) for p in want[::-1]], "one x y z line each, the seed first"
    code, lines, err = run(grow + ",centerline=0,0,0", "--mesh=50")
    assert code == 0 and lines[1]["centerline"]["points"] == 0, err
    assert len(run(grow, "--mesh=50")[1]) == len(lines) - 1  # no item: no line
    for bad in ("centerline=", "centerline=1,2", "centerline=1,2,x", "centerline=1,2,3,centerline=1,2,3", "centerline=1,2,-3", "centerline",
                "centerline=1,2,", "centerline=999,2,3"):
        assert run(grow + "," + bad, "--mesh=50")[0] == 1, bad


# ---- 11. status
def test_status_codes_and_nothing_written(gpu_ctx):
    ctx = gpu_ctx
    dims = X, Y, Z = (70, 12, 9)
    n, words = X * Y * Z, scene.mask_words_per_row(X) * Y * Z
    fill = lambda k: ctx.buffer_from(np.full(k, PATTERN, np.uint32))
    domain, short_domain = fill(words), fill(words - 1)
    cost, short_cost = fill(n // 2), fill(n // 2 - 1)  # n is even: 2 * n bytes exactly, and two bytes less
    assert n % 2 == 0
    dist, labels, given, short_map, points, short_points = fill(n + 4), fill(n + 4), fill(n), fill(n - 1), fill(30), fill(29)
    out_cost, short_out = fill(n // 2 + 2), fill(n // 2 - 1)
    as_image = ctx.image([4, 4, n // 16 + 1], 1, np.uint32)
    volume = ctx.image_from(np.zeros((Z, Y, X), np.int16))
    wrong_kind = ctx.image_from(np.zeros((Z, Y, X), np.uint16))
    other_dims = ctx.image_from(np.zeros((Z, Y, X + 1), np.int16))
    odd_domain = ctx.wrap(domain.device_ptr + 4, 4 * words - 4)
    odd_map = ctx.wrap(dist.device_ptr + 2, 4 * n)
    odd_cost = ctx.wrap(dist.device_ptr + 1, 2 * n)
    table = np.arange(1, 9, dtype=np.uint16)
    seeds = [(1, 2, 3, 4)]
    bad_dims = ((0, 12, 9), (70, 0, 9), (70, 12, 0), (1 << 31, 1, 1), (1 << 16, 1 << 15, 1))
    m6 = lambda *face: (face, (0, 0, 0), 0)  # edge and corner multipliers are not in use without CLWH_GEO_26
    bad_mult_6 = (m6(0, 1, 1), m6(1, 0, 1), m6(1, 1, 0), m6(256, 1, 1), m6(1, 1, 1 << 31))
    bad_mult_26 = (((1, 1, 1), (0, 1, 1), 1), ((1, 1, 1), (1, 1, 256), 1), ((1, 1, 1), (1, 1, 1), 0), ((1, 1, 1), (1, 1, 1), 256),
                   ((1, 0, 1), (1, 1, 1), 1))

    def geo(**kw):
        args = dict(cost=cost, dims=dims, seeds=seeds, domain=domain, seed_labels=None, flags=0, multipliers=None, cap=NONE, dist=dist,
                    labels=labels)
        args.update(kw)
        return ctx.cost_geodesic_raw(**args)[0]

    def trace(**kw):
        args = dict(cost=cost, dist=given, dims=dims, target=(1, 2, 3), labels=None, flags=0, multipliers=None, points=points, capacity=10)
        args.update(kw)
        return ctx.cost_trace_raw(**args)[0]

    def field(**kw):
        args = dict(source=given, cost=out_cost, dims=dims, table=table, lo=0, shift=0, kind=ffi.COST_SRC_U32, domain=None, flags=0)
        args.update(kw)
        return ctx.cost_from_field_raw(**args)

    L = ffi.lib()
    for name, desc in (("clwh_cost_geodesic", ffi.CostGeodesicDesc()), ("clwh_cost_trace", ffi.CostTraceDesc()),
                       ("clwh_cost_from_field", ffi.CostFieldDesc())):
        assert getattr(L, name)(None, C.byref(desc)) == INVALID_VALUE and getattr(L, name)(ctx.h, None) == INVALID_VALUE
    cases = [geo(result=False), trace(result=False), field(table=None, n=8)]
    for bad in (None, as_image, odd_cost):
        cases += [geo(cost=bad), trace(cost=bad), field(cost=bad)]
    cases += [geo(domain=bad) for bad in (as_image, odd_domain)] + [field(domain=bad) for bad in (as_image, odd_domain)]
    cases += [geo(dist=None, labels=None)]
    for bad in (as_image, odd_map):
        cases += [geo(dist=bad), geo(labels=bad), geo(dist=None, labels=bad), geo(seed_labels=bad, flags=ffi.GEO_FROM_LABELS)]
        cases += [trace(dist=bad), trace(labels=bad), trace(points=bad), field(source=bad)]
    cases += [geo(seed_labels=None, flags=ffi.GEO_FROM_LABELS), trace(dist=None), trace(points=None), field(source=None)]
    cases += [geo(flags=8), geo(flags=-1), geo(flags=1 << 16), trace(flags=2), trace(flags=4), trace(flags=-1), field(flags=1)]
    for kind in (ffi.COST_SRC_VALUE, ffi.COST_SRC_GRADIENT):  # anything but the S16 volume image of these dims
        cases += [field(source=bad, kind=kind) for bad in (None, given, wrong_kind, other_dims)]
    cases += [field(source=volume), field(kind=3), field(kind=-1), field(source=volume, kind=3)]
    cases += [field(table=table, n=0), field(table=table, n=65537), field(shift=41), field(shift=1 << 31)]
    for bad in bad_dims:
        cases += [geo(dims=bad), trace(dims=bad), field(dims=bad)]
    for bad in bad_mult_6:
        cases += [geo(multipliers=bad[0]), trace(multipliers=bad[0]), geo(multipliers=bad[0], flags=ffi.GEO_26)]
    for bad in bad_mult_26:
        cases += [geo(multipliers=bad, flags=ffi.GEO_26), trace(multipliers=bad, flags=ffi.GEO_26)]
    cases += [geo(cap=ffi.COST_CAP_MAX + 1), geo(cap=NONE - 1)]
    cases += [geo(seeds=[(1, 2, 3, 4)] * (ffi.GROW_MAX_SEEDS + 1)), geo(seeds=None), geo(seeds=[]), geo(seeds=None, seed_labels=given)]
    cases += [geo(seeds=[(1, 2, 3, 4), bad]) for bad in ((70, 2, 3, 4), (1, 12, 3, 4), (1, 2, 9, 4), (1, 2, 3, 0))]
    cases += [trace(target=bad) for bad in ((70, 2, 3), (1, 12, 3), (1, 2, 9))]
    assert cases == [INVALID_VALUE] * len(cases), cases
    # n_seeds > 0 with NULL seeds
    d, res = ffi.CostGeodesicDesc(), ffi.GeodesicResult()
    d.cost, d.dist, d.n_seeds, d.result, d.cap = cost.h, dist.h, 1, C.pointer(res), NONE
    for k in range(3):
        d.dims[k], d.mult_face[k] = dims[k], 1
    assert L.clwh_cost_geodesic(ctx.h, C.byref(d)) == INVALID_VALUE
    sizes = [geo(cost=short_cost), geo(domain=short_domain), geo(dist=short_map), geo(labels=short_map),
             geo(seed_labels=short_map, flags=ffi.GEO_FROM_LABELS), trace(cost=short_cost), trace(dist=short_map), trace(labels=short_map),
             trace(points=short_points), field(source=short_map), field(cost=short_out), field(domain=short_domain),
             field(source=volume, kind=ffi.COST_SRC_VALUE, cost=short_out)]
    assert sizes == [SIZE_MISMATCH] * len(sizes), sizes
    # INVALID_VALUE before SIZE_MISMATCH
    assert geo(cost=short_cost, multipliers=(0, 1, 1)) == INVALID_VALUE and geo(domain=short_domain, seeds=[(1, 2, 3, 0)]) == INVALID_VALUE
    assert trace(points=short_points, target=(70, 2, 3)) == INVALID_VALUE and field(cost=short_out, shift=41) == INVALID_VALUE
    for m in (domain, short_domain, cost, short_cost, dist, labels, given, short_map, points, short_points, out_cost, short_out):
        assert (m.pull(np.uint32, (m.nbytes // 4,)) == PATTERN).all()  # nothing was written
    # and the same arguments without the defect are accepted, limits included
    assert geo() == 0 and geo(multipliers=m6(255, 1, 255), cap=ffi.COST_CAP_MAX) == 0 and geo(cap=0, flags=ffi.GEO_DENSE, dist=None) == 0
    assert geo(domain=None) == 0 and geo(seed_labels=as_image) == 0, "no domain; seed_labels ignored without the flag"
    assert geo(seeds=None, seed_labels=given, flags=ffi.GEO_FROM_LABELS) == 0
    assert (dist.pull()[n:] == PATTERN).all() and (labels.pull()[n:] == PATTERN).all() and (domain.pull() == PATTERN).all()
    pattern_cost = np.full(n // 2, PATTERN, np.uint32).view(np.uint16).reshape(Z, Y, X)
    want = cp.cost_geodesic(pattern_cost, None, 6, None, None, np.full((Z, Y, X), PATTERN, np.uint32),
                            scene.mask_unpack(np.full(words, PATTERN, np.uint32), dims))
    same(dist.pull()[:n].reshape(Z, Y, X), want[0], "the pattern as cost, as domain and as labels")
    assert trace(dist=dist, points=short_points, capacity=9) == 0 and trace(dist=dist, points=None, capacity=0) == 0
    assert field() == 0 and field(table=np.ones(65536, np.uint16), shift=40, lo=-2 ** 63) == 0 and field(domain=domain) == 0
    assert field(source=volume, kind=ffi.COST_SRC_VALUE) == 0 and field(source=volume, kind=ffi.COST_SRC_GRADIENT, lo=2 ** 63 - 1) == 0
    assert (out_cost.pull()[n // 2:] == PATTERN).all()
    for x in (odd_cost, odd_map, odd_domain, other_dims, wrong_kind, volume, as_image, short_out, out_cost, short_points, points, short_map,
              given, labels, dist, short_cost, cost, short_domain, domain):
        x.release()
