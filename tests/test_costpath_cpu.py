"""The contract of clwh_cost_geodesic / clwh_cost_trace / clwh_cost_from_field as tests/costpath_ref.py restates it, pinned without a
device: against scipy's Dijkstra on the directed graph taken literally, against tests/geodesic_ref.py where the cost is 1, the trace
against the map, the centreline's table, and the tube the feature is for."""
import ctypes as C

import numpy as np
import pytest

from cl_volume_renderer_amd import ffi, scene
from tests import costpath_ref as cp
from tests import geodesic_ref as g

NONE = cp.NONE


def scipy_maps(cost, seeds, connectivity, multipliers, cap, domain=None):
    """(dist, labels) from scipy.sparse.csgraph.dijkstra: an edge q -> p of weight mult(p - q) * cost(p) for every pair of neighbours
    in D, one run per seed voxel; the label is the smallest id among the seeds that attain the minimum"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra

    D = cp.in_domain(cost, domain)
    Z, Y, X = D.shape
    flat = lambda x, y, z: (z * Y + y) * X + x
    rows, cols, vals = [], [], []
    for z, y, x in np.argwhere(D):
        for dx, dy, dz, m in cp.steps(connectivity, multipliers):
            qx, qy, qz = x - dx, y - dy, z - dz  # the step (dx, dy, dz) from q enters p = (x, y, z)
            if 0 <= qx < X and 0 <= qy < Y and 0 <= qz < Z and D[qz, qy, qx]:
                rows.append(flat(qx, qy, qz))
                cols.append(flat(x, y, z))
                vals.append(float(m * int(cost[z, y, x])))
    graph = csr_matrix((vals, (rows, cols)), shape=(D.size, D.size))
    keys = g.seed_keys(D, seeds)
    dist = np.full(D.size, np.inf)
    labels = np.zeros(D.size, np.uint32)
    if keys:
        sources = sorted(keys, key=lambda p: keys[p])  # ascending id: the first seed that attains the minimum has the smallest
        each = dijkstra(graph, directed=True, indices=[flat(*p) for p in sources])
        dist = each.min(axis=0)
        labels = np.array([keys[sources[k]] for k in each.argmin(axis=0)], np.uint32)
    reached = dist <= cap
    out = np.where(reached, dist, NONE).astype(np.uint32)
    return out.reshape(D.shape), np.where(reached, labels, 0).astype(np.uint32).reshape(D.shape)


@pytest.mark.parametrize("connectivity", (6, 26))
def test_reference_equals_scipy_on_the_literal_graph(connectivity):
    rng = np.random.default_rng(2)
    dims = X, Y, Z = (9, 7, 5)
    for trial, (high, multipliers) in enumerate(((4, cp.CHAMFER), (65536, cp.ANISO), (3, cp.UNIT))):  # small costs: many ties
        cost = rng.integers(0, high, (Z, Y, X)).astype(np.uint16)
        domain = rng.random((Z, Y, X)) < 0.85 if trial != 1 else None
        seeds = cp.random_seeds(cp.in_domain(cost, domain), trial)
        free = cp.cost_geodesic(cost, seeds, connectivity, multipliers, None, None, domain)
        for cap in (cp.CAP_MAX, int(np.median(free[0][free[0] != NONE]))):
            want = scipy_maps(cost, seeds, connectivity, multipliers, cap, domain)
            got = cp.cost_geodesic(cost, seeds, connectivity, multipliers, cap, None, domain)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (trial, cap)
        assert (free[0] != NONE).sum() > 50 and len(np.unique(free[1])) > 2


@pytest.mark.parametrize("connectivity", (6, 26))
def test_unit_cost_is_the_mask_geodesic(connectivity):
    for dims in ((17, 17, 9), (33, 18, 10)):
        domain = g.random_domain(dims, connectivity)
        seeds = g.random_seeds(domain, 5, 4)
        labels = np.where(np.random.default_rng(1).random(domain.shape) < 0.01, 11, 0).astype(np.uint32)
        for weights, cap in ((g.CHAMFER, None), (g.ANISO, 60), ((3, 5, 11), None)):
            want = g.geodesic(domain, seeds, connectivity, weights, cap, labels)
            as_domain = cp.cost_geodesic(np.ones(domain.shape, np.uint16), seeds, connectivity, weights, cap, labels, domain)
            as_walls = cp.cost_geodesic(domain.astype(np.uint16), seeds, connectivity, weights, cap, labels)
            for got in (as_domain, as_walls):
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (dims, weights, cap)


@pytest.mark.parametrize("connectivity", (6, 26))
def test_traced_paths_sum_to_the_distance(connectivity):
    cost, domain, seeds, dist, labels = cp.random_case((33, 18, 10), connectivity, cp.CHAMFER, None, True)
    reached = np.argwhere(dist != NONE)
    assert len(reached) > 1000
    longest = 0
    for z, y, x in reached[:: len(reached) // 40]:
        for with_labels in (None, labels):
            points, complete = cp.trace(cost, dist, (x, y, z), connectivity, cp.CHAMFER, with_labels)
            assert complete and points[0] == (x, y, z) and int(dist[points[-1][2], points[-1][1], points[-1][0]]) == 0
            assert cp.path_cost(cost, points, connectivity, cp.CHAMFER) == int(dist[z, y, x])
            assert with_labels is None or len({int(labels[p[2], p[1], p[0]]) for p in points}) == 1
            longest = max(longest, len(points))
    assert longest > 8
    z, y, x = np.argwhere(dist == NONE)[0]
    assert cp.trace(cost, dist, (x, y, z), connectivity, cp.CHAMFER) == ([], True)
    # doctored maps end the walk: a distance no neighbour explains, a wall under a positive distance
    z, y, x = reached[np.argmax(dist[dist != NONE])]
    broken = dist.copy()
    broken[z, y, x] += 1
    assert cp.trace(cost, broken, (x, y, z), connectivity, cp.CHAMFER) == ([(x, y, z)], False)
    walled = cost.copy()
    walled[z, y, x] = 0
    assert cp.trace(walled, dist, (x, y, z), connectivity, cp.CHAMFER) == ([(x, y, z)], False)


def test_highway_paths_are_longer_in_steps_than_the_shortest():
    """the case the GPU test stands on: the cheap corridor's detour beats the direct route, so final predecessor chains have more steps
    than the unit-cost shortest path"""
    for connectivity in (6, 26):
        cost, dist, _ = cp.highway_case(connectivity)
        unit = g.geodesic(np.ones(cost.shape, bool), [cp.HIGHWAY_SEED], connectivity)[0]
        target = (2, 34, 3)
        points, complete = cp.trace(cost, dist, target, connectivity, cp.CHAMFER)
        assert complete and len(points) - 1 > 5 * int(unit[target[2], target[1], target[0]])
        assert int(dist[target[2], target[1], target[0]]) < 10 * 1000  # far below the field's direct route of 32 steps


def test_cost_from_field_reference_by_hand():
    words = np.array([[[0, 5, 9, 1000, NONE]]], np.uint32)
    table = np.array([7, 6, 5, 4], np.uint16)
    assert cp.cost_from_field(words, table).tolist() == [[[7, 4, 4, 4, 4]]]
    assert cp.cost_from_field(words, table, lo=4, shift=1).tolist() == [[[7, 7, 5, 4, 4]]]
    assert cp.cost_from_field(words, table, lo=2 ** 63 - 1).tolist() == [[[7] * 5]]
    assert cp.cost_from_field(words, table, lo=-2 ** 63, shift=40).tolist() == [[[4] * 5]]
    assert cp.cost_from_field(words, table, domain=words < 9).tolist() == [[[7, 4, 0, 0, 0]]]
    v = np.array([[[-32768, 32767, 0]]], np.int16)
    assert cp.field_values(v, cp.SRC_GRADIENT).tolist() == [[[65535 ** 2, 32768 ** 2, 32767 ** 2]]]
    corner = np.array([[[-32768, 32767], [32767, 0]], [[32767, 0], [0, 0]]], np.int16)
    assert int(cp.field_values(corner, cp.SRC_GRADIENT)[0, 0, 0]) == 3 * 65535 ** 2 > 2 ** 33
    assert cp.cost_from_field(v, table, lo=-32768, shift=14, kind=cp.SRC_VALUE).tolist() == [[[7, 4, 5]]]


def test_centerline_table():
    for r, sharpness in ((1, 100), (5184, 100), (65535, 65534), (300, 0), (77, 1)):
        t = scene.centerline_cost_table(r, sharpness)
        assert t.dtype == np.uint16 and len(t) == r + 1
        assert int(t[0]) == 1 + sharpness and int(t[-1]) == 1 and (np.diff(t.astype(np.int64)) <= 0).all()
        assert [int(t[d]) for d in (0, r // 2, r)] == [1 + (sharpness * (r - d) ** 2) // (r * r) for d in (0, r // 2, r)]
    assert scene.centerline_cost_table(4).tolist() == [101, 57, 26, 7, 1]
    for bad in ((0, 100), (65536, 100), (10, 65535), (10, -1)):
        with pytest.raises(ValueError):
            scene.centerline_cost_table(*bad)
    assert [scene.centerline_shift(r) for r in (1, 65535, 65536, 2 ** 20)] == [0, 0, 1, 5]
    assert scene.path_length([(0, 0, 0), (1, 0, 0), (2, 1, 0), (3, 2, 1)], (0.5, 0.5, 2.0)) == pytest.approx(0.5 + 0.5 ** 0.5 + 4.5 ** 0.5)
    assert scene.path_length([(4, 4, 4)]) == 0.0 and scene.path_length([]) == 0.0


def test_new_entry_points_refuse_a_null_context_without_a_device():
    L = ffi.lib()
    res, n = ffi.GeodesicResult(7, 7, 7), C.c_uint64(7)
    geo, tr, field = ffi.CostGeodesicDesc(), ffi.CostTraceDesc(), ffi.CostFieldDesc()
    geo.result, tr.n_points = C.pointer(res), C.pointer(n)
    assert L.clwh_cost_geodesic(None, C.byref(geo)) == 1 and L.clwh_cost_trace(None, C.byref(tr)) == 1  # CLWH_ERR_INVALID_VALUE
    assert L.clwh_cost_from_field(None, C.byref(field)) == 1
    assert (res.reached, res.max_dist, res.rounds, n.value) == (7, 7, 7, 7), "nothing written"
    assert (ffi.COST_CAP_MAX, ffi.COST_SRC_U32, ffi.COST_SRC_VALUE, ffi.COST_SRC_GRADIENT) == (0xFF000000, 0, 1, 2)


def test_the_centreline_stays_nearer_the_tube_axis_than_the_shortest_path():
    """two references compared, no threshold: the cost-field path against the plain chamfer path between the same two voxels"""
    mask, start, end = cp.tube()
    assert mask.shape == (14, 44, 44) and mask[start[2], start[1], start[0]] and mask[end[2], end[1], end[0]]
    assert cp.off_axis([start, end]).max() < 1.0, "the clicks are on the axis"
    centre, plain = cp.tube_paths()
    assert centre[0] == end and centre[-1] == start and plain[0] == end and plain[-1] == start
    assert all(mask[z, y, x] for x, y, z in centre)
    worst_centre, worst_plain = float(cp.off_axis(centre).max()), float(cp.off_axis(plain).max())
    print("largest distance from the axis: centreline %.2f, shortest path %.2f" % (worst_centre, worst_plain))
    assert worst_centre < worst_plain
    assert scene.path_length(centre) > scene.path_length(plain), "the shortest path cuts the bend"
