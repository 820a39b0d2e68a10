"""tests/geodesic_ref.py checked against the definition of clwh_mask_geodesic taken literally, against scipy's Dijkstra, and against
closed forms, so that the GPU tests compare with something pinned; the split workflow on the references; and the trace rule."""
import os
import re

import numpy as np
import pytest
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import dijkstra

from cl_volume_renderer_amd import ffi, scene
from tests import geodesic_ref as g
from tests.grow_ref import RANDOM_DIMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = g.NONE
WEIGHTS = (g.UNIT, g.ANISO, g.CHAMFER)


def graph_of(domain, connectivity, weights):
    """the weighted graph of the definition as a sparse matrix over flat voxel indices: an edge for every step between two voxels of D"""
    Z, Y, X = domain.shape
    flat = np.arange(domain.size).reshape(domain.shape)
    rows, cols, costs = [], [], []
    for dx, dy, dz, w in g.steps(connectivity, weights):
        src = (slice(max(0, -dz), Z - max(0, dz)), slice(max(0, -dy), Y - max(0, dy)), slice(max(0, -dx), X - max(0, dx)))
        dst = (slice(max(0, dz), Z - max(0, -dz)), slice(max(0, dy), Y - max(0, -dy)), slice(max(0, dx), X - max(0, -dx)))
        both = domain[src] & domain[dst]
        rows.append(flat[src][both])
        cols.append(flat[dst][both])
        costs.append(np.full(int(both.sum()), w, np.float64))
    return csr_matrix((np.concatenate(costs), (np.concatenate(rows), np.concatenate(cols))), shape=(domain.size, domain.size))


def literal(domain, seeds, connectivity, weights, cap=None):
    """one single-source search per seed inside D (scipy's), then the minimum and the smallest id among the arg-minima; the cap last"""
    Z, Y, X = domain.shape
    inside = [s for s in seeds if domain[s[2], s[1], s[0]]]
    per_seed = dijkstra(graph_of(domain, connectivity, weights), directed=True, indices=[(s[2] * Y + s[1]) * X + s[0] for s in inside])
    best = per_seed.min(axis=0)
    ids = np.array([s[3] for s in inside], np.float64)
    label = np.where(per_seed == best[None, :], ids[:, None], np.inf).min(axis=0)
    reached = np.isfinite(best) & (best <= (g.CAP_MAX if cap is None else cap))
    dist = np.where(reached, best, NONE).astype(np.uint32).reshape(domain.shape)
    return dist, np.where(reached, label, 0).astype(np.uint32).reshape(domain.shape)


def test_weights_from_spacing():
    assert scene.geodesic_weights((1, 1, 1), 10) == g.CHAMFER
    assert scene.geodesic_weights((0.7, 0.7, 2.5), 10) == g.ANISO
    assert scene.geodesic_weights((1, 1, 1), 1) == ((1, 1, 1), (1, 1, 1), 2)  # sqrt 2 rounds down, sqrt 3 up
    assert scene.geodesic_weights((1e-6, 1, 1), 16)[0][0] == 1  # never below 1
    with pytest.raises(ValueError):
        scene.geodesic_weights((1, 1, 5000), 16)


@pytest.mark.parametrize("connectivity", (6, 26))
@pytest.mark.parametrize("dims", RANDOM_DIMS)
def test_reference_equals_the_definition(dims, connectivity):
    domain = g.random_domain(dims, connectivity)
    for weights in WEIGHTS:
        for cap in (None, 40 * min(g.normalise(weights)[0])):
            _, seeds, dist, labels = g.random_case(dims, connectivity, weights, cap)
            want_dist, want_labels = literal(domain, seeds, connectivity, weights, cap)
            assert np.array_equal(dist, want_dist), (dims, connectivity, weights, cap)
            assert np.array_equal(labels, want_labels), (dims, connectivity, weights, cap)
            assert ((dist == NONE) == (labels == 0)).all() and (dist[~domain] == NONE).all()
            reached = g.result(dist)["reached"]
            assert 0 < reached < int(domain.sum()), "some of D is reached and some is not"
            if cap is not None:
                assert reached < g.result(g.random_case(dims, connectivity, weights, None)[2])["reached"], "the cap cuts"
    if dims == (70, 40, 36) and connectivity == 6:
        assert int(domain.sum()) == 36224 and g.result(g.random_case(dims, 6, g.CHAMFER, None)[2])["reached"] == 26818


@pytest.mark.parametrize("connectivity", (6, 26))
@pytest.mark.parametrize("dims", ((65, 17, 17), (70, 40, 36)))
def test_many_seeds_equal_one_search_per_seed(dims, connectivity):
    """the definition once more without scipy: the reference's own search from one seed at a time, the minimum, the smallest id among
    the arg-minima"""
    domain, seeds, dist, labels = g.random_case(dims, connectivity, g.CHAMFER, None)
    inside = [s for s in seeds if domain[s[2], s[1], s[0]]]
    assert len(inside) == len(seeds) - 1 and len({s[:3] for s in inside}) < len(inside), "a seed outside D, and a voxel with several ids"
    alone = np.stack([g.geodesic(domain, [s], connectivity, g.CHAMFER)[0] for s in inside]).astype(np.int64)
    best = alone.min(axis=0)
    ids = np.array([s[3] for s in inside], np.int64)
    smallest = np.where(alone == best[None], ids[:, None, None, None], np.int64(1) << 40).min(axis=0)
    assert np.array_equal(dist, best.astype(np.uint32))
    assert np.array_equal(labels, np.where(best == NONE, 0, smallest).astype(np.uint32))


def test_closed_forms_in_a_box():
    X, Y, Z = 13, 9, 7
    box = np.ones((Z, Y, X), bool)
    sx, sy, sz = 4, 2, 5
    z, y, x = np.indices(box.shape)
    ax, ay, az = abs(x - sx), abs(y - sy), abs(z - sz)
    dist, labels = g.geodesic(box, [(sx, sy, sz, 9)], 6, (3, 5, 11))
    assert np.array_equal(dist, (3 * ax + 5 * ay + 11 * az).astype(np.uint32)) and (labels == 9).all()
    dist, _ = g.geodesic(box, [(sx, sy, sz, 9)], 26, g.CHAMFER)
    s = np.sort(np.stack([ax, ay, az]), axis=0)  # the chamfer 10 / 14 / 17: corner steps, then edge steps, then face steps
    assert np.array_equal(dist, (17 * s[0] + 14 * (s[1] - s[0]) + 10 * (s[2] - s[1])).astype(np.uint32))


def test_mirrored_seeds_tie_on_the_plane_between_them():
    box = np.ones((5, 6, 9), bool)
    seeds = [(6, 2, 2, 8), (2, 2, 2, 5)]
    for connectivity, weights in ((6, (3, 5, 11)), (26, g.CHAMFER)):
        tie = g.ties(box, seeds, connectivity, weights)
        assert tie[:, :, 4].all() and not tie[:, :, :4].any() and not tie[:, :, 5:].any()
        _, labels = g.geodesic(box, seeds, connectivity, weights)
        assert (labels[tie] == 5).all() and (labels[:, :, 5:] == 8).all(), "the smaller id wins a tie, and only a tie"


def test_split_of_two_balls():
    mask, ranks, labels, n_parts = g.two_balls_split()
    assert int(mask.sum()) == 4765
    assert n_parts == 2 and np.bincount(ranks.reshape(-1)).tolist() == [72 * 24 * 24 - 236, 129, 107]
    assert (labels[mask] != 0).all() and (labels[~mask] == 0).all(), "every voxel of the mask is labelled, and nothing else"
    assert np.bincount(labels.reshape(-1)).tolist() == [72 * 24 * 24 - 4765, 3013, 1752]
    assert {int(labels[12, 12, 56]), int(labels[12, 12, 70])} == {1, 2}, "each ball's centre in a part of its own"
    # non-vacuity of ties: the territories meet where both pieces are equally near, and there the smaller label wins
    pieces = [(int(x), int(y), int(z), int(ranks[z, y, x])) for z, y, x in np.argwhere(ranks != 0)]
    tie = g.ties(mask, pieces)
    assert int(tie.sum()) == 101 and (labels[tie] == 1).all()


@pytest.mark.parametrize("connectivity", (6, 26))
def test_trace_follows_a_shortest_path(connectivity):
    dims = (70, 40, 36)
    for weights in (g.UNIT, g.CHAMFER):
        domain, seeds, dist, labels = g.random_case(dims, connectivity, weights, None)
        seeded = g.seed_keys(domain, seeds)
        reached = np.argwhere(dist != NONE)
        for z, y, x in reached[:: max(1, len(reached) // 12)]:
            for with_labels in (None, labels):
                points, complete = g.trace(dist, (x, y, z), connectivity, weights, with_labels)
                assert complete and points[0] == (x, y, z)
                assert g.path_cost(points, connectivity, weights) == int(dist[z, y, x])
                assert all(domain[p[2], p[1], p[0]] for p in points)
                assert int(dist[points[-1][2], points[-1][1], points[-1][0]]) == 0 and points[-1] in seeded
                if with_labels is not None:
                    assert seeded[points[-1]] == int(labels[z, y, x]), "it ends on a seed of the target's label"
        z, y, x = np.argwhere(domain & (dist == NONE))[0]
        assert g.trace(dist, (x, y, z), connectivity, weights) == ([], True)
    broken = dist.copy()
    z, y, x = np.argwhere((dist != NONE) & (dist > 0))[-1]
    broken[z, y, x] += 1  # no neighbour is exactly one step nearer any more
    points, complete = g.trace(broken, (x, y, z), connectivity, weights)
    assert points == [(int(x), int(y), int(z))] and not complete


def test_header_and_binding_declare_the_entry_points():
    with open(os.path.join(ROOT, "include", "clwh.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("clwh_mask_geodesic", "clwh_geodesic_trace"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in ffi.EXPORTED_SYMBOLS
    for name in ("CLWH_GEO_26", "CLWH_GEO_FROM_LABELS", "CLWH_GEO_DENSE"):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, getattr(ffi, name[5:])), header), name
