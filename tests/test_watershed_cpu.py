"""clwh_watershed's reference against the definition taken literally, against the two geodesic references where they must agree and
where they must not, the case a one-phase kernel would get wrong, and scene.watershed_gradient_table.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

from cl_volume_renderer_amd import scene
from tests import costpath_ref as cr
from tests import geodesic_ref as g
from tests import watershed_cases as wc
from tests import watershed_ref as w

NONE = w.NONE


# ---- the definition, literally: every simple path from every seed
def by_paths(cost, seeds, connectivity, plateau_cap, level_cap):
    """(labels, level) from the header's words: ML(p) over all simple paths (cutting a loop out never raises a state), the edges from
    ML, label(p) by reachability from each seed's voxel"""
    cost = np.asarray(cost)
    D = w.in_domain(cost)
    Z, Y, X = D.shape
    keys = g.seed_keys(D, seeds)
    dirs = [(dx, dy, dz) for dx, dy, dz, _ in g.steps(connectivity, None)]
    ML = {}

    def walk(p, state, seen):
        if state[0] > level_cap:
            return
        if state < ML.get(p, (1 << 20, 0)):
            ML[p] = state
        for dx, dy, dz in dirs:
            q = (p[0] + dx, p[1] + dy, p[2] + dz)
            if 0 <= q[0] < X and 0 <= q[1] < Y and 0 <= q[2] < Z and D[q[2], q[1], q[0]] and q not in seen:
                walk(q, w.step(state, int(cost[q[2], q[1], q[0]]), plateau_cap), seen | {q})

    for s in keys:
        walk(s, (0, 0), {s})
    edges = {p: [] for p in ML}
    for q in ML:
        for dx, dy, dz in dirs:
            p = (q[0] + dx, q[1] + dy, q[2] + dz)
            if p in ML and w.step(ML[q], int(cost[p[2], p[1], p[0]]), plateau_cap) == ML[p]:
                edges[q].append(p)
    labels = np.zeros((Z, Y, X), np.uint32)
    level = np.full((Z, Y, X), NONE, np.uint32)
    for p, (M, L) in ML.items():
        level[p[2], p[1], p[0]] = M << 16 | L
    for s, i in sorted(keys.items(), key=lambda kv: -kv[1]):  # descending: the smallest id is written last
        seen, stack = {s}, [s]
        while stack:
            q = stack.pop()
            labels[q[2], q[1], q[0]] = i
            for p in edges[q]:
                if p not in seen:
                    seen.add(p)
                    stack.append(p)
    return labels, level


@pytest.mark.parametrize("connectivity", (6, 26))
@pytest.mark.parametrize("plateau_cap", (0, 2, w.PLATEAU_MAX))
def test_reference_is_the_definition(connectivity, plateau_cap):
    rng = np.random.default_rng(100 + plateau_cap % 7 + connectivity)
    shapes = ((4, 3, 1), (3, 2, 2), (6, 2, 1), (12, 1, 1)) if connectivity == 6 else ((3, 3, 1), (2, 2, 2), (4, 2, 1), (9, 1, 1))
    for trial in range(24):  # at most 12 voxels: every simple path is walked
        X, Y, Z = shapes[trial % len(shapes)]
        cost = rng.integers(0, 4, (Z, Y, X)).astype(np.uint16)
        seeds = [(int(rng.integers(X)), int(rng.integers(Y)), int(rng.integers(Z)), int(i)) for i in (5, 2, 9)[: 2 + trial % 2]]
        level_cap = 2 if trial % 5 == 4 else w.LEVEL_MAX
        want = by_paths(cost, seeds, connectivity, plateau_cap, level_cap)
        got = w.watershed(cost, seeds, connectivity, plateau_cap, level_cap)
        assert np.array_equal(got[1], want[1]), (trial, cost, seeds)
        assert np.array_equal(got[0], want[0]), (trial, cost, seeds)


@pytest.mark.parametrize("connectivity", (6, 26))
def test_constant_cost_is_the_unit_geodesic(connectivity):
    k = wc.case("constant-plateau%d" % w.PLATEAU_MAX)
    labels, level = wc.expected(k["name"], connectivity)
    dist, geo_labels = g.geodesic(np.ones(k["cost"].shape, bool), k["seeds"], connectivity, g.UNIT)
    assert np.array_equal(labels, geo_labels)
    away = dist != 0
    c = int(k["cost"][0, 0, 0])
    assert np.array_equal(level[away], (c << 16 | (dist[away] - 1)).astype(np.uint32))
    assert (level[~away] == 0).all()


def test_the_ridge_holds_the_flood_and_not_the_sum():
    cost = wc.ridge()
    for connectivity in (6, 26):
        labels, level = wc.expected("ridge", connectivity)
        assert (labels[:, :, :wc.RIDGE_WALL_X] == 1).all() and (labels[:, :, wc.RIDGE_WALL_X + 1:] == 2).all()
        assert (level[:, :, wc.RIDGE_WALL_X] >> 16 == 20).all()
        _, summed = cr.cost_geodesic(cost, wc.RIDGE_SEEDS, connectivity)
        assert (summed[:, :, wc.RIDGE_WALL_X + 1:] == 1).sum() > 0  # the near seed's territory spills over the ridge


# ---- the one-phase kernel: a single key M << 48 | L << 32 | id relaxed to rest by Gauss-Seidel sweeps
def single_key_sweeps(k, connectivity, reverse):
    cost, cap = k["cost"], k["plateau_cap"]
    D = w.in_domain(cost, k["domain"])
    Z, Y, X = D.shape
    TOP = (1 << 20, 0, 0)
    key = {}
    cells = [(x, y, z) for z in range(Z) for y in range(Y) for x in range(X) if D[z, y, x]]
    for p in cells:
        key[p] = TOP
    for (x, y, z), i in g.seed_keys(D, k["seeds"], k["seed_labels"]).items():
        key[(x, y, z)] = (0, 0, i)
    dirs = [(dx, dy, dz) for dx, dy, dz, _ in g.steps(connectivity, None)]
    nbrs = {p: [q for q in ((p[0] + dx, p[1] + dy, p[2] + dz) for dx, dy, dz in dirs) if q in key] for p in cells}
    order = cells[::-1] if reverse else cells
    changed = True
    while changed:
        changed = False
        for p in order:
            c = int(cost[p[2], p[1], p[0]])
            best = key[p]
            for q in nbrs[p]:
                M, L, i = key[q]
                if M < (1 << 20):
                    t = w.step((M, L), c, cap) + (i,)
                    if t[0] <= k["level_cap"] and t < best:
                        best = t
            if best != key[p]:
                key[p] = best
                changed = True
    labels = np.zeros((Z, Y, X), np.uint32)
    level = np.full((Z, Y, X), NONE, np.uint32)
    for (x, y, z), (M, L, i) in key.items():
        if M < (1 << 20):
            labels[z, y, x], level[z, y, x] = i, M << 16 | L
    return labels, level


def test_a_single_key_depends_on_the_schedule_where_the_contract_does_not():
    """among the fields the GPU test runs there is one where the one-phase relaxation labels differently in raster and in reverse
    raster order; the levels of both sweeps are the reference's every time"""
    differing = 0
    for k in wc.cases():
        if not k["low"] or k["cost"].size > 3000:
            continue
        for connectivity in (6, 26):
            up, down = single_key_sweeps(k, connectivity, False), single_key_sweeps(k, connectivity, True)
            if not np.array_equal(up[0], down[0]):
                differing += 1
                want = wc.expected(k["name"], connectivity)[1]
                assert np.array_equal(up[1], want) and np.array_equal(down[1], want)
    assert differing >= 1


def test_level_cap_leaves_the_far_basin_unreached():
    labels, level = wc.expected("ridge-levelcap", 6)
    assert (labels[:, :, wc.RIDGE_WALL_X:] == 0).all() and (level[:, :, wc.RIDGE_WALL_X:] == NONE).all()
    assert (labels[:, :, :wc.RIDGE_WALL_X] == 1).all()
    assert w.result(level) == {"reached": 15 * wc.RIDGE_WALL_X, "max_level": 1}


def test_corridor_crosses_more_tile_faces_than_a_batch_has_rounds():
    labels, level = wc.expected("corridor", 6)
    reached = level != NONE
    assert reached.sum() == 17 * 33 + 16 and (labels[reached] == 3).all()
    assert int(level[reached].max()) == 3 << 16 | (17 * 33 + 16 - 2)


@pytest.mark.parametrize("g_max", (1, 255, 256, 4096, 65535 * 2))
def test_gradient_table(g_max):
    table, shift = scene.watershed_gradient_table(g_max)
    assert table.dtype == np.uint16
    assert (g_max * g_max >> shift) < 65536 and (shift == 0 or (g_max * g_max >> (shift - 1)) >= 65536)
    assert len(table) == (g_max * g_max >> shift) + 1
    assert table[0] == 1 and table.min() >= 1
    for i in sorted({0, 1, 2, 3, len(table) // 2, len(table) - 2, len(table) - 1} & set(range(len(table)))):
        assert int(table[i]) == 1 + min(65534, math.isqrt(i << shift))
    assert (np.diff(table.astype(np.int64)) >= 0).all()
    assert int(table[-1]) == 1 + min(65534, math.isqrt((g_max * g_max >> shift) << shift))


def test_gradient_table_rejects_what_it_cannot_hold():
    for bad in (0, -1, 65535 * 2 + 1):
        with pytest.raises(ValueError):
            scene.watershed_gradient_table(bad)


def test_no_kernel_uses_scratch_memory():
    """profiles/watershed_resource_usage.txt is the cross-compile's own report: every kernel of watershed_kernels.hip, no scratch"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "profiles", "watershed_resource_usage.txt")).read()
    source = open(os.path.join(root, "cl_volume_renderer_amd", "csrc", "watershed_kernels.hip")).read()
    kernels = set(re.findall(r"void (k_ws_\w+)\(", source))
    assert kernels == {"k_ws_init", "k_ws_seeds", "k_ws_level_round", "k_ws_label_round", "k_ws_finish"}
    blocks = text.split("Function Name: ")[1:]
    assert len(blocks) == 7 and all(any(k in b.splitlines()[0] for b in blocks) for k in kernels)  # the two round kernels twice
    for b in blocks:
        assert "ScratchSize [bytes/lane]: 0\n" in b and "VGPRs Spill: 0\n" in b and "SGPRs Spill: 0\n" in b, b.splitlines()[0]
