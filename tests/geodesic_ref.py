"""clwh_mask_geodesic and clwh_geodesic_trace restated in Python / numpy (include/clwh.h): Dijkstra over a heap of (dist, id, voxel)
popped in lexicographic order, so that a voxel is settled with the smallest distance and, among the seeds that attain it, the smallest
id; the cap, the seed rules and the trace rule as the header states them.  The voxel is its flat index in an array padded by one
voxel, so nothing clamps or wraps.  Also the inputs the CPU and the GPU tests share."""
import functools
import heapq
import itertools

import numpy as np

from tests import grow_ref as gr

NONE = 0xFFFFFFFF
CAP_MAX = 0xFFFF0000
UNIT = ((1, 1, 1), (1, 1, 1), 1)
ANISO = ((7, 7, 25), (26, 26, 10), 27)  # voxels of 0.7 x 0.7 x 2.5: scene.geodesic_weights((0.7, 0.7, 2.5), 10)
CHAMFER = ((10, 10, 10), (14, 14, 14), 17)  # scene.geodesic_weights((1, 1, 1), 10)


def normalise(weights):
    """None, (fx, fy, fz) or (face, edge, corner) -> (face, edge, corner)"""
    if weights is None:
        return UNIT
    if len(weights) == 3 and np.ndim(weights[0]) == 1:
        return tuple(int(v) for v in weights[0]), tuple(int(v) for v in weights[1]), int(weights[2])
    return tuple(int(v) for v in weights), (1, 1, 1), 1


def steps(connectivity, weights):
    """[(dx, dy, dz, cost)] in the trace's order: (dz, dy, dx) ascending with dx fastest, the non-neighbours left out"""
    face, edge, corner = normalise(weights)
    assert connectivity in (6, 26)
    out = []
    for dz, dy, dx in itertools.product((-1, 0, 1), repeat=3):
        moved = [dx != 0, dy != 0, dz != 0]
        if sum(moved) == 0 or (connectivity == 6 and sum(moved) != 1):
            continue
        w = face[moved.index(True)] if sum(moved) == 1 else edge[moved.index(False)] if sum(moved) == 2 else corner
        assert 1 <= w <= 65535
        out.append((dx, dy, dz, w))
    return out


def seed_keys(domain, seeds=None, seed_labels=None):
    """{(x, y, z): smallest id} of the seeds that count: inside D, listed or from the labels"""
    Z, Y, X = domain.shape
    keys = {}
    for x, y, z, i in (np.asarray(seeds, dtype=np.int64).reshape(-1, 4) if seeds is not None else ()):
        assert 0 <= x < X and 0 <= y < Y and 0 <= z < Z and 1 <= i <= NONE
        if domain[z, y, x]:
            keys[(x, y, z)] = min(int(i), keys.get((x, y, z), NONE))
    if seed_labels is not None:
        for z, y, x in np.argwhere(domain & (seed_labels != 0)):
            keys[(x, y, z)] = min(int(seed_labels[z, y, x]), keys.get((x, y, z), NONE))
    return keys


def geodesic(domain, seeds=None, connectivity=6, weights=None, cap=None, seed_labels=None):
    """(dist, labels), uint32 [z][y][x] each: NONE and 0 outside D and where no seed reaches within the cap"""
    domain = np.asarray(domain, bool)
    Z, Y, X = domain.shape
    cap = CAP_MAX if cap is None or int(cap) == NONE else int(cap)
    assert 0 <= cap <= CAP_MAX
    sy, sz = X + 2, (X + 2) * (Y + 2)
    inside = np.zeros((Z + 2, Y + 2, X + 2), bool)
    inside[1:-1, 1:-1, 1:-1] = domain
    inside = inside.reshape(-1).tolist()
    offs = [(dx + dy * sy + dz * sz, w) for dx, dy, dz, w in steps(connectivity, weights)]
    best = {}
    heap = []
    for (x, y, z), i in seed_keys(domain, seeds, seed_labels).items():
        p = (x + 1) + (y + 1) * sy + (z + 1) * sz
        best[p] = (0, i)
        heap.append((0, i, p))
    heapq.heapify(heap)
    while heap:
        d, i, p = heapq.heappop(heap)
        if best[p] != (d, i):
            continue
        for o, w in offs:
            q, dq = p + o, d + w
            if inside[q] and dq <= cap and (dq, i) < best.get(q, (NONE, 0)):
                best[q] = (dq, i)
                heapq.heappush(heap, (dq, i, q))
    dist = np.full((Z + 2) * (Y + 2) * (X + 2), NONE, np.uint32)
    labels = np.zeros_like(dist)
    if best:
        at = np.fromiter(best.keys(), np.int64, len(best))
        dist[at] = np.fromiter((v[0] for v in best.values()), np.uint32, len(best))
        labels[at] = np.fromiter((v[1] for v in best.values()), np.uint32, len(best))
    cut = (slice(1, -1),) * 3
    return dist.reshape(Z + 2, Y + 2, X + 2)[cut].copy(), labels.reshape(Z + 2, Y + 2, X + 2)[cut].copy()


def result(dist):
    """clwh_geodesic_result's contract fields as ffi.GeodesicResult.as_dict gives them"""
    reached = dist != NONE
    return {"reached": int(reached.sum()), "max_dist": int(dist[reached].max()) if reached.any() else 0}


def trace(dist, target, connectivity=6, weights=None, labels=None):
    """(points [(x, y, z)], complete): the header's walk from the target; complete is False where no direction qualifies"""
    Z, Y, X = dist.shape
    x, y, z = (int(v) for v in target)
    if int(dist[z, y, x]) == NONE:
        return [], True
    order = steps(connectivity, weights)
    points = [(x, y, z)]
    while int(dist[z, y, x]) != 0:
        for dx, dy, dz, w in order:
            px, py, pz = x + dx, y + dy, z + dz
            if not (0 <= px < X and 0 <= py < Y and 0 <= pz < Z) or int(dist[pz, py, px]) == NONE:
                continue
            if int(dist[pz, py, px]) + w != int(dist[z, y, x]) or (labels is not None and labels[pz, py, px] != labels[z, y, x]):
                continue
            x, y, z = px, py, pz
            points.append((x, y, z))
            break
        else:
            return points, False
    return points, True


def path_cost(points, connectivity=6, weights=None):
    cost = {(dx, dy, dz): w for dx, dy, dz, w in steps(connectivity, weights)}
    return sum(cost[tuple(b[k] - a[k] for k in range(3))] for b, a in zip(points[1:], points[:-1]))


def ties(domain, seeds, connectivity=6, weights=None):
    """bool [z][y][x]: the voxels where two seeds of different ids are equally near (and nearest)"""
    ids = sorted({int(s[3]) for s in seeds})
    dist, _ = geodesic(domain, seeds, connectivity, weights)
    count = np.zeros(domain.shape, np.int32)
    for i in ids:
        di, _ = geodesic(domain, [s for s in seeds if int(s[3]) == i], connectivity, weights)
        count += (di == dist) & (dist != NONE)
    return count >= 2


# ---- the inputs the tests share
def random_seeds(domain, seed, n=6):
    """n labelled seeds inside D (ids 3, 5, 7, ... in random order), one of them listed again with a larger and a smaller id, and one
    voxel outside D with id 1: rows of (x, y, z, id)"""
    rng = np.random.default_rng(seed)
    inside, outside = np.argwhere(domain), np.argwhere(~domain)
    rows = [(int(x), int(y), int(z), 3 + 2 * k) for k, (z, y, x) in enumerate(inside[rng.choice(len(inside), n, replace=False)])]
    rows += [rows[0][:3] + (40,), rows[1][:3] + (2,)]
    z, y, x = outside[rng.integers(len(outside))]
    rows.append((int(x), int(y), int(z), 1))
    return rows


@functools.lru_cache(maxsize=None)
def random_domain(dims, connectivity):
    """grow's percolation window of grow's random volume: bool [z][y][x], read only"""
    lo, hi = gr.WINDOWS[connectivity]
    d = gr.admissible(gr.random_volume(dims, 11), lo, hi)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def random_case(dims, connectivity, weights, cap):
    """(domain, seeds, dist, labels) of a random domain, read only"""
    domain = random_domain(dims, connectivity)
    seeds = random_seeds(domain, 5)
    dist, labels = geodesic(domain, seeds, connectivity, weights, cap)
    for a in (dist, labels):
        a.setflags(write=False)
    return domain, seeds, dist, labels


def two_balls():
    """72 x 24 x 24: two balls of radius 9 centred at (56, 12, 12) and (70, 12, 12), straddling the word boundary at x = 64, the second
    cut by the border; they overlap: one component"""
    z, y, x = np.indices((24, 24, 72))
    return ((x - 56) ** 2 + (y - 12) ** 2 + (z - 12) ** 2 <= 81) | ((x - 70) ** 2 + (y - 12) ** 2 + (z - 12) ** 2 <= 81)


TWO_BALLS_RADIUS_SQ = 36


@functools.lru_cache(maxsize=None)
def two_balls_split():
    """the split workflow on the references: (mask, ranks of the eroded pieces, labels of the territories, number of parts)"""
    from tests import distance_ref as dr
    from tests import label_ref as lr

    mask = two_balls()
    eroded = dr.morph(mask, (1, 1, 1), dr.ERODE, TWO_BALLS_RADIUS_SQ)
    ranks, _, info = lr.label_admissible(eroded, 6)
    _, labels = geodesic(mask, None, 6, None, None, seed_labels=ranks)
    for a in (mask, ranks, labels):
        a.setflags(write=False)
    return mask, ranks, labels, int(info["n_components"])
