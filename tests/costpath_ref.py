"""clwh_cost_geodesic, clwh_cost_trace and clwh_cost_from_field restated in Python / numpy (include/clwh.h), and Context.centerline's
composition over tests/distance_ref.py.  The map is tests/geodesic_ref.py's Dijkstra over a heap of (dist, id, voxel) with the cost of
the voxel ENTERED: the step from q to p costs mult(direction) * cost(p).  Also the inputs the CPU and the GPU tests share."""
import functools
import heapq
import math

import numpy as np

from cl_volume_renderer_amd import scene
from tests import distance_ref as dr
from tests import geodesic_ref as g
from tests import grow_ref as gr

NONE = g.NONE
CAP_MAX = 0xFF000000
SRC_U32, SRC_VALUE, SRC_GRADIENT = 0, 1, 2
UNIT, CHAMFER = g.UNIT, g.CHAMFER
ANISO = g.ANISO
LARGEST = ((255, 255, 255), (255, 255, 255), 255)


def steps(connectivity, multipliers):
    """[(dx, dy, dz, multiplier)] in the trace's order; every multiplier in use within 1 .. 255"""
    out = g.steps(connectivity, multipliers)
    assert all(1 <= m <= 255 for _, _, _, m in out)
    return out


def in_domain(cost, domain=None):
    cost = np.asarray(cost)
    return (cost != 0) if domain is None else ((cost != 0) & np.asarray(domain, bool))


def cost_geodesic(cost, seeds=None, connectivity=6, multipliers=None, cap=None, seed_labels=None, domain=None):
    """(dist, labels), uint32 [z][y][x] each: NONE and 0 outside D and where no seed reaches within the cap"""
    cost = np.asarray(cost, np.uint16)
    D = in_domain(cost, domain)
    Z, Y, X = D.shape
    cap = CAP_MAX if cap is None or int(cap) == NONE else int(cap)
    assert 0 <= cap <= CAP_MAX
    sy, sz = X + 2, (X + 2) * (Y + 2)
    padded = np.zeros((Z + 2, Y + 2, X + 2), np.int64)
    padded[1:-1, 1:-1, 1:-1] = np.where(D, cost, 0)
    entry = padded.reshape(-1).tolist()  # the cost of entering a voxel; 0: not in D
    offs = [(dx + dy * sy + dz * sz, m) for dx, dy, dz, m in steps(connectivity, multipliers)]
    best = {}
    heap = []
    for (x, y, z), i in g.seed_keys(D, seeds, seed_labels).items():
        p = (x + 1) + (y + 1) * sy + (z + 1) * sz
        best[p] = (0, i)
        heap.append((0, i, p))
    heapq.heapify(heap)
    while heap:
        d, i, p = heapq.heappop(heap)
        if best[p] != (d, i):
            continue
        for o, m in offs:
            q = p + o
            c = entry[q]
            if c:
                dq = d + m * c
                if dq <= cap and (dq, i) < best.get(q, (NONE, 0)):
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


def trace(cost, dist, target, connectivity=6, multipliers=None, labels=None):
    """(points [(x, y, z)], complete): the header's walk from the target; complete is False where the cost is 0 or no direction
    qualifies at a point with dist > 0"""
    Z, Y, X = dist.shape
    x, y, z = (int(v) for v in target)
    if int(dist[z, y, x]) == NONE:
        return [], True
    order = steps(connectivity, multipliers)
    points = [(x, y, z)]
    while int(dist[z, y, x]) != 0:
        here, c = int(dist[z, y, x]), int(cost[z, y, x])
        for dx, dy, dz, m in order:
            px, py, pz = x + dx, y + dy, z + dz
            if c == 0 or not (0 <= px < X and 0 <= py < Y and 0 <= pz < Z) or int(dist[pz, py, px]) == NONE:
                continue
            if int(dist[pz, py, px]) + m * c != here or (labels is not None and labels[pz, py, px] != labels[z, y, x]):
                continue
            x, y, z = px, py, pz
            points.append((x, y, z))
            break
        else:
            return points, False
    return points, True


def path_cost(cost, points, connectivity=6, multipliers=None):
    """the length of the forward path behind a traced one (target first): every point but the last, the seed, was entered"""
    mult = {(dx, dy, dz): m for dx, dy, dz, m in steps(connectivity, multipliers)}
    return sum(mult[tuple(b[k] - a[k] for k in range(3))] * int(cost[a[2], a[1], a[0]]) for a, b in zip(points[:-1], points[1:]))


def field_values(source, kind):
    """s(p) of clwh_cost_from_field as int64 [z][y][x]"""
    if kind == SRC_U32:
        return np.asarray(source, np.uint32).astype(np.int64)
    v = np.asarray(source, np.int16).astype(np.int64)
    if kind == SRC_VALUE:
        return v
    assert kind == SRC_GRADIENT
    s = np.zeros(v.shape, np.int64)
    for axis in range(3):
        i = np.arange(v.shape[axis])
        d = np.take(v, np.minimum(i + 1, len(i) - 1), axis) - np.take(v, np.maximum(i - 1, 0), axis)
        s += d * d
    return s


def cost_from_field(source, table, lo=0, shift=0, kind=SRC_U32, domain=None):
    """uint16 [z][y][x]: table[clamp((s - lo) >> shift, 0, n - 1)] in Python integers, 0 outside the domain"""
    table = np.asarray(table, np.uint16).reshape(-1)
    n, lo, shift = len(table), int(lo), int(shift)
    assert 1 <= n <= 65536 and 0 <= shift <= 40 and -2 ** 63 <= lo < 2 ** 63
    s = field_values(source, kind)
    index = np.array([min(max(v - lo, 0) >> shift, n - 1) for v in s.reshape(-1).tolist()], np.int64).reshape(s.shape)
    out = table[index]
    return out if domain is None else np.where(np.asarray(domain, bool), out, np.uint16(0)).astype(np.uint16)


def centerline(mask, start, end, spacing=(1, 1, 1), connectivity=26, max_radius=None, sharpness=100):
    """Context.centerline on the references: (points, cost, depth)"""
    mask = np.asarray(mask, bool)
    multipliers = scene.geodesic_weights(spacing, 10)
    depth = dr.distance(mask, scene.mask_weights(spacing), to_clear=True)
    inside = mask & (depth != NONE)
    r_sq_max = scene.radius_sq(max_radius) if max_radius is not None else int(depth[inside].max()) if inside.any() else 1
    shift = scene.centerline_shift(r_sq_max)
    table = scene.centerline_cost_table(max(r_sq_max, 1) >> shift, sharpness)
    cost = cost_from_field(depth, table, 0, shift, SRC_U32, mask)
    dist, _ = cost_geodesic(cost, [tuple(int(v) for v in start) + (1,)], connectivity, multipliers)
    points, complete = trace(cost, dist, end, connectivity, multipliers)
    assert complete
    return points, cost, depth


# ---- the inputs the tests share
SHAPES = ((1, 1, 1), (17, 17, 9), (33, 18, 10), (70, 9, 5))  # X, Y, Z: one face crossed per axis; ragged; the domain's word boundary


def random_cost(dims, seed=3, walls=0.1):
    """uint16 [z][y][x]: uniform in 1 .. 65535, a tenth of the voxels 0"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 65536, (Z, Y, X)).astype(np.uint16)
    c[rng.random((Z, Y, X)) < walls] = 0
    return c


def random_seeds(D, seed=5, n=4):
    """up to n labelled seeds inside D (ids 3, 5, ...), the first listed again with a larger id and the second with a smaller one, and,
    if there is one, a voxel outside D with id 1"""
    rng = np.random.default_rng(seed)
    inside, outside = np.argwhere(D), np.argwhere(~D)
    pick = inside[rng.choice(len(inside), min(n, len(inside)), replace=False)] if len(inside) else []
    rows = [(int(x), int(y), int(z), 3 + 2 * k) for k, (z, y, x) in enumerate(pick)]
    if rows:
        rows += [rows[0][:3] + (40,), rows[-1][:3] + (2,)]
    if len(outside):
        z, y, x = outside[rng.integers(len(outside))]
        rows.append((int(x), int(y), int(z), 1))
    if not rows:
        rows = [(0, 0, 0, 1)]
    return rows


@functools.lru_cache(maxsize=None)
def random_case(dims, connectivity, multipliers=CHAMFER, cap=None, with_domain=False):
    """(cost, domain or None, seeds, dist, labels), read only"""
    cost = random_cost(dims)
    domain = None
    if with_domain:
        X, Y, Z = dims
        domain = np.random.default_rng(9).random((Z, Y, X)) < 0.8
    seeds = random_seeds(in_domain(cost, domain))
    dist, labels = cost_geodesic(cost, seeds, connectivity, multipliers, cap, None, domain)
    for a in (cost, dist, labels) + ((domain,) if domain is not None else ()):
        a.setflags(write=False)
    return cost, domain, seeds, dist, labels


HIGHWAY_SEED = (2, 2, 3, 7)


def highway():
    """66 x 36 x 8 = 5 x 3 x 1 tiles: a field of cost 1000 with a corridor of cost 1 in the plane z = 3, rows y = 2, 10, 18, 26, 34 from
    x = 2 to 63 joined at alternating ends: a serpentine across every tile, 20 tile faces long.  From the seed at the corridor's start
    the field's direct route reaches the tiles below in three rounds; the corridor's cheap detour lowers them many rounds later."""
    c = np.full((8, 36, 66), 1000, np.uint16)
    rows = (2, 10, 18, 26, 34)
    for k, y in enumerate(rows):
        c[3, y, 2:64] = 1
        if k + 1 < len(rows):
            c[3, y:rows[k + 1], 63 if k % 2 == 0 else 2] = 1
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def highway_case(connectivity):
    cost = highway()
    dist, labels = cost_geodesic(cost, [HIGHWAY_SEED], connectivity, CHAMFER)
    for a in (dist, labels):
        a.setflags(write=False)
    return cost, dist, labels


@functools.lru_cache(maxsize=None)
def serpentine_case(connectivity):
    """grow's serpentine as the domain, random costs without walls over the whole box: one path of 2739 voxels whose length stays
    below the cap (about 2738 * 10 * 32768 = 9e8)"""
    domain = gr.serpentine() == 100
    Z, Y, X = domain.shape
    cost = random_cost((X, Y, Z), 21, 0.0)
    dist, labels = cost_geodesic(cost, [(0, 0, 1, 7)], connectivity, CHAMFER, None, None, domain)
    for a in (domain, cost, dist, labels):
        a.setflags(write=False)
    return cost, domain, dist, labels


# ---- the tube: a torus with a sector removed, radius 4 about an axis circle of radius 15
TUBE_CENTRE, TUBE_AXIS_RADIUS, TUBE_Z, TUBE_RADIUS, TUBE_GAP = 21.5, 15.0, 6.5, 4.0, 0.4


def off_axis(points):
    """the distance of each (x, y, z) from the tube's axis circle"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    rho = np.hypot(p[:, 0] - TUBE_CENTRE, p[:, 1] - TUBE_CENTRE)
    return np.hypot(rho - TUBE_AXIS_RADIUS, p[:, 2] - TUBE_Z)


@functools.lru_cache(maxsize=None)
def tube():
    """(mask bool [14][44][44], start, end): the clicks are the mask's voxels nearest the axis circle's two ends"""
    z, y, x = np.indices((14, 44, 44))
    rho = np.hypot(x - TUBE_CENTRE, y - TUBE_CENTRE)
    angle = np.arctan2(y - TUBE_CENTRE, x - TUBE_CENTRE)
    mask = ((rho - TUBE_AXIS_RADIUS) ** 2 + (z - TUBE_Z) ** 2 <= TUBE_RADIUS ** 2) & (np.abs(angle) >= TUBE_GAP)
    voxels = np.argwhere(mask)[:, ::-1]
    clicks = []
    for end in (TUBE_GAP, -TUBE_GAP):
        tip = (TUBE_CENTRE + TUBE_AXIS_RADIUS * math.cos(end), TUBE_CENTRE + TUBE_AXIS_RADIUS * math.sin(end), TUBE_Z)
        clicks.append(tuple(int(v) for v in voxels[np.argmin(((voxels - tip) ** 2).sum(axis=1))]))
    mask.setflags(write=False)
    return mask, clicks[0], clicks[1]


@functools.lru_cache(maxsize=None)
def tube_paths():
    """(the centreline's points, the plain shortest path's points) between the tube's clicks, 26 neighbours, chamfer 10 / 14 / 17"""
    mask, start, end = tube()
    centre = centerline(mask, start, end)[0]
    dist, _ = g.geodesic(mask, [start + (1,)], 26, CHAMFER)
    plain, complete = g.trace(dist, end, 26, CHAMFER)
    assert complete
    return centre, plain
