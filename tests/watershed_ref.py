"""clwh_watershed restated in Python / numpy (include/clwh.h).  Stage 1 is Dijkstra over a heap of ((M, L), voxel): the step never
lowers a state and is monotone in it, so a voxel popped first holds the smallest state of any path.  Stage 2 is a min-propagation of
the seeds' ids over the edges q -> p with step(ML(q), cost(p)) == ML(p), run from a worklist until nothing falls any more.  The voxel
is its flat index in an array padded by one voxel, so nothing clamps or wraps."""
import heapq
from collections import deque

import numpy as np

from tests import geodesic_ref as g

NONE = g.NONE
PLATEAU_MAX, LEVEL_MAX = 65534, 65535


def in_domain(cost, domain=None):
    cost = np.asarray(cost)
    return (cost != 0) if domain is None else ((cost != 0) & np.asarray(domain, bool))


def step(state, c, plateau_cap):
    """the state one step into a voxel of cost c behind `state` = (M, L)"""
    M, L = state
    return (c, 0) if c > M else (M, min(L + 1, plateau_cap))


def offsets(connectivity, sy, sz):
    return [dx + dy * sy + dz * sz for dx, dy, dz, _ in g.steps(connectivity, None)]


def levels(cost, seed_keys, connectivity=6, plateau_cap=PLATEAU_MAX, level_cap=LEVEL_MAX, domain=None):
    """stage 1: {padded flat index: (M, L)} of the reached voxels, and what stage 2 needs"""
    cost = np.asarray(cost, np.uint16)
    D = in_domain(cost, domain)
    Z, Y, X = D.shape
    assert 0 <= plateau_cap <= PLATEAU_MAX and 0 <= level_cap <= LEVEL_MAX
    sy, sz = X + 2, (X + 2) * (Y + 2)
    padded = np.zeros((Z + 2, Y + 2, X + 2), np.int64)
    padded[1:-1, 1:-1, 1:-1] = np.where(D, cost, 0)
    entry = padded.reshape(-1).tolist()  # the cost of entering a voxel; 0: not in D
    offs = offsets(connectivity, sy, sz)
    best, heap = {}, []
    for (x, y, z) in seed_keys:
        p = (x + 1) + (y + 1) * sy + (z + 1) * sz
        best[p] = (0, 0)
        heap.append(((0, 0), p))
    heapq.heapify(heap)
    while heap:
        s, p = heapq.heappop(heap)
        if best[p] != s:
            continue
        for o in offs:
            q = p + o
            c = entry[q]
            if c:
                t = step(s, c, plateau_cap)
                if t[0] <= level_cap and t < best.get(q, (LEVEL_MAX + 1, 0)):
                    best[q] = t
                    heapq.heappush(heap, (t, q))
    return best, entry, offs, (sy, sz)


def watershed(cost, seeds=None, connectivity=6, plateau_cap=PLATEAU_MAX, level_cap=LEVEL_MAX, seed_labels=None, domain=None):
    """(labels, level), uint32 [z][y][x] each: 0 and NONE outside D and where no seed reaches within the level cap"""
    cost = np.asarray(cost, np.uint16)
    D = in_domain(cost, domain)
    Z, Y, X = D.shape
    keys = g.seed_keys(D, seeds, seed_labels)
    best, entry, offs, (sy, sz) = levels(cost, keys, connectivity, plateau_cap, level_cap, domain)
    # stage 2: the smallest id that reaches a voxel along the edges; the seeds in ascending order, so most voxels fall once
    label = {}
    for (x, y, z), i in sorted(keys.items(), key=lambda kv: kv[1]):
        s = (x + 1) + (y + 1) * sy + (z + 1) * sz
        if label.get(s, NONE + 1) <= i:
            continue  # (cannot happen: no edge enters a seed's voxel)
        label[s] = i
        work = deque([s])
        while work:
            q = work.popleft()
            lq, sq = label[q], best[q]
            for o in offs:
                p = q + o
                sp = best.get(p)
                if sp is not None and sp != (0, 0) and step(sq, entry[p], plateau_cap) == sp and lq < label.get(p, NONE + 1):
                    label[p] = lq
                    work.append(p)
    assert label.keys() == best.keys()  # every reached voxel has a seed
    n = (Z + 2) * (Y + 2) * (X + 2)
    level = np.full(n, NONE, np.uint32)
    labels = np.zeros(n, np.uint32)
    if best:
        at = np.fromiter(best.keys(), np.int64, len(best))
        level[at] = np.fromiter((M << 16 | L for M, L in best.values()), np.uint32, len(best))
        labels[at] = np.fromiter((label[p] for p in best.keys()), np.uint32, len(best))
    cut = (slice(1, -1),) * 3
    return labels.reshape(Z + 2, Y + 2, X + 2)[cut].copy(), level.reshape(Z + 2, Y + 2, X + 2)[cut].copy()


def result(level):
    """clwh_watershed_result's contract fields as ffi.WatershedResult.as_dict gives them"""
    reached = level != NONE
    return {"reached": int(reached.sum()), "max_level": int(level[reached].max() >> 16) if reached.any() else 0}
