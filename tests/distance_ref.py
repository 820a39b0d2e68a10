"""clwh_mask_distance, clwh_mask_morph and clwh_mask_combine restated in numpy (include/clwh.h).  `brute` is the definition over all
pairs; `separable` is three 1-D lower-envelope passes (each the definition of a 1-D pass, min over i of f(i) + w (j - i)^2, as one
broadcast per line set).  Both are int64 throughout; "no site" is an int64 infinity until the end, where it becomes NONE.  Pure numpy."""
import functools

import numpy as np

NONE = 0xFFFFFFFF
INF = np.int64(1) << np.int64(62)
DILATE, ERODE, OPEN, CLOSE = 0, 1, 2, 3
AND, OR, XOR, ANDNOT, NOT = 0, 1, 2, 3, 4


def weights_ok(dims, w):
    """the contract's rule: no weight of 0 and wx (X - 1)^2 + wy (Y - 1)^2 + wz (Z - 1)^2 <= 2^32 - 2 (Python integers)"""
    return all(int(v) >= 1 for v in w) and sum(int(v) * (int(n) - 1) ** 2 for v, n in zip(w, dims)) <= 2 ** 32 - 2


def _finish(d):
    return np.where(d >= INF, NONE, d).astype(np.uint32)


def brute(sites, w):
    """uint32 [z][y][x]: min over the sites q of wx dx^2 + wy dy^2 + wz dz^2, NONE without a site.  sites: bool [z][y][x]; w = (wx, wy, wz)"""
    sites = np.asarray(sites, bool)
    Z, Y, X = sites.shape
    assert weights_ok((X, Y, Z), w)
    wx, wy, wz = (np.int64(v) for v in w)
    qz, qy, qx = (c.astype(np.int64) for c in np.nonzero(sites))
    best = np.full(sites.shape, INF, np.int64)
    z, y, x = (c.astype(np.int64) for c in np.indices(sites.shape))
    for k in range(len(qx)):
        np.minimum(best, wx * (x - qx[k]) ** 2 + wy * (y - qy[k]) ** 2 + wz * (z - qz[k]) ** 2, out=best)
    return _finish(best)


def _envelope(f, w, axis):
    """out(j) = min over i of f(i) + w (j - i)^2 along `axis`; f int64 with INF for "nothing" (INF + w d^2 stays far above any value)"""
    f = np.ascontiguousarray(np.moveaxis(f, axis, -1))  # (contiguous: the reshapes below are views)
    n = f.shape[-1]
    i = np.arange(n, dtype=np.int64)
    cost = np.int64(w) * (i[:, None] - i[None, :]) ** 2  # [j][i]
    out = np.empty_like(f)
    lines = f.reshape(-1, n)
    flat = out.reshape(-1, n)
    step = max(1, (1 << 22) // (n * n))
    for a in range(0, len(lines), step):
        flat[a:a + step] = (lines[a:a + step, None, :] + cost[None]).min(axis=2)
    return np.moveaxis(np.minimum(out, INF), -1, axis)


def separable(sites, w):
    """the same map by a pass along x, then y, then z"""
    sites = np.asarray(sites, bool)
    Z, Y, X = sites.shape
    assert weights_ok((X, Y, Z), w)
    d = np.where(sites, np.int64(0), INF)
    for axis, wq in ((2, w[0]), (1, w[1]), (0, w[2])):
        d = _envelope(d, wq, axis)
    return _finish(d)


def distance(mask, w, to_clear=False, cap=None):
    """clwh_mask_distance's output: D to the set (or, to_clear, to the clear) voxels, NONE above cap"""
    mask = np.asarray(mask, bool)
    d = separable(~mask if to_clear else mask, w)
    if cap is not None and int(cap) != NONE:
        d = np.where(d <= np.uint32(cap), d, np.uint32(NONE)).astype(np.uint32)
    return d


def _dilate(mask, w, radius_sq):
    d = separable(mask, w)
    return (d != NONE) & (d.astype(np.int64) <= int(radius_sq))


def _erode(mask, w, radius_sq):
    d = separable(~mask, w)
    return mask & ((d == NONE) | (d.astype(np.int64) > int(radius_sq)))


def morph(mask, w, op, radius_sq):
    """clwh_mask_morph's set as bool [z][y][x]; NONE counts as farther than any radius_sq"""
    mask = np.asarray(mask, bool)
    if op == DILATE:
        return _dilate(mask, w, radius_sq)
    if op == ERODE:
        return _erode(mask, w, radius_sq)
    if op == OPEN:
        return _dilate(_erode(mask, w, radius_sq), w, radius_sq)
    assert op == CLOSE
    return _erode(_dilate(mask, w, radius_sq), w, radius_sq)


def combine(a, b, op):
    """clwh_mask_combine's set as bool [z][y][x]; b is not looked at for NOT"""
    a = np.asarray(a, bool)
    if op == NOT:
        return ~a
    b = np.asarray(b, bool)
    return {AND: a & b, OR: a | b, XOR: a ^ b, ANDNOT: a & ~b}[op]


# ---- the cases the CPU and GPU tests share
CPU_CASES = (((65, 17, 17), (1, 1, 1)), ((33, 20, 9), (49, 49, 625)), ((7, 5, 130), (4, 9, 1)), ((1, 1, 1), (1, 1, 1)), ((70, 40, 36), (1, 1, 1)))


@functools.lru_cache(maxsize=None)
def random_mask(dims, density, seed):
    """bool [z][y][x], read only; at least one voxel set"""
    X, Y, Z = dims
    m = np.random.default_rng(seed).random((Z, Y, X)) < density
    if not m.any():
        m[Z // 2, Y // 2, X // 3] = True
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def random_distance(dims, density, seed, w, to_clear):
    d = distance(random_mask(dims, density, seed), w, to_clear)
    d.setflags(write=False)
    return d
