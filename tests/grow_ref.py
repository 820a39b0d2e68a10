"""clwh_segment_grow and clwh_volume_apply_mask restated in numpy (include/clwh.h): the admissible image, neighbours by flat offsets
in an array padded by one voxel (so nothing clamps or wraps), growth as a frontier search over flat indices, the packed mask, the
statistics in Python integers.  The search costs in proportion to the component, not to depth x volume.  Pure numpy."""
import functools
import itertools

import numpy as np

from cl_volume_renderer_amd import scene


def box_of(dims, box=None):
    """((lo), (hi)) in voxels, hi exclusive; box None or hi all zero: the whole volume"""
    if box is None:
        return (0, 0, 0), tuple(dims)
    lo, hi = tuple(int(v) for v in box[0]), tuple(int(v) for v in box[1])
    return lo, (hi if any(hi) else tuple(dims))


def admissible(vol, lo, hi, box=None):
    """bool [z][y][x]: lo <= V <= hi and inside the box"""
    Z, Y, X = vol.shape
    blo, bhi = box_of((X, Y, Z), box)
    assert all(0 <= a <= b <= d for a, b, d in zip(blo, bhi, (X, Y, Z)))
    a = (vol >= lo) & (vol <= hi)
    inside = np.zeros_like(a)
    inside[blo[2]:bhi[2], blo[1]:bhi[1], blo[0]:bhi[0]] = True
    return a & inside


def offsets(connectivity):
    """(dx, dy, dz) of a voxel's neighbours"""
    assert connectivity in (6, 26)
    out = [d for d in itertools.product((-1, 0, 1), repeat=3) if any(d)]
    return [d for d in out if connectivity == 26 or sum(map(abs, d)) == 1]


def _padded(a, fill):
    p = np.full(tuple(n + 2 for n in a.shape), fill, a.dtype)
    p[1:-1, 1:-1, 1:-1] = a
    return p


def grow_admissible(adm, start, connectivity=6):
    """the smallest superset of start & adm closed under "an admissible neighbour of a member is a member": (bool [z][y][x], layers),
    layers = the geodesic depth (the number of frontier steps that found something)"""
    Z, Y, X = adm.shape
    ap = _padded(adm, False).reshape(-1)
    sy, sz = X + 2, (X + 2) * (Y + 2)
    offs = [dx + dy * sy + dz * sz for dx, dy, dz in offsets(connectivity)]
    reached = np.zeros_like(ap)
    frontier = np.flatnonzero(_padded(start & adm, False).reshape(-1))
    reached[frontier] = True
    layers = 0
    while len(frontier):
        found = []
        for o in offs:
            n = frontier + o
            n = n[ap[n] & ~reached[n]]
            reached[n] = True  # (a voxel found twice under one offset is the same voxel; under two offsets the second finds it reached)
            found.append(n)
        frontier = np.unique(np.concatenate(found))
        layers += len(frontier) > 0
    return reached.reshape(Z + 2, Y + 2, X + 2)[1:-1, 1:-1, 1:-1].copy(), layers


def seeds_image(shape, seeds):
    s = np.zeros(shape, bool)
    for x, y, z in np.asarray(seeds, dtype=np.int64).reshape(-1, 3):
        assert 0 <= x < shape[2] and 0 <= y < shape[1] and 0 <= z < shape[0]
        s[z, y, x] = True
    return s


def grow(vol, seeds, lo, hi, connectivity=6, box=None, from_mask=None):
    """the contract's R as bool [z][y][x], and the geodesic depth.  from_mask: the bool image CLWH_GROW_FROM_MASK finds in `mask`"""
    start = seeds_image(vol.shape, seeds if seeds is not None else [])
    if from_mask is not None:
        start |= from_mask
    return grow_admissible(admissible(vol, lo, hi, box), start, connectivity)


def stats(vol, region):
    """clwh_grow_result's contract fields as ffi.GrowResult.as_dict gives them"""
    z, y, x = np.nonzero(region)
    if len(x) == 0:
        return {"count": 0, "bbox_lo": (0, 0, 0), "bbox_hi": (0, 0, 0), "sum": 0, "sum_sq": 0, "vmin": 0, "vmax": 0}
    v = vol[region].astype(np.int64)
    return {"count": len(x), "bbox_lo": (int(x.min()), int(y.min()), int(z.min())), "bbox_hi": (int(x.max()) + 1, int(y.max()) + 1, int(z.max()) + 1),
            "sum": int(v.sum()), "sum_sq": int((v * v).sum()), "vmin": int(v.min()), "vmax": int(v.max())}


def packed(region):
    """the mask's words, padding included"""
    return scene.mask_pack(region)


def apply_mask(vol, region, fill=-32768, invert=False):
    return np.where(region != invert, vol, np.int16(fill)).astype(np.int16)


def labels(adm, connectivity=6):
    """int64 [z][y][x]: the smallest flat index (z, y, x order) of the voxel's component, -1 outside adm.  Minimum propagation over the
    neighbours with pointer jumping (a label is the index of a voxel of the same component whose label is no larger): for choosing
    test inputs, not part of the contract"""
    Z, Y, X = adm.shape
    big = np.int64(adm.size)
    lab = np.where(adm, np.arange(adm.size, dtype=np.int64).reshape(adm.shape), big)
    offs = offsets(connectivity)
    while True:
        p = _padded(lab, big)
        m = lab.copy()
        for dx, dy, dz in offs:
            np.minimum(m, p[1 + dz:Z + 1 + dz, 1 + dy:Y + 1 + dy, 1 + dx:X + 1 + dx], out=m)
        m = np.where(adm, m, big)
        flat, inside = m.reshape(-1), adm.reshape(-1)
        for _ in range(4):
            flat[inside] = flat[flat[inside]]
        if np.array_equal(m, lab):
            return np.where(adm, lab, -1)
        lab = m


def largest_component(adm, connectivity=6):
    """(first voxel (x, y, z) in z, y, x order, size, number of components) of the largest component; the earliest of equals"""
    lab = labels(adm, connectivity)
    ids, counts = np.unique(lab[lab >= 0], return_counts=True)
    first = int(ids[np.argmax(counts)])
    Z, Y, X = adm.shape
    return (first % X, (first // X) % Y, first // (X * Y)), int(counts.max()), len(ids)


def tiles_spanned(region):
    """the number of 64 x 16 x 16 tiles that hold a voxel of the region"""
    z, y, x = np.nonzero(region)
    return len(set(zip((x >> 6).tolist(), (y >> 4).tolist(), (z >> 4).tolist())))


def serpentine():
    """136 x 40 x 3, z = 1 only: every even row admissible along all of x, the odd rows between two even ones at one end only,
    alternating x = 135 and x = 0 (the last row, y = 39, joins nothing and stays empty): one path of 20 * 136 + 19 = 2739 voxels and
    geodesic depth 2738 from (0, 0, 1), crossing the tile faces at x = 64 and 128 in every even row and those at y = 16 and 32.
    Admissible = 100, everything else 0"""
    v = np.zeros((3, 40, 136), np.int16)
    v[1, 0::2, :] = 100
    for y in range(1, 39, 2):
        v[1, y, 135 if (y // 2) % 2 == 0 else 0] = 100
    return v


# ---- the random volumes the tests share: int16 uniform in [-1000, 1000), the seed is the first voxel of the largest component
RANDOM_DIMS = ((65, 17, 17), (70, 40, 36), (33, 40, 35), (129, 33, 18))
WINDOWS = {6: (-1000, -280), 26: (-1000, -760)}  # 36 % and 12 % admissible: just above the lattice's percolation thresholds


def random_volume(dims, seed):
    X, Y, Z = dims
    return np.random.default_rng(seed).integers(-1000, 1000, (Z, Y, X)).astype(np.int16)


@functools.lru_cache(maxsize=None)
def random_case(dims, seed, connectivity):
    """(volume, seed voxel = the first voxel of the largest component, that component, its depth, number of components)"""
    vol = random_volume(dims, seed)
    lo, hi = WINDOWS[connectivity]
    first, size, n = largest_component(admissible(vol, lo, hi), connectivity)
    region, depth = grow(vol, [first], lo, hi, connectivity)
    assert int(region.sum()) == size
    for a in (vol, region):
        a.setflags(write=False)
    return vol, first, region, depth, n
