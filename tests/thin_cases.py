"""The cases of tests/test_gpu_thin.py, shared with the CPU test of their non-vacuity (tests/test_thin_cpu.py): the smallest shapes at
which the kernels can still go wrong.  A tile is 64 x 16 x 16 voxels and a row's word 64 voxels, so the shapes cross x = 64 (and 128),
y = 16 and z = 16, and the structures run through the corner (64, 16, 16) where eight tiles meet.  Every case has a mask and an
anchor image; the references are computed once per (case, keep_ends, anchored) and shared."""
import functools

import numpy as np

from tests import thin_ref as tr
from tests.grow_ref import RANDOM_DIMS

MAX_ITERATIONS = (0, 1, 2)


def _noise(dims, density, seed):
    X, Y, Z = dims
    return np.random.default_rng(seed).random((Z, Y, X)) < density


def _grid(dims):
    X, Y, Z = dims
    return np.mgrid[:Z, :Y, :X]


def _tube(dims, axis, centre, radius):
    """a tube along `axis` (0 = x) through the whole volume, its axis at `centre` in the two other coordinates"""
    z, y, x = _grid(dims)
    c = [x, y, z]
    others = [q for q in range(3) if q != axis]
    return (c[others[0]] - centre[0]) ** 2 + (c[others[1]] - centre[1]) ** 2 <= radius ** 2


def _torus(dims, centre, R, r):
    z, y, x = _grid(dims)
    return (np.hypot(x - centre[0], y - centre[1]) - R) ** 2 + (z - centre[2]) ** 2 <= r ** 2


def _bars(dims, centre, half, thick):
    """three bars of `thick`^2 voxels across, 2 * half long, crossed at `centre`"""
    X, Y, Z = dims
    m = np.zeros((Z, Y, X), bool)
    cx, cy, cz = centre
    a, b = thick // 2, thick - thick // 2
    m[cz - a:cz + b, cy - a:cy + b, cx - half:cx + half] = True
    m[cz - a:cz + b, cy - half:cy + half, cx - a:cx + b] = True
    m[cz - half:cz + half, cy - a:cy + b, cx - a:cx + b] = True
    return m


def _hollow_box(dims, lo, hi, wall):
    X, Y, Z = dims
    m = np.zeros((Z, Y, X), bool)
    m[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
    m[lo[2] + wall:hi[2] - wall, lo[1] + wall:hi[1] - wall, lo[0] + wall:hi[0] - wall] = False
    return m


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (mask, anchors)}, bool [z][y][x] each, anchors a sparse subset of the mask"""
    out = {}
    for k, (dims, density) in enumerate(zip(RANDOM_DIMS, (0.5, 0.2, 0.8, 0.5))):
        out["noise %d x %d x %d at %.1f" % (dims + (density,))] = _noise(dims, density, 100 + k)
    for k, density in enumerate((0.2, 0.5, 0.8)):
        out["noise 130 x 17 x 17 at %.1f" % density] = _noise((130, 17, 17), density, 110 + k)
        out["noise 65 x 33 x 18 at %.1f" % density] = _noise((65, 33, 18), density, 120 + k)
    for dims in ((64, 16, 16), (130, 17, 17), (3, 3, 3), (1, 1, 1), (63, 1, 1), (64, 1, 1), (65, 1, 1)):
        out["solid %d x %d x %d" % dims] = np.ones(dims[::-1], bool)
    out["tube along x"] = _tube((130, 34, 34), 0, (16, 16), 2.6)
    out["tube along y"] = _tube((80, 40, 34), 1, (64, 16), 2.6)
    out["tube along z"] = _tube((80, 34, 40), 2, (64, 16), 2.6)
    out["torus"] = _torus((80, 32, 32), (63.5, 15.5, 15.5), 7.0, 2.6)
    out["bars"] = _bars((80, 32, 32), (64, 16, 16), 13, 4)
    out["hollow box"] = _hollow_box((72, 33, 20), (58, 10, 3), (70, 24, 19), 2)
    rng = np.random.default_rng(7)
    return {name: (m, m & (rng.random(m.shape) < 0.03)) for name, m in out.items()}


def garbage(mask):
    """the mask's words with every bit at x >= X and every padding word set (tests/test_gpu_distance.py's)"""
    from cl_volume_renderer_amd import scene

    Z, Y, X = mask.shape
    wpr = scene.mask_words_per_row(X)
    padded = np.ones((Z, Y, wpr * 32), np.uint8)
    padded[:, :, :X] = mask
    return np.packbits(padded, axis=2, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def dims_of(mask):
    Z, Y, X = mask.shape
    return X, Y, Z


@functools.lru_cache(maxsize=None)
def reference(name, keep_ends, anchored):
    """{max_iterations: (mask, result dict)} for MAX_ITERATIONS, from one run of the reference"""
    mask, anchors = cases()[name]
    final, result, kept = tr.thin(mask, tr.KEEP_ENDS if keep_ends else 0, anchors if anchored else None, 0, (1, 2))
    kept[0] = (final, result)  # (a run limited to k iterations is the unlimited run after k, or its end if that comes first)
    return kept
