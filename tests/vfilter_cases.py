"""The cases the volume filter's CPU and GPU tests share: shapes at which the kernels can still go wrong, value fields, and the
parameters of every kind; the references are computed once (tests/vfilter_ref.py) and kept."""
import functools

import numpy as np

from cl_volume_renderer_amd import scene
from tests import vfilter_ref as vr

# X not a multiple of the 8 or 64 the tiles use; the degenerate ones; a radius larger than two of the dims; more than one 64- and
# one 128-voxel unit in x with an odd row length
SHAPES = {"main": (70, 19, 21), "one": (1, 1, 1), "flat": (2, 3, 1), "thin": (5, 40, 3), "wide": (129, 9, 17)}
FIELDS = ("random", "ball", "extremes", "constant", "ties")
MAIN = ("main", "random")


@functools.lru_cache(maxsize=None)
def field(shape, name):
    """int16 [z][y][x]"""
    X, Y, Z = SHAPES[shape]
    rng = np.random.default_rng(sum(map(ord, shape + name)))
    if name == "random":  # the full range
        return rng.integers(-32768, 32768, (Z, Y, X)).astype(np.int16)
    if name == "ball":  # a noisy phantom: -1000 outside, 300 inside, +-40
        z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
        inside = ((x - X / 2) / (0.35 * X + 1)) ** 2 + ((y - Y / 2) / (0.35 * Y + 1)) ** 2 + ((z - Z / 2) / (0.35 * Z + 1)) ** 2 < 1.0
        return (np.where(inside, 300, -1000) + rng.integers(-40, 41, (Z, Y, X))).astype(np.int16)
    if name == "extremes":  # only -32768 and 32767: packed minima that saturate or sums that overflow show here
        return np.where(rng.random((Z, Y, X)) < 0.5, -32768, 32767).astype(np.int16)
    if name == "constant":
        return np.full((Z, Y, X), -32768 if X % 2 else 32767, np.int16)
    if name == "ties":  # long runs of equal values along x, three levels
        return np.repeat(rng.integers(-1, 2, (Z, Y, (X + 6) // 7)), 7, axis=2)[:, :, :X].astype(np.int16) * 1000
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def mask_of(shape):
    """(bool [z][y][x] random bits, its words with every padding bit and word set)"""
    X, Y, Z = SHAPES[shape]
    m = np.random.default_rng(X * 31 + Y).random((Z, Y, X)) < 0.5
    wpr = scene.mask_words_per_row(X)
    padded = np.ones((Z, Y, wpr * 32), np.uint8)
    padded[:, :, :X] = m
    return m, np.packbits(padded, axis=2, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def outer_tap(r):
    """all of the weight on the outermost taps: pins the clamped indexing"""
    return np.array([0] * r + [2048], np.uint16) if r else np.array([4096], np.uint16)


def _params():
    out = []
    for radius in ((1, 1, 1), (1, 1, 0), (0, 1, 1), (1, 0, 0), (0, 0, 0)):
        out.append(("median %d%d%d" % radius, vr.MEDIAN, radius, None))
    for kind, name in ((vr.MIN, "min"), (vr.MAX, "max")):
        # (the last two: every radius at which the y and z passes change their ring, 4 | 5 and 12 | 13)
        for radius in ((1, 1, 1), (3, 0, 2), (16, 16, 16), (4, 5, 12), (13, 12, 5)):
            out.append(("%s %d %d %d" % ((name,) + radius), kind, radius, None))
    smooths = {
        "gauss 1 1 0.6": scene.gaussian_weights((1.0, 1.0, 0.6)),
        "gauss 5.4": scene.gaussian_weights(5.4),
        "outer 16 3 1": [outer_tap(16), outer_tap(3), outer_tap(1)],
        "outer 0 16 16": [outer_tap(0), outer_tap(16), outer_tap(16)],
        "binomial 4 5 6": [scene.binomial_weights(p) for p in (4, 5, 6)],
        "outer 5 13 12": [outer_tap(5), outer_tap(13), outer_tap(12)],
        "identity": [outer_tap(0)] * 3,
    }
    for name, w in smooths.items():
        out.append(("smooth " + name, vr.SMOOTH, tuple(len(v) - 1 for v in w), w))
    return out


PARAMS = _params()
PARAM = {p[0]: p for p in PARAMS}


@functools.lru_cache(maxsize=None)
def reference(shape, field_name, label):
    """F of the whole volume (without a mask), read only"""
    _, kind, radius, weights = PARAM[label]
    out = vr.filtered(field(shape, field_name), kind, radius, weights)
    out.setflags(write=False)
    return out
