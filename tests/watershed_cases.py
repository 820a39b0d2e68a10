"""The inputs the CPU and the GPU tests of clwh_watershed share, all small, and their expected outputs from tests/watershed_ref.py,
computed once per (case, connectivity) and read only.  The tile is 16 x 16 x 8: the shapes are the smallest at which a face, an edge
or a corner between tiles, a ragged last tile or a mask word boundary is crossed."""
import functools

import numpy as np

from tests import watershed_ref as w

SHAPES = ((16, 16, 8), (17, 17, 9), (37, 35, 19), (65, 3, 2), (1, 1, 1), (5, 1, 1))  # X, Y, Z
RIDGE_WALL_X, RIDGE_DIMS = 5, (48, 5, 3)
RIDGE_SEEDS = [(RIDGE_WALL_X - 3, 2, 1, 1), (RIDGE_WALL_X + 40, 2, 1, 2)]


def low_cost(dims, seed=11):
    """uint16 [z][y][x] uniform in 0 .. 4: walls, many ties and plateaus"""
    X, Y, Z = dims
    return np.random.default_rng(seed + X).integers(0, 5, (Z, Y, X)).astype(np.uint16)


def full_cost(dims, seed=13):
    """uniform in 0 .. 65535, with both ends of the range present"""
    X, Y, Z = dims
    c = np.random.default_rng(seed).integers(0, 65536, (Z, Y, X)).astype(np.uint16)
    c.reshape(-1)[:2] = (65535, 1)
    return c


def scattered_seeds(D, seed=5, n=5):
    """3 .. 6 labelled seeds inside D whose ids are not in spatial order, the first listed again with a larger id and the last with a
    smaller one (two ids on one voxel), and, if there is one, a voxel outside D (a wall, or outside the domain) with id 1"""
    rng = np.random.default_rng(seed)
    inside, outside = np.argwhere(D), np.argwhere(~D)
    pick = inside[rng.choice(len(inside), min(n, len(inside)), replace=False)] if len(inside) else []
    ids = [9, 4, 30, 6, 17, 12]
    rows = [(int(x), int(y), int(z), ids[k]) for k, (z, y, x) in enumerate(pick)]
    if rows:
        rows += [rows[0][:3] + (40,), rows[-1][:3] + (2,)]
    if len(outside):
        z, y, x = outside[rng.integers(len(outside))]
        rows.append((int(x), int(y), int(z), 1))
    if not rows:
        rows = [(0, 0, 0, 1)]
    return rows


def ridge():
    """two flat basins of cost 1 separated by the one-voxel wall x = RIDGE_WALL_X of cost 20; seed 1 is 3 voxels from the wall, seed 2
    is 40 voxels from it on the other side"""
    X, Y, Z = RIDGE_DIMS
    c = np.ones((Z, Y, X), np.uint16)
    c[:, :, RIDGE_WALL_X] = 20
    return c


def corridor():
    """33 x 33 x 9: a corridor of cost 3, one voxel wide, in the plane z = 4 along the rows y = 0, 2, .., 32 joined at alternating ends,
    walls around it: 33 tile faces from the seed at its start, so more than eight rounds in each phase"""
    c = np.zeros((9, 33, 33), np.uint16)
    for y in range(0, 33, 2):
        c[4, y, :] = 3
        if y + 2 < 33:
            c[4, y + 1, 32 if (y // 2) % 2 == 0 else 0] = 3
    return c


def _case(name, cost, seeds=None, domain=None, seed_labels=None, plateau_cap=w.PLATEAU_MAX, level_cap=w.LEVEL_MAX, in_place=False,
          low=False):
    return dict(name=name, cost=cost, seeds=seeds, domain=domain, seed_labels=seed_labels, plateau_cap=plateau_cap, level_cap=level_cap,
                in_place=in_place, low=low)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for dims in SHAPES:
        c = low_cost(dims)
        out.append(_case("low-%dx%dx%d" % dims, c, scattered_seeds(w.in_domain(c)), low=True))
    c = low_cost((17, 17, 9))
    for cap in (0, 3):
        out.append(_case("low-17x17x9-plateau%d" % cap, c, scattered_seeds(w.in_domain(c)), plateau_cap=cap, low=True))
    c = full_cost((17, 17, 9))
    out.append(_case("full-17x17x9", c, scattered_seeds(w.in_domain(c))))
    out.append(_case("full-17x17x9-levelcap", c, scattered_seeds(w.in_domain(c)), level_cap=30000))
    c = np.full((9, 17, 17), 7, np.uint16)
    for cap in (0, 3, w.PLATEAU_MAX):  # a plateau longer than 3
        out.append(_case("constant-plateau%d" % cap, c, [(2, 3, 1, 5), (14, 12, 7, 2), (15, 1, 8, 8)], plateau_cap=cap))
    out.append(_case("ridge", ridge(), RIDGE_SEEDS))
    out.append(_case("ridge-levelcap", ridge(), RIDGE_SEEDS[:1], level_cap=19))  # nothing behind the wall is reached
    out.append(_case("corridor", corridor(), [(0, 0, 4, 3)]))
    # a domain in a shape whose mask row is longer than one 64-bit word; the GPU test sets the padding bits
    c = low_cost((65, 3, 2), 17) + np.uint16(1)
    dom = np.random.default_rng(9).random(c.shape) < 0.85
    out.append(_case("domain-65x3x2", c, scattered_seeds(w.in_domain(c, dom)), domain=dom))
    c = low_cost((37, 35, 19), 19)
    dom = np.random.default_rng(10).random(c.shape) < 0.9
    out.append(_case("domain-37x35x19", c, scattered_seeds(w.in_domain(c, dom)), domain=dom, low=True))
    # seeds from a label map, alone and with a list beside it; separate and in place
    c = low_cost((17, 17, 9), 23)
    sl = np.zeros(c.shape, np.uint32)
    sl[np.random.default_rng(3).random(c.shape) < 0.01] = 7
    sl[0, 0, :3] = (0xFFFFFFFF, 3, 1)
    out.append(_case("from-labels", c, None, seed_labels=sl))
    out.append(_case("from-labels-in-place", c, [(16, 16, 8, 2)], seed_labels=sl, in_place=True))
    for k in out:
        for a in (k["cost"], k["domain"], k["seed_labels"]):
            if a is not None:
                a.setflags(write=False)
    return tuple(out)


def case(name):
    return next(k for k in cases() if k["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(name, connectivity):
    """(labels, level) of the reference, read only"""
    k = case(name)
    labels, level = w.watershed(k["cost"], k["seeds"], connectivity, k["plateau_cap"], k["level_cap"], k["seed_labels"], k["domain"])
    labels.setflags(write=False)
    level.setflags(write=False)
    return labels, level


NAMES = tuple(k["name"] for k in cases())
