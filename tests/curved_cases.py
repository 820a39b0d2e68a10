"""The inputs of the curved view's and the section profile's tests, chosen with the reference on the CPU (tests/test_curved_cpu.py
asserts what they reach) and run on the GPU by tests/test_gpu_curved.py.  A reference is computed once per case and shared."""
import functools
import math

import numpy as np

from cl_volume_renderer_amd import scene
from tests import costpath_ref as cp
from tests import curved_ref as cr
from tests.view_helpers import F, quiet_phantom

FRAME, REGION = (64, 48), (56, 40)
MODES = (cr.MAX, cr.MIN, cr.MEAN)
PHANTOM_DIMS = [(64, 64, 64), (70, 33, 45), (130, 20, 9), (5, 4, 3), (1, 1, 1)]
SLABS = [(1, 0.5), (7, 0.37), (64, 0.5)]
PADDING_ROW = np.array([-1, -1, -1, 0, 0, 0, 0, 0, 0], F)


def _frame(a, b):
    u = np.array([math.cos(a), math.sin(a) * math.cos(b), math.sin(a) * math.sin(b)])
    v = np.array([-math.sin(a), math.cos(a) * math.cos(b), math.cos(a) * math.sin(b)])
    return u, v, np.cross(u, v)


def twisted_rows(dims, region_wh=REGION, n=1, step=0.5):
    """float32 [h][9]: a plane about the volume's centre whose frame turns and drifts from row to row, so that the lanes of one wave
    hold different directions; then the special rows: a zero normal (3), components of du and normal that are -0 and +0 (5), a row
    far outside the volume (9), rows through the corners (0, 0, 0) and (X, Y, Z) (11, 12), a row that does not move across (14:
    du = 0) and a last tile row of padding rows"""
    X, Y, Z = dims
    w, h = region_wh
    c = np.array([X / 2, Y / 2, Z / 2])
    sp = 1.3 * max(dims) / 56
    rows = np.zeros((h, 9), np.float64)
    for y in range(h):
        u, v, nn = _frame(0.6 + 0.04 * y, 0.35 - 0.03 * y)
        drift = np.array([0.11 * (y % 5), -0.07 * (y % 3), 0.05 * (y % 7)])
        rows[y, 0:3] = c + v * sp * (y - h / 2) - u * sp * w / 2 - nn * (n - 1) * step / 2 + drift
        rows[y, 3:6] = u * sp
        rows[y, 6:9] = nn
    rows = rows.astype(F)
    rows[3, 6:9] = 0.0
    rows[5, 3], rows[5, 7] = -0.0, 0.0
    rows[9, 0:3] += F(1000.0)
    d = F(0.25 if max(dims) >= 16 else 0.125)
    rows[11] = np.array([-28 * d, -28 * d, -28 * d, d, d, d, 0.5, -0.5, 0.0], F)  # pixel 28 sits on the corner (0, 0, 0) exactly
    rows[12] = np.array([X - 28 * d, Y - 28 * d, Z - 28 * d, d, d, d, -0.5, 0.0, 0.5], F)  # ... on (X, Y, Z), which is outside
    rows[14, 3:6] = 0.0
    rows[h - 8:] = PADDING_ROW
    return rows


def _case(vol, rows, n=1, step=0.5, window=(0.0, 2000.0), frame_wh=FRAME, region_wh=REGION):
    return dict(vol=vol, rows=np.ascontiguousarray(rows, F), n=n, step=step, window=window, frame_wh=frame_wh, region_wh=region_wh)


def reference_of(case):
    """({mode: (frame, values, t_extreme)}, stats) of a case, computed once"""
    c = case
    if "_want" not in c:
        c["_want"] = cr.curved_view(c["vol"], c["rows"], c["region_wh"], modes=MODES, slab_samples=c["n"], step=c["step"], window_cw=c["window"])
    return c["_want"]


@functools.lru_cache(maxsize=None)
def twisted_cases():
    cases = []
    for dims in PHANTOM_DIMS:
        vol = scene.phantom(max(dims), dims=dims)
        for n, step in SLABS:
            cases.append(_case(vol, twisted_rows(dims, n=n, step=step), n=n, step=step))
    quiet = quiet_phantom(48)  # constant regions: ties, and whole bricks are stepped over once the slab has entered the air
    for n in (64, 200):
        cases.append(_case(quiet, twisted_rows((48, 48, 48), n=n, step=0.5), n=n, step=0.5))
    return cases


def planar_rows(origin, du, dv, normal, h):
    """the rows of clwh_render_slice's plane: row y has origin + y * dv in float32, as the slice computes it for x = 0"""
    origin, du, dv, normal = (np.asarray(v, F) for v in (origin, du, dv, normal))
    rows = np.zeros((h, 9), F)
    for y in range(h):
        rows[y, 0:3] = origin + F(y) * dv
        rows[y, 3:6] = du
        rows[y, 6:9] = normal
    return rows


@functools.lru_cache(maxsize=None)
def planar_cases():
    """planar rows through a phantom: each row is also a slice's region row 0"""
    dims = (70, 33, 45)
    vol = scene.phantom(70, dims=dims)
    w, h = REGION
    cases = []
    for n, step in SLABS:
        u, v, nn = _frame(0.6, 0.35)
        sp = 1.3 * 70 / 56
        origin = np.array(dims) / 2 - u * sp * w / 2 - v * sp * h / 2 - nn * (n - 1) * step / 2
        cases.append(_case(vol, planar_rows(origin, u * sp, v * sp, nn, h), n=n, step=step))
    return cases


# ---- the section profile's cases: masks painted station by station
SECTION_DIMS = (75, 70, 13)  # X is no multiple of 32
SECTION_SHAPES = [(64, 64), (63, 64), (64, 63), (63, 63), (1, 64), (64, 1), (1, 1)]
STATIONS = ("empty", "full", "clear centre", "two components", "touches the border", "serpentine", "partly outside", "beyond z", "centre alone")


@functools.lru_cache(maxsize=None)
def painted_mask():
    """(mask bool [13][70][75], rows float32 [9][9]): station j reads z = j, sample (x, k) the voxel (4 + x, 3 + k, j) through its
    centre -- but station 6, shifted so that part of its grid lies outside the volume, and station 7, beyond the last z"""
    X, Y, Z = SECTION_DIMS
    mask = np.zeros((Z, Y, X), bool)
    ox, oy = 4, 3
    grid = lambda z: mask[z, oy:oy + 64, ox:ox + 64]  # [k][x]
    grid(1)[:] = True
    grid(2)[:] = True
    grid(2)[24:40, 24:40] = False                      # a ring about a clear centre
    grid(3)[28:36, 28:36] = True                       # the centre's component ...
    grid(3)[5:12, 40:60] = True                        # ... and another
    grid(4)[30:34, 0:40] = True                        # a bar from the centre to the edge x = 0
    s = grid(5)                                        # a snake along x: every other line k, joined at alternating ends
    s[0::2, :] = True
    for k in range(1, 64, 2):
        s[k, 63 if (k // 2) % 2 == 0 else 0] = True
    mask[6] = True
    mask[8, oy + 31, ox + 32] = True                    # one centre sample of the 64 x 64 grid alone
    rng = np.random.default_rng(11)
    mask[9:] = rng.random((Z - 9, Y, X)) < 0.66         # (above the site percolation threshold: a large component, and debris)
    mask[10:12, 33:37, 36:40] = True                    # ... about a set centre
    rows = np.zeros((len(STATIONS) + 4, 9), F)
    for j in range(len(STATIONS)):
        rows[j] = np.array([ox + 0.5, oy + 0.5, j + 0.5, 1, 0, 0, 0, 1, 0], F)
    rows[6, 0:3] = np.array([40.5, 30.5, 6.5], F)         # x runs to 103.5: over the row's padding bits (X = 75 of 128) and beyond them
    rows[7, 2] = Z + 0.5
    for j in range(4):                                  # tilted stations through the random part, samples half a voxel apart
        u, v, _ = _frame(0.5 + 0.3 * j, 0.03 * j)
        c = np.array([X / 2, Y / 2, 11.0])
        rows[len(STATIONS) + j] = np.concatenate([c - u * 0.5 * 31.5 - v * 0.5 * 31.5, u * 0.5, v * 0.5]).astype(F)
    mask.setflags(write=False)
    return mask, rows


@functools.lru_cache(maxsize=None)
def section_reference(width, slab_samples, connected):
    """(records, depths) of the painted mask's stations"""
    mask, rows = painted_mask()
    depths = []
    return cr.section_records(mask, rows, width, slab_samples, 1.0, connected, depth_out=depths), depths


# ---- the tube of tests/costpath_ref.py: a torus of tube radius 4 about an axis circle of radius 15, a sector removed
def tube_axis_points(n=1500):
    """points exactly on the axis circle, in voxel indices (curve_frames adds the half voxel), from one end of the tube to the other"""
    theta = np.linspace(cp.TUBE_GAP, 2 * math.pi - cp.TUBE_GAP, n)
    return np.stack([cp.TUBE_CENTRE + cp.TUBE_AXIS_RADIUS * np.cos(theta), cp.TUBE_CENTRE + cp.TUBE_AXIS_RADIUS * np.sin(theta),
                     np.full(n, cp.TUBE_Z)], axis=1)
