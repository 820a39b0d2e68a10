"""clwh_volume_filter's contract (include/clwh.h) restated in numpy, literally: every tap a gather at the clamped coordinate, the median
a sort of the gathered taps, the sums in int64.  Volumes are int16 [z][y][x]; radius = (rx, ry, rz); masks are bool [z][y][x]."""
import numpy as np

MEDIAN, MIN, MAX, SMOOTH = 0, 1, 2, 3


def tap(vol, dx, dy, dz, border="clamp"):
    """V(clamp(x + dx), clamp(y + dy), clamp(z + dz)) for every voxel; border="zero": 0 outside the volume (NOT the contract)"""
    Z, Y, X = vol.shape
    z, y, x = np.arange(Z) + dz, np.arange(Y) + dy, np.arange(X) + dx
    got = vol[np.clip(z, 0, Z - 1)[:, None, None], np.clip(y, 0, Y - 1)[None, :, None], np.clip(x, 0, X - 1)[None, None, :]]
    if border == "zero":
        inside = ((z >= 0) & (z < Z))[:, None, None] & ((y >= 0) & (y < Y))[None, :, None] & ((x >= 0) & (x < X))[None, None, :]
        got = np.where(inside, got, 0)
    return got


def taps(vol, radius, border="clamp"):
    """all taps of the box, [n][z][y][x]"""
    rx, ry, rz = radius
    return np.stack([tap(vol, dx, dy, dz, border) for dz in range(-rz, rz + 1) for dy in range(-ry, ry + 1) for dx in range(-rx, rx + 1)])


def median(vol, radius, border="clamp"):
    assert all(r in (0, 1) for r in radius)
    t = np.sort(taps(vol, radius, border), axis=0)
    return t[(len(t) - 1) // 2].astype(np.int16)


def extreme(vol, radius, kind, border="clamp"):
    """the minimum / maximum over the box, tap by tap"""
    assert all(0 <= r <= 16 for r in radius)
    rx, ry, rz = radius
    pick = np.minimum if kind == MIN else np.maximum
    out = None
    for dz in range(-rz, rz + 1):
        for dy in range(-ry, ry + 1):
            for dx in range(-rx, rx + 1):
                t = tap(vol, dx, dy, dz, border)
                out = t if out is None else pick(out, t)
    return out.astype(np.int16)


def extreme_by_axes(vol, radius, kind):
    """the same set function axis by axis (a minimum of minima): what the large boxes on the large cases are checked against, itself
    checked against extreme() on the small ones (tests/test_vfilter_cpu.py)"""
    out = vol
    for axis in range(3):
        r = [0, 0, 0]
        r[axis] = radius[axis]
        out = extreme(out, r, kind)
    return out


def smooth_pass(vol, axis, w):
    """one pass along axis 0 = x, 1 = y, 2 = z: (sum_k w[|k|] S(clamp(p + k e)) + 2048) >> 12 in int64, back to int16"""
    w = [int(v) for v in w]
    r = len(w) - 1
    assert 0 <= r <= 16 and w[0] + 2 * sum(w[1:]) == 4096
    acc = np.zeros(vol.shape, np.int64)
    for k in range(-r, r + 1):
        off = [0, 0, 0]
        off[axis] = k
        acc += w[abs(k)] * tap(vol, *off).astype(np.int64)
    out = (acc + 2048) >> 12  # numpy's >> on signed integers is arithmetic
    assert out.min() >= -32768 and out.max() <= 32767
    return out.astype(np.int16)


def smooth(vol, weights, order=(0, 1, 2)):
    out = vol
    for axis in order:
        out = smooth_pass(out, axis, weights[axis])
    return out


def smooth_single_rounding(vol, weights):
    """NOT the contract: the three passes in exact integers and one rounding at the end, (sum + 2^35) >> 36"""
    acc = vol.astype(np.int64)
    for axis in (0, 1, 2):
        w = [int(v) for v in weights[axis]]
        r = len(w) - 1
        nxt = np.zeros_like(acc)
        for k in range(-r, r + 1):
            off = [0, 0, 0]
            off[axis] = k
            nxt += w[abs(k)] * tap(acc, *off)
        acc = nxt
    return ((acc + (1 << 35)) >> 36).astype(np.int16)


def filtered(vol, kind, radius=None, weights=None, mask=None):
    """the call: F where the mask is None or set, V elsewhere"""
    if kind == MEDIAN:
        f = median(vol, radius)
    elif kind in (MIN, MAX):
        n_taps = (2 * radius[0] + 1) * (2 * radius[1] + 1) * (2 * radius[2] + 1)
        f = extreme(vol, radius, kind) if n_taps <= 1000 else extreme_by_axes(vol, radius, kind)  # (a gather per tap: 35 937 at radius 16)
    else:
        f = smooth(vol, weights)
    return f if mask is None else np.where(mask, f, vol).astype(np.int16)
