"""numpy restatement of the curved reformat and the section profile (include/clwh.h, clwh_render_curved and clwh_curve_profile) and
of the curve's frames (scene.curve_frames).

curved_view() is tests/slice_ref.py's slice_view with a frame per image row: pixel (x, y) owns the ray o = origin_y + (float)x * du_y
along normal_y; it tests every k of every pixel and always reads every kept sample.  curved_scalar() reads the contract literally for
one pixel, in Python integers.  section_records() finds a station's section by a plain breadth-first search.
curve_frames_literal() is the frames' definition written out point by point in Python floats."""
import math
from collections import deque

import numpy as np

from tests import isosurface_ref as ir
from tests import projection_ref as pr
from tests import slice_ref as sr

F = np.float32
MAX, MIN, MEAN = sr.MAX, sr.MIN, sr.MEAN
DENSE = 1
CONNECTED = 1
TWO_M24, TWO_24 = sr.TWO_M24, sr.TWO_24
RECORD = np.dtype([("count", np.uint32), ("sum_x", np.uint32), ("sum_k", np.uint32), ("border", np.uint32)])


def pixel_rays(rows, region_wh):
    """(o [h * w][3], normal [h * w][3]) float32, row-major over the region: o = origin_y + (float)x * du_y"""
    w, h = region_wh
    rows = np.asarray(rows, F).reshape(-1, 9)[:h]
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    fx, y = xs.reshape(-1, 1).astype(F), ys.reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        return rows[y, 0:3] + fx * rows[y, 3:6], rows[y, 6:9]


def curved_view(vol, rows, region_wh, modes=(MAX,), slab_samples=1, step=0.5, window_cw=(0.0, 1.0), chunk=64):
    """({mode: (frame [h][w][4] uint8, values [h][w] float32, t_extreme [h][w] float32)}, stats) of the launched region: slice_view's
    outputs and its stats dictionary (none, cut, full, tie, samples, straddle, clamped, skipped, skip_changed)"""
    Z, Y, X = vol.shape
    w, h = region_wh
    n = int(slab_samples)
    dims = np.array([X, Y, Z], F)
    top = np.array([X - 1, Y - 1, Z - 1], np.int64)
    o, nrm = pixel_rays(rows, region_wh)
    npx = o.shape[0]
    dmin, dmax = ir.dilated_brick_bounds(vol)
    bound_of = {MAX: dmax * TWO_24, MIN: dmin * TWO_24}
    extreme = [MAX, MIN]
    best = {m: np.zeros(npx, np.int64) for m in extreme}
    k_ext = {m: np.zeros(npx, np.int64) for m in extreme}
    n_at = {m: np.zeros(npx, np.int64) for m in extreme}
    skipping = {m: np.zeros(npx, bool) for m in extreme}
    skipped = {m: 0 for m in extreme}
    skip_changed = {m: 0 for m in extreme}
    total = np.zeros(npx, np.int64)
    count = np.zeros(npx, np.int64)
    cur_brick = np.full((npx, 3), -1, np.int64)
    straddle = clamped = 0
    for k0 in range(0, n, chunk):
        ks = np.arange(k0, min(k0 + chunk, n), dtype=np.int64)
        t = ks.astype(F) * F(step)
        with np.errstate(invalid="ignore", over="ignore"):
            p = o[None, :, :] + nrm[None, :, :] * t[:, None, None]
            kept = np.all((p >= 0) & (p < dims), axis=2)  # (false for NaN)
        kk, ii = np.nonzero(kept)  # row-major: sorted by k
        if not kk.size:
            continue
        pk = p[kk, ii]
        i0, wt = ir.cell(pk)
        S = ir.field(vol, i0, wt)
        clamped += int(((i0 < 0) | (i0 >= top)).any(axis=1).sum())
        straddle += int(((i0 >= 0) & (i0 < top) & ((i0 & 7) == 7)).any(axis=1).sum())
        b = pk.astype(np.int64) >> 3  # kept: 0 <= p < dim, truncation is floor
        edges = np.searchsorted(kk, np.arange(ks.size + 1))
        for j in range(ks.size):
            lo, hi = edges[j], edges[j + 1]
            if lo == hi:
                continue
            idx, Sj, bj = ii[lo:hi], S[lo:hi], b[lo:hi]
            new = (bj != cur_brick[idx]).any(axis=1)  # the ray's first sample in this brick
            cur_brick[idx] = bj
            have = count[idx] > 0
            for m in extreme:
                bound = bound_of[m][bj[:, 2], bj[:, 1], bj[:, 0]]
                rule = have & (bound <= best[m][idx] if m == MAX else bound >= best[m][idx])
                sk = np.where(new, rule, skipping[m][idx])
                skipping[m][idx] = sk
                better = ~have | (Sj > best[m][idx] if m == MAX else Sj < best[m][idx])
                skipped[m] += int(sk.sum())
                skip_changed[m] += int((sk & better).sum())
                n_at[m][idx] = np.where(better, 1, n_at[m][idx] + (have & (Sj == best[m][idx])))
                best[m][idx] = np.where(better, Sj, best[m][idx])
                k_ext[m][idx] = np.where(better, ks[j], k_ext[m][idx])
            total[idx] += Sj
            count[idx] += 1
    some = count > 0
    out = {}
    for m in modes:
        if m == MEAN:
            with np.errstate(invalid="ignore", divide="ignore"):
                values = np.where(some, (total.astype(np.float64) / (count.astype(np.float64) * 16777216.0)).astype(F), F(np.nan)).astype(F)
            t_ext = np.full(npx, np.nan, F)
        else:
            values = np.where(some, best[m].astype(np.float64).astype(F) * TWO_M24, F(np.nan)).astype(F)
            t_ext = np.where(some, k_ext[m].astype(F) * F(step), F(np.nan)).astype(F)
        values, t_ext = values.reshape(h, w), t_ext.reshape(h, w)
        out[m] = (pr.window(values, *window_cw), values, t_ext)
    stats = {"none": ~some.reshape(h, w), "cut": (some & (count < n)).reshape(h, w), "full": (count == n).reshape(h, w),
             "tie": {m: (some & (n_at[m] > 1)).reshape(h, w) for m in extreme}, "samples": int(count.sum()), "straddle": straddle,
             "clamped": clamped, "skipped": skipped, "skip_changed": skip_changed}
    return out, stats


def sample_position(row, x, k, step):
    """p(x, k) of a row, literally: three float32 values"""
    row = np.asarray(row, F)
    with np.errstate(invalid="ignore", over="ignore"):
        t = F(k) * F(step)
        return [(row[c] + F(x) * row[3 + c]) + row[6 + c] * t for c in range(3)]


def curved_scalar(vol, rows, x, y, mode, slab_samples=1, step=0.5, window_cw=(0.0, 1.0)):
    """one pixel, sample by sample over every k, the field in Python integers: (pixel [4] uint8, value float32, t_extreme float32)"""
    Z, Y, X = vol.shape
    dims = (X, Y, Z)
    row = np.asarray(rows, F).reshape(-1, 9)[y]
    best, k_best, total, count = None, None, 0, 0
    for k in range(int(slab_samples)):
        p = sample_position(row, x, k, step)
        if not all(p[c] >= 0 and p[c] < F(dims[c]) for c in range(3)):
            continue
        S = 0
        i0, wt = [], []
        for c in range(3):
            q = p[c] - F(0.5)
            f = np.floor(q)
            i0.append(int(f))
            wt.append(min(int((q - f) * F(256.0)), 255))
        for bz in (0, 1):
            for by in (0, 1):
                for bx in (0, 1):
                    weight = (wt[0] if bx else 256 - wt[0]) * (wt[1] if by else 256 - wt[1]) * (wt[2] if bz else 256 - wt[2])
                    cx, cy, cz = (min(max(i0[c] + bit, 0), dims[c] - 1) for c, bit in enumerate((bx, by, bz)))
                    S += weight * int(vol[cz, cy, cx])
        total, count = total + S, count + 1
        if best is None or (S > best if mode == MAX else S < best):
            best, k_best = S, k
    if count == 0:
        return np.zeros(4, np.uint8), F(np.nan), F(np.nan)
    if mode == MEAN:
        value, t_ext = F(np.float64(total) / (np.float64(count) * 16777216.0)), F(np.nan)
    else:
        value, t_ext = F(np.float64(best)) * TWO_M24, F(k_best) * F(step)
    return pr.window(np.array([value], F), *window_cw)[0], value, t_ext


def set_samples(mask, rows, width, slab_samples, step):
    """bool [n_rows][slab_samples][width]: sample (x, k) of a station is kept and its voxel's bit is set"""
    Z, Y, X = mask.shape
    rows = np.asarray(rows, F).reshape(-1, 9)
    dims = np.array([X, Y, Z], F)
    fx = np.arange(width).astype(F)[None, None, :, None]
    t = (np.arange(slab_samples).astype(F) * F(step))[None, :, None, None]
    with np.errstate(invalid="ignore", over="ignore"):
        o = rows[:, None, None, 0:3] + fx * rows[:, None, None, 3:6]
        p = o + rows[:, None, None, 6:9] * t
        kept = np.all((p >= 0) & (p < dims), axis=3)
    v = np.where(kept[..., None], p, 0).astype(np.int64)
    return kept & mask[v[..., 2], v[..., 1], v[..., 0]]


def section_records(mask, rows, width, slab_samples, step, connected, depth_out=None):
    """the records (RECORD) of clwh_curve_profile for a bool mask [z][y][x], by breadth-first search from the centre samples;
    depth_out (a list) receives per station the search's depth: the steps to the section's sample farthest from the centre"""
    S = set_samples(mask, rows, width, slab_samples, step)
    out = np.zeros(S.shape[0], RECORD)
    for y in range(S.shape[0]):
        s = S[y]
        deepest = 0
        if connected:
            sec = np.zeros_like(s)
            queue = deque((k, x, 0) for k in sorted({(slab_samples - 1) // 2, slab_samples // 2})
                          for x in sorted({(width - 1) // 2, width // 2}) if s[k, x])
            for k, x, _ in queue:
                sec[k, x] = True
            while queue:
                k, x, deepest = queue.popleft()
                for kk, xx in ((k - 1, x), (k + 1, x), (k, x - 1), (k, x + 1)):
                    if 0 <= kk < slab_samples and 0 <= xx < width and s[kk, xx] and not sec[kk, xx]:
                        sec[kk, xx] = True
                        queue.append((kk, xx, deepest + 1))
        else:
            sec = s
        ks, xs = np.nonzero(sec)
        edge = (xs == 0) | (xs == width - 1) | (ks == 0) | (ks == slab_samples - 1)
        out[y] = (len(ks), int(xs.sum()), int(ks.sum()), int(edge.sum()))
        if depth_out is not None:
            depth_out.append(deepest)
    return out


# ---- the curve's frames, point by point in Python floats (scene.curve_frames' steps 1 to 9)
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _unit(v):
    n = math.sqrt(_dot(v, v))
    return [v[0] / n, v[1] / n, v[2] / n]


def curve_frames_literal(points, spacing, width, pixel_mm, station_mm, smooth_passes=8, angle=0.0, slab_samples=1, step_mm=None, parts=None):
    """(rows float32 [H][9], s_mm, n); parts (a dictionary) receives the binary64 C, T, U per station"""
    step_mm = pixel_mm if step_mm is None else step_mm
    sp = [float(v) for v in spacing]
    q = [[(float(p[c]) + 0.5) * sp[c] for c in range(3)] for p in points]
    m = len(q)
    for _ in range(smooth_passes):
        q = [q[0]] + [[((q[i - 1][c] + 2.0 * q[i][c]) + q[i + 1][c]) / 4.0 for c in range(3)] for i in range(1, m - 1)] + [q[-1]]
    L = [0.0]
    for i in range(m - 1):
        d = [q[i + 1][c] - q[i][c] for c in range(3)]
        L.append(L[i] + math.sqrt(_dot(d, d)))
    n = int(math.floor(L[-1] / station_mm)) + 1
    s_mm = [j * station_mm for j in range(n)]
    Cs = []
    for s in s_mm:
        i = 0
        while i < m - 2 and L[i + 1] <= s:
            i += 1
        span = L[i + 1] - L[i]
        f = (s - L[i]) / span if span > 0.0 else 0.0
        Cs.append([q[i][c] + f * (q[i + 1][c] - q[i][c]) for c in range(3)])
    Ts = []
    for j in range(n):
        a, b = Cs[min(j + 1, n - 1)], Cs[max(j - 1, 0)]
        Ts.append(_unit([a[c] - b[c] for c in range(3)]))
    axis = 0
    for c in (1, 2):
        if abs(Ts[0][c]) < abs(Ts[0][axis]):
            axis = c
    e = [1.0 if c == axis else 0.0 for c in range(3)]
    d0 = _dot(e, Ts[0])
    Us = [_unit([e[c] - d0 * Ts[0][c] for c in range(3)])]
    for j in range(n - 1):
        U, T, T1 = Us[j], Ts[j], Ts[j + 1]
        v1 = [Cs[j + 1][c] - Cs[j][c] for c in range(3)]
        c1 = _dot(v1, v1)
        ku, kt = (2.0 / c1) * _dot(v1, U), (2.0 / c1) * _dot(v1, T)
        rL = [U[c] - ku * v1[c] for c in range(3)]
        tL = [T[c] - kt * v1[c] for c in range(3)]
        v2 = [T1[c] - tL[c] for c in range(3)]
        c2 = _dot(v2, v2)
        if c2 == 0.0:
            r = rL
        else:
            k2 = (2.0 / c2) * _dot(v2, rL)
            r = [rL[c] - k2 * v2[c] for c in range(3)]
        dr = _dot(r, T1)
        Us.append(_unit([r[c] - dr * T1[c] for c in range(3)]))
    co, si = math.cos(angle), math.sin(angle)
    hw, hk = (width - 1) / 2.0, ((slab_samples - 1) / 2.0) * step_mm
    H = (n + 7) // 8 * 8
    rows = np.zeros((H, 9), F)
    rows[n:, :3] = -1.0
    for j in range(n):
        T, U = Ts[j], Us[j]
        W = [T[1] * U[2] - T[2] * U[1], T[2] * U[0] - T[0] * U[2], T[0] * U[1] - T[1] * U[0]]
        A = [co * U[c] + si * W[c] for c in range(3)]
        N = [(-si) * U[c] + co * W[c] for c in range(3)]
        du = [(A[c] * pixel_mm) / sp[c] for c in range(3)]
        nrm = [N[c] / sp[c] for c in range(3)]
        origin = [(Cs[j][c] / sp[c] - hw * du[c]) - hk * nrm[c] for c in range(3)]
        rows[j] = np.array(origin + du + nrm, np.float64).astype(F)
    if parts is not None:
        parts.update(C=np.array(Cs), T=np.array(Ts), U=np.array(Us))
    return rows, np.array(s_mm, np.float64), n
