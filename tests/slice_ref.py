"""numpy restatement of the slice contract (include/clwh.h, clwh_render_slice): parallel rays with one origin per pixel,
o = (origin + x * du) + y * dv, samples p_k = o + normal * ((float)k * step) for 0 <= k < slab_samples, kept iff inside the volume;
a sample's value is the isosurface contract's fixed-point trilinear field S (tests/isosurface_ref.py: cell, field); MAX / MIN keep
the extreme S and the first k that attains it, MEAN the int64 sum; the value is windowed to grey as the projections' is.

slice_view() is vectorised over pixels, tests every k of every pixel and always reads every kept sample: brick skipping must not
change a byte.  slice_scalar() reads the contract literally for one pixel, in Python integers."""
import numpy as np

from tests import isosurface_ref as ir
from tests import projection_ref as pr

F = np.float32
MAX, MIN, MEAN = 0, 1, 2
DENSE = 1
TWO_M24 = F(2.0 ** -24)
TWO_24 = 1 << 24


def pixel_origins(origin, du, dv, region_wh):
    """o [h * w][3] float32, row-major over the region: (origin + (float)x * du) + (float)y * dv"""
    w, h = region_wh
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    fx, fy = xs.reshape(-1, 1).astype(F), ys.reshape(-1, 1).astype(F)
    origin, du, dv = (np.asarray(v, F)[None, :] for v in (origin, du, dv))
    with np.errstate(invalid="ignore", over="ignore"):
        return (origin + fx * du) + fy * dv


def slice_view(vol, origin, du, dv, normal, region_wh, modes=(MAX,), slab_samples=1, step=0.5, window_cw=(0.0, 1.0), chunk=64):
    """({mode: (frame [h][w][4] uint8, values [h][w] float32, t_extreme [h][w] float32)}, stats) of the launched region.
    stats: the per-pixel masks "none" (no kept sample), "cut" (1 .. slab_samples - 1 kept samples; with slab_samples == 1 nothing
    is), "full" (all kept) and per extreme mode "tie"[mode] (the extreme is attained at more than one k); the sample counts
    "samples" (kept), "straddle" (the sample's cell crosses an 8^3 brick face), "clamped" (a corner was clamped at a volume face) and
    per extreme mode "skipped"[mode] (samples lying in a brick that the skip rule -- dilated bound against the running extreme --
    steps over when applied at the ray's first sample in that brick) and "skip_changed"[mode] (those among them that would have
    changed best or k_ext: the contract's proof says none)."""
    Z, Y, X = vol.shape
    w, h = region_wh
    n = int(slab_samples)
    dims = np.array([X, Y, Z], F)
    top = np.array([X - 1, Y - 1, Z - 1], np.int64)
    o = pixel_origins(origin, du, dv, region_wh)
    nrm = np.asarray(normal, F)
    npx = o.shape[0]
    dmin, dmax = ir.dilated_brick_bounds(vol)
    bound_of = {MAX: dmax * TWO_24, MIN: dmin * TWO_24}
    extreme = [m for m in (MAX, MIN)]
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
            p = o[None, :, :] + nrm[None, None, :] * t[:, None, None]
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


def slice_scalar(vol, origin, du, dv, normal, x, y, mode, slab_samples=1, step=0.5, window_cw=(0.0, 1.0)):
    """one pixel, sample by sample over every k, the field in Python integers: (pixel [4] uint8, value float32, t_extreme float32)"""
    Z, Y, X = vol.shape
    dims = (X, Y, Z)
    origin, du, dv, nrm = (np.asarray(v, F) for v in (origin, du, dv, normal))
    with np.errstate(invalid="ignore", over="ignore"):
        o = [(origin[c] + F(x) * du[c]) + F(y) * dv[c] for c in range(3)]
        best, k_best, total, count = None, None, 0, 0
        for k in range(int(slab_samples)):
            t = F(k) * F(step)
            p = [o[c] + nrm[c] * t for c in range(3)]
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
